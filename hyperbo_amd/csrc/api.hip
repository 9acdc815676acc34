// C ABI of libhbo (see include/hbo.h), the part that belongs to no topic of its own: the context, the options, the profile getters
// and the gradient layout.  (Datasets: dataset.hip; dense entry points on host arrays: dense.hip; test and measurement hooks: probe.hip.)
#include "api_internal.h"

thread_local std::string hbo_g_err;

// ---- context -----------------------------------------------------------------------------
extern "C" const char* hbo_version(void) { return "hbo 0.1 (gfx950)"; }
extern "C" int hbo_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
extern "C" int hbo_device_info(int device, char* name_out, int32_t cap, int32_t* cus, int64_t* mem_bytes) {
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, device) != hipSuccess) {
    (void)hipGetLastError();   // (not sticky: a later HIPCHK(hipGetLastError()) of this thread must not trip over it)
    return fail(nullptr, HBO_ERR_NODEV, "hbo_device_info: no such device");
  }
  if (name_out && cap > 0) { snprintf(name_out, (size_t)cap, "%s (%s)", p.name, p.gcnArchName); }
  if (cus) *cus = p.multiProcessorCount;
  if (mem_bytes) *mem_bytes = (int64_t)p.totalGlobalMem;
  return HBO_OK;
}
extern "C" const char* hbo_last_error(hbo_ctx* ctx) { return ctx ? ctx->err.c_str() : hbo_g_err.c_str(); }

extern "C" int hbo_ctx_create(int device, hbo_ctx** out) {
  if (!out) return fail(nullptr, HBO_ERR_ARG, "hbo_ctx_create: out is null");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(nullptr, HBO_ERR_NODEV, "hbo_ctx_create: no HIP device visible");
  if (device < 0 || device >= n) return fail(nullptr, HBO_ERR_ARG, "hbo_ctx_create: bad device index");
  hbo_ctx* c = new hbo_ctx();
  c->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreate(&c->stream);
  if (e == hipSuccess) e = hipStreamCreate(&c->stream2);
  if (e == hipSuccess) e = hipStreamCreate(&c->stream3);
  if (e == hipSuccess) e = hipStreamCreate(&c->stream4);
  if (e == hipSuccess) e = hbo_malloc(c, (void**)&c->d_model, sizeof(ModelDev));
  if (e == hipSuccess) e = hbo_malloc(c, (void**)&c->d_yield, sizeof(int) * HBO_YIELD_TAB_ENTRIES);
  if (e == hipSuccess) e = hipMemset(c->d_yield, 0, sizeof(int) * HBO_YIELD_TAB_ENTRIES);
  if (e == hipSuccess) e = hipHostMalloc((void**)&c->h_model, sizeof(ModelDev), hipHostMallocDefault);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_upload, hipEventDisableTiming);
  if (e != hipSuccess) {
    hbo_g_err = std::string("hbo_ctx_create: ") + hipGetErrorString(e);
    delete c;
    return HBO_ERR_HIP;
  }
  { hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
      c->n_cus = prop.multiProcessorCount;
      c->lds_per_block = (int)std::min<size_t>(prop.sharedMemPerBlock, (size_t)1 << 30);
      // parked buffers of freed datasets / caches: at most a quarter of the device memory (option pool_cap_mb)
      c->pool_cap = std::min<size_t>(c->pool_cap, (size_t)prop.totalGlobalMem / 4);
    } }
  *out = c;
  return HBO_OK;
}
extern "C" int hbo_comm_destroy(hbo_ctx* ctx);
extern "C" int hbo_ctx_destroy(hbo_ctx* c) {
  if (!c) return HBO_OK;
  hipSetDevice(c->device);
  hbo_comm_destroy(c);
  prof_begin(c);
  for (int l = 0; l < HBO_MAX_MLP_LAYERS; ++l) { if (c->d_mlp_w[l]) hipFree(c->d_mlp_w[l]); if (c->d_mlp_b[l]) hipFree(c->d_mlp_b[l]); }
  for (hipEvent_t ev : c->prof_events) hipEventDestroy(ev);
  if (c->d_model) hipFree(c->d_model);
  if (c->d_yield) hipFree(c->d_yield);
  if (c->h_model) hipHostFree(c->h_model);
  if (c->hp_stage) hipHostFree(c->hp_stage);
  if (c->ev_upload) hipEventDestroy(c->ev_upload);
  for (auto& kv : c->ws) if (kv.second.first) hipFree(kv.second.first);
  for (auto& kv : c->pool_free) for (void* p : kv.second) hipFree(p);
  c->pool_free.clear(); c->pool_live.clear(); c->pool_bytes = 0;
  for (hipEvent_t ev : c->ev_pool) hipEventDestroy(ev);
  for (hipEvent_t ev : c->ev_pool_sweep) hipEventDestroy(ev);
  for (hipEvent_t ev : c->ev_timed) if (ev) hipEventDestroy(ev);
  if (c->stream4) hipStreamDestroy(c->stream4);
  if (c->stream3) hipStreamDestroy(c->stream3);
  if (c->stream2) hipStreamDestroy(c->stream2);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
  return HBO_OK;
}
// ---- options -------------------------------------------------------------------------------
// One table under hbo_set_option, hbo_get_option and hbo_tune.  PUBLIC rows are the options of the boundary (include/hbo.h): set and
// read by name, a value out of range answered with the row's message.  TUNE rows are the measurement hooks of include/hbo_tune.h:
// placement and overlap knobs of the schedules, for the A/B tools under tools/ and the scheduling sweep of the tests (every non-default
// value was measured equal or worse; none changes a result); hbo_tune sets them, nothing reads them back.  READ rows can only be read.
// Two public options are no int field and stand beside the table: pool_cap_mb (a size_t, and lowering it trims the pool) and bf16x3
// (sets four TUNE fields, reads as 1 only when all four are on).
namespace {
enum OptKind { OPT_PUBLIC, OPT_TUNE, OPT_READ };
struct Option { const char* name; int hbo_ctx::*field; int64_t lo, hi; const char* range_msg; OptKind kind; };
const Option options[] = {
    {"potrf_group", &hbo_ctx::opt_group, 0, 16, "potrf_group in 0..16 (0: auto)", OPT_PUBLIC},
    {"lookahead", &hbo_ctx::opt_lookahead, 0, 2, "lookahead in 0..2", OPT_PUBLIC},
    {"small_nblk", &hbo_ctx::opt_small_nblk, INT64_MIN, INT64_MAX, "", OPT_PUBLIC},   // (never had a range: any value, cut to int)
    {"post_chunk", &hbo_ctx::opt_post_chunk, 128, 65536, "post_chunk in 128..65536", OPT_PUBLIC},
    {"spectral", &hbo_ctx::opt_spectral, 0, 1, "spectral is 0 or 1", OPT_PUBLIC},
    {"acq_fused", &hbo_ctx::opt_acq_fused, 0, 1, "acq_fused is 0 or 1", OPT_PUBLIC},
    {"eig_sweeps", &hbo_ctx::eig_last_sweeps, 0, 0, nullptr, OPT_READ}, {"chol_form", &hbo_ctx::last_chol_form, 0, 0, nullptr, OPT_READ},
    {"inv_forms", &hbo_ctx::last_inv_forms, 0, 0, nullptr, OPT_READ}, {"post_resident", &hbo_ctx::last_post_resident, 0, 0, nullptr, OPT_READ},   // (chol_form, inv_forms: include/hbo_tune.h)
    {"overlap_trtri", &hbo_ctx::opt_overlap_trtri, 0, 1, nullptr, OPT_TUNE}, {"cu_yield", &hbo_ctx::opt_cu_yield, 0, 2, nullptr, OPT_TUNE}, {"persist_free", &hbo_ctx::opt_persist_free, -1, 200, nullptr, OPT_TUNE},
    {"trtri_at", &hbo_ctx::opt_trtri_at, 0, 63, nullptr, OPT_TUNE}, {"trtri_free", &hbo_ctx::opt_trtri_free, 0, 200, nullptr, OPT_TUNE}, {"lauum_persist", &hbo_ctx::opt_lauum_persist, 0, 128, nullptr, OPT_TUNE},
    {"split_f1", &hbo_ctx::opt_split_f1, 0, 2, nullptr, OPT_TUNE}, {"poison", &hbo_ctx::opt_poison, 0, 1, nullptr, OPT_TUNE}, {"sweep", &hbo_ctx::opt_sweep, 0, 2, nullptr, OPT_TUNE},
    {"sweep_qs", &hbo_ctx::opt_sweep_qs, 0, 16, nullptr, OPT_TUNE}, {"sweep_side", &hbo_ctx::opt_sweep_side, 0, 1, nullptr, OPT_TUNE}, {"sweep_free", &hbo_ctx::opt_sweep_free, 1, 200, nullptr, OPT_TUNE},
    {"sweep_big", &hbo_ctx::opt_sweep_big, 0, 1 << 30, nullptr, OPT_TUNE}, {"batch_bg", &hbo_ctx::opt_batch_bg, -1, 2, nullptr, OPT_TUNE}, {"post_bf16x3", &hbo_ctx::opt_post_bf16x3, 0, 1, nullptr, OPT_TUNE},
    {"post_f16x2", &hbo_ctx::opt_post_f16x2, 0, 1, nullptr, OPT_TUNE}, {"chol_f16x2", &hbo_ctx::opt_chol_f16x2, 0, 1, nullptr, OPT_TUNE}, {"group_inner", &hbo_ctx::opt_group_inner, -1, 16, nullptr, OPT_TUNE},
    {"syrk_bf16x3", &hbo_ctx::opt_syrk_bf16x3, 0, 1, nullptr, OPT_TUNE}, {"trtri_bf16x3", &hbo_ctx::opt_trtri_bf16x3, 0, 1, nullptr, OPT_TUNE}, {"lauum_bf16x3", &hbo_ctx::opt_lauum_bf16x3, 0, 1, nullptr, OPT_TUNE},
    {"trtri3_min_s", &hbo_ctx::opt_trtri3_min_s, 1, 1024, nullptr, OPT_TUNE}, {"fault_shard", &hbo_ctx::opt_fault_shard, 0, 2, nullptr, OPT_TUNE}, {"small_fused", &hbo_ctx::opt_small_fused, 0, 1, nullptr, OPT_TUNE},
    {"gram_mfma", &hbo_ctx::opt_gram_mfma, 0, 4096, nullptr, OPT_TUNE}, {"post_serial", &hbo_ctx::opt_post_serial, 0, 1, nullptr, OPT_TUNE}, {"syrk3_free", &hbo_ctx::opt_syrk3_free, 0, 200, nullptr, OPT_TUNE},
    {"spd_diag_bound", &hbo_ctx::opt_spd_diag_bound, 0, 1, nullptr, OPT_TUNE},
};
const Option* find_option(const char* name) {
  for (const Option& o : options) if (!strcmp(name, o.name)) return &o;
  return nullptr;
}
}  // namespace
extern "C" int hbo_set_option(hbo_ctx* c, const char* name, int64_t value) {
  if (!c || !name) return HBO_ERR_ARG;
  if (!strcmp(name, "pool_cap_mb")) {
    if (value < 0) return fail(c, HBO_ERR_ARG, "pool_cap_mb >= 0");
    c->pool_cap = (size_t)value << 20;
    if (c->pool_bytes > c->pool_cap) { hipSetDevice(c->device); pool_release_all(c); }   // trim: release everything parked (simple and rare)
    return HBO_OK;
  }
  if (!strcmp(name, "bf16x3")) { c->opt_post_bf16x3 = c->opt_syrk_bf16x3 = c->opt_trtri_bf16x3 = c->opt_lauum_bf16x3 = value != 0; return HBO_OK; }
  const Option* o = find_option(name);
  if (!o || o->kind != OPT_PUBLIC) return fail(c, HBO_ERR_ARG, std::string("unknown option ") + name);
  if (value < o->lo || value > o->hi) return fail(c, HBO_ERR_ARG, o->range_msg);
  c->*(o->field) = (int)value;
  return HBO_OK;
}
extern "C" int hbo_get_option(hbo_ctx* c, const char* name, int64_t* out) {
  if (!c || !name || !out) return fail(c, HBO_ERR_ARG, "hbo_get_option: null argument");
  if (!strcmp(name, "pool_cap_mb")) { *out = (int64_t)(c->pool_cap >> 20); return HBO_OK; }
  if (!strcmp(name, "bf16x3")) { *out = c->opt_post_bf16x3 && c->opt_syrk_bf16x3 && c->opt_trtri_bf16x3 && c->opt_lauum_bf16x3; return HBO_OK; }
  const Option* o = find_option(name);
  if (!o || o->kind == OPT_TUNE) return fail(c, HBO_ERR_ARG, std::string("unknown option ") + name);
  *out = c->*(o->field);
  return HBO_OK;
}
extern "C" int hbo_tune(hbo_ctx* c, const char* name, int64_t value) {
  if (!c || !name) return HBO_ERR_ARG;
  const Option* o = find_option(name);
  if (!o || o->kind != OPT_TUNE) return hbo_set_option(c, name, value);   // (the tools pass every name through one entry point)
  if (value < o->lo || value > o->hi) return fail(c, HBO_ERR_ARG, std::string(name) + " out of range");
  c->*(o->field) = (int)value;
  return HBO_OK;
}
extern "C" int hbo_profile_enable(hbo_ctx* c, int level) { if (!c) return HBO_ERR_ARG; c->prof_level = level; return HBO_OK; }
extern "C" int hbo_profile_get(hbo_ctx* c, char names[][32], double* ms, int32_t* launches, int32_t* n) {
  if (!c || !n) return HBO_ERR_ARG;
  int k = (int)std::min<size_t>(c->prof_names.size(), HBO_MAX_PROFILE_STAGES);
  for (int i = 0; i < k; ++i) {
    if (names) { strncpy(names[i], c->prof_names[i].c_str(), 31); names[i][31] = 0; }
    if (ms) ms[i] = c->prof_ms[i];
    if (launches) launches[i] = c->prof_count[i];
  }
  *n = k;
  return HBO_OK;
}

extern "C" int hbo_grad_layout_of(const hbo_model* m, hbo_grad_layout* out) {
  if (!m || !out) return HBO_ERR_ARG;
  const char* why = nullptr;
  if (int rc = check_input_warp(m, &why)) { hbo_g_err = std::string("hbo_grad_layout_of: ") + why; return rc; }
  int pos = 0;
  const bool dot = m->kernel_id == HBO_KERNEL_DOT;
  out->lengthscale = dot ? -1 : pos; if (!dot) pos += m->n_lengthscale;
  out->signal_variance = dot ? -1 : pos; if (!dot) pos += 1;
  out->noise_variance = pos++;
  out->constant = (m->mean_id == HBO_MEAN_CONSTANT) ? pos++ : -1;
  out->dot_prod_sigma = dot ? pos++ : -1;
  out->dot_prod_bias = dot ? pos++ : -1;
  const int fm = mean_feature_dim(m);
  out->linear_kernel = fm ? pos : -1; pos += fm;
  out->linear_bias = fm ? pos++ : -1;
  for (int l = 0; l < HBO_MAX_MLP_LAYERS; ++l) { out->mlp_kernel[l] = -1; out->mlp_bias[l] = -1; }
  if (needs_mlp(m)) {
    int fin = m->input_dim;
    for (int l = 0; l < m->n_layers; ++l) {
      out->mlp_kernel[l] = pos; pos += fin * m->features[l];
      out->mlp_bias[l] = pos; pos += m->features[l];
      fin = m->features[l];
    }
  }
  if (is_kumar(m)) pos += 2 * m->input_dim;   // d/da, d/db at the end (hbo_grad_layout_kumar_of)
  out->total = pos;
  return HBO_OK;
}
extern "C" int hbo_grad_layout_kumar_of(const hbo_model* m, int32_t* a_off, int32_t* b_off) {
  if (!m || !a_off || !b_off) return HBO_ERR_ARG;
  hbo_grad_layout lay;
  if (int rc = hbo_grad_layout_of(m, &lay)) return rc;
  *a_off = is_kumar(m) ? lay.total - 2 * m->input_dim : -1;
  *b_off = is_kumar(m) ? lay.total - m->input_dim : -1;
  return HBO_OK;
}

