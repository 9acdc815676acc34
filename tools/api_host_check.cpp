// Stand-alone comparison of the host helpers that api.hip, dataset.hip, dense.hip and cache.hip share since api.hip was split by topic
// (profiles/api_refactor.md) with the code they replaced: the option table under hbo_set_option / hbo_get_option / hbo_tune against the
// two strcmp chains and the knob table, task_stats against hbo_dataset_create's two loops, dataset_place / dataset_finish / task_shape
// against the layouts and tails of hbo_dataset_create and hbo_dataset_subsample, cols_to_rows / rows_to_cols against the six double loops.
// No GPU, no libhbo, host code only; it makes no HIP call (pool_bytes stays 0, so pool_cap_mb never trims):
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g tools/api_host_check.cpp -o tools/api_host_check && tools/api_host_check
// and once more with  -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all  on the same line.
// The "before" functions are the old lines as they stood.  Exit 0 and "ran clean" when nothing differs.
#include <cstdio>
#include <random>
#include <set>

#include "../hyperbo_amd/csrc/api.hip"
#include "../hyperbo_amd/csrc/dataset_host.h"

extern "C" int hbo_comm_destroy(hbo_ctx*) { return HBO_OK; }   // (link seam: comm.hip)

namespace {
long long n_cases = 0, n_bad = 0;
char where[256];
void differ(const char* what, bool same) {
  if (same) return;
  if (++n_bad <= 30) std::printf("DIFFERENT %s  (%s)\n", what, where);
}

// ---- before: the options of api.hip ------------------------------------------------------------------------------------------
int before_set_option(hbo_ctx* c, const char* name, int64_t value) {
  if (!c || !name) return HBO_ERR_ARG;
  if (!strcmp(name, "potrf_group")) { if (value < 0 || value > 16) return fail(c, HBO_ERR_ARG, "potrf_group in 0..16 (0: auto)"); c->opt_group = (int)value; return HBO_OK; }
  if (!strcmp(name, "lookahead")) { if (value < 0 || value > 2) return fail(c, HBO_ERR_ARG, "lookahead in 0..2"); c->opt_lookahead = (int)value; return HBO_OK; }
  if (!strcmp(name, "small_nblk")) { c->opt_small_nblk = (int)value; return HBO_OK; }
  if (!strcmp(name, "pool_cap_mb")) {
    if (value < 0) return fail(c, HBO_ERR_ARG, "pool_cap_mb >= 0");
    c->pool_cap = (size_t)value << 20;
    if (c->pool_bytes > c->pool_cap) { std::printf("the check reached the pool trim\n"); exit(2); }
    return HBO_OK;
  }
  if (!strcmp(name, "post_chunk")) { if (value < 128 || value > 65536) return fail(c, HBO_ERR_ARG, "post_chunk in 128..65536"); c->opt_post_chunk = (int)value; return HBO_OK; }
  if (!strcmp(name, "bf16x3")) { c->opt_post_bf16x3 = c->opt_syrk_bf16x3 = c->opt_trtri_bf16x3 = c->opt_lauum_bf16x3 = value != 0; return HBO_OK; }
  if (!strcmp(name, "spectral")) { if (value < 0 || value > 1) return fail(c, HBO_ERR_ARG, "spectral is 0 or 1"); c->opt_spectral = (int)value; return HBO_OK; }
  if (!strcmp(name, "acq_fused")) { if (value < 0 || value > 1) return fail(c, HBO_ERR_ARG, "acq_fused is 0 or 1"); c->opt_acq_fused = (int)value; return HBO_OK; }
  return fail(c, HBO_ERR_ARG, std::string("unknown option ") + name);
}
int before_get_option(hbo_ctx* c, const char* name, int64_t* out) {
  if (!c || !name || !out) return fail(c, HBO_ERR_ARG, "hbo_get_option: null argument");
  if (!strcmp(name, "potrf_group")) { *out = c->opt_group; return HBO_OK; }
  if (!strcmp(name, "lookahead")) { *out = c->opt_lookahead; return HBO_OK; }
  if (!strcmp(name, "small_nblk")) { *out = c->opt_small_nblk; return HBO_OK; }
  if (!strcmp(name, "pool_cap_mb")) { *out = (int64_t)(c->pool_cap >> 20); return HBO_OK; }
  if (!strcmp(name, "post_chunk")) { *out = c->opt_post_chunk; return HBO_OK; }
  if (!strcmp(name, "bf16x3")) { *out = c->opt_post_bf16x3 && c->opt_syrk_bf16x3 && c->opt_trtri_bf16x3 && c->opt_lauum_bf16x3; return HBO_OK; }
  if (!strcmp(name, "spectral")) { *out = c->opt_spectral; return HBO_OK; }
  if (!strcmp(name, "acq_fused")) { *out = c->opt_acq_fused; return HBO_OK; }
  if (!strcmp(name, "eig_sweeps")) { *out = c->eig_last_sweeps; return HBO_OK; }
  if (!strcmp(name, "chol_form")) { *out = c->last_chol_form; return HBO_OK; }
  if (!strcmp(name, "inv_forms")) { *out = c->last_inv_forms; return HBO_OK; }
  if (!strcmp(name, "post_resident")) { *out = c->last_post_resident; return HBO_OK; }
  return fail(c, HBO_ERR_ARG, std::string("unknown option ") + name);
}
struct Knob { const char* name; int hbo_ctx::*field; int64_t lo, hi; };
const Knob before_knobs[] = {
    {"overlap_trtri", &hbo_ctx::opt_overlap_trtri, 0, 1}, {"cu_yield", &hbo_ctx::opt_cu_yield, 0, 2},
    {"persist_free", &hbo_ctx::opt_persist_free, -1, 200}, {"trtri_at", &hbo_ctx::opt_trtri_at, 0, 63},
    {"trtri_free", &hbo_ctx::opt_trtri_free, 0, 200}, {"lauum_persist", &hbo_ctx::opt_lauum_persist, 0, 128}, {"split_f1", &hbo_ctx::opt_split_f1, 0, 2}, {"poison", &hbo_ctx::opt_poison, 0, 1},
    {"sweep", &hbo_ctx::opt_sweep, 0, 2}, {"sweep_qs", &hbo_ctx::opt_sweep_qs, 0, 16}, {"sweep_side", &hbo_ctx::opt_sweep_side, 0, 1}, {"sweep_free", &hbo_ctx::opt_sweep_free, 1, 200}, {"sweep_big", &hbo_ctx::opt_sweep_big, 0, 1 << 30}, {"batch_bg", &hbo_ctx::opt_batch_bg, -1, 2},
    {"post_bf16x3", &hbo_ctx::opt_post_bf16x3, 0, 1}, {"post_f16x2", &hbo_ctx::opt_post_f16x2, 0, 1}, {"chol_f16x2", &hbo_ctx::opt_chol_f16x2, 0, 1}, {"group_inner", &hbo_ctx::opt_group_inner, -1, 16}, {"syrk_bf16x3", &hbo_ctx::opt_syrk_bf16x3, 0, 1},
    {"trtri_bf16x3", &hbo_ctx::opt_trtri_bf16x3, 0, 1}, {"lauum_bf16x3", &hbo_ctx::opt_lauum_bf16x3, 0, 1}, {"trtri3_min_s", &hbo_ctx::opt_trtri3_min_s, 1, 1024},
    {"fault_shard", &hbo_ctx::opt_fault_shard, 0, 2}, {"small_fused", &hbo_ctx::opt_small_fused, 0, 1}, {"gram_mfma", &hbo_ctx::opt_gram_mfma, 0, 4096}, {"post_serial", &hbo_ctx::opt_post_serial, 0, 1},
    {"syrk3_free", &hbo_ctx::opt_syrk3_free, 0, 200}, {"spd_diag_bound", &hbo_ctx::opt_spd_diag_bound, 0, 1},
};
int before_tune(hbo_ctx* c, const char* name, int64_t value) {
  if (!c || !name) return HBO_ERR_ARG;
  for (const Knob& k : before_knobs)
    if (!strcmp(name, k.name)) {
      if (value < k.lo || value > k.hi) return fail(c, HBO_ERR_ARG, std::string(name) + " out of range");
      c->*(k.field) = (int)value;
      return HBO_OK;
    }
  return before_set_option(c, name, value);
}
// every int field an option function can reach (the knobs', the chains', the read-only ones)
const char* const chain_names[] = {"potrf_group", "lookahead", "small_nblk", "pool_cap_mb", "post_chunk", "bf16x3", "spectral", "acq_fused",
                                   "eig_sweeps", "chol_form", "inv_forms", "post_resident"};
int hbo_ctx::*const chain_fields[] = {&hbo_ctx::opt_group, &hbo_ctx::opt_lookahead, &hbo_ctx::opt_small_nblk, &hbo_ctx::opt_post_chunk, &hbo_ctx::opt_spectral,
                                      &hbo_ctx::opt_acq_fused, &hbo_ctx::eig_last_sweeps, &hbo_ctx::last_chol_form, &hbo_ctx::last_inv_forms, &hbo_ctx::last_post_resident};
std::vector<int hbo_ctx::*> all_fields() {
  std::vector<int hbo_ctx::*> f(std::begin(chain_fields), std::end(chain_fields));
  for (const Knob& k : before_knobs) f.push_back(k.field);
  for (const Option& o : options) f.push_back(o.field);
  return f;
}
// initial states: 0 every option field zero (and pool_cap 0); 1 the defaults of a fresh context; 2 field i holds i + 2, so that a read tells fields apart
void ctx_state(hbo_ctx& c, int state) {
  const std::vector<int hbo_ctx::*> f = all_fields();
  for (size_t i = 0; i < f.size(); ++i) if (state != 1) c.*(f[i]) = 0;
  if (state == 2) for (size_t i = 0; i < f.size(); ++i) c.*(f[i]) = (int)i + 2;
  if (state != 1) c.pool_cap = state == 2 ? (size_t)77 << 20 : 0;
  c.pool_bytes = 0;
}
bool same_ctx(const hbo_ctx& a, const hbo_ctx& b) {
  for (int hbo_ctx::*f : all_fields()) if (a.*f != b.*f) return false;
  return a.pool_cap == b.pool_cap && a.pool_bytes == b.pool_bytes && a.err == b.err;
}
void check_options() {
  std::vector<const char*> names(std::begin(chain_names), std::end(chain_names));
  for (const Knob& k : before_knobs) names.push_back(k.name);
  for (const Option& o : options) names.push_back(o.name);
  names.push_back("no_such_option"); names.push_back(""); names.push_back(nullptr);
  // every bound either side knows, one beside it on both sides, and the fixed values
  std::set<int64_t> values = {0, 1, -1, (int64_t)1 << 40, -((int64_t)1 << 40), INT64_MAX, INT64_MIN, (int64_t)INT_MAX + 1};
  auto bounds = [&](int64_t lo, int64_t hi) { values.insert(lo); values.insert(hi); if (lo > INT64_MIN) values.insert(lo - 1); if (hi < INT64_MAX) values.insert(hi + 1); };
  for (const Knob& k : before_knobs) bounds(k.lo, k.hi);
  for (const Option& o : options) bounds(o.lo, o.hi);
  bounds(0, 16); bounds(0, 2); bounds(128, 65536);
  for (const char* name : names)
    for (int state = 0; state < 3; ++state)
      for (int fn = 0; fn < 3; ++fn)
        for (int nullcase = 0; nullcase < 3; ++nullcase)   // 0: all arguments; 1: no context; 2: no `out` (hbo_get_option)
          for (int64_t v : values) {
            if (nullcase == 2 && fn != 1) continue;
            if (fn == 1 && v != 0) continue;   // (a read takes no value)
            hbo_ctx a, b;
            ctx_state(a, state); ctx_state(b, state);
            a.err = b.err = "untouched";
            int64_t oa = -12345, ob = -12345;
            hbo_g_err = "untouched";
            int ra, rb;
            hbo_ctx* pa = nullcase == 1 ? nullptr : &a; hbo_ctx* pb = nullcase == 1 ? nullptr : &b;
            if (fn == 0) ra = before_set_option(pa, name, v); else if (fn == 1) ra = before_get_option(pa, name, nullcase == 2 ? nullptr : &oa); else ra = before_tune(pa, name, v);
            const std::string ga = hbo_g_err;
            hbo_g_err = "untouched";
            if (fn == 0) rb = hbo_set_option(pb, name, v); else if (fn == 1) rb = hbo_get_option(pb, name, nullcase == 2 ? nullptr : &ob); else rb = hbo_tune(pb, name, v);
            std::snprintf(where, sizeof where, "%s(%s, %lld) state %d nullcase %d", fn == 0 ? "set" : (fn == 1 ? "get" : "tune"), name ? name : "NULL", (long long)v, state, nullcase);
            ++n_cases;
            differ("return code", ra == rb); differ("*out", oa == ob); differ("context fields / err", same_ctx(a, b)); differ("ctx-less error", ga == hbo_g_err);
          }
}

// ---- before: the per-task statistics of hbo_dataset_create -------------------------------------------------------------------------
void before_task_stats(const void* y, int64_t n, int m, int dtype, unsigned char* ys, unsigned char* yd) {
  for (int64_t i = 0; i < n; ++i) {
    double sum = 0;
    for (int a = 0; a < m; ++a) sum += host_elem(y, dtype, i * m + a);
    if (dtype == HBO_F64) ((double*)ys)[i] = sum; else ((float*)ys)[i] = (float)sum;
  }
  const double rs = 1.0 / sqrt((double)m);
  for (int64_t i = 0; i < n; ++i) {
    double mu0 = 0;
    for (int a = 0; a < m; ++a) mu0 += host_elem(y, dtype, i * m + a);
    mu0 /= m;
    for (int a = 0; a <= m; ++a) {
      const double v = a < m ? (host_elem(y, dtype, i * m + a) - mu0) * rs : -mu0;
      if (dtype == HBO_F64) ((double*)yd)[(size_t)a * n + i] = v; else ((float*)yd)[(size_t)a * n + i] = (float)v;
    }
  }
}
void check_task_stats() {
  std::mt19937_64 rng(7);
  std::normal_distribution<double> nd(0.0, 1.0);
  for (int dtype : {HBO_F32, HBO_F64})
    for (int64_t n : {1, 2, 127, 128, 129, 300})
      for (int m : {1, 2, 3, 127, 128, 129})
        for (int kind = 0; kind < 3; ++kind) {   // 0 random; 1 with a column of equal values; 2 magnitudes up to 1e30
          const size_t es = esize(dtype);
          std::vector<unsigned char> y((size_t)n * m * es);
          for (int64_t i = 0; i < n * m; ++i) {
            double v = nd(rng);
            if (kind == 1 && i % m == 0) v = 0.3;
            if (kind == 2) v *= (i % 3 == 0) ? 1e30 : ((i % 3 == 1) ? 1e-30 : 1.0);
            if (dtype == HBO_F64) ((double*)y.data())[i] = v; else ((float*)y.data())[i] = (float)v;
          }
          std::vector<unsigned char> s0((size_t)n * es + 8, 0xAB), s1(s0), d0((size_t)(m + 1) * n * es + 8, 0xCD), d1(d0);
          before_task_stats(y.data(), n, m, dtype, s0.data(), d0.data());
          task_stats(y.data(), n, m, dtype, s1.data(), d1.data());
          std::snprintf(where, sizeof where, "task_stats dtype %d n %lld m %d kind %d", dtype, (long long)n, m, kind);
          ++n_cases;
          differ("ysum bytes", s0 == s1); differ("ydiv bytes", d0 == d1);
        }
}

// ---- before: layouts, shapes and task order of hbo_dataset_create / hbo_dataset_subsample -------------------------------------------
struct OldOff { size_t x, ysum, ydiv; };
void check_layouts() {
  std::mt19937_64 rng(11);
  const int64_t ns[] = {0, 1, 5, 5, 127, 128, 129, 300, 300, 1290, -3};
  for (int dtype : {HBO_F32, HBO_F64})
    for (int D : {1, 4, 7})
      for (int rep = 0; rep < 200; ++rep) {
        const size_t es = esize(dtype);
        const int T = 1 + (int)(rng() % 12);
        std::vector<int64_t> n(T); std::vector<int> m(T);
        for (int k = 0; k < T; ++k) { n[k] = ns[rng() % (sizeof ns / sizeof ns[0])]; m[k] = 1 + (int)(rng() % 4) * 43; }
        std::snprintf(where, sizeof where, "layout dtype %d D %d rep %d", dtype, D, rep);
        // create: the old first loop, tasks with n <= 0 skipped
        std::vector<OldOff> old(T, OldOff{0, 0, 0});
        BlockLayout lay0;
        for (int k = 0; k < T; ++k) {
          if (n[k] <= 0) continue;
          old[k].x = lay0.take((size_t)n[k] * D * es); old[k].ysum = lay0.take((size_t)n[k] * es);
          old[k].ydiv = lay0.take((size_t)(m[k] + 1) * n[k] * es);
        }
        hbo_dataset before, now;
        before.dtype = now.dtype = dtype;
        before.d_inputs = now.d_inputs = reinterpret_cast<void*>((uintptr_t)1 << 32);   // (a stand-in base: only compared)
        BlockLayout lay1;
        for (int k = 0; k < T; ++k) {
          if (n[k] <= 0) continue;
          const TaskOff o = dataset_place(lay1, n[k], D, m[k], true, es);
          ++n_cases;
          differ("create offsets", o.x == old[k].x && o.ysum == old[k].ysum && o.ydiv == old[k].ydiv);
          // the old second loop's TaskHost
          TaskHost* t = new TaskHost();
          before.tasks.push_back(t);
          t->owns_inputs = false;
          t->n = n[k]; t->m = m[k]; t->npad = round_up(n[k], HBO_TILE); t->nblk = t->npad / HBO_TILE; t->ld = padded_ld(t->npad, dtype);
          t->X = (char*)before.d_inputs + old[k].x; t->ysum = (char*)before.d_inputs + old[k].ysum; t->ydiv = (char*)before.d_inputs + old[k].ydiv;
          before.max_nblk = std::max(before.max_nblk, t->nblk);
          t->svec_cols = k;   // (the caller's index rides along: shows the order among equal n)
          dataset_add_task(&now, n[k], m[k], o, true)->svec_cols = k;
        }
        differ("create total", lay0.off == lay1.off);
        before.ntasks = (int)before.tasks.size();
        std::stable_sort(before.tasks.begin(), before.tasks.end(), [](TaskHost* a, TaskHost* b) { return a->n > b->n; });
        dataset_finish(&now);
        auto same_tasks = [&](const hbo_dataset& a, const hbo_dataset& b) {
          bool same = a.ntasks == b.ntasks && a.max_nblk == b.max_nblk && a.tasks.size() == b.tasks.size();
          for (size_t z = 0; same && z < a.tasks.size(); ++z) {
            const TaskHost *p = a.tasks[z], *q = b.tasks[z];
            same = p->svec_cols == q->svec_cols && p->n == q->n && p->m == q->m && p->npad == q->npad && p->nblk == q->nblk && p->ld == q->ld &&
                   p->X == q->X && p->ysum == q->ysum && p->ydiv == q->ydiv && p->owns_inputs == q->owns_inputs;
          }
          return same;
        };
        ++n_cases;
        differ("create tasks and their order", same_tasks(before, now));
        // subsample of that dataset: counts negative (the whole task), n, or smaller; the source with or without divergence rows
        for (int has_ydiv = 0; has_ydiv < 2; ++has_ydiv) {
          hbo_dataset sb, sn;
          sb.dtype = sn.dtype = dtype;
          sb.d_inputs = sn.d_inputs = reinterpret_cast<void*>((uintptr_t)1 << 33);
          BlockLayout l0, l1;
          const int Ts = now.ntasks;
          std::vector<OldOff> so(Ts);
          std::vector<int64_t> cnt(Ts);
          for (int k = 0; k < Ts; ++k) {
            const TaskHost* t = now.tasks[k];
            const int pick = (int)(rng() % 3);
            cnt[k] = pick == 0 ? -1 : (pick == 1 ? t->n : 1 + (int64_t)(rng() % t->n));
            const int64_t nd = cnt[k] < 0 ? t->n : cnt[k];
            so[k].x = l0.take((size_t)nd * D * es); so[k].ysum = l0.take((size_t)nd * es);
            so[k].ydiv = has_ydiv ? l0.take((size_t)(t->m + 1) * nd * es) : 0;
            const TaskOff o = dataset_place(l1, nd, D, t->m, has_ydiv != 0, es);
            ++n_cases;
            differ("subsample offsets", o.x == so[k].x && o.ysum == so[k].ysum && o.ydiv == so[k].ydiv);
            TaskHost* u = new TaskHost();
            sb.tasks.push_back(u);
            u->owns_inputs = false;
            u->n = nd; u->m = t->m; u->npad = round_up(nd, HBO_TILE); u->nblk = u->npad / HBO_TILE; u->ld = padded_ld(u->npad, dtype);
            u->X = (char*)sb.d_inputs + so[k].x; u->ysum = (char*)sb.d_inputs + so[k].ysum;
            if (has_ydiv) u->ydiv = (char*)sb.d_inputs + so[k].ydiv;
            sb.max_nblk = std::max(sb.max_nblk, u->nblk);
            u->svec_cols = k;
            dataset_add_task(&sn, nd, t->m, o, has_ydiv != 0)->svec_cols = k;
          }
          differ("subsample total", l0.off == l1.off);
          sb.ntasks = (int)sb.tasks.size();
          std::stable_sort(sb.tasks.begin(), sb.tasks.end(), [](TaskHost* a, TaskHost* b) { return a->n > b->n; });
          dataset_finish(&sn);
          ++n_cases;
          differ("subsample tasks and their order", same_tasks(sb, sn));
          for (hbo_dataset* d : {&sb, &sn}) for (TaskHost* t : d->tasks) delete t;
        }
        for (hbo_dataset* d : {&before, &now}) for (TaskHost* t : d->tasks) delete t;
      }
}

// ---- before: the six column <-> row loops ------------------------------------------------------------------------------------------
void check_repack() {
  std::mt19937_64 rng(13);
  for (size_t es : {(size_t)4, (size_t)8})
    for (int64_t n : {1, 2, 63, 64, 65, 127, 128, 129, 300})
      for (int m : {1, 2, 3, 127, 128})
        for (int64_t npad : {n, (int64_t)round_up(n, 64), (int64_t)round_up(n, 128)})   // (n itself: the y^T of hbo_factor / hbo_acq_samples)
          for (int prefill : {0x00, 0xEE}) {
            std::vector<unsigned char> cols((size_t)n * m * es);
            for (unsigned char& b : cols) b = (unsigned char)(1 + rng() % 200);
            std::snprintf(where, sizeof where, "repack es %zu n %lld m %d npad %lld prefill %d", es, (long long)n, m, (long long)npad, prefill);
            // host -> device rows: hbo_chol_solve's loop (= transpose_y's with npad = n)
            std::vector<unsigned char> r0((size_t)m * npad * es, (unsigned char)prefill), r1(r0);
            for (int64_t i = 0; i < n; ++i)
              for (int a = 0; a < m; ++a) memcpy(r0.data() + ((size_t)a * npad + i) * es, cols.data() + ((size_t)i * m + a) * es, es);
            cols_to_rows(r1.data(), cols.data(), n, m, npad, es);
            ++n_cases;
            differ("cols_to_rows bytes (padding included)", r0 == r1);
            bool pad_kept = true;
            for (int a = 0; a < m; ++a) for (size_t b = (size_t)(a * npad + n) * es; b < (size_t)(a + 1) * npad * es; ++b) pad_kept = pad_kept && r1[b] == (unsigned char)prefill;
            differ("cols_to_rows leaves the padding alone", pad_kept);
            // device rows -> host: hbo_chol_solve's loop (rows outer) and hbo_cache_export's / hbo_spd_solve's (columns outer)
            std::vector<unsigned char> c0((size_t)n * m * es, 0x55), c1(c0), c2(c0);
            for (int64_t i = 0; i < n; ++i)
              for (int a = 0; a < m; ++a) memcpy(c0.data() + ((size_t)i * m + a) * es, r0.data() + ((size_t)a * npad + i) * es, es);
            for (int a = 0; a < m; ++a)
              for (int64_t i = 0; i < n; ++i) memcpy(c1.data() + ((size_t)i * m + a) * es, r0.data() + ((size_t)a * npad + i) * es, es);
            rows_to_cols(c2.data(), r1.data(), n, m, npad, es);
            ++n_cases;
            differ("rows_to_cols bytes", c0 == c2 && c1 == c2); differ("round trip", c2 == cols);
          }
}

// ---- before: the shape lines of the four TaskHost sites ---------------------------------------------------------------------------------
void check_task_shape() {
  for (int dtype : {HBO_F32, HBO_F64})
    for (int64_t n = 1; n <= 70000; n += (n < 600 ? 1 : 977))
      for (int m : {1, 3, 128}) {
        TaskHost a, b;
        a.n = n; a.m = m; a.npad = round_up(n, HBO_TILE); a.nblk = a.npad / HBO_TILE; a.ld = padded_ld(a.npad, dtype);
        task_shape(&b, n, m, dtype);
        std::snprintf(where, sizeof where, "task_shape dtype %d n %lld m %d", dtype, (long long)n, m);
        ++n_cases;
        differ("shape", a.n == b.n && a.m == b.m && a.npad == b.npad && a.nblk == b.nblk && a.ld == b.ld);
      }
}
}  // namespace

int main() {
  check_options();
  const long long n_opt = n_cases;
  check_task_stats();
  const long long n_stats = n_cases - n_opt;
  check_layouts();
  const long long n_lay = n_cases - n_opt - n_stats;
  check_repack();
  check_task_shape();
  std::printf("%lld cases (%lld options, %lld task statistics, %lld layouts and orders, %lld repacks and shapes), %lld differences%s\n", n_cases, n_opt, n_stats,
              n_lay, n_cases - n_opt - n_stats - n_lay, n_bad, n_bad ? "" : ": ran clean");
  return n_bad ? 1 : 0;
}
