// Host-side internals shared by the translation units of the C ABI (api.hip: context, options, profile, gradient layout; dataset.hip:
// datasets; dense.hip: the dense entry points on host arrays; probe.hip: the hooks of include/hbo_tune.h; objective.hip: hbo_objective /
// hbo_objective_sharded; cache.hip: hbo_factor, cache export, row append, posterior, acquisition; acq_grad.hip: its gradient): model validation and upload, the set-up the batched entry points share (model_family_check, mlp_shape, models_pack,
// stage_begin / stage_upload), the MLP feature pipeline and the query-side features of everything that reads a factor
// (query_features), the per-task device buffers and the descriptors the kernels read, the plans of a posterior call and of an
// objective evaluation (post_plan, obj_plan: every decision, no HIP call), and the gradient scatter table of the objectives
// (GradScatter).
#pragma once
#include "ctx.h"

#include <dlfcn.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "runtime.h"
#include "sched.h"

// ---- model ---------------------------------------------------------------------------------
static int feature_dim(const hbo_model* m) {
  return m->kernel_uses_mlp ? m->features[m->n_layers - 1] : m->input_dim;
}
static int mean_feature_dim(const hbo_model* m) {
  if (m->mean_id == HBO_MEAN_LINEAR) return m->input_dim;
  if (m->mean_id == HBO_MEAN_LINEAR_MLP) return m->features[m->n_layers - 1];
  return 0;
}
static bool needs_mlp(const hbo_model* m) { return m->kernel_uses_mlp || m->mean_id == HBO_MEAN_LINEAR_MLP; }
// Kumaraswamy input warp (hbo.h hbo_model_kumar): the covariance reads w(x) from a buffer of its own, the mean the raw x
static bool is_kumar(const hbo_model* m) { return m->input_warp == HBO_WARP_KUMAR; }
static const hbo_model_kumar* as_kumar(const hbo_model* m) { return reinterpret_cast<const hbo_model_kumar*>(m); }
// host-only part of the check (no context needed: hbo_grad_layout_of runs it too)
static int check_input_warp(const hbo_model* m, const char** why) {
  if (m->input_warp == HBO_WARP_NONE) return HBO_OK;
  if (m->input_warp != HBO_WARP_KUMAR) { *why = "unknown input_warp"; return HBO_ERR_UNSUPPORTED; }
  if (m->kernel_uses_mlp) { *why = "a Kumaraswamy warp together with an MLP basis is not supported"; return HBO_ERR_UNSUPPORTED; }
  if (!as_kumar(m)->kumar_a || !as_kumar(m)->kumar_b) { *why = "kumar_a / kumar_b missing"; return HBO_ERR_ARG; }
  return HBO_OK;
}
// an hbo_model, or the hbo_model_kumar it heads, copied whole (callers that modify a copy of the model must not drop a, b)
struct ModelCopy {
  hbo_model_kumar k;
  explicit ModelCopy(const hbo_model* m) { memset(&k, 0, sizeof k); if (is_kumar(m)) k = *as_kumar(m); else k.base = *m; }
  hbo_model* get() { return &k.base; }
};

static int validate_model(hbo_ctx* c, const hbo_model* m) {
  if (!m) return fail(c, HBO_ERR_ARG, "model is null");
  if (m->dtype != HBO_F32 && m->dtype != HBO_F64) return fail(c, HBO_ERR_ARG, "bad dtype");
  if (m->kernel_id < 0 || m->kernel_id > HBO_KERNEL_DOT) return fail(c, HBO_ERR_ARG, "bad kernel_id");
  if (m->mean_id < 0 || m->mean_id > HBO_MEAN_LINEAR_MLP) return fail(c, HBO_ERR_ARG, "bad mean_id");
  if (m->input_dim <= 0 || m->input_dim > HBO_MAX_FEATURE_DIM) return fail(c, HBO_ERR_ARG, "bad input_dim");
  const char* why = nullptr;   // (before the MLP fields: a Kumaraswamy model with an MLP basis is UNSUPPORTED, whatever they hold)
  if (int rc = check_input_warp(m, &why)) return fail(c, rc, why);
  if (needs_mlp(m)) {
    if (m->n_layers <= 0 || m->n_layers > HBO_MAX_MLP_LAYERS) return fail(c, HBO_ERR_ARG, "bad n_layers");
    for (int l = 0; l < m->n_layers; ++l) {
      if (m->features[l] <= 0 || m->features[l] > HBO_MAX_FEATURE_DIM) return fail(c, HBO_ERR_ARG, "bad mlp feature size");
      if (!m->mlp_kernel[l] || !m->mlp_bias[l]) return fail(c, HBO_ERR_ARG, "mlp parameters missing");
    }
  }
  const int fd = feature_dim(m);
  if (m->kernel_id != HBO_KERNEL_DOT) {
    if (!m->lengthscale) return fail(c, HBO_ERR_ARG, "lengthscale missing");
    if (m->n_lengthscale != 1 && m->n_lengthscale != fd)
      return fail(c, HBO_ERR_ARG, "lengthscale must have 1 or feature-dim entries");
  }
  if (mean_feature_dim(m) > 0 && !m->linear_kernel) return fail(c, HBO_ERR_ARG, "linear_mean kernel missing");
  return HBO_OK;
}

// S hyper-parameter samples of ONE model family: same dtype, covariance, mean, input_dim and MLP architecture -- everything that
// shapes a launch; only the values differ
static bool same_model_family(const hbo_model* m, const hbo_model* m0) {
  bool same = m->dtype == m0->dtype && m->kernel_id == m0->kernel_id && m->mean_id == m0->mean_id && m->input_dim == m0->input_dim &&
              m->kernel_uses_mlp == m0->kernel_uses_mlp && m->n_lengthscale == m0->n_lengthscale && needs_mlp(m) == needs_mlp(m0);
  if (same && needs_mlp(m0)) { same = m->n_layers == m0->n_layers; for (int l = 0; same && l < m0->n_layers; ++l) same = m->features[l] == m0->features[l]; }
  return same;
}
// What every batched entry point asks of its S models, per sample in this order: no input warp (HBO_ERR_UNSUPPORTED; before
// validate_model: a packed array element has no hbo_model_kumar tail to read), a valid model, the family of models[0] (HBO_ERR_ARG).
// fn: "hbo_xyz: ", the head of every message; advice: what to call instead for a warped model.  Touches no device (c may be null).
static int model_family_check(hbo_ctx* c, const std::string& fn, const hbo_model* models, int32_t S, const char* advice) {
  for (int s = 0; s < S; ++s) {
    const hbo_model* m = &models[s];
    if (m->input_warp != HBO_WARP_NONE) return fail(c, HBO_ERR_UNSUPPORTED, fn + "input-warped (Kumaraswamy) models are not supported; " + advice);
    if (int rc = validate_model(c, m)) return rc;
    if (!same_model_family(m, &models[0])) return fail(c, HBO_ERR_ARG, fn + "the samples' models must share dtype, covariance, mean, input_dim and MLP architecture");
  }
  return HBO_OK;
}

// The MLP of a model layer by layer (L = 0 without one): inputs, outputs, bytes of the weights [fin][fout] and of the bias, and
// `per_sample`, the bytes of one model's weights with every array at a 256-byte boundary (models_pack below)
struct MlpShape { int L; int fin[HBO_MAX_MLP_LAYERS], fout[HBO_MAX_MLP_LAYERS]; size_t wb[HBO_MAX_MLP_LAYERS], bb[HBO_MAX_MLP_LAYERS]; size_t per_sample; };
static MlpShape mlp_shape(const hbo_model* m) {
  MlpShape s = {};
  if (!needs_mlp(m)) return s;
  s.L = m->n_layers;
  int fin = m->input_dim;
  for (int l = 0; l < s.L; ++l) {
    s.fin[l] = fin; s.fout[l] = m->features[l];
    s.wb[l] = (size_t)fin * m->features[l] * esize(m->dtype); s.bb[l] = (size_t)m->features[l] * esize(m->dtype);
    s.per_sample += align256(s.wb[l]) + align256(s.bb[l]);
    fin = m->features[l];
  }
  return s;
}

static double host_elem(const void* p, int dtype, int64_t i) {
  return dtype == HBO_F64 ? ((const double*)p)[i] : (double)((const float*)p)[i];
}

// max_i A_ii of Gram + (noise + jitter) I for a stationary covariance (k(x, x) = signal variance): what the fp32 factorisation's
// f16x2 products scale the factor's entries by (ctx.h: chol_diag_bound); 0 = unknown (dot-product kernel, parameters not finite)
static inline double chol_diag_bound_of(const hbo_model* m) {
  if (m->kernel_id == HBO_KERNEL_DOT) return 0.0;
  const double b = (double)m->signal_variance + (double)m->noise_variance + (double)m->eps;
  return (b > 0 && b < 1e30) ? b : 0.0;
}
// ... of a batch of S models factorised together: the largest bound; any unknown -> unknown
static inline double chol_diag_bound_of(const hbo_model* models, int S) {
  double all = chol_diag_bound_of(&models[0]);
  for (int s = 1; s < S; ++s) { const double b = chol_diag_bound_of(&models[s]); all = (b > 0 && all > 0) ? std::max(all, b) : 0.0; }
  return all;
}
struct CholBoundScope {   // valid from run_potrf to the last product of the inverse / K^-1 of the same matrices
  hbo_ctx* c;
  CholBoundScope(hbo_ctx* ctx, double b) : c(ctx) { c->run.chol_diag_bound = b; }
  ~CholBoundScope() { c->run.chol_diag_bound = 0; }
};
// the device-side form of an (already warped) model (model_dev_fill: the same code fills it on the device in hbo_train_adam)
static void fill_model_dev(ModelDev& h, const hbo_model* m) {
  memset(&h, 0, sizeof h);
  model_dev_fill(h, m, 0, 1);
}
// S models of one family and their MLP weights as ONE block (hbo_acq_samples, hbo_bo_simulated):
//   [ModelDev[S]] [sample 0: per layer the weights, then the bias, each at a 256-byte boundary] [sample 1: ...] ...
// models_pack fills its host copy `h` (models_pack_bytes; the padding is the caller's to zero) and the tables w_dev / b_dev
// [S][HBO_MAX_MLP_LAYERS] with the addresses the arrays have once the block sits at d_base on the device.
static size_t models_pack_bytes(const MlpShape& sh, int S) { return align256(sizeof(ModelDev) * S) + sh.per_sample * S; }
static void models_pack(char* h, char* d_base, const hbo_model* models, int S, const MlpShape& sh, void** w_dev, void** b_dev) {
  ModelDev* hm = reinterpret_cast<ModelDev*>(h);
  BlockLayout lay;
  lay.take(sizeof(ModelDev) * S);
  for (int s = 0; s < S; ++s) {
    fill_model_dev(hm[s], &models[s]);
    for (int l = 0; l < sh.L; ++l) {
      const size_t o_w = lay.take(sh.wb[l]), o_b = lay.take(sh.bb[l]);
      memcpy(h + o_w, models[s].mlp_kernel[l], sh.wb[l]); memcpy(h + o_b, models[s].mlp_bias[l], sh.bb[l]);
      w_dev[(size_t)s * HBO_MAX_MLP_LAYERS + l] = d_base + o_w; b_dev[(size_t)s * HBO_MAX_MLP_LAYERS + l] = d_base + o_b;
    }
  }
}

// ---- the pinned stage ------------------------------------------------------------------------
// Small uploads go through ONE pinned buffer per context, hp_stage (and the model through a pinned ModelDev of its own, h_model),
// copied asynchronously; ev_upload marks the last such copy.  The protocol, whole:
//   stage_begin(c, fn, bytes) -> fill -> stage_upload(c, dst, stage, bytes, st)
// stage_begin waits until the previous upload has read the buffer, then returns it grown to `bytes` (null: c->err says why, behind fn = "hbo_xyz: ");
// stage_upload queues the copy and records ev_upload behind it.  Two rules keep this free of races:
//   * between the fill and stage_upload nothing may ask for a LARGER stage (stage_begin, pinned_stage): growing frees the buffer;
//   * after stage_upload the buffer is not written again before the next stage_begin (stage_wait) has returned.
// A call may also use the buffer as the target of a copy BACK on the stream of its uploads (pinned_stage alone: such a copy is
// ordered behind them).
static void* pinned_stage(hbo_ctx* c, size_t bytes) {
  if (c->hp_stage_bytes < bytes) {
    if (c->hp_stage) { hipDeviceSynchronize(); hipHostFree(c->hp_stage); c->hp_stage = nullptr; c->hp_stage_bytes = 0; }
    const size_t want = std::max<size_t>(bytes * 2, 1 << 16);
    if (hipHostMalloc(&c->hp_stage, want, hipHostMallocDefault) != hipSuccess) { c->hp_stage = nullptr; return nullptr; }
    c->hp_stage_bytes = want;
  }
  return c->hp_stage;
}
static hipError_t stage_wait(hbo_ctx* c) { return hipEventSynchronize(c->ev_upload); }
static void* stage_begin(hbo_ctx* c, const char* fn, size_t bytes) {
  const hipError_t e = stage_wait(c);
  if (e != hipSuccess) { fail(c, HBO_ERR_HIP, std::string(fn) + "waiting for the last staged upload failed: " + hipGetErrorString(e)); return nullptr; }
  void* p = pinned_stage(c, bytes);
  if (!p) fail(c, HBO_ERR_HIP, std::string(fn) + "no pinned staging memory");
  return p;
}
static hipError_t stage_upload(hbo_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st) {
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
  return e != hipSuccess ? e : hipEventRecord(c->ev_upload, st);
}

// hbo_objective's per-call work up to the copy back (objective.hip).  With `sh` set it reduces [nll, count, grad] on the device into
// ShardOut::d_red with the scatter map it uploads (launch_shard_reduce) and returns without waiting: the sharded objective all-reduces
// that buffer, hbo_train_adam (train.hip) queues its first Adam step behind it and reuses the map for the steps after it.
struct ShardReq { double* count; double* timing; };
struct ShardOut { double* d_red = nullptr; hipEvent_t ev0 = nullptr, ev1 = nullptr; int red_count = 0; int* d_map = nullptr; int nseg = 0; int out_stride = 0; };
int objective_local(hbo_ctx* c, const hbo_model* m_in, hbo_dataset* ds, int objective, double* nll_sum, double* nll_per_task,
                    double* grad_sum, const ShardReq* sh, ShardOut* so);
// Two pieces of an evaluation with gradient that the test hook hbo_probe_factor_inverse (probe.hip) runs as well (objective.hip):
// the fork to the stream of the small reductions behind run_potrf (side_reduce: the idle panel stream; otherwise the main stream
// itself), and everything between the factorisation and the contraction -- W = L^-1 and K^-1 by the route of inv.pl, alpha = W^T z
// for the first max_naug augmented rows behind W on `side`, there also d f / d mu (dmu_obj: the objective; < 0: none).  Returns the
// event behind the side stream's work, which the main stream has been told to wait for (null: there is no side stream).
hipStream_t obj_fork_side(hbo_ctx* c, bool side_reduce);
hipEvent_t obj_inverse_step(hbo_ctx* c, InvRun& inv, int max_naug, hipStream_t side, int dmu_obj);
// one row gather of hbo_dataset_subsample (dataset.hip): row r of task blockIdx.y of the destination = row idx[idx_off + r] (or r) of
// the source task; hbo_train_adam points the destinations at a batch that already exists and overwrites its rows in place
struct GatherTask { const void* sx; const void* sys; const void* syd; void* dx; void* dys; void* dyd; int64_t n_src, n_dst, idx_off; int m, has_idx; };
void launch_gather_rows(int dtype, const GatherTask* tasks, const int32_t* idx, int T, int64_t max_dst, int D, hipStream_t st);
// the launches of one single-workgroup evaluation (forward) and of the backward passes, without any host-side set-up
void enqueue_fused_forward(hbo_ctx* c, const hbo_model* m, hbo_dataset* ds, int64_t max_n, int out_stride, bool want_grad);
int enqueue_backward(hbo_ctx* c, const hbo_model* m, hbo_dataset* ds, int64_t max_n, int obj, bool want_grad);
void launch_shard_reduce(const double* nll, const double* grad, const int* info, int T, int out_stride, const int* map,
                         const double* mlp, const int* mlp_seg, int n_mlp_seg, double* out, int out_count, hipStream_t st);   // grad.hip
// Task-sharded form (hbo_objective_sharded): the sums over this rank's tasks are formed on the device, all-reduced in place
// over the context's RCCL communicator and copied to the host once.
int comm_allreduce_device(hbo_ctx* c, double* d_buf, int count, hipStream_t st);   // comm.hip
// The sharded form never leaves its peers alone in the collective: objective_local does everything up to (not including) the
// all-reduce and hands back the device buffer [nll, count, grad]; whatever it returns, objective_impl then takes part in the ONE
// all-reduce of the evaluation -- with NaN in every slot after a local failure (the peers see a NaN objective, not a hang) --
// and only if not even that buffer can be had does it abort the communicator, so that the peers' collective fails too.
int comm_abort(hbo_ctx* c);   // comm.hip

// fills ctx->h_model, uploads it and the MLP weights
static int upload_model(hbo_ctx* c, const hbo_model* m) {
  int rc = validate_model(c, m);
  if (rc) return rc;
  // the pinned copy may still be read by the previous upload (calls that return without waiting for the stream)
  HIPCHK(c, stage_wait(c));
  ModelDev& h = *c->h_model;
  fill_model_dev(h, m);
  HIPCHK(c, stage_upload(c, c->d_model, &h, sizeof h, c->stream));
  const MlpShape sh = mlp_shape(m);
  for (int l = 0; l < sh.L; ++l) {
    const size_t wb = sh.wb[l], bb = sh.bb[l];
    if (c->mlp_w_bytes[l] < wb) { if (c->d_mlp_w[l]) hipFree(c->d_mlp_w[l]); HIPCHK(c, hbo_malloc(c, &c->d_mlp_w[l], wb)); c->mlp_w_bytes[l] = wb; }
    if (c->mlp_b_bytes[l] < bb) { if (c->d_mlp_b[l]) hipFree(c->d_mlp_b[l]); HIPCHK(c, hbo_malloc(c, &c->d_mlp_b[l], bb)); c->mlp_b_bytes[l] = bb; }
    HIPCHK(c, hipMemcpyAsync(c->d_mlp_w[l], m->mlp_kernel[l], wb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_mlp_b[l], m->mlp_bias[l], bb, hipMemcpyHostToDevice, c->stream));
  }
  // the MLP weights come from the caller's pageable memory: make sure the copies have consumed them
  if (sh.L) HIPCHK(c, hipStreamSynchronize(c->stream));
  return HBO_OK;
}

// ---- feature pipeline ----------------------------------------------------------------------
// Computes the MLP activations of x (n x D, device) into acts[l] (allocated by the caller: n x f_l)
// (w / b: the layers' device weights -- the context's own copy of the last uploaded model unless a caller keeps several;
//  st: the context's main stream unless given)
static void run_mlp(hbo_ctx* c, const hbo_model* m, const void* x, int64_t n, void* const* acts, void* const* w = nullptr, void* const* b = nullptr,
                    hipStream_t st = nullptr) {
  const void* in = x;
  int fin = m->input_dim;
  if (!w) { w = c->d_mlp_w; b = c->d_mlp_b; }
  if (!st) st = c->stream;
  for (int l = 0; l < m->n_layers; ++l) {
    launch_dense_tanh(m->dtype, in, w[l], b[l], acts[l], n, fin, m->features[l], st);
    in = acts[l];
    fin = m->features[l];
  }
}

// The query side of everything that reads a factor (row append, posterior, d acquisition / dx): for `n` rows xq (device) the MLP
// activations into acts[l] (n x f_l each; unused without an MLP), the warped rows into `wq` (Kumaraswamy models; null otherwise), then
// the prior mean into mu0 and k(x, x) into kd, all on `st`.  The mean reads the raw x (or the MLP output), the covariance w(x).
// md / w / b: the model and its MLP weights on the device.  timed: the "features" / "kumar_forward" scopes of the profile.
struct QueryFeat { const void* Fq; const void* fq_last; };   // what the covariance reads; the last MLP layer (null without an MLP)
static QueryFeat query_features(hbo_ctx* c, const hbo_model* m, const ModelDev* md, void* const* w, void* const* b, const void* xq, int64_t n,
                                void* const* acts, void* wq, void* mu0, void* kd, hipStream_t st, bool timed = false) {
  const int lvl = timed ? 1 : INT_MAX;
  QueryFeat f = {nullptr, nullptr};
  { ProfScope ps(c, "features", lvl, st);
    if (needs_mlp(m)) { run_mlp(c, m, xq, n, acts, w, b, st); f.fq_last = acts[m->n_layers - 1]; } }
  f.Fq = m->kernel_uses_mlp ? f.fq_last : xq;
  if (is_kumar(m)) {
    ProfScope ps(c, "kumar_forward", lvl, st);
    launch_kumar_forward(m->dtype, nullptr, 0, 0, xq, wq, nullptr, n, m->input_dim, md, st);
    f.Fq = wq;
  }
  const void* Fmq = (m->mean_id == HBO_MEAN_LINEAR) ? xq : (m->mean_id == HBO_MEAN_LINEAR_MLP ? f.fq_last : nullptr);
  launch_mean(m->dtype, Fmq, n, mean_feature_dim(m), md, mu0, st);
  launch_kdiag(m->dtype, f.Fq, n, feature_dim(m), md, kd, st);
  return f;
}

struct FeatBuf {   // device activations of one input matrix
  std::vector<void*> acts; std::vector<size_t> bytes;
  ~FeatBuf() { for (void* p : acts) if (p) hipFree(p); }
  int ensure(hbo_ctx* c, const hbo_model* m, int64_t n) {
    acts.resize(HBO_MAX_MLP_LAYERS, nullptr); bytes.resize(HBO_MAX_MLP_LAYERS, 0);
    for (int l = 0; l < m->n_layers; ++l) {
      const size_t need = (size_t)std::max<int64_t>(n, 1) * m->features[l] * esize(m->dtype);
      if (bytes[l] < need) { if (acts[l]) hipFree(acts[l]); acts[l] = nullptr; HIPCHK(c, hbo_malloc(c, &acts[l], need)); bytes[l] = need; }
    }
    return HBO_OK;
  }
};

// ---- datasets ----------------------------------------------------------------------------
struct TaskHost {
  int64_t n = 0; int m = 0; int npad = 0, nblk = 0; int64_t ld = 0;
  bool owns_inputs = true;   // false: X / ysum / ydiv point into the dataset's single input block
  void* X = nullptr; void* ysum = nullptr;
  void* ydiv = nullptr;   // (m+1) x n rows for the divergence objectives: (y_a - mean_a y)/sqrt(m), then -mean_a y
  void* A = nullptr; void* W = nullptr; void* S = nullptr; void* wscr = nullptr; void* svec = nullptr; int svec_cols = 0; bool svec_shared = false;   // svec_shared: a slice of hbo_dataset::d_svec
  double* dmu = nullptr; double* fnorm = nullptr;
  double* dF = nullptr; double* dtmp = nullptr; size_t dF_elems = 0;   // MLP backward workspaces
  FeatBuf feat;
  void* KW = nullptr; size_t kw_bytes = 0;     // Kumaraswamy: w(X), the covariance's features
  double* KH = nullptr; size_t kh_bytes = 0;   // Kumaraswamy gradient: dw/da, dw/db (n x D doubles each)
};
// the shape of a task of n points and m target columns: padded to whole 128-blocks
static void task_shape(TaskHost* t, int64_t n, int m, int dtype) {
  t->n = n; t->m = m; t->npad = round_up(n, HBO_TILE); t->nblk = t->npad / HBO_TILE; t->ld = padded_ld(t->npad, dtype);
}
struct hbo_dataset {
  int dtype = 0, D = 0, ntasks = 0, max_nblk = 0;
  std::vector<TaskHost*> tasks;
  std::vector<TaskDesc> h_desc;
  TaskDesc* d_desc = nullptr;
  void* d_inputs = nullptr;   // x, column sums of y and divergence rows of every task (one upload)
  void* d_svec = nullptr;     // the tasks' alpha vectors in one block (one memset instead of one per task: a fresh batch of 64
                              // tasks per Adam step paid 64 fill kernels)
  // results of one evaluation, one device block = one copy back: [value T][gradient T x out_stride][info T (int)]
  double* d_pack = nullptr; size_t pack_bytes = 0;
  int* d_info = nullptr;
  double* d_nll = nullptr;
  std::vector<TaskDesc> h_desc_dev;   // what d_desc holds
  double* d_partials = nullptr; size_t partials_bytes = 0;
  double* d_gradout = nullptr;
  double* d_mlpgrad = nullptr; size_t mlpgrad_elems = 0;
  MlpTaskDev* d_mlp = nullptr; std::vector<MlpTaskDev> h_mlp_dev;   // per-task pointers of the batched MLP passes (what d_mlp holds)
  bool has_S = false;
};

static void free_task(hbo_ctx* c, TaskHost* t) {
  if (!t) return;
  if (t->owns_inputs) for (void* p : {t->X, t->ysum, t->ydiv}) dev_free(c, p);
  for (void* p : {t->A, t->W, t->S, t->wscr, t->svec_shared ? nullptr : t->svec, (void*)t->dmu, (void*)t->fnorm}) dev_free(c, p);
  for (void* p : {(void*)t->dF, (void*)t->dtmp, t->KW, (void*)t->KH}) dev_free(c, p);
  delete t;
}

static int ensure_task_workspace(hbo_ctx* c, int dtype, TaskHost* t, bool need_S, int naug_cols) {
  const size_t es = esize(dtype);
  const size_t ld = (size_t)t->ld;
  if (!t->A) HIPCHK(c, dev_alloc(c, &t->A, (size_t)(t->npad + HBO_TILE) * ld * es));
  if (!t->W) {   // a W that served the same shape before still has its zeros above the diagonal
    bool reused = false;
    HIPCHK(c, dev_alloc(c, &t->W, (size_t)t->npad * ld * es, dtype == HBO_F64 ? 2 : 1, &reused));
    if (!reused) HIPCHK(c, hipMemsetAsync(t->W, 0, (size_t)t->npad * ld * es, c->stream));
  }
  if (need_S && !t->S) HIPCHK(c, dev_alloc(c, &t->S, (size_t)t->npad * ld * es));
  if (!t->wscr) HIPCHK(c, dev_alloc(c, &t->wscr, (size_t)((t->npad + 511) / 512) * ld * es));
  if (t->svec_cols < naug_cols) {
    if (t->svec && !t->svec_shared) { HIPCHK(c, hipStreamSynchronize(c->stream)); dev_free(c, t->svec); }
    t->svec = nullptr; t->svec_shared = false;
    HIPCHK(c, dev_alloc(c, &t->svec, (size_t)t->npad * es * naug_cols));
    HIPCHK(c, hipMemsetAsync(t->svec, 0, (size_t)t->npad * es * naug_cols, c->stream));
    t->svec_cols = naug_cols;
  }
  if (!t->dmu) { HIPCHK(c, dev_alloc(c, (void**)&t->dmu, (size_t)t->npad * sizeof(double))); HIPCHK(c, dev_alloc(c, (void**)&t->fnorm, 2 * sizeof(double))); }
  return HBO_OK;
}

// role of the augmented rows (see TaskDesc): the three training objectives + the posterior cache
enum { ROLE_FACTOR = 100 };

static void fill_desc(TaskDesc& d, TaskHost* t, const hbo_model* m, int dtype, int role) {
  memset(&d, 0, sizeof d);
  d.A = t->A; d.W = t->W; d.S = t->S; d.wscr = t->wscr; d.X = t->X; d.ysum = t->ysum; d.svec = t->svec;
  d.dmu = t->dmu; d.fnorm = t->fnorm;
  const double mm = (double)t->m;
  switch (role) {
    case OBJ_NLL:   // objectives.py:144-156 incl. the (m,m)+scalar broadcast for m > 1
      d.naug = 1; d.e_last = -mm; d.coef_c = 0.5; d.coef_lh = 0.5 * mm * mm;
      d.coef_const = mm * mm * 0.5 * (double)t->n * log(2.0 * M_PI);
      break;
    case OBJ_EKL:   // utils.py:84-106 partial KL: tr(K1^-1 C0) + d^T K1^-1 d + logdet K1
      d.ysum = t->ydiv; d.naug = t->m + 1; d.e_last = 1.0; d.coef_c = 1.0; d.coef_lh = 1.0;
      break;
    case OBJ_EUC:   // utils.py:151-173 |mu0 - mu1| + |C0 - K1|_F  (no factorisation)
      d.ysum = t->ydiv; d.naug = t->m + 1; d.e_last = 1.0;
      break;
    default:        // posterior cache: rows y_a - mu
      d.naug = t->m; d.e_all = -1.0; d.coef_c = 0.5; d.coef_lh = 0.5;
      break;
  }
  d.last_src = d.naug - 1;
  if ((role == OBJ_EKL || role == OBJ_EUC) && t->m + 1 > HBO_TILE) { d.naug = 1; d.last_src = t->m; d.nvec = t->m + 1; }   // see TaskDesc::nvec
  d.n = (int)t->n; d.npad = t->npad; d.nblk = t->nblk; d.m = t->m; d.ld = t->ld;
  // (a task whose activations were never allocated -- hbo_nll_samples keeps its own -- gets null; the caller sets F / Fm)
  const void* last = (needs_mlp(m) && (int)t->feat.acts.size() >= m->n_layers) ? t->feat.acts[m->n_layers - 1] : nullptr;
  d.F = m->kernel_uses_mlp ? last : (is_kumar(m) ? t->KW : t->X);
  d.kh = is_kumar(m) ? t->KH : nullptr;
  d.fdim = feature_dim(m);
  d.fmean = mean_feature_dim(m);
  d.Fm = (m->mean_id == HBO_MEAN_LINEAR) ? t->X : (m->mean_id == HBO_MEAN_LINEAR_MLP ? last : nullptr);
  d.dF = t->dF;
  (void)dtype;
}

// Kumaraswamy buffers of a task: w(X) for `rows` rows, and (want_h) dw/da, dw/db for its n rows
static int ensure_kumar_buffers(hbo_ctx* c, const hbo_model* m, TaskHost* t, int64_t rows, bool want_h) {
  const size_t wb = (size_t)std::max<int64_t>(rows, 1) * m->input_dim * esize(m->dtype);
  if (t->kw_bytes < wb) { dev_free(c, t->KW); t->KW = nullptr; t->kw_bytes = 0; HIPCHK(c, dev_alloc(c, &t->KW, wb)); t->kw_bytes = wb; }
  const size_t hb = want_h ? (size_t)2 * std::max<int64_t>(t->n, 1) * m->input_dim * sizeof(double) : 0;
  if (t->kh_bytes < hb) { dev_free(c, t->KH); t->KH = nullptr; t->kh_bytes = 0; HIPCHK(c, dev_alloc(c, (void**)&t->KH, hb)); t->kh_bytes = hb; }
  return HBO_OK;
}

// ---- GPCache -----------------------------------------------------------------------------
struct hbo_cache {
  int dtype = 0, D = 0, m = 0;
  int input_warp = 0;      // the cached inputs were warped (hbo_model::input_warp of the factorising model): appends warp the new rows
  TaskHost* t = nullptr;
  TaskDesc h_desc; TaskDesc* d_desc = nullptr;
  int* d_info = nullptr; int info = INT_MAX;
  void* resid = nullptr;   // m x npad : y - mu
  void* zvec = nullptr;    // m x npad : z = L^-1 (y - mu), kept for O(N^2) row appends
  // fp32 caches: W = L^-1 split into three bf16 planes for the posterior product (post3.hip), built at the first use
  unsigned short* w3 = nullptr; size_t w3_elems = 0; bool w3_valid = false;
  int w3_planes = 0;                 // 3: bf16x3 planes, 2: fp16 planes scaled by the power of two behind *d_wmax (post3.hip)
  unsigned int* d_wmax = nullptr;    // device: bits of max |W|
};

// What hbo_acq_grad_samples and hbo_acq_maximize ask of their S (model, cache) pairs, before any device work: one model family
// (model_family_check) without MLP basis or linear_mlp mean, and finished caches of 1..max_n observations that match their models
// (HBO_TILE: the one-block entry points; INT_MAX: the _blocked ones).  *any_bad: a cache is not positive definite.
// allow_mlp (the _mlp entry points): the two MLP refusals are skipped, everything else stays.
// advice, advice_one: what the message of a refusal tells the caller to do instead, about the samples and about one sample (the qEI
// entry points, which have no other route, say so).
static int acq_samples_check(hbo_ctx* c, const std::string& fn, const hbo_model* models, int32_t S, hbo_cache* const* caches, int max_n, bool* any_bad,
                             bool allow_mlp, const char* advice = "evaluate the samples with hbo_acq_grad",
                             const char* advice_one = "evaluate it with hbo_acq_grad") {
  if (int rc = model_family_check(c, fn, models, S, advice)) return rc;
  for (int s = 0; s < S; ++s) {
    const hbo_model* m = &models[s];
    if (!allow_mlp && m->kernel_uses_mlp) return fail(c, HBO_ERR_UNSUPPORTED, fn + "a kernel on an MLP basis is not supported; " + advice);
    if (!allow_mlp && m->mean_id == HBO_MEAN_LINEAR_MLP) return fail(c, HBO_ERR_UNSUPPORTED, fn + "a linear_mlp mean is not supported; " + advice);
    const hbo_cache* k = caches[s];
    if (!k || !k->t || k->t->n <= 0) return fail(c, HBO_ERR_UNSUPPORTED, fn + "a sample without observations (the prior branch) is not supported; " + advice_one);
    if (k->t->n > max_n) return fail(c, HBO_ERR_UNSUPPORTED, fn + "a cache has n > " + std::to_string(max_n) + "; " + advice);
    if (k->dtype != m->dtype || k->D != m->input_dim) return fail(c, HBO_ERR_ARG, fn + "cache/model mismatch");
    if (k->input_warp != m->input_warp) return fail(c, HBO_ERR_ARG, fn + "the cache was factorised with another input warp");
    *any_bad = *any_bad || k->info != INT_MAX;
  }
  return HBO_OK;
}

// ---- which acquisition a call asks for, and by which route --------------------------------------
// AcqWhat: what the entry points over finished caches and posterior() (cache.hip) evaluate.  `step` is the scalar step of the kernels of
// acq_small.hip / acq_blocked.hip and the epilogue of posterior() (hbo_internal.h: ACQ_STEP_*); the other fields are the host arrays the
// step reads, per sample: REGISTRY -- acq_id and params [S]; MES -- ystar [S][K], the sampled maxima; LOGEI -- params [S], the targets.
struct AcqWhat {
  int step, acq_id;
  const double* params;
  const double* ystar; int32_t K;
  const double* given() const { return step == ACQ_STEP_MES ? ystar : params; }   // the array the caller must have passed
};
static AcqWhat acq_what_registry(int acq_id, const double* params) { return {ACQ_STEP_REGISTRY, acq_id, params, nullptr, 0}; }
static AcqWhat acq_what_mes(const double* ystar, int32_t K) { return {ACQ_STEP_MES, 0, nullptr, ystar, K}; }
static AcqWhat acq_what_logei(const double* targets) { return {ACQ_STEP_LOGEI, 0, targets, nullptr, 0}; }
// The request over `count` samples (given() is not null): acq_id in the registry; K in 1..HBO_MES_MAX_K and finite maxima; finite
// targets.  Touches no device (c may be null).
static int acq_what_check(hbo_ctx* c, const std::string& fn, const AcqWhat& w, int64_t count) {
  switch (w.step) {
    case ACQ_STEP_MES:
      if (w.K < 1 || w.K > HBO_MES_MAX_K) return fail(c, HBO_ERR_ARG, fn + "1 <= K <= " + std::to_string(HBO_MES_MAX_K));
      for (int64_t i = 0; i < count * w.K; ++i) if (!isfinite(w.ystar[i])) return fail(c, HBO_ERR_ARG, fn + "ystar holds a value that is not finite");
      return HBO_OK;
    case ACQ_STEP_LOGEI:
      for (int64_t i = 0; i < count; ++i) if (!isfinite(w.params[i])) return fail(c, HBO_ERR_ARG, fn + "targets holds a value that is not finite");
      return HBO_OK;
    default:
      return (w.acq_id < 0 || w.acq_id > HBO_ACQ_UCB) ? fail(c, HBO_ERR_ARG, fn + "bad acq_id") : HBO_OK;
  }
}
// AcqRoute: how an entry point runs the bodies acq_grad_samples (acq_grad.hip) and acq_maximize (acq_opt.hip).  An entry point copies
// one of the three constants and sets fn; the test hooks of include/hbo_tune.h also set force_blocked and chunk_queries.
struct AcqRoute {
  const char* fn;          // the entry point's name in messages
  int max_n;               // the largest cache the entry point takes (acq_samples_check)
  bool allow_mlp;          // MLP-basis kernels and linear_mlp means are served (acq_mlp.h)
  bool force_blocked;      // test hook: caches of n <= 128 through the blocked kernels too
  int64_t chunk_queries;   // test hook: > 0 overrides the chunk size
  AcqRoute named(const char* name) const { AcqRoute r = *this; r.fn = name; return r; }
  AcqRoute probed(const char* name, int32_t force, int64_t chunk) const { AcqRoute r = named(name); r.force_blocked = force != 0; r.chunk_queries = chunk; return r; }
};
constexpr AcqRoute ACQ_ROUTE_SMALL = {nullptr, HBO_TILE, false, false, 0};     // one 128-block per cache: one launch
constexpr AcqRoute ACQ_ROUTE_BLOCKED = {nullptr, INT_MAX, false, false, 0};    // caches of any size
constexpr AcqRoute ACQ_ROUTE_MLP = {nullptr, INT_MAX, true, false, 0};         // ... and MLP models
// what the hooks hbo_probe_*_grad_samples*64 ask of their own two arguments; `hook` names the hook in the message
static int acq_probe_check(hbo_ctx* c, const char* hook, const double* val64_out, int64_t chunk_queries) {
  if (!val64_out) return fail(c, HBO_ERR_ARG, std::string(hook) + ": val64_out is null");
  if (chunk_queries < 0) return fail(c, HBO_ERR_ARG, std::string(hook) + ": chunk_queries < 0");
  return HBO_OK;
}
int acq_grad_samples(hbo_ctx* c, const AcqRoute& route, const AcqWhat& what, const hbo_model* models, int32_t S, hbo_cache* const* caches,
                     const void* xq, int64_t M, const double* add_noise, double scale, void* acq_out, double* grad_out, double* val64_out);
int acq_maximize(hbo_ctx* c, const AcqRoute& route, const AcqWhat& what, const hbo_model* models, int32_t S, hbo_cache* const* caches,
                 const void* x0, int32_t R, const double* lo, const double* hi, const double* add_noise, double scale,
                 const hbo_acq_opt_opts* opts, double* state, int32_t evals, double* x_out, double* val_out, int32_t* status,
                 hbo_acq_opt_eval* log);
// hbo_predict / hbo_acq / hbo_acq_mes / hbo_acq_logei / one sample of hbo_acq_samples (cache.hip).  what: one sample's request (its
// params[0], its K maxima), read when acq_out or an override asks for the acquisition; the entry points check it (acq_what_check).
struct PosteriorOverride;
struct PostProbe;   // test hook hbo_probe_posterior (probe.hip): caller-chosen operands in place of the producer's launches; below, after PostPlan
int posterior(hbo_ctx* c, const hbo_model* m, hbo_cache* k, const void* xq, int64_t M, int full_cov, void* mu_out, void* var_out,
              void* acq_out, const AcqWhat& what, double add_noise, double scale, const PosteriorOverride* ov = nullptr,
              PostProbe* probe = nullptr);

// the records acq_small_kernel and the kernels of acq_blocked.hip read of those pairs (hbo_internal.h: AcqSmallSample) and their
// per-feature values, hv [S][fdim + mdim]: 1 / lengthscale over the kernel's own space, the linear mean's weights over the mean's
// (acq_vec_widths; without an MLP both are D: [S][2 D]) (params: null for the MES step, which reads none)
struct AcqVecWidths { int fdim, mdim; };
static AcqVecWidths acq_vec_widths(const hbo_model* m0) {
  return {feature_dim(m0), needs_mlp(m0) ? mean_feature_dim(m0) : m0->input_dim};
}
static void acq_small_pack(AcqSmallSample* hs, double* hv, const hbo_model* models, int32_t S, hbo_cache* const* caches, const double* params,
                           const double* add_noise) {
  const AcqVecWidths vw = acq_vec_widths(&models[0]);
  const size_t stride = (size_t)vw.fdim + vw.mdim;
  ModelDev md;
  for (int s = 0; s < S; ++s) {
    const hbo_cache* k = caches[s]; const TaskHost* t = k->t;
    fill_model_dev(md, &models[s]);
    AcqSmallSample& r = hs[s];
    memset(&r, 0, sizeof r);
    r.F = k->h_desc.F; r.W = t->W; r.alpha = t->svec; r.ld = t->ld; r.n = (int)t->n; r.bad = k->info != INT_MAX;
    r.sv = md.sv; r.inv_sigma2 = 1.0 / (md.dot_sigma * md.dot_sigma); r.bias2 = md.dot_bias * md.dot_bias;
    r.constant = md.constant; r.linear_bias = md.linear_bias; r.param = params ? params[s] : 0.0; r.add_noise = add_noise[s];
    memcpy(hv + (size_t)s * stride, md.inv_ls, sizeof(double) * vw.fdim);
    memcpy(hv + (size_t)s * stride + vw.fdim, md.lin_w, sizeof(double) * vw.mdim);
  }
}
// The MLP part of such a call's one staged upload (the _mlp entry points): the S weight sets as models_pack lays them out, then the
// tables of their device addresses [S][HBO_MAX_MLP_LAYERS], weights and biases.  bytes = 0 without an MLP: the upload is the
// _blocked entry point's, byte for byte.  acq_mlp_fill writes the host copy `h` for a block that sits at `d_base` (256-byte aligned)
// and points the kernels' arguments at it.
struct AcqMlpPack { MlpShape sh; size_t o_w, o_b, bytes; int ftot; };
static AcqMlpPack acq_mlp_layout(const hbo_model* m0, int S) {
  AcqMlpPack p = {};
  p.sh = mlp_shape(m0);
  if (!p.sh.L) return p;
  BlockLayout lay;
  lay.take(models_pack_bytes(p.sh, S));
  p.o_w = lay.take(sizeof(void*) * (size_t)S * HBO_MAX_MLP_LAYERS);
  p.o_b = lay.take(sizeof(void*) * (size_t)S * HBO_MAX_MLP_LAYERS);
  p.bytes = lay.off;
  for (int l = 0; l < p.sh.L; ++l) p.ftot += p.sh.fout[l];
  return p;
}
static void acq_mlp_fill(const AcqMlpPack& p, char* h, char* d_base, const hbo_model* models, int S, AcqSmallArgs& a) {
  const hbo_model* m0 = &models[0];
  const AcqVecWidths vw = acq_vec_widths(m0);
  a.fdim = vw.fdim; a.mdim = vw.mdim;
  if (!p.sh.L) return;
  memset(h, 0, p.bytes);
  models_pack(h, d_base, models, S, p.sh, reinterpret_cast<void**>(h + p.o_w), reinterpret_cast<void**>(h + p.o_b));
  a.feat = (m0->kernel_uses_mlp ? 1 : 0) | (m0->mean_id == HBO_MEAN_LINEAR_MLP ? 2 : 0);   // acq_mlp.h: ACQ_FEAT_KERNEL, ACQ_FEAT_MEAN
  a.L = p.sh.L;
  for (int l = 0; l < p.sh.L; ++l) a.fout[l] = p.sh.fout[l];
  a.mlp_w = reinterpret_cast<const void* const*>(d_base + p.o_w); a.mlp_b = reinterpret_cast<const void* const*>(d_base + p.o_b);
}

// ldv of the blocked kernels' workspace (acq_blocked.hip): the largest n of the caches rounded up to the 128-row block
static int acq_blocked_ldv(int32_t S, hbo_cache* const* caches) {
  int64_t n = 1;
  for (int s = 0; s < S; ++s) n = std::max<int64_t>(n, caches[s]->t->n);
  return round_up(n, HBO_TILE);
}

// ---- sample paths (paths.hip), shared with the path maximiser (path_opt.hip) ------------------
// path_check: what both ask of (model, cache, S, F, eps) before any device call.  path_solve: the draws on the device and the weights
// v of the update term over the cache's observations, with `scale` on the amplitude and the noise draw.
struct PathSolve {
  const void* om; const void* ph; const void* w;   // the draws on the device, model dtype (om / ph empty for the dot product)
  double* sums;                                    // [rows][S] prior sums: scratch of the prior kernel
  double* v; int64_t vld;                          // [S][vld] weights (null without a cache)
  double A;                                        // the amplitude sqrt(2 signal_variance / F) (1 for the dot product), without `scale`
};
int path_check(hbo_ctx* c, const std::string& fn, const hbo_model* m, const hbo_cache* k, int32_t S, int32_t F, bool has_eps);
int path_solve(hbo_ctx* c, const hbo_model* m, hbo_cache* k, int32_t S, int32_t F, const void* omega, const void* phase, const void* w,
               const void* eps, double scale, int64_t sum_rows, PathSolve* ps);

static void fill_nan(void* p, size_t count, int dtype) {
  if (dtype == HBO_F64) for (size_t i = 0; i < count; ++i) ((double*)p)[i] = NAN;
  else for (size_t i = 0; i < count; ++i) ((float*)p)[i] = NAN;
}
// Host arrays are [n][m] (column a of row i at i * m + a); the device keeps them as m rows of npad (at a * npad + i).  Both directions
// copy the n x m elements and nothing else: what `dst` holds beyond them (the rows' padding) stays as it was.
static void cols_to_rows(void* dst, const void* src, int64_t n, int m, int64_t npad, size_t es) {
  for (int64_t i = 0; i < n; ++i) for (int a = 0; a < m; ++a) memcpy((unsigned char*)dst + ((size_t)a * npad + i) * es, (const unsigned char*)src + ((size_t)i * m + a) * es, es);
}
static void rows_to_cols(void* dst, const void* src, int64_t n, int m, int64_t npad, size_t es) {
  for (int64_t i = 0; i < n; ++i) for (int a = 0; a < m; ++a) memcpy((unsigned char*)dst + ((size_t)i * m + a) * es, (const unsigned char*)src + ((size_t)a * npad + i) * es, es);
}
// the three launches of the fp32 posterior product on the 16-bit matrix cores (cache.hip), which hbo_probe_post_product runs too
void post3_split_w(const float* W, int64_t ld, int nblk, bool h2, unsigned short* w3, unsigned int* d_wmax, hipStream_t st);
void post3_split_kxq(const float* K, int64_t ldq, int mpad, int npad, bool h2, float kscale, unsigned short* K3, hipStream_t st);
bool post3_product(const unsigned short* w3, const unsigned short* K3, int nblk, int mpad, bool h2, const unsigned int* d_wmax, float kscale, float* colsq, int64_t ldc, int* counter, hipStream_t st);

// ---- posterior plan ------------------------------------------------------------------------
// Every decision of one posterior / acquisition call (cache.hip: posterior), from sizes and options alone: no HIP call, no allocation.
// nblk: 128-blocks of the cache (0: prior branch).  ov_lane: null for a call of its own, else the lane of the override (hbo_acq_samples).
// deny: forms the caller could not get the memory for -- the plan without them.
enum { POST_NO_SPLITK = 1, POST_NO_SPLIT3 = 2 };
struct PostChunk {
  int64_t q0, mc; int b;       // first query, queries, workspace
  int mpad; int64_t ldq;       // the chunk's padded candidates and their leading dimension
  int counter;                 // the product as a resident grid drawing its tiles from this word of the tile-counter array (-1: plain grid)
};
struct PostPlan {
  int refuse;                  // not 0: the call is not run (HBO_ERR_UNSUPPORTED: full_cov beyond 65536 queries)
  int dtype, nblk; bool full_cov;
  int64_t M, CH, mc_max, nchunks; int nbuf;   // chunks of CH queries through nbuf alternating workspaces
  int mpad_max; int64_t ldq_max;
  int lane, wso;               // side-stream lane of an override's single-chunk pass; its workspace-slot offset
  hipStream_t sa, sb;          // consumer (products, epilogue, copy back) and producer (features, cross Gram) streams
  int kchunk, nch;             // split-K product: 128-blocks per K chunk (0: not split) and the chunks of the longest row
  Fp32Form form; int planes; float kscale;   // the product's fp32 form (FORM_MFMA: also all of fp64), planes of its split operands, scale of Kxq's
  bool direct_form;            // the producer's cross Gram in the direct form
  bool own_counters; int n_cus;
  // One rule for both products: a resident grid with a tile counter for calls of their own, with lauum_persist on, beyond `min_tiles` tiles
  // (one counter per chunk in flight)
  bool resident(int64_t tiles, int64_t min_tiles) const { return own_counters && tiles > min_tiles; }
  PostChunk chunk(int64_t i) const {
    PostChunk ch;
    ch.q0 = i * CH; ch.mc = std::min<int64_t>(CH, M - ch.q0); ch.b = (int)(i % nbuf);
    ch.mpad = round_up(ch.mc, HBO_TILE); ch.ldq = padded_ld(ch.mpad, dtype);
    const int64_t tiles = (int64_t)(ch.mpad / HBO_TILE) * nblk;
    // the bf16 / fp16 form hands launch_post3 a counter whatever the size (it decides); launch_gemm's takes one for the large products
    const bool res = nblk && kchunk == 0 && resident(tiles, form != FORM_MFMA ? 0 : 4 * (int64_t)n_cus);
    ch.counter = res ? HBO_N_COUNTERS - 8 + (ch.b & 1) : -1;
    return ch;
  }
};
static PostPlan post_plan(const hbo_ctx* c, const hbo_model* m, int64_t M, int nblk, bool full_cov, const int* ov_lane, int deny = 0) {
  PostPlan p = {};
  p.dtype = m->dtype; p.nblk = nblk; p.full_cov = full_cov; p.M = M; p.n_cus = c->n_cus;
  // Candidates are STREAMED: chunks of `CH` queries, so that the cross-Gram workspace (npad x CH) does not grow with M
  // (gp.py:295-305 materialises all of Kxq; at cfg 3 that is 16384 x 65536 fp32 = 4.3 GB).  Two workspaces alternate:
  // upload + features + cross Gram of chunk i+1 run on a second stream beside the triangular product of chunk i; the
  // results of all chunks are gathered in M-sized vectors and come back in one copy.  full_cov keeps a single pass.
  p.CH = full_cov ? 65536 : std::max<int64_t>(c->opt_post_chunk, HBO_TILE);
  if (full_cov && M > p.CH) p.refuse = HBO_ERR_UNSUPPORTED;
  p.mc_max = std::min<int64_t>(M, p.CH);
  p.nchunks = (M + p.CH - 1) / p.CH;
  p.nbuf = (!full_cov && M > p.CH) ? 2 : 1;
  p.mpad_max = round_up(p.mc_max, HBO_TILE);
  p.ldq_max = padded_ld(p.mpad_max, p.dtype);
  p.lane = (ov_lane && p.nbuf == 1) ? *ov_lane : 0;
  p.wso = 4096 * p.lane;   // workspace slots of this lane
  p.sa = p.lane == 1 ? c->stream2 : (p.lane == 2 ? c->stream4 : c->stream);
  p.sb = (p.nbuf == 2 && !c->opt_post_serial) ? c->stream2 : p.sa;
  // Few candidates (a BO step asks for tens of them): one workgroup per 128-row tile of W would walk a K range of up to N alone
  // (N = 8192, 64 queries: 1.1 ms for 8.6 GFLOP); the K range is cut into chunks of `kchunk` blocks instead, one workgroup per
  // (row tile, chunk), partial products to a workspace, summed and squared by a second small kernel (0.1-0.2 ms).
  // (decided on the TOTAL number of candidates, not on the chunk: every post_chunk then gives the same bits)
  if (nblk && !(deny & POST_NO_SPLITK) && !full_cov && nblk >= 2 && (int64_t)((M + HBO_TILE - 1) / HBO_TILE) * nblk < 2 * c->n_cus) {
    p.kchunk = std::max(2, std::min(8, nblk / 8));   // N = 8100: 1 / 2 / 4 / 8 / 16 blocks per chunk: 0.81 / 0.48 / 0.35 / 0.35 / 0.35 ms; N = 2000: 2 / 4 / 8: 0.11 / 0.11 / 0.17
    // (below 8 blocks one block per chunk: the lone 128-tile of the last row block of an N = 512 cache ran its K = 512 alone on a
    //  CU for 75 us -- an HGP acquisition over 32 samples spent half its time there)
    if (nblk < 8) p.kchunk = 1;
    p.nch = (nblk + p.kchunk - 1) / p.kchunk;
  }
  // fp32: the product runs on the bf16 matrix cores from exact three-way splits of both operands (post3.hip)
  const bool use3 = nblk && !(deny & POST_NO_SPLIT3) && p.dtype == HBO_F32 && c->opt_post_bf16x3 && !full_cov && p.kchunk == 0;
  // stationary covariances (|k| <= signal variance: the cross Gram's scale is known without a pass over it): two-way fp16 split,
  // three MFMAs per product instead of six (post3.hip, H2)
  const bool use2h = use3 && c->opt_post_f16x2 && m->kernel_id != HBO_KERNEL_DOT;
  p.form = use2h ? FORM_F16X2 : (use3 ? FORM_BF16X3 : FORM_MFMA);
  p.planes = use2h ? 2 : 3;
  p.kscale = use2h ? post2h_scale_for(m->signal_variance) : 1.f;
  // the producer of a streamed posterior runs BESIDE the product of the previous chunk, in the slots its resident grid leaves: there the
  // matrix-core form (38 KB of LDS per workgroup, the product's own MFMA pipes) is the slower one -- cfg 3: EI 58.5 ms with the direct
  // form, 59.0 with it, although alone it takes 0.33 ms per chunk against 0.58 (round 6)
  p.direct_form = p.nbuf == 2;
  p.own_counters = c->opt_lauum_persist && !ov_lane;
  return p;
}
// hbo_probe_posterior (probe.hip): the one step of posterior() a test swaps.  With a PostProbe, produce_chunk copies columns
// [q0, q0 + mc) of these device operands into the chunk's slices (on the producer stream, the padding zeroed as the padded Gram leaves
// it) instead of running query_features and the cross Gram; everything else of the call is untouched.  Kxq [n, M] dense, kdiag, mu0 [M].
// Out: the plan as it ran (after post_acquire) and the chunks whose product ran as a resident grid.
struct PostProbe {
  const void *Kxq, *kdiag, *mu0;
  PostPlan plan; int resident_chunks;
};

// ---- objective plan ------------------------------------------------------------------------
// Every decision of one hbo_objective evaluation (objective.hip: objective_local) that follows from the options, the model, the
// dataset's shape (tasks, blocks, dtype, each task's n and m), the objective, want_grad and whether the call is sharded: no HIP call,
// no allocation.  What needs the filled descriptors (the largest naug) is obj_setup's.  ds may be null or empty (a rank beyond the
// task count): such a call only reads red_count.
struct ObjPlan {
  int obj, dtype, T, max_nblk, max_npad; bool want_grad, sharded;
  bool euc, kumar, mlp, extras;
  bool small_ok, fused_small, lds_only;
  bool need_S;                 // the tasks' workspaces include S (K^-1, or the sweep's running matrix)
  bool la; InvPlan inv;        // look-ahead; the route and placement of the inverse (sched.h: inv_plan)
  bool side_reduce;            // the small reductions on the idle panel stream
  bool value_inverse;          // a value-only call that needs the inverse for its extra rows
  bool contract;               // the gradient contraction runs (EUC: its value comes out of it too)
  int64_t max_n; int fdim, nacc, out_stride; size_t pack_bytes;
  int64_t stride_task; size_t partials_bytes;
  int red_count;               // sharded: [nll, count, grad] of the whole job, reduced on the device
};
static ObjPlan obj_plan(const hbo_ctx* c, const hbo_model* m, const hbo_dataset* ds, const hbo_grad_layout& lay, int obj, bool want_grad, bool sharded) {
  ObjPlan p = {};
  p.obj = obj; p.want_grad = want_grad; p.sharded = sharded;
  p.T = ds ? ds->ntasks : 0; p.dtype = ds ? ds->dtype : m->dtype; p.max_nblk = ds ? ds->max_nblk : 0; p.max_npad = p.max_nblk * HBO_TILE;
  p.euc = obj == OBJ_EUC; p.kumar = is_kumar(m); p.mlp = needs_mlp(m);
  p.red_count = 2 + (want_grad ? lay.total : 0);
  // tasks with more than 127 aligned columns: their data rows do not ride in the augmented tile-row (TaskDesc::nvec)
  if (obj != OBJ_NLL) for (int k = 0; k < p.T; ++k) if (ds->tasks[k]->m + 1 > HBO_TILE) p.extras = true;
  for (int k = 0; k < p.T; ++k) p.max_n = std::max<int64_t>(p.max_n, ds->tasks[k]->n);
  // (the single-workgroup evaluation needs 132 KB (fp64) / 68 KB (fp32) of LDS in one workgroup: a device that cannot give it -- any
  //  ARCH other than gfx950 the Makefile is pointed at -- takes the blocked pipeline instead of failing at launch)
  p.small_ok = c->opt_small_fused && ds && small_eval_lds(p.dtype) <= c->lds_per_block;
  // every task fits one 128-block (the reference's training regime: sub-sampled tasks of 50-100 points): ONE launch, one workgroup
  // per task does Gram -> factorisation -> inverse -> K^-1 -> contraction in LDS (small.hip) instead of the 13 launches of the blocked
  // pipeline
  // (a batch that takes the single-workgroup evaluation sets its info words itself: one launch less on a 60 us path)
  p.fused_small = obj == OBJ_NLL && p.max_nblk == 1 && p.small_ok;
  // A batch that takes the single-workgroup evaluation (small.hip) without an MLP keeps its matrices in
  // LDS: no A / W / S / alpha buffers at all (a freshly sub-sampled batch per Adam step paid ~150 pool operations and two fills for
  // buffers its one launch never reads); the leaf inverses that leaf_cholesky4 also stores go to one shared scratch block
  p.lds_only = p.fused_small && !p.mlp && !(p.kumar && want_grad);
  // (a batch with extra rows runs the inverse over ALL its tasks, value-only calls too: GEMM_TRTRI_A stores S21 of every task with
  //  two or more blocks, so every task of such a batch needs S -- not only the ones with more than 127 aligned columns)
  p.need_S = (want_grad || p.extras) && !p.euc;
  p.la = use_lookahead(c, p.T, p.max_nblk);
  // the inverse and K^-1 behind the panel chain, row group by row group (sched.hip:sweep_advance) -- or the block-recursive
  // inverse started beside the chain and K^-1 = W^T W after it (a gradient); or W alone behind the factorisation (a value with extra rows)
  p.value_inverse = p.extras && !p.euc && !want_grad;   // value only: the inverse is needed for the extra rows all the same
  p.inv = inv_plan(c, p.dtype, p.T, p.max_nblk, (want_grad && !p.euc) ? INV_W_KINV : ((want_grad || p.value_inverse) ? INV_W : INV_NONE), p.T == 1, want_grad);
  // the small reductions (log-determinant + quadratic form now, alpha = W^T z and d nll / d mu after the inverse) run on
  // the idle panel stream beside the inverse and K^-1 = W^T W instead of between them (0.14 ms at cfg 2)
  p.side_reduce = want_grad && obj == OBJ_NLL && p.la;
  p.contract = !p.fused_small && (want_grad || p.euc);   // EUC: the Frobenius norm of the value comes out of the contraction pass
  p.fdim = feature_dim(m);
  p.nacc = grad_nacc(m->kernel_id, p.fdim);
  p.stride_task = (int64_t)(p.max_nblk * (p.max_nblk + 1)) * p.nacc;   // two half-tile slots per lower tile
  p.partials_bytes = !p.contract ? 0 : sizeof(double) * (p.stride_task * p.T + (size_t)HBO_GRAD_PRE_ROWS * p.nacc * p.T);   // per-tile partials + their pre-reduction
  // results of one evaluation, one device block = one copy back: [value T][gradient T x out_stride][info T (int)]
  p.out_stride = (m->kernel_id == HBO_KERNEL_DOT ? 0 : m->n_lengthscale) + 6 + mean_feature_dim(m);
  p.pack_bytes = sizeof(double) * p.T * (1 + (size_t)p.out_stride) + sizeof(int) * p.T;
  return p;
}

// ---- gradient scatter table ------------------------------------------------------------------
// Where an evaluation's gradient goes in the caller's layout (hbo_grad_layout): entry j of a task's gradient block (out_stride
// entries: lengthscales, signal and noise variance, constant, dot-product sigma and bias, linear-mean weights and bias) is ADDED to
// leaf map[j] (-1: the model has no such leaf); the leaves that come out already summed over the tasks -- the 2 D Kumaraswamy sums and
// the MLP gradient, both in hbo_dataset::d_mlpgrad -- are ASSIGNED by segments (destination, source position, length).  Built once per
// call; the sharded path uploads `w` as it stands ([out_stride ints][3 ints per segment]: what shard_reduce_kernel reads) and the host
// finish walks the same words (grad_scatter_host).  Sized for the worst case a valid model has, so nothing here can overflow:
// two Kumaraswamy segments beside a linear_mlp mean of HBO_MAX_MLP_LAYERS layers.
enum { HBO_SCATTER_MAX_SEG = 2 + 2 * HBO_MAX_MLP_LAYERS, HBO_SCATTER_MAX_STRIDE = 2 * HBO_MAX_FEATURE_DIM + 6 };
struct GradScatter {
  int out_stride, nseg;
  int w[HBO_SCATTER_MAX_STRIDE + 3 * HBO_SCATTER_MAX_SEG];
  const int* seg() const { return w + out_stride; }
  size_t bytes() const { return sizeof(int) * (out_stride + 3 * HBO_SCATTER_MAX_SEG); }
};
// kumar_a / kumar_b: hbo_grad_layout_kumar_of's offsets.  Without want_grad: every entry -1, no segment.
static void grad_scatter_fill(GradScatter& g, const hbo_model* m, const hbo_grad_layout& lay, int32_t kumar_a, int32_t kumar_b, int out_stride, bool want_grad) {
  g.out_stride = out_stride; g.nseg = 0;
  for (int i = 0; i < out_stride + 3 * HBO_SCATTER_MAX_SEG; ++i) g.w[i] = -1;
  if (!want_grad) return;
  const int n_ls = m->kernel_id == HBO_KERNEL_DOT ? 0 : m->n_lengthscale;
  const int fm = mean_feature_dim(m);
  for (int d = 0; d < n_ls; ++d) g.w[d] = lay.lengthscale < 0 ? -1 : lay.lengthscale + d;
  g.w[n_ls] = lay.signal_variance; g.w[n_ls + 1] = lay.noise_variance; g.w[n_ls + 2] = lay.constant;
  g.w[n_ls + 3] = lay.dot_prod_sigma; g.w[n_ls + 4] = lay.dot_prod_bias;
  for (int d = 0; d < fm; ++d) g.w[n_ls + 5 + d] = lay.linear_kernel < 0 ? -1 : lay.linear_kernel + d;
  g.w[n_ls + 5 + fm] = lay.linear_bias;
  auto segment = [&](int dst, int src, int len) { int* sg = g.w + out_stride + 3 * g.nseg++; sg[0] = dst; sg[1] = src; sg[2] = len; };
  if (is_kumar(m)) {   // the 2 D Kumaraswamy leaves, already summed over the tasks
    segment(kumar_a, 0, m->input_dim); segment(kumar_b, m->input_dim, m->input_dim);
  }
  if (needs_mlp(m)) {   // the MLP gradient, already summed over the tasks: per layer the weights, then the bias
    int pos = 0, fin0 = m->input_dim;
    for (int l = 0; l < m->n_layers; ++l) {
      const int wn = fin0 * m->features[l], bn = m->features[l];
      segment(lay.mlp_kernel[l], pos, wn); pos += wn;
      segment(lay.mlp_bias[l], pos, bn); pos += bn;
      fin0 = m->features[l];
    }
  }
}
// The host finish over the table: h_grad [T][out_stride] and h_info [T] as they come back from the device, h_seg the summed leaves
// (may be null without segments).  Per-task entries are added, NaN for a task whose info word is set; segments are assigned, NaN
// when any task failed (notpd).
static void grad_scatter_host(const GradScatter& g, int T, const double* h_grad, const int* h_info, const double* h_seg, bool notpd, double* grad_sum) {
  for (int k = 0; k < T; ++k) {
    const double* o = h_grad + (size_t)k * g.out_stride;
    const bool bad = h_info[k] != INT_MAX;
    for (int j = 0; j < g.out_stride; ++j) if (g.w[j] >= 0) grad_sum[g.w[j]] += bad ? NAN : o[j];
  }
  for (int s = 0; s < g.nseg; ++s) {
    const int* sg = g.seg() + 3 * s;
    for (int i = 0; i < sg[2]; ++i) grad_sum[sg[0] + i] = notpd ? NAN : h_seg[sg[1] + i];
  }
}
