// hbo_train_adam: K Adam steps of infer_parameters(method='adam') (hyperbo/gp_utils/gp.py:53-195) queued on the device for a batch
// whose tasks all fit one 128-block.  Per step: [gather the step's rows in place] -> single-workgroup evaluation and its backward
// passes (objective.hip: enqueue_fused_forward / enqueue_backward) -> launch_shard_reduce ([nll_sum, T, grad] in the caller's
// layout) -> adam_step_kernel.  No host wait between steps: one copy back and one synchronisation per call.
//
// hbo_train_lbfgs: the evaluations of infer_parameters(method='lbfgs') (basics/lbfgs.py) queued the same way on one resident batch:
// evaluation -> launch_shard_reduce -> lbfgs_ctl_kernel, which runs the state machine of lbfgs_ctl.h on [nll_sum / T, grad / T]
// chained through the warps and writes the model of the next point.  Both step kernels share the chain rule, the leaf -> model field
// staging and the host-side leaf checks and packing below.
#include "api_internal.h"
#define HBO_LBFGS_FN static __host__ __device__ inline
#include "lbfgs_ctl.h"

#include <numeric>

// gp.py:_Adam.step and the warps are restated operation by operation: no fused multiply-adds anywhere in this file
#pragma clang fp contract(off)

namespace {

constexpr int ADAM_THREADS = 256;

// numpy's npy_logaddexp(x, 0) (utils.py softplus_warp = logaddexp(x, 0))
__device__ double logaddexp0(double x) {
  if (x == 0.0) return x + 0.693147180559945309417232121458176568;
  const double tmp = x - 0.0;
  if (tmp > 0) return x + log1p(exp(-tmp));
  if (tmp <= 0) return 0.0 + log1p(exp(tmp));
  return tmp;   // NaN
}
__device__ double warp_value(int w, double x) {
  switch (w) {
    case HBO_TRAIN_WARP_SOFTPLUS: return logaddexp0(x);
    case HBO_TRAIN_WARP_SOFTPLUS_EPS: return logaddexp0(x) + 1e-10;   // utils.DEFAULT_SOFTPLUS
    case HBO_TRAIN_WARP_SQUAREPLUS: return 0.5 * (x + sqrt(x * x + 4.0));
    default: return x;
  }
}
// utils.warp_derivative
__device__ double warp_slope(int w, double x) {
  switch (w) {
    case HBO_TRAIN_WARP_SOFTPLUS: case HBO_TRAIN_WARP_SOFTPLUS_EPS: return 1.0 / (1.0 + exp(-x));
    case HBO_TRAIN_WARP_SQUAREPLUS: return 0.5 * (1.0 + x / sqrt(x * x + 4.0));
    default: return 1.0;
  }
}
__device__ void put_elem(void* p, int dtype, int i, double v) {
  if (dtype == HBO_F64) static_cast<double*>(p)[i] = v;
  else static_cast<float*>(p)[i] = (float)v;
}

// What both step kernels read: the leaf map, where each leaf's gradient sits in the reduction, the starting model (its array pointers
// point at device copies in the model dtype) and where the next model goes.
struct TrainDev {
  const hbo_train_leaf* leaves; const int* goff; int P;
  const double* red;                 // [nll_sum, T, grad sum in the caller's layout]
  hbo_model_kumar init;
  int n_ls, fm;
  void* mlp_w[HBO_MAX_MLP_LAYERS]; void* mlp_b[HBO_MAX_MLP_LAYERS];
  ModelDev* md;
};
// the warped fields of the next model while its leaves are written (arrays in the model dtype)
struct ModelStage {
  double ls[HBO_MAX_FEATURE_DIM], lin[HBO_MAX_FEATURE_DIM], ka[HBO_MAX_FEATURE_DIM], kb[HBO_MAX_FEATURE_DIM];
  double sc[6];   // signal variance, noise variance, constant, dot sigma, dot bias, linear bias
};
// the starting model's fields into the stage (fields no leaf targets keep them); ends with a barrier
__device__ void stage_load(const TrainDev& t, ModelStage& s, int tid, int nthr) {
  const hbo_model& m0 = t.init.base;
  const int dtype = m0.dtype, D = m0.input_dim;
  for (int d = tid; d < HBO_MAX_FEATURE_DIM; d += nthr) {
    if (d < t.n_ls) put_elem(s.ls, dtype, d, model_elem(m0.lengthscale, dtype, d));
    if (d < t.fm) put_elem(s.lin, dtype, d, model_elem(m0.linear_kernel, dtype, d));
    if (m0.input_warp == HBO_WARP_KUMAR && d < D) {
      put_elem(s.ka, dtype, d, model_elem(t.init.kumar_a, dtype, d));
      put_elem(s.kb, dtype, d, model_elem(t.init.kumar_b, dtype, d));
    }
  }
  if (tid == 0) {
    s.sc[0] = m0.signal_variance; s.sc[1] = m0.noise_variance; s.sc[2] = m0.constant;
    s.sc[3] = m0.dot_prod_sigma; s.sc[4] = m0.dot_prod_bias; s.sc[5] = m0.linear_bias;
  }
  __syncthreads();
}
// d loss / d x[i] from the reduction: grad / count, then d warp / d raw (_model.BuiltModel.unflatten_grad; a leaf the model does not
// read has gradient zero)
__device__ double chained_grad(const TrainDev& t, const hbo_train_leaf& lf, int i, double x, double count) {
  const double xr = lf.round_f32 ? (double)(float)x : x;
  double g = 0.0;
  if (t.goff[i] >= 0) g = (t.red[2 + t.goff[i]] / count) * warp_slope(lf.warp, xr);
  return g;
}
// leaf value x -> its warped field of the next model
__device__ void stage_put(const TrainDev& t, ModelStage& s, const hbo_train_leaf& lf, double x) {
  const int dtype = t.init.base.dtype;
  const double xr = lf.round_f32 ? (double)(float)x : x;
  double w = warp_value(lf.warp, xr);
  if (lf.round_f32) w = (double)(float)w;
  switch (lf.target) {
    case HBO_TRAIN_LENGTHSCALE: put_elem(s.ls, dtype, lf.index, w); break;
    case HBO_TRAIN_SIGNAL_VARIANCE: s.sc[0] = w; break;
    case HBO_TRAIN_NOISE_VARIANCE: s.sc[1] = w; break;
    case HBO_TRAIN_CONSTANT: s.sc[2] = w; break;
    case HBO_TRAIN_DOT_PROD_SIGMA: s.sc[3] = w; break;
    case HBO_TRAIN_DOT_PROD_BIAS: s.sc[4] = w; break;
    case HBO_TRAIN_LINEAR_BIAS: s.sc[5] = w; break;
    case HBO_TRAIN_LINEAR_KERNEL: put_elem(s.lin, dtype, lf.index, w); break;
    case HBO_TRAIN_MLP_KERNEL: put_elem(t.mlp_w[lf.layer], dtype, lf.index, w); break;
    case HBO_TRAIN_MLP_BIAS: put_elem(t.mlp_b[lf.layer], dtype, lf.index, w); break;
    case HBO_TRAIN_KUMAR_A: put_elem(s.ka, dtype, lf.index, w); break;
    case HBO_TRAIN_KUMAR_B: put_elem(s.kb, dtype, lf.index, w); break;
    default: break;
  }
}
// the staged model into ModelDev (the MLP weights went to their buffers leaf by leaf); begins with a barrier
__device__ void stage_store(const TrainDev& t, ModelStage& s, int tid, int nthr) {
  __syncthreads();
  hbo_model_kumar mk = t.init;
  mk.base.signal_variance = s.sc[0]; mk.base.noise_variance = s.sc[1]; mk.base.constant = s.sc[2];
  mk.base.dot_prod_sigma = s.sc[3]; mk.base.dot_prod_bias = s.sc[4]; mk.base.linear_bias = s.sc[5];
  mk.base.lengthscale = s.ls; mk.base.linear_kernel = s.lin; mk.kumar_a = s.ka; mk.kumar_b = s.kb;
  model_dev_fill(*t.md, &mk.base, tid, nthr);
}

struct AdamStepArgs {
  TrainDev t;
  double* x; double* am; double* av;
  const double* bias1; const double* bias2;
  double lr, b1, b2, eps;
  double* losses; double* trace;     // trace nullable
  int* halt; int* steps_done;
};

// One step: loss check (gp.py:135-142), warp chain rule, Adam (gp.py:_Adam.step), then the warped next model into ModelDev and the
// MLP weight buffers.  A non-finite loss sets the halt word: every later step returns here.
__global__ __launch_bounds__(ADAM_THREADS) void adam_step_kernel(AdamStepArgs a, int step) {
  __shared__ ModelStage s;
  __shared__ int s_halt;
  const int tid = threadIdx.x, nthr = blockDim.x;
  if (tid == 0) s_halt = *a.halt;
  __syncthreads();
  if (s_halt) return;
  const double count = a.t.red[1];
  const double loss = a.t.red[0] / count;
  if (tid == 0) a.losses[step] = loss;
  if (!isfinite(loss)) {
    if (tid == 0) { *a.halt = 1; *a.steps_done = step; }
    return;
  }
  stage_load(a.t, s, tid, nthr);
  const double b1 = a.b1, b2 = a.b2, c1 = 1 - b1, c2 = 1 - b2;
  const double bias1 = a.bias1[step], bias2 = a.bias2[step];
  for (int i = tid; i < a.t.P; i += nthr) {
    const hbo_train_leaf lf = a.t.leaves[i];
    const double x = a.x[i];
    if (a.trace) a.trace[(size_t)step * a.t.P + i] = x;
    const double g = chained_grad(a.t, lf, i, x, count);
    const double m = b1 * a.am[i] + c1 * g;
    const double v = b2 * a.av[i] + c2 * g * g;
    const double mhat = m / bias1;
    const double vhat = v / bias2;
    const double xn = x - a.lr * mhat / (sqrt(vhat) + a.eps);
    a.am[i] = m; a.av[i] = v; a.x[i] = xn;
    stage_put(a.t, s, lf, xn);
  }
  stage_store(a.t, s, tid, nthr);
}

// ---- L-BFGS ----------------------------------------------------------------------------------------------------------------
static_assert(sizeof(hbo_lbfgs_opts) == sizeof(hbo_lbfgs_opts_ctl) && sizeof(hbo_lbfgs_eval) == sizeof(hbo_lbfgs_eval_ctl), "lbfgs_ctl.h restates hbo.h");
static_assert(HBO_LBFGS_START == HBO_LBFGS_CTL_START && HBO_LBFGS_MAIN == HBO_LBFGS_CTL_MAIN && HBO_LBFGS_LINE_SEARCH == HBO_LBFGS_CTL_LINE_SEARCH &&
              HBO_LBFGS_IDLE == HBO_LBFGS_CTL_IDLE && HBO_LBFGS_STEPS_DONE == HBO_LBFGS_CTL_STEPS_DONE, "lbfgs_ctl.h restates hbo.h");

struct LbfgsArgs {
  TrainDev t;
  hbo_lbfgs_opts_ctl o;
  double* state;
  hbo_lbfgs_eval_ctl* log;
  double* trace;   // nullable
};

// the model of the point the state wants evaluated next
__device__ void lbfgs_write_model(const LbfgsArgs& a, ModelStage& s, int tid, int nthr) {
  const hbo_lbfgs_view v = hbo_lbfgs_view_of(a.state, a.t.P, a.o.memory);
  stage_load(a.t, s, tid, nthr);
  for (int i = tid; i < a.t.P; i += nthr) stage_put(a.t, s, a.t.leaves[i], v.xt[i]);
  stage_store(a.t, s, tid, nthr);
}
// a call that continues a run: the model of the pending point with the device's warps, as every other evaluation of the run got it
__global__ __launch_bounds__(ADAM_THREADS) void lbfgs_model_kernel(LbfgsArgs a) {
  __shared__ ModelStage s;
  lbfgs_write_model(a, s, threadIdx.x, blockDim.x);
}
// One evaluation: value and chained gradient of the point evaluated, the state machine, the next model, one log entry.  Once the run
// has stopped every later slot logs IDLE and returns.
__global__ __launch_bounds__(ADAM_THREADS) void lbfgs_ctl_kernel(LbfgsArgs a, int slot) {
  __shared__ ModelStage s;
  __shared__ double scratch[HBO_LBFGS_PARTIALS];
  const int tid = threadIdx.x, nthr = blockDim.x, P = a.t.P;
  const hbo_lbfgs_view v = hbo_lbfgs_view_of(a.state, P, a.o.memory);
  if (v.hdr[HBO_LBFGS_S_STATUS] != (double)HBO_LBFGS_CTL_RUNNING) {   // (no thread of this launch writes the status before this read)
    if (tid == 0) { hbo_lbfgs_eval_ctl e; e.kind = HBO_LBFGS_CTL_IDLE; e.iter = (int)v.hdr[HBO_LBFGS_S_ITER]; e.alpha = 0.0; e.value = NAN; a.log[slot] = e; }
    return;
  }
  const double count = a.t.red[1];
  const double value = a.t.red[0] / count;
  for (int i = tid; i < P; i += nthr) {
    const double x = v.xt[i];
    if (a.trace) a.trace[(size_t)slot * P + i] = x;
    v.g[i] = chained_grad(a.t, a.t.leaves[i], i, x, count);
  }
  __syncthreads();
  hbo_lbfgs_eval_ctl ev;
  hbo_lbfgs_ctl_step(a.state, P, a.o, value, tid, nthr, scratch, &ev);
  if (tid == 0) a.log[slot] = ev;
  if (v.hdr[HBO_LBFGS_S_STATUS] == (double)HBO_LBFGS_CTL_RUNNING) lbfgs_write_model(a, s, tid, nthr);
}

int train_gradient_offset(const hbo_model* m, const hbo_grad_layout& lay, int32_t ka, int32_t kb, const hbo_train_leaf& lf) {
  switch (lf.target) {
    case HBO_TRAIN_LENGTHSCALE: return lay.lengthscale < 0 ? -1 : lay.lengthscale + lf.index;
    case HBO_TRAIN_SIGNAL_VARIANCE: return lay.signal_variance;
    case HBO_TRAIN_NOISE_VARIANCE: return lay.noise_variance;
    case HBO_TRAIN_CONSTANT: return lay.constant;
    case HBO_TRAIN_DOT_PROD_SIGMA: return lay.dot_prod_sigma;
    case HBO_TRAIN_DOT_PROD_BIAS: return lay.dot_prod_bias;
    case HBO_TRAIN_LINEAR_KERNEL: return lay.linear_kernel < 0 ? -1 : lay.linear_kernel + lf.index;
    case HBO_TRAIN_LINEAR_BIAS: return lay.linear_bias;
    case HBO_TRAIN_MLP_KERNEL: return lay.mlp_kernel[lf.layer] < 0 ? -1 : lay.mlp_kernel[lf.layer] + lf.index;
    case HBO_TRAIN_MLP_BIAS: return lay.mlp_bias[lf.layer] < 0 ? -1 : lay.mlp_bias[lf.layer] + lf.index;
    case HBO_TRAIN_KUMAR_A: return ka < 0 ? -1 : ka + lf.index;
    case HBO_TRAIN_KUMAR_B: return kb < 0 ? -1 : kb + lf.index;
    default: return -1;
  }
}
// number of elements of a leaf's target (the bound of its index); 0 = the model has no such field
int train_target_size(const hbo_model* m, const hbo_train_leaf& lf) {
  switch (lf.target) {
    case HBO_TRAIN_NONE: return 1;
    case HBO_TRAIN_LENGTHSCALE: return m->kernel_id == HBO_KERNEL_DOT ? 0 : m->n_lengthscale;
    case HBO_TRAIN_LINEAR_KERNEL: return mean_feature_dim(m);
    case HBO_TRAIN_MLP_KERNEL: case HBO_TRAIN_MLP_BIAS:
      if (!needs_mlp(m) || lf.layer < 0 || lf.layer >= m->n_layers) return 0;
      return lf.target == HBO_TRAIN_MLP_BIAS ? m->features[lf.layer] : (lf.layer ? m->features[lf.layer - 1] : m->input_dim) * m->features[lf.layer];
    case HBO_TRAIN_KUMAR_A: case HBO_TRAIN_KUMAR_B: return is_kumar(m) ? m->input_dim : 0;
    default: return 1;
  }
}

// The checks of model and leaf map that need neither the dataset nor the context; goff[i]: where leaf i's gradient sits in the layout
int train_check_leaves(hbo_ctx* c, const std::string& fn, const hbo_model* m, const hbo_train_leaf* leaves, int32_t P, hbo_grad_layout& lay,
                       std::vector<int>& goff) {
  if (int rc = validate_model(c, m)) return rc;
  if (m->n_lengthscale > HBO_MAX_FEATURE_DIM) return fail(c, HBO_ERR_ARG, fn + "bad n_lengthscale");
  if (int rc = hbo_grad_layout_of(m, &lay)) return fail(c, rc, fn + "bad model");
  int32_t ka = -1, kb = -1;
  hbo_grad_layout_kumar_of(m, &ka, &kb);
  goff.resize(P);
  for (int i = 0; i < P; ++i) {
    const hbo_train_leaf& lf = leaves[i];
    if (lf.warp < HBO_TRAIN_WARP_IDENTITY || lf.warp > HBO_TRAIN_WARP_SQUAREPLUS)
      return fail(c, HBO_ERR_ARG, fn + "leaf " + std::to_string(i) + ": unknown warp");
    if (lf.target < HBO_TRAIN_NONE || lf.target > HBO_TRAIN_KUMAR_B)
      return fail(c, HBO_ERR_ARG, fn + "leaf " + std::to_string(i) + ": unknown target");
    if (lf.round_f32 != 0 && lf.round_f32 != 1) return fail(c, HBO_ERR_ARG, fn + "leaf " + std::to_string(i) + ": round_f32 is 0 or 1");
    if (lf.index < 0 || lf.index >= train_target_size(m, lf))
      return fail(c, HBO_ERR_ARG, fn + "leaf " + std::to_string(i) + ": layer / index outside its target");
    goff[i] = train_gradient_offset(m, lay, ka, kb, lf);
    if (lf.target != HBO_TRAIN_NONE && (goff[i] < 0 || goff[i] >= lay.total))
      return fail(c, HBO_ERR_ARG, fn + "leaf " + std::to_string(i) + ": the model does not read its target");
  }
  return HBO_OK;
}
// The argument checks of both training entry points, in the order both report them: model and P; own(), the caller's other arguments
// that need neither the dataset nor the context; the leaf map; the dataset against the model; sizes(), which may lower the task sizes
// s.nd to those of the caller's batch; then the context and the fused regime: every task of the batch in one 128-block, small_fused
// on, enough LDS.
struct TrainSetup { hbo_grad_layout lay; std::vector<int> goff; std::vector<int64_t> nd; int T = 0; int64_t max_n = 0; };
template <class Own, class Sizes>
int train_prologue(hbo_ctx* c, const std::string& fn, const hbo_model* m, int32_t P, const hbo_train_leaf* leaves, const hbo_dataset* ds,
                   Own own, Sizes sizes, TrainSetup& s) {
  if (!m) return fail(c, HBO_ERR_ARG, fn + "model is null");
  if (P <= 0) return fail(c, HBO_ERR_ARG, fn + "P must be positive");
  if (int rc = own()) return rc;
  if (int rc = train_check_leaves(c, fn, m, leaves, P, s.lay, s.goff)) return rc;
  if (!ds) return fail(c, HBO_ERR_ARG, fn + "dataset is null");
  if (ds->ntasks <= 0) return fail(c, HBO_ERR_ARG, fn + "the dataset has no tasks");
  if (m->dtype != ds->dtype || m->input_dim != ds->D) return fail(c, HBO_ERR_ARG, fn + "model/dataset dtype or input_dim mismatch");
  s.T = ds->ntasks;
  s.nd.resize(s.T);
  for (int k = 0; k < s.T; ++k) s.nd[k] = ds->tasks[k]->n;
  if (int rc = sizes()) return rc;
  for (int k = 0; k < s.T; ++k) s.max_n = std::max(s.max_n, s.nd[k]);
  if (!c) return fail(c, HBO_ERR_ARG, fn + "context is null");
  if (s.max_n > HBO_TILE) return fail(c, HBO_ERR_UNSUPPORTED, fn + "a task of the batch has more than 128 points (only the fused regime runs on the device)");
  if (!c->opt_small_fused) return fail(c, HBO_ERR_UNSUPPORTED, fn + "small_fused is off (only the fused regime runs on the device)");
  if (small_eval_lds(ds->dtype) > c->lds_per_block) return fail(c, HBO_ERR_UNSUPPORTED, fn + "the device cannot give the single-workgroup evaluation its LDS");
  return HBO_OK;
}

// The evaluations of one resident batch, queued on the context's stream.  first() is everything hbo_objective does, up to the
// device-side reduction: objective_local reduces [nll_sum, T, grad] on the device, without waiting, only for a caller that hands it a
// ShardReq (the sharded objective's door), so it gets one whose count nobody reads, and host results that stay zero.  What it leaves in
// ShardOut -- the reduction buffer the step kernels read, the scatter map, the stride -- serves every later evaluation: again() is the
// three launches alone, no host-side set-up.
struct TrainEval {
  hbo_ctx* c; const hbo_model* m; int T; int64_t max_n; int grad_total;
  ShardOut so;
  int first(const std::string& fn, hbo_dataset* batch) {
    std::vector<double> grad0(std::max(grad_total, 1));
    double nll0 = 0, count0 = 0;
    const ShardReq sh{&count0, nullptr};
    if (int rc = objective_local(c, m, batch, HBO_OBJ_NLL, &nll0, nullptr, grad0.data(), &sh, &so)) return rc;
    if (!so.d_red || so.red_count != 2 + grad_total) return fail(c, HBO_ERR_HIP, fn + "no reduction buffer");
    return HBO_OK;
  }
  int again(hbo_dataset* batch) {
    enqueue_fused_forward(c, m, batch, max_n, so.out_stride, true);
    if (int rc = enqueue_backward(c, m, batch, max_n, OBJ_NLL, true)) return rc;
    launch_shard_reduce(batch->d_nll, batch->d_gradout, batch->d_info, T, so.out_stride, so.d_map, batch->d_mlpgrad,
                        so.d_map + so.out_stride, so.nseg, so.d_red, so.red_count, c->stream);
    return HBO_OK;
  }
};
// The end of both calls: the launches' error, ONE copy back of the block's bytes [first, total) to the same offsets of its host copy, one wait
int train_finish(hbo_ctx* c, unsigned char* host, const unsigned char* dev, size_t first, size_t total) {
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(host + first, dev + first, total - first, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  prof_collect(c);
  return HBO_OK;
}

// The head of both loops' upload: [leaves | goff | the starting model's arrays (model dtype)], the first parts of the block `lay` lays out
struct TrainPack { size_t o_leaf, o_goff, o_ls, o_lin, o_ka, o_kb; int n_ls, fm; };
TrainPack train_pack_layout(BlockLayout& lay, const hbo_model* m, int32_t P) {
  TrainPack p;
  const size_t es = esize(m->dtype);
  p.n_ls = m->kernel_id == HBO_KERNEL_DOT ? 0 : m->n_lengthscale; p.fm = mean_feature_dim(m);
  p.o_leaf = lay.take(sizeof(hbo_train_leaf) * P); p.o_goff = lay.take(sizeof(int) * P);
  p.o_ls = lay.take(es * std::max(p.n_ls, 1)); p.o_lin = lay.take(es * std::max(p.fm, 1));
  p.o_ka = lay.take(es * m->input_dim); p.o_kb = lay.take(es * m->input_dim);
  return p;
}
void train_pack_fill(unsigned char* h, const TrainPack& p, const hbo_model* m, const hbo_train_leaf* leaves, const std::vector<int>& goff, int32_t P) {
  const size_t es = esize(m->dtype);
  memcpy(h + p.o_leaf, leaves, sizeof(hbo_train_leaf) * P); memcpy(h + p.o_goff, goff.data(), sizeof(int) * P);
  if (p.n_ls) memcpy(h + p.o_ls, m->lengthscale, es * p.n_ls);
  if (p.fm) memcpy(h + p.o_lin, m->linear_kernel, es * p.fm);
  if (is_kumar(m)) { memcpy(h + p.o_ka, as_kumar(m)->kumar_a, es * m->input_dim); memcpy(h + p.o_kb, as_kumar(m)->kumar_b, es * m->input_dim); }
}
// d: the device copy of the upload; red: the reduction the step kernels read
void train_dev_set(TrainDev& t, hbo_ctx* c, const hbo_model* m, unsigned char* d, const TrainPack& p, int32_t P, const double* red) {
  memset(&t, 0, sizeof t);
  const bool kumar = is_kumar(m);
  t.leaves = reinterpret_cast<const hbo_train_leaf*>(d + p.o_leaf); t.goff = reinterpret_cast<const int*>(d + p.o_goff); t.P = P;
  t.red = red;
  if (kumar) t.init = *as_kumar(m); else t.init.base = *m;
  t.init.base.lengthscale = d + p.o_ls; t.init.base.linear_kernel = d + p.o_lin;
  if (kumar) { t.init.kumar_a = d + p.o_ka; t.init.kumar_b = d + p.o_kb; }
  for (int l = 0; l < HBO_MAX_MLP_LAYERS; ++l) { t.init.base.mlp_kernel[l] = nullptr; t.init.base.mlp_bias[l] = nullptr; }
  t.n_ls = p.n_ls; t.fm = p.fm;
  for (int l = 0; l < HBO_MAX_MLP_LAYERS; ++l) { t.mlp_w[l] = c->d_mlp_w[l]; t.mlp_b[l] = c->d_mlp_b[l]; }
  t.md = c->d_model;
}

int lbfgs_check_opts(hbo_ctx* c, const std::string& fn, const hbo_lbfgs_opts* o) {
  if (!o) return fail(c, HBO_ERR_ARG, fn + "opts is null");
  if (o->memory < 1) return fail(c, HBO_ERR_ARG, fn + "opts.memory must be at least 1");
  if (o->ls_steps < 1) return fail(c, HBO_ERR_ARG, fn + "opts.ls_steps must be at least 1");
  if (o->max_iters < 1) return fail(c, HBO_ERR_ARG, fn + "opts.max_iters must be at least 1");
  if (!(o->alpha == o->alpha) || !(o->tol == o->tol) || !(o->c1 == o->c1) || !(o->c2 == o->c2) || !(o->grow == o->grow) || !(o->tau == o->tau))
    return fail(c, HBO_ERR_ARG, fn + "opts.alpha, tol, c1, c2, grow and tau must be numbers");
  return HBO_OK;
}
hbo_lbfgs_opts_ctl lbfgs_ctl_opts(const hbo_lbfgs_opts* o) {
  hbo_lbfgs_opts_ctl r;
  r.memory = o->memory; r.ls_steps = o->ls_steps; r.max_iters = o->max_iters;
  r.alpha = o->alpha; r.tol = o->tol; r.c1 = o->c1; r.c2 = o->c2; r.grow = o->grow; r.tau = o->tau;
  return r;
}
// A state the control code can index with: all zero (a fresh run), or a header hbo_lbfgs_ctl_step left.  *fresh: the run starts at x.
int lbfgs_check_state(hbo_ctx* c, const std::string& fn, const double* state, const hbo_lbfgs_opts* o, bool* fresh) {
  const double* h = state;
  auto whole = [&](int k, double lo, double hi) { return h[k] >= lo && h[k] <= hi && h[k] == (double)(int64_t)h[k]; };
  const bool ok = whole(HBO_LBFGS_S_PHASE, 0, 2) && whole(HBO_LBFGS_S_STATUS, 0, HBO_LBFGS_CTL_STEPS_DONE) && whole(HBO_LBFGS_S_ITER, 0, INT_MAX) &&
                  whole(HBO_LBFGS_S_PROBES, 0, INT_MAX) && whole(HBO_LBFGS_S_NHIST, 0, o->memory) && whole(HBO_LBFGS_S_HEAD, 0, o->memory - 1) &&
                  whole(HBO_LBFGS_S_EVALS, 0, INT_MAX);
  *fresh = ok && h[HBO_LBFGS_S_PHASE] == HBO_LBFGS_PHASE_START && h[HBO_LBFGS_S_EVALS] == 0 && h[HBO_LBFGS_S_STATUS] == 0;
  if (!ok || (h[HBO_LBFGS_S_PHASE] == HBO_LBFGS_PHASE_START && !*fresh && h[HBO_LBFGS_S_STATUS] == 0))
    return fail(c, HBO_ERR_ARG, fn + "state is neither all zero nor one an earlier call with the same P and memory left");
  return HBO_OK;
}

}  // namespace

extern "C" int hbo_train_adam(hbo_ctx* c, const hbo_model* m, hbo_dataset* ds, const hbo_train_leaf* leaves, int32_t P,
                              double* x, double* adam_m, double* adam_v, const double* bias1, const double* bias2,
                              int32_t steps, double lr, double b1, double b2, double adam_eps,
                              const int64_t* batch_counts, const int32_t* batch_rows,
                              double* losses, double* x_trace, int32_t* steps_done) {
  const std::string fn = "hbo_train_adam: ";
  TrainSetup ts;
  int64_t nidx = 0;
  auto own = [&]() -> int {
    if (steps <= 0) return fail(c, HBO_ERR_ARG, fn + "steps must be positive");
    if (!leaves || !x || !adam_m || !adam_v || !bias1 || !bias2 || !losses || !steps_done)
      return fail(c, HBO_ERR_ARG, fn + "null array argument (leaves, x, adam_m, adam_v, bias1, bias2, losses, steps_done)");
    if (!batch_counts != !batch_rows) return fail(c, HBO_ERR_ARG, fn + "batch_counts and batch_rows are both given or both null");
    if (!(lr == lr) || !(b1 == b1) || !(b2 == b2) || !(adam_eps == adam_eps))
      return fail(c, HBO_ERR_ARG, fn + "lr, b1, b2 and adam_eps must be numbers");
    return HBO_OK;
  };
  // the batch: its task sizes (the same every step) and the rows a step consumes
  auto sizes = [&]() -> int {
    if (!batch_counts) return HBO_OK;
    const int T = ts.T;
    for (int k = 0; k < T; ++k) {
      const int64_t ck = batch_counts[k];
      if (ck == 0 || ck > ts.nd[k]) return fail(c, HBO_ERR_ARG, fn + "batch_counts[k] must be in 1..n_k (or negative: the whole task)");
      if (ck > 0) { ts.nd[k] = ck; nidx += ck; }
    }
    for (int s = 1; s < steps; ++s)
      for (int k = 0; k < T; ++k)
        if ((batch_counts[(size_t)s * T + k] < 0) != (batch_counts[k] < 0) || (batch_counts[k] >= 0 && batch_counts[(size_t)s * T + k] != batch_counts[k]))
          return fail(c, HBO_ERR_ARG, fn + "batch_counts must be the same at every step");
    for (int s = 0; s < steps; ++s) {
      int64_t off = (int64_t)s * nidx;
      for (int k = 0; k < T; ++k) {
        if (batch_counts[k] < 0) continue;
        for (int64_t r = 0; r < batch_counts[k]; ++r, ++off)
          if (batch_rows[off] < 0 || batch_rows[off] >= ds->tasks[k]->n) return fail(c, HBO_ERR_ARG, fn + "batch_rows: index out of range");
      }
    }
    return HBO_OK;
  };
  if (int rc = train_prologue(c, fn, m, P, leaves, ds, own, sizes, ts)) return rc;
  const int T = ts.T, D = ds->D, dtype = ds->dtype;
  const int64_t max_n = ts.max_n;

  // ---- step 0: the batch, then everything hbo_objective does, up to the device-side reduction
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  hbo_dataset* batch = ds;
  if (batch_counts) { if (int rc = hbo_dataset_subsample(c, ds, batch_counts, batch_rows, &batch)) return rc; }
  struct BatchGuard {   // (a queued launch may still read the batch: wait before it goes back to the pool)
    hbo_ctx* c; hbo_dataset* b;
    ~BatchGuard() { if (b) { (void)hipStreamSynchronize(c->stream); hbo_dataset_free(c, b); } }
  } guard{c, batch_counts ? batch : nullptr};
  TrainEval ev{c, m, T, max_n, ts.lay.total};
  if (int rc = ev.first(fn, batch)) return rc;

  // ---- one upload: [leaves | goff | initial arrays | bias1 | bias2 | gather table | rows | x | m | v | halt, steps_done | losses],
  //      then the trace; the copy back takes [x .. trace]
  std::vector<int> perm(T);
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return ts.nd[a] > ts.nd[b]; });   // dataset_finish's task order (dataset.hip), as hbo_dataset_subsample leaves it
  std::vector<GatherTask> gt;
  if (batch_counts) {
    std::vector<int64_t> ioff(T, 0);
    for (int k = 0, o = 0; k < T; ++k) { ioff[k] = o; if (batch_counts[k] > 0) o += batch_counts[k]; }
    for (int j = 0; j < T; ++j) {
      const int k = perm[j];
      if (batch_counts[k] < 0) continue;   // kept whole: its rows never change
      const TaskHost* s = ds->tasks[k]; TaskHost* t = batch->tasks[j];
      gt.push_back(GatherTask{s->X, s->ysum, s->ydiv, t->X, t->ysum, t->ydiv, s->n, t->n, ioff[k], s->m, 1});
    }
  }
  BlockLayout blk;
  const TrainPack pack = train_pack_layout(blk, m, P);
  const size_t o_b1 = blk.take(sizeof(double) * steps), o_b2 = blk.take(sizeof(double) * steps);
  const size_t o_gt = blk.take(sizeof(GatherTask) * std::max<size_t>(gt.size(), 1));
  const size_t o_rows = blk.take(sizeof(int32_t) * std::max<int64_t>(batch_counts ? nidx * steps : 0, 1));
  const size_t o_x = blk.take(sizeof(double) * P), o_m = blk.take(sizeof(double) * P), o_v = blk.take(sizeof(double) * P);
  const size_t o_int = blk.take(2 * sizeof(int)), o_loss = blk.take(sizeof(double) * steps);
  const size_t up_bytes = blk.off;
  const size_t o_trace = blk.take(x_trace ? sizeof(double) * steps * (size_t)P : 0);
  const size_t total = blk.off;
  std::vector<unsigned char> h(total, 0);
  auto cp = [&](size_t o, const void* src, size_t b) { if (b) memcpy(h.data() + o, src, b); };
  train_pack_fill(h.data(), pack, m, leaves, ts.goff, P);
  cp(o_b1, bias1, sizeof(double) * steps); cp(o_b2, bias2, sizeof(double) * steps);
  cp(o_gt, gt.data(), sizeof(GatherTask) * gt.size());
  if (batch_counts) cp(o_rows, batch_rows, sizeof(int32_t) * nidx * steps);
  cp(o_x, x, sizeof(double) * P); cp(o_m, adam_m, sizeof(double) * P); cp(o_v, adam_v, sizeof(double) * P);
  const int ints[2] = {0, steps};
  cp(o_int, ints, sizeof ints);
  for (int s = 0; s < steps; ++s) reinterpret_cast<double*>(h.data() + o_loss)[s] = NAN;
  unsigned char* d = static_cast<unsigned char*>(ws_get(c, WS_TRAIN, total));
  if (!d) return HBO_ERR_HIP;
  HIPCHK(c, hipMemcpyAsync(d, h.data(), up_bytes, hipMemcpyHostToDevice, st));

  AdamStepArgs a;
  memset(&a, 0, sizeof a);
  train_dev_set(a.t, c, m, d, pack, P, ev.so.d_red);
  a.x = reinterpret_cast<double*>(d + o_x); a.am = reinterpret_cast<double*>(d + o_m); a.av = reinterpret_cast<double*>(d + o_v);
  a.bias1 = reinterpret_cast<const double*>(d + o_b1); a.bias2 = reinterpret_cast<const double*>(d + o_b2);
  a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = adam_eps;
  a.losses = reinterpret_cast<double*>(d + o_loss); a.trace = x_trace ? reinterpret_cast<double*>(d + o_trace) : nullptr;
  a.halt = reinterpret_cast<int*>(d + o_int); a.steps_done = a.halt + 1;

  const GatherTask* d_gt = reinterpret_cast<const GatherTask*>(d + o_gt);
  const int32_t* d_rows = reinterpret_cast<const int32_t*>(d + o_rows);
  for (int s = 0; s < steps; ++s) {
    if (s > 0) {
      if (!gt.empty()) launch_gather_rows(dtype, d_gt, d_rows + (size_t)s * nidx, (int)gt.size(), max_n, D, st);
      if (int rc = ev.again(batch)) return rc;
    }
    { ProfScope ps(c, "adam_step", 1);
      hipLaunchKernelGGL(adam_step_kernel, dim3(1), dim3(ADAM_THREADS), 0, st, a, s); }
  }
  if (int rc = train_finish(c, h.data(), d, o_x, total)) return rc;
  memcpy(x, h.data() + o_x, sizeof(double) * P); memcpy(adam_m, h.data() + o_m, sizeof(double) * P); memcpy(adam_v, h.data() + o_v, sizeof(double) * P);
  memcpy(losses, h.data() + o_loss, sizeof(double) * steps);
  if (x_trace) memcpy(x_trace, h.data() + o_trace, sizeof(double) * steps * (size_t)P);
  *steps_done = reinterpret_cast<const int*>(h.data() + o_int)[1];
  return HBO_OK;
}

extern "C" int64_t hbo_lbfgs_state_doubles(int32_t P, int32_t memory) {
  if (P <= 0 || memory < 1) return 0;
  return hbo_lbfgs_state_size(P, memory);
}

extern "C" int hbo_train_lbfgs(hbo_ctx* c, const hbo_model* m, hbo_dataset* ds, const hbo_train_leaf* leaves, int32_t P,
                               const hbo_lbfgs_opts* opts, double* x, double* state, int32_t evals, hbo_lbfgs_eval* log,
                               double* x_trace, double* x_next, int32_t* evals_done, int32_t* status) {
  const std::string fn = "hbo_train_lbfgs: ";
  TrainSetup ts;
  bool fresh = false;
  auto own = [&]() -> int {
    if (evals <= 0) return fail(c, HBO_ERR_ARG, fn + "evals must be positive");
    if (!leaves || !x || !state || !log || !evals_done || !status)
      return fail(c, HBO_ERR_ARG, fn + "null array argument (leaves, x, state, log, evals_done, status)");
    if (int rc = lbfgs_check_opts(c, fn, opts)) return rc;
    return lbfgs_check_state(c, fn, state, opts, &fresh);
  };
  if (int rc = train_prologue(c, fn, m, P, leaves, ds, own, [] { return (int)HBO_OK; }, ts)) return rc;

  const int64_t ns = hbo_lbfgs_state_size(P, opts->memory);
  hbo_lbfgs_view hv = hbo_lbfgs_view_of(state, P, opts->memory);
  *evals_done = 0;
  *status = (int32_t)state[HBO_LBFGS_S_STATUS];
  if (*status != HBO_LBFGS_RUNNING) {   // a run that has stopped: nothing to queue
    memcpy(x, hv.x, sizeof(double) * P);
    if (x_next) memcpy(x_next, hv.xt, sizeof(double) * P);
    return HBO_OK;
  }
  if (fresh) hbo_lbfgs_state_start(state, P, opts->memory, x);

  // ---- the first evaluation: everything hbo_objective does, up to the device-side reduction
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  TrainEval ev{c, m, ts.T, ts.max_n, ts.lay.total};
  if (int rc = ev.first(fn, ds)) return rc;

  // ---- one upload: [leaves | goff | initial arrays | state], then log and trace; the copy back takes [state .. trace]
  BlockLayout blk;
  const TrainPack pack = train_pack_layout(blk, m, P);
  const size_t o_state = blk.take(sizeof(double) * ns);
  const size_t up_bytes = blk.off;
  const size_t o_log = blk.take(sizeof(hbo_lbfgs_eval) * evals);
  const size_t o_trace = blk.take(x_trace ? sizeof(double) * evals * (size_t)P : 0);
  const size_t total = blk.off;
  std::vector<unsigned char> h(total, 0);
  train_pack_fill(h.data(), pack, m, leaves, ts.goff, P);
  memcpy(h.data() + o_state, state, sizeof(double) * ns);
  unsigned char* d = static_cast<unsigned char*>(ws_get(c, WS_TRAIN, total));
  if (!d) return HBO_ERR_HIP;
  HIPCHK(c, hipMemcpyAsync(d, h.data(), up_bytes, hipMemcpyHostToDevice, st));

  LbfgsArgs a;
  memset(&a, 0, sizeof a);
  train_dev_set(a.t, c, m, d, pack, P, ev.so.d_red);
  a.o = lbfgs_ctl_opts(opts);
  a.state = reinterpret_cast<double*>(d + o_state);
  a.log = reinterpret_cast<hbo_lbfgs_eval_ctl*>(d + o_log);
  a.trace = x_trace ? reinterpret_cast<double*>(d + o_trace) : nullptr;

  if (!fresh) {
    // A continued run: the pending point's model again with the device's warps (objective_local evaluated the caller's, whose host
    // warps may differ in the last bit), so that a run gives the same bits however it is cut into calls.
    { ProfScope ps(c, "lbfgs_ctl", 1);
      hipLaunchKernelGGL(lbfgs_model_kernel, dim3(1), dim3(ADAM_THREADS), 0, st, a); }
    if (int rc = ev.again(ds)) return rc;
  }
  for (int s = 0; s < evals; ++s) {
    if (s > 0) { if (int rc = ev.again(ds)) return rc; }
    { ProfScope ps(c, "lbfgs_ctl", 1);
      hipLaunchKernelGGL(lbfgs_ctl_kernel, dim3(1), dim3(ADAM_THREADS), 0, st, a, s); }
  }
  if (int rc = train_finish(c, h.data(), d, o_state, total)) return rc;
  memcpy(state, h.data() + o_state, sizeof(double) * ns);
  memcpy(log, h.data() + o_log, sizeof(hbo_lbfgs_eval) * evals);
  if (x_trace) memcpy(x_trace, h.data() + o_trace, sizeof(double) * evals * (size_t)P);
  memcpy(x, hv.x, sizeof(double) * P);
  if (x_next) memcpy(x_next, hv.xt, sizeof(double) * P);
  int done = 0;
  while (done < evals && log[done].kind != HBO_LBFGS_IDLE) ++done;
  *evals_done = done;
  *status = (int32_t)state[HBO_LBFGS_S_STATUS];
  return HBO_OK;
}

// include/hbo_tune.h (TEST HOOK): the control code of lbfgs_ctl.h on the host, one thread, for one evaluation
extern "C" int hbo_probe_lbfgs_ctl(double* state, int32_t P, const hbo_lbfgs_opts* opts, const double* x0, double value, const double* grad,
                                   double* x_next, double* x_iter, hbo_lbfgs_eval* eval, int32_t* status) {
  const std::string fn = "hbo_probe_lbfgs_ctl: ";
  if (P <= 0) return fail(nullptr, HBO_ERR_ARG, fn + "P must be positive");
  if (!state || !grad || !x_next || !eval || !status) return fail(nullptr, HBO_ERR_ARG, fn + "null argument (state, grad, x_next, eval, status)");
  if (int rc = lbfgs_check_opts(nullptr, fn, opts)) return rc;
  bool fresh = false;
  if (int rc = lbfgs_check_state(nullptr, fn, state, opts, &fresh)) return rc;
  if (fresh && !x0) return fail(nullptr, HBO_ERR_ARG, fn + "an all-zero state needs x0");
  if (fresh) hbo_lbfgs_state_start(state, P, opts->memory, x0);
  const hbo_lbfgs_view v = hbo_lbfgs_view_of(state, P, opts->memory);
  memcpy(v.g, grad, sizeof(double) * P);
  double scratch[HBO_LBFGS_PARTIALS];
  hbo_lbfgs_eval_ctl ev;
  hbo_lbfgs_ctl_step(state, P, lbfgs_ctl_opts(opts), value, 0, 1, scratch, &ev);
  eval->kind = ev.kind; eval->iter = ev.iter; eval->alpha = ev.alpha; eval->value = ev.value;
  memcpy(x_next, v.xt, sizeof(double) * P);
  if (x_iter) memcpy(x_iter, v.x, sizeof(double) * P);
  *status = (int32_t)state[HBO_LBFGS_S_STATUS];
  return HBO_OK;
}
