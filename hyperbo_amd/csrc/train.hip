// hbo_train_adam: K Adam steps of infer_parameters(method='adam') (hyperbo/gp_utils/gp.py:53-195) queued on the device for a batch
// whose tasks all fit one 128-block.  Per step: [gather the step's rows in place] -> single-workgroup evaluation and its backward
// passes (objective.hip: enqueue_fused_forward / enqueue_backward) -> launch_shard_reduce ([nll_sum, T, grad] in the caller's
// layout) -> adam_step_kernel.  No host wait between steps: one copy back and one synchronisation per call.
#include "api_internal.h"

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

struct AdamStepArgs {
  const hbo_train_leaf* leaves; const int* goff; int P;
  double* x; double* am; double* av;
  const double* bias1; const double* bias2;
  double lr, b1, b2, eps;
  const double* red;                 // [nll_sum, T, grad sum in the caller's layout]
  double* losses; double* trace;     // trace nullable
  int* halt; int* steps_done;
  hbo_model_kumar init;              // the starting model; its array pointers point at device copies (model dtype)
  int n_ls, fm;
  void* mlp_w[HBO_MAX_MLP_LAYERS]; void* mlp_b[HBO_MAX_MLP_LAYERS];
  ModelDev* md;
};

// One step: loss check (gp.py:135-142), warp chain rule (_model.BuiltModel.unflatten_grad), Adam (gp.py:_Adam.step), then the
// warped next model into ModelDev and the MLP weight buffers.  A non-finite loss sets the halt word: every later step returns here.
__global__ __launch_bounds__(ADAM_THREADS) void adam_step_kernel(AdamStepArgs a, int step) {
  __shared__ double s_ls[HBO_MAX_FEATURE_DIM], s_lin[HBO_MAX_FEATURE_DIM], s_ka[HBO_MAX_FEATURE_DIM], s_kb[HBO_MAX_FEATURE_DIM];
  __shared__ double s_sc[6];   // signal variance, noise variance, constant, dot sigma, dot bias, linear bias
  __shared__ int s_halt;
  const int tid = threadIdx.x, nthr = blockDim.x;
  if (tid == 0) s_halt = *a.halt;
  __syncthreads();
  if (s_halt) return;
  const double count = a.red[1];
  const double loss = a.red[0] / count;
  if (tid == 0) a.losses[step] = loss;
  if (!isfinite(loss)) {
    if (tid == 0) { *a.halt = 1; *a.steps_done = step; }
    return;
  }
  const hbo_model& m0 = a.init.base;
  const int dtype = m0.dtype, D = m0.input_dim;
  for (int d = tid; d < HBO_MAX_FEATURE_DIM; d += nthr) {
    if (d < a.n_ls) put_elem(s_ls, dtype, d, model_elem(m0.lengthscale, dtype, d));
    if (d < a.fm) put_elem(s_lin, dtype, d, model_elem(m0.linear_kernel, dtype, d));
    if (m0.input_warp == HBO_WARP_KUMAR && d < D) {
      put_elem(s_ka, dtype, d, model_elem(a.init.kumar_a, dtype, d));
      put_elem(s_kb, dtype, d, model_elem(a.init.kumar_b, dtype, d));
    }
  }
  if (tid == 0) {
    s_sc[0] = m0.signal_variance; s_sc[1] = m0.noise_variance; s_sc[2] = m0.constant;
    s_sc[3] = m0.dot_prod_sigma; s_sc[4] = m0.dot_prod_bias; s_sc[5] = m0.linear_bias;
  }
  __syncthreads();
  const double b1 = a.b1, b2 = a.b2, c1 = 1 - b1, c2 = 1 - b2;
  const double bias1 = a.bias1[step], bias2 = a.bias2[step];
  for (int i = tid; i < a.P; i += nthr) {
    const hbo_train_leaf lf = a.leaves[i];
    const double x = a.x[i];
    if (a.trace) a.trace[(size_t)step * a.P + i] = x;
    const double xr = lf.round_f32 ? (double)(float)x : x;
    // grad / count, then d warp / d raw (a leaf the model does not read has gradient zero)
    double g = 0.0;
    if (a.goff[i] >= 0) g = (a.red[2 + a.goff[i]] / count) * warp_slope(lf.warp, xr);
    const double m = b1 * a.am[i] + c1 * g;
    const double v = b2 * a.av[i] + c2 * g * g;
    const double mhat = m / bias1;
    const double vhat = v / bias2;
    const double xn = x - a.lr * mhat / (sqrt(vhat) + a.eps);
    a.am[i] = m; a.av[i] = v; a.x[i] = xn;
    const double xnr = lf.round_f32 ? (double)(float)xn : xn;
    double w = warp_value(lf.warp, xnr);
    if (lf.round_f32) w = (double)(float)w;
    switch (lf.target) {
      case HBO_TRAIN_LENGTHSCALE: put_elem(s_ls, dtype, lf.index, w); break;
      case HBO_TRAIN_SIGNAL_VARIANCE: s_sc[0] = w; break;
      case HBO_TRAIN_NOISE_VARIANCE: s_sc[1] = w; break;
      case HBO_TRAIN_CONSTANT: s_sc[2] = w; break;
      case HBO_TRAIN_DOT_PROD_SIGMA: s_sc[3] = w; break;
      case HBO_TRAIN_DOT_PROD_BIAS: s_sc[4] = w; break;
      case HBO_TRAIN_LINEAR_BIAS: s_sc[5] = w; break;
      case HBO_TRAIN_LINEAR_KERNEL: put_elem(s_lin, dtype, lf.index, w); break;
      case HBO_TRAIN_MLP_KERNEL: put_elem(a.mlp_w[lf.layer], dtype, lf.index, w); break;
      case HBO_TRAIN_MLP_BIAS: put_elem(a.mlp_b[lf.layer], dtype, lf.index, w); break;
      case HBO_TRAIN_KUMAR_A: put_elem(s_ka, dtype, lf.index, w); break;
      case HBO_TRAIN_KUMAR_B: put_elem(s_kb, dtype, lf.index, w); break;
      default: break;
    }
  }
  __syncthreads();
  hbo_model_kumar mk = a.init;
  mk.base.signal_variance = s_sc[0]; mk.base.noise_variance = s_sc[1]; mk.base.constant = s_sc[2];
  mk.base.dot_prod_sigma = s_sc[3]; mk.base.dot_prod_bias = s_sc[4]; mk.base.linear_bias = s_sc[5];
  mk.base.lengthscale = s_ls; mk.base.linear_kernel = s_lin; mk.kumar_a = s_ka; mk.kumar_b = s_kb;
  model_dev_fill(*a.md, &mk.base, tid, nthr);
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

}  // namespace

extern "C" int hbo_train_adam(hbo_ctx* c, const hbo_model* m, hbo_dataset* ds, const hbo_train_leaf* leaves, int32_t P,
                              double* x, double* adam_m, double* adam_v, const double* bias1, const double* bias2,
                              int32_t steps, double lr, double b1, double b2, double adam_eps,
                              const int64_t* batch_counts, const int32_t* batch_rows,
                              double* losses, double* x_trace, int32_t* steps_done) {
  // ---- arguments: everything that does not need the context or the dataset first, then the dataset, then the context
  const char* fn = "hbo_train_adam: ";
  if (!m) return fail(c, HBO_ERR_ARG, std::string(fn) + "model is null");
  if (P <= 0) return fail(c, HBO_ERR_ARG, std::string(fn) + "P must be positive");
  if (steps <= 0) return fail(c, HBO_ERR_ARG, std::string(fn) + "steps must be positive");
  if (!leaves || !x || !adam_m || !adam_v || !bias1 || !bias2 || !losses || !steps_done)
    return fail(c, HBO_ERR_ARG, std::string(fn) + "null array argument (leaves, x, adam_m, adam_v, bias1, bias2, losses, steps_done)");
  if (!batch_counts != !batch_rows) return fail(c, HBO_ERR_ARG, std::string(fn) + "batch_counts and batch_rows are both given or both null");
  if (!(lr == lr) || !(b1 == b1) || !(b2 == b2) || !(adam_eps == adam_eps))
    return fail(c, HBO_ERR_ARG, std::string(fn) + "lr, b1, b2 and adam_eps must be numbers");
  if (int rc = validate_model(c, m)) return rc;
  if (m->n_lengthscale > HBO_MAX_FEATURE_DIM) return fail(c, HBO_ERR_ARG, std::string(fn) + "bad n_lengthscale");
  hbo_grad_layout lay;
  if (int rc = hbo_grad_layout_of(m, &lay)) return fail(c, rc, std::string(fn) + "bad model");
  int32_t ka = -1, kb = -1;
  hbo_grad_layout_kumar_of(m, &ka, &kb);
  std::vector<int> goff(P);
  for (int i = 0; i < P; ++i) {
    const hbo_train_leaf& lf = leaves[i];
    if (lf.warp < HBO_TRAIN_WARP_IDENTITY || lf.warp > HBO_TRAIN_WARP_SQUAREPLUS)
      return fail(c, HBO_ERR_ARG, std::string(fn) + "leaf " + std::to_string(i) + ": unknown warp");
    if (lf.target < HBO_TRAIN_NONE || lf.target > HBO_TRAIN_KUMAR_B)
      return fail(c, HBO_ERR_ARG, std::string(fn) + "leaf " + std::to_string(i) + ": unknown target");
    if (lf.round_f32 != 0 && lf.round_f32 != 1) return fail(c, HBO_ERR_ARG, std::string(fn) + "leaf " + std::to_string(i) + ": round_f32 is 0 or 1");
    if (lf.index < 0 || lf.index >= train_target_size(m, lf))
      return fail(c, HBO_ERR_ARG, std::string(fn) + "leaf " + std::to_string(i) + ": layer / index outside its target");
    goff[i] = train_gradient_offset(m, lay, ka, kb, lf);
    if (lf.target != HBO_TRAIN_NONE && (goff[i] < 0 || goff[i] >= lay.total))
      return fail(c, HBO_ERR_ARG, std::string(fn) + "leaf " + std::to_string(i) + ": the model does not read its target");
  }
  if (!ds) return fail(c, HBO_ERR_ARG, std::string(fn) + "dataset is null");
  const int T = ds->ntasks, D = ds->D, dtype = ds->dtype;
  if (T <= 0) return fail(c, HBO_ERR_ARG, std::string(fn) + "the dataset has no tasks");
  if (m->dtype != dtype || m->input_dim != D) return fail(c, HBO_ERR_ARG, std::string(fn) + "model/dataset dtype or input_dim mismatch");
  // the batch: its task sizes (the same every step), the rows a step consumes, and the order hbo_dataset_subsample keeps its tasks in
  std::vector<int64_t> nd(T);
  int64_t nidx = 0;
  for (int k = 0; k < T; ++k) {
    const int64_t n = ds->tasks[k]->n;
    nd[k] = n;
    if (!batch_counts) continue;
    const int64_t ck = batch_counts[k];
    if (ck == 0 || ck > n) return fail(c, HBO_ERR_ARG, std::string(fn) + "batch_counts[k] must be in 1..n_k (or negative: the whole task)");
    if (ck > 0) { nd[k] = ck; nidx += ck; }
  }
  if (batch_counts) {
    for (int s = 1; s < steps; ++s)
      for (int k = 0; k < T; ++k)
        if ((batch_counts[(size_t)s * T + k] < 0) != (batch_counts[k] < 0) || (batch_counts[k] >= 0 && batch_counts[(size_t)s * T + k] != batch_counts[k]))
          return fail(c, HBO_ERR_ARG, std::string(fn) + "batch_counts must be the same at every step");
    for (int s = 0; s < steps; ++s) {
      int64_t off = (int64_t)s * nidx;
      for (int k = 0; k < T; ++k) {
        if (batch_counts[k] < 0) continue;
        for (int64_t r = 0; r < batch_counts[k]; ++r, ++off)
          if (batch_rows[off] < 0 || batch_rows[off] >= ds->tasks[k]->n) return fail(c, HBO_ERR_ARG, std::string(fn) + "batch_rows: index out of range");
      }
    }
  }
  if (!c) return fail(c, HBO_ERR_ARG, std::string(fn) + "context is null");
  int64_t max_n = 0;
  for (int k = 0; k < T; ++k) max_n = std::max(max_n, nd[k]);
  if (max_n > HBO_TILE) return fail(c, HBO_ERR_UNSUPPORTED, std::string(fn) + "a task of the batch has more than 128 points (only the fused regime runs on the device)");
  if (!c->opt_small_fused) return fail(c, HBO_ERR_UNSUPPORTED, std::string(fn) + "small_fused is off (only the fused regime runs on the device)");
  if (small_eval_lds(dtype) > c->lds_per_block) return fail(c, HBO_ERR_UNSUPPORTED, std::string(fn) + "the device cannot give the single-workgroup evaluation its LDS");

  // ---- step 0: the batch, then everything hbo_objective does, up to the device-side reduction
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  hbo_dataset* batch = ds;
  if (batch_counts) { if (int rc = hbo_dataset_subsample(c, ds, batch_counts, batch_rows, &batch)) return rc; }
  struct BatchGuard {   // (a queued launch may still read the batch: wait before it goes back to the pool)
    hbo_ctx* c; hbo_dataset* b;
    ~BatchGuard() { if (b) { (void)hipStreamSynchronize(c->stream); hbo_dataset_free(c, b); } }
  } guard{c, batch_counts ? batch : nullptr};
  std::vector<double> grad0(std::max(lay.total, 1));
  double nll0 = 0, count0 = 0;
  ShardReq sh{&count0, nullptr};
  ShardOut so;
  if (int rc = objective_local(c, m, batch, HBO_OBJ_NLL, &nll0, nullptr, grad0.data(), &sh, &so)) return rc;
  if (!so.d_red || so.red_count != 2 + lay.total) return fail(c, HBO_ERR_HIP, std::string(fn) + "no reduction buffer");

  // ---- one upload: [leaves | goff | bias1 | bias2 | initial arrays | gather table | rows | x | m | v | halt, steps_done | losses],
  //      then the trace; the copy back takes [x .. trace]
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t es = esize(dtype);
  const int n_ls = m->kernel_id == HBO_KERNEL_DOT ? 0 : m->n_lengthscale, fm = mean_feature_dim(m);
  const bool kumar = is_kumar(m);
  std::vector<int> perm(T);
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return nd[a] > nd[b]; });   // hbo_dataset_subsample's task order
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
  size_t off = 0;
  auto take = [&](size_t b) { const size_t o = off; off += al(b); return o; };
  const size_t o_leaf = take(sizeof(hbo_train_leaf) * P), o_goff = take(sizeof(int) * P);
  const size_t o_b1 = take(sizeof(double) * steps), o_b2 = take(sizeof(double) * steps);
  const size_t o_ls = take(es * std::max(n_ls, 1)), o_lin = take(es * std::max(fm, 1));
  const size_t o_ka = take(es * D), o_kb = take(es * D);
  const size_t o_gt = take(sizeof(GatherTask) * std::max<size_t>(gt.size(), 1));
  const size_t o_rows = take(sizeof(int32_t) * std::max<int64_t>(batch_counts ? nidx * steps : 0, 1));
  const size_t o_x = take(sizeof(double) * P), o_m = take(sizeof(double) * P), o_v = take(sizeof(double) * P);
  const size_t o_int = take(2 * sizeof(int)), o_loss = take(sizeof(double) * steps);
  const size_t up_bytes = off;
  const size_t o_trace = take(x_trace ? sizeof(double) * steps * (size_t)P : 0);
  const size_t total = off;
  std::vector<unsigned char> h(total, 0);
  auto cp = [&](size_t o, const void* src, size_t b) { if (b) memcpy(h.data() + o, src, b); };
  cp(o_leaf, leaves, sizeof(hbo_train_leaf) * P); cp(o_goff, goff.data(), sizeof(int) * P);
  cp(o_b1, bias1, sizeof(double) * steps); cp(o_b2, bias2, sizeof(double) * steps);
  if (n_ls) cp(o_ls, m->lengthscale, es * n_ls);
  if (fm) cp(o_lin, m->linear_kernel, es * fm);
  if (kumar) { cp(o_ka, as_kumar(m)->kumar_a, es * D); cp(o_kb, as_kumar(m)->kumar_b, es * D); }
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
  a.leaves = reinterpret_cast<const hbo_train_leaf*>(d + o_leaf); a.goff = reinterpret_cast<const int*>(d + o_goff); a.P = P;
  a.x = reinterpret_cast<double*>(d + o_x); a.am = reinterpret_cast<double*>(d + o_m); a.av = reinterpret_cast<double*>(d + o_v);
  a.bias1 = reinterpret_cast<const double*>(d + o_b1); a.bias2 = reinterpret_cast<const double*>(d + o_b2);
  a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = adam_eps;
  a.red = so.d_red;
  a.losses = reinterpret_cast<double*>(d + o_loss); a.trace = x_trace ? reinterpret_cast<double*>(d + o_trace) : nullptr;
  a.halt = reinterpret_cast<int*>(d + o_int); a.steps_done = a.halt + 1;
  if (kumar) a.init = *as_kumar(m); else a.init.base = *m;
  a.init.base.lengthscale = d + o_ls; a.init.base.linear_kernel = d + o_lin;
  if (kumar) { a.init.kumar_a = d + o_ka; a.init.kumar_b = d + o_kb; }
  for (int l = 0; l < HBO_MAX_MLP_LAYERS; ++l) { a.init.base.mlp_kernel[l] = nullptr; a.init.base.mlp_bias[l] = nullptr; }
  a.n_ls = n_ls; a.fm = fm;
  for (int l = 0; l < HBO_MAX_MLP_LAYERS; ++l) { a.mlp_w[l] = c->d_mlp_w[l]; a.mlp_b[l] = c->d_mlp_b[l]; }
  a.md = c->d_model;

  const GatherTask* d_gt = reinterpret_cast<const GatherTask*>(d + o_gt);
  const int32_t* d_rows = reinterpret_cast<const int32_t*>(d + o_rows);
  for (int s = 0; s < steps; ++s) {
    if (s > 0) {
      if (!gt.empty()) launch_gather_rows(dtype, d_gt, d_rows + (size_t)s * nidx, (int)gt.size(), max_n, D, st);
      enqueue_fused_forward(c, m, batch, max_n, so.out_stride, true);
      if (int rc = enqueue_backward(c, m, batch, max_n, OBJ_NLL, true)) return rc;
      launch_shard_reduce(batch->d_nll, batch->d_gradout, batch->d_info, T, so.out_stride, so.d_map, batch->d_mlpgrad, so.d_map + so.out_stride,
                          so.nseg, so.d_red, so.red_count, st);
    }
    { ProfScope ps(c, "adam_step", 1);
      hipLaunchKernelGGL(adam_step_kernel, dim3(1), dim3(ADAM_THREADS), 0, st, a, s); }
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(h.data() + o_x, d + o_x, total - o_x, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  prof_collect(c);
  memcpy(x, h.data() + o_x, sizeof(double) * P); memcpy(adam_m, h.data() + o_m, sizeof(double) * P); memcpy(adam_v, h.data() + o_v, sizeof(double) * P);
  memcpy(losses, h.data() + o_loss, sizeof(double) * steps);
  if (x_trace) memcpy(x_trace, h.data() + o_trace, sizeof(double) * steps * (size_t)P);
  *steps_done = reinterpret_cast<const int*>(h.data() + o_int)[1];
  return HBO_OK;
}
