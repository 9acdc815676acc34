// The simulated BO loop (hyperbo/bo_utils/bayesopt.py:136-190) on the device: every iteration of R independent runs from launches that
// are all queued up front (hbo_bo_simulated, at the end of this file), two per step.
//
// The posterior at a FIXED set of columns after one more observation is one more row of forward substitution.  With
// V = L^-1 K(X_obs, C) (rows = observations, columns = the run's M candidates followed by its n0 initial observations), appending
// the observation taken at column p adds the row
//   V[n, j] = (k(c_p, c_j) - sum_{t<n} V[t, p] V[t, j]) / l_pp,   l_pp^2 = k(c_p, c_p) + noise + eps - sum_t V[t, p]^2,
// and z_n = (y_p - mu_p) / l_pp;  then  sum_t V[t, j]^2 += V[n, j]^2  and  mu_j += V[n, j] z_n.  This is gp.predict's solve_triangular +
// sum v^2 (gp.py:295-305) row by row: O(n M) per iteration, no factor L, no W = L^-1, no 128-row limit.  The cross term k(c_p, c_j)
// carries no noise even for j == p (a candidate chosen again is a new noisy observation of the same latent value); the pivot does.
//
// Step l of a run with T = n0 + iters rows:
//   bo_row_kernel(l),    l = 0..T:   thread = column.  l >= 1: row l-1 from the pivot record (column p, l_pp, z); l == 0: the prior.
//                                    n0 <= l < T: the acquisition value of every candidate (post.hip's epilogue in fp64, rounded to the
//                                    model dtype) and one (value, index) arg-max partial per workgroup.  l == T: the final mu / var.
//   bo_select_kernel(l), l = 0..T-1: one workgroup per run.  l < n0: the forced pivot on column M + l; else the arg-max of the partials
//                                    with np.argmax's rule (first NaN, else first of the largest).  Then the statistics of the observed
//                                    y, the next acquisition parameter, l_pp^2 and z, the next pivot record.
// V, sum v^2, mu, z and the y statistics are fp64 for both model dtypes; features stay in the model dtype.  No atomics; every sum runs
// in a fixed order that depends on the run alone, so a run's results do not depend on what shares the call.
#include "api_internal.h"
#include "kernfun.h"

namespace {

// np.argmax's order on (value, index) pairs: any NaN beats any number, among NaNs and among equal values the lower index wins.
// A total order: the result of a reduction does not depend on its shape.  (no candidate: value -inf at index INT_MAX)
__device__ __forceinline__ bool bo_better(double av, int ai, double bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  if (an || bn) return (an && bn) ? ai < bi : an;
  if (av != bv) return av > bv;
  return ai < bi;
}
__device__ __forceinline__ void bo_wave_best(double& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    if (bo_better(ov, oi, v, i)) { v = ov; i = oi; }
  }
}
// best pair of a 256-thread workgroup, valid in thread 0 (sv / si: 4 entries of LDS)
__device__ __forceinline__ void bo_block_best(double& v, int& i, double* sv, int* si) {
  bo_wave_best(v, i);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = i; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < 4; ++w)
      if (bo_better(sv[w], si[w], v, i)) { v = sv[w]; i = si[w]; }
}

template <typename T>
__global__ __launch_bounds__(256) void bo_row_kernel(const BoRunDev* runs, int step) {
  const BoRunDev& r = runs[blockIdx.y];
  const int64_t ncol = r.ncol;
  if (step > r.steps || (int64_t)blockIdx.x * 256 >= ncol) return;   // (uniform per workgroup)
  __shared__ double s_fp[HBO_MAX_FEATURE_DIM], s_il[HBO_MAX_FEATURE_DIM];
  __shared__ double s_pc[256];
  __shared__ double s_bv[4];
  __shared__ int s_bi[4];
  const int tid = threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * 256 + tid;
  const bool live = j < ncol;
  const int64_t jc = live ? j : ncol - 1;   // every load comes from a valid address
  const T* F = static_cast<const T*>(r.F);
  const int fdim = r.fdim;
  double ss, mu;
  double param = r.piv->param;
  if (step == 0) {
    ss = 0.0;
    mu = (double)static_cast<const T*>(r.mu0)[jc];
  } else {
    const BoPivot pv = *r.piv;
    const int64_t p = pv.p;
    const int s = step - 1;   // the row this launch adds
    const bool is_dot = r.kernel_id == HBO_KERNEL_DOT;
    for (int d = tid; d < fdim; d += 256) {
      const double il = is_dot ? 1.0 : r.inv_ls[d];
      s_il[d] = il;
      s_fp[d] = (double)F[p * fdim + d] * il;
    }
    __syncthreads();
    const T* Fj = F + jc * fdim;
    double u = 0, k;
    if (is_dot) {
      for (int d = 0; d < fdim; ++d) u += s_fp[d] * (double)Fj[d];
      k = u * r.inv_sigma2 + r.bias2;
    } else {
      for (int d = 0; d < fdim; ++d) { const double df = s_fp[d] - (double)Fj[d] * s_il[d]; u += df * df; }
      k = kfun(r.kernel_id, u, r.sv, 1.0, 0.0, ExpLit());
    }
    // sum_{t<s} V[t, p] V[t, j]: the pivot column through LDS 256 rows at a time, V's rows read coalesced
    const double* V = r.V;
    double acc = 0;
    for (int t0 = 0; t0 < s; t0 += 256) {
      __syncthreads();
      s_pc[tid] = t0 + tid < s ? V[(int64_t)(t0 + tid) * ncol + p] : 0.0;
      __syncthreads();
      const int cnt = min(256, s - t0);
      const double* Vt = V + (int64_t)t0 * ncol + jc;
#pragma unroll 4
      for (int t = 0; t < cnt; ++t) acc += s_pc[t] * Vt[(int64_t)t * ncol];
    }
    const double v = (k - acc) / pv.l;
    // (threads beyond the last column start from zeros: column ncol - 1 is being written by its own thread in this launch)
    ss = (live ? r.sumsq[j] : 0.0) + v * v;
    mu = (live ? r.mu[j] : 0.0) + v * pv.z;
    param = pv.param;
    if (live) r.V[(int64_t)s * ncol + j] = v;
  }
  if (live) { r.sumsq[j] = ss; r.mu[j] = mu; }
  const double var = (double)static_cast<const T*>(r.kd)[jc] - ss;
  if (step == r.steps) {   // posterior at the pool after the last append, before noise and scale
    if (live && j < r.M) {
      if (r.mu_out) static_cast<T*>(r.mu_out)[j] = (T)mu;
      if (r.var_out) static_cast<T*>(r.var_out)[j] = (T)var;
    }
    return;
  }
  if (step < r.n0 || (int64_t)blockIdx.x * 256 >= r.M) return;   // (uniform) forced pivots take no selection; no candidate in this chunk
  // GP.predict's post-processing (gp.py:607-619), then acfun.py:96-142 -- post.hip: post_epilogue_kernel in fp64 -- rounded to the model dtype
  double bv = -INFINITY;
  int bi = INT_MAX;
  if (j < r.M) {
    const double v2 = (var + r.add_noise) * (step == r.n0 ? r.scale0 : r.scale);
    const double sd = sqrt(v2);
    double val;
    if (r.acq_id == HBO_ACQ_UCB) val = mu + param * sd;
    else {
      const double gamma = (param - mu) / sd;
      val = r.acq_id == HBO_ACQ_PI ? -gamma : ei_over_sd(-gamma) * sd;
    }
    bv = (double)(T)val;
    bi = (int)j;
  }
  bo_block_best(bv, bi, s_bv, s_bi);
  if (tid == 0) { r.part_val[blockIdx.x] = bv; r.part_idx[blockIdx.x] = bi; }
}

template <typename T>
__global__ __launch_bounds__(256) void bo_select_kernel(const BoRunDev* runs, int step) {
  const BoRunDev& r = runs[blockIdx.x];
  if (step >= r.steps) return;
  __shared__ double s_bv[4], sred[4];
  __shared__ int s_bi[4];
  __shared__ int s_p;
  const int tid = threadIdx.x;
  if (step < r.n0) {
    if (tid == 0) s_p = (int)(r.M + step);
  } else {
    double bv = -INFINITY;
    int bi = INT_MAX;
    const int nch = (int)((r.M + 255) / 256);
    for (int c = tid; c < nch; c += 256) {
      const double v = r.part_val[c];
      const int i = r.part_idx[c];
      if (bo_better(v, i, bv, bi)) { bv = v; bi = i; }
    }
    bo_block_best(bv, bi, s_bv, s_bi);
    if (tid == 0) {
      // (every chunk holds a candidate, so the index is one: anything else is a bug, reported as such and kept away from the addresses)
      if ((unsigned)bi >= (unsigned)r.M) { bi = 0; bv = NAN; *r.status = HBO_ERR_HIP; }
      s_p = bi;
      r.sel[step - r.n0] = bi;
      r.acq[step - r.n0] = bv;
    }
  }
  __syncthreads();
  const int p = s_p;
  const double yp = (double)static_cast<const T*>(r.y)[p];
  // np.std of the observed y (pi2's callback, acfun.py:160-166): two passes, as NumPy takes it
  double sd_y = 0.0;
  if (r.param_mode == HBO_BO_PARAM_MAX_PLUS_STD) {
    const int n = step + 1;
    double a = 0;
    for (int t = tid; t < n; t += 256) a += t < step ? r.yobs[t] : yp;
    const double mean = block_sum(a, sred) / n;
    a = 0;
    for (int t = tid; t < n; t += 256) { const double dy = (t < step ? r.yobs[t] : yp) - mean; a += dy * dy; }
    sd_y = sqrt(block_sum(a, sred) / n);
  }
  if (tid == 0) {
    BoPivot pv = *r.piv;
    // np.max: a NaN stays
    const double ymax = step == 0 ? yp : ((pv.ymax != pv.ymax || yp != yp) ? NAN : (yp > pv.ymax ? yp : pv.ymax));
    double param = r.param;
    if (r.param_mode == HBO_BO_PARAM_MAX_PLUS) param = ymax + r.param;
    else if (r.param_mode == HBO_BO_PARAM_MAX_PLUS_STD) param = ymax + r.param * sd_y;
    const double l2 = (double)static_cast<const T*>(r.kd)[p] + r.noise_eps - r.sumsq[p];
    double l = NAN;
    if (l2 > 0.0) l = sqrt(l2);
    else *r.status = HBO_NOT_PD;   // (l2 <= 0 or NaN) the row and everything after it is NaN, as a cache that failed to factorise
    pv.p = p; pv.l = l; pv.z = (yp - r.mu[p]) / l; pv.param = param; pv.ymax = ymax;
    *r.piv = pv;
    r.yobs[step] = yp;
  }
}
}  // namespace

void launch_bo_row(int dtype, const BoRunDev* runs, int R, int64_t max_ncol, int step, hipStream_t st) {
  const dim3 grid((unsigned)((max_ncol + 255) / 256), (unsigned)R);
  if (dtype == HBO_F64) hipLaunchKernelGGL((bo_row_kernel<double>), grid, dim3(256), 0, st, runs, step);
  else hipLaunchKernelGGL((bo_row_kernel<float>), grid, dim3(256), 0, st, runs, step);
}
void launch_bo_select(int dtype, const BoRunDev* runs, int R, int step, hipStream_t st) {
  if (dtype == HBO_F64) hipLaunchKernelGGL((bo_select_kernel<double>), dim3((unsigned)R), dim3(256), 0, st, runs, step);
  else hipLaunchKernelGGL((bo_select_kernel<float>), dim3((unsigned)R), dim3(256), 0, st, runs, step);
}

// ---- the simulated BO loop of R runs in one call (bayesopt.py:136-190; kernels and the recurrence: above) ----
// ONE layout pass over its four device blocks: [in] what goes up, [feat] set-up results (model dtype), [v] the fp64 state, [out] what
// comes back + the arg-max partials.  The head of [in] -- run records, pivots, 1 / lengthscale, models with their MLP weights
// (models_pack) -- is staged in pinned memory; the pools behind it go up straight from the caller's arrays.  From sizes alone: no HIP call.
struct BoSimLayout {
  struct Run { size_t x, y, acts[HBO_MAX_MLP_LAYERS], mu0, kd, V, sumsq, mu, yobs, part_val, part_idx; };
  BlockLayout in, feat, v, out;
  size_t o_runs, o_piv, o_ils, o_md, head_b;   // [in]: the head
  size_t o_acq, o_sel, o_st, st_b, o_mu, o_var;   // [out]: what comes back, in the caller's layout
  std::vector<Run> runs;
  int64_t sum_M = 0, max_ncol = 0, max_steps = 0;
};
static BoSimLayout bo_sim_layout(const hbo_bo_run* runs, int32_t R, int32_t iters, const MlpShape& sh, int D, int fdim, size_t es) {
  BoSimLayout l;
  l.o_runs = l.in.take(sizeof(BoRunDev) * R); l.o_piv = l.in.take(sizeof(BoPivot) * R); l.o_ils = l.in.take(sizeof(double) * fdim * R);
  l.o_md = l.in.take(models_pack_bytes(sh, R)); l.head_b = l.in.off;
  for (int r = 0; r < R; ++r) l.sum_M += runs[r].M;
  l.o_acq = l.out.take(sizeof(double) * (size_t)R * iters); l.o_sel = l.out.take(sizeof(int32_t) * (size_t)R * iters);
  l.o_st = l.out.take(sizeof(int32_t) * R); l.st_b = l.out.off - l.o_st;
  l.o_mu = l.out.take((size_t)l.sum_M * es); l.o_var = l.out.take((size_t)l.sum_M * es);
  l.runs.resize(R);
  for (int r = 0; r < R; ++r) {
    const int64_t ncol = runs[r].M + runs[r].n0, steps = runs[r].n0 + iters;
    BoSimLayout::Run& o = l.runs[r];
    o.x = l.in.take((size_t)ncol * D * es); o.y = l.in.take((size_t)ncol * es);   // the pool, then the initial observations
    for (int k = 0; k < sh.L; ++k) o.acts[k] = l.feat.take((size_t)ncol * sh.fout[k] * es);
    o.mu0 = l.feat.take((size_t)ncol * es); o.kd = l.feat.take((size_t)ncol * es);
    o.V = l.v.take(sizeof(double) * (size_t)steps * ncol); o.sumsq = l.v.take(sizeof(double) * ncol); o.mu = l.v.take(sizeof(double) * ncol);
    o.yobs = l.v.take(sizeof(double) * steps);
    const size_t nch = (size_t)((runs[r].M + 255) / 256);
    o.part_val = l.out.take(sizeof(double) * nch); o.part_idx = l.out.take(sizeof(int32_t) * nch);
    l.max_ncol = std::max(l.max_ncol, ncol); l.max_steps = std::max(l.max_steps, steps);
  }
  return l;
}

// Set-up once per call through the device code every posterior uses (query_features: MLP forward, mean, prior diagonal -- per run, with
// its own model and weights), then the n0 + iters steps of every run as two stream-ordered launches each, all queued before the one
// synchronisation.  The small records go up through the pinned stage, the pools straight from the caller's arrays, and the results
// come back straight into the caller's arrays: no host-side copy of a pool.
extern "C" int hbo_bo_simulated(hbo_ctx* c, const hbo_model* models, const hbo_bo_run* runs, int32_t R, int32_t iters, int32_t* sel_out,
                                double* acq_out, void* mu_out, void* var_out, int32_t* status) {
  if (!models || !runs || !sel_out || !acq_out || !status) return fail(c, HBO_ERR_ARG, "hbo_bo_simulated: null argument");
  if (R <= 0 || R > 4096) return fail(c, HBO_ERR_ARG, "hbo_bo_simulated: 1 <= R <= 4096");
  if (iters <= 0 || iters > 65536) return fail(c, HBO_ERR_ARG, "hbo_bo_simulated: 1 <= iters <= 65536");
  const hbo_model* m0 = &models[0];
  if (int rc = model_family_check(c, "hbo_bo_simulated: ", models, R, "run the host loop")) return rc;
  for (int r = 0; r < R; ++r) {
    const hbo_bo_run& u = runs[r];
    if (u.M <= 0) return fail(c, HBO_ERR_ARG, "hbo_bo_simulated: a run has an empty candidate pool (M <= 0)");
    if (u.n0 < 0 || u.M + u.n0 >= ((int64_t)1 << 31)) return fail(c, HBO_ERR_ARG, "hbo_bo_simulated: need n0 >= 0 and M + n0 < 2^31");
    if (!u.xc || !u.yc || (u.n0 > 0 && (!u.x0 || !u.y0))) return fail(c, HBO_ERR_ARG, "hbo_bo_simulated: a run's pool or observations are null");
    if (u.acq_id < 0 || u.acq_id > HBO_ACQ_UCB) return fail(c, HBO_ERR_ARG, "hbo_bo_simulated: bad acq_id");
    if (u.param_mode < 0 || u.param_mode > HBO_BO_PARAM_MAX_PLUS_STD) return fail(c, HBO_ERR_ARG, "hbo_bo_simulated: bad param_mode");
  }
  const int dtype = m0->dtype, D = m0->input_dim, fdim = feature_dim(m0);
  const size_t es = esize(dtype);
  const bool mlp = needs_mlp(m0);
  const MlpShape sh = mlp_shape(m0);
  const int L = sh.L;
  const BoSimLayout lay = bo_sim_layout(runs, R, iters, sh, D, fdim, es);
  if (!c) return fail(c, HBO_ERR_ARG, "hbo_bo_simulated: ctx is null");
  HIPCHK(c, hipSetDevice(c->device));
  { size_t total = 0;
    HIPCHK(c, hipDeviceTotalMem(&total, c->device));
    if (lay.v.off > total / 2) return fail(c, HBO_ERR_UNSUPPORTED, "hbo_bo_simulated: the runs' workspaces ((n0 + iters) x (M + n0) doubles each) exceed half of the device memory; split the batch"); }
  hipStream_t st = c->stream;
  char* d_in = static_cast<char*>(ws_get(c, WS_BO_IN, lay.in.off));
  char* d_feat = static_cast<char*>(ws_get(c, WS_BO_FEAT, lay.feat.off));
  char* d_v = static_cast<char*>(ws_get(c, WS_BO_V, lay.v.off));
  char* d_out = static_cast<char*>(ws_get(c, WS_BO_OUT, lay.out.off));
  if (!d_in || !d_feat || !d_v || !d_out) return HBO_ERR_HIP;
  // ---- the head of the block that goes up, and the device addresses of everything else
  char* h_in = static_cast<char*>(stage_begin(c, "hbo_bo_simulated: ", lay.head_b));
  if (!h_in) return HBO_ERR_HIP;
  memset(h_in, 0, lay.head_b);
  BoRunDev* h_runs = reinterpret_cast<BoRunDev*>(h_in + lay.o_runs);
  BoPivot* h_piv = reinterpret_cast<BoPivot*>(h_in + lay.o_piv);
  double* h_ils = reinterpret_cast<double*>(h_in + lay.o_ils);
  const ModelDev* h_md = reinterpret_cast<const ModelDev*>(h_in + lay.o_md);
  std::vector<void*> w_dev((size_t)R * HBO_MAX_MLP_LAYERS, nullptr), b_dev((size_t)R * HBO_MAX_MLP_LAYERS, nullptr), acts((size_t)R * HBO_MAX_MLP_LAYERS, nullptr);
  models_pack(h_in + lay.o_md, d_in + lay.o_md, models, R, sh, w_dev.data(), b_dev.data());
  std::vector<const void*> d_x(R);
  size_t moff = 0;
  for (int r = 0; r < R; ++r) {
    const hbo_bo_run& u = runs[r];
    const BoSimLayout::Run& o = lay.runs[r];
    BoRunDev& q = h_runs[r];
    const ModelDev& md = h_md[r];
    memcpy(h_ils + (size_t)r * fdim, md.inv_ls, sizeof(double) * fdim);
    q.inv_ls = reinterpret_cast<const double*>(d_in + lay.o_ils) + (size_t)r * fdim;
    d_x[r] = d_in + o.x;
    q.y = d_in + o.y;
    for (int l = 0; l < L; ++l) acts[(size_t)r * HBO_MAX_MLP_LAYERS + l] = d_feat + o.acts[l];
    q.F = m0->kernel_uses_mlp ? acts[(size_t)r * HBO_MAX_MLP_LAYERS + L - 1] : d_x[r];   // what query_features hands the covariance
    q.mu0 = d_feat + o.mu0; q.kd = d_feat + o.kd;
    q.V = reinterpret_cast<double*>(d_v + o.V); q.sumsq = reinterpret_cast<double*>(d_v + o.sumsq);
    q.mu = reinterpret_cast<double*>(d_v + o.mu); q.yobs = reinterpret_cast<double*>(d_v + o.yobs);
    q.piv = reinterpret_cast<BoPivot*>(d_in + lay.o_piv) + r;
    q.part_val = reinterpret_cast<double*>(d_out + o.part_val); q.part_idx = reinterpret_cast<int32_t*>(d_out + o.part_idx);
    q.acq = reinterpret_cast<double*>(d_out + lay.o_acq) + (size_t)r * iters;
    q.sel = reinterpret_cast<int32_t*>(d_out + lay.o_sel) + (size_t)r * iters;
    q.status = reinterpret_cast<int32_t*>(d_out + lay.o_st) + r;
    q.mu_out = mu_out ? d_out + lay.o_mu + moff * es : nullptr;
    q.var_out = var_out ? d_out + lay.o_var + moff * es : nullptr;
    moff += (size_t)u.M;
    q.M = u.M; q.ncol = u.M + u.n0; q.n0 = (int)u.n0; q.steps = (int)(u.n0 + iters);
    q.fdim = fdim; q.kernel_id = m0->kernel_id; q.acq_id = u.acq_id; q.param_mode = u.param_mode;
    q.param = u.param; q.add_noise = u.add_noise; q.scale0 = u.scale0; q.scale = u.scale;
    q.sv = md.sv; q.inv_sigma2 = 1.0 / (md.dot_sigma * md.dot_sigma); q.bias2 = md.dot_bias * md.dot_bias; q.noise_eps = md.noise + md.eps;
    h_piv[r].p = 0; h_piv[r].l = NAN; h_piv[r].z = NAN; h_piv[r].ymax = NAN;
    h_piv[r].param = u.param_mode == HBO_BO_PARAM_CONST ? u.param : 0.0;   // over an empty y (acfun.py:145-148, 160-166)
  }
  // (from the first queued copy on, an error waits for the stream before it returns: the copies read and write the caller's memory)
  auto bail = [&]() { hipStreamSynchronize(st); };
  HIPCHK_OR(c, stage_upload(c, d_in, h_in, lay.head_b, st), bail());
  for (int r = 0; r < R; ++r) {
    const hbo_bo_run& u = runs[r];
    char* dx = static_cast<char*>(const_cast<void*>(d_x[r]));
    char* dy = static_cast<char*>(const_cast<void*>(h_runs[r].y));
    HIPCHK_OR(c, hipMemcpyAsync(dx, u.xc, (size_t)u.M * D * es, hipMemcpyHostToDevice, st), bail());
    HIPCHK_OR(c, hipMemcpyAsync(dy, u.yc, (size_t)u.M * es, hipMemcpyHostToDevice, st), bail());
    if (u.n0 > 0) {
      HIPCHK_OR(c, hipMemcpyAsync(dx + (size_t)u.M * D * es, u.x0, (size_t)u.n0 * D * es, hipMemcpyHostToDevice, st), bail());
      HIPCHK_OR(c, hipMemcpyAsync(dy + (size_t)u.M * es, u.y0, (size_t)u.n0 * es, hipMemcpyHostToDevice, st), bail());
    }
  }
  HIPCHK_OR(c, hipMemsetAsync(d_out + lay.o_st, 0, lay.st_b, st), bail());
  // ---- set-up: features of all columns, the mean and the prior diagonal at them, per run under its own model
  const ModelDev* d_md = reinterpret_cast<const ModelDev*>(d_in + lay.o_md);
  for (int r = 0; r < R; ++r) {
    const int64_t ncol = runs[r].M + runs[r].n0;
    const BoRunDev& q = h_runs[r];
    query_features(c, &models[r], d_md + r, mlp ? &w_dev[(size_t)r * HBO_MAX_MLP_LAYERS] : nullptr, mlp ? &b_dev[(size_t)r * HBO_MAX_MLP_LAYERS] : nullptr,
                   d_x[r], ncol, &acts[(size_t)r * HBO_MAX_MLP_LAYERS], nullptr, const_cast<void*>(q.mu0), const_cast<void*>(q.kd), st);
  }
  // ---- the steps, all queued: row l (the prior at l = 0, the final posterior at l = steps), then the selection / forced pivot of row l
  const BoRunDev* d_runs = reinterpret_cast<const BoRunDev*>(d_in + lay.o_runs);
  for (int l = 0; l <= (int)lay.max_steps; ++l) {
    launch_bo_row(dtype, d_runs, R, lay.max_ncol, l, st);
    if (l < (int)lay.max_steps) launch_bo_select(dtype, d_runs, R, l, st);
  }
  // ---- the results straight into the caller's arrays (the device block holds them in the caller's layout), one wait
  HIPCHK_OR(c, hipMemcpyAsync(acq_out, d_out + lay.o_acq, sizeof(double) * (size_t)R * iters, hipMemcpyDeviceToHost, st), bail());
  HIPCHK_OR(c, hipMemcpyAsync(sel_out, d_out + lay.o_sel, sizeof(int32_t) * (size_t)R * iters, hipMemcpyDeviceToHost, st), bail());
  HIPCHK_OR(c, hipMemcpyAsync(status, d_out + lay.o_st, sizeof(int32_t) * R, hipMemcpyDeviceToHost, st), bail());
  if (mu_out) HIPCHK_OR(c, hipMemcpyAsync(mu_out, d_out + lay.o_mu, (size_t)lay.sum_M * es, hipMemcpyDeviceToHost, st), bail());
  if (var_out) HIPCHK_OR(c, hipMemcpyAsync(var_out, d_out + lay.o_var, (size_t)lay.sum_M * es, hipMemcpyDeviceToHost, st), bail());
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  for (int r = 0; r < R; ++r) if (status[r] < 0) return fail(c, HBO_ERR_HIP, "hbo_bo_simulated: a selection left the candidate pool (internal error)");
  for (int r = 0; r < R; ++r) if (status[r] != HBO_OK) return HBO_NOT_PD;
  return HBO_OK;
}
