// The simulated BO loop (hyperbo/bo_utils/bayesopt.py:136-190) on the device: every iteration of R independent runs from launches that
// are all queued up front (hbo_bo_simulated, cache.hip), two per step.
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
