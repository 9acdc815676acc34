// d acquisition / d x_query over the parameter samples of an HGP in ONE launch, for caches of n <= 128 observations (one 128-block):
// what bayesopt()'s inner L-BFGS-B asks for dozens of times per BO iteration (bayesopt.py:116-125 over acfun.py:72-82).  The per-sample
// path (acq_grad.hip: hbo_acq_grad) is about eight latency-bound launches and a host round trip per sample; here one workgroup owns one
// (sample, query) pair and does all of post.hip: acq_grad_kernel's maths itself, from the finished cache of that sample:
//   k_i = k(x, X_i),  l = W k,  beta = W^T l,  mu = k.alpha + m(x),  var = k(x, x) - |l|^2,  coef_i = a_mu alpha_i - 2 a_var beta_i,
//   SE / Matern: g_d = sum_i coef_i dk/du_i 2 (x_d - X_id) / ls_d^2;  dot: g = sum_i coef_i X_i / sigma^2 + a_var 2 x / sigma^2;
//   a linear mean adds a_mu lin_w.
// Every sum is fp64 in a fixed order (no atomics), and a pair reads nothing another pair writes: a row of the result does not depend
// on which samples or queries share the launch.  The scalar functions are those of kernfun.h.
#include "acq_mlp.h"

#include <assert.h>

namespace {
// STEP, the scalar step (hbo_internal.h: ACQ_STEP_*; kernfun.h: acq_scalar_step): acq_scalars by a.acq_id; mes_scalars_block over the
// sample's K maxima (a.ystar; hbo_mes_grad_samples); logei_scalars against the sample's target (sm.param; hbo_logei_grad_samples)
// FEAT (acq_mlp.h; hbo_acq_grad_samples_mlp): 0 -- no MLP basis; otherwise ACQ_FEAT_KERNEL | ACQ_FEAT_MEAN, who reads the last layer.
// The pair's workgroup then runs the forward pass first, works in the kernel's own space of width D = fdim below, takes the mean in
// the mean's own space and ends with the backward pass (acq_mlp_tail).
template <typename T, int STEP, int FEAT>
__global__ __launch_bounds__(256) void acq_small_kernel(AcqSmallArgs a) {
  __shared__ double s_xq[HBO_MAX_FEATURE_DIM], s_il[HBO_MAX_FEATURE_DIM];
  __shared__ double s_k[HBO_TILE], s_l[HBO_TILE], s_w[HBO_TILE];
  __shared__ double s_acc[256];   // beta's two row-parity partials, then the gradient's partials per row group
  __shared__ double sred[4];
  const int64_t q = blockIdx.x;
  const int s = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const AcqSmallSample& sm = a.smp[s];
  const int n = sm.n;
  const int D = (FEAT & ACQ_FEAT_KERNEL) ? a.fdim : a.D;   // width of the kernel's space
  T* acq = static_cast<T*>(a.acq_out) + (int64_t)s * a.M + q;
  double* g = a.grad_out + ((int64_t)s * a.M + q) * a.D;
  if (sm.bad) {   // (uniform) the factor is not positive definite: NaN rows, as hbo_acq_grad
    if (tid == 0) { *acq = (T)NAN; if (a.val64_out) a.val64_out[(int64_t)s * a.M + q] = NAN; }
    for (int d = tid; d < a.D; d += 256) g[d] = NAN;
    return;
  }
  const double* vec = a.vec + (int64_t)s * (FEAT ? a.fdim + a.mdim : 2 * D);   // 1 / lengthscale [D], linear mean weights [D | mean width]
  const T* xq = static_cast<const T*>(a.xq) + q * a.D;
  const T* F = static_cast<const T*>(sm.F);
  const T* W = static_cast<const T*>(sm.W);
  const T* al = static_cast<const T*>(sm.alpha);
  const int64_t ld = sm.ld;
  const int kid = a.kernel_id;
  const bool is_dot = (kid == HBO_KERNEL_DOT);
  const double* s_raw = s_xq;   // the raw query; s_xq: the query in the kernel's space
  double* s_act = nullptr;      // FEAT: every layer's activations
  if constexpr (FEAT != 0) {
    __shared__ double s_x0[HBO_MAX_FEATURE_DIM], s_acts[HBO_MAX_MLP_LAYERS * HBO_MAX_FEATURE_DIM];
    for (int d = tid; d < a.D; d += 256) s_x0[d] = (double)xq[d];
    for (int d = tid; d < D; d += 256) s_il[d] = vec[d];
    __syncthreads();
    acq_mlp_fwd_block<T>(a, s, s_x0, s_acts);
    const double* last = s_acts + (a.L - 1) * HBO_MAX_FEATURE_DIM;
    for (int d = tid; d < D; d += 256) s_xq[d] = (FEAT & ACQ_FEAT_KERNEL) ? last[d] : s_x0[d];
    s_raw = s_x0; s_act = s_acts;
  } else {
    for (int d = tid; d < D; d += 256) { s_xq[d] = (double)xq[d]; s_il[d] = vec[d]; }
  }
  __syncthreads();
  const ExpCoef ec = hbo_exp_coef();
  // ---- k_i = k(x, X_i): thread i walks the features of row i in order
  double u = 0, k = 0, ai = 0;
  if (tid < n) {
    const T* Fi = F + (int64_t)tid * D;
    if (is_dot) {
      for (int d = 0; d < D; ++d) u += s_xq[d] * (double)Fi[d];
      k = u * sm.inv_sigma2 + sm.bias2;
    } else {
      for (int d = 0; d < D; ++d) { const double df = (s_xq[d] - (double)Fi[d]) * s_il[d]; u += df * df; }
      k = kfun(kid, u, sm.sv, 1.0, 0.0, ec);
    }
    ai = (double)al[tid];
  }
  if (tid < HBO_TILE) s_k[tid] = k;   // (zeros beyond n)
  // ---- prior at x: k(x, x) and the mean on the raw x (D <= 256: one feature per thread)
  double kqq = sm.sv, mean = 0;
  if (is_dot) kqq = block_sum(tid < D ? s_xq[tid] * s_xq[tid] : 0.0, sred) * sm.inv_sigma2 + sm.bias2;
  if (a.mean_id == HBO_MEAN_CONSTANT) mean = sm.constant;
  else if (a.mean_id == HBO_MEAN_LINEAR) mean = sm.linear_bias + block_sum(tid < a.D ? s_raw[tid] * vec[D + tid] : 0.0, sred);
  if constexpr (FEAT != 0) {
    if (a.mean_id == HBO_MEAN_LINEAR_MLP)   // on the last layer, whoever else reads it
      mean = sm.linear_bias + block_sum(tid < a.mdim ? s_act[(a.L - 1) * HBO_MAX_FEATURE_DIM + tid] * vec[D + tid] : 0.0, sred);
  }
  __syncthreads();
  // ---- l = W k: a wave per row, lanes along the row (two columns each); four rows of loads in flight.  Every load comes from a valid
  //      address (row clamped) and entries above the diagonal are dropped by a select, never multiplied
  for (int r0 = wave; r0 < n; r0 += 16) {
    double p[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int r = r0 + 4 * b, rc = r < n ? r : n - 1;
      const T w0 = W[rc * ld + lane], w1 = W[rc * ld + lane + 64];
      p[b] = (lane <= r ? (double)w0 : 0.0) * s_k[lane] + (lane + 64 <= r ? (double)w1 : 0.0) * s_k[lane + 64];
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const double v = wave_sum(p[b]);
      if (lane == 0 && r0 + 4 * b < n) s_l[r0 + 4 * b] = v;
    }
  }
  __syncthreads();
  const double li = tid < n ? s_l[tid] : 0.0;
  const double ka = block_sum(k * ai, sred);   // (k = ai = 0 beyond n)
  const double ll = block_sum(li * li, sred);
  // ---- beta = W^T l: lane = column (the row reads coalesce), the rows of each parity on one half of the workgroup
  {
    const int j = tid & (HBO_TILE - 1), h = tid >> 7;
    double b = 0;
    if (j < n) {
#pragma unroll 4
      for (int r = j + ((j & 1) != h); r < n; r += 2) b += (double)W[r * ld + j] * s_l[r];
    }
    s_acc[tid] = b;
  }
  double amu, avar;
  acq_scalar_step<T, STEP>(a, sm, s, q, ka + mean, kqq - ll, acq, amu, avar);
  if constexpr (STEP == ACQ_STEP_MES) __syncthreads();   // (s_acc is read next, and mes_scalars_block leaves without a barrier when v2 <= 0)
  // ---- w_i = coef_i * (dk/du_i * 2 | 1 / sigma^2)
  if (tid < n) {
    const double beta = s_acc[tid] + s_acc[HBO_TILE + tid];
    const double coef = amu * ai - 2.0 * avar * beta;
    s_w[tid] = is_dot ? coef * sm.inv_sigma2 : coef * dk_du(kid, u, k, sm.sv, ec) * 2.0;
  }
  __syncthreads();
  // ---- g_d = sum_i w_i (x_d - X_id | X_id): FD = pow2 >= D lanes along the features, G groups over the rows, summed group by group
  int FD = 1; while (FD < D) FD <<= 1;
  const int G = 256 / FD, grp = tid / FD, dl = tid % FD;
  double acc = 0;
  if (dl < D)
    for (int i = grp; i < n; i += G) {
      const double fi = (double)F[(int64_t)i * D + dl];
      acc += is_dot ? s_w[i] * fi : s_w[i] * (s_xq[dl] - fi);
    }
  s_acc[tid] = acc;
  __syncthreads();
  if (grp == 0 && dl < D) {
    double r = 0;
    for (int gg = 0; gg < G; ++gg) r += s_acc[gg * FD + dl];
    if (is_dot) r += avar * 2.0 * s_xq[dl] * sm.inv_sigma2;
    else r *= s_il[dl] * s_il[dl];
    if constexpr (FEAT == 0) {
      if (a.mean_id == HBO_MEAN_LINEAR) r += amu * vec[D + dl];
      g[dl] = r;
    } else {
      s_acc[dl] = r;   // the gradient in the kernel's space (thread dl of group 0 has read its column of s_acc, and only it did)
    }
  }
  if constexpr (FEAT != 0) {
    __shared__ double s_gk[HBO_MAX_FEATURE_DIM], s_top[HBO_MAX_FEATURE_DIM], s_tmp[HBO_MAX_FEATURE_DIM];
    __syncthreads();
    if (tid < D) s_gk[tid] = s_acc[tid];
    acq_mlp_tail<T, FEAT>(a, s, s_act, s_gk, vec + D, amu, s_top, s_tmp, g);
  }
}
template <typename T, int STEP>
void launch_small_f(const AcqSmallArgs& a, const dim3& grid, hipStream_t st) {
  switch (a.feat) {
    case 0: hipLaunchKernelGGL((acq_small_kernel<T, STEP, 0>), grid, dim3(256), 0, st, a); break;
    case ACQ_FEAT_KERNEL: hipLaunchKernelGGL((acq_small_kernel<T, STEP, ACQ_FEAT_KERNEL>), grid, dim3(256), 0, st, a); break;
    case ACQ_FEAT_MEAN: hipLaunchKernelGGL((acq_small_kernel<T, STEP, ACQ_FEAT_MEAN>), grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL((acq_small_kernel<T, STEP, ACQ_FEAT_KERNEL | ACQ_FEAT_MEAN>), grid, dim3(256), 0, st, a); break;
  }
}
template <typename T>
void launch_small_t(const AcqSmallArgs& a, const dim3& grid, hipStream_t st) {
  switch (a.step) {
    case ACQ_STEP_MES: hipLaunchKernelGGL((acq_small_kernel<T, ACQ_STEP_MES, 0>), grid, dim3(256), 0, st, a); break;
    case ACQ_STEP_LOGEI: launch_small_f<T, ACQ_STEP_LOGEI>(a, grid, st); break;
    default: launch_small_f<T, ACQ_STEP_REGISTRY>(a, grid, st); break;
  }
}
}  // namespace

// a.step == ACQ_STEP_MES needs a.feat == 0 (hbo_internal.h: AcqSmallArgs::step); no MES kernel exists for an MLP basis
void launch_acq_small(int dtype, const AcqSmallArgs& a, int S, hipStream_t st) {
  if (a.M <= 0 || S <= 0) return;
  assert(!(a.step == ACQ_STEP_MES && a.feat != 0) && "the MES step has no instantiation for an MLP basis");
  const dim3 grid((unsigned)a.M, (unsigned)S);
  if (dtype == HBO_F64) launch_small_t<double>(a, grid, st);
  else launch_small_t<float>(a, grid, st);
}
