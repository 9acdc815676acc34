// d acquisition / d x_query over the parameter samples of an HGP for caches of ANY n >= 1: acq_small.hip's maths per (sample s, query q),
//   k_i = k(x, X_i),  l = W k,  beta = W^T l,  mu = k.alpha + m(x),  var = k(x, x) - |l|^2,  coef_i = a_mu alpha_i - 2 a_var beta_i,
//   the feature gradient and the linear mean's term,
// as four stream-ordered launches over all pairs.  A phase boundary is a launch boundary: no grid-wide barrier, no wait between
// workgroups, no atomics.  k, l and beta live in an fp64 workspace [S][mc][ldv] (acq_small keeps them in fp64 LDS); W, F and alpha are read
// in the model dtype and every product and sum is fp64.  Sample s works on its own npad_s = n_s rounded up to 128, whatever ldv is.
//   1  acq_blk_k_kernel      grid (ldv / 128, mc, S)         thread i walks the features of row i in order; zeros in n_s <= i < ldv
//   2  acq_blk_fwd_kernel    grid (ldv / 16, ceil(mc / 8), S)   post.hip: tri_matmat_fwd_kernel -- 16 rows per workgroup, four per wave
//   3  acq_blk_trans_kernel  grid (ldv / 64, ceil(mc / 8), S)   post.hip: tri_matmat_trans_kernel -- lane = column, 256 rows of l in LDS per step
//   4  acq_blk_finish_kernel grid (mc, S)                    the sums over the rows in chunks of 256, the scalar step, the gradient
// Every sum runs in an order fixed by (n_s, D) alone and a pair reads nothing another pair writes: a result row does not depend on the
// other queries, its place in a group of eight, the other samples, ldv or how the call was cut into query chunks, and identical calls give
// identical bits.  Entries of W above the diagonal and rows beyond n_s are dropped by a select, never multiplied: the padding of a cache
// and what an earlier call left in the workspace cannot reach a result.
// MLP basis (FEAT != 0; acq_mlp.h, hbo_acq_grad_samples_mlp): one launch in front of the four,
//   0  acq_blk_mlp_kernel    grid (mc, S)                    the forward pass of the pair's query; every layer's activations into the
//                                                            fp64 plane acts [S][mc][ftot]
// launch 1 then reads the pair's query in the kernel's space from that plane and launch 4 reads the activations back for the mean and
// the backward pass: five launches per chunk.
#include "acq_mlp.h"

#include <assert.h>

namespace {
enum { BLK_MC = 8 };   // queries per workgroup of the two triangular products

__device__ __forceinline__ int blk_npad(int n) { return (n + HBO_TILE - 1) / HBO_TILE * HBO_TILE; }
__device__ __forceinline__ int64_t blk_row(const AcqBlockedArgs& b, int s, int64_t ql) { return ((int64_t)s * b.mc + ql) * b.ldv; }

__device__ __forceinline__ double* blk_acts(const AcqBlockedArgs& b, int s, int64_t ql) { return b.acts + ((int64_t)s * b.mc + ql) * b.ftot; }

// ---- 0 (FEAT): the forward pass of query q under sample s's weights, layer after layer into acts[s][q][ftot]
template <typename T>
__global__ __launch_bounds__(256) void acq_blk_mlp_kernel(AcqBlockedArgs b) {
  __shared__ double s_x0[HBO_MAX_FEATURE_DIM], s_act[HBO_MAX_MLP_LAYERS * HBO_MAX_FEATURE_DIM];
  const AcqSmallArgs& a = b.a;
  const int64_t ql = blockIdx.x;
  const int s = blockIdx.y, tid = threadIdx.x;
  if (a.smp[s].bad) return;   // (uniform) nothing of the sample's planes is read
  const T* xq = static_cast<const T*>(a.xq) + (b.q0 + ql) * a.D;
  for (int d = tid; d < a.D; d += 256) s_x0[d] = (double)xq[d];
  __syncthreads();
  acq_mlp_fwd_block<T>(a, s, s_x0, s_act);
  double* out = blk_acts(b, s, ql);
  for (int l = 0, off = 0; l < a.L; off += a.fout[l], ++l)
    if (tid < a.fout[l]) out[off + tid] = s_act[l * HBO_MAX_FEATURE_DIM + tid];
}

// ---- 1: k[s][q][i] = k(x_q, X_i) for i < n_s, zeros up to ldv
template <typename T, int FEAT>
__global__ __launch_bounds__(HBO_TILE) void acq_blk_k_kernel(AcqBlockedArgs b) {
  __shared__ double s_xq[HBO_MAX_FEATURE_DIM], s_il[HBO_MAX_FEATURE_DIM];
  const AcqSmallArgs& a = b.a;
  const int s = blockIdx.z, tid = threadIdx.x;
  const int64_t ql = blockIdx.y;
  const AcqSmallSample& sm = a.smp[s];
  if (sm.bad) return;   // (uniform) the finish kernel writes the NaN rows and reads nothing of the workspace
  const int D = (FEAT & ACQ_FEAT_KERNEL) ? a.fdim : a.D, n = sm.n;   // width of the kernel's space
  const int i = blockIdx.x * HBO_TILE + tid;
  double* kout = b.k + blk_row(b, s, ql);
  if (blockIdx.x * HBO_TILE >= n) { kout[i] = 0.0; return; }   // (uniform) a block of padding
  const double* vec = a.vec + (int64_t)s * (FEAT ? a.fdim + a.mdim : 2 * D);
  if constexpr ((FEAT & ACQ_FEAT_KERNEL) != 0) {
    const double* fq = blk_acts(b, s, ql) + (b.ftot - D);   // the last layer
    for (int d = tid; d < D; d += HBO_TILE) { s_xq[d] = fq[d]; s_il[d] = vec[d]; }
  } else {
    const T* xq = static_cast<const T*>(a.xq) + (b.q0 + ql) * D;
    for (int d = tid; d < D; d += HBO_TILE) { s_xq[d] = (double)xq[d]; s_il[d] = vec[d]; }
  }
  __syncthreads();
  const ExpCoef ec = hbo_exp_coef();
  double u = 0, k = 0;
  if (i < n) {
    const T* Fi = static_cast<const T*>(sm.F) + (int64_t)i * D;
    if (a.kernel_id == HBO_KERNEL_DOT) {
      for (int d = 0; d < D; ++d) u += s_xq[d] * (double)Fi[d];
      k = u * sm.inv_sigma2 + sm.bias2;
    } else {
      for (int d = 0; d < D; ++d) { const double df = (s_xq[d] - (double)Fi[d]) * s_il[d]; u += df * df; }
      k = kfun(a.kernel_id, u, sm.sv, 1.0, 0.0, ec);
    }
  }
  kout[i] = k;
}

// ---- 2: l = W k for MC queries per pass over W.  Rows n_s <= r < npad_s are written as zeros
template <typename T, int MC>
__global__ __launch_bounds__(256) void acq_blk_fwd_kernel(AcqBlockedArgs b) {
  const int s = blockIdx.z;
  const AcqSmallSample& sm = b.a.smp[s];
  const int n = sm.n, npad = blk_npad(n);
  if (sm.bad || (int)blockIdx.x * 16 >= npad) return;   // (uniform)
  const int64_t c0 = (int64_t)blockIdx.y * MC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.x * 16 + wave * 4;
  const T* W = static_cast<const T*>(sm.W);
  const int64_t ld = sm.ld;
  const double* kin = b.k + blk_row(b, s, c0);
  double* lout = b.l + blk_row(b, s, c0);
  double acc[4][MC];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < MC; ++c) acc[r][c] = 0;
  const int rmax = r0 >= n ? -1 : (r0 + 3 < n ? r0 + 3 : n - 1);   // (four rows of padding: no column at all)
  for (int j = lane; j <= rmax; j += 64) {
    double kv[MC];
#pragma unroll
    for (int c = 0; c < MC; ++c) kv[c] = c0 + c < b.mc ? kin[(int64_t)c * b.ldv + j] : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + r;
      const T wv = W[(int64_t)row * ld + j];   // (row < npad_s: inside the cache's W)
      const double w = (j <= row && row < n) ? (double)wv : 0.0;
#pragma unroll
      for (int c = 0; c < MC; ++c) acc[r][c] += w * kv[c];
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < MC; ++c) {
      const double v = wave_sum(acc[r][c]);
      if (lane == 0 && c0 + c < b.mc) lout[(int64_t)c * b.ldv + r0 + r] = v;
    }
}

// ---- 3: beta = W^T l for MC queries per pass over W; columns n_s <= j < npad_s come out as zeros
template <typename T, int MC>
__global__ __launch_bounds__(256) void acq_blk_trans_kernel(AcqBlockedArgs b) {
  __shared__ double red[4][MC][64];
  __shared__ double ls[MC][256];   // l of the current 256 rows (read by every lane: LDS broadcast)
  const int s = blockIdx.z;
  const AcqSmallSample& sm = b.a.smp[s];
  const int n = sm.n, npad = blk_npad(n);
  const int j0 = blockIdx.x * 64;
  if (sm.bad || j0 >= npad) return;   // (uniform)
  const int64_t c0 = (int64_t)blockIdx.y * MC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = j0 + lane;
  const T* W = static_cast<const T*>(sm.W);
  const int64_t ld = sm.ld;
  const double* lin = b.l + blk_row(b, s, c0);
  double acc[MC];
#pragma unroll
  for (int c = 0; c < MC; ++c) acc[c] = 0;
  for (int rc = j0 / 256 * 256; rc < n; rc += 256) {   // the last chunk may be short
    __syncthreads();
#pragma unroll
    for (int c = 0; c < MC; ++c) {
      const int r = rc + threadIdx.x;
      ls[c][threadIdx.x] = (c0 + c < b.mc && r < n) ? lin[(int64_t)c * b.ldv + r] : 0.0;
    }
    __syncthreads();
    // each wave takes 64 rows of the chunk, eight at a time: their loads of W are in flight together
#pragma unroll 2
    for (int g = 0; g < 8; ++g) {
      const int rl = wave * 64 + g * 8;
      T w[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { const int r = rc + rl + u; w[u] = (r < n && r >= j) ? W[(int64_t)r * ld + j] : (T)0; }
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int c = 0; c < MC; ++c) acc[c] += (double)w[u] * ls[c][rl + u];
    }
  }
#pragma unroll
  for (int c = 0; c < MC; ++c) red[wave][c][lane] = acc[c];
  __syncthreads();
  if (wave == 0) {
    double* bout = b.beta + blk_row(b, s, c0);
#pragma unroll
    for (int c = 0; c < MC; ++c)
      if (c0 + c < b.mc) bout[(int64_t)c * b.ldv + j] = ((red[0][c][lane] + red[1][c][lane]) + red[2][c][lane]) + red[3][c][lane];
  }
}

// ---- 4: one workgroup per (sample, query): the sums over the rows, the scalar step, the gradient
//         (STEP: the scalar step, as in acq_small_kernel (kernfun.h: acq_scalar_step))
//         (FEAT: D below is the width of the kernel's space; the activations come back from the plane and acq_mlp_tail ends the pair)
template <typename T, int STEP, int FEAT>
__global__ __launch_bounds__(256) void acq_blk_finish_kernel(AcqBlockedArgs b) {
  __shared__ double s_xq[HBO_MAX_FEATURE_DIM], s_il[HBO_MAX_FEATURE_DIM];
  __shared__ double s_w[256];
  __shared__ double s_acc[256];
  __shared__ double sred[4];
  const AcqSmallArgs& a = b.a;
  const int64_t ql = blockIdx.x, q = b.q0 + ql;
  const int s = blockIdx.y;
  const int tid = threadIdx.x;
  const AcqSmallSample& sm = a.smp[s];
  const int D = (FEAT & ACQ_FEAT_KERNEL) ? a.fdim : a.D, n = sm.n;
  T* acq = static_cast<T*>(a.acq_out) + (int64_t)s * a.M + q;
  double* g = a.grad_out + ((int64_t)s * a.M + q) * a.D;
  if (sm.bad) {   // (uniform) the factor is not positive definite: NaN rows, as hbo_acq_grad
    if (tid == 0) { *acq = (T)NAN; if (a.val64_out) a.val64_out[(int64_t)s * a.M + q] = NAN; }
    for (int d = tid; d < a.D; d += 256) g[d] = NAN;
    return;
  }
  const double* vec = a.vec + (int64_t)s * (FEAT ? a.fdim + a.mdim : 2 * D);
  const T* xq = static_cast<const T*>(a.xq) + q * a.D;
  const T* F = static_cast<const T*>(sm.F);
  const T* al = static_cast<const T*>(sm.alpha);
  const double* kv = b.k + blk_row(b, s, ql);
  const double* lv = b.l + blk_row(b, s, ql);
  const double* bv = b.beta + blk_row(b, s, ql);
  const int kid = a.kernel_id;
  const bool is_dot = (kid == HBO_KERNEL_DOT);
  const double* s_raw = s_xq;   // the raw query; s_xq: the query in the kernel's space
  double* s_act = nullptr;      // FEAT: every layer's activations, as acq_mlp_fwd_block lays them out
  if constexpr (FEAT != 0) {
    __shared__ double s_x0[HBO_MAX_FEATURE_DIM], s_acts[HBO_MAX_MLP_LAYERS * HBO_MAX_FEATURE_DIM];
    const double* in = blk_acts(b, s, ql);
    for (int l = 0, off = 0; l < a.L; off += a.fout[l], ++l)
      if (tid < a.fout[l]) s_acts[l * HBO_MAX_FEATURE_DIM + tid] = in[off + tid];
    for (int d = tid; d < a.D; d += 256) s_x0[d] = (double)xq[d];
    for (int d = tid; d < D; d += 256) s_il[d] = vec[d];
    __syncthreads();
    const double* last = s_acts + (a.L - 1) * HBO_MAX_FEATURE_DIM;
    for (int d = tid; d < D; d += 256) s_xq[d] = (FEAT & ACQ_FEAT_KERNEL) ? last[d] : s_x0[d];
    s_raw = s_x0; s_act = s_acts;
  } else {
    for (int d = tid; d < D; d += 256) { s_xq[d] = (double)xq[d]; s_il[d] = vec[d]; }
  }
  __syncthreads();
  // ---- ka = sum k_i alpha_i, ll = sum l_i^2: chunk by chunk of 256 rows, then over the workgroup
  double pka = 0, pll = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + tid;
    if (i < n) { pka += kv[i] * (double)al[i]; const double li = lv[i]; pll += li * li; }
  }
  const double ka = block_sum(pka, sred);
  const double ll = block_sum(pll, sred);
  // ---- prior at x: k(x, x) and the mean on the raw x (D <= 256: one feature per thread)
  double kqq = sm.sv, mean = 0;
  if (is_dot) kqq = block_sum(tid < D ? s_xq[tid] * s_xq[tid] : 0.0, sred) * sm.inv_sigma2 + sm.bias2;
  if (a.mean_id == HBO_MEAN_CONSTANT) mean = sm.constant;
  else if (a.mean_id == HBO_MEAN_LINEAR) mean = sm.linear_bias + block_sum(tid < a.D ? s_raw[tid] * vec[D + tid] : 0.0, sred);
  if constexpr (FEAT != 0) {
    if (a.mean_id == HBO_MEAN_LINEAR_MLP)   // on the last layer, whoever else reads it
      mean = sm.linear_bias + block_sum(tid < a.mdim ? s_act[(a.L - 1) * HBO_MAX_FEATURE_DIM + tid] * vec[D + tid] : 0.0, sred);
  }
  double amu, avar;
  acq_scalar_step<T, STEP>(a, sm, s, q, ka + mean, kqq - ll, acq, amu, avar);
  if constexpr (STEP == ACQ_STEP_MES) __syncthreads();
  // ---- g_d = sum_i w_i (x_d - X_id | X_id), w_i = coef_i * (dk/du_i * 2 | 1 / sigma^2): FD = pow2 >= D lanes along the features, G groups
  //      over the rows of a chunk; a thread keeps its sum across the chunks and the groups meet once, group by group
  int FD = 1; while (FD < D) FD <<= 1;
  const int G = 256 / FD, grp = tid / FD, dl = tid % FD;
  const ExpCoef ec = hbo_exp_coef();
  const bool need_u = (kid == HBO_KERNEL_MATERN32 || kid == HBO_KERNEL_MATERN52);   // (SE: dk/du = -k / 2)
  double acc = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + tid;
    double w = 0;
    if (i < n) {
      const double coef = amu * (double)al[i] - 2.0 * avar * bv[i];
      if (is_dot) w = coef * sm.inv_sigma2;
      else {
        double u = 0;
        if (need_u) {   // as the k kernel took it
          const T* Fi = F + (int64_t)i * D;
          for (int d = 0; d < D; ++d) { const double df = (s_xq[d] - (double)Fi[d]) * s_il[d]; u += df * df; }
        }
        w = coef * dk_du(kid, u, kv[i], sm.sv, ec) * 2.0;
      }
    }
    __syncthreads();
    s_w[tid] = w;
    __syncthreads();
    const int lim = n - i0 < 256 ? n - i0 : 256;
    if (dl < D)
      for (int ii = grp; ii < lim; ii += G) {
        const double fi = (double)F[(int64_t)(i0 + ii) * D + dl];
        acc += is_dot ? s_w[ii] * fi : s_w[ii] * (s_xq[dl] - fi);
      }
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

template <typename T, int FEAT>
void launch_blocked_f(const AcqBlockedArgs& b, int S, hipStream_t st) {
  const unsigned mc = (unsigned)b.mc, grp = (unsigned)((b.mc + BLK_MC - 1) / BLK_MC);
  if constexpr (FEAT != 0) hipLaunchKernelGGL((acq_blk_mlp_kernel<T>), dim3(mc, S), dim3(256), 0, st, b);
  hipLaunchKernelGGL((acq_blk_k_kernel<T, FEAT>), dim3(b.ldv / HBO_TILE, mc, S), dim3(HBO_TILE), 0, st, b);
  hipLaunchKernelGGL((acq_blk_fwd_kernel<T, BLK_MC>), dim3(b.ldv / 16, grp, S), dim3(256), 0, st, b);
  hipLaunchKernelGGL((acq_blk_trans_kernel<T, BLK_MC>), dim3(b.ldv / 64, grp, S), dim3(256), 0, st, b);
  if constexpr (FEAT == 0) {
    if (b.a.step == ACQ_STEP_MES) { hipLaunchKernelGGL((acq_blk_finish_kernel<T, ACQ_STEP_MES, 0>), dim3(mc, S), dim3(256), 0, st, b); return; }
  }
  if (b.a.step == ACQ_STEP_LOGEI) { hipLaunchKernelGGL((acq_blk_finish_kernel<T, ACQ_STEP_LOGEI, FEAT>), dim3(mc, S), dim3(256), 0, st, b); return; }
  hipLaunchKernelGGL((acq_blk_finish_kernel<T, ACQ_STEP_REGISTRY, FEAT>), dim3(mc, S), dim3(256), 0, st, b);
}
template <typename T>
void launch_blocked_t(const AcqBlockedArgs& b, int S, hipStream_t st) {
  switch (b.a.feat) {
    case 0: launch_blocked_f<T, 0>(b, S, st); break;
    case ACQ_FEAT_KERNEL: launch_blocked_f<T, ACQ_FEAT_KERNEL>(b, S, st); break;
    case ACQ_FEAT_MEAN: launch_blocked_f<T, ACQ_FEAT_MEAN>(b, S, st); break;
    default: launch_blocked_f<T, ACQ_FEAT_KERNEL | ACQ_FEAT_MEAN>(b, S, st); break;
  }
}
}  // namespace

// b.mc <= 65535 (grid.y of the first launch) and S <= 4096: the callers' chunking and checks see to it
// b.a.step == ACQ_STEP_MES needs b.a.feat == 0 (hbo_internal.h: AcqSmallArgs::step); no MES kernel exists for an MLP basis
void launch_acq_blocked(int dtype, const AcqBlockedArgs& b, int S, hipStream_t st) {
  if (b.mc <= 0 || S <= 0 || b.ldv <= 0) return;
  assert(!(b.a.step == ACQ_STEP_MES && b.a.feat != 0) && "the MES step has no instantiation for an MLP basis");
  if (dtype == HBO_F64) launch_blocked_t<double>(b, S, st);
  else launch_blocked_t<float>(b, S, st);
}
