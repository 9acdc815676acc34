// Kumaraswamy input warp of the *_kumar kernels (hyperbo/gp_utils/kernel.py:186-222 with_kumar_bases, basis_functions.py:48-70
// KumarWarp): the base covariance runs on w(x) = 1 - (1 - x^a)^b, per input column, with a, b already squareplus-warped by the
// caller.  A feature map with F = D, so it rides on the feature slot of the pipeline (TaskDesc::F) the way the MLP basis does:
//   forward   one launch for a whole batch of tasks (or one matrix): x -> w(x), and for gradient calls dw/da, dw/db (fp64)
//   backward  d f / d a_d = sum_ij (d f / d K_ij) (d K_ij / d w) (dw/da), contracted per lower tile like grad_feat_kernel (grad.hip)
//             but without materialising d f / d w: every tile writes 2 D partial sums, one ordered finalisation sums tiles and tasks
//             (no float atomics: two identical calls give bit-identical gradients, as the rest of the objective)
//   query     hbo_acq_grad: d acq / d x = d acq / d w * dw/dx
#include "pair_tile.h"

namespace {
constexpr int KC = 8;   // features per LDS chunk of the contraction (six [KC][128] blocks: fp64 fits the 64 KB of static LDS)

// 2^y in fp64 on the project's exp path (kernfun.h hbo_exp): y ln2 is split into p + e exactly enough (fma residual) that the
// rounding of the product does not cost the ~|y| ulp a plain exp(y * ln2) would; exp(p + e) = exp(p) (1 + e), |e| < 2^-52 |p|
__device__ __forceinline__ double kexp2(double y) {
  const double ln2_hi = 6.93147180559945286227e-01, ln2_lo = 2.31904681384629955842e-17;
  const double p = y * ln2_hi;
  const double e = fma(y, ln2_hi, -p) + y * ln2_lo;
  const double E = hbo_exp(p, ExpLit());
  return e == e ? fma(E, e, E) : E;   // (y = -inf: p = -inf, e = NaN -> 0 from hbo_exp)
}
__device__ __forceinline__ float kexp2(float y) { return exp2f(y); }
__device__ __forceinline__ double klog2(double x) { return log2(x); }
__device__ __forceinline__ float klog2(float x) { return log2f(x); }
// x^p as exp2(p log2 x) in the model dtype; exactly p == 1 -> x and p == 0 -> 1 (pow's own conventions, x = 0 included)
template <typename T>
__device__ __forceinline__ T kpow(T x, T p) {
  if (p == (T)1) return x;
  if (p == (T)0) return (T)1;
  return kexp2(p * klog2(x));
}
// w(x) = 1 - (1 - x^a)^b; exactly b == 1 gives u itself (1 - (1 - u) == u in exact arithmetic), so a = b = 1 is the identity
template <typename T>
__device__ __forceinline__ T kumar_w(T x, T a, T b) {
  const T u = kpow(x, a);
  return b == (T)1 ? u : (T)1 - kpow((T)1 - u, b);
}
// v = 1 - x^a for the derivatives, without the cancellation of 1 - u near x = 1: -expm1(a ln x) is good to a few ulp of v itself
// (1 - u is off by an ulp of 1, which v^(b-1) with b < 1 turns into anything up to inf once v is of that size).  a == 1: 1 - x, exact
__device__ __forceinline__ double kumar_v(double x, double a, double lx) { return a == 1.0 ? 1.0 - x : 0.0 - expm1(a * lx); }
__device__ __forceinline__ float kumar_v(float x, float a, float lx) { return a == 1.f ? 1.f - x : 0.f - expm1f(a * lx); }
// dw/da = b v^(b-1) u ln x, dw/db = -v^b ln v (u = x^a, v = 1 - u), in fp64; 0 at x = 0 and x = 1 (their limits), so that 0 ln 0
// never reaches a sum.  ln v: log1p(-u) while u < 1/2 (v near 1), ln of kumar_v above.  Outside [0, 1] the formula's NaN goes through.
__device__ __forceinline__ void kumar_dab(double x, double a, double b, double& ha, double& hb) {
  ha = 0.0; hb = 0.0;
  if (x == 0.0 || x == 1.0) return;
  const double lx = log(x);
  const double u = a == 1.0 ? x : exp(a * lx);
  const double lv = u < 0.5 ? log1p(-u) : log(kumar_v(x, a, lx));
  if (lv == -INFINITY) return;
  const double vb1 = b == 1.0 ? 1.0 : exp((b - 1.0) * lv);
  ha = b * vb1 * u * lx;
  hb = -exp(b * lv) * lv;
}

template <typename T>
__global__ void kumar_forward_kernel(const TaskDesc* __restrict__ tasks, const T* x, T* w, double* h, int64_t n, int D,
                                     const ModelDev* __restrict__ md) {
  if (tasks) {
    const TaskDesc& t = tasks[blockIdx.y];
    x = static_cast<const T*>(t.X); w = static_cast<T*>(const_cast<void*>(t.F)); h = t.kh; n = t.n;
  }
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * D) return;
  const int d = (int)(idx % D);
  const T xv = x[idx];
  w[idx] = kumar_w(xv, (T)md->kumar_a[d], (T)md->kumar_b[d]);
  if (h) {
    double ha, hb;
    kumar_dab((double)xv, md->kumar_a[d], md->kumar_b[d], ha, hb);
    h[idx] = ha; h[n * D + idx] = hb;
  }
}

// one lower tile (ti, tj) of one task: the G_ij * dk/du of grad_feat_kernel (the same pt_g_dkdu of pair_tile.h), then per feature d
//   SE / Matern: c_d sum_ij g_ij (fs_i - fs_j)_d (h_i - [off-diagonal] h_j)_d,   c_d = 4 / ls_d
//   dot:         c_d sum_ij G_ij (f_j h_i + [off-diagonal] f_i h_j)_d,          c_d = 2 / sigma^2
// -- what grad_feat_kernel adds to dF for this tile, multiplied by h = dw/da (dw/db) and summed over its rows.  Wave shuffles, then
// the four waves in order: a fixed summation order.  partials[(task * max_nblk^2 + ti * max_nblk + tj) * 2D + {d, D + d}]
template <typename T, int KID>
__global__ __launch_bounds__(256) void kumar_contract_kernel(const TaskDesc* tasks, const ModelDev* __restrict__ md, int fdim, int obj,
                                                             int max_nblk, double* __restrict__ partials) {
  constexpr int P1 = 2 * DC * SXS * (int)sizeof(T);
  constexpr int P2 = 2 * KC * SXS * (int)sizeof(T) + 4 * KC * SXS * (int)sizeof(double);
  __shared__ __attribute__((aligned(16))) unsigned char lds[P1 > P2 ? P1 : P2];
  __shared__ double red[4][2 * KC];
  const TaskDesc& t = tasks[blockIdx.z];
  const int ti = blockIdx.x, tj = blockIdx.y;
  if (ti >= t.nblk || tj > ti) return;
  constexpr bool is_dot = (KID == HBO_KERNEL_DOT);
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t r0 = (int64_t)ti * HBO_TILE, c0 = (int64_t)tj * HBO_TILE;
  const T* F = static_cast<const T*>(t.F);
  int64_t vstride; int nvec;
  const T* sv_ = outer_vecs<T>(t, obj, vstride, nvec);
  const int64_t n = t.n;
  T* sA = reinterpret_cast<T*>(lds);
  T* sB = sA + DC * SXS;

  T acc[8][8];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[a][b] = (T)0;
  pt_accumulate<T, 8, is_dot>(acc, sA, sB, F, n, F, n, fdim, r0, c0, md->inv_ls, tid);
  pt_g_dkdu<T, KID>(acc, t, md, obj == OBJ_EUC, sv_, vstride, nvec, r0, c0, tx, ty);
  const bool offdiag = (ti != tj);
  // phase 2 staging: scaled features and dw/da, dw/db of the tile's rows (A) and columns (B), KC features at a time
  T* fA = reinterpret_cast<T*>(lds);
  T* fB = fA + KC * SXS;
  double* hA = reinterpret_cast<double*>(lds + 2 * KC * SXS * sizeof(T));   // [2][KC][SXS]: dw/da, dw/db
  double* hB = hA + 2 * KC * SXS;
  const double* kh = t.kh;
  double* out = partials + ((int64_t)blockIdx.z * max_nblk * max_nblk + (int64_t)ti * max_nblk + tj) * 2 * fdim;
  for (int d0 = 0; d0 < fdim; d0 += KC) {
    __syncthreads();
    for (int e = tid; e < KC * HBO_TILE; e += 256) {
      const int dd = e % KC, rr = e / KC, d = d0 + dd;
      const bool dok = d < fdim;
      const T sc = (!is_dot && dok) ? (T)md->inv_ls[d] : (T)1;
      const int64_t ra = r0 + rr, rb = c0 + rr;
      const bool oka = dok && ra < n, okb = dok && rb < n;
      fA[dd * SXS + rr] = oka ? F[ra * fdim + d] * sc : (T)0;
      fB[dd * SXS + rr] = okb ? F[rb * fdim + d] * sc : (T)0;
      hA[dd * SXS + rr] = oka ? kh[ra * fdim + d] : 0.0;
      hA[(KC + dd) * SXS + rr] = oka ? kh[n * fdim + ra * fdim + d] : 0.0;
      hB[dd * SXS + rr] = okb ? kh[rb * fdim + d] : 0.0;
      hB[(KC + dd) * SXS + rr] = okb ? kh[n * fdim + rb * fdim + d] : 0.0;
    }
    __syncthreads();
    const int dlim = (fdim - d0) < KC ? (fdim - d0) : KC;
    for (int dd = 0; dd < dlim; ++dd) {
      double sa = 0, sb = 0;
#pragma unroll
      for (int a = 0; a < 8; ++a) {
        const int ra = ty + 16 * a;
        const T av = fA[dd * SXS + ra];
        const double haa = hA[dd * SXS + ra], hab = hA[(KC + dd) * SXS + ra];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int cb = pt_col<T>(tx, q);
          const T bv = fB[dd * SXS + cb];
          const double hba = offdiag ? hB[dd * SXS + cb] : 0.0, hbb = offdiag ? hB[(KC + dd) * SXS + cb] : 0.0;
          if (is_dot) {
            const double wr = (double)(acc[a][q] * bv), wc = offdiag ? (double)(acc[a][q] * av) : 0.0;
            sa += wr * haa + wc * hba; sb += wr * hab + wc * hbb;
          } else {
            const double w = (double)(acc[a][q] * (av - bv));
            sa += w * (haa - hba); sb += w * (hab - hbb);
          }
        }
      }
      sa = wave_sum(sa); sb = wave_sum(sb);
      if ((tid & 63) == 0) { red[tid >> 6][dd] = sa; red[tid >> 6][KC + dd] = sb; }
    }
    __syncthreads();
    if (tid < 2 * KC) {
      const int dd = tid % KC, d = d0 + dd;
      if (d < fdim) {
        const double cd = is_dot ? 2.0 / (md->dot_sigma * md->dot_sigma) : 4.0 * md->inv_ls[d];
        const double v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        out[(tid < KC ? 0 : fdim) + d] = cd * v;
      }
    }
  }
}

// out[j] = sum over tasks (in order) of scale_task * sum over the task's lower tiles of partials[..][j]; one block per j, a fixed
// tile-to-thread assignment and block_sum's fixed tree.  EUC: the kernel part of its gradient was built with the un-normalised G
// (as scale_dF_kernel divides dF by |C0 - K1|_F)
__global__ __launch_bounds__(256) void kumar_finalize_kernel(const TaskDesc* tasks, int ntasks, int max_nblk, int D2, int obj,
                                                             const double* __restrict__ partials, double* __restrict__ out) {
  __shared__ double sred[4];
  const int j = blockIdx.x;
  const int64_t nt = (int64_t)max_nblk * max_nblk;
  double total = 0;
  for (int k = 0; k < ntasks; ++k) {
    const TaskDesc& t = tasks[k];
    double s = 0;
    for (int64_t e = threadIdx.x; e < nt; e += 256) {
      const int ti = (int)(e / max_nblk), tj = (int)(e % max_nblk);
      if (ti < t.nblk && tj <= ti) s += partials[(k * nt + e) * D2 + j];
    }
    s = block_sum(s, sred);
    if (obj == OBJ_EUC) { const double f = t.fnorm[0]; s *= (f > 0 ? 1.0 / f : 0.0); }
    total += s;
  }
  if (threadIdx.x == 0) out[j] = total;
}

template <typename T>
__global__ void kumar_chain_dx_kernel(const T* __restrict__ xq, int64_t M, int D, const ModelDev* __restrict__ md,
                                      const double* __restrict__ gf, double* __restrict__ gx) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= M * D) return;
  const int d = (int)(idx % D);
  const T a = (T)md->kumar_a[d], b = (T)md->kumar_b[d], x = xq[idx];
  const T v = kumar_v(x, a, log(x));
  const T dwdx = a * b * kpow(x, a - (T)1) * kpow(v, b - (T)1);
  gx[idx] = gf[idx] * (double)dwdx;
}
}  // namespace

void launch_kumar_forward(int dtype, const TaskDesc* tasks, int ntasks, int64_t max_n, const void* x, void* w, double* h, int64_t n, int D,
                          const ModelDev* md, hipStream_t st) {
  const int64_t rows = tasks ? max_n : n;
  if (rows <= 0 || D <= 0 || (tasks && ntasks <= 0)) return;
  const dim3 grid((unsigned)((rows * D + 255) / 256), tasks ? (unsigned)ntasks : 1u);
  dispatch_dtype(dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    hipLaunchKernelGGL(kumar_forward_kernel<T>, grid, dim3(256), 0, st, tasks, (const T*)x, (T*)w, h, n, D, md);
  });
}

void launch_kumar_grad(int dtype, const TaskDesc* tasks, int ntasks, int max_nblk, const ModelDev* md, int kernel_id, int D, int obj,
                       double* partials, double* out, hipStream_t st) {
  if (ntasks <= 0 || max_nblk <= 0) return;
  const dim3 grid(max_nblk, max_nblk, ntasks);
  dispatch_dtype(dtype, [&](auto tag) {
    dispatch_kid(kernel_id, [&](auto kid) {
      hipLaunchKernelGGL((kumar_contract_kernel<typename decltype(tag)::type, decltype(kid)::value>), grid, dim3(256), 0, st, tasks, md, D, obj, max_nblk, partials);
    });
  });
  hipLaunchKernelGGL(kumar_finalize_kernel, dim3(2 * D), dim3(256), 0, st, tasks, ntasks, max_nblk, 2 * D, obj, partials, out);
}

void launch_kumar_chain_dx(int dtype, const void* xq, int64_t M, int D, const ModelDev* md, const double* gf, double* gx, hipStream_t st) {
  if (M <= 0) return;
  const dim3 grid((unsigned)((M * D + 255) / 256));
  dispatch_dtype(dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    hipLaunchKernelGGL(kumar_chain_dx_kernel<T>, grid, dim3(256), 0, st, (const T*)xq, M, D, md, gf, gx);
  });
}
