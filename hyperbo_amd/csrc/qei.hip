// Batch (q-point) expected improvement, qEI (include/hbo.h has the formulas): the kernel that couples the q points of a batch, and the
// entry points hbo_qei_grad_samples and hbo_qei_maximize over it.  One 256-thread workgroup owns one (batch, sample) pair on grid (M, S),
// for finished caches of n <= 128 observations (the range of acq_small.hip), and reads its sample's W = L^-1 once for all q points:
//   1  the q points and 1 / lengthscale to LDS; k_j = k(x_j, X) (thread i walks row X_i for all j), the prior block k(x_j, x_l), m(x_j)
//   2  l_j = W k_j and mu_j = k_j . alpha + m(x_j): a wave per row of W, lanes along the row (acq_small.hip's load pattern: the row is
//      clamped, entries above the diagonal are dropped by a select and never multiplied), the row kept in registers for the q dot
//      products, alpha riding as row n;  beta_j = W^T l_j, lane = column, the rows of each parity on one half of the workgroup
//   3  Sigma' = (k(x_j, x_l) - l_j . l_l + add_noise [j == l]) scale and its lower Cholesky factor C, right-looking, column by column
//      (pivot test !(p > 0): the pair's value and gradient are NaN)
//   4  thread b takes base samples b, b + 256, ...: f_bj = mu_j + sum_{l<=j} C_jl z_bl, the lowest arg max j*_b and imp_b > 0 go to LDS,
//      the value is a block_sum of the per-thread partials;  mubar_j and Cbar_jl are summed in rising b by the thread that owns (j, l)
//   5  P = tril(C^T Cbar) with its diagonal halved, Y = P C^-1 (a thread per row), Sbar = C^-T Y (a thread per column),
//      G = scale (Sbar + Sbar^T) / 2
//   6  w_ji = (mubar_j alpha_i - 2 sum_l G_jl beta_l[i]) (2 dk/du_ji | 1 / sigma^2), then the gradient rows as acq_small.hip forms
//      them: FD lanes along the q * D coordinates, groups over the rows of X, summed group by group; the coupling terms
//      2 sum_{l != j} G_jl dk(x_j, x_l)/dx_j (dot product: 2 / sigma^2 sum_l G_jl x_l, the G_jj term included) and mubar_j dm/dx_j
// Every product and sum is fp64 whatever the model dtype (X, W, alpha and the points are read in it); no atomics, every sum in an order
// fixed by (n, D, q, B): a pair does not depend on what shares the launch, and identical launches are bit-identical.
// LDS (dynamic, hipFuncSetAttribute): doubles  q (D | 1) + D + 3 q 129 + 128 + 4 * 272 + 32 + 260 + ceil(B / 2):
//   q = 4, D = 8, B = 256: 25.2 KB;  q = 16, D = 8, B = 256: 62.3 KB;  the largest call (q = 16, D = 256, B = 1024): 98.3 KB of the 160.
// k is dead once l is there -- beta takes its place -- and the k-derivative factors become the weights w in place: three [q][129] arrays.
// Out of scope (refused before any device work): caches of n > 128 (a blocked route in the manner of acq_blocked.hip), MLP bases,
// Kumaraswamy warps, the prior branch.
#include "kernfun.h"
#include "acq_opt_host.h"

namespace {
enum { QEI_LDR = HBO_TILE + 1, QEI_QS = HBO_QEI_MAX_Q + 1, QEI_QQ = HBO_QEI_MAX_Q * QEI_QS };

struct QeiArgs {
  const AcqSmallSample* smp; const double* vec;   // [S] records (param: the sample's target), [S][2 D]: 1 / lengthscale, linear mean weights
  const void* xq;                                 // [M][q][D] model dtype
  const double* z;                                // [B][q] base samples
  double* val_out; double* grad_out;              // [S][M], [S][M][q][D]
  int64_t M;
  int D, q, B, kernel_id, mean_id;
  double scale;
};

size_t qei_lds_doubles(int q, int D, int B) {
  return (size_t)q * (D | 1) + D + 3 * (size_t)q * QEI_LDR + HBO_TILE + 4 * QEI_QQ + 2 * HBO_QEI_MAX_Q + 256 + 4 + (size_t)(B + 1) / 2;
}

// QP: q rounded up to a power of two, the length of the per-thread register arrays
template <typename T, int QP>
__global__ __launch_bounds__(256) void qei_kernel(QeiArgs a) {
  extern __shared__ double qei_lds[];
  const int q = a.q, D = a.D, B = a.B, XS = D | 1, LDR = QEI_LDR, QS = QEI_QS;
  double* s_x = qei_lds;                    // [q][XS] the batch
  double* s_il = s_x + q * XS;              // [D] 1 / lengthscale
  double* s_A = s_il + D;                   // [q][LDR] k, then beta
  double* s_L = s_A + q * LDR;              // [q][LDR] l
  double* s_W = s_L + q * LDR;              // [q][LDR] 2 dk/du | 1 / sigma^2, then the weights w
  double* s_al = s_W + q * LDR;             // [128] alpha (zeros beyond n)
  double* s_C = s_al + HBO_TILE;            // [16][QS] the prior block, Sigma', C
  double* s_D2 = s_C + QEI_QQ;              // [16][QS] 2 dk/du of the batch pairs
  double* s_Cb = s_D2 + QEI_QQ;             // [16][QS] Cbar, then Sbar
  double* s_G = s_Cb + QEI_QQ;              // [16][QS] P, Y, then G
  double* s_mu = s_G + QEI_QQ;              // [16] m(x_j), then mu_j
  double* s_mub = s_mu + HBO_QEI_MAX_Q;     // [16] mubar
  double* s_acc = s_mub + HBO_QEI_MAX_Q;    // [256] the gradient's partials per row group
  double* sred = s_acc + 256;               // [4]
  int* s_rec = reinterpret_cast<int*>(sred + 4);   // [B] j*_b, or -1 where imp_b <= 0

  const int64_t m = blockIdx.x;
  const int s = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const AcqSmallSample& sm = a.smp[s];
  const int n = sm.n, qD = q * D;
  double* val = a.val_out + (int64_t)s * a.M + m;
  double* g = a.grad_out + ((int64_t)s * a.M + m) * qD;
  if (sm.bad) {   // (uniform) the cache is not positive definite: NaN rows, as the siblings
    if (tid == 0) *val = NAN;
    for (int e = tid; e < qD; e += 256) g[e] = NAN;
    return;
  }
  const double* vec = a.vec + (int64_t)s * 2 * D;
  const T* xq = static_cast<const T*>(a.xq) + m * qD;
  const T* F = static_cast<const T*>(sm.F);
  const T* W = static_cast<const T*>(sm.W);
  const T* al = static_cast<const T*>(sm.alpha);
  const int64_t ld = sm.ld;
  const int kid = a.kernel_id;
  const bool is_dot = (kid == HBO_KERNEL_DOT);
  const ExpCoef ec = hbo_exp_coef();

  // ---- 1: stage the batch
  for (int e = tid; e < qD; e += 256) { const int j = e / D; s_x[j * XS + (e - j * D)] = (double)xq[e]; }
  for (int d = tid; d < D; d += 256) s_il[d] = vec[d];
  if (tid < HBO_TILE) s_al[tid] = tid < n ? (double)al[tid] : 0.0;
  __syncthreads();
  if (tid < HBO_TILE) {
    // k_j[i] = k(x_j, X_i): thread i walks the features of row i in order, once for all j
    double u[QP];
#pragma unroll
    for (int j = 0; j < QP; ++j) u[j] = 0;
    if (tid < n) {
      const T* Fi = F + (int64_t)tid * D;
      if (is_dot) {
        for (int d = 0; d < D; ++d) {
          const double fd = (double)Fi[d];
#pragma unroll
          for (int j = 0; j < QP; ++j) if (j < q) u[j] += s_x[j * XS + d] * fd;
        }
      } else {
        for (int d = 0; d < D; ++d) {
          const double fd = (double)Fi[d], il = s_il[d];
#pragma unroll
          for (int j = 0; j < QP; ++j) if (j < q) { const double df = (s_x[j * XS + d] - fd) * il; u[j] += df * df; }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < QP; ++j)
      if (j < q) {
        double k = 0, dkf = 0;
        if (tid < n) {
          k = is_dot ? u[j] * sm.inv_sigma2 + sm.bias2 : kfun(kid, u[j], sm.sv, 1.0, 0.0, ec);
          dkf = is_dot ? sm.inv_sigma2 : dk_du(kid, u[j], k, sm.sv, ec) * 2.0;
        }
        s_A[j * LDR + tid] = k; s_W[j * LDR + tid] = dkf;   // (zeros beyond n)
      }
  } else {
    // the prior block k(x_j, x_l), l <= j, the pairs' 2 dk/du (both triangles) and the mean at x_j, on the other half of the workgroup
    for (int p = tid - HBO_TILE; p < q * q; p += HBO_TILE) {
      const int j = p / q, l = p - j * q;
      if (l > j) continue;
      double u = 0;
      if (is_dot) for (int d = 0; d < D; ++d) u += s_x[j * XS + d] * s_x[l * XS + d];
      else for (int d = 0; d < D; ++d) { const double df = (s_x[j * XS + d] - s_x[l * XS + d]) * s_il[d]; u += df * df; }
      const double k = is_dot ? u * sm.inv_sigma2 + sm.bias2 : kfun(kid, u, sm.sv, 1.0, 0.0, ec);
      const double d2 = is_dot ? 0.0 : dk_du(kid, u, k, sm.sv, ec) * 2.0;
      s_C[j * QS + l] = k;
      s_D2[j * QS + l] = d2; s_D2[l * QS + j] = d2;
      if (l == j) {
        double mean = 0;
        if (a.mean_id == HBO_MEAN_CONSTANT) mean = sm.constant;
        else if (a.mean_id == HBO_MEAN_LINEAR) {
          for (int d = 0; d < D; ++d) mean += s_x[j * XS + d] * vec[D + d];
          mean += sm.linear_bias;
        }
        s_mu[j] = mean;
      }
    }
  }
  __syncthreads();
  // ---- 2: l_j = W k_j, and mu_j += k_j . alpha with alpha as row n.  Four rows of loads in flight per wave
  for (int r0 = wave; r0 <= n; r0 += 16) {
    double w0[4], w1[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int r = r0 + 4 * b, rc = r < n ? r : n - 1;
      const T t0 = W[rc * ld + lane], t1 = W[rc * ld + lane + 64];
      w0[b] = lane <= r ? (double)t0 : 0.0; w1[b] = lane + 64 <= r ? (double)t1 : 0.0;
      if (r == n) { w0[b] = s_al[lane]; w1[b] = s_al[lane + 64]; }
    }
    for (int j = 0; j < q; ++j) {
      const double k0 = s_A[j * LDR + lane], k1 = s_A[j * LDR + lane + 64];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const double v = wave_sum(w0[b] * k0 + w1[b] * k1);
        const int r = r0 + 4 * b;
        if (lane == 0) {
          if (r < n) s_L[j * LDR + r] = v;
          else if (r == n) s_mu[j] += v;
        }
      }
    }
  }
  __syncthreads();
  // ---- beta_j = W^T l_j (into k's place: k is dead)
  {
    const int cidx = tid & (HBO_TILE - 1), h = tid >> 7;
    double bt[QP];
#pragma unroll
    for (int j = 0; j < QP; ++j) bt[j] = 0;
    if (cidx < n)
      for (int r = cidx + ((cidx & 1) != h); r < n; r += 2) {
        const double w = (double)W[r * ld + cidx];
#pragma unroll
        for (int j = 0; j < QP; ++j) if (j < q) bt[j] += w * s_L[j * LDR + r];
      }
    if (h == 1) {
#pragma unroll
      for (int j = 0; j < QP; ++j) if (j < q) s_A[j * LDR + cidx] = bt[j];
    }
    __syncthreads();
    if (h == 0) {
#pragma unroll
      for (int j = 0; j < QP; ++j) if (j < q) s_A[j * LDR + cidx] = bt[j] + s_A[j * LDR + cidx];
    }
  }
  // ---- 3: Sigma' = (k(x_j, x_l) - l_j . l_l + add_noise [j == l]) scale, the lower triangle
  const int cj = tid >> 4, cm = tid & 15;   // the thread's entry of the q x q matrices
  if (cj < q && cm <= cj) {
    double dot = 0;
    for (int i = 0; i < n; ++i) dot += s_L[cj * LDR + i] * s_L[cm * LDR + i];
    double sig = s_C[cj * QS + cm] - dot;
    if (cj == cm) sig += sm.add_noise;
    s_C[cj * QS + cm] = sig * a.scale;
  }
  __syncthreads();
  // ---- its Cholesky factor, right-looking.  Every thread reads the same pivot: the loop and its barriers are uniform
  bool pbad = false;
  for (int c = 0; c < q; ++c) {
    const double p = s_C[c * QS + c];
    if (!(p > 0.0)) { pbad = true; break; }
    const double dg = sqrt(p);
    __syncthreads();
    if (cm == c && cj >= c && cj < q) s_C[cj * QS + c] = cj == c ? dg : s_C[cj * QS + c] / dg;
    __syncthreads();
    if (cj > c && cj < q && cm > c && cm <= cj) s_C[cj * QS + cm] -= s_C[cj * QS + c] * s_C[cm * QS + c];
    __syncthreads();
  }
  if (pbad) {   // (uniform) duplicate points without noise, or an input that is not finite: this pair is NaN, the others are untouched
    if (tid == 0) *val = NAN;
    for (int e = tid; e < qD; e += 256) g[e] = NAN;
    return;
  }
  // ---- 4: the Monte-Carlo pass
  const double target = sm.param;
  double part = 0;
  for (int b = tid; b < B; b += 256) {
    double zz[QP];
#pragma unroll
    for (int j = 0; j < QP; ++j) zz[j] = j < q ? a.z[(int64_t)b * q + j] : 0.0;
    double best = 0; int js = 0;
#pragma unroll
    for (int j = 0; j < QP; ++j)
      if (j < q) {
        double f = s_mu[j];
#pragma unroll
        for (int l = 0; l <= j; ++l) f += s_C[j * QS + l] * zz[l];
        if (j == 0 || f > best) { best = f; js = j; }   // strictly greater: the lowest index among equals
      }
    const double imp = best - target;
    s_rec[b] = imp > 0.0 ? js : -1;
    if (!(imp <= 0.0)) part += imp;   // (a NaN stays one)
  }
  const double value = block_sum(part, sred) / (double)B;   // (its barriers publish s_rec)
  if (cj < q && cm <= cj) {
    double acc = 0, cnt = 0;
    for (int b = 0; b < B; ++b)
      if (s_rec[b] == cj) { acc += a.z[(int64_t)b * q + cm]; cnt += 1.0; }
    s_Cb[cj * QS + cm] = acc / (double)B;
    if (cm == 0) s_mub[cj] = cnt / (double)B;
  }
  __syncthreads();
  // ---- 5: the reverse pass through the factor
  if (cj < q && cm <= cj) {   // P = tril(C^T Cbar), diagonal halved
    double p = 0;
    for (int r = cj; r < q; ++r) p += s_C[r * QS + cj] * s_Cb[r * QS + cm];
    s_G[cj * QS + cm] = cj == cm ? 0.5 * p : p;
  }
  __syncthreads();
  if (tid < q) {   // Y = P C^-1: row tid, from its diagonal down to column 0, in place
    const int r = tid;
    for (int b = r; b >= 0; --b) {
      double v = s_G[r * QS + b];
      for (int k2 = b + 1; k2 <= r; ++k2) v -= s_G[r * QS + k2] * s_C[k2 * QS + b];
      s_G[r * QS + b] = v / s_C[b * QS + b];
    }
  }
  __syncthreads();
  if (tid < q) {   // Sbar = C^-T Y: column tid, from the last row up (Y is lower triangular)
    const int c = tid;
    for (int r = q - 1; r >= 0; --r) {
      double v = r >= c ? s_G[r * QS + c] : 0.0;
      for (int k2 = r + 1; k2 < q; ++k2) v -= s_C[k2 * QS + r] * s_Cb[k2 * QS + c];
      s_Cb[r * QS + c] = v / s_C[r * QS + r];
    }
  }
  __syncthreads();
  if (cj < q && cm < q) s_G[cj * QS + cm] = a.scale * (0.5 * (s_Cb[cj * QS + cm] + s_Cb[cm * QS + cj]));
  __syncthreads();
  // ---- 6: w_ji = coef_ji (2 dk/du_ji | 1 / sigma^2), in the factors' place
  {
    const int i = tid & (HBO_TILE - 1), h = tid >> 7;
    if (i < n)
      for (int j = h; j < q; j += 2) {
        double acc = 0;
        for (int l = 0; l < q; ++l) acc += s_G[j * QS + l] * s_A[l * LDR + i];
        const double coef = s_mub[j] * s_al[i] - 2.0 * acc;
        s_W[j * LDR + i] = coef * s_W[j * LDR + i];
      }
  }
  __syncthreads();
  // ---- the gradient: FD = pow2 >= q D (at most 256) lanes along the coordinates, NG groups over the rows, summed group by group
  int FD = 1; while (FD < qD && FD < 256) FD <<= 1;
  const int NG = 256 / FD, grp = tid / FD, dl = tid % FD;
  for (int e0 = 0; e0 < qD; e0 += FD) {   // (uniform)
    const int e = e0 + dl;
    const int j = e < qD ? e / D : 0, d = e < qD ? e - j * D : 0;
    const double xjd = s_x[j * XS + d];
    double acc = 0;
    if (e < qD)
      for (int i = grp; i < n; i += NG) {
        const double fi = (double)F[(int64_t)i * D + d], w = s_W[j * LDR + i];
        acc += is_dot ? w * fi : w * (xjd - fi);
      }
    s_acc[tid] = acc;
    __syncthreads();
    if (grp == 0 && e < qD) {
      double r = 0;
      for (int gg = 0; gg < NG; ++gg) r += s_acc[gg * FD + dl];
      double cpl = 0;
      if (is_dot) {
        for (int l = 0; l < q; ++l) cpl += s_G[j * QS + l] * s_x[l * XS + d];
        r += 2.0 * sm.inv_sigma2 * cpl;
      } else {
        for (int l = 0; l < q; ++l) if (l != j) cpl += s_G[j * QS + l] * s_D2[j * QS + l] * (xjd - s_x[l * XS + d]);
        r = (r + 2.0 * cpl) * (s_il[d] * s_il[d]);
      }
      if (a.mean_id == HBO_MEAN_LINEAR) r += s_mub[j] * vec[D + d];
      g[e] = r;
    }
    __syncthreads();
  }
  if (tid == 0) *val = value;
}

template <typename T, int QP>
void qei_launch_q(const QeiArgs& a, const dim3& grid, size_t lds, hipStream_t st) {
  static unsigned long long seen = 0;
  if (hbo_first_use_on_device(seen))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&qei_kernel<T, QP>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(sizeof(double) * qei_lds_doubles(QP, HBO_MAX_FEATURE_DIM, HBO_QEI_MAX_BASE)));
  hipLaunchKernelGGL((qei_kernel<T, QP>), grid, dim3(256), lds, st, a);
}
template <typename T>
void qei_launch_t(const QeiArgs& a, const dim3& grid, size_t lds, hipStream_t st) {
  if (a.q <= 1) qei_launch_q<T, 1>(a, grid, lds, st);
  else if (a.q <= 2) qei_launch_q<T, 2>(a, grid, lds, st);
  else if (a.q <= 4) qei_launch_q<T, 4>(a, grid, lds, st);
  else if (a.q <= 8) qei_launch_q<T, 8>(a, grid, lds, st);
  else qei_launch_q<T, 16>(a, grid, lds, st);
}
void launch_qei(int dtype, const QeiArgs& a, int S, hipStream_t st) {
  if (a.M <= 0 || S <= 0) return;
  const dim3 grid((unsigned)a.M, (unsigned)S);
  const size_t lds = sizeof(double) * qei_lds_doubles(a.q, a.D, a.B);
  if (dtype == HBO_F64) qei_launch_t<double>(a, grid, lds, st);
  else qei_launch_t<float>(a, grid, lds, st);
}

// What both entry points ask of (models, caches, q, z, B, targets, add_noise, scale) before any device work
int qei_check(hbo_ctx* c, const std::string& fn, const hbo_model* models, int32_t S, hbo_cache* const* caches, int32_t q, const double* z,
              int32_t B, const double* targets, const double* add_noise, double scale, bool* any_bad) {
  if (S <= 0 || S > 4096) return fail(c, HBO_ERR_ARG, fn + "1 <= S <= 4096");
  if (q < 1 || q > HBO_QEI_MAX_Q) return fail(c, HBO_ERR_ARG, fn + "1 <= q <= " + std::to_string(HBO_QEI_MAX_Q));
  if (B < 1 || B > HBO_QEI_MAX_BASE) return fail(c, HBO_ERR_ARG, fn + "1 <= B <= " + std::to_string(HBO_QEI_MAX_BASE));
  for (int64_t i = 0; i < (int64_t)B * q; ++i) if (!isfinite(z[i])) return fail(c, HBO_ERR_ARG, fn + "z holds a value that is not finite");
  for (int s = 0; s < S; ++s) {
    if (!isfinite(targets[s])) return fail(c, HBO_ERR_ARG, fn + "targets holds a value that is not finite");
    if (!isfinite(add_noise[s]) || add_noise[s] < 0.0) return fail(c, HBO_ERR_ARG, fn + "add_noise must be finite and >= 0");
  }
  if (!isfinite(scale) || !(scale > 0.0)) return fail(c, HBO_ERR_ARG, fn + "scale must be finite and > 0");
  if (!c) return fail(c, HBO_ERR_ARG, fn + "ctx is null");
  // the siblings' checks of the (model, cache) pairs on the one-block route (api_internal.h), under this entry point's advice
  if (int rc = acq_samples_check(c, fn, models, S, caches, HBO_TILE, any_bad, false, "batch expected improvement has no other route for them (out of scope)",
                                 "batch expected improvement has no other route for it (out of scope)"))
    return rc;
  if (sizeof(double) * qei_lds_doubles(q, models[0].input_dim, B) > (size_t)c->lds_per_block)
    return fail(c, HBO_ERR_UNSUPPORTED, fn + "the device cannot give the batch's workgroup its LDS");
  return HBO_OK;
}
}  // namespace

extern "C" int hbo_qei_grad_samples(hbo_ctx* c, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq, int64_t M, int32_t q,
                                    const double* z, int32_t B, const double* targets, const double* add_noise, double scale, double* val_out,
                                    double* grad_out) {
  const std::string fn = "hbo_qei_grad_samples: ";
  if (!models || !caches || !xq || !z || !targets || !add_noise || !val_out || !grad_out) return fail(c, HBO_ERR_ARG, fn + "null argument");
  if (M < 0 || M > INT_MAX) return fail(c, HBO_ERR_ARG, fn + "0 <= M <= 2^31 - 1 (grid.x carries the batches)");
  bool any_bad = false;
  if (int rc = qei_check(c, fn, models, S, caches, q, z, B, targets, add_noise, scale, &any_bad)) return rc;
  if (M == 0) return HBO_OK;
  const hbo_model* m0 = &models[0];
  HIPCHK(c, hipSetDevice(c->device));
  prof_begin(c);
  const int dtype = m0->dtype, D = m0->input_dim;
  const int64_t qD = (int64_t)q * D;
  const size_t es = esize(dtype);
  hipStream_t st = c->stream;
  // one block up: [S records][S x 2 D doubles][B x q base samples][M x q x D points]; one block down: [S x M x q x D doubles][S x M values]
  const size_t smp_b = align256(sizeof(AcqSmallSample) * S), vec_b = align256(sizeof(double) * 2 * D * S), z_b = align256(sizeof(double) * (size_t)B * q);
  const size_t in_b = smp_b + vec_b + z_b + (size_t)M * qD * es;
  const size_t grad_b = align256(sizeof(double) * (size_t)S * M * qD), out_b = grad_b + sizeof(double) * (size_t)S * M;
  char* d_in = static_cast<char*>(ws_get(c, WS_AF_IN, in_b));
  char* d_out = static_cast<char*>(ws_get(c, WS_AF_OUT, out_b));
  if (!d_in || !d_out) return HBO_ERR_HIP;
  char* stage = static_cast<char*>(stage_begin(c, fn.c_str(), align256(in_b) + out_b));
  if (!stage) return HBO_ERR_HIP;
  char* stage_out = stage + align256(in_b);
  acq_small_pack(reinterpret_cast<AcqSmallSample*>(stage), reinterpret_cast<double*>(stage + smp_b), models, S, caches, targets, add_noise);
  memcpy(stage + smp_b + vec_b, z, sizeof(double) * (size_t)B * q);
  memcpy(stage + smp_b + vec_b + z_b, xq, (size_t)M * qD * es);
  HIPCHK(c, stage_upload(c, d_in, stage, in_b, st));
  QeiArgs a = {};
  a.smp = reinterpret_cast<const AcqSmallSample*>(d_in); a.vec = reinterpret_cast<const double*>(d_in + smp_b);
  a.z = reinterpret_cast<const double*>(d_in + smp_b + vec_b); a.xq = d_in + smp_b + vec_b + z_b;
  a.grad_out = reinterpret_cast<double*>(d_out); a.val_out = reinterpret_cast<double*>(d_out + grad_b);
  a.M = M; a.D = D; a.q = q; a.B = B; a.kernel_id = m0->kernel_id; a.mean_id = m0->mean_id; a.scale = scale;
  { ProfScope ps(c, "qei_eval", 1); launch_qei(dtype, a, S, st); }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(stage_out, d_out, out_b, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  prof_collect(c);
  memcpy(grad_out, stage_out, sizeof(double) * (size_t)S * M * qD);
  memcpy(val_out, stage_out + grad_b, sizeof(double) * (size_t)S * M);
  return any_bad ? HBO_NOT_PD : HBO_OK;
}

extern "C" int hbo_qei_maximize(hbo_ctx* c, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* x0, int32_t R, int32_t q,
                                const double* lo, const double* hi, const double* z, int32_t B, const double* targets, const double* add_noise,
                                double scale, const hbo_acq_opt_opts* opts, double* state, int32_t evals, double* x_out, double* val_out,
                                int32_t* status, hbo_acq_opt_eval* log) {
  const std::string fn = "hbo_qei_maximize: ";
  if (!models || !caches || !x0 || !z || !targets || !add_noise || !state || !x_out || !val_out || !status) return fail(c, HBO_ERR_ARG, fn + "null argument");
  if (R <= 0 || R > 4096) return fail(c, HBO_ERR_ARG, fn + "1 <= R <= 4096");
  if (evals <= 0 || evals > 4096) return fail(c, HBO_ERR_ARG, fn + "1 <= evals <= 4096");
  if (int rc = acq_opt_check_opts(c, fn, opts)) return rc;
  bool any_bad = false;
  if (int rc = qei_check(c, fn, models, S, caches, q, z, B, targets, add_noise, scale, &any_bad)) return rc;
  const hbo_model* m0 = &models[0];
  const int dtype = m0->dtype, D = m0->input_dim, qD = q * D;
  if (int rc = acq_opt_check_box(c, fn, lo, hi, D, dtype)) return rc;
  const int64_t ns = hbo_acq_opt_state_size(qD, opts->memory);
  if (acq_opt_lds_bytes(ns) > ACQ_OPT_LDS_MAX)
    return fail(c, HBO_ERR_UNSUPPORTED, fn + "the state of a start (q * input_dim, opts.memory) does not fit 64 KB of LDS");
  // the box of the flattened variable: lo, hi tiled q times
  std::vector<double> blo(qD), bhi(qD), xs(qD);
  for (int i = 0; i < qD; ++i) { blo[i] = lo ? lo[i % D] : 0.0; bhi[i] = hi ? hi[i % D] : 1.0; }
  for (int r = 0; r < R; ++r) {
    bool fresh = false;
    if (int rc = acq_opt_check_state(c, fn, state + r * ns, opts, &fresh)) return rc;
    if (!fresh) continue;
    for (int i = 0; i < qD; ++i) xs[i] = host_elem(x0, dtype, (int64_t)r * qD + i);
    if (!acq_opt_in_box(xs.data(), blo.data(), bhi.data(), qD)) return fail(c, HBO_ERR_ARG, fn + "a start lies outside the box (or is not finite)");
  }

  HIPCHK(c, hipSetDevice(c->device));
  prof_begin(c);
  const size_t es = esize(dtype);
  hipStream_t st = c->stream;
  // one block up: [S records][S x 2 D doubles][B x q base samples][lo, hi tiled][R x q D pending batches][R states]; the log follows the
  // states, and one copy brings [states | log] back.  Scratch of the rounds: [S x R x q D gradients][S x R values]
  const size_t smp_b = align256(sizeof(AcqSmallSample) * S), vec_b = align256(sizeof(double) * 2 * D * S), z_b = align256(sizeof(double) * (size_t)B * q);
  const size_t box_b = align256(sizeof(double) * 2 * qD), pend_b = align256((size_t)R * qD * es), state_b = align256(sizeof(double) * (size_t)R * ns);
  const size_t log_b = log ? sizeof(hbo_acq_opt_eval) * (size_t)evals * R : 0;
  const size_t o_box = smp_b + vec_b + z_b, o_pend = o_box + box_b, o_state = o_pend + pend_b, up_b = o_state + state_b, down_b = state_b + log_b;
  const size_t grad_b = align256(sizeof(double) * (size_t)S * R * qD), val_b = align256(sizeof(double) * (size_t)S * R);
  char* d_in = static_cast<char*>(ws_get(c, WS_AO_IN, up_b + log_b));
  char* d_out = static_cast<char*>(ws_get(c, WS_AO_OUT, grad_b + val_b));
  if (!d_in || !d_out) return HBO_ERR_HIP;
  char* stage = static_cast<char*>(stage_begin(c, fn.c_str(), up_b + log_b));
  if (!stage) return HBO_ERR_HIP;
  acq_small_pack(reinterpret_cast<AcqSmallSample*>(stage), reinterpret_cast<double*>(stage + smp_b), models, S, caches, targets, add_noise);
  memcpy(stage + smp_b + vec_b, z, sizeof(double) * (size_t)B * q);
  double* hbox = reinterpret_cast<double*>(stage + o_box);
  memcpy(hbox, blo.data(), sizeof(double) * qD); memcpy(hbox + qD, bhi.data(), sizeof(double) * qD);
  // the states go up from a copy, and a fresh one is started in that copy: the caller's array is written once, by the copy back
  double* hstate = reinterpret_cast<double*>(stage + o_state);
  memcpy(hstate, state, sizeof(double) * (size_t)R * ns);
  char* hpend = stage + o_pend;
  for (int r = 0; r < R; ++r) {
    double* sr = hstate + r * ns;
    bool fresh = true;
    for (int k = 0; k < HBO_ACQ_OPT_S_HEADER; ++k) fresh = fresh && sr[k] == 0.0;
    if (fresh) {
      for (int i = 0; i < qD; ++i) xs[i] = host_elem(x0, dtype, (int64_t)r * qD + i);
      hbo_acq_opt_state_start(sr, qD, opts->memory, xs.data());
    }
    const hbo_acq_opt_view v = hbo_acq_opt_view_of(sr, qD, opts->memory);   // the pending batch, as the state holds it
    for (int i = 0; i < qD; ++i) {
      if (dtype == HBO_F64) reinterpret_cast<double*>(hpend)[(size_t)r * qD + i] = v.xt[i];
      else reinterpret_cast<float*>(hpend)[(size_t)r * qD + i] = (float)v.xt[i];
    }
  }
  HIPCHK(c, stage_upload(c, d_in, stage, up_b, st));

  QeiArgs a = {};
  a.smp = reinterpret_cast<const AcqSmallSample*>(d_in); a.vec = reinterpret_cast<const double*>(d_in + smp_b);
  a.z = reinterpret_cast<const double*>(d_in + smp_b + vec_b); a.xq = d_in + o_pend;
  a.grad_out = reinterpret_cast<double*>(d_out); a.val_out = reinterpret_cast<double*>(d_out + grad_b);
  a.M = R; a.D = D; a.q = q; a.B = B; a.kernel_id = m0->kernel_id; a.mean_id = m0->mean_id; a.scale = scale;
  AcqOptArgs k = {};
  k.reduce = HBO_ACQ_OPT_REDUCE_MEAN;
  k.o = acq_opt_ctl_opts(opts);
  k.state = reinterpret_cast<double*>(d_in + o_state); k.ns = ns;
  k.lo = reinterpret_cast<const double*>(d_in + o_box); k.hi = k.lo + qD;
  k.pending = d_in + o_pend;
  k.vals = a.val_out; k.grads = a.grad_out;
  k.log = log ? reinterpret_cast<hbo_acq_opt_eval_ctl*>(d_in + up_b) : nullptr;
  k.D = qD; k.R = R; k.S = S;
  if (c->opt_poison && log_b) HIPCHK(c, hipMemsetAsync(d_in + up_b, 0xFF, log_b, st));
  for (int e = 0; e < evals; ++e) {
    { ProfScope ps(c, "qei_eval", 2); launch_qei(dtype, a, S, st); }
    { ProfScope ps(c, "qei_ctl", 2); launch_acq_opt_ctl(dtype, k, e, st); }
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(stage + o_state, d_in + o_state, down_b, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  prof_collect(c);
  memcpy(state, stage + o_state, sizeof(double) * (size_t)R * ns);
  if (log) memcpy(log, stage + up_b, log_b);
  for (int r = 0; r < R; ++r) {
    const hbo_acq_opt_view v = hbo_acq_opt_view_of(state + r * ns, qD, opts->memory);
    memcpy(x_out + (size_t)r * qD, v.x, sizeof(double) * qD);
    val_out[r] = -v.hdr[HBO_ACQ_OPT_S_CUR];
    status[r] = (int32_t)v.hdr[HBO_ACQ_OPT_S_STATUS];
  }
  return any_bad ? HBO_NOT_PD : HBO_OK;
}
