// Posterior sample paths by Matheron's rule (hbo_sample_paths, include/hbo.h): S paths over one shared basis of F features,
//   f_s(x) = m(x) + p_s(x) + sum_i k(x, X_i) v[i,s],   v[:,s] = Ktilde^-1 (y - m(X) - p_s(X) - sqrt(noise + eps) eps[:,s]),
// with the prior path p_s from random Fourier features (SE / Matern) or the exact finite basis of the dot-product kernel.
// Three steps on the device:
//   path_prior_kernel    sums[row, s] = sum_j c(row, j) w[j, s] over rows that are queries or cached observations; every c(row, j) --
//                        the cosine of omega_j . phi(row) + b_j, or phi_j / sigma and the bias for the dot product -- is evaluated
//                        ONCE and applied to all S columns
//   path_tri_*_kernel    z = W r, v = W^T z with W = L^-1 of the cache, S right-hand sides
//   path_update_kernel   out[q, s] = m(x_q) + A sums[q, s] + sum_i Kxq[i, q] v[i, s] on the cross-Gram chunk launch_gram leaves
// Every sum is taken in fp64 in an order fixed by n, F and fdim alone (no atomics): a column does not depend on the columns
// beside it, a row not on the chunk it came in, and two identical calls agree to the bit.  Loads are from clamped, valid
// addresses; what lies beyond an extent is masked to zero.
#include "api_internal.h"

namespace {
constexpr int PP_RT = 32;   // rows per workgroup
constexpr int PP_FT = 64;   // features per pass
constexpr int PP_DC = 32;   // feature-space columns of omega / phi staged per step
constexpr int PP_SW = 32;   // columns of w staged per step
constexpr int PATH_SC = 8;  // right-hand sides / path columns per workgroup of the solve and the update

__device__ __forceinline__ double path_cos(double x) { return cos(x); }
__device__ __forceinline__ float path_cos(float x) { return cosf(x); }
__device__ __forceinline__ double path_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

struct PathPriorArgs {
  const void* feat; int64_t rows; int fdim;               // phi: [rows][fdim], model dtype
  const void* omega; const void* phase; const void* w;    // [F][fdim], [F], [F][S], model dtype (omega / phase unused by the dot product)
  int F, S, is_dot;
  double* sums;                                           // [rows][S]: sum_j c(row, j) w[j, s], without the amplitude
};

// A workgroup owns PP_RT rows and walks the features PP_FT at a time.  Per pass: (1) the arguments omega_j . phi(row) of its 32 x 64
// (row, feature) pairs, each thread a 4 x 2 register tile, omega and phi staged PP_DC columns at a time (d ascending, fp64), the
// cosine taken in the model dtype; (2) the 32 x S sums of the pass, w staged PP_SW columns at a time (j ascending, fp64), added to
// the running sums the workgroup keeps in `sums` (pass 0 writes them: the buffer needs no zeroing).
template <typename T>
__global__ __launch_bounds__(256) void path_prior_kernel(PathPriorArgs a, const ModelDev* __restrict__ md) {
  __shared__ T s_om[PP_FT][PP_DC + 1];
  __shared__ T s_ph[PP_RT][PP_DC];
  __shared__ T s_w[PP_FT][PP_SW];
  __shared__ double s_c[PP_RT][PP_FT];
  const int tid = threadIdx.x;
  const int jl = tid & 31, rg = tid >> 5;   // features jl, jl + 32; rows rg + 8 u
  const int64_t r0 = (int64_t)blockIdx.x * PP_RT;
  const T* feat = static_cast<const T*>(a.feat);
  const T* om = static_cast<const T*>(a.omega);
  const T* ph = static_cast<const T*>(a.phase);
  const T* w = static_cast<const T*>(a.w);
  const int fdim = a.fdim, F = a.F, S = a.S;
  const double inv_sigma = 1.0 / md->dot_sigma, bias = md->dot_bias;
  for (int j0 = 0; j0 < F; j0 += PP_FT) {
    double arg[4][2];
#pragma unroll
    for (int u = 0; u < 4; ++u) { arg[u][0] = 0; arg[u][1] = 0; }
    if (!a.is_dot) {
      for (int d0 = 0; d0 < fdim; d0 += PP_DC) {
        __syncthreads();   // the previous step's tiles are no longer read
#pragma unroll
        for (int k = 0; k < PP_FT * PP_DC / 256; ++k) {
          const int idx = tid + 256 * k, jj = idx / PP_DC, dd = idx % PP_DC;
          const bool ok = j0 + jj < F && d0 + dd < fdim;
          const T v = om[(int64_t)min(j0 + jj, F - 1) * fdim + min(d0 + dd, fdim - 1)];
          s_om[jj][dd] = ok ? v : (T)0;
        }
#pragma unroll
        for (int k = 0; k < PP_RT * PP_DC / 256; ++k) {
          const int idx = tid + 256 * k, rr = idx / PP_DC, dd = idx % PP_DC;
          const bool ok = r0 + rr < a.rows && d0 + dd < fdim;
          const T v = feat[min(r0 + rr, a.rows - 1) * fdim + min(d0 + dd, fdim - 1)];
          s_ph[rr][dd] = ok ? v : (T)0;
        }
        __syncthreads();
        const int dl = min(PP_DC, fdim - d0);
        for (int dd = 0; dd < dl; ++dd) {
          const double o0 = (double)s_om[jl][dd], o1 = (double)s_om[jl + 32][dd];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const double p = (double)s_ph[rg + 8 * u][dd];
            arg[u][0] += o0 * p; arg[u][1] += o1 * p;
          }
        }
      }
    }
    __syncthreads();   // the previous pass no longer reads s_c
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int j = j0 + jl + 32 * v;
      const double bj = a.is_dot ? 0.0 : (double)ph[min(j, F - 1)];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = rg + 8 * u;
        double cv;
        if (a.is_dot) {   // the finite basis of k = phi . phi' / sigma^2 + bias^2: phi_j / sigma for j < fdim, then the bias
          const double f = (double)feat[min(r0 + r, a.rows - 1) * fdim + min(j, fdim - 1)];
          cv = j < fdim ? f * inv_sigma : bias;
        } else {
          cv = (double)path_cos((T)(arg[u][v] + bj));
        }
        s_c[r][jl + 32 * v] = j < F ? cv : 0.0;
      }
    }
    const int jn = min(PP_FT, F - j0);
    for (int s0 = 0; s0 < S; s0 += PP_SW) {
      __syncthreads();   // s_c is written; the previous step no longer reads s_w
#pragma unroll
      for (int k = 0; k < PP_FT * PP_SW / 256; ++k) {
        const int idx = tid + 256 * k, jj = idx / PP_SW, ss = idx % PP_SW;
        const bool ok = j0 + jj < F && s0 + ss < S;
        const T v = w[(int64_t)min(j0 + jj, F - 1) * S + min(s0 + ss, S - 1)];
        s_w[jj][ss] = ok ? v : (T)0;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < PP_RT * PP_SW / 256; ++k) {
        const int o = tid + 256 * k, ss = o % PP_SW, r = o / PP_SW;
        double acc = 0;
        for (int jj = 0; jj < jn; ++jj) acc += s_c[r][jj] * (double)s_w[jj][ss];
        if (r0 + r < a.rows && s0 + ss < S) {
          double* p = a.sums + (r0 + r) * S + s0 + ss;
          *p = j0 ? *p + acc : acc;
        }
      }
    }
  }
}

// r[s][i] = (y - m(X))_i - A sums[i, s] - sn eps[i, s]: the right-hand sides of the solve, one vector of ld doubles per path
template <typename T>
__global__ void path_rhs_kernel(const T* __restrict__ resid, const double* __restrict__ sums, const T* __restrict__ eps, double A, double sn,
                                int n, int S, int64_t ld, double* __restrict__ r) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n * S) return;
  const int64_t i = idx / S; const int s = (int)(idx % S);
  r[(int64_t)s * ld + i] = ((double)resid[i] - A * sums[idx]) - sn * (double)eps[idx];
}

// out[c] = W x[c] over the leading n x n block of the lower-triangular W: one wave per row, PATH_SC right-hand sides per workgroup
template <typename T>
__global__ __launch_bounds__(256) void path_tri_fwd_kernel(const T* __restrict__ W, int64_t ld, int n, const double* __restrict__ x, int64_t xld,
                                                           int S, double* __restrict__ out) {
  const int c0 = blockIdx.y * PATH_SC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 4 + wave;
  if (i >= n) return;
  double s[PATH_SC];
#pragma unroll
  for (int c = 0; c < PATH_SC; ++c) s[c] = 0;
  for (int64_t j = lane; j <= i; j += 64) {
    const double wv = (double)W[i * ld + j];
#pragma unroll
    for (int c = 0; c < PATH_SC; ++c) s[c] += wv * x[(int64_t)min(c0 + c, S - 1) * xld + j];
  }
#pragma unroll
  for (int c = 0; c < PATH_SC; ++c) {
    const double v = path_wave_sum(s[c]);
    if (lane == 0 && c0 + c < S) out[(int64_t)(c0 + c) * xld + i] = v;
  }
}

// out[c] = W^T x[c]: the transposed step.  A workgroup owns 64 columns of W (lane = column: the row reads coalesce); the right-hand
// sides of 256 rows at a time are staged in LDS, each wave takes 64 of them eight at a time; the waves' sums meet in LDS in a fixed order.
template <typename T>
__global__ __launch_bounds__(256) void path_tri_trans_kernel(const T* __restrict__ W, int64_t ld, int n, const double* __restrict__ x, int64_t xld,
                                                             int S, double* __restrict__ out) {
  __shared__ double red[4][PATH_SC][64];
  __shared__ double xs[PATH_SC][256];
  const int c0 = blockIdx.y * PATH_SC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t j0 = (int64_t)blockIdx.x * 64, j = j0 + lane, jc = min(j, (int64_t)n - 1);
  double s[PATH_SC];
#pragma unroll
  for (int c = 0; c < PATH_SC; ++c) s[c] = 0;
  for (int64_t rc = j0 / 256 * 256; rc < n; rc += 256) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < PATH_SC; ++c) {
      const int64_t r = rc + threadIdx.x;
      const double v = x[(int64_t)min(c0 + c, S - 1) * xld + min(r, (int64_t)n - 1)];
      xs[c][threadIdx.x] = (c0 + c < S && r < n) ? v : 0.0;
    }
    __syncthreads();
#pragma unroll 2
    for (int g = 0; g < 8; ++g) {
      const int rl = wave * 64 + g * 8;
      double wv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t r = rc + rl + u;
        const double v = (double)W[min(r, (int64_t)n - 1) * ld + jc];
        wv[u] = (r < n && r >= j && j < n) ? v : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int c = 0; c < PATH_SC; ++c) s[c] += wv[u] * xs[c][rl + u];
    }
  }
#pragma unroll
  for (int c = 0; c < PATH_SC; ++c) red[wave][c][lane] = s[c];
  __syncthreads();
  if (wave == 0 && j < n)
#pragma unroll
    for (int c = 0; c < PATH_SC; ++c)
      if (c0 + c < S) out[(int64_t)(c0 + c) * xld + j] = ((red[0][c][lane] + red[1][c][lane]) + red[2][c][lane]) + red[3][c][lane];
}

// out[q, s] = (m(x_q) + A sums[q, s]) + sum_i K[i, q] v[s][i] over a chunk of mc queries; K [n rows][ldq] is the cross Gram in the layout
// of the posterior's chunks.  A workgroup owns 64 queries (lane = query: the row reads of K coalesce) and PATH_SC paths; wave w takes
// the w-th quarter of the n observations (quarters of ceil(n / 4): fixed by n alone), v staged in LDS 64 rows at a time; the four
// partial sums meet in a fixed order.  n = 0 is the prior branch.
template <typename T>
__global__ __launch_bounds__(256) void path_update_kernel(const T* __restrict__ K, int64_t ldq, int n, const double* __restrict__ v, int64_t vld,
                                                          const double* __restrict__ sums, double A, const T* __restrict__ mu0, int64_t mc, int S,
                                                          T* __restrict__ out) {
  __shared__ double vs[4][PATH_SC][64];
  __shared__ double red[4][PATH_SC][64];
  const int c0 = blockIdx.y * PATH_SC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t q = (int64_t)blockIdx.x * 64 + lane, qc = min(q, mc - 1);
  const int nq = (n + 3) / 4;
  double s[PATH_SC];
#pragma unroll
  for (int c = 0; c < PATH_SC; ++c) s[c] = 0;
  for (int t0 = 0; t0 < nq; t0 += 64) {
    __syncthreads();
    {
      const int i = wave * nq + t0 + lane;
      const bool ok = t0 + lane < nq && i < n;
#pragma unroll
      for (int c = 0; c < PATH_SC; ++c) {
        const double x = v[(int64_t)min(c0 + c, S - 1) * vld + min(i, n - 1)];
        vs[wave][c][lane] = ok ? x : 0.0;
      }
    }
    __syncthreads();
    const int lim = min(64, nq - t0);
    for (int ii = 0; ii < lim; ++ii) {
      const int i = wave * nq + t0 + ii;
      if (i >= n) break;   // (uniform over the wave; no barrier inside)
      const double kv = (double)K[(int64_t)i * ldq + qc];
#pragma unroll
      for (int c = 0; c < PATH_SC; ++c) s[c] += kv * vs[wave][c][ii];
    }
  }
#pragma unroll
  for (int c = 0; c < PATH_SC; ++c) red[wave][c][lane] = s[c];
  __syncthreads();
  if (wave == 0 && q < mc)
#pragma unroll
    for (int c = 0; c < PATH_SC; ++c)
      if (c0 + c < S) {
        const double ksum = ((red[0][c][lane] + red[1][c][lane]) + red[2][c][lane]) + red[3][c][lane];
        out[q * S + c0 + c] = (T)(((double)mu0[q] + A * sums[q * S + c0 + c]) + ksum);
      }
}

template <typename T>
void launch_path_prior_t(const PathPriorArgs& a, const ModelDev* md, hipStream_t st) {
  hipLaunchKernelGGL((path_prior_kernel<T>), dim3((unsigned)((a.rows + PP_RT - 1) / PP_RT)), dim3(256), 0, st, a, md);
}
void launch_path_prior(int dtype, const PathPriorArgs& a, const ModelDev* md, hipStream_t st) {
  if (a.rows <= 0) return;
  if (dtype == HBO_F64) launch_path_prior_t<double>(a, md, st); else launch_path_prior_t<float>(a, md, st);
}

// v = W^T (W r) for S right-hand sides r [S][ld] (doubles) over the cache's n observations; z is scratch of the same shape
template <typename T>
void launch_path_solve_t(const void* W, int64_t ldw, int n, const double* r, double* z, double* v, int64_t ld, int S, hipStream_t st) {
  const unsigned cb = (unsigned)((S + PATH_SC - 1) / PATH_SC);
  hipLaunchKernelGGL((path_tri_fwd_kernel<T>), dim3((unsigned)((n + 3) / 4), cb), dim3(256), 0, st, static_cast<const T*>(W), ldw, n, r, ld, S, z);
  hipLaunchKernelGGL((path_tri_trans_kernel<T>), dim3((unsigned)((n + 63) / 64), cb), dim3(256), 0, st, static_cast<const T*>(W), ldw, n, z, ld, S, v);
}
}  // namespace

// What hbo_sample_paths and the entry points of path_opt.hip ask of (model, cache, S, F, eps), before any device call (c may be null)
int path_check(hbo_ctx* c, const std::string& fn, const hbo_model* m, const hbo_cache* k, int32_t S, int32_t F, bool has_eps) {
  if (S < 1 || S > 1024) return fail(c, HBO_ERR_ARG, fn + "need 1 <= S <= 1024");
  if (F < 1 || F > 65536) return fail(c, HBO_ERR_ARG, fn + "need 1 <= F <= 65536");
  int rc = validate_model(c, m);
  if (rc) return rc;
  const int dtype = m->dtype, D = m->input_dim, fdim = feature_dim(m);
  const bool is_dot = m->kernel_id == HBO_KERNEL_DOT;
  if (is_dot && F != fdim + 1) return fail(c, HBO_ERR_ARG, fn + "a dot-product model takes F = feature dim + 1 (its basis is exact)");
  if ((k != nullptr) != has_eps) return fail(c, HBO_ERR_ARG, fn + "eps goes with a cache: both or neither");
  if (k && (k->dtype != dtype || k->D != D)) return fail(c, HBO_ERR_ARG, fn + "cache/model mismatch");
  if (k && k->input_warp != m->input_warp) return fail(c, HBO_ERR_ARG, fn + "the cache was factorised with another input warp");
  if (k && (!k->t || k->t->n <= 0)) return fail(c, HBO_ERR_ARG, fn + "the cache holds no observations");
  return HBO_OK;
}

// The draws on the device and the weights of the update term, v[:,s] = Ktilde^-1 (y - m(X) - scale p_s(X) - scale sqrt(noise + eps) eps[:,s]):
// the prior paths at the cached observations, the right-hand sides, the two triangular products.  `scale` multiplies the amplitude
// and the noise scale (1 for hbo_sample_paths; the unbiased deviation scale of path_opt.hip).  sum_rows: rows the caller wants of the
// [rows][S] prior sums (at least n are taken).  A cache that is not positive definite (or none) is left alone: v stays unset.
int path_solve(hbo_ctx* c, const hbo_model* m, hbo_cache* k, int32_t S, int32_t F, const void* omega, const void* phase, const void* w,
               const void* eps, double scale, int64_t sum_rows, PathSolve* ps) {
  const int dtype = m->dtype, fdim = feature_dim(m);
  const bool is_dot = m->kernel_id == HBO_KERNEL_DOT;
  const size_t es = esize(dtype);
  hipStream_t st = c->stream;
  TaskHost* t = k ? k->t : nullptr;
  const int n = t ? (int)t->n : 0;
  ps->A = is_dot ? 1.0 : sqrt(2.0 * (double)m->signal_variance / (double)F);
  const double sn = sqrt((double)m->noise_variance + (double)m->eps);
  // the draws (omega / phase stay empty for the dot product)
  const size_t om_b = is_dot ? 0 : (size_t)F * fdim * es, ph_b = is_dot ? 0 : (size_t)F * es, w_b = (size_t)F * S * es;
  char* d_draw = (char*)ws_get(c, WS_PATH_DRAWS, om_b + ph_b + w_b + (size_t)n * S * es + 64);
  double* d_sums = (double*)ws_get(c, WS_PATH_SUMS, (size_t)std::max<int64_t>(std::max<int64_t>(sum_rows, n), 1) * S * sizeof(double));
  if (!d_draw || !d_sums) return HBO_ERR_HIP;
  char* d_om = d_draw; char* d_ph = d_om + om_b; char* d_w = d_ph + ph_b; char* d_eps = d_w + w_b;
  double *d_r = nullptr, *d_z = nullptr, *d_v = nullptr;
  if (t) {
    d_r = (double*)ws_get(c, WS_PATH_R, (size_t)S * t->npad * sizeof(double));
    d_z = (double*)ws_get(c, WS_PATH_Z, (size_t)S * t->npad * sizeof(double));
    d_v = (double*)ws_get(c, WS_PATH_V, (size_t)S * t->npad * sizeof(double));
    if (!d_r || !d_z || !d_v) return HBO_ERR_HIP;
  }
  if (om_b) HIPCHK(c, hipMemcpyAsync(d_om, omega, om_b, hipMemcpyHostToDevice, st));
  if (ph_b) HIPCHK(c, hipMemcpyAsync(d_ph, phase, ph_b, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_w, w, w_b, hipMemcpyHostToDevice, st));
  if (t) HIPCHK(c, hipMemcpyAsync(d_eps, eps, (size_t)n * S * es, hipMemcpyHostToDevice, st));
  ps->om = d_om; ps->ph = d_ph; ps->w = d_w; ps->sums = d_sums; ps->v = d_v; ps->vld = t ? t->npad : 0;
  if (!t || k->info != INT_MAX) return HBO_OK;
  PathPriorArgs pa = {};
  pa.fdim = fdim; pa.omega = d_om; pa.phase = d_ph; pa.w = d_w; pa.F = F; pa.S = S; pa.is_dot = is_dot; pa.sums = d_sums;
  // the prior paths at the observations (their features are the cache's), the right-hand sides, v = W^T (W r)
  { ProfScope pp(c, "path_prior", 1);
    pa.feat = k->h_desc.F; pa.rows = n;
    launch_path_prior(dtype, pa, c->d_model, st); }
  ProfScope pp(c, "path_solve", 1);
  const unsigned gb = (unsigned)(((int64_t)n * S + 255) / 256);
  const double A = ps->A * scale, sns = sn * scale;
  if (dtype == HBO_F64) {
    hipLaunchKernelGGL((path_rhs_kernel<double>), dim3(gb), dim3(256), 0, st, (const double*)k->resid, d_sums, (const double*)d_eps, A, sns, n, S, (int64_t)t->npad, d_r);
    launch_path_solve_t<double>(t->W, t->ld, n, d_r, d_z, d_v, t->npad, S, st);
  } else {
    hipLaunchKernelGGL((path_rhs_kernel<float>), dim3(gb), dim3(256), 0, st, (const float*)k->resid, d_sums, (const float*)d_eps, A, sns, n, S, (int64_t)t->npad, d_r);
    launch_path_solve_t<float>(t->W, t->ld, n, d_r, d_z, d_v, t->npad, S, st);
  }
  return HBO_OK;
}

extern "C" int hbo_sample_paths(hbo_ctx* c, const hbo_model* m, hbo_cache* k, const void* xq, int64_t M, int32_t S, int32_t F,
                                const void* omega, const void* phase, const void* w, const void* eps, void* out) {
  const std::string fn = "hbo_sample_paths: ";
  // ---- every argument check, before any device call ----
  if (!m || !xq || !omega || !phase || !w || !out) return fail(c, HBO_ERR_ARG, fn + "null argument");
  int rc = path_check(c, fn, m, k, S, F, eps != nullptr);
  if (rc) return rc;
  const int dtype = m->dtype, D = m->input_dim, fdim = feature_dim(m);
  const bool is_dot = m->kernel_id == HBO_KERNEL_DOT;
  if (!c) return fail(c, HBO_ERR_ARG, fn + "ctx is null");
  if (M <= 0) return HBO_OK;
  HIPCHK(c, hipSetDevice(c->device));
  prof_begin(c);
  rc = upload_model(c, m);
  if (rc) return rc;
  const size_t es = esize(dtype);
  hipStream_t st = c->stream;
  TaskHost* t = k ? k->t : nullptr;
  const int n = t ? (int)t->n : 0;
  // queries stream in chunks of post_chunk, as hbo_predict's do
  const int64_t CH = std::max<int64_t>(c->opt_post_chunk, HBO_TILE), mc_max = std::min<int64_t>(M, CH);
  const int mpad_max = round_up(mc_max, HBO_TILE);
  const int64_t ldq_max = padded_ld(mpad_max, dtype);
  void* d_xq = ws_get(c, WS_XQ, (size_t)M * D * es);
  void* d_mu0 = ws_get(c, WS_MU0, (size_t)mc_max * es);
  void* d_kd = ws_get(c, WS_KD, (size_t)mc_max * es);
  void* d_out = ws_get(c, WS_PATH_OUT, (size_t)mc_max * S * es);
  if (!d_xq || !d_mu0 || !d_kd || !d_out) return HBO_ERR_HIP;
  void* d_kwq = is_kumar(m) ? ws_get(c, WS_KW_Q, (size_t)mc_max * D * es) : nullptr;
  if (is_kumar(m) && !d_kwq) return HBO_ERR_HIP;
  void* fq_acts[HBO_MAX_MLP_LAYERS] = {nullptr};
  if (needs_mlp(m)) for (int l = 0; l < m->n_layers; ++l) { fq_acts[l] = ws_get(c, WS_FQ0 + l, (size_t)mc_max * m->features[l] * es); if (!fq_acts[l]) return HBO_ERR_HIP; }
  void* d_K = nullptr;
  if (t) {
    d_K = ws_get(c, WS_K, (size_t)t->npad * ldq_max * es);
    if (!d_K) return HBO_ERR_HIP;
  }
  HIPCHK(c, hipMemcpyAsync(d_xq, xq, (size_t)M * D * es, hipMemcpyHostToDevice, st));
  PathSolve sol = {};
  rc = path_solve(c, m, k, S, F, omega, phase, w, eps, 1.0, mc_max, &sol);
  if (rc) return rc;
  double* d_sums = sol.sums; double* d_v = sol.v;
  const double A = sol.A;
  PathPriorArgs pa = {};
  pa.fdim = fdim; pa.omega = sol.om; pa.phase = sol.ph; pa.w = sol.w; pa.F = F; pa.S = S; pa.is_dot = is_dot; pa.sums = d_sums;
  const bool bad = k && k->info != INT_MAX;
  for (int64_t q0 = 0; q0 < M && !bad; q0 += CH) {
    const int64_t mc = std::min<int64_t>(CH, M - q0);
    const int mpad = round_up(mc, HBO_TILE);
    const int64_t ldq = padded_ld(mpad, dtype);
    const void* xc = (const char*)d_xq + (size_t)q0 * D * es;
    const void* Fq = query_features(c, m, c->d_model, c->d_mlp_w, c->d_mlp_b, xc, mc, fq_acts, d_kwq, d_mu0, d_kd, st, true).Fq;
    { ProfScope ps(c, "path_prior", 1);
      pa.feat = Fq; pa.rows = mc;
      launch_path_prior(dtype, pa, c->d_model, st); }
    if (t) {
      ProfScope ps(c, "cross_gram", 1);
      GramArgs g = {}; g.kernel_id = m->kernel_id; g.mfma_min_f = c->opt_gram_mfma; g.x1 = k->h_desc.F; g.x2 = Fq; g.out = d_K; g.n1 = n; g.n2 = mc; g.ldo = ldq;
      g.n1pad = t->npad; g.n2pad = mpad; g.fdim = fdim; g.symmetric = 0; g.padded = 1;
      launch_gram(dtype, g, c->d_model, dim3(mpad / HBO_TILE, t->nblk, 1), st);
    }
    { ProfScope ps(c, "path_update", 1);
      const dim3 grid((unsigned)((mc + 63) / 64), (unsigned)((S + PATH_SC - 1) / PATH_SC));
      if (dtype == HBO_F64)
        hipLaunchKernelGGL((path_update_kernel<double>), grid, dim3(256), 0, st, (const double*)d_K, ldq, n, d_v, (int64_t)(t ? t->npad : 0), d_sums, A,
                           (const double*)d_mu0, mc, S, (double*)d_out);
      else
        hipLaunchKernelGGL((path_update_kernel<float>), grid, dim3(256), 0, st, (const float*)d_K, ldq, n, d_v, (int64_t)(t ? t->npad : 0), d_sums, A,
                           (const float*)d_mu0, mc, S, (float*)d_out); }
    // (the next chunk overwrites d_out: the copy is waited for)
    HIPCHK(c, hipMemcpyAsync((char*)out + (size_t)q0 * S * es, d_out, (size_t)mc * S * es, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
  }
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  prof_collect(c);
  if (bad) { fill_nan(out, (size_t)M * S, dtype); return HBO_NOT_PD; }
  return HBO_OK;
}
