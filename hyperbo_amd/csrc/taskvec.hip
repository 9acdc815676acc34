// What surrounds the Gram of a task on gfx950 and is not the Gram itself: the augmented residual rows (aug_rows), the NLL reduction
// (nll_reduce), s = W^T z (the two wtz kernels), the poison kernel of the tests, the row helpers of the divergence objectives
// (expand_rows, add_sumsq), the dense import / export helpers of hbo_spd_solve / hbo_cache_export (extract_lower, symmetrize, fill_spd,
// set_aug), and the single-matrix MLP layer and mean (dense_tanh, mean).  One thread per element or a short reduction each: bound by
// HBM or by launch latency, none of them a pair kernel.
//
// Reference restated: hyperbo/gp_utils/basis_functions.py:24-36 (MLP), mean.py:30-79, objectives.py:144-156 (NLL).
#include "kernfun.h"

namespace {

// out[i][o] = tanh(sum_k in[i][k] w[k][o] + b[o])   (flax Dense + tanh)
template <typename T>
__global__ void dense_tanh_kernel(const T* __restrict__ in, const T* __restrict__ w, const T* __restrict__ b,
                                  T* __restrict__ out, int64_t n, int fin, int fout) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * fout) return;
  const int64_t i = idx / fout;
  const int o = (int)(idx % fout);
  T s = b[o];
  for (int k = 0; k < fin; ++k) s += in[i * fin + k] * w[(int64_t)k * fout + o];
  out[idx] = tanh(s);
}

template <typename T>
__global__ void mean_kernel(const T* __restrict__ fm, int64_t n, int fmean, const ModelDev* __restrict__ md,
                            T* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = mean_at<T>(md, fm, fmean, i);
}

// augmented tile-row: row b < naug holds  aug_src[b*n + j] + e_b * mu_j  (see TaskDesc); everything else zero.
template <typename T>
__global__ void aug_rows_kernel(const TaskDesc* tasks, const ModelDev* __restrict__ md, int model_stride) {
  const TaskDesc& t = tasks[blockIdx.z];
  md += (int64_t)blockIdx.z * model_stride;
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= t.npad) return;
  T* Ar = static_cast<T*>(t.A) + (int64_t)t.npad * t.ld + j;
  const T* ys = static_cast<const T*>(t.ysum);
  T mu = (T)0;
  if (j < t.n) mu = mean_at<T>(md, static_cast<const T*>(t.Fm), t.fmean, j);
  for (int a = 0; a < HBO_TILE; ++a) {
    T v = (T)0;
    if (a < t.naug && j < t.n) {
      const T e = (T)(t.e_all + (a == t.naug - 1 ? t.e_last : 0.0));
      v = ys[(int64_t)(a == t.naug - 1 ? t.last_src : a) * t.n + j] + e * mu;
    }
    Ar[(int64_t)a * t.ld] = v;
  }
}

// f_t = c * sum_b |z_b|^2 + 2 lh * sum log diag L + const   (NLL: objectives.py:153-155; EKL: utils.py:84-106)
template <typename T>
__global__ __launch_bounds__(256) void nll_reduce_kernel(const TaskDesc* tasks, const int* info, double* out) {
  __shared__ double sred[4];
  const TaskDesc& t = tasks[blockIdx.x];
  const T* A = static_cast<const T*>(t.A);
  double ld_sum = 0, q = 0;
  // four elements per thread and pass: the strided diagonal loads of a pass are in flight together (this kernel, the
  // dmu and the finalize kernel sit serially at the end of an evaluation: 36 + 25 + 55 us before)
  for (int64_t i0 = threadIdx.x; i0 < t.n; i0 += 1024) {
    T dg[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int64_t i = i0 + 256 * u; dg[u] = i < t.n ? A[i * t.ld + i] : (T)1; }
    for (int b = 0; b < t.naug; ++b) {
      const T* zr = A + ((int64_t)t.npad + b) * t.ld;
#pragma unroll
      for (int u = 0; u < 4; ++u) { const int64_t i = i0 + 256 * u; const double z = i < t.n ? (double)zr[i] : 0.0; q += z * z; }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) ld_sum += log((double)dg[u]);
  }
  ld_sum = block_sum(ld_sum, sred);
  q = block_sum(q, sred);
  if (threadIdx.x == 0) {
    double v = t.coef_c * q + 2.0 * t.coef_lh * ld_sum + t.coef_const;
    if (info[blockIdx.x] != 0x7fffffff) v = NAN;
    out[blockIdx.x] = v;
  }
}

// s = W^T z, stage 1: partial[rc][col] over 512-row chunks, stored in the scratch matrix S.
template <typename T>
__global__ __launch_bounds__(256) void wtz_partial_kernel(const TaskDesc* tasks, int aug_row, const T* xover) {
  __shared__ T sred[256];
  const TaskDesc& t = tasks[blockIdx.z];
  const int cb = blockIdx.x, rc = blockIdx.y;
  if (cb >= t.nblk || (!xover && aug_row >= t.naug)) return;
  const int64_t row_lo = (int64_t)rc * 512;
  if (row_lo >= t.npad) return;
  T* part = static_cast<T*>(t.wscr) + (int64_t)rc * t.ld + (int64_t)cb * HBO_TILE;
  const int col = threadIdx.x & 127, half = threadIdx.x >> 7;
  T acc = (T)0;
  if (row_lo + 512 > (int64_t)cb * HBO_TILE) {  // chunk reaches the lower triangle
    const T* W = static_cast<const T*>(t.W);
    const T* z = xover ? xover : static_cast<const T*>(t.A) + ((int64_t)t.npad + aug_row) * t.ld;
    int64_t r_begin = row_lo + half * 256, r_end = r_begin + 256;
    if (r_end > t.npad) r_end = t.npad;
    const int64_t diag0 = (int64_t)cb * HBO_TILE;
    if (r_begin < diag0) r_begin = diag0;
    // eight independent accumulators: the loads of a row group are in flight together (a single dependent chain ran
    // at 1.9 TB/s and took 31 us on one 128-row block; four: 2.7 TB/s)
    T a[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] = (T)0;
    const T* wp = W + diag0 + col;
    int64_t r = r_begin;
    for (; r + 8 <= r_end; r += 8) {
      T w[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) w[u] = wp[(r + u) * t.ld];
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] += w[u] * z[r + u];
    }
    for (; r < r_end; ++r) a[0] += wp[r * t.ld] * z[r];
    acc = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  }
  sred[threadIdx.x] = acc;
  __syncthreads();
  if (half == 0) part[col] = sred[col] + sred[col + 128];
}
template <typename T>
__global__ void wtz_final_kernel(const TaskDesc* tasks, int out_col, int out_ld, T* oover) {
  const TaskDesc& t = tasks[blockIdx.z];
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= t.npad || (!oover && out_col >= t.naug)) return;
  const T* part = static_cast<const T*>(t.wscr);
  const int nrc = (t.npad + 511) / 512;
  T s = (T)0;
  for (int rc = 0; rc < nrc; ++rc) s += part[(int64_t)rc * t.ld + j];
  if (oover) oover[j] = s;
  else static_cast<T*>(t.svec)[(int64_t)out_col * t.npad + j] = s;   // per-task stride (ragged tasks)
}

// rows of n elements -> rows of npad elements, zero padded (the data rows of a divergence objective with more than 127 aligned columns)
template <typename T>
__global__ void expand_rows_kernel(const T* __restrict__ src, int64_t n, int npad, T* __restrict__ dst) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= npad) return;
  dst[(int64_t)blockIdx.y * npad + j] = j < n ? src[(int64_t)blockIdx.y * n + j] : (T)0;
}
// value[0] += coef * sum over `count` rows of npad elements of z^2 (one workgroup: the rows are few and short)
template <typename T>
__global__ __launch_bounds__(256) void add_sumsq_kernel(const T* __restrict__ z, int64_t total, double coef, double* value) {
  __shared__ double sred[4];
  double q = 0;
  for (int64_t i = threadIdx.x; i < total; i += 256) { const double v = (double)z[i]; q += v * v; }
  q = block_sum(q, sred);
  if (threadIdx.x == 0) value[0] += coef * q;
}
template <typename T>
__global__ void extract_lower_kernel(const T* __restrict__ A, int64_t ld, int64_t n, T* out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t r = blockIdx.y;
  if (c >= n) return;
  out[r * n + c] = (c <= r) ? A[r * ld + c] : (T)0;
}
template <typename T>
__global__ void symmetrize_kernel(const T* __restrict__ S, int64_t ld, int64_t n, T* out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t r = blockIdx.y;
  if (c >= n) return;
  // lower tiles of S are valid (full 128x128 tiles on and below the tile diagonal)
  const bool lower_tile = (c / HBO_TILE) <= (r / HBO_TILE);
  out[r * n + c] = lower_tile ? S[r * ld + c] : S[c * ld + r];
}
// dense SPD (n x n host layout, already on device) -> padded A (identity on the padded diagonal)
template <typename T>
__global__ void fill_spd_kernel(const T* __restrict__ a, int64_t n, T* A, int64_t ld, int npad) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t r = blockIdx.y;
  if (c >= npad) return;
  T v;
  if (r < n && c < n) v = a[r * n + c];
  else v = (r == c) ? (T)1 : (T)0;
  A[r * ld + c] = v;
}
// augmented rows from b (n x m, row-major): A[(npad+a)*ld + j] = b[j*m + a]; the rest zero
template <typename T>
__global__ void set_aug_kernel(const T* __restrict__ b, int64_t n, int m, T* A, int64_t ld, int npad) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int a = blockIdx.y;
  if (j >= npad) return;
  T v = (T)0;
  if (b && a < m && j < n) v = b[j * m + a];
  A[((int64_t)npad + a) * ld + j] = v;
}

}  // namespace

// hbo_tune "poison" (tests): everything an evaluation is about to recompute is set to NaN first -- the lower triangles of A (Gram -> L)
// and W (L^-1; the zeros above its diagonal are an invariant of the buffer and stay), all of S (scratch -> K^-1), alpha and d f / d mu.
// A launch that silently skips work (a tile counter shared by two launches, a K range cut short) then shows up as NaN instead of hiding
// behind the previous evaluation's identical numbers in the same buffers.  The augmented tile-row (rows npad...) is left alone: its
// unused rows are independent of every result, and the fp32 split's scale measurement reads the whole tile-row.
template <typename T>
__global__ __launch_bounds__(256) void poison_kernel(const TaskDesc* tasks) {
  const TaskDesc& t = tasks[blockIdx.z];
  const int64_t row = blockIdx.x;
  if (row >= t.npad) return;
  const T nanv = (T)NAN;
  T* A = static_cast<T*>(t.A) + row * t.ld;
  T* W = t.W ? static_cast<T*>(t.W) + row * t.ld : nullptr;
  T* S = t.S ? static_cast<T*>(t.S) + row * t.ld : nullptr;
  for (int64_t cc = threadIdx.x; cc < t.npad; cc += blockDim.x) {
    if (cc <= row) { A[cc] = nanv; if (W) W[cc] = nanv; }
    if (S) S[cc] = nanv;
  }
  if (row == 0) {
    const int ncol = t.nvec ? t.nvec : (t.naug > 0 ? t.naug : 1);
    if (t.svec) for (int64_t cc = threadIdx.x; cc < (int64_t)t.npad * ncol; cc += blockDim.x) static_cast<T*>(t.svec)[cc] = nanv;
    if (t.dmu) for (int64_t cc = threadIdx.x; cc < t.npad; cc += blockDim.x) static_cast<double*>(t.dmu)[cc] = (double)NAN;
  }
}

void launch_expand_rows(int dtype, const void* src, int64_t n, int npad, void* dst, int count, hipStream_t st) {
  if (count <= 0) return;
  const dim3 grid((npad + 255) / 256, count);
  dispatch_dtype(dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    hipLaunchKernelGGL((expand_rows_kernel<T>), grid, dim3(256), 0, st, (const T*)src, n, npad, (T*)dst);
  });
}
void launch_add_sumsq(int dtype, const void* z, int npad, int count, double coef, double* value, hipStream_t st) {
  if (count <= 0) return;
  dispatch_dtype(dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    hipLaunchKernelGGL((add_sumsq_kernel<T>), dim3(1), dim3(256), 0, st, (const T*)z, (int64_t)npad * count, coef, value);
  });
}
void launch_dense_tanh(int dtype, const void* in, const void* w, const void* b, void* out, int64_t n, int fin,
                       int fout, hipStream_t st) {
  if (n <= 0) return;
  dim3 grid((unsigned)((n * fout + 255) / 256));
  dispatch_dtype(dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    hipLaunchKernelGGL((dense_tanh_kernel<T>), grid, dim3(256), 0, st, (const T*)in, (const T*)w, (const T*)b, (T*)out, n, fin, fout);
  });
}
void launch_mean(int dtype, const void* fm, int64_t n, int fmean, const ModelDev* md, void* mu, hipStream_t st) {
  if (n <= 0) return;
  dim3 grid((unsigned)((n + 255) / 256));
  dispatch_dtype(dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    hipLaunchKernelGGL((mean_kernel<T>), grid, dim3(256), 0, st, (const T*)fm, n, fmean, md, (T*)mu);
  });
}
void launch_poison(int dtype, const TaskDesc* tasks, int ntasks, int max_npad, hipStream_t st) {
  dim3 grid(max_npad, 1, ntasks);
  dispatch_dtype(dtype, [&](auto tag) {
    hipLaunchKernelGGL((poison_kernel<typename decltype(tag)::type>), grid, dim3(256), 0, st, tasks);
  });
}
void launch_aug_rows(int dtype, const TaskDesc* tasks, int ntasks, int max_npad, const ModelDev* md, hipStream_t st, int model_stride) {
  dim3 grid((max_npad + 255) / 256, 1, ntasks);
  dispatch_dtype(dtype, [&](auto tag) {
    hipLaunchKernelGGL((aug_rows_kernel<typename decltype(tag)::type>), grid, dim3(256), 0, st, tasks, md, model_stride);
  });
}
void launch_nll_reduce(int dtype, const TaskDesc* tasks, int ntasks, const int* info, double* out, hipStream_t st) {
  dispatch_dtype(dtype, [&](auto tag) {
    hipLaunchKernelGGL((nll_reduce_kernel<typename decltype(tag)::type>), dim3(ntasks), dim3(256), 0, st, tasks, info, out);
  });
}
void launch_wt_z(int dtype, const TaskDesc* tasks, int ntasks, int max_nblk, int aug_row, int out_col,
                 int out_ld, hipStream_t st, const void* xover, void* oover) {
  const int max_npad = max_nblk * HBO_TILE;
  dim3 g1(max_nblk, (max_npad + 511) / 512, ntasks);
  dim3 g2((max_npad + 255) / 256, 1, ntasks);
  dispatch_dtype(dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    hipLaunchKernelGGL((wtz_partial_kernel<T>), g1, dim3(256), 0, st, tasks, aug_row, (const T*)xover);
    hipLaunchKernelGGL((wtz_final_kernel<T>), g2, dim3(256), 0, st, tasks, out_col, out_ld, (T*)oover);
  });
}
void launch_extract_lower(int dtype, const void* A, int64_t ld, int64_t n, void* out, hipStream_t st) {
  if (n <= 0) return;
  dim3 grid((unsigned)((n + 255) / 256), (unsigned)n);
  dispatch_dtype(dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    hipLaunchKernelGGL((extract_lower_kernel<T>), grid, dim3(256), 0, st, (const T*)A, ld, n, (T*)out);
  });
}
void launch_symmetrize_from_lower(int dtype, const void* S, int64_t ld, int64_t n, void* out, hipStream_t st) {
  if (n <= 0) return;
  dim3 grid((unsigned)((n + 255) / 256), (unsigned)n);
  dispatch_dtype(dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    hipLaunchKernelGGL((symmetrize_kernel<T>), grid, dim3(256), 0, st, (const T*)S, ld, n, (T*)out);
  });
}
void launch_fill_spd(int dtype, const void* a, int64_t n, void* A, int64_t ld, int npad, hipStream_t st) {
  dim3 grid((npad + 255) / 256, npad);
  dispatch_dtype(dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    hipLaunchKernelGGL((fill_spd_kernel<T>), grid, dim3(256), 0, st, (const T*)a, n, (T*)A, ld, npad);
  });
}
void launch_set_aug(int dtype, const void* b, int64_t n, int m, void* A, int64_t ld, int npad, hipStream_t st) {
  dim3 grid((npad + 255) / 256, HBO_TILE);
  dispatch_dtype(dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    hipLaunchKernelGGL((set_aug_kernel<T>), grid, dim3(256), 0, st, (const T*)b, n, m, (T*)A, ld, npad);
  });
}
