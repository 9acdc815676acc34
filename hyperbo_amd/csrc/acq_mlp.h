// The MLP basis inside the per-pair acquisition kernels (acq_small.hip, acq_blocked.hip): forward and backward pass of one query through
// the tanh stack of basis_functions.py:24-36 by the 256-thread workgroup that owns the (sample, query) pair, and the tail that joins
// the feature-space and raw-space pieces of d acquisition / d x.
//   forward   h_0 = x,  z_j = b_j + sum_i W_l[i][j] h_{l-1,i} (i rising, one thread per output j: the reads of the row-major [in][out]
//             weights coalesce along j),  h_l = tanh(z)
//   backward  dz_j = g_j (1 - h_{l,j}^2),  g'_i = sum_j W_l[i][j] dz_j: a wave per input row, lanes along j, wave_sum -- the order of
//             the sum is fixed by the layer's shape alone
// Weights and biases are read in the model dtype from the sample's own block (AcqSmallArgs::mlp_w / mlp_b); every product and sum is
// fp64; no atomics.  All L <= 8 layers of <= 256 outputs stay in fp64 LDS: act[l * HBO_MAX_FEATURE_DIM + j], 16 KB.
#pragma once
#include "kernfun.h"

namespace {
enum { ACQ_FEAT_KERNEL = 1, ACQ_FEAT_MEAN = 2 };   // AcqSmallArgs::feat: who reads the last layer

// x [D] (LDS) -> act (LDS).  Ends behind a barrier: every thread may read every layer.
template <typename T>
__device__ __forceinline__ void acq_mlp_fwd_block(const AcqSmallArgs& a, int s, const double* x, double* act) {
  const int tid = threadIdx.x;
  const double* in = x;
  int fin = a.D;
  for (int l = 0; l < a.L; ++l) {
    const int fout = a.fout[l];
    const T* w = static_cast<const T*>(a.mlp_w[(int64_t)s * HBO_MAX_MLP_LAYERS + l]);
    const T* b = static_cast<const T*>(a.mlp_b[(int64_t)s * HBO_MAX_MLP_LAYERS + l]);
    double* out = act + l * HBO_MAX_FEATURE_DIM;
    if (tid < fout) {
      double z = (double)b[tid];
      for (int i = 0; i < fin; ++i) z += (double)w[(int64_t)i * fout + tid] * in[i];
      out[tid] = tanh(z);
    }
    __syncthreads();
    in = out; fin = fout;
  }
}

// g (LDS, [fout of the last layer], written by the caller behind no barrier) -> d / d x [D]; returns the buffer that holds it (g or
// tmp, both [HBO_MAX_FEATURE_DIM] of LDS), behind a barrier.
template <typename T>
__device__ __forceinline__ double* acq_mlp_bwd_block(const AcqSmallArgs& a, int s, const double* act, double* g, double* tmp) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __syncthreads();
  for (int l = a.L - 1; l >= 0; --l) {
    const int fout = a.fout[l], fin = l ? a.fout[l - 1] : a.D;
    const T* w = static_cast<const T*>(a.mlp_w[(int64_t)s * HBO_MAX_MLP_LAYERS + l]);
    const double* h = act + l * HBO_MAX_FEATURE_DIM;
    if (tid < fout) g[tid] *= 1.0 - h[tid] * h[tid];
    __syncthreads();
    // four rows of loads in flight per wave; a row beyond fin reads the last row and is dropped
    for (int i0 = wave; i0 < fin; i0 += 16) {
      double p[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * r, ic = i < fin ? i : fin - 1;
        double acc = 0;
        for (int j = lane; j < fout; j += 64) acc += (double)w[(int64_t)ic * fout + j] * g[j];
        p[r] = acc;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double v = wave_sum(p[r]);
        if (lane == 0 && i0 + 4 * r < fin) tmp[i0 + 4 * r] = v;
      }
    }
    __syncthreads();
    double* t = g; g = tmp; tmp = t;
  }
  return g;
}

// The end of a pair with an MLP basis.  gk (LDS, [fdim], complete behind the caller's last barrier or written by the calling threads
// themselves at index tid): the gradient in the kernel's own space; the mean's a_mu . w term is added in the mean's own space; the
// backward pass takes the sum of the feature-space pieces, the raw-space pieces are added to its result.  wlin: the sample's linear
// mean weights [mean width].
template <typename T, int FEAT>
__device__ __forceinline__ void acq_mlp_tail(const AcqSmallArgs& a, int s, const double* act, const double* gk, const double* wlin,
                                             double amu, double* top, double* tmp, double* g_out) {
  const int tid = threadIdx.x;
  const int flast = a.fout[a.L - 1];
  __syncthreads();
  if (tid < flast) {
    double v = 0.0;
    if constexpr ((FEAT & ACQ_FEAT_KERNEL) != 0) v = gk[tid];
    if (a.mean_id == HBO_MEAN_LINEAR_MLP) v += amu * wlin[tid];
    top[tid] = v;
  }
  const double* gx = acq_mlp_bwd_block<T>(a, s, act, top, tmp);
  for (int d = tid; d < a.D; d += 256) {
    double r = gx[d];
    if constexpr ((FEAT & ACQ_FEAT_KERNEL) == 0) r += gk[d];
    if (a.mean_id == HBO_MEAN_LINEAR) r += amu * wlin[d];
    g_out[d] = r;
  }
}
}  // namespace
