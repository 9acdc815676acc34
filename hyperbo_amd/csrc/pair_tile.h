// The pair tile of the blocked element-wise kernels (gram.hip: gram_kernel; grad.hip: grad_contract_kernel, grad_feat_kernel;
// kumar.hip: kumar_contract_kernel), once: a 256-thread workgroup holds 16 NR rows x 128 columns of pairs, thread (ty, tx) =
// (tid >> 4, tid & 15) the rows ty + 16 a (a < NR) and eight columns in 16-byte groups (pt_col).  The features of the rows and
// columns are staged DC at a time (kernfun.h: stage_x), and acc[a][q] becomes the scaled squared distance sum (a - b)^2, or the
// inner product sum a b of the dot-product covariance.  Everything here is a compile-time shape: no helper takes a run-time switch.
// grad_feat_kernel and kumar_contract_kernel run all of it.  gram_kernel and grad_contract_kernel take the column index, the
// coefficients and (the second pass of the latter) the staging and the read, and keep a copy of pt_accumulate's loop each: inlined from
// here the same text costs them 2 to 10 registers, enough to lose a wave per SIMD (profiles/pair_tile_refactor.md).
#pragma once
#include "kernfun.h"

namespace {

// column, from the tile's first, of element q of a thread's eight: VEC = 16 bytes of consecutive columns per thread and group of 16 VEC
template <typename T>
__device__ __forceinline__ constexpr int pt_col(int tx, int q) {
  constexpr int VEC = 16 / sizeof(T);
  return 16 * VEC * (q / VEC) + VEC * tx + (q % VEC);
}

// the thread's NR row values and eight column values of staged feature dd
template <typename T, int NR>
__device__ __forceinline__ void pt_read(const T* sA, const T* sB, int dd, int tx, int ty, T (&av)[NR], T (&bv)[8]) {
#pragma unroll
  for (int a = 0; a < NR; ++a) av[a] = sA[dd * SXS + ty + 16 * a];
#pragma unroll
  for (int q = 0; q < 8; ++q) bv[q] = sB[dd * SXS + pt_col<T>(tx, q)];
}

// features [d0, d0 + DC) of rows r0... of x1 into sA and of rows c0... of x2 into sB ([DC * SXS] of LDS each), over 1 / lengthscale
// unless DOT, behind a barrier and in front of one; returns how many of the DC are features
template <typename T, int NR, bool DOT>
__device__ __forceinline__ int pt_stage(T* sA, T* sB, const T* x1, int64_t n1, const T* x2, int64_t n2, int fdim, int64_t r0, int64_t c0,
                                        int d0, const double* inv_ls, int tid) {
  __syncthreads();
  stage_x<T, NR>(sA, x1, n1, fdim, r0, d0, inv_ls, !DOT, tid);
  stage_x<T, 8>(sB, x2, n2, fdim, c0, d0, inv_ls, !DOT, tid);
  __syncthreads();
  return (fdim - d0) < DC ? (fdim - d0) : DC;
}

// acc += over all features of the pairs (rows r0... of x1) x (rows c0... of x2)
template <typename T, int NR, bool DOT>
__device__ __forceinline__ void pt_accumulate(T (&acc)[NR][8], T* sA, T* sB, const T* x1, int64_t n1, const T* x2, int64_t n2, int fdim,
                                              int64_t r0, int64_t c0, const double* inv_ls, int tid) {
  const int tx = tid & 15, ty = tid >> 4;
  for (int d0 = 0; d0 < fdim; d0 += DC) {
    const int dlim = pt_stage<T, NR, DOT>(sA, sB, x1, n1, x2, n2, fdim, r0, c0, d0, inv_ls, tid);
    // (left to the compiler, no unroll pragma: gram_kernel records what forcing it by 4 or 16 costs)
    for (int dd = 0; dd < dlim; ++dd) {
      T av[NR], bv[8];
      pt_read<T, NR>(sA, sB, dd, tx, ty, av, bv);
#pragma unroll
      for (int a = 0; a < NR; ++a)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          if (DOT) acc[a][q] += av[a] * bv[q];
          else { const T df = av[a] - bv[q]; acc[a][q] += df * df; }
        }
    }
  }
}

// what the covariance functions (kernfun.h: kfun, dk_du) and G take from the model, in the model dtype
template <typename T> struct PairCoef { T sv, inv_sigma2, bias2, noise; };
template <typename T>
__device__ __forceinline__ PairCoef<T> pair_coef(const ModelDev* md) {
  return {(T)md->sv, (T)(1.0 / (md->dot_sigma * md->dot_sigma)), (T)(md->dot_bias * md->dot_bias), (T)md->noise};
}

// In place on the 8 x 8 micro-tile of a 128 x 128 tile of task t: acc = u (what pt_accumulate left) -> g = G_ij dk/du (dot product:
// G_ij), 0 beyond the data, with G = d objective / d K1 as at the head of grad.hip:
//   NLL / EKL: lh S_ij - c sum_b v_b,i v_b,j     EUC: k_ij + [i == j] noise - sum_b v_b,i v_b,j     (v: outer_vecs)
template <typename T, int KID>
__device__ __forceinline__ void pt_g_dkdu(T (&acc)[8][8], const TaskDesc& t, const ModelDev* md, bool euc, const T* vecs, int64_t vstride,
                                          int nvec, int64_t r0, int64_t c0, int tx, int ty) {
  constexpr bool is_dot = (KID == HBO_KERNEL_DOT);
  const ExpLit ec;
  const PairCoef<T> pc = pair_coef<T>(md);
  const T lh = (T)t.coef_lh, cc = (T)t.coef_c;
  const T* S = static_cast<const T*>(t.S);
  const int64_t n = t.n;
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    const int64_t row = r0 + ty + 16 * a;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int64_t col = c0 + pt_col<T>(tx, q);
      T g = (T)0;
      if (row < n && col < n) {
        const T u = acc[a][q];
        const T k = kfun(KID, u, pc.sv, pc.inv_sigma2, pc.bias2, ec);
        T outer = (T)0;
        for (int b = 0; b < nvec; ++b) outer += vecs[(int64_t)b * vstride + row] * vecs[(int64_t)b * vstride + col];
        const T G = euc ? (k + (row == col ? pc.noise : (T)0) - outer) : (lh * S[row * t.ld + col] - cc * outer);
        if (is_dot) g = G;
        else g = G * dk_du(KID, u, k, pc.sv, ec);
      }
      acc[a][q] = g;
    }
  }
}
}  // namespace
