// The Gram matrix on gfx950: the pairwise-kernel build on the vector units (gram_kernel: the pair tile of pair_tile.h, coalesced
// 16-byte stores, fused +(sigma^2+eps) I), the fp32 build of the stationary covariances on the matrix cores (gram_mfma_*), and the
// diagonal k(x, x) (kdiag_kernel).  What surrounds the Gram of a task -- residual rows, NLL reduction, W^T z -- is taskvec.hip.
//
// Reference restated: hyperbo/gp_utils/kernel.py:29-145 (Gram), basics/linalg.py:36-69 (jitter).
#include "pair_tile.h"

namespace {

// The two epilogues of gram_kernel share these: the value of an element from its accumulator, and the store of a vector of them.
// Ablation builds (tools/gram_time.py): HBO_GRAM_NOEXP leaves the covariance function out, HBO_GRAM_NOSTORE the stores (behind a test
// no value passes, so that the values stay live).
template <int KID, typename T>
__device__ __forceinline__ T gram_value(T u, const PairCoef<T>& pc, const ExpCoef& ec) {
#ifdef HBO_GRAM_NOEXP
  return u * pc.sv;
#else
  return kfun(KID, u, pc.sv, pc.inv_sigma2, pc.bias2, ec);
#endif
}
template <typename T>
__device__ __forceinline__ void gram_store(T* p, typename V16<T>::type vv) {
#ifdef HBO_GRAM_NOSTORE
  if (vv[0] == (T)123.456)
#endif
  gst(reinterpret_cast<typename V16<T>::type*>(p), vv);
}

// KID: covariance id as a compile-time constant -- with a run-time id every one of a thread's 32 elements carried the
// switch over all four covariances (188 VGPRs, 2 waves per SIMD, constants re-materialised per exponential)
template <typename T, bool PADDED, int KID>
__global__ __launch_bounds__(256) void gram_kernel(GramArgs g, const ModelDev* __restrict__ md) {
  typedef typename V16<T>::type vec_t;
  constexpr int VEC = 16 / sizeof(T);
  __shared__ T sA[DC * SXS];
  __shared__ T sB[DC * SXS];
  // ti in units of GTR rows, tj in units of 128 columns.  Symmetric mode computes the tiles with tj <= ti/2 only, and
  // workgroup i runs on XCD (i + const) mod 8: with tj = blockIdx.x the low XCDs would get one more tile than the high ones in
  // every row (grid.x is a multiple of 8 for the sizes that matter), so the column index is rotated by the row
  const int ti = blockIdx.y;
  const int tj = g.symmetric ? (int)((blockIdx.x + blockIdx.y) % gridDim.x) : (int)blockIdx.x;
  const T* x1; const T* x2; T* out; int64_t n1, n2, ldo; int64_t e1, e2;  // e*: padded extents
  if (g.tasks) {
    const TaskDesc& t = g.tasks[blockIdx.z];
    md += (int64_t)blockIdx.z * g.model_stride;
    if ((int64_t)ti * GTR >= t.npad || tj >= t.nblk) return;
    x1 = x2 = static_cast<const T*>(t.F);
    out = static_cast<T*>(t.A);
    n1 = n2 = t.n; ldo = t.ld; e1 = e2 = t.npad;
  } else {
    x1 = static_cast<const T*>(g.x1); x2 = static_cast<const T*>(g.x2); out = static_cast<T*>(g.out);
    n1 = g.n1; n2 = g.n2; ldo = g.ldo; e1 = PADDED ? g.n1pad : g.n1; e2 = PADDED ? g.n2pad : g.n2;
  }
  const int64_t r0 = (int64_t)ti * GTR, c0 = (int64_t)tj * HBO_TILE;
  if (g.symmetric && c0 > r0 + GTR - 1) return;   // entirely above the diagonal
  const int fdim = g.fdim;
  constexpr int kid = KID;
  constexpr bool is_dot = (kid == HBO_KERNEL_DOT);
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;

  T acc[GRA][8];
#pragma unroll
  for (int a = 0; a < GRA; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[a][b] = (T)0;

  // (its own copy of pt_accumulate: through the helper <double, true, SE> takes 130 VGPRs for 128, three waves per SIMD for four)
  for (int d0 = 0; d0 < fdim; d0 += DC) {
    __syncthreads();
    stage_x<T, GRA>(sA, x1, n1, fdim, r0, d0, md->inv_ls, !is_dot, tid);
    stage_x<T, 8>(sB, x2, n2, fdim, c0, d0, md->inv_ls, !is_dot, tid);
    __syncthreads();
    const int dlim = (fdim - d0) < DC ? (fdim - d0) : DC;
    auto step = [&](int dd) {
      T av[GRA], bv[8];
#pragma unroll
      for (int a = 0; a < GRA; ++a) av[a] = sA[dd * SXS + ty + 16 * a];
#pragma unroll
      for (int q = 0; q < 8; ++q) bv[q] = sB[dd * SXS + pt_col<T>(tx, q)];
      if (is_dot) {
#pragma unroll
        for (int a = 0; a < GRA; ++a)
#pragma unroll
          for (int q = 0; q < 8; ++q) acc[a][q] += av[a] * bv[q];
      } else {
#pragma unroll
        for (int a = 0; a < GRA; ++a)
#pragma unroll
          for (int q = 0; q < 8; ++q) { const T df = av[a] - bv[q]; acc[a][q] += df * df; }
      }
    };
    // (not unrolled: by 4 or 16 the LDS reads of all the steps are hoisted -- 232-238 VGPRs, two waves per SIMD)
    for (int dd = 0; dd < dlim; ++dd) step(dd);
  }

  const ExpCoef ec = hbo_exp_coef();
  const PairCoef<T> pc = pair_coef<T>(md);
  const T diag_add = (T)(md->noise + md->eps);
  // Interior tiles -- all 64 x 128 elements are data and none is on the diagonal -- take a straight epilogue: the per-element
  // "inside the data? on the diagonal?" 64-bit compares, selects and exec-mask branches of the general one were a third of the
  // kernel's instructions (it is bound by VALU issue: ~3700 instructions per wave x 4 cycles x 16 waves per SIMD = the 100 us
  // of the N = 8192 build), and all but ~3 % of the tiles of a large matrix are interior.
  const bool interior = PADDED && r0 + GTR <= n1 && c0 + HBO_TILE <= n2 && !(g.symmetric && r0 < c0 + HBO_TILE && c0 < r0 + GTR);
  if (interior) {
    // (a scheduling barrier per row of 8 elements: left alone the scheduler interleaves all 32 exponentials: 232 VGPRs)
#pragma unroll
    for (int a = 0; a < GRA; ++a) {
      __builtin_amdgcn_sched_barrier(0);
      T* orow = out + (r0 + ty + 16 * a) * ldo + c0 + VEC * tx;
#pragma unroll
      for (int qb = 0; qb < 8 / VEC; ++qb) {
        vec_t vv;
#pragma unroll
        for (int e = 0; e < VEC; ++e) vv[e] = gram_value<KID>(acc[a][qb * VEC + e], pc, ec);
        gram_store(orow + 16 * VEC * qb, vv);
      }
    }
    return;
  }
#pragma unroll
  for (int a = 0; a < GRA; ++a) {
    __builtin_amdgcn_sched_barrier(0);
    const int64_t row = r0 + ty + 16 * a;
    if (row >= e1) continue;
#pragma unroll
    for (int qb = 0; qb < 8 / VEC; ++qb) {
      const int64_t col0 = c0 + 16 * VEC * qb + VEC * tx;
      T vals[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const int64_t col = col0 + e;
        T v;
        if (row < n1 && col < n2) {
          v = gram_value<KID>(acc[a][qb * VEC + e], pc, ec);
          if (g.symmetric && row == col) v += diag_add;
        } else {
          v = (g.symmetric && row == col) ? (T)1 : (T)0;   // identity / zero padding
        }
        vals[e] = v;
      }
      if (PADDED) {
        vec_t vv;
#pragma unroll
        for (int e = 0; e < VEC; ++e) vv[e] = vals[e];
        gram_store(out + row * ldo + col0, vv);
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          if (col0 + e < e2) gst(out + row * ldo + col0 + e, vals[e]);
      }
    }
  }
}

// ---- fp32 Gram of a stationary covariance on the matrix cores (round 6) ----------------------------------------------------------
// With 32 or more features the distance loop of gram_kernel -- two VALU instructions per pair and feature -- is what the fp32 Gram
// costs (cfg 3: 64 tanh features, cross Gram 0.58 ms per chunk of 8192 candidates = 0.93 TB/s written).  Here the pair term comes off
// the bf16 matrix cores: u_ij = |a_i|^2 + |b_j|^2 - 2 a_i . b_j, the norms summed in fp32 by the thread that stages the row, and the
// dot product from the EXACT three-way bf16 split of both operands (hbo_split3: six v_mfma_f32_32x32x16_bf16 per product, fp32
// accumulate -- every bit of both fp32 factors, as post3.hip).  128 x 128 tile per workgroup, 4 waves of 2 x 2 MFMA blocks, features
// staged 16 at a time.  Reference: kernel.py:63-123.
//
// Accuracy.  The operands are a = (x - x_c) / lengthscale with x_c one row of x1 per tile (distances do not depend on translation):
// inputs offset far from the origin cost nothing, (x - x_c) is exact for nearby rows.  The rounding of u is then ABSOLUTE,
// |du| <= C eps (|a|^2 + |b|^2) with eps = 2^-24, where the direct form's error is relative to u; and |dk/du| <= kappa k(u) with
// kappa = 1/2 (SE: dk/du = -k/2), 3/2 (Matern-3/2: dk/du = -3/2 sv e^-r = -3/2 k / (1 + r), r = sqrt(3u)) and 5/6 (Matern-5/2:
// dk/du = -5/6 sv (1 + r) e^-r = -5/6 k (1 + r) / (1 + r + r^2/3), r = sqrt(5u)).  So a pair's covariance is off by at most
// kappa k(u) C eps (|a|^2 + |b|^2): small where the pair is far apart (k small) or the tile's rows are short, large for CLOSE pairs of
// LONG rows (small length-scales: |a| ~ sqrt(d) / lengthscale).  With C = 32 (an emulation of this kernel's rounding over uniform and
// tanh data, 32..65 features, length-scales 0.05..2, gives C <= 9; duplicated rows on the device, round 6: C ~ 25) the
// budget of 1e-6 sv -- ten times the direct form's own error, a twentieth of the 2e-5 the fp32 Gram is held to -- holds while
// kappa k(u) (|a|^2 + |b|^2) <= GM_RISK sv.  A tile in which any pair breaks that is marked, and gram_mfma_redo_kernel
// -- launched behind every gram_mfma_kernel -- computes it again in the direct form sum ((x1 - x_c) / l - (x2 - x_c) / l)^2, whose error
// is relative to u.  (That form inside gram_mfma_kernel, as a branch, cost the main path registers: 245 -> 277 us on cfg 3's cross Gram.)
// Well-scaled data stays on the matrix cores (cfg 3's 64 tanh features, length-scale 1, |a|^2 ~ 50: a tile falls back only if it holds a
// pair with k > 0.006 sv, u < ~18 where the typical pair has u ~ 50).  The diagonal of a symmetric Gram gets u = 0 exactly; hbo_gram's
// symmetric Gram (x1 == x2) computes the lower tiles only and stores each pair at (i, j) and (j, i): it equals its transpose exactly.
// The diagonal tiles of the task form store their pairs the same way (tests/test_gpu_gram.py, group E).
typedef __bf16 gm_bf16x8 __attribute__((ext_vector_type(8)));
typedef float gm_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned short gm_u16x8 __attribute__((ext_vector_type(8)));
constexpr int GM_KC = 16;     // features per staged chunk (one MFMA k step): 38 KB of LDS, FOUR workgroups per CU -- with 32 (62 KB, two per CU) the
                              // waves spent half of their 41 000 cycles waiting (SQ_WAIT_ANY / SQ_WAVE_CYCLES, profiles/r06_gram_mfma.md)
constexpr int GM_ROWB = 2 * GM_KC + 16;   // bytes of one LDS row of one plane: the chunk's bf16 + 16 bytes (the b128 fragment reads of a lane group cover all 64 banks once)
constexpr int GM_LPR = GM_KC / 4;         // lanes per row of the staging (one float4 each)
constexpr int GM_RPP = 256 / GM_LPR;      // rows per staging pass
constexpr int GM_NQ = 256 / GM_RPP;       // passes: the tile's 128 rows, then its 128 columns
constexpr int GM_FS = HBO_TILE + 4;       // direct-form fallback: floats per LDS row of one feature of one operand
constexpr float GM_RISK = 1e-6f / (32.f * 5.9604645e-8f);   // kappa k (|a|^2 + |b|^2) / sv above which a pair may break the 1e-6 sv budget
constexpr unsigned GM_REDO = 0x7fc0d1e5u;   // a quiet NaN with a payload of its own: the marker of a tile that takes the direct form
// one tile of gram_mfma_kernel, as its epilogue and its direct-form fallback see it
struct GmTile {
  const float* x1; const float* x2; const float* xc; float* out; const double* inv_ls;
  int64_t n1, n2, ldo, e1, e2, r0, c0;
  int fdim, nrow, ncol;           // nrow / ncol: data rows / columns of the tile
  bool symmetric, mirror, on_diag, interior;
  float sv, diag_add, risk_lim;
};
template <int KID>
__device__ __forceinline__ float gm_cov(float sv, float u) {   // on the fast hardware functions (v_sqrt_f32, v_exp_f32: ~1 ulp each)
  if (KID == HBO_KERNEL_SE) return sv * __builtin_amdgcn_exp2f(u * (-0.5f * 1.44269504088896341f));
  const float r = __builtin_amdgcn_sqrtf((KID == HBO_KERNEL_MATERN32 ? 3.f : 5.f) * u);
  const float e = sv * __builtin_amdgcn_exp2f(r * -1.44269504088896341f);
  return KID == HBO_KERNEL_MATERN32 ? e * (1.f + r) : e * fmaf(r, fmaf(r, 1.f / 3.f, 1.f), 1.f);
}
// u -> the covariance -> out, one block of 16 elements at a time.  u from the expansion (DIRECT = false; returns whether a data pair of the
// tile may break the error budget: the caller then computes the tile again and these stores are overwritten by the same threads) or from
// acc itself (DIRECT = true: the fallback's sums).  Accumulator layout of v_mfma_f32_32x32x16_bf16 with the operands swapped: Gram row =
// lane & 31 of block b, Gram column = (q & 3) + 8 (q >> 2) + 4 (lane >> 5) of block a
template <int KID, bool DIRECT>
__device__ __forceinline__ bool gm_finish(const GmTile& t, const gm_f32x16 (&acc)[2][2], const float (*sN)[128]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1, l32 = lane & 31, lh = lane >> 5;
  float risk = 0.f;   // max of k (|a|^2 + |b|^2) over the data pairs (a running max: per-element flags and validity tests cost the main path registers)
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int rl = wm * 64 + b * 32 + l32;
    const float na = sN[0][rl];
    const int64_t gr = t.r0 + rl;
    float* orow = t.out + gr * t.ldo + t.c0;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      __builtin_amdgcn_sched_barrier(0);   // (one block of 16 elements at a time)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cl = wn * 64 + a * 32 + 8 * j + 4 * lh;
        const float4 nb4 = *reinterpret_cast<const float4*>(&sN[1][cl]);
        const float nbv[4] = {nb4.x, nb4.y, nb4.z, nb4.w};
        float val[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float s = acc[a][b][4 * j + e];
          const bool self = t.on_diag && rl == cl + e;   // a point and itself: exactly sv
          val[e] = gm_cov<KID>(t.sv, self ? 0.f : (DIRECT ? s : fmaxf(na + nbv[e] - 2.f * s, 0.f)));
          if (!DIRECT) risk = fmaxf(risk, self ? 0.f : val[e] * (na + nbv[e]));   // (rows / columns beyond the data: -inf or NaN)
        }
        if (t.interior) {
          V16<float>::type vv; vv[0] = val[0]; vv[1] = val[1]; vv[2] = val[2]; vv[3] = val[3];
          gst(reinterpret_cast<V16<float>::type*>(orow + cl), vv);
          continue;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int64_t gcol = t.c0 + cl + e;
          float v = val[e];
          if (gr < t.n1 && gcol < t.n2) {
            if (t.symmetric && gr == gcol) v += t.diag_add;
          } else {
            v = (t.symmetric && gr == gcol) ? 1.f : 0.f;   // identity / zero padding
          }
          if (t.mirror) {   // (no padding: n1 == n2 == e1 == e2)
            if (gr < t.n1 && gcol <= gr) { gst(orow + cl + e, v); if (gcol != gr) gst(t.out + gcol * t.ldo + gr, v); }
          } else if (t.symmetric && t.on_diag) {   // a diagonal tile of the task form: what lies above the diagonal is the mirror of what lies below it,
            // to the bit, as gram_kernel leaves it (the six products of a pair are summed in another order at (j, i) than at (i, j))
            if (gr < t.e1 && gcol <= gr) { gst(orow + cl + e, v); if (gcol != gr) gst(t.out + gcol * t.ldo + gr, v); }
          } else if (gr < t.e1 && gcol < t.e2) {
            gst(orow + cl + e, v);
          }
        }
      }
    }
  }
  return risk > t.risk_lim;
}
// The direct form for a whole tile: ((x1 - x_c) / l - (x2 - x_c) / l)^2 summed in fp32, the operands [operand][feature][row] in sF.
template <int KID>
__device__ __forceinline__ void gm_direct_tile(const GmTile t, float* sF, const float (*sN)[128]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, l32 = lane & 31, lh = lane >> 5;
  gm_f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[a][b][q] = 0.f;
  for (int d0 = 0; d0 < t.fdim; d0 += GM_KC) {
    __syncthreads();
#pragma nounroll
    for (int i = tid; i < 2 * GM_KC * HBO_TILE; i += 256) {
      const int opq = i / (GM_KC * HBO_TILE), k = (i / HBO_TILE) % GM_KC, rr = i % HBO_TILE, d = d0 + k;
      const int64_t gr = (opq ? t.c0 : t.r0) + rr;
      float sx = 0.f;   // (features beyond fdim and rows beyond the data: zero)
      if (d < t.fdim && gr < (opq ? t.n2 : t.n1)) sx = ((opq ? t.x2 : t.x1)[gr * t.fdim + d] - t.xc[d]) * (float)t.inv_ls[d];
      sF[(opq * GM_KC + k) * GM_FS + rr] = sx;
    }
    __syncthreads();
#pragma nounroll
    for (int k = 0; k < GM_KC; ++k) {
      const float* fr = sF + k * GM_FS;
      const float* fc = sF + (GM_KC + k) * GM_FS;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const float ra = fr[wm * 64 + b * 32 + l32];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float4 cb = *reinterpret_cast<const float4*>(fc + wn * 64 + a * 32 + 8 * j + 4 * lh);
            const float cv[4] = {cb.x, cb.y, cb.z, cb.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float df = ra - cv[e]; acc[a][b][4 * j + e] = fmaf(df, df, acc[a][b][4 * j + e]); }
          }
      }
    }
  }
  gm_finish<KID, true>(t, acc, sN);
}
// the tile of workgroup (blockIdx) of a gram_mfma_kernel launch; false: no tile of data (above the diagonal, beyond the matrix)
template <int KID>
__device__ __forceinline__ bool gm_make_tile(const GramArgs& g, const ModelDev*& md, GmTile& t) {
  const int ti = blockIdx.y;
  const int tj = g.symmetric ? (int)((blockIdx.x + blockIdx.y) % gridDim.x) : (int)blockIdx.x;
  if (g.tasks) {
    const TaskDesc& k = g.tasks[blockIdx.z];
    md += (int64_t)blockIdx.z * g.model_stride;
    if (ti >= k.nblk || tj >= k.nblk) return false;
    t.x1 = t.x2 = static_cast<const float*>(k.F);
    t.out = static_cast<float*>(k.A);
    t.n1 = t.n2 = k.n; t.ldo = k.ld; t.e1 = t.e2 = k.npad;
  } else {
    t.x1 = static_cast<const float*>(g.x1); t.x2 = static_cast<const float*>(g.x2); t.out = static_cast<float*>(g.out);
    t.n1 = g.n1; t.n2 = g.n2; t.ldo = g.ldo; t.e1 = g.padded ? g.n1pad : g.n1; t.e2 = g.padded ? g.n2pad : g.n2;
  }
  // mirror: a symmetric Gram in direct mode (hbo_gram with x2 == NULL, the prior's full covariance): no noise, no padding, both triangles written
  t.mirror = !g.tasks && !g.symmetric && t.x1 == t.x2 && t.n1 == t.n2;
  t.symmetric = g.symmetric;
  t.r0 = (int64_t)ti * HBO_TILE; t.c0 = (int64_t)tj * HBO_TILE;
  if ((g.symmetric || t.mirror) && tj > ti) return false;   // entirely above the diagonal
  if (t.r0 >= t.e1 || t.c0 >= t.e2 || t.n1 <= 0) return false;
  t.fdim = g.fdim;
  t.xc = t.x1 + (t.r0 < t.n1 ? t.r0 : t.n1 - 1) * (int64_t)t.fdim;   // the centre x_c: the tile's first row (its last data row in padding)
  t.inv_ls = md->inv_ls;
  t.nrow = (int)min(t.n1 - t.r0, (int64_t)HBO_TILE); t.ncol = (int)min(t.n2 - t.c0, (int64_t)HBO_TILE);
  t.on_diag = (g.symmetric || t.mirror) && ti == tj;
  return true;
}
// ... and what only its epilogue reads (apart, so that gram_mfma_kernel does not hold it through the products)
template <int KID>
__device__ __forceinline__ void gm_epilogue_fields(const ModelDev* md, GmTile& t) {
  t.interior = t.r0 + HBO_TILE <= t.n1 && t.c0 + HBO_TILE <= t.n2 && !t.on_diag && !t.mirror && (t.ldo & 3) == 0 &&
               (reinterpret_cast<unsigned long long>(t.out) & 15) == 0;
  t.sv = (float)md->sv; t.diag_add = (float)(md->noise + md->eps);
  constexpr float kappa = KID == HBO_KERNEL_SE ? 0.5f : (KID == HBO_KERNEL_MATERN32 ? 1.5f : 5.f / 6.f);
  t.risk_lim = (GM_RISK / kappa) * t.sv;
}
template <int KID>
__global__ __launch_bounds__(256, 3) void gram_mfma_kernel(GramArgs g, const ModelDev* __restrict__ md0) {
  __shared__ __attribute__((aligned(16))) unsigned char sP[2 * 3 * 128 * GM_ROWB];   // [operand][plane][row]
  __shared__ float sN[2][128];
  GmTile t;
  const ModelDev* md = md0;
  if (!gm_make_tile<KID>(g, md, t)) return;
  const float* x1 = t.x1; const float* x2 = t.x2; const float* xc = t.xc; const double* inv_ls = t.inv_ls;
  const int64_t n1 = t.n1, n2 = t.n2, r0 = t.r0, c0 = t.c0;
  const int fdim = t.fdim;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, l32 = lane & 31, lh = lane >> 5;

  // staging: GM_LPR consecutive lanes read the chunk's features of one row (a float4 each), a pass of the 256 threads covers GM_RPP rows;
  // the first half of the passes are the tile's rows (x1), the second half its columns (x2).  Every thread keeps the partial |row|^2 of its
  // pieces; GM_LPR-lane sums at the end.
  const int sc4 = tid % GM_LPR, srow = tid / GM_LPR;
  const bool vec_ok = (fdim & 3) == 0 && ((reinterpret_cast<unsigned long long>(x1) | reinterpret_cast<unsigned long long>(x2)) & 15) == 0;
  auto load4 = [&](const float* xr, int d) -> float4 {
    if (vec_ok && d + 4 <= fdim) return *reinterpret_cast<const float4*>(xr + d);
    return make_float4(d < fdim ? xr[d] : 0.f, d + 1 < fdim ? xr[d + 1] : 0.f, d + 2 < fdim ? xr[d + 2] : 0.f, d + 3 < fdim ? xr[d + 3] : 0.f);
  };
  auto load_chunk = [&](int d0, float4 (&v)[GM_NQ]) {
    const int d = d0 + 4 * sc4;
#pragma unroll
    for (int q = 0; q < GM_NQ; ++q) {
      const int opq = q / (GM_NQ / 2), rr = srow + GM_RPP * (q % (GM_NQ / 2));
      const float* src = opq ? x2 : x1;
      const int64_t nrow = opq ? n2 : n1;
      const int64_t gr = (opq ? c0 : r0) + rr;
      const float* xr = src + (gr < nrow ? gr : (nrow > 0 ? nrow - 1 : 0)) * (int64_t)fdim;   // (clamped: always a valid address)
      v[q] = gr < nrow ? load4(xr, d) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  gm_f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[a][b][q] = 0.f;

  float nrm[GM_NQ];
#pragma unroll
  for (int q = 0; q < GM_NQ; ++q) nrm[q] = 0.f;
  float4 vcur[GM_NQ];
  load_chunk(0, vcur);
  for (int d0 = 0; d0 < fdim; d0 += GM_KC) {
    const int d = d0 + 4 * sc4;
    float isc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) isc[e] = (d + e < fdim) ? (float)inv_ls[d + e] : 0.f;
    const float4 vc = load4(xc, d);   // this thread's features of the centre
    __syncthreads();   // the previous chunk's fragments are read
#pragma unroll
    for (int q = 0; q < GM_NQ; ++q) {
      const float sx[4] = {(vcur[q].x - vc.x) * isc[0], (vcur[q].y - vc.y) * isc[1], (vcur[q].z - vc.z) * isc[2], (vcur[q].w - vc.w) * isc[3]};
      unsigned short ph[4], pm[4], pl[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) { nrm[q] = fmaf(sx[e], sx[e], nrm[q]); hbo_split3(sx[e], ph[e], pm[e], pl[e]); }
      const int opq = q / (GM_NQ / 2), rr = srow + GM_RPP * (q % (GM_NQ / 2));
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const unsigned short* w = p == 0 ? ph : (p == 1 ? pm : pl);
        uint2 pk;
        pk.x = (unsigned)w[0] | ((unsigned)w[1] << 16); pk.y = (unsigned)w[2] | ((unsigned)w[3] << 16);
        *reinterpret_cast<uint2*>(sP + (size_t)((opq * 3 + p) * 128 + rr) * GM_ROWB + 8 * sc4) = pk;
      }
    }
    if (d0 + GM_KC < fdim) load_chunk(d0 + GM_KC, vcur);   // in flight beside this chunk's products
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < GM_KC / 16; ++ks) {
      // the COLUMN block is the MFMA's row operand: a lane then holds 4 consecutive Gram columns of one Gram row (16-byte stores)
      gm_bf16x8 fa[3][2], fb[3][2];
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          fa[p][t] = *reinterpret_cast<const gm_bf16x8*>(sP + (size_t)((1 * 3 + p) * 128 + wn * 64 + t * 32 + l32) * GM_ROWB + ks * 32 + lh * 16);
          fb[p][t] = *reinterpret_cast<const gm_bf16x8*>(sP + (size_t)((0 * 3 + p) * 128 + wm * 64 + t * 32 + l32) * GM_ROWB + ks * 32 + lh * 16);
        }
      constexpr int PA[6] = {2, 0, 1, 1, 0, 0};   // smallest products first: l h', h l', m m', m h', h m', h h'
      constexpr int PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
      for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[PA[q]][a], fb[PB[q]][b], acc[a][b], 0, 0, 0);
    }
  }
#pragma unroll
  for (int q = 0; q < GM_NQ; ++q) {
    float s_ = nrm[q];
#pragma unroll
    for (int o = 1; o < GM_LPR; o *= 2) s_ += __shfl_xor(s_, o);
    const int opq = q / (GM_NQ / 2), rr = srow + GM_RPP * (q % (GM_NQ / 2));
    // rows beyond the data: -inf, out of the risk test of gm_finish (their u clamps to 0; padding is stored instead)
    if (sc4 == 0) sN[opq][rr] = (opq ? c0 : r0) + rr < (opq ? n2 : n1) ? s_ : -INFINITY;
  }
  __syncthreads();

  // a tile with a pair that may break the budget is computed again by gram_mfma_redo_kernel, launched behind this one: its element
  // (r0, c0) -- a data pair whenever the tile has one, stored by thread 0 -- becomes the marker GM_REDO
  gm_epilogue_fields<KID>(md, t);
  if (__syncthreads_or((int)gm_finish<KID, false>(t, acc, sN)) && tid == 0) t.out[t.r0 * t.ldo + t.c0] = __builtin_bit_cast(float, GM_REDO);
}
// The direct form for the tiles gram_mfma_kernel marked (GM_REDO at their element (r0, c0)), on the same grid and stream; every other
// workgroup reads that one element and leaves.  (A NaN input that carries the marker's payload only sends its tile down the exact path.)
template <int KID>
__global__ __launch_bounds__(256) void gram_mfma_redo_kernel(GramArgs g, const ModelDev* __restrict__ md0) {
  __shared__ __attribute__((aligned(16))) float sF[2 * GM_KC * GM_FS];
  __shared__ float sN[2][128];   // (not read by the direct epilogue)
  GmTile t;
  const ModelDev* md = md0;
  if (!gm_make_tile<KID>(g, md, t) || t.nrow <= 0 || t.ncol <= 0) return;
  if (__builtin_bit_cast(unsigned, t.out[t.r0 * t.ldo + t.c0]) != GM_REDO) return;
  gm_epilogue_fields<KID>(md, t);
  gm_direct_tile<KID>(t, sF, sN);
}

template <typename T>
__global__ void kdiag_kernel(const T* __restrict__ f, int64_t n, int fdim, const ModelDev* __restrict__ md,
                             T* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (md->kernel_id == HBO_KERNEL_DOT) {
    T s = 0;
    for (int d = 0; d < fdim; ++d) { const T v = f[i * fdim + d]; s += v * v; }
    out[i] = s * (T)(1.0 / (md->dot_sigma * md->dot_sigma)) + (T)(md->dot_bias * md->dot_bias);
  } else {
    out[i] = (T)md->sv;
  }
}

template <typename T>
void launch_gram_t(const GramArgs& a, const ModelDev* md, dim3 grid, hipStream_t st) {
  if constexpr (sizeof(T) == 4) {
    if (a.mfma_min_f > 0 && a.fdim >= a.mfma_min_f && a.kernel_id != HBO_KERNEL_DOT && !a.direct_form) {
      dispatch_kid(a.kernel_id, [&](auto kid) {   // (never the dot product: an id that is none of the four counts as matern52 here)
        constexpr int K = decltype(kid)::value == HBO_KERNEL_DOT ? (int)HBO_KERNEL_MATERN52 : (int)decltype(kid)::value;
        hipLaunchKernelGGL((gram_mfma_kernel<K>), grid, dim3(256), 0, st, a, md);
        hipLaunchKernelGGL((gram_mfma_redo_kernel<K>), grid, dim3(256), 0, st, a, md);
      });
      return;
    }
  }
  grid.y *= HBO_TILE / GTR;   // callers size the grid in 128x128 tiles; the kernel tiles rows by GTR
  dispatch_kid(a.kernel_id, [&](auto kid) {
    constexpr int K = decltype(kid)::value;
    if (a.padded || a.tasks) hipLaunchKernelGGL((gram_kernel<T, true, K>), grid, dim3(256), 0, st, a, md);
    else hipLaunchKernelGGL((gram_kernel<T, false, K>), grid, dim3(256), 0, st, a, md);
  });
}

}  // namespace

void launch_gram(int dtype, const GramArgs& a, const ModelDev* md, dim3 grid, hipStream_t st) {
  dispatch_dtype(dtype, [&](auto tag) { launch_gram_t<typename decltype(tag)::type>(a, md, grid, st); });
}
void launch_kdiag(int dtype, const void* f, int64_t n, int fdim, const ModelDev* md, void* out, hipStream_t st) {
  if (n <= 0) return;
  dim3 grid((unsigned)((n + 255) / 256));
  dispatch_dtype(dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    hipLaunchKernelGGL((kdiag_kernel<T>), grid, dim3(256), 0, st, (const T*)f, n, fdim, md, (T*)out);
  });
}
