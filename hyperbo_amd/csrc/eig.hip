// Symmetric eigensolver in fp64 (hbo_sym_eig) and the spectral NLL built on it (hbo_nll_spectral): the device form of the
// reference's SVD routines (hyperbo/gp_utils/objectives.py:157-176, hyperbo/basics/linalg.py:113-126, gp.py:198-240).
//
// Two-sided Jacobi.  A matrix of order n is padded to npad = round_up(n, 64) (zeros off the diagonal: padded indices never couple,
// because a rotation with a_pq == 0 is skipped exactly) and cut into npad / 32 blocks of 32.  One sweep pairs the blocks round-robin,
// npad/32 - 1 rounds of npad/64 disjoint pairs; each round
//   (a) jacobi_lds_kernel: one workgroup per pair diagonalises the 64 x 64 sub-matrix [[A_pp, A_pq], [A_qp, A_qq]] in LDS (cyclic
//       round-robin Jacobi, 32 disjoint rotations per step, Rutishauser's formulas), accumulating its rotations in J_k and applying
//       them to the carried column (the NLL's Q^T y), and writes the diagonalised block back;
//   (b) eig_update_kernel: every off-diagonal 64 x 64 tile (k, l) becomes J_k^T A_(k,l) J_l (the lower tiles are computed, each is
//       written with its mirror, so A stays exactly symmetric).  The rotation products are kept as D = J - I and applied as
//       A + A D, V + V D: their rounding scales with the rotations, not with the identity (V stays orthogonal to ~0.4 n eps);
//   (c) eig_vec_kernel (vectors only): V^T[P u Q, :] <- J_k^T V^T[P u Q, :].
// After each sweep off(A) = |A - diag A|_F is formed from per-tile partials summed in one fixed order (no float atomics: identical
// calls are bit-identical), and a problem stops when off(A) <= sqrt(npad) eps |A|_F or when a whole sweep rotated nothing.  Sweeps are capped
// (EIG_MAX_SWEEPS = 40 -- measured: 26 at n = 8192 on an SE Gram matrix -- and EIG_INNER_SWEEPS inside a pair): over the cap is a status (HBO_NOT_CONVERGED), not a hang.  n <= 64 is the
// same code with one pair per matrix: the whole solve is one jacobi_lds_kernel launch per sweep, batched across matrices.
#include "api_internal.h"

#include <numeric>

namespace {
constexpr int EB = 32;               // block of the blocked method
constexpr int EP = 64;               // order of a pair's sub-problem
constexpr int ELD = 65;              // LDS leading dimension of the sub-problem (doubles)
constexpr int EIG_INNER_SWEEPS = 40;
constexpr int EIG_MAX_SWEEPS = 40;
constexpr double EIG_EPS = 2.220446049250313e-16;
constexpr int LDS_KERNEL_BYTES = 2 * EP * ELD * sizeof(double) + EP * sizeof(double);

struct EigBatch {        // T problems of order npad, fp64, row-major, leading dimension npad
  double* A;             // [T][npad][npad]
  double* J;             // [T][npairs][64][64]: D_k = J_k - I, the rotation product of each pair in the current round minus the identity
  double* Vt;            // [T][npad][npad] or null: V^T (row i = eigenvector i)
  double* cvec;          // [T][npad] or null: the carried column
  const double* thr;     // [T]: rotations with |a_pq| <= thr are skipped (eps |A|_F / npad)
  const int* active;     // [T]: 0 = converged or failed, nothing runs for it
  int* rotated;          // [T]: set to 1 by a pair that rotated in this sweep (plain stores)
  int* jrot;             // [T][npairs]: 1 when J_k of this round is not the identity
  const int* nreal;      // [T]: the order n of each problem (indices >= n are padding)
  int npad;
};

// round-robin ordering over B indices (B even): pair k of round r, r in [0, B-1), k in [0, B/2); a < b
__host__ __device__ inline void rr_pair(int r, int k, int B, int& a, int& b) {
  const int M = B - 1;
  if (k == 0) { a = M; b = r; }
  else { a = (r + k) % M; b = (r - k + M) % M; }
  if (a > b) { const int x = a; a = b; b = x; }
}

// (a) one 64 x 64 sub-problem per workgroup (blockIdx.x = pair, blockIdx.y = problem)
__global__ __launch_bounds__(256) void jacobi_lds_kernel(EigBatch b, int round) {
  const int t = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
  if (!b.active[t]) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char eig_smem[];
  double* a = reinterpret_cast<double*>(eig_smem);   // [64][ELD]
  double* j = a + EP * ELD;                           // [64][ELD]: D = J - I (J = the product of this kernel's rotations)
  double* cv = j + EP * ELD;                          // [64]
  __shared__ double rs[32], ru[32], rt[32];
  __shared__ int rp[32], rq[32], rf[32];
  __shared__ int sweep_rot, any_rot, perm[EP], nonid;
  const int npad = b.npad, B = npad / EB;
  int P, Q;
  rr_pair(round, k, B, P, Q);
  double* A = b.A + (size_t)t * npad * npad;
  auto gi = [&](int i) { return i < EB ? P * EB + i : Q * EB + (i - EB); };
  for (int e = tid; e < EP * EP; e += 256) {
    const int r = e / EP, col = e % EP;
    a[r * ELD + col] = A[(size_t)gi(r) * npad + gi(col)];
    j[r * ELD + col] = 0.0;
  }
  if (b.cvec && tid < EP) cv[tid] = b.cvec[(size_t)t * npad + gi(tid)];
  const double thr = b.thr[t];
  if (tid == 0) { sweep_rot = 0; any_rot = 0; }
  __syncthreads();
  for (int sweep = 0; sweep < EIG_INNER_SWEEPS; ++sweep) {
    for (int step = 0; step < EP - 1; ++step) {
      if (tid < 32) {
        int p, q;
        rr_pair(step, tid, EP, p, q);
        const double apq = a[p * ELD + q];
        // exact zeros never rotate (padding stays decoupled); a NaN never rotates either (such a problem was stopped before)
        const int rot = apq != 0.0 && fabs(apq) > thr;
        double s = 0.0, tau = 0.0, tn = 0.0;
        if (rot) {
          const double app = a[p * ELD + p], aqq = a[q * ELD + q];
          const double theta = (aqq - app) / (2.0 * apq);
          // Rutishauser: t = sign(theta) / (|theta| + sqrt(1 + theta^2)); 1/(2 theta) where theta^2 would overflow
          if (fabs(theta) > 1e150) tn = 0.5 / theta;
          else tn = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
          const double c = 1.0 / sqrt(1.0 + tn * tn);
          s = tn * c;
          tau = s / (1.0 + c);   // tan(theta / 2): x' = x - s (y + tau x), y' = y + s (x - tau y) is c x - s y, s x + c y with the
                                 // rounding of the correction, not of x -- the accumulated product stays orthogonal to ~0.2 n eps
          sweep_rot = 1;
        }
        rs[tid] = s; ru[tid] = tau; rt[tid] = tn; rp[tid] = p; rq[tid] = q; rf[tid] = rot;
      }
      __syncthreads();
      // A <- G^T A G, 2 x 2 block (pair i, pair jj) at a time; each lower block is read and written (with its mirror) by one thread
      for (int e = tid; e < 32 * 32; e += 256) {
        const int i = e >> 5, jj = e & 31;
        if (jj > i) continue;
        const int pi = rp[i], qi = rq[i];
        if (i == jj) {
          if (rf[i]) {
            const double apq = a[pi * ELD + qi];
            a[pi * ELD + pi] -= rt[i] * apq;
            a[qi * ELD + qi] += rt[i] * apq;
            a[pi * ELD + qi] = 0.0;
            a[qi * ELD + pi] = 0.0;
          }
          continue;
        }
        if (!rf[i] && !rf[jj]) continue;
        const int pj = rp[jj], qj = rq[jj];
        double b00 = a[pi * ELD + pj], b01 = a[pi * ELD + qj], b10 = a[qi * ELD + pj], b11 = a[qi * ELD + qj];
        if (rf[jj]) {   // right: columns pj, qj
          const double s = rs[jj], u = ru[jj];
          const double n00 = b00 - s * (b01 + u * b00), n01 = b01 + s * (b00 - u * b01);
          const double n10 = b10 - s * (b11 + u * b10), n11 = b11 + s * (b10 - u * b11);
          b00 = n00; b01 = n01; b10 = n10; b11 = n11;
        }
        if (rf[i]) {    // left: rows pi, qi
          const double s = rs[i], u = ru[i];
          const double n00 = b00 - s * (b10 + u * b00), n10 = b10 + s * (b00 - u * b10);
          const double n01 = b01 - s * (b11 + u * b01), n11 = b11 + s * (b01 - u * b11);
          b00 = n00; b01 = n01; b10 = n10; b11 = n11;
        }
        a[pi * ELD + pj] = b00; a[pi * ELD + qj] = b01; a[qi * ELD + pj] = b10; a[qi * ELD + qj] = b11;
        a[pj * ELD + pi] = b00; a[qj * ELD + pi] = b01; a[pj * ELD + qi] = b10; a[qj * ELD + qi] = b11;
      }
      // J <- J G, kept as D = J - I (the corrections are added to D, not to the identity: late, small rotations keep their bits)
      for (int e = tid; e < EP * 32; e += 256) {
        const int r = e >> 5, i = e & 31;
        if (!rf[i]) continue;
        const int p = rp[i], q = rq[i];
        const double s = rs[i], u = ru[i], dp = j[r * ELD + p], dq = j[r * ELD + q];
        const double x = dp + (r == p ? 1.0 : 0.0), y = dq + (r == q ? 1.0 : 0.0);
        j[r * ELD + p] = dp - s * (y + u * x);
        j[r * ELD + q] = dq + s * (x - u * y);
      }
      if (b.cvec && tid < 32 && rf[tid]) {   // carried column <- G^T column
        const int p = rp[tid], q = rq[tid];
        const double s = rs[tid], u = ru[tid], x = cv[p], y = cv[q];
        cv[p] = x - s * (y + u * x);
        cv[q] = y + s * (x - u * y);
      }
      __syncthreads();
    }
    const int rotated = sweep_rot;
    __syncthreads();
    if (!rotated) break;
    if (tid == 0) { sweep_rot = 0; any_rot = 1; }
    __syncthreads();
  }
  // the diagonalised sub-problem leaves with its eigenvalues in descending order, the larger ones in the lower block P (a sweep
  // then gathers large and small eigenvalues in different blocks: 8 instead of 15 sweeps on a 256-point SE Gram matrix).  Padded
  // indices keep their place (the eigenpairs of index >= n are the padding's, whatever the order).  perm[j]: old index at place j.
  if (tid < EP) {
    const int nr = b.nreal[t];
    const int cntP = min(max(nr - P * EB, 0), EB), cntQ = min(max(nr - Q * EB, 0), EB);
    auto real = [&](int i) { return i < EB ? i < cntP : i - EB < cntQ; };
    if (!real(tid)) perm[tid] = tid;
    else {
      const double di = a[tid * ELD + tid];
      int rank = 0;
      for (int q = 0; q < EP; ++q) {
        if (!real(q)) continue;
        const double dq = a[q * ELD + q];
        rank += (dq > di) || (dq == di && q < tid);
      }
      perm[rank < cntP ? rank : EB + (rank - cntP)] = tid;
    }
  }
  if (tid == 0) nonid = 0;
  __syncthreads();
  if (tid < EP && perm[tid] != tid) nonid = 1;
  __syncthreads();
  // A <- P^T A P, J <- J P (as D = J P - I), column <- P^T column
  for (int e = tid; e < EP * EP; e += 256) {
    const int r = e / EP, col = e % EP, pc = perm[col];
    A[(size_t)gi(r) * npad + gi(col)] = a[perm[r] * ELD + pc];
    b.J[((size_t)t * (npad / EP) + k) * EP * EP + e] = j[r * ELD + pc] + ((r == pc ? 1.0 : 0.0) - (r == col ? 1.0 : 0.0));
  }
  if (b.cvec && tid < EP) b.cvec[(size_t)t * npad + gi(tid)] = cv[perm[tid]];
  if (tid == 0) {
    b.jrot[(size_t)t * (npad / EP) + k] = any_rot || nonid;
    if (any_rot) b.rotated[t] = 1;
  }
}

// C = X^T Y for 64 x 64 row-major X, Y in LDS (leading dimension 64); thread (ty, tx) of a 16 x 16 grid holds rows ty + 16 a,
// columns tx + 16 b
__device__ inline void xty_64(const double* X, const double* Y, double acc[4][4]) {
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
#pragma unroll
  for (int aa = 0; aa < 4; ++aa)
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) acc[aa][bb] = 0.0;
  for (int r = 0; r < EP; ++r) {
    double xa[4], yb[4];
#pragma unroll
    for (int aa = 0; aa < 4; ++aa) xa[aa] = X[r * EP + ty + 16 * aa];
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) yb[bb] = Y[r * EP + tx + 16 * bb];
#pragma unroll
    for (int aa = 0; aa < 4; ++aa)
#pragma unroll
      for (int bb = 0; bb < 4; ++bb) acc[aa][bb] = fma(xa[aa], yb[bb], acc[aa][bb]);
  }
}

// (b) tile (k, l), k > l: A_(k,l) <- J_k^T A_(k,l) J_l, written with its mirror (grid: pairs x pairs x problems)
__global__ __launch_bounds__(256) void eig_update_kernel(EigBatch b, int round) {
  const int k = blockIdx.x, l = blockIdx.y, t = blockIdx.z, tid = threadIdx.x;
  if (l >= k || !b.active[t]) return;
  const int npairs = b.npad / EP;
  if (!b.jrot[(size_t)t * npairs + k] && !b.jrot[(size_t)t * npairs + l]) return;
  __shared__ double X[EP * EP], Y[EP * EP];
  const int npad = b.npad, B = npad / EB;
  int Pk, Qk, Pl, Ql;
  rr_pair(round, k, B, Pk, Qk);
  rr_pair(round, l, B, Pl, Ql);
  auto gk = [&](int i) { return i < EB ? Pk * EB + i : Qk * EB + (i - EB); };
  auto gl = [&](int i) { return i < EB ? Pl * EB + i : Ql * EB + (i - EB); };
  double* A = b.A + (size_t)t * npad * npad;
  const double* Jk = b.J + ((size_t)t * npairs + k) * EP * EP;
  const double* Jl = b.J + ((size_t)t * npairs + l) * EP * EP;
  // X[r][i] = A_(k,l)[i][r] = A[gl(r)][gk(i)] (A is exactly symmetric): contiguous reads, contiguous LDS stores
  for (int e = tid; e < EP * EP; e += 256) {
    const int r = e / EP, i = e % EP;
    X[e] = A[(size_t)gl(r) * npad + gk(i)];
    Y[e] = Jl[e];
  }
  __syncthreads();
  // T = A_(k,l) J_l = A_(k,l) + A_(k,l) D_l, then J_k^T T = T + D_k^T T: the products carry only the rotations' part (their
  // rounding scales with |D|, which is small once the sweeps settle), the base is added once
  double acc[4][4];
  xty_64(X, Y, acc);
  const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
  for (int aa = 0; aa < 4; ++aa)
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) acc[aa][bb] += X[(tx + 16 * bb) * EP + ty + 16 * aa];
  __syncthreads();
#pragma unroll
  for (int aa = 0; aa < 4; ++aa)
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) Y[(ty + 16 * aa) * EP + tx + 16 * bb] = acc[aa][bb];
  for (int e = tid; e < EP * EP; e += 256) X[e] = Jk[e];
  __syncthreads();
  xty_64(X, Y, acc);
#pragma unroll
  for (int aa = 0; aa < 4; ++aa)
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) acc[aa][bb] += Y[(ty + 16 * aa) * EP + tx + 16 * bb];
  __syncthreads();
#pragma unroll
  for (int aa = 0; aa < 4; ++aa)
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) X[(ty + 16 * aa) * EP + tx + 16 * bb] = acc[aa][bb];
  __syncthreads();
  for (int e = tid; e < EP * EP; e += 256) {
    const int r = e / EP, col = e % EP;
    A[(size_t)gk(r) * npad + gl(col)] = X[r * EP + col];
    A[(size_t)gl(r) * npad + gk(col)] = X[col * EP + r];
  }
}

// (c) V^T[P u Q, c0 : c0 + 64] <- J_k^T V^T[P u Q, c0 : c0 + 64] = V^T[..] + D_k^T V^T[..] (grid: column chunks x pairs x problems)
__global__ __launch_bounds__(256) void eig_vec_kernel(EigBatch b, int round) {
  const int cb = blockIdx.x, k = blockIdx.y, t = blockIdx.z, tid = threadIdx.x;
  const int npad = b.npad, npairs = npad / EP, B = npad / EB;
  if (!b.active[t] || !b.jrot[(size_t)t * npairs + k]) return;
  __shared__ double X[EP * EP], Y[EP * EP];
  int P, Q;
  rr_pair(round, k, B, P, Q);
  auto gk = [&](int i) { return i < EB ? P * EB + i : Q * EB + (i - EB); };
  double* Vt = b.Vt + (size_t)t * npad * npad;
  const double* Jk = b.J + ((size_t)t * npairs + k) * EP * EP;
  const int c0 = cb * EP;
  for (int e = tid; e < EP * EP; e += 256) {
    const int r = e / EP, col = e % EP;
    X[e] = Jk[e];
    Y[e] = Vt[(size_t)gk(r) * npad + c0 + col];
  }
  __syncthreads();
  double acc[4][4];
  xty_64(X, Y, acc);
  const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
  for (int aa = 0; aa < 4; ++aa)
#pragma unroll
    for (int bb = 0; bb < 4; ++bb)
      Vt[(size_t)gk(ty + 16 * aa) * npad + c0 + tx + 16 * bb] = Y[(ty + 16 * aa) * EP + tx + 16 * bb] + acc[aa][bb];
}

// per 64 x 64 tile: [sum of squared diagonal entries, sum of squared off-diagonal entries], fixed-order reduction
__global__ __launch_bounds__(256) void eig_norm_partials_kernel(const double* __restrict__ A, int npad, const int* __restrict__ active,
                                                                double* __restrict__ part) {
  const int ti = blockIdx.y, tj = blockIdx.x, t = blockIdx.z, tid = threadIdx.x;
  const int nt = npad / EP;
  if (active && !active[t]) return;
  const double* At = A + (size_t)t * npad * npad;
  double d = 0.0, o = 0.0;
  for (int e = tid; e < EP * EP; e += 256) {
    const int r = ti * EP + e / EP, col = tj * EP + e % EP;
    const double v = At[(size_t)r * npad + col];
    if (r == col) d = fma(v, v, d); else o = fma(v, v, o);
  }
  __shared__ double sd[256], so[256];
  sd[tid] = d; so[tid] = o;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) { sd[tid] += sd[tid + s]; so[tid] += so[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    double* p = part + ((size_t)t * nt * nt + (size_t)ti * nt + tj) * 2;
    p[0] = sd[0]; p[1] = so[0];
  }
}

// one workgroup of 64 per problem: the ordered sum of the partials -> off(A), |A|_F; `init`: the first call also sets the rotation
// threshold and marks non-finite problems failed.  active = not failed && off > sqrt(npad) eps |A|_F && (init || something rotated).
// (The rotations skip entries below eps |A|_F / npad, so off(A) settles at the rounding floor of order eps |A|_F -- a stop AT eps |A|_F
// would sit on that floor; sqrt(npad) eps |A|_F is still within n eps |A|_2, the backward error the callers are promised.)
__global__ __launch_bounds__(64) void eig_norm_finish_kernel(const double* __restrict__ part, int npad, int init, int* active,
                                                             int* failed, const int* __restrict__ rotated, double* thr, double* nrm0) {
  const int t = blockIdx.x, tid = threadIdx.x;
  if (!init && !active[t]) return;
  const int nt = npad / EP, cnt = nt * nt;
  const double* p = part + (size_t)t * cnt * 2;
  __shared__ double sd[64], so[64];
  double d = 0.0, o = 0.0;
  const int per = (cnt + 63) / 64;
  for (int i = tid * per; i < min(cnt, (tid + 1) * per); ++i) { d += p[2 * i]; o += p[2 * i + 1]; }
  sd[tid] = d; so[tid] = o;
  __syncthreads();
  if (tid) return;
  d = 0.0; o = 0.0;
  for (int i = 0; i < 64; ++i) { d += sd[i]; o += so[i]; }
  const double tot = d + o;
  if (init) {
    const double n = sqrt(tot);
    nrm0[t] = n;
    thr[t] = EIG_EPS * n / npad;
    failed[t] = !(tot <= 1.7e308);   // NaN / inf anywhere
    active[t] = !failed[t] && sqrt(o) > EIG_EPS * sqrt((double)npad) * n;
  } else {
    if (!(tot <= 1.7e308)) { failed[t] = 1; active[t] = 0; return; }
    active[t] = rotated[t] && sqrt(o) > EIG_EPS * sqrt((double)npad) * nrm0[t];
  }
}

__global__ void eig_diag_kernel(const double* __restrict__ A, int npad, int T, double* __restrict__ w) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)T * npad) return;
  const int64_t t = e / npad, i = e % npad;
  w[e] = A[(size_t)t * npad * npad + (size_t)i * npad + i];
}

__global__ void eig_identity_kernel(double* __restrict__ V, int npad, int T) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per = (int64_t)npad * npad;
  if (e >= (int64_t)T * per) return;
  const int64_t r = (e % per) / npad, col = e % npad;
  V[e] = r == col ? 1.0 : 0.0;
}

// the spectral NLL's matrix: G (model dtype, n x n) + (noise + eps) on the diagonal in the model dtype -- what
// compute_delta_y_and_cov does on the host before np.asarray(cov, float64) -- promoted into the padded fp64 A; and the carried column
// y~ = sum over the m columns of (y - mu)
template <typename T>
__global__ void spectral_fill_kernel(const T* __restrict__ G, int64_t n, int npad, double diag_add, double* __restrict__ A) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)npad * npad) return;
  const int64_t r = e / npad, col = e % npad;
  double v = 0.0;
  if (r < n && col < n) {
    T g = G[r * n + col];
    if (r == col) g = g + (T)diag_add;
    v = (double)g;
  }
  A[e] = v;
}
template <typename T>
__global__ void spectral_rhs_kernel(const T* __restrict__ ysum, const T* __restrict__ mu, int64_t n, int npad, int m, double* __restrict__ cv) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npad) return;
  double v = 0.0;
  if (i < n) v = m == 1 ? (double)(T)(ysum[i] - mu[i]) : (double)ysum[i] - (double)m * (double)mu[i];
  cv[i] = v;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }
}  // namespace

// Runs the blocked Jacobi on T problems of order npad in d_A (fp64, exactly symmetric, padded), with V^T in d_Vt (nullable, set to
// the identity here) and the carried column in d_c (nullable).  failed[t]: 1 when problem t held a NaN / inf or hit the sweep cap.
int eig_run(hbo_ctx* c, int T, int npad, const int* h_nreal, double* d_A, double* d_Vt, double* d_c, std::vector<int>& failed, int* sweeps_out) {
  hipStream_t st = c->stream;
  const int npairs = npad / EP, nt = npad / EP, B = npad / EB;
  DevBuf buf;
  double *d_J = nullptr, *d_part = nullptr, *d_thr = nullptr, *d_nrm = nullptr;
  int* d_flags = nullptr;   // [active T][failed T][rotated T]
  int* d_jrot = nullptr;
  int* d_nreal = nullptr;
  HIPCHK(c, buf.get(c, &d_nreal, sizeof(int) * T));
  HIPCHK(c, hipMemcpyAsync(d_nreal, h_nreal, sizeof(int) * T, hipMemcpyHostToDevice, st));
  HIPCHK(c, buf.get(c, &d_J, sizeof(double) * T * npairs * EP * EP));
  HIPCHK(c, buf.get(c, &d_part, sizeof(double) * 2 * T * nt * nt));
  HIPCHK(c, buf.get(c, &d_thr, sizeof(double) * T));
  HIPCHK(c, buf.get(c, &d_nrm, sizeof(double) * T));
  HIPCHK(c, buf.get(c, &d_flags, sizeof(int) * 3 * T));
  HIPCHK(c, buf.get(c, &d_jrot, sizeof(int) * T * npairs));
  int* d_active = d_flags; int* d_failed = d_flags + T; int* d_rot = d_flags + 2 * T;
  HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&jacobi_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_KERNEL_BYTES));
  if (d_Vt) hipLaunchKernelGGL(eig_identity_kernel, dim3(blocks_of((int64_t)T * npad * npad)), dim3(256), 0, st, d_Vt, npad, T);
  HIPCHK(c, hipMemsetAsync(d_flags, 0, sizeof(int) * 3 * T, st));
  hipLaunchKernelGGL(eig_norm_partials_kernel, dim3(nt, nt, T), dim3(256), 0, st, d_A, npad, nullptr, d_part);
  hipLaunchKernelGGL(eig_norm_finish_kernel, dim3(T), dim3(64), 0, st, d_part, npad, 1, d_active, d_failed, d_rot, d_thr, d_nrm);
  EigBatch eb{d_A, d_J, d_Vt, d_c, d_thr, d_active, d_rot, d_jrot, d_nreal, npad};
  std::vector<int> h_flags(3 * T);
  int sweeps = 0;
  for (;;) {
    HIPCHK(c, hipMemcpyAsync(h_flags.data(), d_flags, sizeof(int) * 3 * T, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    bool any = false;
    for (int t = 0; t < T; ++t) any = any || h_flags[t];
    if (!any || sweeps == EIG_MAX_SWEEPS) break;
    ++sweeps;
    HIPCHK(c, hipMemsetAsync(d_rot, 0, sizeof(int) * T, st));
    for (int r = 0; r < B - 1; ++r) {
      hipLaunchKernelGGL(jacobi_lds_kernel, dim3(npairs, T), dim3(256), LDS_KERNEL_BYTES, st, eb, r);
      if (npairs > 1) hipLaunchKernelGGL(eig_update_kernel, dim3(npairs, npairs, T), dim3(256), 0, st, eb, r);
      if (d_Vt) hipLaunchKernelGGL(eig_vec_kernel, dim3(npad / EP, npairs, T), dim3(256), 0, st, eb, r);
    }
    hipLaunchKernelGGL(eig_norm_partials_kernel, dim3(nt, nt, T), dim3(256), 0, st, d_A, npad, d_active, d_part);
    hipLaunchKernelGGL(eig_norm_finish_kernel, dim3(T), dim3(64), 0, st, d_part, npad, 0, d_active, d_failed, d_rot, d_thr, d_nrm);
  }
  failed.assign(T, 0);
  for (int t = 0; t < T; ++t) failed[t] = h_flags[T + t] || h_flags[t];   // failed, or still active at the cap
  if (sweeps_out) *sweeps_out = sweeps;
  return HBO_OK;
}

static int64_t eig_npad(int64_t n) { return round_up(n, EP); }

extern "C" int hbo_sym_eig(hbo_ctx* c, int dtype, const void* a, int64_t n, int32_t count, double* w_out, double* v_out) {
  if (!c || !a || !w_out) return fail(c, HBO_ERR_ARG, "hbo_sym_eig: null argument");
  if (n <= 0 || count <= 0) return fail(c, HBO_ERR_ARG, "hbo_sym_eig: n and count must be positive");
  if (dtype != HBO_F32 && dtype != HBO_F64) return fail(c, HBO_ERR_ARG, "hbo_sym_eig: bad dtype");
  if (n > (int64_t)1 << 16) return fail(c, HBO_ERR_ARG, "hbo_sym_eig: n too large");
  HIPCHK(c, hipSetDevice(c->device));
  const int npad = (int)eig_npad(n);
  const size_t per = (size_t)npad * npad;
  // problems per batch: at most ~4 GB of A (+ V^T) on the device
  const int64_t chunk = std::min<int64_t>(16384, std::max<int64_t>(1, ((int64_t)1 << 29) / (int64_t)(per * (v_out ? 2 : 1))));
  c->eig_last_sweeps = 0;
  bool bad_any = false;
  for (int32_t t0 = 0; t0 < count; t0 += (int32_t)chunk) {
    const int T = (int)std::min<int64_t>(chunk, count - t0);
    // host: the lower triangle, promoted to fp64, symmetrised, padded, and scaled by a power of two so that max |a| is in [0.5, 1)
    // (exact; the rotations and the norms then neither overflow nor underflow for any finite input)
    std::vector<double> h((size_t)T * per, 0.0);
    std::vector<int> scale_exp(T, 0);
    for (int t = 0; t < T; ++t) {
      const int64_t base = (int64_t)(t0 + t) * n * n;
      double mx = 0.0;
      for (int64_t i = 0; i < n; ++i)
        for (int64_t jj = 0; jj <= i; ++jj) { const double v = fabs(host_elem(a, dtype, base + i * n + jj)); if (v > mx) mx = v; }
      int ex = 0;
      if (mx > 0 && mx <= 1.7976931348623157e308) frexp(mx, &ex);
      scale_exp[t] = ex;
      double* ht = h.data() + (size_t)t * per;
      for (int64_t i = 0; i < n; ++i)
        for (int64_t jj = 0; jj <= i; ++jj) {
          const double v = ldexp(host_elem(a, dtype, base + i * n + jj), -ex);
          ht[(size_t)i * npad + jj] = v;
          ht[(size_t)jj * npad + i] = v;
        }
    }
    DevBuf buf;
    double *d_A = nullptr, *d_Vt = nullptr, *d_w = nullptr;
    HIPCHK(c, buf.get(c, &d_A, sizeof(double) * T * per));
    HIPCHK(c, buf.get(c, &d_w, sizeof(double) * T * npad));
    if (v_out) HIPCHK(c, buf.get(c, &d_Vt, sizeof(double) * T * per));
    HIPCHK(c, hipMemcpyAsync(d_A, h.data(), sizeof(double) * T * per, hipMemcpyHostToDevice, c->stream));
    std::vector<int> failed;
    int sweeps = 0;
    std::vector<int> nreal(T, (int)n);
    int rc = eig_run(c, T, npad, nreal.data(), d_A, d_Vt, nullptr, failed, &sweeps);
    if (rc) return rc;
    c->eig_last_sweeps = std::max(c->eig_last_sweeps, sweeps);
    hipLaunchKernelGGL(eig_diag_kernel, dim3(blocks_of((int64_t)T * npad)), dim3(256), 0, c->stream, d_A, npad, T, d_w);
    std::vector<double> hw((size_t)T * npad);
    HIPCHK(c, hipMemcpyAsync(hw.data(), d_w, sizeof(double) * T * npad, hipMemcpyDeviceToHost, c->stream));
    if (v_out) HIPCHK(c, hipMemcpyAsync(h.data(), d_Vt, sizeof(double) * T * per, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    for (int t = 0; t < T; ++t) {
      double* wt = w_out + (size_t)(t0 + t) * n;
      double* vt = v_out ? v_out + (size_t)(t0 + t) * n * n : nullptr;
      if (failed[t]) {
        bad_any = true;
        for (int64_t i = 0; i < n; ++i) wt[i] = NAN;
        if (vt) for (int64_t i = 0; i < n * n; ++i) vt[i] = NAN;
        continue;
      }
      // ascending (numpy.linalg.eigh); ties keep the index order
      std::vector<int> idx(n);
      std::iota(idx.begin(), idx.end(), 0);
      const double* d = hw.data() + (size_t)t * npad;
      std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return d[x] < d[y]; });
      for (int64_t jj = 0; jj < n; ++jj) wt[jj] = ldexp(d[idx[jj]], scale_exp[t]);
      if (vt) {
        const double* V = h.data() + (size_t)t * per;
        for (int64_t jj = 0; jj < n; ++jj) {
          const double* row = V + (size_t)idx[jj] * npad;   // eigenvector idx[jj] is row idx[jj] of V^T
          for (int64_t r = 0; r < n; ++r) vt[(size_t)r * n + jj] = row[r];
        }
      }
    }
  }
  return bad_any ? HBO_NOT_CONVERGED : HBO_OK;
}

extern "C" int hbo_nll_spectral(hbo_ctx* c, const hbo_model* m, hbo_dataset* ds, double* nll_sum, double* nll_per_task,
                                double* abs_eig_min_per_task) {
  if (!c || !m || !ds || !nll_sum) return fail(c, HBO_ERR_ARG, "hbo_nll_spectral: null argument");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = validate_model(c, m);
  if (rc) return rc;
  *nll_sum = 0;
  const int T = ds->ntasks;
  if (T == 0) return HBO_OK;
  if (m->dtype != ds->dtype || m->input_dim != ds->D) return fail(c, HBO_ERR_ARG, "hbo_nll_spectral: model/dataset dtype or input_dim mismatch");
  rc = upload_model(c, m);
  if (rc) return rc;
  const int dtype = m->dtype;
  const size_t es = esize(dtype);
  hipStream_t st = c->stream;
  const int fdim = feature_dim(m);
  const double diag_add = m->noise_variance + m->eps;
  int64_t max_n = 0;
  for (TaskHost* t : ds->tasks) max_n = std::max(max_n, t->n);
  DevBuf scratch;
  void *d_G = nullptr, *d_mu = nullptr, *d_w = nullptr;
  HIPCHK(c, scratch.get(c, &d_G, (size_t)max_n * max_n * es));
  HIPCHK(c, scratch.get(c, &d_mu, (size_t)max_n * es));
  if (is_kumar(m)) HIPCHK(c, scratch.get(c, &d_w, (size_t)max_n * m->input_dim * es));
  FeatBuf feat;
  if (needs_mlp(m)) { rc = feat.ensure(c, m, max_n); if (rc) return rc; }
  std::vector<double> vals(T, 0.0), mins(T, 0.0);
  bool bad_any = false;
  c->eig_last_sweeps = 0;
  // tasks are held largest first: those of one padded order are consecutive, one batch each
  for (int g0 = 0; g0 < T;) {
    const int npad = (int)eig_npad(ds->tasks[g0]->n);
    int g1 = g0;
    while (g1 < T && eig_npad(ds->tasks[g1]->n) == npad) ++g1;
    const size_t per = (size_t)npad * npad;
    const int64_t chunk = std::min<int64_t>(16384, std::max<int64_t>(1, ((int64_t)1 << 29) / (int64_t)per));
    for (int b0 = g0; b0 < g1; b0 += (int)chunk) {
      const int Tb = (int)std::min<int64_t>(chunk, g1 - b0);
      DevBuf buf;
      double *d_A = nullptr, *d_c = nullptr, *d_diag = nullptr;
      HIPCHK(c, buf.get(c, &d_A, sizeof(double) * Tb * per));
      HIPCHK(c, buf.get(c, &d_c, sizeof(double) * Tb * npad));
      HIPCHK(c, buf.get(c, &d_diag, sizeof(double) * Tb * npad));
      for (int q = 0; q < Tb; ++q) {
        TaskHost* t = ds->tasks[b0 + q];
        const int64_t n = t->n;
        // covariance features exactly as hbo_gram builds them (cov_func of the host path), mean exactly as hbo_mean
        const void* F = t->X;
        const void* Fm = m->mean_id == HBO_MEAN_LINEAR ? t->X : nullptr;
        if (needs_mlp(m)) {
          run_mlp(c, m, t->X, n, feat.acts.data());
          if (m->kernel_uses_mlp) F = feat.acts[m->n_layers - 1];
          if (m->mean_id == HBO_MEAN_LINEAR_MLP) Fm = feat.acts[m->n_layers - 1];
        }
        if (is_kumar(m)) {
          launch_kumar_forward(dtype, nullptr, 0, 0, t->X, d_w, nullptr, n, m->input_dim, c->d_model, st);
          F = d_w;
        }
        GramArgs ga = {}; ga.kernel_id = c->h_model->kernel_id; ga.mfma_min_f = c->opt_gram_mfma; ga.x1 = F; ga.x2 = F; ga.out = d_G;
        ga.n1 = n; ga.n2 = n; ga.ldo = n; ga.fdim = fdim;
        launch_gram(dtype, ga, c->d_model, dim3((unsigned)((n + 127) / 128), (unsigned)((n + 127) / 128), 1), st);
        launch_mean(dtype, Fm, n, mean_feature_dim(m), c->d_model, d_mu, st);
        double* A = d_A + (size_t)q * per;
        double* cv = d_c + (size_t)q * npad;
        if (dtype == HBO_F64) {
          hipLaunchKernelGGL(spectral_fill_kernel<double>, dim3(blocks_of((int64_t)per)), dim3(256), 0, st, (const double*)d_G, n, npad, diag_add, A);
          hipLaunchKernelGGL(spectral_rhs_kernel<double>, dim3(blocks_of(npad)), dim3(256), 0, st, (const double*)t->ysum, (const double*)d_mu, n, npad, t->m, cv);
        } else {
          hipLaunchKernelGGL(spectral_fill_kernel<float>, dim3(blocks_of((int64_t)per)), dim3(256), 0, st, (const float*)d_G, n, npad, diag_add, A);
          hipLaunchKernelGGL(spectral_rhs_kernel<float>, dim3(blocks_of(npad)), dim3(256), 0, st, (const float*)t->ysum, (const float*)d_mu, n, npad, t->m, cv);
        }
      }
      std::vector<int> failed;
      int sweeps = 0;
      std::vector<int> nreal(Tb);
      for (int q = 0; q < Tb; ++q) nreal[q] = (int)ds->tasks[b0 + q]->n;
      rc = eig_run(c, Tb, npad, nreal.data(), d_A, nullptr, d_c, failed, &sweeps);
      if (rc) return rc;
      c->eig_last_sweeps = std::max(c->eig_last_sweeps, sweeps);
      hipLaunchKernelGGL(eig_diag_kernel, dim3(blocks_of((int64_t)Tb * npad)), dim3(256), 0, st, d_A, npad, Tb, d_diag);
      std::vector<double> hw((size_t)Tb * npad), hc((size_t)Tb * npad);
      HIPCHK(c, hipMemcpyAsync(hw.data(), d_diag, sizeof(double) * Tb * npad, hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipMemcpyAsync(hc.data(), d_c, sizeof(double) * Tb * npad, hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipStreamSynchronize(st));
      HIPCHK(c, hipGetLastError());
      for (int q = 0; q < Tb; ++q) {
        TaskHost* t = ds->tasks[b0 + q];
        const int64_t n = t->n;
        if (failed[q]) { bad_any = true; vals[b0 + q] = NAN; mins[b0 + q] = NAN; continue; }
        // K = Q diag(w) Q^T: y~^T K^-1 y~ = sum (Q^T y~)_i^2 / w_i (the sign kept, as the SVD's V diag(1/s) U^T), sum log s = sum log |w_i|
        const double* w = hw.data() + (size_t)q * npad;
        const double* z = hc.data() + (size_t)q * npad;
        double quad = 0.0, logdet = 0.0, mn = INFINITY;
        for (int64_t i = 0; i < n; ++i) {
          quad += z[i] * z[i] / w[i];
          logdet += log(fabs(w[i]));
          mn = std::min(mn, fabs(w[i]));
        }
        const double mm = (double)t->m;
        vals[b0 + q] = 0.5 * (quad + mm * mm * (logdet + (double)n * log(2.0 * M_PI)));
        mins[b0 + q] = mn;
      }
    }
    g0 = g1;
  }
  double s = 0.0;
  for (int k = 0; k < T; ++k) s += vals[k];
  *nll_sum = s;
  if (nll_per_task) for (int k = 0; k < T; ++k) nll_per_task[k] = vals[k];
  if (abs_eig_min_per_task) for (int k = 0; k < T; ++k) abs_eig_min_per_task[k] = mins[k];
  return bad_any ? HBO_NOT_CONVERGED : HBO_OK;
}
