"""CPU side of the inverse tier: L, W = L^-1 and K^-1 = W^T W per 128-tile across the routes of the inverse (hyperbo_amd/csrc/sched.hip:
sweep_advance, trtri_advance beside the chain, run_trtri + run_lauum), through the test hook hbo_probe_factor_inverse
(include/hbo_tune.h).  Shared by tests/test_inverse_cases_host.py (this file judged on its own, on the CPU) and
tests/test_gpu_inverse.py (the device against it).

  exact_case(n, seed, m)   the EXACT family: A = L L^T with a unit-diagonal integer L whose inverse is a small integer matrix (the design
                           of split_oracle.exact_spd, denser: see dense_spd), right-hand sides b, and everything the hook returns as int64.
                           Every product and partial sum of the factorisation, the inverse and K^-1 is an integer far below 2^24: the
                           result is the same bits in fp64 and fp32, in any summation order, tile size, stream layout or group size
  zero_triples(case, tile) the block products the algorithms must perform that would contribute nothing on this case (must be none)
  fit_report(case)         what the products read and reach: significant bits, magnitudes, the sweep's running matrix for every group size
  not_pd_case(case, row)   the same matrix with one diagonal entry lowered so that the pivot of that row is negative
  compare_tiles(got, want) per 128-tile the count of unequal entries (NaN counts as unequal)
  real_case(n)             the REAL-VALUED family: K = Gram(SE, lengthscale 0.3, d = 3) + 1e-2 I in fp64, the reference L, W, W^T W in
                           np.longdouble (plain unblocked loops: LAPACK has no longdouble), the yardstick from scipy.linalg in float64
  tile_errors / bound      per 128-tile max |got - ref| / max |ref|, and REL_FACTOR x (yardstick's worst tile) + FLOOR_C eps n
"""
import functools

import numpy as np
import scipy.linalg

import split_oracle as so

TILE = 128
_mm = so._mm

# ---- shapes of the GPU tier ------------------------------------------------------------------------------------------------------------
SINGLES = (129, 300, 515, 897, 1025, 1290)
BATCHES = {
    'B1': (700, 130, 1, 515, 1290, 1153),   # ragged: tasks shorter than a row group, a group cut by a task's end, a one-point task
    'B2': (1025, 897),
    'B3': (260, 520, 300, 385, 513, 450, 511, 384, 299),   # more than 8 tasks: batch_bg auto takes plain grids
}
M_RHS = 3                                    # right-hand sides per task


def task_seed(k):
  """seed of task k of a batch: every task its own matrix, so that a tile taken from the neighbouring task is a wrong integer"""
  return 10 + k


def all_task_keys():
  """every (n, seed) the GPU tier factorises"""
  keys = {(n, 0) for n in SINGLES}
  for ns in BATCHES.values():
    keys |= {(n, task_seed(k)) for k, n in enumerate(ns)}
  return sorted(keys)


# ---- the exact family ------------------------------------------------------------------------------------------------------------------
PER_BLOCK = 2        # columns a row picks in every 128-column block to its left (its own block included)
SHORT_BLOCK = 16     # rows of a ragged last block shorter than this ...
PER_BLOCK_SHORT = 24   # ... pick this many: few rows have to make every product with that block non-zero


def dense_spd(n, seed=0):
  """split_oracle.exact_spd's design (classes 0..3, L[i, j] != 0 only where class(j) < class(i): N = L - I has no path longer than three,
  N^4 = 0, W = I - N + N^2 - N^3), made dense enough that every block product of the factorisation, the inverse and K^-1 contributes: the
  last row gets class 3, every row picks PER_BLOCK columns in EVERY 128-column block to its left, and the rows of a ragged last block of
  fewer than SHORT_BLOCK rows (on the 128-grid, or on the 64-grid that the small shapes use) pick PER_BLOCK_SHORT.  -> (A, L, W) as int64 arrays."""
  rng = np.random.default_rng(seed)
  cls = rng.integers(0, 4, size=n)
  cls[n - 1] = 3
  # first row of a ragged last block of fewer than SHORT_BLOCK rows, on the 128-grid or on the 64-grid of the small shapes (n: none)
  short_from = n
  for tile in (TILE, TILE // 2):
    start = (n - 1) // tile * tile
    if n - start < SHORT_BLOCK:
      short_from = min(short_from, start)
  N = np.zeros((n, n), np.int64)
  for i in range(1, n):
    per = PER_BLOCK_SHORT if i >= short_from else PER_BLOCK
    for c in range(i // TILE + 1):
      lo, hi = c * TILE, min((c + 1) * TILE, i)
      cand = lo + np.nonzero(cls[lo:hi] < cls[i])[0]
      if cand.size:
        pick = rng.choice(cand, size=min(per, cand.size), replace=False)
        N[i, pick] = rng.choice([-1, 1], size=pick.size)
  L = N + np.eye(n, dtype=np.int64)
  N2 = _mm(N, N)
  W = np.eye(n, dtype=np.int64) - N + N2 - _mm(N2, N)
  return _mm(L, L.T), L, W


@functools.lru_cache(maxsize=None)
def exact_case(n, seed=0, m=M_RHS):
  """One exact input of the hook and everything it returns, as int64 (cached: the arrays are shared, do not write to them)."""
  A, L, W = dense_spd(n, seed)
  rng = np.random.default_rng(seed + 1000 + m)
  b = rng.integers(-3, 4, size=(n, m))
  z = _mm(W, b)
  case = dict(n=n, seed=seed, A=A, L=L, W=W, Kinv=_mm(W.T, W), b=b, z=z, x=_mm(W.T, z))
  for v in case.values():
    if isinstance(v, np.ndarray):
      v.setflags(write=False)
  return case


def _blocks(n, tile):
  return [(o, min(o + tile, n)) for o in range(0, n, tile)]


def zero_triples(case, tile=TILE):
  """The block products that contribute nothing on this case, over the `tile` grid (ragged last block included), as (kind, i, j, k):
    'LLt'  L_ik L_jk^T  for k < j <= i    the factorisation's trailing updates
    'LW'   L_ik W_kj    for j <= k < i    the inverse (block-recursive: S21 = L21 W11; sweep: its running matrix)
    'WtW'  W_ki^T W_kj  for k >= i >= j   K^-1 = W^T W
  A schedule that skips such a product cannot be seen on the case."""
  L, W = case['L'], case['W']
  bl = _blocks(case['n'], tile)
  nb = len(bl)
  Lb = [[L[r0:r1, c0:c1].astype(np.float64) for (c0, c1) in bl] for (r0, r1) in bl]
  Wb = [[W[r0:r1, c0:c1].astype(np.float64) for (c0, c1) in bl] for (r0, r1) in bl]
  out = []
  for i in range(nb):
    for j in range(i + 1):
      for k in range(j):
        if not (Lb[i][k] @ Lb[j][k].T).any(): out.append(('LLt', i, j, k))
      for k in range(j, i):
        if not (Lb[i][k] @ Wb[k][j]).any(): out.append(('LW', i, j, k))
      for k in range(i, nb):
        if not (Wb[k][i].T @ Wb[k][j]).any(): out.append(('WtW', i, j, k))
  return out


def count_triples(n, tile=TILE):
  nb = len(_blocks(n, tile))
  return sum(j + (i - j) + (nb - i) for i in range(nb) for j in range(i + 1))


SWEEP_QS = (1, 2, 4, 8)


def fit_report(case):
  """split_oracle.spd_operand_report (significant bits of L, W and every level's S21; of z; the largest magnitude any partial sum of any
  product can reach, as sums of |.| |.|; the largest output) and the sweep's operands: for every row-group size qs the running matrix
  T[R, <R] = sum over the finished groups g' of L[R, g'] W[g', <R], every partial sum of it -- what (b) W[R, <R] = -W[R, R] T[R, <R]
  reads (sched.hip: sweep_advance).  sweep_bits / sweep_max over all qs, groups and partial sums.  The reach of (b), (c) and (d) is
  inside `reach`: |W| |L| |W| bounds every partial sum of W[R, R] T, |L| |W| of T, |W|^T |W| of K^-1."""
  r = so.spd_operand_report(case)
  L, W, n = case['L'], case['W'], case['n']
  nblk = so.npad_of(n) // TILE
  sweep_bits, sweep_max = 0, 0
  for qs in SWEEP_QS:
    groups = [(g * TILE, min((g + qs) * TILE, n)) for g in range(0, nblk, qs)]
    for gi, (r0, r1) in enumerate(groups):
      T = np.zeros((r1 - r0, r0), np.int64)
      for (c0, c1) in groups[:gi]:
        T[:, :c1] += _mm(L[r0:r1, c0:c1], W[c0:c1, :c1])
        sweep_bits = max(sweep_bits, so.sig_bits(T)); sweep_max = max(sweep_max, int(np.abs(T).max(initial=0)))
      if gi:   # complete: T = L21 W11, and (b) gives the rows of W
        assert np.array_equal(-_mm(W[r0:r1, r0:r1], T), W[r0:r1, :r0])
  r['reach'] = max(r['reach'], int(_mm(np.abs(L), np.abs(W)).max()))
  r.update(sweep_bits=sweep_bits, sweep_max=sweep_max, a_diag_max=int(case['A'].diagonal().max()))
  return r


def not_pd_case(case, row):
  """(A', row): A with A[row, row] lowered by 2.  The rows before it factorise as before (unit pivots, the same integers); the pivot at
  `row` is 1 - 2 = -1."""
  assert 0 <= row < case['n']
  A = case['A'].copy()
  A[row, row] -= 2
  return A, row


# ---- comparing --------------------------------------------------------------------------------------------------------------------------
def compare_tiles(got, want, mask=None):
  """[ceil(rows / 128), ceil(cols / 128)] int64: per 128-tile the count of entries of `got` that differ from `want` (NaN differs from
  everything).  mask (bool, same shape): entries outside it are not looked at."""
  got = np.asarray(got, dtype=np.float64); want = np.asarray(want, dtype=np.float64)
  assert got.shape == want.shape and got.ndim == 2
  bad = ~(got == want)
  if mask is not None:
    bad &= mask
  R, Cc = got.shape
  nr, nc = so.npad_of(R) // TILE, so.npad_of(Cc) // TILE
  pad = np.zeros((nr * TILE, nc * TILE), bool); pad[:R, :Cc] = bad
  return pad.reshape(nr, TILE, nc, TILE).sum(axis=(1, 3)).astype(np.int64)


def lower_tile_mask(n):
  """entries of an [n, n] matrix in 128-tiles on or below the tile diagonal (whole diagonal tiles): where K^-1 is valid in S"""
  t = np.arange(n) // TILE
  return t[None, :] <= t[:, None]


def expected_outputs(case):
  """name -> (want [as float64], mask or None) for the hook's outputs on an exact case.  chol and W are compared everywhere, the part above
  the diagonal included (zeros); K^-1 on the tiles on and below the tile diagonal, diagonal tiles whole (symmetric)."""
  f = lambda a: a.astype(np.float64)
  return {'chol': (f(case['L']), None), 'w': (f(case['W']), None), 'kinv': (f(case['Kinv']), lower_tile_mask(case['n'])),
          'z': (f(case['z']), None), 'x': (f(case['x']), None)}


# ---- the real-valued family ---------------------------------------------------------------------------------------------------------------
LD = np.longdouble
REL_FACTOR = 4.0     # the rule and the names of divergence_cases.py: the device rounds where LAPACK rounds, only the order differs ...
FLOOR_C = 8.0        # ... and the floor covers a yardstick that lands within an ulp
REAL_NS = (515, 1153)
REAL_LENGTHSCALE, REAL_DIM, REAL_NOISE = 0.3, 3, 1e-2


def real_matrix(n):
  rng = np.random.default_rng(4242 + n)
  x = rng.uniform(size=(n, REAL_DIM)) / REAL_LENGTHSCALE
  d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=-1)
  return np.exp(-0.5 * d2) + REAL_NOISE * np.eye(n)


def chol_ld(K):
  """plain unblocked Cholesky in np.longdouble, column by column (left-looking: a column minus the rows so far times its own row)"""
  A = np.asarray(K, dtype=LD)
  n = A.shape[0]
  L = np.zeros((n, n), LD)
  for j in range(n):
    v = A[j:, j] - L[j:, :j] @ L[j, :j]
    L[j, j] = np.sqrt(v[0])
    L[j + 1:, j] = v[1:] / L[j, j]
  return L


def inv_lower_ld(L):
  """W = L^-1 by forward substitution on the identity, row by row, in np.longdouble (Wt holds W^T: the products read rows)"""
  n = L.shape[0]
  Wt = np.zeros((n, n), LD)
  for i in range(n):
    Wt[:i, i] = -(Wt[:i, :i] @ L[i, :i]) / L[i, i]
    Wt[i, i] = LD(1) / L[i, i]
  return np.ascontiguousarray(Wt.T)


def wtw_lower_ld(W):
  """W^T W in np.longdouble on the 128-tiles on and below the tile diagonal (zeros above), from the rows of W that reach them"""
  n = W.shape[0]
  Wt = np.ascontiguousarray(W.T)
  S = np.zeros((n, n), LD)
  for r0 in range(0, n, TILE):
    r1 = min(r0 + TILE, n)
    S[r0:r1, :r1] = Wt[r0:r1, r0:] @ W[r0:, :r1]
  return S


@functools.lru_cache(maxsize=None)
def real_case(n):
  """K (float64), the longdouble reference (L, W, Kinv = W^T W), and the float64 yardstick from scipy.linalg."""
  K = real_matrix(n)
  L = chol_ld(K)
  W = inv_lower_ld(L)
  ref = {'chol': L, 'w': W, 'kinv': wtw_lower_ld(W)}
  L64 = scipy.linalg.cholesky(K, lower=True)
  W64 = scipy.linalg.solve_triangular(L64, np.eye(n), lower=True)
  yard = {'chol': L64, 'w': W64, 'kinv': W64.T @ W64}
  rng = np.random.default_rng(n)
  return dict(n=n, K=K, b=rng.normal(size=(n, 1)), ref=ref, yard=yard)


def tile_errors(got, ref, mask=None):
  """[nblk, nblk]: per 128-tile max |got - ref| over the tile (masked entries count as 0; NaN as inf), over max |ref| of the whole matrix"""
  ref = np.asarray(ref, dtype=LD)
  err = np.abs(np.asarray(got, dtype=LD) - ref)
  err = np.where(np.isnan(err), np.inf, err)
  if mask is not None:
    err = np.where(mask, err, 0)
  n = ref.shape[0]
  nb = so.npad_of(n) // TILE
  pad = np.zeros((nb * TILE, nb * TILE), LD); pad[:n, :n] = err
  return (pad.reshape(nb, TILE, nb, TILE).max(axis=(1, 3)) / np.abs(ref).max()).astype(np.float64)


def real_masks(n):
  """where each output is compared: chol and W on and below the diagonal, K^-1 on the lower tiles"""
  low = np.tril(np.ones((n, n), bool))
  return {'chol': low, 'w': low, 'kinv': lower_tile_mask(n)}


def real_bound(case, name):
  """REL_FACTOR x (the yardstick's worst tile) + FLOOR_C eps n"""
  yard = tile_errors(case['yard'][name], case['ref'][name], real_masks(case['n'])[name]).max()
  return REL_FACTOR * yard + FLOOR_C * np.finfo(np.float64).eps * case['n'], yard


# ---- the option sets of the GPU tier ----------------------------------------------------------------------------------------------------
# Every set names the shapes it runs on (n of a single matrix, or the name of a batch), the options it sets on top of the defaults, and
# the fields of hbo_probe_plan it expects (include/hbo_tune.h; derived by hand from csrc/sched.h: potrf_plan, inv_plan): the GPU test
# asserts them BEFORE it compares, so that a set cannot silently test the default route.  forms (fp32 only): (chol_form, inv_forms).
OPTION_DEFAULTS = dict(lookahead=1, potrf_group=0, group_inner=-1, overlap_trtri=1, trtri_at=0, sweep=1, sweep_qs=0, small_nblk=-1,
                       sweep_big=4000, batch_bg=-1, split_f1=1, sweep_side=1, lauum_persist=1, trtri_free=48, cu_yield=2, bf16x3=1,
                       trtri3_min_s=8, spd_diag_bound=0, chol_f16x2=1)


class OptSet:
  def __init__(self, name, shapes, opts, plan, beside=1, dtypes=('fp64', 'fp32'), forms=None):
    assert set(opts) <= set(OPTION_DEFAULTS), name
    self.name, self.shapes, self.opts, self.plan, self.beside, self.dtypes, self.forms = name, tuple(shapes), dict(opts), dict(plan), beside, dtypes, forms


_LA = dict(lookahead=2)
_REC = dict(lookahead=2, sweep=0)     # the block-recursive inverse, started beside the chain
_SW = dict(lookahead=2, sweep=2)      # the one-sweep inverse
_BIG = dict(small_nblk=0)             # 128-tiles
_F32 = ('fp32',)
OPTION_SETS = [
    # ---- one matrix
    OptSet('default', SINGLES, {}, dict(la=0, q=1, sweep=0, early=0, small_shape=1)),
    OptSet('behind_chain', (1290,), _SW, dict(la=1, sweep=0, early=0, qs=0), beside=0),
    OptSet('early', (897, 1025, 1290), _REC, dict(la=1, q=3, q_inner=0, sweep=0, early=1, early_at=4, split_f1=0, small_shape=1)),
    OptSet('early_short', (515,), _REC, dict(la=1, early=1, early_at=-1)),            # five blocks: an early inverse that never gets a piece
    OptSet('no_overlap', (1290,), dict(_REC, overlap_trtri=0), dict(la=1, sweep=0, early=0)),
    OptSet('trtri_at12', (1290,), dict(_REC, trtri_at=12), dict(early=1, early_at=-1)),
    OptSet('trtri_at60', (897, 1290), dict(_REC, trtri_at=60), dict(early=1)),        # early_at 7 / 10: asserted per shape by the test
    OptSet('sweep_auto', (897, 1025, 1290), _SW, dict(la=1, sweep=1, qs=4, early=0, small_shape=1, d_own_stream=0)),
    OptSet('sweep_qs1', (1025,), dict(_SW, sweep_qs=1), dict(sweep=1, qs=1)),
    OptSet('sweep_qs2', (1025, 1290), dict(_SW, sweep_qs=2), dict(sweep=1, qs=2)),
    OptSet('sweep_qs8', (897, 1025), dict(_SW, sweep_qs=8), dict(sweep=1, qs=8)),
    OptSet('sweep_128', (1025, 1290), dict(_SW, **_BIG), dict(sweep=1, qs=4, small_shape=0, d_own_stream=1)),
    OptSet('sweep_128_side0', (1290,), dict(_SW, sweep_side=0, **_BIG), dict(sweep=1, small_shape=0, d_own_stream=0)),
    OptSet('sweep_big0', (1290,), dict(_SW, sweep_big=0), dict(sweep=1, small_shape=1)),
    OptSet('sweep_big_max', (1290,), dict(_SW, sweep_big=1 << 30), dict(sweep=1, small_shape=1)),
    OptSet('small_nblk4', (300, 515), dict(_REC, small_nblk=4), dict(la=1, sweep=0)),  # small_shape 1 / 0: asserted per shape by the test
    OptSet('early_128', (1290,), dict(_REC, **_BIG), dict(early=1, early_at=4, small_shape=0)),
    OptSet('lauum_plain', (1290,), dict(_REC, lauum_persist=0, **_BIG), dict(early=1, small_shape=0)),
    OptSet('trtri_free0', (1290,), dict(_REC, trtri_free=0), dict(early=1)),
    OptSet('trtri_free0_sweep', (1290,), dict(_SW, trtri_free=0), dict(sweep=1)),
    OptSet('trtri_free200', (1290,), dict(_SW, trtri_free=200, **_BIG), dict(sweep=1, small_shape=0)),
    OptSet('cu_yield0', (1290,), dict(_SW, cu_yield=0), dict(sweep=1, **{'yield': 0})),
    OptSet('cu_yield1', (1290,), dict(_REC, cu_yield=1), dict(early=1, **{'yield': 1})),
    OptSet('cu_yield2', (1290,), _SW, dict(sweep=1, **{'yield': 2})),
    OptSet('group2_la0', (515,), dict(lookahead=0, potrf_group=2), dict(la=0, q=2, q_inner=0)),            # panel groups 2, 2, 1
    OptSet('group8_la0', (1025,), dict(lookahead=0, potrf_group=8), dict(la=0, q=8)),
    OptSet('group1', (897,), dict(_SW, potrf_group=1), dict(la=1, q=1, sweep=1)),
    OptSet('group3', (1290,), dict(_REC, potrf_group=3), dict(la=1, q=3, early=1)),                        # panel groups 3, 3, 3, 2
    OptSet('group4_inner2', (1290,), dict(_SW, potrf_group=4, group_inner=2), dict(q=4, q_inner=2, sweep=1)),
    OptSet('group8_inner4', (1290,), dict(_REC, potrf_group=8, group_inner=4), dict(q=8, q_inner=4, early=1)),
    OptSet('split_f1_2', (1290,), dict(_REC, split_f1=2), dict(split_f1=1, early=1)),
    # ---- one matrix, fp32: the three product forms
    OptSet('fp32_mfma', (1290,), dict(_REC, bf16x3=0, trtri3_min_s=1, **_BIG), dict(early=1, small_shape=0), dtypes=_F32, forms=(0, 0)),
    OptSet('fp32_bf16x3', (897, 1290), dict(_REC, trtri3_min_s=1, **_BIG), dict(early=1, small_shape=0), dtypes=_F32, forms=(1, 1 | 4)),
    OptSet('fp32_bf16x3_behind', (1290,), dict(lookahead=0, trtri3_min_s=1, **_BIG), dict(la=0, early=0, small_shape=0), dtypes=_F32, forms=(1, 1 | 4)),
    OptSet('fp32_bf16x3_sweep', (1290,), dict(_SW, trtri3_min_s=1, **_BIG), dict(sweep=1, qs=4, small_shape=0), dtypes=_F32, forms=(1, 1)),
    OptSet('fp32_f16x2', (897, 1290), dict(_REC, trtri3_min_s=1, spd_diag_bound=1, **_BIG), dict(early=1, small_shape=0), dtypes=_F32, forms=(2, 2 | 8)),
    OptSet('fp32_f16x2_default', (1290,), dict(spd_diag_bound=1), dict(la=0, small_shape=1), dtypes=_F32, forms=(2, 0)),
    # ---- batches
    OptSet('batch_default', ('B1', 'B2'), {}, dict(la=0, q=1, sweep=0, early=0, batch_bg=1)),
    OptSet('batch_default_9', ('B3',), {}, dict(la=0, q=3, sweep=0, early=0, batch_bg=0)),
    OptSet('batch_sweep', ('B1', 'B2'), _LA, dict(la=1, q=3, sweep=1, qs=4, early=0, batch_bg=1, split_f1=1, tgran=4, small_shape=1, d_own_stream=0, **{'yield': 0})),
    OptSet('batch_9_la', ('B3',), _LA, dict(la=1, sweep=0, early=1, tgran=4, early_at=-1, batch_bg=0, split_f1=1)),   # five blocks: no sweep
    OptSet('batch_early', ('B1', 'B2'), _REC, dict(la=1, sweep=0, early=1, tgran=4, early_at=-1)),
    OptSet('batch_no_overlap', ('B1',), dict(_REC, overlap_trtri=0), dict(la=1, sweep=0, early=0)),
    OptSet('batch_behind', ('B1',), _LA, dict(la=1, sweep=0, early=0), beside=0),
    OptSet('batch_bg0', ('B1',), dict(_LA, batch_bg=0), dict(sweep=1, batch_bg=0, **{'yield': 0})),
    OptSet('batch_bg1', ('B2',), dict(_LA, batch_bg=1), dict(sweep=1, batch_bg=1, **{'yield': 0})),
    OptSet('batch_bg2', ('B1', 'B2'), dict(_LA, batch_bg=2), dict(sweep=1, batch_bg=2, **{'yield': 2})),
    OptSet('batch_bg2_yield0', ('B1',), dict(_LA, batch_bg=2, cu_yield=0), dict(sweep=1, batch_bg=2, **{'yield': 0})),
    OptSet('batch_qs1', ('B2',), dict(_LA, sweep_qs=1), dict(sweep=1, qs=1)),
    OptSet('batch_qs2', ('B1',), dict(_LA, sweep_qs=2), dict(sweep=1, qs=2)),
    OptSet('batch_qs8', ('B1',), dict(_LA, sweep_qs=8), dict(sweep=1, qs=8)),
    OptSet('batch_split_f1_0', ('B1',), dict(_LA, split_f1=0), dict(sweep=1, split_f1=0)),
    OptSet('batch_sweep_big0', ('B1',), dict(_LA, sweep_big=0), dict(sweep=1, small_shape=1)),
    OptSet('batch_128', ('B2',), dict(_LA, **_BIG), dict(sweep=1, small_shape=0, d_own_stream=0)),
    OptSet('batch_early_128', ('B1',), dict(_REC, **_BIG), dict(early=1, small_shape=0)),
    OptSet('batch_group4_inner2', ('B1',), dict(_LA, potrf_group=4, group_inner=2), dict(q=4, q_inner=2, sweep=1)),
    OptSet('batch_group2', ('B2',), dict(_REC, potrf_group=2), dict(q=2, early=1)),
    OptSet('batch_trtri_free0', ('B1',), dict(_LA, trtri_free=0), dict(sweep=1)),
    OptSet('batch_f16x2', ('B2',), dict(_LA, spd_diag_bound=1), dict(sweep=1), dtypes=_F32, forms=(2, 0)),
    OptSet('batch_mfma', ('B2',), dict(_LA, bf16x3=0), dict(sweep=1), dtypes=_F32, forms=(0, 0)),
]
# fields that depend on the shape, where a set runs on several: (set, shape) -> fields
PLAN_BY_SHAPE = {('trtri_at60', 897): dict(early_at=7), ('trtri_at60', 1290): dict(early_at=10),
                 ('small_nblk4', 300): dict(small_shape=1, early=0), ('small_nblk4', 515): dict(small_shape=0, early=1, early_at=-1)}


def shape_ns(shape):
  """(sizes, seeds) of a shape: one matrix of n points (seed 0), or a batch by name"""
  if isinstance(shape, str):
    ns = BATCHES[shape]
    return ns, tuple(task_seed(k) for k in range(len(ns)))
  return (shape,), (0,)


def expected_plan(s, shape):
  return dict(s.plan, **PLAN_BY_SHAPE.get((s.name, shape), {}))
