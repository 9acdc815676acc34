"""CPU side of the full-covariance tier (hbo_predict(..., full_cov=1): GEMM_POST writing V, GEMM_VTV, the multi-tile M x M Gram with the
candidates' padded leading dimension, the pitched copy out).  Shared by tests/test_full_cov_host.py (this file judged on its own) and
tests/test_gpu_full_cov.py (the device against it):

  reference(case)      mu, the prior Kqq and cov from oracle/hyperbo_oracle.py: predict(..., full_cov=True), always evaluated in fp64
                       (fp32 cases: on the fp32-rounded inputs and parameters, as tests/test_gpu_small_path.py does)
  second_route(case)   the same covariance without a Cholesky: Kqq - Kxq^T solve(K + (noise + eps) I, Kxq); its gap to reference() is
                       the reference's own uncertainty
  fp32_yardstick(case) the same formula in NumPy float32 on Gram entries rounded once from the fp64 oracle: NOT a tolerance, the scale of
                       error that fp32 arithmetic itself produces on the case (printed beside the device's error)
  MUTANTS              the reference with one failure the kernels could have, each; test_full_cov_host.py proves that every one of them
                       is far outside the bound the GPU test applies
  CASES ...            the case lists of both test files, and the bounds
"""
import functools
from typing import NamedTuple, Optional

import numpy as np
import scipy.linalg as spla

import helpers
import kumar_oracle
from oracle import hyperbo_oracle as o

WFO = o.DEFAULT_WARP_FUNC
TILE = 128
EPS_JITTER = 1e-6           # the eps of solve_gp_linear_system (oracle and library)

# ---- bounds of the GPU tier ------------------------------------------------------------------------------------------------------
FP64_COV_TOL = 1e-9         # max |cov - ref| <= tol * max |ref|  (the bound test_factor_predict_acquisition_vs_oracle holds M = 70 to)
FP64_MU_TOL = 1e-9
FP32_MU_TOL = 5e-4          # of max(max |mu|, 1)
# fp32: relative to max |Kqq| (the operands' scale).  10 x the worst device error measured on the MI355X over the list
# (profiles/full_cov_errors.md).
FP32_COV_TOL = 8.7e-6       # edge cases (worst 8.68e-7: matern32 + linear, n = M = 300), the resident-grid case (9.3e-7) and the direct-form Gram of the wide cases (6.3e-7)
FP32_COV_TOL_WIDE_MFMA = 6.7e-6   # d = 64 with the Gram on the matrix cores (worst 6.61e-7): a row of its own, an absolute Gram error is amplified through K^-1
ROUTE_GAP_TOL = 1e-10       # the two fp64 routes, relative to max |cov|
CONDITION = 0.5             # every 128-tile: max |Kqq - cov| >= CONDITION * max |Kqq|
MUTANT_FACTOR = 100.0       # every mutant moves an entry by at least this many bounds

# (kernel, MLP basis, mean, Kumaraswamy warp): tests/test_gpu_parity.py CASES plus one *_kumar family
FAMILIES = [('squared_exponential', False, 'constant', False), ('matern52', True, 'linear_mlp', False),
            ('matern32', False, 'linear', False), ('dot_product', True, 'zero', False), ('matern52', False, 'constant', True)]
EDGE_SIZES = [(1, 1), (5, 129), (128, 128), (129, 127), (129, 257), (257, 129), (300, 1), (300, 300), (385, 300)]
DTYPES = ['fp64', 'fp32']


class Case(NamedTuple):
  group: str                 # 'edge' | 'wide' | 'resident'
  kname: str
  mlp: bool
  mname: str
  kumar: bool
  n: int
  M: int
  d: int
  dtype: str                 # 'fp64' | 'fp32'
  noise: Optional[float] = None   # raw noise_variance when the default of helpers.make_model does not do

  @property
  def id(self):
    fam = self.kname + ('_mlp' if self.mlp else '') + ('_kumar' if self.kumar else '') + '+' + self.mname
    return f'{self.group}-{fam}-n{self.n}-M{self.M}-d{self.d}-{self.dtype}'

  @property
  def np_dtype(self):
    return np.float64 if self.dtype == 'fp64' else np.float32

  @property
  def kernel_name(self):
    return self.kname + ('_mlp' if self.mlp else '') + ('_kumar' if self.kumar else '')


def _edge_noise(kname, n, M):
  """Raw noise variance of an edge case (None: that of helpers.make_model, softplus(-2) = 0.13).  The dot-product kernel on 5 MLP
  features has rank 6: after 256 observations the last 44 rows of V hold what the noise leaves, 3e-4 of the prior's scale, and
  mutant (b) would not be live in fp32 at n = M = 300; with softplus(0.5) = 0.97 it is."""
  return 0.5 if (kname, n, M) == ('dot_product', 300, 300) else None


EDGE_CASES = [Case('edge', k, mlp, mn, ku, n, M, 3, dt, _edge_noise(k, n, M))
              for (k, mlp, mn, ku) in FAMILIES for (n, M) in EDGE_SIZES for dt in DTYPES]
# fp32 with >= 32 features: the Gram matrices take the matrix-core form (or the direct form on a context with gram_mfma = 0)
WIDE_CASES = [Case('wide', k, False, 'constant', False, 300, 300, 64, 'fp32') for k in ('squared_exponential', 'matern52')]
# the resident-grid product: 32 row blocks; M for a device of `cus` compute units from resident_sizes()
RESIDENT_N = 4096
RESIDENT_PER_TILE = 4       # queries checked per 128-tile of the query grid


def resident_sizes(cus):
  """(M of the resident grid, M of the plain grid) for n = 4096: the smallest multiple of 128 with (M / 128) * 32 > 4 * cus, and the
  largest one that still is not (api_internal.h: PostPlan::chunk)."""
  nblk = RESIDENT_N // TILE
  t = (4 * cus) // nblk + 1
  return t * TILE, (t - 1) * TILE


def resident_case(dtype, cus=256):
  return Case('resident', 'matern52', False, 'constant', False, RESIDENT_N, resident_sizes(cus)[0], 4, dtype)


def resident_subset(M):
  """RESIDENT_PER_TILE queries of every 128-tile of M queries: the tile's first and last valid index and two drawn ones."""
  rng = np.random.default_rng(M)
  idx = []
  for lo in range(0, M, TILE):
    hi = min(M, lo + TILE) - 1
    idx += [lo, hi] + sorted(int(i) for i in rng.choice(np.arange(lo + 1, hi), size=RESIDENT_PER_TILE - 2, replace=False))
  return np.asarray(idx)


RESIDENT_CASES = [resident_case(dt) for dt in DTYPES]
CASES = EDGE_CASES + WIDE_CASES + RESIDENT_CASES   # what test_full_cov_host.py judges


def cov_bound(case, gram_form='default'):
  """(tolerance, name of the scale) of the GPU test for this case: fp64 relative to max |ref cov|, fp32 to max |Kqq|."""
  if case.dtype == 'fp64':
    return FP64_COV_TOL, 'cov'
  if case.group == 'wide' and gram_form != 'direct':
    return FP32_COV_TOL_WIDE_MFMA, 'kqq'
  return FP32_COV_TOL, 'kqq'


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def cast(tree, dtype):
  return {k: cast(v, dtype) for k, v in tree.items()} if isinstance(tree, dict) else np.asarray(tree, dtype=dtype)


@functools.lru_cache(maxsize=None)
def inputs(case):
  """model (in the case's dtype), x, y, xq (in the case's dtype).  Observations from helpers.synthetic_task; queries uniform in the unit
  cube, except below one block of observations, where uniform queries are mostly far from all of them and the posterior correction
  would be a small part of most tiles: there every query is an observed input moved by 1e-2."""
  fam = FAMILIES.index((case.kname, case.mlp, case.mname, case.kumar)) if (case.kname, case.mlp, case.mname, case.kumar) in FAMILIES else 9
  rng = np.random.default_rng([fam, case.n, case.M, case.d, 17])
  model = helpers.make_model(rng, case.mname, case.mlp, case.d)
  if case.d >= 32:   # a Gram that neither decays to the diagonal nor fills with ones (tests/test_gpu_small_path.py: _lengthscale)
    model['lengthscale'] = helpers.inv_softplus(0.5 * np.sqrt(case.d) * np.exp(rng.uniform(-0.4, 0.4, size=case.d)))
  if case.kumar:
    model['kumar_params'] = {'a': rng.uniform(-1.0, 1.0, size=case.d), 'b': rng.uniform(-1.0, 1.0, size=case.d)}
  if case.noise is not None:
    model['noise_variance'] = np.array(case.noise)
  x, y = helpers.synthetic_task(rng, case.n, case.d)
  if case.n >= TILE:
    xq = rng.uniform(size=(case.M, case.d))
  else:
    xq = np.clip(x[np.arange(case.M) % case.n] + 1e-2 * rng.normal(size=(case.M, case.d)), 0.0, 1.0)
  # the first query of every 128-tile: the observed input of the largest prior variance, moved by 1e-2.  (The dot-product kernel is not
  # stationary: a tile of one query -- M = 129, 257 -- whose query has a small norm would hold nothing of the prior's scale.)
  po = o.GPParams(model=cast(model, np.float64), config={'mlp_features': helpers.MLP_FEATURES})
  top = int(np.argmax(oracle_funcs(case)[1](po, x, warp_func=WFO, diag=True)))
  first = np.arange(0, case.M, TILE)
  xq[first] = np.clip(x[top] + 1e-2 * rng.normal(size=(len(first), case.d)), 0.0, 1.0)
  dt = case.np_dtype
  return cast(model, dt), x.astype(dt), y.astype(dt), xq.astype(dt)


def oracle_funcs(case):
  ko = getattr(o, case.kname + ('_mlp' if case.mlp else ''))
  if case.kumar:
    ko = kumar_oracle.kumar_kernel(ko)
  return getattr(o, case.mname), ko


def oracle_params(case):
  return o.GPParams(model=cast(inputs(case)[0], np.float64), config={'mlp_features': helpers.MLP_FEATURES})


def _xyq64(case, idx):
  _, x, y, xq = inputs(case)
  xq = xq if idx is None else xq[np.asarray(idx)]
  return x.astype(np.float64), y.astype(np.float64), xq.astype(np.float64)


class Ref(NamedTuple):
  mu: np.ndarray
  kqq: np.ndarray
  cov: np.ndarray


def _reference(case, idx):
  mo, ko = oracle_funcs(case)
  po = oracle_params(case)
  x, y, xq = _xyq64(case, idx)
  mu, cov = o.predict(mo, ko, po, x, y, xq, WFO, full_cov=True)
  return Ref(mu, ko(po, xq, warp_func=WFO), cov)


@functools.lru_cache(maxsize=None)
def _reference_whole(case):
  return _reference(case, None)


def reference(case, idx=None):
  """Ref(mu, Kqq, cov) of the case's queries (idx: of that subset of them), fp64.  Shared and not to be written to."""
  return _reference_whole(case) if idx is None else _reference(case, tuple(int(i) for i in idx))


def _grams(case, idx=None):
  """K + (noise + eps) I, Kxq, Kqq from the fp64 oracle.  Shared and not to be written to."""
  return _grams_cached(case, None if idx is None else tuple(int(i) for i in idx))


@functools.lru_cache(maxsize=4)
def _grams_cached(case, idx):
  mo, ko = oracle_funcs(case)
  po = oracle_params(case)
  x, y, xq = _xyq64(case, idx)
  _, a = o.compute_delta_y_and_cov(mo, ko, po, x, y, WFO, EPS_JITTER)
  return a, ko(po, x, xq, warp_func=WFO), ko(po, xq, warp_func=WFO)


def second_route(case, idx=None):
  a, kxq, kqq = _grams(case, idx)
  return kqq - kxq.T @ np.linalg.solve(a, kxq)


def fp32_yardstick(case, idx=None):
  """cov in NumPy float32: Cholesky (spotrf), triangular solve (strsm), product (sgemm) on entries rounded once from fp64."""
  a, kxq, kqq = (m.astype(np.float32) for m in _grams(case, idx))
  chol = np.linalg.cholesky(a)
  v = spla.solve_triangular(chol, kxq, lower=True, check_finite=False)
  assert chol.dtype == np.float32 and v.dtype == np.float32
  return kqq - v.T @ v


# ---- per-tile errors -------------------------------------------------------------------------------------------------------------
def tile_errors(got, ref):
  """max |got - ref| per 128-tile: array [ceil(M / 128), ceil(M / 128)] (NaN counts as infinite)."""
  diff = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
  diff = np.where(np.isfinite(diff), diff, np.inf)
  m = diff.shape[0]
  nt = (m + TILE - 1) // TILE
  out = np.zeros((nt, nt))
  for i in range(nt):
    for j in range(nt):
      out[i, j] = diff[i * TILE:(i + 1) * TILE, j * TILE:(j + 1) * TILE].max()
  return out


def worst_tile(got, ref):
  """(max |got - ref|, (tile row, tile column) where it is)."""
  te = tile_errors(got, ref)
  ij = np.unravel_index(int(np.argmax(te)), te.shape)
  return float(te[ij]), (int(ij[0]), int(ij[1]))


def condition_per_tile(ref):
  """min over the 128-tiles of max |Kqq - cov| in the tile, as a fraction of max |Kqq|."""
  te = tile_errors(ref.kqq, ref.cov)
  return float(te.min() / np.max(np.abs(ref.kqq)))


# ---- mutants ---------------------------------------------------------------------------------------------------------------------
def _parts(case):
  """Kqq, Kxq and V = L^-1 Kxq of the reference."""
  a, kxq, kqq = _grams(case)
  chol = spla.cholesky(a, lower=True, check_finite=False)
  return kqq, kxq, spla.solve_triangular(chol, kxq, lower=True, check_finite=False)


def _padded_ld(mpad, itemsize):
  """The candidates' padded leading dimension (csrc/runtime.h: padded_ld): 128 bytes beyond mpad."""
  return mpad + 128 // itemsize


def mutant_a(case):
  """One 128-tile of the output left at Kqq: GEMM_VTV skipped a tile.  The off-diagonal tile (1, 0) where the query grid has one;
  with a single tile of queries, that tile."""
  ref = reference(case)
  out = ref.cov.copy()
  r, c = ((1, 0) if case.M > TILE else (0, 0))
  out[r * TILE:(r + 1) * TILE, c * TILE:(c + 1) * TILE] = ref.kqq[r * TILE:(r + 1) * TILE, c * TILE:(c + 1) * TILE]
  return out


def mutant_b(case):
  """The last 128-row block of V (for n not a multiple of 128: the last, partial block) missing from V^T V: a K range one block short."""
  kqq, _, v = _parts(case)
  keep = ((case.n - 1) // TILE) * TILE
  return kqq - v[:keep].T @ v[:keep]


def mutant_c(case):
  """Rows >= n of V not zero: the identity padding of W leaking what the padded rows of Kxq hold (ones).  None when n has no padded
  rows."""
  npad = -(-case.n // TILE) * TILE
  if npad == case.n:
    return None
  kqq, _, v = _parts(case)
  vp = np.vstack([v, np.ones((npad - case.n, case.M))])
  return kqq - vp.T @ vp


def mutant_d(case, delta=32):
  """The copy out with the wrong pitch: row i read at offset i * ldq from a buffer laid out with ldq + delta (delta = +-32).  None for a
  single row, which has no pitch."""
  if case.M == 1:
    return None
  ref = reference(case)
  m = case.M
  mpad = -(-m // TILE) * TILE
  ldq = _padded_ld(mpad, 8 if case.dtype == 'fp64' else 4)
  ld_buf = ldq + delta
  buf = np.zeros(mpad * ld_buf + ldq * mpad)
  for i in range(m):
    buf[i * ld_buf:i * ld_buf + m] = ref.cov[i]
  return np.stack([buf[i * ldq:i * ldq + m] for i in range(m)])


def mutant_e(case):
  """The second tile column of Kqq computed from the first tile's queries (bxi dropped from the Gram's x2 address).  None with a
  single tile column."""
  if case.M <= TILE:
    return None
  mo, ko = oracle_funcs(case)
  kqq, _, v = _parts(case)
  _, _, xq = _xyq64(case, None)
  w = min(case.M, 2 * TILE) - TILE
  kqq = kqq.copy()
  kqq[:, TILE:TILE + w] = ko(oracle_params(case), xq, xq[:w], warp_func=WFO)
  return kqq - v.T @ v


MUTANTS = {'a': mutant_a, 'b': mutant_b, 'c': mutant_c, 'd': mutant_d, 'e': mutant_e}


def not_applicable(case):
  """Mutants whose failure cannot exist at the case's shape (each returns None there): nothing to skip, there is no such tile, row
  or pitch."""
  na = set()
  if case.n % TILE == 0:
    na.add('c')      # no padded rows
  if case.M == 1:
    na.add('d')      # one row: no pitch
  if case.M <= TILE:
    na.add('e')      # one tile column
  return na


# Mutants that exist at a case's shape but move no entry by MUTANT_FACTOR bounds there, at most one per case.  All of them are (b) in
# fp32 (in fp64 every mutant is live at every case): with one or two full blocks of observations in front of it, the last, partial block
# of V holds 2e-5 .. 7e-4 of the prior's scale, below 100 x the fp32 bound = 8.7e-4 of it.  (n, M, kernel) -> letters.
WEAK_FP32 = {(257, 129, 'squared_exponential'): 'b', (300, 1, 'squared_exponential'): 'b', (385, 300, 'squared_exponential'): 'b',
             (300, 1, 'matern52_mlp'): 'b', (385, 300, 'matern52_mlp'): 'b', (300, 1, 'matern32'): 'b',
             (129, 127, 'dot_product_mlp'): 'b', (129, 257, 'dot_product_mlp'): 'b', (257, 129, 'dot_product_mlp'): 'b',
             (300, 1, 'dot_product_mlp'): 'b', (385, 300, 'dot_product_mlp'): 'b', (257, 129, 'matern52_kumar'): 'b'}


def weak_mutants(case):
  return WEAK_FP32.get((case.n, case.M, case.kernel_name), '') if case.dtype == 'fp32' else ''
