"""CPU side of the row-append tier (hbo_cache_append, csrc/cache.hip: tri_matvec_kernel for l = W k(X, x*), wtz_partial_kernel /
wtz_final_kernel through xover / oover for W^T l, append_row_kernel) on caches of MORE than one 128-row block.  Shared by
tests/test_append_cases_host.py (this file judged on its own) and tests/test_gpu_cache_append.py (the device against it):

  CASES / FP32_CASES   n0 observations, then append calls of the given sizes: two blocks; the capacity edge (the append that ends at
                       npad exactly is accepted in place, one row more is not); five blocks (a second 512-row chunk of W^T l); nine
                       blocks (the split-K posterior); 60 single-row calls (drift); the registry, Kumaraswamy and three target columns
  inputs(case)         model, x, y, xq in the case's dtype; three of the queries ARE appended points (their variance is made of the
                       new rows of W almost alone)
  reference(case)      per call, the oracle's from-scratch factorisation of the data so far (o.solve_gp_linear_system, o.predict,
                       o.gp_predict_postprocess), always in fp64 (fp32 cases: on the fp32-rounded inputs and parameters)
  oracle_state_ld      the same in np.longdouble: the yardstick of the reference's own error
  restate(case, mut)   a NumPy fp64 restatement of the recurrences in the comment above append_row_kernel, maintaining L, W, z, alpha
                       and resid row by row; `mut` names the one line of it that is changed (MUTANTS)
  errors / ratios      what the GPU test measures after every call, and the fp64 bounds it holds them to; part_errors /
                       array_errors / relative_bounds: the same for the drift and fp32 cases, against a fresh factorisation's error
"""
import functools
import types
from typing import NamedTuple, Tuple

import numpy as np
import scipy.linalg as spla

import helpers
import kumar_oracle
from oracle import hyperbo_oracle as o

WFO = o.DEFAULT_WARP_FUNC
TILE = 128
EPS = 1e-6                  # the jitter of linalg.py:36-69

# ---- bounds of the GPU tier ------------------------------------------------------------------------------------------------------
# fp64: the project's bounds for this operation (test_incremental_cache_append_matches_refactorisation: chol 1e-9, kinvy 1e-8, mu / var
# 1e-8, helpers.rel_err), here on every part of its own.  ymu = y - m(x) is one subtraction behind the mean function: 1e-13 of its
# largest entry, the bound of test_factor_predict_acquisition_vs_oracle.
FP64_BOUNDS = {'chol_new': 1e-9, 'kinvy_old': 1e-8, 'kinvy_new': 1e-8, 'ymu': 1e-13, 'mu': 1e-8, 'var': 1e-8}
# drift and fp32: err_append <= REL_FACTOR * err_fresh + FLOOR_C * eps(dtype), every error relative to the largest reference entry of its
# array (part_errors, array_errors, relative_bounds).  The 4: each appended row adds one more pair of length-n dot products, summed in
# fp64 and rounded to the dtype; measured on an MI355X the ratio stays below 2 (tests/test_gpu_cache_append.py: RATIOS_MEASURED).
# The floor, for where the fresh factorisation happens to land within an ulp of the reference: five roundings to the dtype stand between
# the fp64 sums and a stored element (l, W^T l, z, the pivot d, the element itself), half an ulp each = 2.5 eps; 8 eps leaves a factor of
# three for their way through the two dot products.
REL_FACTOR = 4.0
FLOOR_C = 8.0
MUTANT_FACTOR = 100.0       # fp64: every applicable mutant is at least this many bounds away in some part, after some call


class Case(NamedTuple):
  name: str
  kname: str                 # the base kernel
  mlp: bool                  # the kernel works on the MLP basis (helpers.MLP_FEATURES)
  mname: str
  kumar: bool
  n0: int                    # observations of the first factorisation
  calls: Tuple[int, ...]     # rows per append call, in order
  mcols: int = 1             # target columns
  M: int = 40                # queries
  d: int = 3
  dtype: str = 'fp64'

  @property
  def id(self):
    return f'{self.name}-{self.kernel_name}+{self.mname}-n{self.n0}' + ''.join(f'+{c}' for c in self.calls[:4]) + \
        (f'..x{len(self.calls)}' if len(self.calls) > 4 else '') + (f'-m{self.mcols}' if self.mcols > 1 else '') + f'-{self.dtype}'

  @property
  def kernel_name(self):
    return self.kname + ('_mlp' if self.mlp else '') + ('_kumar' if self.kumar else '')

  @property
  def np_dtype(self):
    return np.float64 if self.dtype == 'fp64' else np.float32

  @property
  def n_total(self):
    return self.n0 + sum(self.calls)

  @property
  def sizes(self):
    """(n before, n after) of every call."""
    out, n = [], self.n0
    for c in self.calls:
      out.append((n, n + c)); n += c
    return out

  @property
  def in_place(self):
    """Per call: it fits the padded capacity of the cache it meets (hbo_cache_append accepts it) -- else the cache is re-factorised."""
    out, cap = [], -(-self.n0 // TILE) * TILE
    for n, n1 in self.sizes:
      out.append(n1 <= cap)
      if n1 > cap:
        cap = -(-n1 // TILE) * TILE
    return out


SHAPE = ('matern52', False, 'constant', False)
REGISTRY = [('squared_exponential', False, 'constant'), ('matern52', True, 'linear_mlp'), ('matern32', False, 'linear'),
            ('dot_product', True, 'zero')]      # tests/test_gpu_parity.py: CASES
TWO_BLOCKS = [Case('two', *SHAPE, 129, (1,)), Case('two', *SHAPE, 200, (7, 1, 1))]
EDGE = Case('edge', *SHAPE, 250, (6, 1))        # 256 = npad: in place; the 257th row is refused, the cache re-factorised
FIVE_BLOCKS = [Case('five', *SHAPE, 513, (3,)), Case('five', *SHAPE, 600, (40,))]
NINE_BLOCKS = Case('nine', *SHAPE, 1030, (5,))
DRIFT = Case('drift', *SHAPE, 130, (1,) * 60)
REGISTRY_CASES = ([Case('registry', k, mlp, mn, False, 200, (5,)) for (k, mlp, mn) in REGISTRY] +
                  [Case('registry', 'squared_exponential', False, 'constant', True, 200, (5,)),
                   Case('registry', 'matern52', False, 'constant', False, 200, (5,), mcols=3)])
FIXED_BOUND_CASES = TWO_BLOCKS + [EDGE] + FIVE_BLOCKS + [NINE_BLOCKS] + REGISTRY_CASES     # fp64, held to FP64_BOUNDS
CASES = FIXED_BOUND_CASES + [DRIFT]
FP32_CASES = [c._replace(dtype='fp32') for c in TWO_BLOCKS + FIVE_BLOCKS + [DRIFT]]
ONCE_CASES = [TWO_BLOCKS[1], FIVE_BLOCKS[1]]    # full covariance, EI and its gradient after the first call: 200 +7 and 600 +40


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def cast(tree, dtype):
  return {k: cast(v, dtype) for k, v in tree.items()} if isinstance(tree, dict) else np.asarray(tree, dtype=dtype)


def _seed(case):
  return [sum(ord(ch) for ch in case.name), helpers.KERNELS.index(case.kname), int(case.mlp), helpers.MEANS.index(case.mname), int(case.kumar),
          case.n0, case.n_total, len(case.calls), case.mcols, case.M, case.d, 29]


def new_queries(case):
  """Indices into x of the three appended points that are also queries 0, 1, 2: the first, the middle and the last appended row."""
  return [case.n0, case.n0 + (case.n_total - case.n0) // 2, case.n_total - 1]


@functools.lru_cache(maxsize=None)
def inputs(case):
  """(model, x, y, xq) in the case's dtype; fp32 cases are rounded here, once.  The dtype is not part of the seed."""
  rng = np.random.default_rng(_seed(case))
  model = helpers.make_model(rng, case.mname, case.mlp, case.d)
  if case.kumar:
    model['kumar_params'] = {'a': rng.uniform(-1.0, 1.0, size=case.d), 'b': rng.uniform(-1.0, 1.0, size=case.d)}
  x, y = helpers.synthetic_task(rng, case.n_total, case.d, m=case.mcols)
  xq = rng.uniform(0.05, 0.95, size=(case.M, case.d))
  xq[:3] = x[new_queries(case)]
  dt = case.np_dtype
  return cast(model, dt), x.astype(dt), y.astype(dt), np.ascontiguousarray(xq.astype(dt))


def config(case):
  return {'mlp_features': helpers.MLP_FEATURES}


class Setup(NamedTuple):
  mo: object
  ko: object
  po: object
  x: np.ndarray
  y: np.ndarray
  xq: np.ndarray
  noise: float


@functools.lru_cache(maxsize=None)
def oracle_setup(case):
  """The oracle's functions and fp64 parameters and inputs (a Kumaraswamy kernel: kumar_oracle's composition with the base kernel)."""
  model, x, y, xq = inputs(case)
  m64 = cast(model, np.float64)
  base = getattr(o, case.kname + ('_mlp' if case.mlp else ''))
  ko = kumar_oracle.kumar_kernel(base) if case.kumar else base
  po = o.GPParams(model=m64, config=config(case))
  noise = float(np.squeeze(o.retrieve_params(po, ['noise_variance'], WFO)[0]))
  return Setup(getattr(o, case.mname), ko, po, x.astype(np.float64), y.astype(np.float64), xq.astype(np.float64), noise)


# ---- reference -------------------------------------------------------------------------------------------------------------------
class State(NamedTuple):
  """What the GPU test reads back after a call (or the reference's counterpart): the export and the posterior at the queries."""
  n: int
  chol: np.ndarray   # (n, n)
  kinvy: np.ndarray  # (n, mcols)
  ymu: np.ndarray    # (n, mcols)
  mu: np.ndarray     # (M,)  GP.predict: column 0, with noise, T / (T - 1) = 1 (one sub-dataset)
  var: np.ndarray    # (M,)


def oracle_state(case, n):
  """The oracle's from-scratch factorisation of the first n observations and its posterior at the queries."""
  s = oracle_setup(case)
  x, y = s.x[:n], s.y[:n]
  chol, kinvy, ymu = o.solve_gp_linear_system(s.mo, s.ko, s.po, x, y, WFO)
  mu, var = o.predict(s.mo, s.ko, s.po, x, y, s.xq, WFO, cache=types.SimpleNamespace(chol=chol, kinvy=kinvy))
  mu, var = o.gp_predict_postprocess(s.po, {0: o.SubDataset(x, y)}, mu, var, WFO, False, True, True)
  return State(n, chol, kinvy, ymu, np.asarray(mu, dtype=np.float64)[:, 0].copy(), np.asarray(var, dtype=np.float64)[:, 0].copy())


@functools.lru_cache(maxsize=None)
def reference(case):
  """One State per call.  Shared and not to be written to."""
  return [oracle_state(case, n1) for _, n1 in case.sizes]


@functools.lru_cache(maxsize=None)
def initial(case):
  return oracle_state(case, case.n0)


# ---- the same in np.longdouble ---------------------------------------------------------------------------------------------------
LD = np.longdouble


def _chol_ld(a):
  n = a.shape[0]
  c = np.zeros_like(a)
  for j in range(n):
    v = a[j:, j] - c[j:, :j] @ c[j, :j]
    c[j, j] = np.sqrt(v[0])
    c[j + 1:, j] = v[1:] / c[j, j]
  return c


def _solve_lower_ld(c, b, trans=False):
  """c^-1 b (trans: c^-T b), c lower triangular, b (n, k)."""
  n = c.shape[0]
  v = np.zeros_like(b)
  if not trans:
    for i in range(n):
      v[i] = (b[i] - c[i, :i] @ v[:i]) / c[i, i]
  else:
    for i in range(n - 1, -1, -1):
      v[i] = (b[i] - c[i + 1:, i] @ v[i + 1:]) / c[i, i]
  return v


def oracle_state_ld(case, n):
  """oracle_state with every array in np.longdouble: the oracle's own kernels and means on longdouble inputs (they compute in the dtype of
  their inputs), the Kumaraswamy warp restated here (kumar_oracle.warp rounds to fp64), Cholesky and substitutions by hand."""
  s = oracle_setup(case)
  x, y, xq = s.x[:n].astype(LD), s.y[:n].astype(LD), s.xq.astype(LD)
  ko = s.ko
  if case.kumar:
    kp = s.po.model['kumar_params']
    a, b = kumar_oracle.squareplus(kp['a']).astype(LD), kumar_oracle.squareplus(kp['b']).astype(LD)
    x, xq = 1 - (1 - x ** a) ** b, 1 - (1 - xq ** a) ** b
    ko = getattr(o, case.kname)
  ymu = y - s.mo(s.po, s.x[:n].astype(LD), warp_func=WFO)
  cov = ko(s.po, x, warp_func=WFO) + np.eye(n, dtype=LD) * (LD(s.noise) + LD(EPS))
  assert cov.dtype == LD and ymu.dtype == LD
  chol = _chol_ld(cov)
  kinvy = _solve_lower_ld(chol, _solve_lower_ld(chol, ymu), trans=True)
  kxq = ko(s.po, x, xq, warp_func=WFO)
  mu = kxq.T @ kinvy[:, 0] + s.mo(s.po, s.xq.astype(LD), warp_func=WFO)[:, 0]
  v = _solve_lower_ld(chol, kxq)
  var = ko(s.po, xq, warp_func=WFO, diag=True) - np.sum(v * v, axis=0) + LD(s.noise)
  assert mu.dtype == LD and var.dtype == LD
  return State(n, chol, kinvy, ymu, mu, var)


# ---- what the GPU test measures --------------------------------------------------------------------------------------------------
def _rel(a, b):
  """max |a - b| over max |b|, in the precision of the wider side; anything not finite is infinitely far."""
  a, b = np.asarray(a), np.asarray(b)
  wide = LD if LD in (a.dtype.type, b.dtype.type) else np.float64
  a, b = a.astype(wide), b.astype(wide)
  if not a.size:
    return 0.0
  e = np.max(np.abs(a - b))
  return float(e / (np.max(np.abs(b)) + wide(1e-300))) if np.isfinite(e) else np.inf


QUERY_FLOOR = 1e-3          # of the largest reference value: the scale of a query whose own value all but cancels (helpers.assert_grad_close)


def _per_query(a, b):
  """max over the queries of |a_q - b_q| / max(|b_q|, QUERY_FLOOR max |b|): every query against its own size.  (mu_q = k_q . alpha + m(x_q)
  can cancel to nothing; its rounding error cannot, so a query below the floor is held to the floor.)"""
  a, b = np.asarray(a), np.asarray(b)
  wide = LD if LD in (a.dtype.type, b.dtype.type) else np.float64
  a, b = a.astype(wide), b.astype(wide)
  e = np.abs(a - b) / np.maximum(np.abs(b), wide(QUERY_FLOOR) * np.max(np.abs(b)))
  return float(np.max(e)) if np.isfinite(e).all() else np.inf


def errors(got, ref, n0):
  """The parts the fp64 bounds are applied to -- the appended parts on their own, a max-norm over a whole array hides a wrong last row:
  rows n0: of chol; kinvy over :n0 and over n0:; ymu; each relative to the largest reference entry of the part (helpers.rel_err); mu and
  var per query (_per_query)."""
  assert got.n == ref.n and got.chol.shape == ref.chol.shape, (got.n, ref.n)
  return {'chol_new': _rel(got.chol[n0:], ref.chol[n0:]), 'kinvy_old': _rel(got.kinvy[:n0], ref.kinvy[:n0]),
          'kinvy_new': _rel(got.kinvy[n0:], ref.kinvy[n0:]), 'ymu': _rel(got.ymu, ref.ymu),
          'mu': _per_query(got.mu, ref.mu), 'var': _per_query(got.var, ref.var)}


def ratios(got, ref, n0):
  """errors() over FP64_BOUNDS."""
  e = errors(got, ref, n0)
  return {k: v / FP64_BOUNDS[k] for k, v in e.items()}


# drift and fp32 -- the parts of an appended cache, and the array of a fresh factorisation whose error each is held against
PART_OF = {'chol_new': 'chol', 'kinvy_old': 'kinvy', 'kinvy_new': 'kinvy', 'ymu': 'ymu', 'mu': 'mu', 'var': 'var', 'mu_new': 'mu', 'var_new': 'var'}
ARRAYS = ('chol', 'kinvy', 'ymu', 'mu', 'var')


def _max_err(a, b):
  e = np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))) if np.size(a) else 0.0
  return float(e) if np.isfinite(e) else np.inf


def array_errors(got, ref):
  """max |got - ref| over each whole array, relative to the array's largest reference entry: the error level of a factorisation."""
  return {k: _max_err(getattr(got, k), getattr(ref, k)) / float(np.max(np.abs(getattr(ref, k)))) for k in ARRAYS}


def part_errors(got, ref, n0):
  """max |got - ref| over each part (the parts of errors(), and the three queries that are appended points on their own), relative
  to the largest reference entry of the WHOLE array: the same unit as array_errors()."""
  assert got.n == ref.n and got.chol.shape == ref.chol.shape, (got.n, ref.n)
  sc = {k: float(np.max(np.abs(getattr(ref, k)))) for k in ARRAYS}
  return {'chol_new': _max_err(got.chol[n0:], ref.chol[n0:]) / sc['chol'], 'kinvy_old': _max_err(got.kinvy[:n0], ref.kinvy[:n0]) / sc['kinvy'],
          'kinvy_new': _max_err(got.kinvy[n0:], ref.kinvy[n0:]) / sc['kinvy'], 'ymu': _max_err(got.ymu, ref.ymu) / sc['ymu'],
          'mu': _max_err(got.mu, ref.mu) / sc['mu'], 'var': _max_err(got.var, ref.var) / sc['var'],
          'mu_new': _max_err(got.mu[:3], ref.mu[:3]) / sc['mu'], 'var_new': _max_err(got.var[:3], ref.var[:3]) / sc['var']}


def relative_bounds(fresh, dtype):
  """The bound of the drift and fp32 cases per part, from array_errors() of the device's fresh factorisation of the same data in the
  same dtype: a fresh factorisation has no appended part, its error level is that of the whole array."""
  eps = float(np.finfo(dtype).eps)
  return {part: REL_FACTOR * fresh[arr] + FLOOR_C * eps for part, arr in PART_OF.items()}


# ---- the device's recurrences restated, and their mutants ------------------------------------------------------------------------
MUTANTS = {
    'alpha_old': 'alpha[:n] is not updated',
    'z': 'z[n] is not stored: a later row reads a z that was never extended',
    'w_sign': 'row n of W without the minus sign',
    'w_no_div': 'row n of W without the division by d',
    'l_128': 'l = W k(X, x*) from the first 128 rows of W only',
    'wtl_512': 'W^T l without the rows from 512 on (the second 512-row chunk)',
    'col0': 'several target columns: column 0 of the new targets used for every column',
    'resid': 'resid[n] is not stored',
    'feat_row': 'the new row (its features) written at row n - 128',
}


def not_applicable(case):
  """Mutants whose failure cannot exist at the case's shape, by the shape alone."""
  na = set()
  if case.n_total - case.n0 < 2:
    na.add('z')            # no later row
  if case.n_total - 1 <= 512:
    na.add('wtl_512')      # no row of W beyond 512 is read (the last appended row reads rows < n_total - 1)
  if case.mcols < 2:
    na.add('col0')
  return na


@functools.lru_cache(maxsize=None)
def _start(case):
  """L, W = L^-1, z = L^-1 (y - mu), alpha, resid of the first factorisation."""
  st = initial(case)
  W = spla.solve_triangular(st.chol, np.eye(case.n0), lower=True, check_finite=False)
  z = spla.solve_triangular(st.chol, st.ymu, lower=True, check_finite=False)
  return st.chol, np.tril(W), z


def restate(case, mutant=None):
  """One State per call, by the recurrences of append_row_kernel:
       l = W k(X, x*),  wl = W^T l,  d = sqrt(k(x*, x*) + noise + eps - l.l),  row n of L = [l, d],  row n of W = [-wl / d, 1 / d],
       per column a:  z_a[n] = (y*_a - mu(x*) - l.z_a) / d,  alpha_a[:n] += W[n, :n] z_a[n],  alpha_a[n] = z_a[n] / d,  resid_a[n] = y*_a - mu(x*)
     and the posterior the device forms from them: mu = k(X, xq)^T alpha + m(xq), var = k(xq, xq) - |W k(X, xq)|^2 (+ noise)."""
  assert mutant is None or mutant in MUTANTS
  s = oracle_setup(case)
  N, m, n0 = case.n_total, case.mcols, case.n0
  chol0, W0, z0 = _start(case)
  X = np.zeros((N, case.d)); X[:n0] = s.x[:n0]
  L, W = np.zeros((N, N)), np.zeros((N, N))
  L[:n0, :n0], W[:n0, :n0] = chol0, W0
  z, alpha, resid = np.zeros((m, N)), np.zeros((m, N)), np.zeros((m, N))
  z[:, :n0], alpha[:, :n0], resid[:, :n0] = z0.T, initial(case).kinvy.T, initial(case).ymu.T
  mu_q = np.asarray(s.mo(s.po, s.xq, warp_func=WFO), dtype=np.float64)[:, 0]
  kd_q = np.asarray(s.ko(s.po, s.xq, warp_func=WFO, diag=True), dtype=np.float64)
  out = []
  for n_before, n_after in case.sizes:
    for n in range(n_before, n_after):
      xs, ys = s.x[n:n + 1], s.y[n]
      X[n - TILE if mutant == 'feat_row' else n] = xs[0]
      kx = np.asarray(s.ko(s.po, X[:n], xs, warp_func=WFO), dtype=np.float64)[:, 0]
      kd = float(np.asarray(s.ko(s.po, xs, warp_func=WFO, diag=True))[0])
      mu_new = float(np.asarray(s.mo(s.po, xs, warp_func=WFO))[0, 0])
      Wn = W[:n, :n]
      l = Wn @ kx
      if mutant == 'l_128':
        l[TILE:] = 0.0
      wl = Wn[:512].T @ l[:512] if mutant == 'wtl_512' else Wn.T @ l
      d = np.sqrt(kd + s.noise + EPS - l @ l)
      L[n, :n], L[n, n] = l, d
      W[n, :n] = wl / d if mutant == 'w_sign' else (-wl if mutant == 'w_no_div' else -wl / d)
      W[n, n] = 1.0 / d
      for a in range(m):
        r_new = ys[0 if mutant == 'col0' else a] - mu_new
        zn = (r_new - l @ z[a, :n]) / d
        if mutant != 'alpha_old':
          alpha[a, :n] += (-wl / d) * zn
        alpha[a, n] = zn / d
        if mutant != 'z':
          z[a, n] = zn
        if mutant != 'resid':
          resid[a, n] = r_new
    n = n_after
    kxq = np.asarray(s.ko(s.po, X[:n], s.xq, warp_func=WFO), dtype=np.float64)
    v = W[:n, :n] @ kxq
    out.append(State(n, L[:n, :n].copy(), alpha[:, :n].T.copy(), resid[:, :n].T.copy(), kxq.T @ alpha[0, :n] + mu_q,
                     kd_q - np.sum(v * v, axis=0) + s.noise))
  return out


@functools.lru_cache(maxsize=None)
def mutant_errors(case, mutant):
  """Per call, part_errors() of the mutant against the reference: how far it is from what the drift and fp32 bounds allow."""
  with np.errstate(invalid='ignore'):     # a mutant may leave a negative pivot: NaN, infinitely far from the reference
    got = restate(case, mutant)
  return [part_errors(g, r, case.n0) for g, r in zip(got, reference(case))]


def unseen_mutants(case, bounds):
  """The applicable mutants that no part after no call puts beyond `bounds` (per call: part -> bound)."""
  out = set()
  for mutant in set(MUTANTS) - not_applicable(case):
    errs = mutant_errors(case, mutant)
    if not any(e[k] > b[k] for e, b in zip(errs, bounds) for k in b):
      out.add(mutant)
  return out
