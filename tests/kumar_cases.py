"""CPU side of the Kumaraswamy tier (csrc/kumar.hip: the warp w(x) = 1 - (1 - x^a)^b of the *_kumar kernels, its a / b leaves and dw/dx).
Shared by tests/test_kumar_cases_host.py (this file judged on its own, on the CPU) and tests/test_gpu_kumar_leaves.py (the device
against it):

  element-wise        one [211, 36] grid per dtype for the test hook hbo_probe_kumar_warp: a column per (a, b) in GRID_AB^2, the rows of
                      grid_x.  elem_reference: w, dw/da, dw/db, dw/dx in mpmath (MP_DIGITS digits) at the inputs as the device sees
                      them (x, a, b rounded to the model dtype first) with the first-order term scale S of each quantity (_elem_point);
                      elem_restatement: the device's formulas in NumPy, in the dtype the device uses for each quantity;
                      elem_ratios: error over bound = REL_FACTOR x |restatement - mpmath| + FLOOR_C eps_T S, the rule of
                      pathwise_cases.bound and divergence_cases.value_bounds.  eps_T: the model dtype's for w and dw/dx; eps64 for
                      dw/da, dw/db, which kumar_dab computes in fp64 on (double) x whatever the model dtype.
  CASES               NLL + gradient.  A: every family x d in 1, 7, 8, 9, 16, 17 (both sides of the KC = 8 chunk of the contraction
                      and of the DC = 16 chunk of pt_accumulate), tasks (129, 40); B: every family, d = 9, one task of n in 1, 2,
                      127, 128, 129, 257 (the single-workgroup route up to 128, the blocked one beyond; 257: three row blocks, tiles
                      (2, 0), (2, 1)); C: every family, d = 9, one batch (257, 100, 1) (three blocks beside one: the tile slots
                      kumar_finalize_kernel must skip); D: scalar length-scale, linear mean on raw x, m = 3 target columns;
                      E: fp32 for A at d in 7, 9, 17 and for C; F: warped duplicates -- Matern, d = 1, a = 8: a third of the rows at
                      x in 0, 1e-200, 1e-60 (x^a underflows: w = 0 exactly), so u == 0 OFF the diagonal, fp64 and an fp32 twin
  reference(case)     per task: value, gradient tree with the a / b leaves, analytic: d f / d w [n, D] restated from the oracle's
                      nll_sub_dataset_value_and_grad (gmat, dk/du with its u == 0 rule, the d features expressions), contracted with
                      kumar_oracle.dw_dab, chained through squareplus_grad
  MUTANTS             changed lines of the reference (the tiled form of the contraction, kumar_contract_kernel's); mutant_ratio: how
                      many bounds of the GPU tier away a mutant lies
"""
import functools
from typing import NamedTuple, Tuple

import mpmath
import numpy as np
import scipy.linalg as spla

import helpers
import kumar_oracle as ko
from oracle import hyperbo_oracle as o

WFO = o.DEFAULT_WARP_FUNC
TILE = 128
KC = 8                      # csrc/kumar.hip: features per LDS chunk of the contraction
MP_DIGITS = 60

# ---- bounds ------------------------------------------------------------------------------------------------------------------------
REL_FACTOR = 4.0            # pathwise_cases.REL_FACTOR / divergence_cases.REL_FACTOR
FLOOR_C = 8.0               # pathwise_cases.FLOOR_C / divergence_cases.FLOOR_C
RESTATE_CAP = 8.0           # the NumPy restatement stays within RESTATE_CAP eps_T S on the grid: if not, S is wrong
FP64_VALUE_TOL = 1e-10      # per task, of |value| (tests/test_gpu_kumar.py, tests/test_gpu_parity.py)
FP32_VALUE_TOL = 2e-4
FP64_GRAD_TOL = 1e-10       # per leaf, helpers.assert_grad_close with its default floor_rel
FP32_GRAD_TOL = 2.5e-3
MUTANT_FACTOR = 10.0        # every mutant lies at least this many bounds away on a case of each tier it belongs to
AB_FD_TOL = 1e-6            # the analytic a / b leaves against central differences of the oracle value (tests/test_gpu_kumar.py)
SE_AB_TOL = 1e-13           # ... and against kumar_oracle.se_nll_ab_grad on the squared exponential

# ---- the element-wise grid ---------------------------------------------------------------------------------------------------------
GRID_AB = (0.3, 0.5, 1.0, 2.0, 3.3, 8.0)
N_UNIFORM = 200
QUANTITIES = ('w', 'da', 'db', 'dx')
# dw/dx = a b x^(a-1) (1 - x^a)^(b-1) is infinite at x = 0 where a < 1 and at x = 1 where b < 1; those entries are left out of the
# dw/dx comparison and nothing else is: one row (x = 0) in each of the 12 columns with a < 1 and one row (x = 1) in each of the 12
# columns with b < 1 -- at most 2 of the 211 rows of a column, 24 of the 7596 entries of a grid
DX_LEFT_OUT = 24


def np_dtype(dtype):
  return np.float64 if dtype == 'fp64' else np.float32


def grid_ab(dtype):
  """(raw a, raw b, warped a, warped b) per column: raw t = a - 1/a (squareplus(t) = a) in the model dtype, warped as BuiltModel warps
  (in fp64) and rounds them to the model dtype -- what the device reads."""
  dt = np_dtype(dtype)
  a0 = np.repeat(np.array(GRID_AB), len(GRID_AB)); b0 = np.tile(np.array(GRID_AB), len(GRID_AB))
  ra, rb = (a0 - 1.0 / a0).astype(dt), (b0 - 1.0 / b0).astype(dt)
  return ra, rb, ko.squareplus(ra).astype(dt), ko.squareplus(rb).astype(dt)


@functools.lru_cache(maxsize=None)
def grid_x(dtype):
  """[211, 36] in the model dtype: 11 edge rows (the same x in every column) and 200 uniform draws per column.  Not to be written to."""
  dt = np_dtype(dtype)
  tiny = np.finfo(dt).tiny
  edge = np.array([0.0, tiny, 1e-30, 1e-10, 1e-3, 0.1, 0.5, 0.9, 1 - 1e-6, np.nextafter(dt(1), dt(0)), 1.0], dtype=np.float64).astype(dt)
  rng = np.random.default_rng(211)
  ncol = len(GRID_AB) ** 2
  x = np.concatenate([np.repeat(edge[:, None], ncol, axis=1), rng.uniform(size=(N_UNIFORM, ncol)).astype(dt)], axis=0)
  x.setflags(write=False)
  return x


class ElemRef(NamedTuple):
  ref: dict                  # quantity -> [211, 36] object array of mpf (dw/dx: +inf where it is infinite)
  scale: dict                # quantity -> [211, 36] object array of mpf: S
  dx_finite: np.ndarray      # [211, 36] bool: where dw/dx is compared


def _elem_point(x, a, b, tiny):
  """(reference, S) per quantity at one point, mpmath.  S by first-order propagation through the device's formulas, every elementary
  operation with relative error eps, exp2(y) / exp(y) passing an absolute error of y on as a relative one; tau = the smallest normal
  number of the dtype a quantity is computed in (an intermediate that underflows is off by up to tau eps):
    w = 1 - v^b, u = x^a = exp2(a log2 x), v = 1 - u (kumar_w: the cancellation in 1 - u is the formula's own):
        du = u (1 + |a log2 x|) eps
        S_w = |w| + |b v^(b-1)| u (1 + |a log2 x|) + v^b (1 + |b log2 v|) + tau |b v^(b-1)|
    dw/dx = a b x^(a-1) v^(b-1) with v = -expm1(a log x) (kumar_chain_dx_kernel; a == 1: v = 1 - x):
        dv / v = (1 + 2 u |a log x| / v) eps =: V eps       (u |a log x| / v <= 1: no cancellation)
        S_dx = |dw/dx| (3 + |(a-1) log2 x| + |(b-1) log2 v| + |b-1| V) + tau (1 + a b v^(b-1))
    kumar_dab (fp64): lx = log x, u = exp(a lx): du = u (1 + 2 |a lx|) eps;  lv = log1p(-u) where u < 1/2, log(-expm1(a lx)) above:
        dlv = (|lv| + (u < 1/2 ? (u / v) (1 + 2 |a lx|) : V)) eps =: L eps
        dw/da = b exp((b-1) lv) u lx:   S_da = |dw/da| (6 + 2 |a lx| + |b-1| (|lv| + L)) + tau (1 + b v^(b-1) |lx|)
        dw/db = -exp(b lv) lv:          S_db = |dw/db| (2 + |b lv| + (b + 1 / |lv|) L) + tau (1 + v^b / v)"""
  mp = mpmath
  one, zero = mp.mpf(1), mp.mpf(0)
  tau, tau64 = mp.mpf(tiny), mp.mpf(float(np.finfo(np.float64).tiny))
  if x == 0 or x == 1:
    w = zero if x == 0 else one
    # dw/dx at the ends: x = 0: 0 (a > 1), b (a = 1), inf (a < 1); x = 1: 0 (b > 1), a (b = 1), inf (b < 1)
    p = a if x == 0 else b
    dx = zero if p > 1 else ((b if x == 0 else a) if p == 1 else mp.inf)
    return {'w': (w, w), 'da': (zero, zero), 'db': (zero, zero), 'dx': (dx, abs(dx) * 3 if p >= 1 else zero)}
  l2x, lx = mp.log(x, 2), mp.log(x)
  u = x if a == 1 else mp.power(x, a)
  v = one - x if a == 1 else -mp.expm1(a * lx)
  lv = mp.log1p(-u)           # (x^a below 1e-60 must not round v to 1)
  l2v = lv / mp.log(2)
  vb, vb1 = mp.exp(b * lv), mp.exp((b - 1) * lv)
  w = u if b == 1 else -mp.expm1(b * lv)
  s_w = abs(w) + abs(b * vb1) * u * (1 + abs(a * l2x)) + vb * (1 + abs(b * l2v)) + tau * abs(b * vb1)
  dx = a * b * mp.power(x, a - 1) * vb1
  big_v = 1 + 2 * u * abs(a * lx) / v
  s_dx = abs(dx) * (3 + abs((a - 1) * l2x) + abs((b - 1) * l2v) + abs(b - 1) * big_v) + tau * (1 + a * b * vb1)
  big_l = abs(lv) + ((u / v) * (1 + 2 * abs(a * lx)) if u < 0.5 else big_v)
  da = b * vb1 * u * lx
  s_da = abs(da) * (6 + 2 * abs(a * lx) + abs(b - 1) * (abs(lv) + big_l)) + tau64 * (1 + b * vb1 * abs(lx))
  db = -vb * lv
  s_db = abs(db) * (2 + abs(b * lv) + (b + 1 / abs(lv)) * big_l) + tau64 * (1 + vb / v)
  return {'w': (w, s_w), 'da': (da, s_da), 'db': (db, s_db), 'dx': (dx, s_dx)}


@functools.lru_cache(maxsize=None)
def elem_reference(dtype):
  """Shared and not to be written to."""
  x = grid_x(dtype)
  _, _, a, b = grid_ab(dtype)
  ref = {q: np.empty(x.shape, dtype=object) for q in QUANTITIES}
  scale = {q: np.empty(x.shape, dtype=object) for q in QUANTITIES}
  tiny = float(np.finfo(np_dtype(dtype)).tiny)
  with mpmath.workdps(MP_DIGITS):
    for j in range(x.shape[1]):
      aj, bj = mpmath.mpf(float(a[j])), mpmath.mpf(float(b[j]))
      for i in range(x.shape[0]):
        pt = _elem_point(mpmath.mpf(float(x[i, j])), aj, bj, tiny)
        for q in QUANTITIES:
          ref[q][i, j], scale[q][i, j] = pt[q]
  finite = np.array([[mpmath.isfinite(v) for v in row] for row in ref['dx']], dtype=bool)
  return ElemRef(ref, scale, finite)


def elem_eps(dtype, q):
  return float(np.finfo(np_dtype(dtype) if q in ('w', 'dx') else np.float64).eps)


def elem_restatement(dtype):
  """The device's formulas (csrc/kumar.hip: kpow, kumar_w, kumar_dab, kumar_chain_dx_kernel) in NumPy: w and dw/dx in the model dtype,
  dw/da and dw/db in fp64 on (double) x, with the shortcuts and guards of the device."""
  dt = np_dtype(dtype)
  x = grid_x(dtype)
  _, _, a, b = grid_ab(dtype)
  a, b = np.broadcast_to(a, x.shape), np.broadcast_to(b, x.shape)

  def kpow(xv, p):
    with np.errstate(divide='ignore', invalid='ignore', under='ignore', over='ignore'):
      r = np.exp2(p * np.log2(xv))
    r = np.where(p == 1, xv, np.where(p == 0, dt(1), r))
    assert r.dtype == dt
    return r

  u = kpow(x, a)
  w = np.where(b == 1, u, dt(1) - kpow(dt(1) - u, b))
  with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
    v = np.where(a == 1, dt(1) - x, dt(0) - np.expm1(a * np.log(x)))
    dx = a * b * kpow(x, a - dt(1)) * kpow(v, b - dt(1))
  assert w.dtype == dt and dx.dtype == dt
  x64, a64, b64 = x.astype(np.float64), a.astype(np.float64), b.astype(np.float64)
  with np.errstate(divide='ignore', invalid='ignore', under='ignore'):
    lx = np.log(x64)
    u64 = np.where(a64 == 1, x64, np.exp(a64 * lx))
    lv = np.where(u64 < 0.5, np.log1p(-u64), np.log(np.where(a64 == 1, 1.0 - x64, 0.0 - np.expm1(a64 * lx))))
    vb1 = np.where(b64 == 1, 1.0, np.exp((b64 - 1.0) * lv))
    da = b64 * vb1 * u64 * lx
    db = -np.exp(b64 * lv) * lv
  dead = (x64 == 0) | (x64 == 1) | (lv == -np.inf)
  return {'w': w, 'da': np.where(dead, 0.0, da), 'db': np.where(dead, 0.0, db), 'dx': dx.astype(np.float64)}


def elem_errors(dtype, got):
  """quantity -> [211, 36] object array of mpf: |got - reference| (dw/dx: 0 where it is left out).  got: quantity -> array."""
  er = elem_reference(dtype)
  out = {}
  with mpmath.workdps(MP_DIGITS):
    for q in QUANTITIES:
      g = np.asarray(got[q])
      assert g.shape == er.ref[q].shape, (q, g.shape)
      e = np.empty(g.shape, dtype=object)
      for idx in np.ndindex(g.shape):
        if q == 'dx' and not er.dx_finite[idx]:
          e[idx] = mpmath.mpf(0)
        else:
          gv = float(g[idx])
          e[idx] = abs(mpmath.mpf(gv) - er.ref[q][idx]) if np.isfinite(gv) else mpmath.inf
      out[q] = e
  return out


@functools.lru_cache(maxsize=None)
def elem_restatement_errors(dtype):
  return elem_errors(dtype, elem_restatement(dtype))


def _worst(num, den):
  """max over the grid of num / den (mpf object arrays), 0 / 0 = 0; and where."""
  worst, at = 0.0, None
  for idx in np.ndindex(num.shape):
    n_, d_ = num[idx], den[idx]
    r = 0.0 if n_ == 0 else (float('inf') if d_ == 0 else float(n_ / d_))
    if r > worst:
      worst, at = r, idx
  return worst, at


def elem_restatement_ratios(dtype):
  """quantity -> (worst |restatement - mpmath| / (eps_T S), its grid index): the check of S."""
  er, err = elem_reference(dtype), elem_restatement_errors(dtype)
  with mpmath.workdps(MP_DIGITS):
    return {q: _worst(err[q], er.scale[q] * mpmath.mpf(elem_eps(dtype, q))) for q in QUANTITIES}


def elem_ratios(dtype, got):
  """quantity -> (worst |got - mpmath| / bound, its grid index) with bound = REL_FACTOR |restatement - mpmath| + FLOOR_C eps_T S."""
  er, rest, err = elem_reference(dtype), elem_restatement_errors(dtype), elem_errors(dtype, got)
  with mpmath.workdps(MP_DIGITS):
    return {q: _worst(err[q], rest[q] * mpmath.mpf(REL_FACTOR) + er.scale[q] * mpmath.mpf(FLOOR_C * elem_eps(dtype, q))) for q in QUANTITIES}


def elem_mutant(dtype, mutant):
  """The restatement with one line changed: 'vb_for_vb1' (v^b for v^(b-1) in dw/da), 'h_fp32' (dw/da, dw/db rounded to fp32)."""
  got = dict(elem_restatement(dtype))
  if mutant == 'h_fp32':
    got['da'], got['db'] = got['da'].astype(np.float32).astype(np.float64), got['db'].astype(np.float32).astype(np.float64)
  elif mutant == 'vb_for_vb1':
    x = grid_x(dtype).astype(np.float64)
    _, _, a, b = grid_ab(dtype)
    da, _ = dw_dab_mutant(x, a.astype(np.float64), b.astype(np.float64), mutant)
    got['da'] = da
  else:
    raise ValueError(mutant)
  return got


# ---- the NLL cases -----------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
  group: str                 # 'A' .. 'F'
  kname: str                 # the base kernel
  d: int
  tasks: Tuple[int, ...]     # n of every task, in the dataset's order
  dtype: str = 'fp64'
  ls: str = 'ard'            # 'ard' | 'scalar' (n_ls == 1)
  mname: str = 'constant'
  m: int = 1                 # target columns

  @property
  def data_id(self):
    return f'{self.group}-{self.kname}-d{self.d}-' + '_'.join(str(n) for n in self.tasks) + f'-{self.ls}-{self.mname}-m{self.m}'

  @property
  def id(self):
    return f'{self.data_id}-{self.dtype}'

  @property
  def np_dtype(self):
    return np_dtype(self.dtype)

  @property
  def grad_tol(self):
    return FP64_GRAD_TOL if self.dtype == 'fp64' else FP32_GRAD_TOL

  @property
  def value_tol(self):
    return FP64_VALUE_TOL if self.dtype == 'fp64' else FP32_VALUE_TOL


A_D = (1, 7, 8, 9, 16, 17)
A_TASKS = (129, 40)
B_N = (1, 2, 127, 128, 129, 257)
C_TASKS = (257, 100, 1)
E_D = (7, 9, 17)
F_N = (40, 140)
GROUP_A = [Case('A', k, d, A_TASKS) for k in helpers.KERNELS for d in A_D]
GROUP_B = [Case('B', k, 9, (n,)) for k in helpers.KERNELS for n in B_N]
GROUP_C = [Case('C', k, 9, C_TASKS) for k in helpers.KERNELS]
# (the dot product has no length-scale: its scalar-length-scale case does not exist)
GROUP_D = ([Case('D', 'matern52', 9, A_TASKS, ls='scalar'), Case('D', 'matern52', 9, A_TASKS, mname='linear'), Case('D', 'matern52', 9, A_TASKS, m=3),
            Case('D', 'dot_product', 9, A_TASKS, mname='linear'), Case('D', 'dot_product', 9, A_TASKS, m=3)])
GROUP_E = ([c._replace(group='E', dtype='fp32') for c in GROUP_A if c.d in E_D] + [c._replace(group='E', dtype='fp32') for c in GROUP_C])
GROUP_F = [Case('F', k, 1, (n,), dtype) for k in ('matern32', 'matern52') for n in F_N for dtype in ('fp64', 'fp32')]
CASES = GROUP_A + GROUP_B + GROUP_C + GROUP_D + GROUP_E + GROUP_F
GROUPS = {'A': GROUP_A, 'B': GROUP_B, 'C': GROUP_C, 'D': GROUP_D, 'E': GROUP_E, 'F': GROUP_F}
F_TINY = {'fp64': (0.0, 1e-200, 1e-60), 'fp32': (0.0, 1e-30, 1e-20)}     # x^8 underflows in the dtype: w = 0 exactly
F_A, F_B = 8.0, 2.0         # group F: warped a, b (raw 7.875 and 1.5: squareplus is exact on both, in fp32 too)


def cast(tree, dtype):
  return {k: cast(v, dtype) for k, v in tree.items()} if isinstance(tree, dict) else np.asarray(tree, dtype=dtype)


class Inputs(NamedTuple):
  model: dict                # raw params.model in the case's dtype, 'kumar_params' included
  tasks: tuple               # ((x [n, d], y [n, m]), ...) in the case's dtype


def planted_x(rng, n, d):
  """_x of tests/test_gpu_kumar.py: uniform rows with zeros and ones planted."""
  x = rng.uniform(size=(n, d))
  x.flat[::7] = 0.0
  x.flat[3::11] = 1.0
  return x


def _f_x(rng, n, dtype):
  """Group F, d = 1: a third of the rows at F_TINY, two rows at nextafter(1, 0), two at 1, the rest uniform; shuffled."""
  dt = np_dtype(dtype)
  x = rng.uniform(0.05, 0.95, size=n)
  k = n // 3
  x[:k] = np.resize(np.array(F_TINY[dtype]), k)
  x[k:k + 2] = float(np.nextafter(dt(1), dt(0)))
  x[k + 2:k + 4] = 1.0
  return rng.permutation(x)[:, None]


@functools.lru_cache(maxsize=None)
def inputs(case):
  """The case's model and tasks in its dtype, seeded by the case's id without the dtype (fp32 sees the fp64 numbers rounded once, here;
  group F: the tiny rows are the dtype's own).  Shared and not to be written to."""
  rng = np.random.default_rng([ord(ch) for ch in case.data_id])
  model = helpers.make_model(rng, case.mname, False, case.d)
  model['kumar_params'] = {'a': rng.uniform(-1.5, 1.5, size=case.d), 'b': rng.uniform(-1.5, 1.5, size=case.d)}
  if case.ls == 'scalar':
    model['lengthscale'] = model['lengthscale'][:1]
  if case.group == 'F':
    model['kumar_params'] = {'a': np.array([F_A - 1 / F_A]), 'b': np.array([F_B - 1 / F_B])}
  tasks = []
  for n in case.tasks:
    x = _f_x(rng, n, case.dtype) if case.group == 'F' else planted_x(rng, n, case.d)
    y = np.sin(3 * rng.uniform(size=(n, case.m)))
    tasks.append((x, y))
  dt = case.np_dtype
  return Inputs(cast(model, dt), tuple((np.ascontiguousarray(x, dtype=dt), np.ascontiguousarray(y, dtype=dt)) for x, y in tasks))


def warped_ab(case):
  """(a, b) as the device reads them: squareplus of the raw leaves (in fp64), rounded to the model dtype; as fp64 arrays."""
  kp = inputs(case).model['kumar_params']
  dt = case.np_dtype
  return (ko.squareplus(np.asarray(kp['a'], dtype=np.float64)).astype(dt).astype(np.float64),
          ko.squareplus(np.asarray(kp['b'], dtype=np.float64)).astype(dt).astype(np.float64))


# ---- the analytic reference ----------------------------------------------------------------------------------------------------------
MUTANTS = {
    'no_col_term': 'the column-side term h_j dropped on the off-diagonal tiles',
    'drop_last_chunk': 'the last KC = 8 chunk of features dropped (d >= 9)',
    'dkdu_unguarded': "Matern: dk/du = (dk/dr) (dr/du) without the u == 0 rule off the diagonal (0 x inf)",
    'vb_for_vb1': 'v^b for v^(b-1) in dw/da',
    'cd_2': 'c_d = 2 / ls_d for 4 / ls_d',
    'drop_slot2': 'the second lower tile, (1, 0), of a three-block task left out of the sum over its partials',
    'h_fp32': 'dw/da, dw/db rounded to fp32',
}
MUTANT_TIERS = {m: (('fp64',) if m == 'h_fp32' else ('fp64', 'fp32')) for m in MUTANTS}     # fp32 rounding of h is inside the fp32 bound


def applicable(case, mutant):
  """By the shapes alone: whether the mutant can differ from the reference on this case."""
  return {'no_col_term': max(case.tasks) > TILE, 'drop_last_chunk': case.d >= KC + 1,
          'dkdu_unguarded': case.kname in ('matern32', 'matern52'), 'vb_for_vb1': True, 'cd_2': case.kname != 'dot_product',
          'drop_slot2': any(2 * TILE < n <= 3 * TILE for n in case.tasks), 'h_fp32': True}[mutant]


def dw_dab_mutant(x, a, b, mutant=None):
  da, db = ko.dw_dab(x, a, b)
  if mutant == 'vb_for_vb1':
    inner = (x > 0) & (x < 1)
    xs = np.where(inner, x, 0.5)
    u = xs ** a
    da = np.where(inner, b * (1.0 - u) ** b * u * np.log(xs), 0.0)
  if mutant == 'h_fp32':
    da, db = da.astype(np.float32).astype(np.float64), db.astype(np.float32).astype(np.float64)
  return da, db


def df_dw_from(kname, gk, w, par):
  """d f / d w [n, D] from gk = (d f / d K) dk/du (dot product: d f / d K itself, symmetric) and par = ls [D] (dot product: sigma):
  the d features expressions of the oracle's backward passes."""
  if kname == 'dot_product':
    return 2.0 * (gk @ w) / par ** 2
  return 4.0 * np.einsum('ij,ijd->id', gk, w[:, None, :] - w[None, :, :]) / par ** 2


def kernel_dk_du(kname, model, w):
  """(dk/du [n, n] of the base kernel on the features w, 0 where u == 0 for Matern -- None for the dot product --, ls [D] or sigma).
  model: raw params.model."""
  warped = lambda key: np.asarray(WFO[key](np.asarray(model[key], dtype=np.float64)), dtype=np.float64)
  if kname == 'dot_product':
    return None, float(warped('dot_prod_sigma'))
  ls = np.broadcast_to(warped('lengthscale').reshape(-1), (w.shape[1],))
  sv = float(warped('signal_variance'))
  u = np.sum(((w[:, None, :] - w[None, :, :]) / ls) ** 2, axis=-1)
  if kname == 'squared_exponential':
    return -0.5 * sv * np.exp(-u / 2), ls
  c = 3.0 if kname == 'matern32' else 5.0
  rr = np.sqrt(c * u)
  return np.where(u == 0, 0.0, -sv * c * np.exp(-rr) / 2 * (1.0 if kname == 'matern32' else (1 + rr) / 3)), ls


def ab_from_adjoint(kname, model, x, gmat):
  """d f / d (raw a, raw b) of one task of ANY objective whose kernel adjoint d f / d K = gmat (symmetric) is known: the kernel on
  w(x) with the raw kumar_params of `model` (fp64), contracted with kumar_oracle.dw_dab and chained through squareplus_grad."""
  kp = model['kumar_params']
  ra, rb = np.asarray(kp['a'], dtype=np.float64), np.asarray(kp['b'], dtype=np.float64)
  a, b = ko.squareplus(ra), ko.squareplus(rb)
  x = np.asarray(x, dtype=np.float64)
  w = 1.0 - (1.0 - x ** a) ** b
  dk_du, par = kernel_dk_du(kname, model, w)
  dfw = df_dw_from(kname, gmat if dk_du is None else gmat * dk_du, w, par)
  ha, hb = ko.dw_dab(x, a, b)
  return {'a': np.sum(dfw * ha, axis=0) * ko.squareplus_grad(ra), 'b': np.sum(dfw * hb, axis=0) * ko.squareplus_grad(rb)}


def ab_tiled(kname, gk, w, par, ha, hb, mutant=None):
  """[2, D]: d f / d (warped a, b) of one task in kumar_contract_kernel's form -- per lower 128-tile (ti, tj)
       SE / Matern: c_d sum_ij g_ij (fs_i - fs_j)_d (h_i - [off-diagonal] h_j)_d,   c_d = 4 / ls_d, fs = w / ls, g = G dk/du
       dot:         c_d sum_ij G_ij (w_j h_i + [off-diagonal] w_i h_j)_d,           c_d = 2 / sigma^2
  summed over the tiles.  par: ls [D] or sigma."""
  n, dim = w.shape
  nblk = -(-n // TILE)
  dot = kname == 'dot_product'
  out = np.zeros((2, dim))
  cd = np.full(dim, 2.0 / par ** 2) if dot else (2.0 if mutant == 'cd_2' else 4.0) / par
  fs = w if dot else w / par
  for ti in range(nblk):
    for tj in range(ti + 1):
      if mutant == 'drop_slot2' and nblk == 3 and (ti, tj) == (1, 0):
        continue
      ri, rj = slice(ti * TILE, min(n, (ti + 1) * TILE)), slice(tj * TILE, min(n, (tj + 1) * TILE))
      g = gk[ri, rj]
      col = ti != tj and mutant != 'no_col_term'
      for k, h in enumerate((ha, hb)):
        if dot:
          t = np.einsum('ij,jd,id->d', g, fs[rj], h[ri])
          if col:
            t = t + np.einsum('ij,id,jd->d', g, fs[ri], h[rj])
        else:
          hd = h[ri][:, None, :] - (h[rj][None, :, :] if col else 0.0)
          t = np.einsum('ij,ijd,ijd->d', g, fs[ri][:, None, :] - fs[rj][None, :, :], hd)
        out[k] += cd * t
  if mutant == 'drop_last_chunk' and dim >= KC + 1:
    out[:, KC * ((dim - 1) // KC):] = 0.0
  return out


class TaskRef(NamedTuple):
  value: float
  grad: dict                 # d value / d raw params.model, the a / b leaves included
  ab_scale: dict             # 'a' / 'b' -> [D]: sum_i |d f / d w_id  dw_id / da_d| squareplus'(raw): the un-cancelled terms of the leaf
  u_zero_offdiag: int        # entries off the diagonal of the reference Gram with u == 0 (0 for the dot product)
  min_eig: float             # smallest eigenvalue of K + (noise + jitter) I


def task_reference(kname, mname, model, a, b, x, y, mutant=None):
  """One task: the Cholesky NLL of oracle.nll_sub_dataset_value_and_grad with the kernel on w(x) and the mean on x, and its gradient,
  fp64.  model: raw params.model; a, b: the warped Kumaraswamy parameters.  The lines of the oracle, restated: gmat = 1/2 (m^2 K^-1 -
  s s^T), dk/du with 0 where u == 0 (Matern), d f / d w = 4 sum_j (gmat dk/du)_ij (w_i - w_j) / ls^2 (dot: 2 gmat w / sigma^2)."""
  model = cast(model, np.float64)
  x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
  n, m = y.shape
  dim = x.shape[1]
  w = 1.0 - (1.0 - x ** a) ** b
  warped = lambda key: np.asarray(WFO[key](model[key]) if key in WFO else model[key], dtype=np.float64)
  chain = lambda key, g: np.reshape(np.asarray(g) * o.warp_derivative(WFO[key], model[key]) if key in WFO else np.asarray(g), np.shape(model[key]))
  if mname == 'constant':
    mu = np.full((n, 1), float(warped('constant')))
  elif mname == 'linear':
    mu = x @ model['linear_mean']['kernel'] + model['linear_mean']['bias']
  else:
    raise ValueError(mname)
  r = y - mu
  noise = float(warped('noise_variance'))
  u_zero = 0
  if kname == 'dot_product':
    sigma, bias = float(warped('dot_prod_sigma')), float(warped('dot_prod_bias'))
    dots = w @ w.T
    kmat = dots / sigma ** 2 + bias ** 2
  else:
    ls = np.broadcast_to(warped('lengthscale').reshape(-1), (dim,))
    sv = float(warped('signal_variance'))
    diff = w[:, None, :] - w[None, :, :]
    u = np.sum((diff / ls) ** 2, axis=-1)
    off = ~np.eye(n, dtype=bool)
    u_zero = int(np.sum((u == 0) & off))
    if kname == 'squared_exponential':
      kmat = sv * np.exp(-u / 2); dk_du = -0.5 * kmat
    else:
      c = 3.0 if kname == 'matern32' else 5.0
      rr = np.sqrt(c * u)
      kmat = sv * ((1 + rr) if kname == 'matern32' else (1 + rr + rr ** 2 / 3)) * np.exp(-rr)
      if mutant == 'dkdu_unguarded':
        with np.errstate(divide='ignore', invalid='ignore'):
          dk_dr = -sv * rr * np.exp(-rr) * (1.0 if kname == 'matern32' else (1 + rr) / 3)
          dk_du = np.where(off, dk_dr * (c / (2 * rr)), 0.0)
      else:
        dk_du = np.where(u == 0, 0.0, -sv * c * np.exp(-rr) / 2 * (1.0 if kname == 'matern32' else (1 + rr) / 3))
  cov = kmat + np.eye(n) * (noise + 1e-6)
  chol = spla.cholesky(cov, lower=True)
  alpha = spla.cho_solve((chol, True), r)
  s = alpha.sum(axis=1, keepdims=True)
  value = float(0.5 * np.sum(r.T @ alpha) + m * m * (np.sum(np.log(np.diag(chol))) + 0.5 * n * np.log(2 * np.pi)))
  kinv = spla.cho_solve((chol, True), np.eye(n))
  gmat = 0.5 * (m * m * kinv - s @ s.T)
  dmu = -m * s
  grad = o._tree_zeros_like(model)
  grad['noise_variance'] = chain('noise_variance', np.trace(gmat))
  if kname == 'dot_product':
    grad['dot_prod_sigma'] = chain('dot_prod_sigma', np.sum(gmat * dots) * (-2.0 / sigma ** 3))
    grad['dot_prod_bias'] = chain('dot_prod_bias', np.sum(gmat) * 2.0 * bias)
    gk, par = gmat, sigma
    dfw = df_dw_from(kname, gk, w, par)
  else:
    grad['signal_variance'] = chain('signal_variance', np.sum(gmat * kmat) / sv)
    gk, par = gmat * dk_du, ls
    per_dim = np.einsum('ij,ijd->d', gk, diff ** 2) * (-2.0 / ls ** 3)
    grad['lengthscale'] = chain('lengthscale', np.sum(per_dim) if np.size(model['lengthscale']) == 1 else per_dim)
    dfw = df_dw_from(kname, gk, w, par)
  if mname == 'constant':
    grad['constant'] = chain('constant', np.sum(dmu))
  else:
    grad['linear_mean'] = {'kernel': (x.T @ dmu).reshape(np.shape(model['linear_mean']['kernel'])),
                           'bias': np.sum(dmu, axis=0).reshape(np.shape(model['linear_mean']['bias']))}
  ha, hb = dw_dab_mutant(x, a, b, mutant)
  kp = model['kumar_params']
  spa, spb = ko.squareplus_grad(kp['a']), ko.squareplus_grad(kp['b'])
  if mutant in (None, 'vb_for_vb1', 'h_fp32', 'dkdu_unguarded'):
    ga, gb = np.sum(dfw * ha, axis=0), np.sum(dfw * hb, axis=0)
  else:
    ga, gb = ab_tiled(kname, gk, w, par, ha, hb, mutant)
  grad['kumar_params'] = {'a': np.reshape(ga * spa, np.shape(kp['a'])), 'b': np.reshape(gb * spb, np.shape(kp['b']))}
  scale = {'a': np.sum(np.abs(dfw * ha), axis=0) * spa, 'b': np.sum(np.abs(dfw * hb), axis=0) * spb}
  return TaskRef(value, grad, scale, u_zero, float(np.linalg.eigvalsh(cov)[0]))


def tree_sum(trees):
  out = trees[0]
  for t in trees[1:]:
    out = o._tree_add(out, t)
  return out


class Ref(NamedTuple):
  tasks: tuple               # TaskRef per task
  value: float               # the mean over the tasks: what objectives.nll_value_and_grad returns
  grad: dict                 # the mean over the tasks
  leaf_scales: dict          # 'kumar_params/a', 'kumar_params/b' -> the largest element of the leaf's un-cancelled terms (mean over the tasks)


def _reference_of(case, mutant=None):
  inp = inputs(case)
  a, b = warped_ab(case)
  tasks = tuple(task_reference(case.kname, case.mname, inp.model, a, b, x, y, mutant) for x, y in inp.tasks)
  t = len(tasks)
  scales = {f'kumar_params/{k}': float(np.max(sum(tr.ab_scale[k] for tr in tasks))) / t for k in ('a', 'b')}
  return Ref(tasks, sum(tr.value for tr in tasks) / t, o._tree_scale(tree_sum([tr.grad for tr in tasks]), 1.0 / t), scales)


@functools.lru_cache(maxsize=None)
def reference(case):
  """Shared and not to be written to."""
  return _reference_of(case)


def grad_ratio(got, ref, tol, leaf_scales=None, floor_rel=1e-3):
  """The worst leaf's error over its bound by the rule of helpers.assert_grad_close (anything not finite: inf), and that leaf."""
  gl, rl = dict(helpers.tree_leaves(got)), dict(helpers.tree_leaves(ref))
  assert set(gl) == set(rl)
  gmax = max((float(np.max(np.abs(r))) for r in rl.values() if r.size), default=0.0)
  worst, leaf = 0.0, ''
  for path, r in rl.items():
    if not r.size:
      continue
    err, nrm = float(np.max(np.abs(gl[path].ravel() - r.ravel()))), float(np.max(np.abs(r)))
    floor = floor_rel * gmax
    if leaf_scales is not None and path in leaf_scales:
      floor = min(floor, leaf_scales[path])
    ratio = err / (tol * max(nrm, floor, 1e-300)) if np.isfinite(err) else np.inf
    if ratio > worst:
      worst, leaf = ratio, path
  return worst, leaf


def mutant_ratio(case, mutant):
  """How many bounds of the GPU tier the mutant's gradient lies from the reference's: the worst leaf."""
  ref = reference(case)
  return grad_ratio(_reference_of(case, mutant).grad, ref.grad, case.grad_tol, ref.leaf_scales)[0]


# ---- d acquisition / d x ---------------------------------------------------------------------------------------------------------------
ACQ_D, ACQ_N, ACQ_Q = 9, 150, 12


@functools.lru_cache(maxsize=None)
def acq_inputs(kname):
  """(model, x [150, 9], y, x_other, y_other, xq [12, 9]): raw a, b > 0 (warped a, b > 1) in columns 0..3, where four of the queries sit
  at x = 0 and four at x = 1; the other queries are interior.  Shared and not to be written to."""
  rng = np.random.default_rng([ord(ch) for ch in 'acq-' + kname])
  model = helpers.make_model(rng, 'constant', False, ACQ_D)
  a, b = rng.uniform(-1.5, 1.5, size=ACQ_D), rng.uniform(-1.5, 1.5, size=ACQ_D)
  a[:4], b[:4] = np.abs(a[:4]) + 0.1, np.abs(b[:4]) + 0.1
  model['kumar_params'] = {'a': a, 'b': b}
  x, y = planted_x(rng, ACQ_N, ACQ_D), np.sin(3 * rng.uniform(size=(ACQ_N, 1)))
  xo, yo = planted_x(rng, 40, ACQ_D), np.sin(3 * rng.uniform(size=(40, 1)))
  xq = rng.uniform(0.05, 0.95, size=(ACQ_Q, ACQ_D))
  for q in range(4):
    xq[q, q] = 0.0
    xq[4 + q, q] = 1.0
  xq[8, :4] = (0.0, 1.0, 0.0, 1.0)
  return model, x, y, xo, yo, xq
