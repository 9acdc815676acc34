"""CPU side of the tests of hbo_acq_maximize (csrc/acq_opt_ctl.h, csrc/acq_opt.hip): a NumPy restatement of the projected L-BFGS of
DESIGN.md section 6, operation by operation (dot products as the 256-partial tree, sums over samples in sample order, no fused
multiply-adds), driven by any value_and_grad(x) -> (vals [S], grads [S, D]); the case list; and the oracle's value and gradient
(oracle/hyperbo_oracle.py: acquisition_value_and_grad per parameter sample) to drive it with.  Shared by tests/test_acq_opt_host.py
and tests/test_gpu_acq_opt.py.

The restatement knows four mutants (MUTANTS), each one rule of the algorithm left out; test_acq_opt_host.py asserts that the case list
catches every one of them."""
import functools
from typing import NamedTuple

import numpy as np

import helpers
from oracle import hyperbo_oracle as o

WFO = o.DEFAULT_WARP_FUNC
SCALE = 1.5
ACQ_IDS = {'ei': 0, 'pi': 1, 'ucb': 2}
START, MAIN, LINE_SEARCH, IDLE = 0, 1, 2, 3
RUNNING, CONVERGED, FTOL, NO_PROGRESS, NONFINITE_AT_START, STEPS_DONE = range(6)
DEFAULTS = dict(memory=10, ls_steps=20, max_iters=200, c1=1e-4, tau=0.5, pgtol=1e-5, ftol=2.2e-9)
MUTANTS = ('no_projection', 'active_set_ignored', 'armijo_unprojected', 'pairs_never_skipped')
MAX_EVALS = 128


def tree_dot(a, b):
  """hbo_lbfgs_dot: 256 strided partial sums in rising index, then p[j] += p[j + s] for s = 128 .. 1."""
  a = np.asarray(a, dtype=np.float64).ravel()
  prod = np.zeros(-(-a.size // 256) * 256)
  prod[:a.size] = a * np.asarray(b, dtype=np.float64).ravel()
  acc = np.zeros(256)
  for row in prod.reshape(-1, 256):
    acc = acc + row
  s = 128
  while s:
    acc[:s] = acc[:s] + acc[s:2 * s]
    s //= 2
  return float(acc[0])


def reduce_samples(vals, grads):
  """f and its gradient from the per-sample acquisition values [S] and gradients [S, D]: sums in sample order, / S, negated."""
  vals, grads = np.asarray(vals, dtype=np.float64), np.asarray(grads, dtype=np.float64)
  s_count = vals.shape[0]
  sv, sg = 0.0, np.zeros(grads.shape[1])
  for s in range(s_count):
    sv = sv + float(vals[s])
    sg = sg + grads[s]
  return -(sv / s_count), -(sg / s_count)


def pg_measure(x, g, lo, hi):
  """SciPy's projected-gradient measure max_i |clip(x_i - g_i, lo_i, hi_i) - x_i| (0 for an all-NaN vector, as the device's maximum)."""
  w = np.abs(np.clip(x - g, lo, hi) - x)
  return float(np.fmax.reduce(w, initial=0.0))


class Run(NamedTuple):
  log: list            # [(kind, iter, alpha, point, f)] per evaluation
  x: np.ndarray        # the iterate
  f: float             # f there (NaN before the start's evaluation counted)
  status: int
  margin: float        # smallest relative distance of any decision of the run from its threshold


def minimise(value_and_grad, x0, lo=None, hi=None, dtype=np.float64, mutant=None, max_evals=MAX_EVALS, **kw):
  """The state machine of csrc/acq_opt_ctl.h for one start.  value_and_grad(x [D] float64) -> (vals [S], grads [S, D])."""
  assert mutant is None or mutant in MUTANTS
  op = dict(DEFAULTS); op.update(kw)
  d = x0.size
  lo = np.zeros(d) if lo is None else np.asarray(lo, dtype=np.float64)
  hi = np.ones(d) if hi is None else np.asarray(hi, dtype=np.float64)
  rnd = (lambda v: v.astype(np.float32).astype(np.float64)) if np.dtype(dtype) == np.float32 else (lambda v: v)
  mem = op['memory']
  x = np.asarray(x0, dtype=np.float64).copy()
  s_ring, y_ring = [], []          # oldest first
  log, margin = [], [np.inf]

  def near(a, b):                  # how far a decision `a <= b` (or >) is from flipping, relative
    if np.isfinite(a) and np.isfinite(b):
      margin[0] = min(margin[0], abs(a - b) / max(abs(a), abs(b), 1e-300))

  def trial(x, alpha, dvec):
    t = x + alpha * dvec
    if mutant != 'no_projection':
      t = np.clip(t, lo, hi)
    return rnd(t)

  def active_of(x, g):
    return ((x == lo) & (g > 0.0)) | ((x == hi) & (g < 0.0))

  vals, grads = value_and_grad(x)
  f, g = reduce_samples(vals, grads)
  log.append((START, 0, 0.0, x.copy(), f))
  if not np.isfinite(f):
    return Run(log, x, float('nan'), NONFINITE_AT_START, margin[0])
  pg = np.where(active_of(x, g), 0.0, g)
  conv = pg_measure(x, g, lo, hi)
  near(conv, op['pgtol'])
  if conv <= op['pgtol']:
    return Run(log, x, f, CONVERGED, margin[0])
  dvec = -pg
  inv = 1.0 / np.sqrt(tree_dot(pg, pg))
  alpha = inv if inv < 1.0 else 1.0
  probes, it = 0, 0
  xt = trial(x, alpha, dvec)
  while len(log) < max_evals:
    vals, grads = value_and_grad(xt)
    ft, gt = reduce_samples(vals, grads)
    dx = xt - x
    gs = alpha * tree_dot(g, dvec) if mutant == 'armijo_unprojected' else tree_dot(g, dx)
    bound = f + op['c1'] * gs
    moved = bool(np.any(dx != 0.0))
    if moved and np.isfinite(ft):
      margin[0] = min(margin[0], abs(ft - bound) / max(abs(ft - f), abs(op['c1'] * gs), 1e-300))
    accepted = bool(np.isfinite(ft) and ft <= bound)
    if not accepted:
      log.append((LINE_SEARCH, it, alpha, xt.copy(), ft))
      probes += 1
      alpha = alpha * op['tau']
      if probes >= op['ls_steps']:
        return Run(log, x, f, NO_PROGRESS, margin[0])
      xt = trial(x, alpha, dvec)
      continue
    if not moved:
      log.append((LINE_SEARCH, it, alpha, xt.copy(), ft))
      return Run(log, x, f, NO_PROGRESS, margin[0])
    it += 1
    log.append((MAIN, it, alpha, xt.copy(), ft))
    yv = gt - g
    f_old, f, x, g = f, ft, xt.copy(), gt
    sy, yy = tree_dot(dx, yv), tree_dot(yv, yv)
    near(sy, 2.2e-16 * yy)
    if sy > 2.2e-16 * yy or mutant == 'pairs_never_skipped':
      s_ring.append(dx); y_ring.append(yv)
      if len(s_ring) > mem:
        s_ring.pop(0); y_ring.pop(0)
    act = active_of(x, g)
    pg = np.where(act, 0.0, g)
    conv = pg_measure(x, g, lo, hi)
    near(conv, op['pgtol'])
    ftol_abs = op['ftol'] * max(abs(f_old), abs(f), 1.0)
    near(f_old - f, ftol_abs)
    if conv <= op['pgtol']:
      return Run(log, x, f, CONVERGED, margin[0])
    if f_old - f <= ftol_abs:
      return Run(log, x, f, FTOL, margin[0])
    if it >= op['max_iters']:
      return Run(log, x, f, STEPS_DONE, margin[0])
    steepest = not s_ring
    if not steepest:
      n = len(s_ring)
      rho = [1.0 / tree_dot(y_ring[j], s_ring[j]) for j in range(n)]
      q = -pg
      al = [0.0] * n
      for j in range(n - 1, -1, -1):
        al[j] = rho[j] * tree_dot(s_ring[j], q)
        q = q - al[j] * y_ring[j]
      gamma = tree_dot(s_ring[-1], y_ring[-1]) / tree_dot(y_ring[-1], y_ring[-1])
      q = gamma * q
      for j in range(n):
        beta = rho[j] * tree_dot(y_ring[j], q)
        q = q + s_ring[j] * (al[j] - beta)
      dvec = q if mutant == 'active_set_ignored' else np.where(act, 0.0, q)
      gd = tree_dot(g, dvec)
      if not gd < 0.0:
        s_ring, y_ring, steepest = [], [], True
    if steepest:
      dvec = -pg
    alpha, probes = 1.0, 0
    xt = trial(x, alpha, dvec)
  return Run(log, x, f, RUNNING, margin[0])


# ---- cases -----------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
  name: str
  kname: str
  mname: str
  acq: str
  n: int
  d: int
  S: int
  R: int
  seed: int = 0
  kind: str = 'grid'       # 'grid' | 'corner' | 'interior' | 'bound'
  lo: float = 0.0          # the box (the same in every dimension)
  hi: float = 1.0


MEANS = ['zero', 'constant', 'linear']
NS, DS, SS, RS = [1, 7, 65, 128], [1, 3, 33], [1, 5], [1, 9]


def _grid():
  """Covariance x mean x acquisition rotated as in profiles/acq_fused.md: n, D, S, R cycle with their own periods."""
  out, i = [], 0
  for kname in helpers.KERNELS:
    for mname in MEANS:
      for acq in ('ei', 'pi', 'ucb'):
        n, d, s, r = NS[i % 4], DS[i % 3], SS[i % 2], RS[(i // 2) % 2]
        out.append(Case(f'{kname}-{mname}-{acq}-n{n}-D{d}-S{s}-R{r}', kname, mname, acq, n, d, s, r, seed=RESEED.get(i, 0)))
        i += 1
  return out


# grid index -> another draw (the first sits on a knife edge of a decision: test_acq_opt_host.py::test_cases_clear_their_thresholds)
RESEED = {}
GRID = _grid()
SPECIAL = [
    # the maximiser on the boundary: a linear mean with large weights under UCB, and a dot-product kernel
    Case('corner-linear-ucb', 'squared_exponential', 'linear', 'ucb', 7, 3, 1, 1, kind='corner'),
    Case('corner-dot-ucb', 'dot_product', 'zero', 'ucb', 7, 3, 5, 9, kind='corner'),
    # the same linear mean over a GP with the smallest signal variance the warp allows (1e-10), long length-scales and a large noise: f is linear up to a curvature of about 1e-12, the first (s, y)
    # pair gives a direction of length ~1e14, and the projection cuts the step to less than 1.  An Armijo test that charges the
    # unprojected step rejects all 20 probes of that search and stops short of the corner
    Case('corner-flat-ucb', 'squared_exponential', 'linear', 'ucb', 7, 3, 1, 1, kind='corner', seed=1),
    # one observation, SE kernel, PI, started nearby: the maximiser is inside
    Case('interior-se-pi', 'squared_exponential', 'constant', 'pi', 1, 3, 1, 1, kind='interior'),
    # started exactly at a bound with the gradient pointing outward in some components
    Case('bound-matern52-ucb', 'matern52', 'linear', 'ucb', 7, 3, 5, 1, kind='bound'),
    # caller bounds other than the unit box
    Case('box-matern32-ei', 'matern32', 'constant', 'ei', 65, 3, 5, 9, kind='grid', lo=0.25, hi=0.75),
]
CASES = GRID + SPECIAL
BY_NAME = {c.name: c for c in CASES}
assert {c.n for c in GRID} == set(NS) and {c.d for c in GRID} == set(DS) and {c.S for c in GRID} == set(SS) and {c.R for c in GRID} == set(RS)

# Cases on which SciPy's L-BFGS-B and this optimiser end at different points (|dx|_inf > 1e-3) from the same start -- filled from the
# CPU run of test_acq_opt_host.py::test_against_scipy, which holds the list to at most a quarter of the cases
UNMATCHED = ('dot_product-zero-ei-n128-D1-S5-R9',      # start 0 crawls down the flat tail of EI (steepest descent, alpha = 1): RUNNING after 128
             'dot_product-zero-ucb-n7-D33-S5-R1',      # another corner than SciPy's, with the larger value
             'dot_product-constant-ei-n65-D1-S1-R9')   # start 8: the flat tail again


def _cast(t, dtype):
  return {k: _cast(v, dtype) for k, v in t.items()} if isinstance(t, dict) else np.asarray(t, dtype=dtype)


class Inputs(NamedTuple):
  samples: list        # S raw params.model dicts (fp64)
  x: np.ndarray
  y: np.ndarray
  x0: np.ndarray       # [R, D] starts
  param: float
  lo: np.ndarray
  hi: np.ndarray


@functools.lru_cache(maxsize=None)
def inputs(case):
  rng = np.random.default_rng([case.seed, NS.index(case.n) if case.n in NS else 9, case.d, case.S, case.R, len(case.name), 911])
  d = case.d
  samples = [helpers.make_model(np.random.default_rng([case.seed, i, 913]), case.mname, False, d) for i in range(case.S)]
  x, y = helpers.synthetic_task(rng, case.n, d)
  x0 = rng.uniform(0.1, 0.9, size=(case.R, d))
  if case.kind == 'corner':
    for smp in samples:
      if case.mname == 'linear':
        smp['linear_mean']['kernel'] = np.array([[25.0], [-30.0], [40.0]])
      smp['dot_prod_sigma'] = np.array(0.2)
  if case.name == 'corner-flat-ucb':
    samples[0].update(signal_variance=np.array(-36.0), noise_variance=np.array(3.0), lengthscale=np.full(d, 4.0))
    samples[0]['linear_mean']['kernel'] = np.array([[-25.0], [30.0], [-40.0]])   # (residuals > 0: f is convex near the observations)
    x0 = np.array([[0.95, 0.5, 0.1]])      # the unit first step ends on two faces, short of the third
  if case.kind == 'interior':
    x = np.full((1, d), 0.5) + np.array([[0.05, -0.1, 0.08]])
    y = np.array([[1.5]])
    x0 = x + np.array([[0.04, 0.03, -0.05]])
    for smp in samples:
      smp['lengthscale'] = helpers.inv_softplus(np.full(d, 0.3))
  if case.kind == 'bound':
    x0 = np.array([[0.0, 1.0, 0.4]])
  if (case.lo, case.hi) != (0.0, 1.0):
    x0 = case.lo + (case.hi - case.lo) * x0
  param = {'ei': float(np.max(y)), 'pi': float(np.max(y)) + 0.1, 'ucb': 3.0}[case.acq]
  return Inputs(samples, x, y, np.ascontiguousarray(x0), param, np.full(d, case.lo), np.full(d, case.hi))


def noise_of(smp):
  return float(np.squeeze(o.retrieve_params(o.GPParams(model=_cast(smp, np.float64)), ['noise_variance'], WFO)[0]))


def oracle_value_and_grad(case):
  """x [D] -> (vals [S], grads [S, D]) from the oracle, one acquisition_value_and_grad per parameter sample."""
  inp = inputs(case)
  ko, mo = getattr(o, case.kname), getattr(o, case.mname)
  ps = [(o.GPParams(model=_cast(smp, np.float64), config={}), noise_of(smp)) for smp in inp.samples]

  def vg(x):
    vals, grads = [], []
    for po, noise in ps:
      v, g = o.acquisition_value_and_grad(case.acq, mo, ko, po, inp.x, inp.y, np.asarray(x, dtype=np.float64)[None, :], inp.param, WFO,
                                          add_noise=noise, scale=SCALE)
      vals.append(float(v[0, 0])); grads.append(np.asarray(g[0], dtype=np.float64))
    return np.array(vals), np.array(grads)
  return vg


@functools.lru_cache(maxsize=None)
def oracle_run(case, r, mutant=None):
  """The oracle-driven restatement of start r of the case (shared, not to be written to)."""
  inp = inputs(case)
  return minimise(oracle_value_and_grad(case), inp.x0[r], inp.lo, inp.hi, mutant=mutant)
