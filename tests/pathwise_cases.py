"""CPU side of the pathwise-sampling tier (hbo_sample_paths, csrc/paths.hip; hyperbo_amd/gp_utils/pathwise.py).  Shared by
tests/test_pathwise_host.py (this file judged on its own, on the CPU) and tests/test_gpu_pathwise.py (the device against it):

  CASES               the shapes of the GPU tier: n in {1, 127, 128, 129, 300} and the prior branch, M in {1, 130, 300}, F in
                      {1, 63, 64, 65, 200}, S in {1, 3, 65}, D in {1, 3, 17}, the four kernels, the four means, an MLP basis, a Kumaraswamy
                      warp; each in fp64 and fp32
  draws(...)          the draws of the contract, restated: one Generator, fp64, fixed order (and the spectral mutants)
  restate(prob, wide) the formulas of include/hbo.h in NumPy, in `wide` = float32, float64 or np.longdouble (Cholesky and substitutions
                      by hand, the oracle's kernels and means, which compute in the dtype of their inputs), and the formula mutants
  bounds              fp64: FP64_BOUND; fp32: REL_FACTOR x the float32 restatement's own error + FLOOR_C eps32
"""
import functools
from typing import NamedTuple

import numpy as np

import helpers
import kumar_oracle
from oracle import hyperbo_oracle as o

WFO = o.DEFAULT_WARP_FUNC
LD = np.longdouble
TILE = 128
EPS = 1e-6                  # the jitter of linalg.py:36-69: part of the matrix the cache factorised
NU = {'matern32': 1.5, 'matern52': 2.5}

# ---- bounds ------------------------------------------------------------------------------------------------------------------------
FP64_BOUND = 1e-9           # the project's bound for predict's mean (test_factor_predict_acquisition_vs_oracle), helpers.rel_err per column
# fp32: err <= REL_FACTOR * (error of the float32 restatement against longdouble) + FLOOR_C * eps32 -- REL_FACTOR / FLOOR_C of
# append_cases.py, for the same reason: the device rounds its operands (W = L^-1, the cross Gram, the cosines) to fp32 as the float32
# restatement does and sums in fp64, so its error is of the restatement's order; the floor covers a restatement that happens to land
# within an ulp.  The restatement's error LEVEL is taken over all columns of the case (the columns are draws through one computation),
# and every column of the device is held to it.
REL_FACTOR = 4.0
FLOOR_C = 8.0
COND_BOUND = 1e-11          # rel_err(fp64 restatement, longdouble) on every case: the yardstick is 100 x finer than FP64_BOUND
MUTANT_FACTOR = 100.0       # every applicable formula mutant lies at least this many FP64_BOUNDs from the longdouble restatement
SPECTRAL_C = 5.0            # max |Phi Phi^T - K| / signal_variance <= SPECTRAL_C / sqrt(F)
SPECTRAL_F = (4096, 16384)


class Case(NamedTuple):
  kname: str
  mlp: bool
  mname: str
  kumar: bool
  n: int                     # observations (0: the prior branch)
  M: int
  F: int                     # features (the dot product: fdim + 1)
  S: int
  d: int
  dtype: str = 'fp64'
  chunk: int = 0             # post_chunk for the call (0: the default)

  @property
  def id(self):
    return (f'{self.kname}{"_mlp" if self.mlp else ""}{"_kumar" if self.kumar else ""}+{self.mname}-n{self.n}-M{self.M}-F{self.F}-S{self.S}'
            f'-D{self.d}-{self.dtype}' + (f'-chunk{self.chunk}' if self.chunk else ''))

  @property
  def np_dtype(self):
    return np.float64 if self.dtype == 'fp64' else np.float32

  @property
  def fdim(self):
    return helpers.MLP_FEATURES[-1] if self.mlp else self.d


_SHAPES = [
    Case('squared_exponential', False, 'constant', False, 1, 1, 1, 1, 1),
    Case('matern32', False, 'linear', False, 127, 130, 63, 3, 3),
    Case('matern52', False, 'zero', False, 128, 130, 64, 65, 17),
    Case('squared_exponential', False, 'linear_mlp', False, 129, 300, 65, 3, 3, chunk=128),   # three chunks of queries
    Case('matern52', False, 'constant', False, 300, 300, 200, 65, 3, chunk=128),
    Case('matern32', False, 'constant', False, 300, 1, 200, 3, 17),
    Case('dot_product', False, 'constant', False, 129, 130, 4, 3, 3),
    Case('dot_product', False, 'linear', False, 300, 130, 18, 65, 17),
    Case('matern52', True, 'linear_mlp', False, 129, 130, 64, 3, 3),                          # the kernel on the MLP basis (fdim 5)
    Case('squared_exponential', False, 'constant', True, 129, 130, 65, 3, 3),                 # Kumaraswamy-warped inputs
    Case('matern52', False, 'constant', False, 0, 130, 200, 3, 3),                            # the prior branch
    Case('dot_product', False, 'linear', False, 0, 130, 4, 3, 3),
]
CASES = _SHAPES + [c._replace(dtype='fp32') for c in _SHAPES]


# ---- the draws, restated -------------------------------------------------------------------------------------------------------------
SPECTRAL_MUTANTS = {
    'gauss_matern': 'Gaussian omega for a Matern kernel (no chi-square mixing)',
    'nu_dof': 'nu in place of 2 nu degrees of freedom',
    'half_phase': 'phases from [0, pi)',       # NOT a defect of the second moments, see test_pathwise_host.py: kept to pin that fact
    'zero_phase': 'no phases at all (b = 0)',
    'amp': 'amplitude sqrt(sv / F)',
}


def draws(rng, kname, fdim, ls, F, S, n, mutant=None):
  """(omega [F, fdim], phase [F], w [F, S], eps [n, S] or None), fp64, in the order of the contract (pathwise.draw's docstring)."""
  if kname == 'dot_product':
    F = fdim + 1
    omega, phase = np.zeros((F, fdim)), np.zeros(F)
  else:
    z = rng.standard_normal((F, fdim))
    if kname in NU and mutant != 'gauss_matern':
      dof = NU[kname] if mutant == 'nu_dof' else 2 * NU[kname]
      g = rng.chisquare(dof, F)
      z *= np.sqrt(dof / g)[:, None]
    omega = z / np.broadcast_to(np.reshape(np.asarray(ls, dtype=np.float64), (-1,)), (fdim,))
    phase = rng.uniform(0, np.pi if mutant == 'half_phase' else 2 * np.pi, F) * (0.0 if mutant == 'zero_phase' else 1.0)
  w = rng.standard_normal((F, S))
  eps = rng.standard_normal((n, S)) if n else None
  return omega, phase, w, eps


def amplitude(sv, F, mutant=None):
  return np.sqrt((1.0 if mutant == 'amp' else 2.0) * sv / F)


# ---- problems ------------------------------------------------------------------------------------------------------------------------
class Problem(NamedTuple):
  kname: str
  mlp: bool
  mname: str
  kumar: bool
  model: dict                # raw params.model, in the model dtype
  x: np.ndarray              # [n, d] (n may be 0), model dtype
  y: np.ndarray              # [n, 1]
  xq: np.ndarray             # [M, d]
  omega: np.ndarray          # the draws, cast to the model dtype
  phase: np.ndarray
  w: np.ndarray
  eps: object                # [n, S] or None


def cast(tree, dtype):
  return {k: cast(v, dtype) for k, v in tree.items()} if isinstance(tree, dict) else np.asarray(tree, dtype=dtype)


def config():
  return {'mlp_features': helpers.MLP_FEATURES}


def warped_lengthscale(model):
  """The fp64 warp of the (model-dtype) raw lengthscale: what omega is divided by."""
  return np.asarray(o.default_softplus(np.asarray(model['lengthscale'], dtype=np.float64)), dtype=np.float64)


def _seed(case):
  return [helpers.KERNELS.index(case.kname), int(case.mlp), helpers.MEANS.index(case.mname), int(case.kumar), case.n, case.M, case.F, case.S,
          case.d, 41]


def draw_seed(case):
  return _seed(case) + [7]


@functools.lru_cache(maxsize=None)
def problem(case):
  """The case's model, data and draws; the dtype is not part of the seed (fp32 cases are the fp64 ones, rounded once, here)."""
  rng = np.random.default_rng(_seed(case))
  model = helpers.make_model(rng, case.mname, case.mlp, case.d)
  if case.kumar:
    model['kumar_params'] = {'a': rng.uniform(-1.0, 1.0, size=case.d), 'b': rng.uniform(-1.0, 1.0, size=case.d)}
  x, y = helpers.synthetic_task(rng, max(case.n, 1), case.d)
  x, y = x[:case.n], y[:case.n]
  xq = rng.uniform(0.05, 0.95, size=(case.M, case.d))
  dt = case.np_dtype
  model = cast(model, dt)
  ls = warped_lengthscale(model) if case.kname != 'dot_product' else None
  om, ph, w, eps = draws(np.random.default_rng(draw_seed(case)), case.kname, case.fdim, ls, case.F, case.S, case.n)
  c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=dt)
  return Problem(case.kname, case.mlp, case.mname, case.kumar, model, c(x), c(y), c(xq), c(om), c(ph), c(w), c(eps))


# ---- the formulas, restated ----------------------------------------------------------------------------------------------------------
MUTANTS = {
    'no_jitter': 'the jitter left out of Ktilde and of the noise scale',
    'no_prior_at_x': 'p_s(X) is not subtracted from the residual',
    'drop_last_block': 'the last partial 128-block of the observations dropped from the update sum',
    'no_phase': 'the cosines without their phase',
}


def not_applicable(prob):
  """Mutants that cannot show at the problem's shape, by the shape alone."""
  na = set()
  n = prob.x.shape[0]
  if n == 0:
    na |= {'no_jitter', 'no_prior_at_x', 'drop_last_block'}      # the prior branch has no solve and no update term
  if n % TILE == 0:
    na.add('drop_last_block')                                      # no partial block
  if prob.kname == 'dot_product':
    na.add('no_phase')                                             # the exact basis has no phase
  return na


def chol(a):
  n = a.shape[0]
  c = np.zeros_like(a)
  for j in range(n):
    v = a[j:, j] - c[j:, :j] @ c[j, :j]
    c[j, j] = np.sqrt(v[0])
    c[j + 1:, j] = v[1:] / c[j, j]
  return c


def solve_lower(c, b, trans=False):
  """c^-1 b (trans: c^-T b), c lower triangular, b (n, k); substitutions in the dtype of the arrays."""
  n = c.shape[0]
  v = np.zeros_like(b)
  if not trans:
    for i in range(n):
      v[i] = (b[i] - c[i, :i] @ v[:i]) / c[i, i]
  else:
    for i in range(n - 1, -1, -1):
      v[i] = (b[i] - c[i + 1:, i] @ v[i + 1:]) / c[i, i]
  return v


def _params(prob, wide):
  """The oracle's parameter container: float32 parameters for the float32 restatement (everything in float32), else fp64 (exact
  images of the model-dtype values; the oracle's functions then compute in the dtype of their inputs)."""
  return o.GPParams(model=cast(prob.model, np.float32 if wide == np.float32 else np.float64), config=config())


def features(prob, po, v):
  """phi(v): what the covariance sees, in the dtype of v."""
  if prob.mlp:
    return o.mlp_apply(o.retrieve_params(po, ['mlp_params'], WFO)[0], v)
  if prob.kumar:
    kp = po.model['kumar_params']
    a, b = kumar_oracle.squareplus(kp['a']).astype(v.dtype), kumar_oracle.squareplus(kp['b']).astype(v.dtype)
    return 1 - (1 - v ** a) ** b
  return v


def prior_paths(prob, po, phi, wide, mutant=None):
  """p_s at the rows of phi: [rows, S]."""
  w = prob.w.astype(wide)
  if prob.kname == 'dot_product':
    sigma, bias = [np.asarray(t, dtype=wide) for t in o.retrieve_params(po, ['dot_prod_sigma', 'dot_prod_bias'], WFO)]
    return (phi / sigma) @ w[:-1] + bias * w[-1][None, :]
  sv = np.asarray(o.retrieve_params(po, ['signal_variance'], WFO)[0], dtype=wide)
  arg = phi @ prob.omega.astype(wide).T
  if mutant != 'no_phase':
    arg = arg + prob.phase.astype(wide)[None, :]
  F = prob.w.shape[0]
  return np.sqrt(wide(2) * sv / wide(F)) * (np.cos(arg) @ w)


def restate(prob, wide, mutant=None, zero=False, no_eps=False):
  """[M, S] path values by the formulas of include/hbo.h, every array in `wide`.  zero: w = 0 and eps = 0 (the posterior mean);
  no_eps: the noise draw left out (the validation's counter-example)."""
  assert mutant is None or mutant in MUTANTS
  if zero:
    prob = prob._replace(w=np.zeros_like(prob.w), eps=None if prob.eps is None else np.zeros_like(prob.eps))
  po = _params(prob, wide)
  base = getattr(o, prob.kname)
  mo = getattr(o, prob.mname)
  x, y, xq = prob.x.astype(wide), prob.y.astype(wide), prob.xq.astype(wide)
  n = x.shape[0]
  phi_q = features(prob, po, xq)
  f = np.asarray(mo(po, xq, warp_func=WFO), dtype=wide) + prior_paths(prob, po, phi_q, wide, mutant)
  assert f.dtype == wide, f.dtype
  if n == 0:
    return f
  phi_x = features(prob, po, x)
  noise = np.asarray(o.retrieve_params(po, ['noise_variance'], WFO)[0], dtype=wide)
  jitter = wide(0) if mutant == 'no_jitter' else wide(EPS)
  kt = base(po, phi_x, warp_func=WFO) + np.eye(n, dtype=wide) * (noise + jitter)
  r = (y - np.asarray(mo(po, x, warp_func=WFO), dtype=wide)) * np.ones((1, prob.w.shape[1]), dtype=wide)
  if mutant != 'no_prior_at_x':
    r = r - prior_paths(prob, po, phi_x, wide, mutant)
  if not no_eps:
    r = r - np.sqrt(noise + jitter) * prob.eps.astype(wide)
  c = chol(kt)
  v = solve_lower(c, solve_lower(c, r), trans=True)
  kxq = base(po, phi_x, phi_q, warp_func=WFO)
  keep = n // TILE * TILE if mutant == 'drop_last_block' else n
  out = f + kxq[:keep].T @ v[:keep]
  assert out.dtype == wide, out.dtype
  return out


@functools.lru_cache(maxsize=None)
def reference(case):
  """The longdouble restatement of the case: shared, not to be written to."""
  return restate(problem(case), LD)


@functools.lru_cache(maxsize=None)
def reference_mean(case):
  return restate(problem(case), LD, zero=True)[:, :1]


def col_errors(got, ref):
  """helpers.rel_err per column."""
  got, ref = np.asarray(got), np.asarray(ref)
  assert got.shape == ref.shape, (got.shape, ref.shape)
  return np.array([helpers.rel_err(got[:, s].astype(np.float64), ref[:, s].astype(np.float64)) if np.isfinite(got[:, s].astype(np.float64)).all()
                   else np.inf for s in range(ref.shape[1])])


@functools.lru_cache(maxsize=None)
def f32_level(case):
  """The float32 restatement's error against longdouble, the largest over the columns."""
  return float(np.max(col_errors(restate(problem(case), np.float32), reference(case))))


def bound(case):
  if case.dtype == 'fp64':
    return FP64_BOUND
  return REL_FACTOR * f32_level(case) + FLOOR_C * float(np.finfo(np.float32).eps)


# ---- the Thompson-sampling loop, restated ----------------------------------------------------------------------------------------------
def thompson_loop(model, x0, y0, pool_x, pool_y, iters, F, seed, kname='matern52', mname='constant'):
  """(selected indices, smallest relative gap between the best and the second-best value of an iteration): simulated_bayesopt with
  thompson_sampling, in longdouble, driven by a Generator seeded as the model's."""
  rng = np.random.default_rng(seed)
  x, y = np.array(x0, dtype=np.float64), np.array(y0, dtype=np.float64)
  sel, gap = [], np.inf
  for _ in range(iters):
    om, ph, w, eps = draws(rng, kname, x.shape[1], warped_lengthscale(model), F, 1, x.shape[0])
    prob = Problem(kname, False, mname, False, model, x, y, np.asarray(pool_x, dtype=np.float64), om, ph, w, eps)
    f = restate(prob, LD)[:, 0]
    order = np.argsort(-f, kind='stable')
    gap = min(gap, float((f[order[0]] - f[order[1]]) / np.max(np.abs(f))))
    sel.append(int(order[0]))
    x = np.vstack([x, pool_x[order[0]][None, :]]); y = np.vstack([y, np.reshape(pool_y[order[0]], (1, 1))])
  return sel, gap


class TsSetup(NamedTuple):
  model: dict
  x0: np.ndarray
  y0: np.ndarray
  pool_x: np.ndarray
  pool_y: np.ndarray
  iters: int
  F: int
  seed: int


TS_GAP = 1e3 * FP64_BOUND   # an argmax is "not decided by rounding" when the runner-up is this far below, relative to max |f|


@functools.lru_cache(maxsize=None)
def ts_setup():
  """A 10-iteration Thompson-sampling run over a pool of 60 candidates, D = 2, matern52 + constant, 20 observations to start with."""
  rng = np.random.default_rng(20241)
  model = helpers.make_model(rng, 'constant', False, 2)
  x, y = helpers.synthetic_task(rng, 80, 2)
  return TsSetup(model, x[:20], y[:20], x[20:], y[20:], 10, 64, 991)
