"""CPU side of the shape tier of hbo_acq_grad (csrc/acq_grad.hip: the per-cache gradient d acquisition / d x_query that bayesopt() hands to
L-BFGS-B; csrc/post.hip: acq_grad_kernel, tri_matvec_kernel, tri_matmat_fwd_kernel / tri_matmat_trans_kernel; the MLP backward to the
query; kumar_chain_dx_kernel).  Shared by tests/test_acq_grad_cases_host.py (this file judged on its own) and
tests/test_gpu_acq_grad_shapes.py (the device against it):

  CASES                the case list, groups A .. F: feature widths on both sides of every thread layout of acq_grad_kernel, MLP stacks,
                       query counts across the 8-column groups and the 1024-query pass, cache sizes across the 64 / 128 / 256-row
                       chunks, the prior branch, Kumaraswamy widths
  inputs(case)         model, x, y, xq in the case's dtype
  reference(case)      value and gradient of UCB(3), EI and PI from oracle/hyperbo_oracle.py: acquisition_value_and_grad, always
                       evaluated in fp64 (fp32 cases: on the fp32-rounded inputs and parameters), with each query's
                       gamma = (target - mu) / sd.  EI and PI share one target per case: the median posterior mean of the queries,
                       or, where that leaves every query within GAMMA_MIN = 0.5 standard deviations of it, the median plus the
                       median standard deviation.  The second form applies to 69 of the 219 fp64 / fp32 pairs: all 42 with M = 1
                       (the median is the query's own mean) and 27 with M >= 2 (C at M = 2 and 8, ten dot-product and one Matern
                       case of D at M = 9, seven of the eight M = 9 prior cases of E, five widths of A, one stack of B)
  ratios(...)          the per-query bounds of the GPU test, as ratios to them
  MUTANTS              the reference with one failure the kernels could have, each, from a NumPy restatement of the device's route
                       (l = W k, beta = W^T l, W = L^-1) that test_acq_grad_cases_host.py first holds against the oracle
"""
import functools
from typing import NamedTuple, Tuple

import numpy as np
import scipy.linalg as spla

import helpers
import kumar_oracle
from oracle import hyperbo_oracle as o

WFO = o.DEFAULT_WARP_FUNC
SCALE = 1.5                 # T / (T - 1) of three sub-datasets (gp.py:607-619)
UCB_BETA = 3.0
ACQS = ('ucb', 'ei', 'pi')
ACQ_IDS = {'ei': 0, 'pi': 1, 'ucb': 2}   # include/hbo.h
STATIONARY = ['squared_exponential', 'matern32', 'matern52']
KERNELS = STATIONARY + ['dot_product']

# ---- bounds of the GPU tier (the project's own: tests/test_gpu_acq_tails.py (d), test_gpu_parity.py) ------------------------------
FP64_VALUE_RTOL, FP64_VALUE_ATOL = 1e-8, 1e-10
FP64_GRAD_TOL = 1e-7        # max_d |g - g_ref| <= tol * (1 + gamma^2) * max_d |g_ref|, per query
FP32_VALUE_TOL = 5e-3       # of max |v_ref| over the case, per query
FP32_GRAD_TOL = 2e-2        # as FP64_GRAD_TOL, at |gamma| <= FP32_GAMMA_MAX only
FP32_GAMMA_MAX = 3.0
GRAD_FLOOR = 1e-8           # condition 3: every query's max_d |g_ref| is at least this much of the case's largest
GAMMA_MIN = 0.5             # condition 5: some query of the case sits at least this far from the target (see reference())
MUTANT_FACTOR = 100.0       # fp64: every applicable mutant is at least this many bounds away on some query
# fp32: 100 bounds would be 2 (1 + gamma^2) times the query's largest gradient component, beyond what a defect that leaves the gradient
# within twice its own size can reach; what the host test asserts instead is that the fp32 bounds of the GPU tier SEE every mutant.
FP32_MUTANT_FACTOR = 1.0


class Case(NamedTuple):
  group: str                 # 'A' .. 'F'
  kname: str                 # the base kernel
  mlp_k: bool                # the kernel works on the MLP basis
  mname: str
  kumar: bool
  n: int                     # observations (0: the prior branch, no cache)
  M: int                     # queries
  d: int                     # input width
  feats: Tuple[int, ...]     # the MLP stack; () without an MLP
  ls: str                    # 'ard' | 'scalar' | 'none' (dot product)
  dtype: str                 # 'fp64' | 'fp32'

  @property
  def kernel_name(self):
    return self.kname + ('_mlp' if self.mlp_k else '') + ('_kumar' if self.kumar else '')

  @property
  def id(self):
    f = ('-f' + 'x'.join(str(v) for v in self.feats)) if self.feats else ''
    return f'{self.group}-{self.kernel_name}+{self.mname}-{self.ls}-n{self.n}-M{self.M}-d{self.d}{f}-{self.dtype}'

  @property
  def np_dtype(self):
    return np.float64 if self.dtype == 'fp64' else np.float32

  @property
  def fdim(self):
    """Width of the kernel's features: what acq_grad_kernel's thread layout is derived from."""
    return self.feats[-1] if self.mlp_k else self.d

  @property
  def npad(self):
    return -(-self.n // 128) * 128


DTYPES = ['fp64', 'fp32']
A_WIDTHS = [1, 2, 5, 16, 17, 32, 33, 64, 65, 128, 129, 256]
B_STACKS = [(12, 17), (12, 33), (12, 64), (12, 256), (40, 17), (7, 40, 9, 33)]
B_PAIRINGS = [(True, 'linear_mlp'), (True, 'linear'), (False, 'linear_mlp')]
C_COUNTS = [1, 2, 8, 9, 1023, 1024, 1025, 2049]
D_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 513]
F_WIDTHS = [1, 17, 40, 256]


def _ls_forms(kname):
  return ('ard', 'scalar') if kname != 'dot_product' else ('none',)


def _c_models(M, dt):
  return [Case('C', 'squared_exponential', False, 'constant', False, 150, M, 4, (), 'ard', dt),
          Case('C', 'matern52', True, 'linear_mlp', False, 150, M, 4, (12, 33), 'ard', dt),
          Case('C', 'squared_exponential', False, 'constant', True, 150, M, 4, (), 'ard', dt)]


CASES_A = [Case('A', k, False, 'linear', False, 300, 9, d, (), ls, dt) for d in A_WIDTHS for k in KERNELS for ls in _ls_forms(k) for dt in DTYPES]
CASES_B = [Case('B', k, mk, mn, False, 150, 9, 5, st, 'ard' if k != 'dot_product' else 'none', dt)
           for st in B_STACKS for k in (('matern52', 'dot_product') if st == (12, 33) else ('matern52',))
           for (mk, mn) in B_PAIRINGS for dt in DTYPES]
CASES_C = [c for M in C_COUNTS for dt in DTYPES for c in _c_models(M, dt)]
CASES_D = [Case('D', k, False, mn, False, n, M, 4, (), ls, dt) for n in D_SIZES for M in (1, 9)
           for (k, mn, ls) in (('matern52', 'constant', 'ard'), ('dot_product', 'linear', 'none')) for dt in DTYPES]
CASES_E = ([Case('E', k, False, 'linear', False, 0, M, d, (), 'ard' if k != 'dot_product' else 'none', dt)
            for d in (17, 256) for k in KERNELS for M in (1, 9) for dt in DTYPES] +
           [Case('E', 'matern52', True, 'linear_mlp', False, 0, M, 5, (12, 33), 'ard', dt) for M in (1, 9) for dt in DTYPES])
CASES_F = [Case('F', k, False, 'constant', True, 150, 9, d, (), 'ard' if k != 'dot_product' else 'none', dt)
           for d in F_WIDTHS for k in ('squared_exponential', 'matern52', 'dot_product') for dt in DTYPES]
CASES = CASES_A + CASES_B + CASES_C + CASES_D + CASES_E + CASES_F


def reuse_cases():
  """The calls of the workspace re-use test, in order (the first is run again after the third)."""
  return [Case('R', 'matern52', False, 'linear', False, 513, 1025, 64, (), 'ard', 'fp64'),
          Case('R', 'matern52', False, 'linear', False, 2, 1, 1, (), 'ard', 'fp64'),
          Case('R', 'dot_product', False, 'linear', False, 0, 9, 256, (), 'none', 'fp64')]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def cast(tree, dtype):
  return {k: cast(v, dtype) for k, v in tree.items()} if isinstance(tree, dict) else np.asarray(tree, dtype=dtype)


# (group, kernel, length-scale form, d) -> another draw: with the first one the case breaks condition 2 (three of its nine queries
# beyond |gamma| = 3 in fp32)
RESEED = {('A', 'squared_exponential', 'scalar', 2): 1}


def _seed(case):
  return [ord(case.group), KERNELS.index(case.kname), int(case.mlp_k), helpers.MEANS.index(case.mname), int(case.kumar), case.n, case.M,
          case.d, len(case.feats), sum(case.feats), int(case.ls == 'scalar'), 23 + RESEED.get((case.group, case.kname, case.ls, case.d), 0)]


def _model(rng, case):
  d, dot = case.d, case.kname == 'dot_product'
  if case.feats:
    model = helpers.mlp_model(rng, d, case.feats, case.kname, case.ls)
    if not case.mlp_k:      # the kernel sees the raw inputs
      if dot:
        model['dot_prod_sigma'] = helpers.inv_softplus(0.5 * np.sqrt(d))
      else:
        model['lengthscale'] = helpers.lengthscale(rng, d, case.ls)
  else:
    model = {'signal_variance': helpers.inv_softplus(0.8), 'noise_variance': helpers.inv_softplus(0.1)}
    if dot:
      model['dot_prod_sigma'] = helpers.inv_softplus(0.5 * np.sqrt(d))
      model['dot_prod_bias'] = np.array(0.2)
    else:
      model['lengthscale'] = helpers.lengthscale(rng, d, case.ls)
  if case.mname == 'linear':
    model['linear_mean'] = {'kernel': rng.normal(size=(d, 1)) / np.sqrt(d), 'bias': rng.normal(size=1)}
  elif case.mname == 'constant':
    model.pop('linear_mean', None)
    model['constant'] = np.array(0.4)
  if case.kumar:
    model['kumar_params'] = {'a': rng.uniform(-1.0, 1.0, size=d), 'b': rng.uniform(-1.0, 1.0, size=d)}
  return model


@functools.lru_cache(maxsize=None)
def inputs(case):
  """(model, x, y, xq) in the case's dtype; fp32 cases are rounded here, once, and everything downstream starts from the rounded
  numbers.  The dtype is not part of the seed: an fp32 case is its fp64 twin, rounded."""
  rng = np.random.default_rng(_seed(case))
  model = _model(rng, case)
  x, y = helpers.synthetic_task(rng, max(case.n, 1), case.d)
  xq = rng.uniform(0.05, 0.95, size=(case.M, case.d)) if case.kumar else rng.uniform(size=(case.M, case.d))
  dt = case.np_dtype
  return cast(model, dt), x[:case.n].astype(dt), y[:case.n].astype(dt), np.ascontiguousarray(xq.astype(dt))


def config(case):
  return {'mlp_features': tuple(case.feats)} if case.feats else {}


class Setup(NamedTuple):
  mo: object
  ko: object
  po: object
  x: object          # None on the prior branch
  y: object
  xq: np.ndarray     # what the oracle's kernel sees: w(xq) for a Kumaraswamy model
  chain: object      # dw/dx at the raw queries (Kumaraswamy), else None
  noise: float


@functools.lru_cache(maxsize=64)
def oracle_setup(case):
  """The oracle's functions, fp64 parameters and fp64 inputs.  Kumaraswamy: the base kernel under a constant mean on warped
  observations and queries; the gradient is then chained with dw/dx at the raw queries."""
  model, x, y, xq = inputs(case)
  m64 = cast(model, np.float64)
  x, y, xq = x.astype(np.float64), y.astype(np.float64), xq.astype(np.float64)
  ko = getattr(o, case.kname + ('_mlp' if case.mlp_k else ''))
  mo = getattr(o, case.mname)
  chain = None
  if case.kumar:
    assert case.mname == 'constant' and not case.feats
    kp = m64.pop('kumar_params')
    chain = kumar_oracle.dw_dx(xq, kumar_oracle.squareplus(kp['a']), kumar_oracle.squareplus(kp['b']))
    x, xq = kumar_oracle.warp(x, kp['a'], kp['b']), kumar_oracle.warp(xq, kp['a'], kp['b'])
  po = o.GPParams(model=m64, config=config(case))
  noise = float(np.squeeze(o.retrieve_params(po, ['noise_variance'], WFO)[0]))
  return Setup(mo, ko, po, x if case.n else None, y if case.n else None, xq, chain, noise)


class Ref(NamedTuple):
  target: float      # of EI and PI, rounded to the model dtype
  mu: np.ndarray
  sd: np.ndarray
  val: dict          # acquisition -> (M,)
  grad: dict         # acquisition -> (M, d)
  gamma: dict        # acquisition -> (M,): (target - mu) / sd; 0 for UCB


def acq_param(acq, ref_or_target):
  t = ref_or_target.target if isinstance(ref_or_target, Ref) else ref_or_target
  return UCB_BETA if acq == 'ucb' else t


def oracle_value_and_grad(case, acq, param, xq=None):
  """o.acquisition_value_and_grad of the case (at other warped / raw queries `xq` when given: the finite differences)."""
  s = oracle_setup(case)
  val, grad = o.acquisition_value_and_grad(acq, s.mo, s.ko, s.po, s.x, s.y, s.xq if xq is None else xq, param, WFO, add_noise=s.noise, scale=SCALE)
  return val[:, 0], grad


@functools.lru_cache(maxsize=None)
def reference(case):
  """Shared and not to be written to."""
  s = oracle_setup(case)
  mu, var = o.predict(s.mo, s.ko, s.po, s.x, s.y, s.xq, WFO)
  mu, var = np.asarray(mu, dtype=np.float64).ravel(), np.asarray(var, dtype=np.float64).ravel()
  sd = np.sqrt((var + s.noise) * SCALE)
  # The shared target of EI and PI: the median posterior mean.  Where that leaves every query closer than GAMMA_MIN standard deviations
  # to it, PI = (mu - target) / sd is small everywhere and a value bound relative to max |v_ref| over the case is a bound relative to
  # little (M = 1: the query's own mean, PI is zero up to the rounding of the target, a bound relative to nothing); the target is then
  # one (median) standard deviation above the median: gamma about 1.  Not only M = 1: see the module docstring for how often.
  target = np.median(mu)
  if np.max(np.abs(target - mu) / sd) < GAMMA_MIN:
    target = target + np.median(sd)
  target = float(case.np_dtype(target))
  val, grad, gamma = {}, {}, {}
  for acq in ACQS:
    v, g = oracle_value_and_grad(case, acq, acq_param(acq, target))
    val[acq], grad[acq] = v, (g if s.chain is None else g * s.chain)
    gamma[acq] = np.zeros_like(mu) if acq == 'ucb' else (target - mu) / sd
  return Ref(target, mu, sd, val, grad, gamma)


# ---- bounds ----------------------------------------------------------------------------------------------------------------------
def checked(case, acq, ref):
  """The queries whose gradient the GPU test judges: all of them in fp64, |gamma| <= 3 in fp32."""
  if case.dtype == 'fp64':
    return np.ones(case.M, dtype=bool)
  return np.abs(ref.gamma[acq]) <= FP32_GAMMA_MAX


def ratios(case, acq, ref, val, grad):
  """Per query: (|v - v_ref| over its bound, max_d |g - g_ref| over its bound; NaN where the gradient is not judged).  A value that
  is not finite is infinitely far."""
  vr, gr, gam = ref.val[acq], ref.grad[acq], ref.gamma[acq]
  val, grad = np.asarray(val, dtype=np.float64).reshape(case.M), np.asarray(grad, dtype=np.float64).reshape(case.M, case.d)
  if case.dtype == 'fp64':
    vb = FP64_VALUE_ATOL + FP64_VALUE_RTOL * np.abs(vr)
    gtol = FP64_GRAD_TOL
  else:
    vb = np.full(case.M, FP32_VALUE_TOL * np.max(np.abs(vr)))
    gtol = FP32_GRAD_TOL
  ev = np.abs(val - vr)
  eg = np.max(np.abs(grad - gr), axis=1)
  rv = np.where(np.isfinite(ev), ev, np.inf) / vb
  rg = np.where(np.isfinite(eg), eg, np.inf) / (gtol * (1.0 + gam * gam) * np.max(np.abs(gr), axis=1))
  return rv, np.where(checked(case, acq, ref), rg, np.nan)


def worst(case, acq, ref, val, grad):
  """(worst value ratio, its query), (worst gradient ratio over the judged queries, its query, its gamma)."""
  rv, rg = ratios(case, acq, ref, val, grad)
  rg = np.where(np.isnan(rg), -1.0, rg)
  qv, qg = int(np.argmax(rv)), int(np.argmax(rg))
  return (float(rv[qv]), qv), (float(rg[qg]), qg, float(ref.gamma[acq][qg]))


def conditions(case, ref):
  """Conditions 1 - 3 of the tier and condition 5 (the values of EI / PI have a scale: GAMMA_MIN), from the oracle alone; a list of
  what is broken (empty: all hold)."""
  out = []
  for acq in ACQS:
    left = int(np.sum(~checked(case, acq, ref)))
    allowed = 0 if (case.dtype == 'fp64' or acq == 'ucb') else -(-case.M // 9)
    if left > allowed:
      out.append(f'{acq}: {left} of {case.M} queries beyond |gamma| = 3 (at most {allowed})')
    gmax = np.max(np.abs(ref.grad[acq]), axis=1)
    if not (np.isfinite(gmax).all() and gmax.min() >= GRAD_FLOOR * gmax.max() and gmax.max() > 0):
      out.append(f'{acq}: per-query gradient ratio {gmax.min() / gmax.max():.2e} < {GRAD_FLOOR:g}')
    if not np.isfinite(ref.val[acq]).all():
      out.append(f'{acq}: value not finite')
    if acq != 'ucb' and not np.max(np.abs(ref.gamma[acq])) >= GAMMA_MIN:
      out.append(f'{acq}: every query within {GAMMA_MIN} standard deviations of the target: max |PI| = {np.max(np.abs(ref.gamma[acq])):.2e}')
  return out


def gram_fraction(case):
  """Condition 4 (stationary kernels with at least two observations): the fraction of off-diagonal pairs of the observations whose
  Gram entry lies strictly inside (0.01, 1) * signal variance."""
  s = oracle_setup(case)
  k = s.ko(s.po, s.x, warp_func=WFO)
  sv = float(np.squeeze(o.retrieve_params(s.po, ['signal_variance'], WFO)[0]))
  off = k[~np.eye(case.n, dtype=bool)]
  return float(np.mean((off > 0.01 * sv) & (off < sv)))


# ---- the device's route restated, and its mutants --------------------------------------------------------------------------------
class Parts(NamedTuple):
  acts_q: object     # MLP activations of the queries (acts[0]: the input), or None
  fq: np.ndarray     # kernel features of the queries
  fo: object         # kernel features of the observations
  mu0: np.ndarray
  kdiag: np.ndarray
  kxq: object        # (n, M)
  alpha: object
  W: object          # L^-1, lower triangular (K^-1 = W^T W)


@functools.lru_cache(maxsize=None)
def parts(case):
  s = oracle_setup(case)
  model = s.po.model
  acts_q = o._mlp_forward_cache(model['mlp_params'], s.xq) if case.feats else None
  fq = acts_q[-1] if case.mlp_k else s.xq
  mu0 = np.asarray(s.mo(s.po, s.xq, warp_func=WFO), dtype=np.float64)[:, 0]
  kdiag = np.asarray(s.ko(s.po, s.xq, warp_func=WFO, diag=True), dtype=np.float64)
  if not case.n:
    return Parts(acts_q, fq, None, mu0, kdiag, None, None, None)
  chol, kinvy, _ = o.solve_gp_linear_system(s.mo, s.ko, s.po, s.x, s.y, WFO)
  fo = o.mlp_apply(model['mlp_params'], s.x) if case.mlp_k else s.x
  W = spla.solve_triangular(chol, np.eye(case.n), lower=True, check_finite=False)
  return Parts(acts_q, fq, fo, mu0, kdiag, np.asarray(s.ko(s.po, s.x, s.xq, warp_func=WFO), dtype=np.float64), kinvy[:, 0], W)


def route(case, acq, param, l=None, beta=None, fmask=None, rowmask=None, chain=None, skip_tanh=None):
  """Value (M,) and gradient (M, d) by the device's route: l = W k, beta = W^T l, mu = k . alpha + m(x), var = k(x, x) - |l|^2,
  coef = a_mu alpha - 2 a_var beta, the feature gradient, the MLP backward, the mean part, dw/dx.  The keyword arguments are the
  mutants' handles: another l / beta, features that contribute nothing to u or g (fmask: 0 / 1 per feature), observation rows the
  feature reduction drops (rowmask: 0 / 1 per row), another dw/dx, an MLP layer whose tanh' is skipped."""
  s, p = oracle_setup(case), parts(case)
  model = s.po.model
  if case.n:
    l = p.W @ p.kxq if l is None else l
    beta = p.W.T @ l if beta is None else beta
    mu, var = p.kxq.T @ p.alpha + p.mu0, p.kdiag - np.sum(l * l, axis=0)
  else:
    mu, var = p.mu0, p.kdiag
  with np.errstate(invalid='ignore'):     # a mutant may leave a negative variance: NaN, infinitely far from the reference
    sd = np.sqrt((var + s.noise) * SCALE)
  if acq == 'ei':
    u = (mu - param) / sd
    val, a_mu, a_sd = sd * (o._norm_pdf(u) + u * o._norm_cdf(u)), o._norm_cdf(u), o._norm_pdf(u)
  elif acq == 'pi':
    val, a_mu, a_sd = (mu - param) / sd, 1.0 / sd, -(mu - param) / sd**2
  else:
    val, a_mu, a_sd = mu + param * sd, np.ones_like(mu), np.full_like(mu, param)
  a_var = a_sd / (2 * sd) * SCALE
  fm = np.ones(p.fq.shape[1]) if fmask is None else fmask
  gfeat = np.zeros_like(p.fq)
  if case.n:
    coef = (a_mu[None, :] * p.alpha[:, None] - 2.0 * a_var[None, :] * beta).T      # (M, n)
    if rowmask is not None:
      coef = coef * rowmask[None, :]
  if case.kname == 'dot_product':
    s2 = float(np.squeeze(o.retrieve_params(s.po, ['dot_prod_sigma'], WFO)[0]))**2
    gfeat += (a_var * 2.0 / s2)[:, None] * p.fq
    if case.n:
      gfeat += coef @ p.fo / s2
    gfeat *= fm
  elif case.n:
    ls, sv = o.retrieve_params(s.po, ['lengthscale', 'signal_variance'], WFO)
    ls = np.broadcast_to(np.asarray(ls, dtype=np.float64).reshape(-1), (p.fq.shape[1],)); sv = float(np.squeeze(sv))
    diff = p.fq[:, None, :] - p.fo[None, :, :]
    u2 = np.sum((diff / ls)**2 * fm, axis=-1)
    if case.kname == 'squared_exponential':
      dk = -0.5 * sv * np.exp(-u2 / 2)
    elif case.kname == 'matern32':
      dk = np.where(u2 == 0, 0.0, -sv * 1.5 * np.exp(-np.sqrt(3.0 * u2)))
    else:
      rr = np.sqrt(5.0 * u2); dk = np.where(u2 == 0, 0.0, -sv * 5.0 * np.exp(-rr) * (1 + rr) / 6)
    gfeat += 2.0 * np.einsum('qi,qid->qd', coef * dk, diff) / ls**2 * fm
  grad = np.zeros((case.M, case.d))
  gmlp = np.zeros_like(p.acts_q[-1]) if case.feats else None
  if case.mlp_k:
    gmlp += gfeat
  else:
    grad += gfeat
  if case.kumar:
    grad *= s.chain if chain is None else chain
  if case.mname == 'linear':
    grad += a_mu[:, None] * np.asarray(model['linear_mean']['kernel'], dtype=np.float64)[:, 0][None, :]
  elif case.mname == 'linear_mlp':
    gmlp += a_mu[:, None] * np.asarray(model['linear_mean']['kernel'], dtype=np.float64)[:, 0][None, :]
  if case.feats:
    g = gmlp
    for layer in range(len(case.feats) - 1, -1, -1):
      out = p.acts_q[layer + 1]
      dz = g if layer == skip_tanh else g * (1.0 - out * out)
      g = dz @ np.asarray(model['mlp_params'][f'Dense_{layer}']['kernel'], dtype=np.float64).T
    grad += g
  return val, grad


def groups_of_reduction(case):
  """G of acq_grad_kernel: 256 / next_pow2(feature width) groups stride the observation rows."""
  fd = 1
  while fd < case.fdim:
    fd *= 2
  return 256 // fd


def mutant_a(case, acq, param):
  """Features from index 64 up contribute nothing to u or to g."""
  return route(case, acq, param, fmask=(np.arange(case.fdim) < 64).astype(np.float64))


def mutant_b(case, acq, param):
  """The last group of the feature reduction is dropped: within every 256 rows, every G-th observation row from G - 1 on."""
  g = groups_of_reduction(case)
  return route(case, acq, param, rowmask=((np.arange(case.n) % 256) % g != g - 1).astype(np.float64))


def mutant_c(case, acq, param):
  """beta = W^T l misses the observation rows of the last 256-row chunk when npad is an odd multiple of 128 (the half chunk)."""
  p = parts(case)
  cut = case.npad - 128
  l = p.W @ p.kxq
  return route(case, acq, param, l=l, beta=p.W[:cut].T @ l[:cut])


def mutant_d(case, acq, param):
  """Right-hand side 8 (the ninth query) takes the eighth's l and beta."""
  p = parts(case)
  l = p.W @ p.kxq
  beta = p.W.T @ l
  l[:, 8], beta[:, 8] = l[:, 7].copy(), beta[:, 7].copy()
  return route(case, acq, param, l=l, beta=beta)


def mutant_e(case, acq, param):
  """Queries from 1024 on get the value and gradient of query q - 1024 (a second pass that reads the first pass's workspaces)."""
  ref = reference(case)
  val, grad = ref.val[acq].copy(), ref.grad[acq].copy()
  val[1024:], grad[1024:] = val[:case.M - 1024].copy(), grad[:case.M - 1024].copy()
  return val, grad


def mutant_f(case, acq, param):
  """M = 1: the forward product l = W k leaves out the diagonal term of W."""
  p = parts(case)
  l = np.tril(p.W, -1) @ p.kxq
  return route(case, acq, param, l=l, beta=p.W.T @ l)


def mutant_g(case, acq, param):
  """dw/dx of the Kumaraswamy chain is taken with a[0], b[0] for every column."""
  kp = inputs(case)[0]['kumar_params']
  a, b = kumar_oracle.squareplus(np.float64(kp['a'][0])), kumar_oracle.squareplus(np.float64(kp['b'][0]))
  return route(case, acq, param, chain=kumar_oracle.dw_dx(inputs(case)[3].astype(np.float64), a, b))


def mutant_h(case, acq, param):
  """The MLP backward skips the tanh' factor of the widest hidden layer."""
  return route(case, acq, param, skip_tanh=int(np.argmax(case.feats[:-1])))


MUTANTS = {'a': mutant_a, 'b': mutant_b, 'c': mutant_c, 'd': mutant_d, 'e': mutant_e, 'f': mutant_f, 'g': mutant_g, 'h': mutant_h}


# Mutants that exist at an fp32 case's shape but stay inside its fp32 bounds: (group, kernel, length-scale form, n, M, d) -> letters, from
# a pass over all 219 fp32 cases (the host test judges a sub-sample that holds every entry, and asserts that each IS inside the bound,
# so that the list stays true).  All of them are (c), beta without the observation rows of the half last chunk, where those rows
# carry little: one row at n = 257 (npad 384, row 256) and n = 513 (npad 640, row 512), 0.01 .. 0.22 of the bound; rows 256 .. 299 of
# n = 300 at d = 1 and 2, where 256 observations already fix the posterior on a line or a square, 0.15 .. 0.88 of the bound.  The fp64
# twin of every entry sees (c) by more than MUTANT_FACTOR bounds; in fp32 the half chunk is seen at every other width of A (>= 1.27
# bounds) and at n = 383, 384 of D.
FP32_BLIND = {('A', 'squared_exponential', 'scalar', 300, 9, 1): 'c', ('A', 'matern52', 'ard', 300, 9, 1): 'c',
              ('A', 'dot_product', 'none', 300, 9, 1): 'c', ('A', 'squared_exponential', 'ard', 300, 9, 2): 'c',
              ('A', 'squared_exponential', 'scalar', 300, 9, 2): 'c', ('A', 'dot_product', 'none', 300, 9, 2): 'c',
              ('D', 'matern52', 'ard', 257, 9, 4): 'c', ('D', 'dot_product', 'none', 257, 9, 4): 'c',
              ('D', 'matern52', 'ard', 513, 9, 4): 'c', ('D', 'dot_product', 'none', 513, 9, 4): 'c'}


def fp32_blind(case):
  return set(FP32_BLIND.get((case.group, case.kname, case.ls, case.n, case.M, case.d), '')) if case.dtype == 'fp32' else set()


def not_applicable(case):
  """Mutants whose failure cannot exist at the case's shape, by the shape alone."""
  na = set()
  if case.fdim <= 64 or (case.n == 0 and case.kname != 'dot_product'):
    na.add('a')      # no feature 64; a stationary kernel on the prior branch has no kernel term
  if case.n < groups_of_reduction(case):
    na.add('b')      # no observation row reaches the last group (the first one is row G - 1)
  if case.n == 0 or case.M < 2 or (case.npad // 128) % 2 == 0:
    na.add('c')      # M = 1 takes tri_matvec_kernel (no chunks); an even number of 128-row blocks has no half chunk
  if case.n == 0 or case.M < 9:
    na.add('d')      # no ninth right-hand side
  if case.M <= 1024:
    na.add('e')      # one pass
  if case.n == 0 or case.M != 1:
    na.add('f')      # M >= 2 takes the tri_matmat kernels
  if not case.kumar or case.d == 1:
    na.add('g')      # no second column
  if len(case.feats) < 2:
    na.add('h')      # no hidden layer
  return na
