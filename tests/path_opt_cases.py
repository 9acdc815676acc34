"""CPU side of the path-gradient / path-maximiser tier (hbo_sample_paths_grad, hbo_paths_maximize; csrc/path_opt.hip).  Shared by
tests/test_path_opt_host.py (this file judged on its own, on the CPU) and tests/test_gpu_path_opt.py (the device against it).  Built on
pathwise_cases (problem, restate, draws, the bounds' constants) and acq_opt_oracle (the optimiser's defaults):

  CASES                  n in {0, 1, 127, 128, 129, 300} and 255 / 256 / 257 around the kernel's observation tile (OBS_TILE); F in
                         {1, 63, 64, 65, 200} and one below / at / one above the kernel's feature tile (feature_tile(D): 256 at D <= 16,
                         16 at D = 256); D in {1, 3, 17, 33, 256}; S in {1, 3, 9}; R in {1, 5}; the four kernels with a scalar and a
                         per-dimension lengthscale; means zero, constant, linear; dev_scale in {1, sqrt(1.5)}; fp64 and fp32.  Six
                         queries each: one that coincides with an observation (the Matern zero-distance rule), the box corners 0 and 1
                         and a mixed corner, two interior points
  restate_vg(...)        value and gradient of every (query, path) pair by the formulas of include/hbo.h, analytically, in float32,
                         float64 or np.longdouble, and the formula mutants
  bounds                 values: pathwise_cases' (fp64 1e-9 per column; fp32 REL_FACTOR x the float32 restatement's own error + FLOOR_C
                         eps32).  Gradients, per (query, path): max_d |g - g_ref| over that path's largest max_d |g_ref| over the case's
                         queries -- fp64: FP64_GRAD_BOUND; fp32: the same REL_FACTOR / FLOOR_C rule on the same measure
"""
import functools
from typing import NamedTuple

import numpy as np

import acq_opt_oracle as ao
import helpers
import pathwise_cases as pc
from oracle import hyperbo_oracle as o

WFO = pc.WFO
LD = pc.LD
OBS_TILE = 256              # csrc/path_opt.hip: PO_OT
OPT_DEFAULTS = ao.DEFAULTS  # the optimiser is hbo_acq_maximize's
SQRT15 = float(np.sqrt(1.5))

# fp64 gradients: 10 x the largest ratio measured on an MI355X over the fp64 cases (the project's rule for gradient tolerances),
# rounded up to one significant digit; the ratios per case are in profiles/path_maximize.md and in tests/test_gpu_path_opt.py.
FP64_GRAD_BOUND = 2e-12
MUTANT_FACTOR = pc.MUTANT_FACTOR


def feature_tile(d):
  """csrc/path_opt.hip: path_opt_feature_tile -- the largest power of two in 16..256 with tile x D <= 4096."""
  ft = 256
  while ft > 16 and ft * d > 4096:
    ft //= 2
  return ft


class Case(NamedTuple):
  kname: str
  ls: str                    # 'scalar' or 'ard' (the dot product has no lengthscale: the label only counts it)
  mname: str
  n: int
  F: int                     # (the dot product: d + 1)
  S: int
  d: int
  R: int
  dev: float                 # dev_scale
  dtype: str = 'fp64'

  @property
  def id(self):
    return f'{self.kname}-{self.ls}+{self.mname}-n{self.n}-F{self.F}-S{self.S}-D{self.d}-R{self.R}-c{self.dev:.3f}-{self.dtype}'

  @property
  def np_dtype(self):
    return np.float64 if self.dtype == 'fp64' else np.float32

  @property
  def base(self):
    return pc.Case(self.kname, False, self.mname, False, self.n, N_QUERIES, self.F, self.S, self.d, self.dtype)


N_QUERIES = 6
_SHAPES = [
    Case('squared_exponential', 'scalar', 'constant', 1, 1, 1, 1, 1, 1.0),
    Case('matern32', 'ard', 'linear', 127, 63, 3, 3, 5, SQRT15),
    Case('matern52', 'scalar', 'zero', 128, 64, 9, 17, 1, 1.0),
    Case('squared_exponential', 'ard', 'linear', 129, 65, 3, 33, 5, SQRT15),
    Case('matern52', 'ard', 'constant', 300, 200, 3, 3, 1, SQRT15),
    Case('matern32', 'scalar', 'constant', 255, 255, 1, 3, 1, 1.0),               # one below both tiles (D = 3: 256 features)
    Case('squared_exponential', 'ard', 'zero', 256, 256, 3, 3, 5, SQRT15),        # at both tiles
    Case('matern52', 'ard', 'linear', 257, 257, 3, 1, 5, 1.0),                    # one above both tiles
    Case('matern32', 'ard', 'zero', 0, 200, 3, 3, 5, 1.0),                        # the prior branch
    Case('squared_exponential', 'scalar', 'linear', 129, 15, 3, 256, 1, SQRT15),  # D = 256: tiles of 16 features
    Case('matern52', 'scalar', 'constant', 1, 16, 1, 256, 5, 1.0),
    Case('matern32', 'ard', 'linear', 127, 17, 9, 256, 1, SQRT15),
    Case('dot_product', 'scalar', 'zero', 129, 4, 3, 3, 5, 1.0),
    Case('dot_product', 'ard', 'linear', 300, 18, 9, 17, 1, SQRT15),
    Case('dot_product', 'scalar', 'constant', 0, 4, 3, 3, 5, SQRT15),             # the prior branch, exact basis
]
CASES = _SHAPES + [c._replace(dtype='fp32') for c in _SHAPES]


@functools.lru_cache(maxsize=None)
def problem(case):
  """pathwise_cases.problem of the case's shape with one or D lengthscales of helpers.lengthscale and the draws made again over them, and the six
  queries: an observation, the corners 0, 1 and a mixed one, two interior points.  Everything in the model dtype; not to be written to."""
  base = case.base
  p = pc.problem(base)
  dt = case.np_dtype
  model = dict(p.model)
  om, ph, w, eps = p.omega, p.phase, p.w, p.eps
  if case.kname != 'dot_product':
    # helpers.lengthscale: one or D lengthscales around 0.5 sqrt(D), so that the update term does not vanish at D = 256
    model['lengthscale'] = np.ascontiguousarray(helpers.lengthscale(np.random.default_rng(pc.draw_seed(base) + [3]), case.d, case.ls), dtype=dt)
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=dt)
    om, ph, w, eps = [c(a) for a in pc.draws(np.random.default_rng(pc.draw_seed(base)), case.kname, case.d, pc.warped_lengthscale(model),
                                             case.F, case.S, case.n)]
  xq = np.array(p.xq)
  if case.n:
    xq[0] = p.x[0]
  xq[1], xq[2] = 0.0, 1.0
  xq[3] = (np.arange(case.d) % 2).astype(dt)
  return p._replace(model=model, xq=np.ascontiguousarray(xq, dtype=dt), omega=om, phase=ph, w=w, eps=eps)


# ---- value and gradient, restated ------------------------------------------------------------------------------------------------------
MUTANTS = {
    'sin_sign': "the sine's sign",
    'no_omega': 'omega left out of the prior gradient',
    'no_inv_ls2': '1 / ls^2 left out of the update gradient',
    'dot_two': '2 instead of 1 on the dot-product update term',
    'no_linear': 'the linear weight left out',
    'scale_mean': 'dev_scale applied to the mean',
    'noise_unscaled': 'dev_scale left off the noise draw',
    'drop_feature_tile': 'the last partial feature tile dropped',
    'drop_obs_tile': 'the last partial observation tile dropped',
    'matern_zero': "a Matern pair at zero distance contributes the NaN of sqrt's derivative at 0 instead of 0",
}


def not_applicable(case):
  """Mutants that cannot show at the case, by its shape and model alone."""
  na = set()
  dot = case.kname == 'dot_product'
  if dot:
    na |= {'sin_sign', 'no_omega', 'no_inv_ls2', 'drop_feature_tile', 'matern_zero'}
  else:
    na.add('dot_two')
  if case.n == 0:
    na |= {'no_inv_ls2', 'dot_two', 'noise_unscaled', 'drop_obs_tile', 'matern_zero'}
  if case.kname == 'squared_exponential':
    na.add('matern_zero')
  if case.mname != 'linear':
    na.add('no_linear')
  if case.dev == 1.0:
    na |= {'scale_mean', 'noise_unscaled'}
  if case.mname == 'zero':
    na.add('scale_mean')
  if case.F % feature_tile(case.d) == 0:
    na.add('drop_feature_tile')
  if case.n % OBS_TILE == 0:
    na.add('drop_obs_tile')
  return na


def _dk_du(kname, u, sv, wide):
  if kname == 'squared_exponential':
    return -sv * np.exp(-u / wide(2)) / wide(2)
  if kname == 'matern32':
    return -wide(1.5) * sv * np.exp(-np.sqrt(wide(3) * u))
  r = np.sqrt(wide(5) * u)
  return -(wide(5) / wide(6)) * sv * (wide(1) + r) * np.exp(-r)


def _chol(a, acc):
  """pathwise_cases.chol with every inner product accumulated in `acc` and rounded once to the dtype of a."""
  n, wide = a.shape[0], a.dtype.type
  c = np.zeros_like(a)
  ca = np.zeros(a.shape, dtype=acc)
  for j in range(n):
    v = a[j:, j].astype(acc) - ca[j:, :j] @ ca[j, :j]
    d = wide(np.sqrt(v[0]))
    c[j, j] = d
    c[j + 1:, j] = (v[1:] / acc(d)).astype(wide)
    ca[j:, j] = c[j:, j]
  return c


def _solve_lower(c, b, acc, trans=False):
  """pathwise_cases.solve_lower with every inner product accumulated in `acc` and rounded once."""
  n, wide = c.shape[0], b.dtype.type
  ca, ba = c.astype(acc), b.astype(acc)
  v = np.zeros_like(b)
  va = np.zeros(b.shape, dtype=acc)
  rows = range(n - 1, -1, -1) if trans else range(n)
  for i in rows:
    t = ca[i + 1:, i] @ va[i + 1:] if trans else ca[i, :i] @ va[:i]
    v[i] = ((ba[i] - t) / ca[i, i]).astype(wide)
    va[i] = v[i]
  return v


def restate_vg(case, wide, mutant=None):
  """(values [M, S], gradients [M, S, D]) of the case's paths at its queries, every array in `wide`."""
  assert mutant is None or mutant in MUTANTS
  prob = problem(case)
  po = pc._params(prob, wide)
  base, mo = getattr(o, prob.kname), getattr(o, prob.mname)
  x, y, xq = prob.x.astype(wide), prob.y.astype(wide), prob.xq.astype(wide)
  w = prob.w.astype(wide)
  n, d, M, S = x.shape[0], xq.shape[1], xq.shape[0], w.shape[1]
  dot = prob.kname == 'dot_product'
  c = wide(case.dev)
  cm = c if mutant == 'scale_mean' else wide(1)
  mean_q = np.asarray(mo(po, xq, warp_func=WFO), dtype=wide)
  g_mean = np.zeros(d, dtype=wide)
  if prob.mname == 'linear' and mutant != 'no_linear':
    g_mean = np.asarray(po.model['linear_mean']['kernel'], dtype=wide)[:, 0]
  # ---- the prior path and its gradient
  if dot:
    sigma, bias = [np.asarray(t, dtype=wide) for t in o.retrieve_params(po, ['dot_prod_sigma', 'dot_prod_bias'], WFO)]
    prior = lambda v: (v / sigma) @ w[:-1] + bias * w[-1][None, :]
    g_prior = np.broadcast_to((w[:-1] / sigma).T[None], (M, S, d))                       # [M, S, D]
  else:
    sv, ls = [np.asarray(t, dtype=wide) for t in o.retrieve_params(po, ['signal_variance', 'lengthscale'], WFO)]
    ls = np.broadcast_to(np.reshape(ls, (-1,)), (d,))
    om, ph = prob.omega.astype(wide), prob.phase.astype(wide)
    F = om.shape[0]
    keep = F // feature_tile(d) * feature_tile(d) if mutant == 'drop_feature_tile' else F
    amp = np.sqrt(wide(2) * sv / wide(F))
    prior = lambda v: amp * (np.cos(v @ om[:keep].T + ph[None, :keep]) @ w[:keep])
    sn = np.sin(xq @ om[:keep].T + ph[None, :keep])                                         # [M, F]
    sign = wide(1) if mutant == 'sin_sign' else wide(-1)
    omg = np.ones_like(om[:keep]) if mutant == 'no_omega' else om[:keep]
    g_prior = sign * amp * np.einsum('mj,js,jd->msd', sn, w[:keep], omg)
  val = cm * mean_q + c * prior(xq)
  grad = cm * g_mean[None, None, :] + c * g_prior
  assert val.dtype == wide and grad.dtype == wide, (val.dtype, grad.dtype)
  if n == 0:
    return val, np.array(grad)
  # ---- u = Ktilde^-1 (y - m(X) - c p(X) - c sqrt(noise + eps) eps)
  noise = np.asarray(o.retrieve_params(po, ['noise_variance'], WFO)[0], dtype=wide)
  kt = base(po, x, warp_func=WFO) + np.eye(n, dtype=wide) * (noise + wide(pc.EPS))
  cn = wide(1) if mutant == 'noise_unscaled' else c
  r = (y - np.asarray(mo(po, x, warp_func=WFO), dtype=wide)) - c * prior(x) - cn * np.sqrt(noise + wide(pc.EPS)) * prob.eps.astype(wide)
  # float64: the inner products of the factorisation and of the substitutions are accumulated in longdouble and rounded once.  Summed
  # by the host's BLAS they are machine-dependent at the level test_path_opt_host.py looks at (the n = 300 dot-product case gave
  # 2.1e-13 on one host and 2.3e-13 on another against FP64_GRAD_BOUND / 10), and a check must not turn on a SIMD width.  The float32
  # restatement stays as pathwise_cases has it: its own error is what the fp32 bounds are made of.
  if wide == np.float64:
    ch = _chol(kt, LD)
    u = _solve_lower(ch, _solve_lower(ch, r, LD), LD, trans=True)                         # [n, S]
  else:
    ch = pc.chol(kt)
    u = pc.solve_lower(ch, pc.solve_lower(ch, r), trans=True)
  keep_n = n // OBS_TILE * OBS_TILE if mutant == 'drop_obs_tile' else n
  kxq = base(po, x, xq, warp_func=WFO)                                                    # [n, M]
  val = val + kxq[:keep_n].T @ u[:keep_n]
  diff = xq[:, None, :] - x[None, :keep_n, :]                                             # [M, n, D]
  if dot:
    two = wide(2) if mutant == 'dot_two' else wide(1)
    g_up = two * np.einsum('is,id->sd', u[:keep_n], x[:keep_n])[None] / (sigma * sigma)
  else:
    dist = np.sum((diff / ls[None, None, :]) ** 2, axis=2)                                # [M, n]
    dk = _dk_du(prob.kname, dist, sv, wide)
    if mutant == 'matern_zero':
      dk = np.where(dist == 0, wide(np.nan), dk)
    il2 = np.ones(d, dtype=wide) if mutant == 'no_inv_ls2' else wide(1) / (ls * ls)
    g_up = wide(2) * np.einsum('mi,is,mid->msd', dk, u[:keep_n], diff) * il2[None, None, :]
  grad = grad + g_up
  assert val.dtype == wide and grad.dtype == wide, (val.dtype, grad.dtype)
  return val, grad


@functools.lru_cache(maxsize=None)
def reference(case):
  """The longdouble restatement of the case (values, gradients): shared, not to be written to."""
  return restate_vg(case, LD)


# ---- measures and bounds ----------------------------------------------------------------------------------------------------------------
def grad_errors(got, ref):
  """[M, S]: max_d |g - g_ref| over the path's largest max_d |g_ref| over the queries; inf where `got` is not finite."""
  got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
  assert got.shape == ref.shape, (got.shape, ref.shape)
  scale = np.max(np.abs(ref), axis=(0, 2))                                                # [S]
  err = np.max(np.abs(got - ref), axis=2) / (scale[None, :] + LD(1e-300))
  return np.where(np.isfinite(got).all(axis=2), err, np.inf).astype(np.float64)


@functools.lru_cache(maxsize=None)
def f32_levels(case):
  """(values, gradients): the float32 restatement's error against longdouble, the largest over the case."""
  v32, g32 = restate_vg(case, np.float32)
  v, g = reference(case)
  return float(np.max(pc.col_errors(v32, v))), float(np.max(grad_errors(g32, g)))


def value_bound(case):
  """pathwise_cases.bound for these cases: helpers.rel_err per column."""
  if case.dtype == 'fp64':
    return pc.FP64_BOUND
  return pc.REL_FACTOR * f32_levels(case)[0] + pc.FLOOR_C * float(np.finfo(np.float32).eps)


def grad_bound(case):
  if case.dtype == 'fp64':
    return FP64_GRAD_BOUND
  return pc.REL_FACTOR * f32_levels(case)[1] + pc.FLOOR_C * float(np.finfo(np.float32).eps)


# ---- linear paths: the maximiser is a corner ------------------------------------------------------------------------------------------
# (the fp32 form of the n = 300, D = 17 case is left out by the rule below: its float32 restatement is 8e-4 off, a value bound of 3e-3,
#  and no gradient component of any of its paths is 1e3 such bounds from 0 -- test_path_opt_host.py checks that this is so)
LINEAR_LEFT_OUT = [c for c in CASES if c.kname == 'dot_product' and c.dtype == 'fp32' and c.n == 300]
LINEAR_CASES = [c for c in CASES if c.kname == 'dot_product' and c not in LINEAR_LEFT_OUT]
CORNER_MARGIN = 1e3         # every gradient component at least this many value bounds away from 0
# A linear f leaves the optimiser no curvature pair (y = 0): it walks by projected steepest descent with unit steps, coordinate d
# moving |g_d| per iteration, so a corner at distance <= 1 takes up to 1 / |g_d| iterations.  The corner test gives every pair
# CORNER_EVALS evaluations (and as many iterations) and takes the paths whose smallest |g_d| leaves a factor 4 of room.
CORNER_EVALS = 1024
CORNER_MIN_GRAD = 4.0 / CORNER_EVALS


def linear_corner(case):
  """(corner [S, D] of [0, 1]^D by the signs of the constant gradient, margin [S]: the path's smallest |g_d| over its largest |value|,
  chosen [S]: the paths of the corner test): a dot product with a zero, constant or linear mean makes f_s linear in x."""
  v, g = reference(case)
  v, g = np.asarray(v, dtype=np.float64), np.asarray(g, dtype=np.float64)
  g0 = g[4]                                                                               # [S, D] at an interior query
  assert np.max(np.abs(g - g0[None])) <= 1e-12 * np.max(np.abs(g0)), 'the path is not linear'
  small = np.min(np.abs(g0), axis=1)
  margin = small / np.max(np.abs(v), axis=0)
  chosen = (margin >= CORNER_MARGIN * value_bound(case)) & (small >= CORNER_MIN_GRAD)
  return (g0 > 0).astype(np.float64), margin, chosen
