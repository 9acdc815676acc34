"""CPU side of the tests of log expected improvement (csrc/kernfun.h: logei_terms, logei_scalars; csrc/logei.hip: hbo_acq_logei,
hbo_logei_grad_samples, hbo_logei_maximize; acfun.LogExpectedImprovement).  Shared by tests/test_logei_cases_host.py (this file judged
on its own, no device) and tests/test_gpu_logei.py (the device against it).

  exact_terms(u)        log h, cdf / h, pdf / h (h = pdf + u cdf) from mpmath, at a precision raised until doubling it changes nothing
  stable_terms(u)       the float64 restatement of logei_terms (SciPy erfc / erfcx, the series beyond SERIES_U): what the device evaluates
  C_VALUE, C_CDF, C_PDF that restatement's worst error against mpmath over a dense u grid, in units of eps64 (1 + u^2) -- absolute for
                        log h, relative for the two ratios (test_logei_cases_host.py::test_restatement_against_mpmath measures them);
                        the device gets mes_cases.DEVICE_FACTOR = 8 times them
  scalars / exact_scalars   value, a_mu, a_var of one query: float64 (with a mutant on request) / mpmath, with the device's bounds
  combine / exact_combine   the S-sample rule (log of the mean of the samples' EI), float64 (with the mutant) / mpmath
  oracle_value_and_grad     per-sample LogEI value + d value / d x from the oracle's posterior and its derivative
  value_bound, grad_tol the bounds of the GPU tier
  MUTANTS               one failure each
  CASES, problem        the shapes of the GPU tier
  flat_tail_problem     the start on which EI's maximiser stops without moving and LogEI's does not
"""
import functools
import types
from typing import NamedTuple

import mpmath as mp
import numpy as np
from scipy import special

import helpers
import mes_cases as mc
from oracle import hyperbo_oracle as o

WFO = o.DEFAULT_WARP_FUNC
EPS64, EPS32 = mc.EPS64, mc.EPS32
SCALE = mc.SCALE
DEVICE_FACTOR = mc.DEVICE_FACTOR
QUANTUM = mc.QUANTUM
U = (-3e7, -1e5, -1e3, -38.0, -8.0, -3.0, -1.0 - 2.0**-40, -1.0, -0.999, 0.0, 0.7, 3.0, 8.3, 38.0, 40.0, 1e3)
SERIES_U = 256.0                  # csrc/kernfun.h: LOGEI_SERIES_U (profiles/logei_errors.md: why not the 2^25 the cancellation allows)
# measured by test_restatement_against_mpmath (which asserts measured <= C <= 2 * measured): 3.15 (u = -1.68), 3.78 (u = -1.03) and
# 3.11 (u = -1.68); a grid five times as dense gave 3.13, 4.44 and 3.29
C_VALUE, C_CDF, C_PDF = 4.0, 5.0, 4.0


def unit(u):
  """One unit of the three constants at u: eps64 (1 + u^2)."""
  return EPS64 * (1.0 + float(u) * float(u))


def pdf_quantum(u):
  """The absolute share of pdf / h where pdf(u) is a denormal (u > 37.6): pdf is then good to half a quantum, not to eps, the quotient by
  h ~ u > 37 is smaller still and is itself stored to half a quantum: two quanta cover both (mes_cases.QUANTUM)."""
  return 2.0 * QUANTUM if u > 37.6 else 0.0


# ---- the reference --------------------------------------------------------------------------------------------------------------
def _mp_terms(u, dps):
  with mp.workdps(dps):
    u = mp.mpf(u)
    p, c = mp.npdf(u), mp.ncdf(u)
    h = p + u * c
    return mp.log(h), c / h, p / h


@functools.lru_cache(maxsize=None)
def exact_terms(u):
  """(log h, cdf / h, pdf / h) at u as floats, correctly rounded: the precision is doubled from 60 digits until two successive results
  agree to 1e-25 relatively (h cancels to 1 / u^2 of its terms: at u = -3e7 that is 15 digits).  u = +-inf: the limits."""
  u = float(u)
  if u == np.inf:
    return np.inf, 0.0, 0.0
  if u == -np.inf:
    return -np.inf, np.inf, np.inf
  dps, prev = 60, None
  while True:
    cur = _mp_terms(u, dps)
    if prev is not None and all(abs(a - b) <= mp.mpf(10)**-25 * abs(b) for a, b in zip(prev, cur)):
      return tuple(float(v) for v in cur)
    prev, dps = cur, 2 * dps
    assert dps <= 7680, u


def stable_terms(u, mutant=None):
  """(log h, cdf / h, pdf / h) in float64, elementwise, as csrc/kernfun.h: logei_terms evaluates them.  Mutants: 'mills_sign' (w = 1 - u m),
  'no_series' (the erfcx form at every u <= -1), 'literal_log' (the literal form at every u, h floored at 0 as ei_over_sd floors it)."""
  u = np.asarray(u, dtype=np.float64)
  logh, cdf_h, pdf_h = (np.full(u.shape, np.nan) for _ in range(3))
  with np.errstate(all='ignore'):
    hi = (u > -1.0) | ((mutant == 'literal_log') & ~np.isnan(u))
    far = (u < -SERIES_U) & ~hi & (mutant != 'no_series')
    mid = ~hi & ~far & ~np.isnan(u)
    x = u[hi]
    p, c = np.exp(-0.5 * x * x) * 0.3989422804014327, 0.5 * special.erfc(-x * 0.7071067811865476)
    h = p + x * c
    if mutant == 'literal_log':
      h = np.maximum(h, 0.0)
    logh[hi], cdf_h[hi], pdf_h[hi] = np.log(h), c / h, p / h
    x = u[mid]
    m = 1.2533141373155003 * special.erfcx(-x * 0.7071067811865476)
    w = 1.0 - x * m if mutant == 'mills_sign' else 1.0 + x * m
    logh[mid], cdf_h[mid], pdf_h[mid] = -0.5 * x * x - 0.9189385332046727 + np.log(w), m / w, 1.0 / w
    x = u[far]
    i2 = 1.0 / (x * x)
    ws = 1.0 + i2 * (-3.0 + i2 * (15.0 - 105.0 * i2))
    ms = 1.0 + i2 * (-1.0 + i2 * (3.0 - 15.0 * i2))
    logh[far], cdf_h[far], pdf_h[far] = -0.5 * x * x - 0.9189385332046727 + (np.log(ws) - 2.0 * np.log(-x)), -x * (ms / ws), x * x / ws
  return logh, cdf_h, pdf_h


def term_ratios(u, got):
  """The errors of (log h, cdf / h, pdf / h) `got` at u against exact_terms in units of C_VALUE, C_CDF, C_PDF times unit(u) (pdf / h: plus
  its quantum); inf for a result that is not finite where the exact one is."""
  e = exact_terms(u)
  out = []
  for i, c in enumerate((C_VALUE, C_CDF, C_PDF)):
    g = float(got[i])
    if not np.isfinite(g):
      out.append(0.0 if g == e[i] else np.inf)
      continue
    b = c * unit(u) * (1.0 if i == 0 else abs(e[i])) + (pdf_quantum(u) if i == 2 else 0.0)
    out.append(abs(g - e[i]) / b)
  return out


# ---- the scalar step of one query ---------------------------------------------------------------------------------------------------
def scalars(mu, var, add_noise, scale, target, mutant=None):
  """(value, a_mu, a_var) of one query in float64, as include/hbo.h states them.  mutant: a key of MUTANTS."""
  v2 = (var + add_noise) * scale
  d = mu - target
  with np.errstate(all='ignore'):
    if v2 <= 0.0 and mutant != 'no_v2_rule':
      if d > 0.0:
        return float(np.log(d)), float(1.0 / d), 0.0
      return (-np.inf, 0.0, 0.0) if d <= 0.0 else (np.nan, np.nan, 0.0)
    sd = np.sqrt(v2)
    logh, cdf_h, pdf_h = (float(t) for t in stable_terms(np.float64(d) / sd, mutant))
    val = logh if mutant == 'no_log_sd' else float(np.log(sd)) + logh
    amu = cdf_h / sd
    asd = (cdf_h if mutant == 'asd_is_cdf' else pdf_h) / sd
    avar = asd / (2.0 * sd) * (1.0 if mutant == 'scale_dropped' else scale)
    if val == -np.inf:
      amu, avar = 0.0, 0.0
  return float(val), float(amu), float(avar)


def exact_scalars(mu, var, add_noise, scale, target, factor=DEVICE_FACTOR):
  """scalars() from exact_terms, with the absolute bounds of the device's three results beside them:
  ((value, a_mu, a_var), (b_value, b_amu, b_avar)).  The value adds the rounding of log sd, eps64 |log sd|, under the same factor."""
  v2 = (var + add_noise) * scale
  d = mu - target
  if v2 <= 0.0:
    if d > 0.0:
      return (float(np.log(d)), 1.0 / d, 0.0), (factor * EPS64 * (1.0 + abs(np.log(d))), factor * EPS64 / d, 0.0)
    return (-np.inf, 0.0, 0.0), (0.0, 0.0, 0.0)
  sd = float(np.sqrt(v2))
  u = d / sd
  logh, cdf_h, pdf_h = exact_terms(u)
  f = scale / (2.0 * sd * sd)
  val = float(mp.log(mp.mpf(sd)) + mp.mpf(logh))
  if val == -np.inf:
    return (val, 0.0, 0.0), (0.0, 0.0, 0.0)
  bv = factor * (C_VALUE * unit(u) + EPS64 * abs(np.log(sd)))
  bm = factor * C_CDF * unit(u) * cdf_h / sd
  bs = factor * (C_PDF * unit(u) * pdf_h + pdf_quantum(u)) * f
  return (val, cdf_h / sd, pdf_h * f), (bv, bm, bs)


def combine(vals, grads=None, mutant=None):
  """The acquisition over S samples from per-sample values [S] and gradients [S, D], float64, sums in sample order (include/hbo.h).
  mutant 'mean_of_logs': the mean taken outside the log."""
  v = np.asarray(vals, dtype=np.float64)
  g = None if grads is None else np.asarray(grads, dtype=np.float64)
  s_count = v.shape[0]
  if mutant == 'mean_of_logs':
    return (float(np.sum(v) / s_count),) + (() if g is None else (np.sum(g, axis=0) / s_count,))
  if np.isnan(v).any():
    return (np.nan,) + (() if g is None else (np.full(g.shape[1], np.nan),))
  m = float(np.max(v))
  if m == -np.inf:
    return (-np.inf,) + (() if g is None else (np.zeros(g.shape[1]),))
  sw, sg = 0.0, (None if g is None else np.zeros(g.shape[1]))
  for s in range(s_count):
    w = float(np.exp(v[s] - m))
    sw = sw + w
    if g is not None:
      sg = sg + w * g[s]
  val = m + float(np.log(sw / s_count))
  return (val,) + (() if g is None else (sg / sw,))


def exact_combine(vals, grads=None):
  """combine() in mpmath (60 digits) from float inputs: (value, gradient or None)."""
  with mp.workdps(60):
    v = [mp.mpf(float(x)) if np.isfinite(x) else (mp.ninf if x == -np.inf else mp.nan) for x in vals]
    if any(mp.isnan(x) for x in v):
      return np.nan, None
    m = max(v)
    if m == mp.ninf:
      return -np.inf, (None if grads is None else np.zeros(np.shape(grads)[1]))
    w = [mp.exp(x - m) if x != mp.ninf else mp.mpf(0) for x in v]
    sw = sum(w)
    val = float(m + mp.log(sw / len(v)))
    if grads is None:
      return val, None
    g = np.asarray(grads, dtype=np.float64)
    return val, np.array([float(sum(w[s] * mp.mpf(float(g[s, i])) for s in range(len(v))) / sw) for i in range(g.shape[1])])


MUTANTS = ('literal_log', 'no_log_sd', 'mills_sign', 'asd_is_cdf', 'scale_dropped', 'no_v2_rule', 'no_series', 'mean_of_logs')

# (mu, var, add_noise, scale, u of the target): the scalar-step cases the mutants are judged on; every u of U, two beyond the point
# where 1 + u m rounds to 0 (|u| = 6.7e7), and the v2 <= 0 rule from both sides of the target
SCALAR_CASES = [(0.3, 0.8, 0.0, SCALE, u) for u in U] + [
    (-1.2, 0.05, 0.01, SCALE, -1e8),
    (0.1, 0.4, 0.0, 1.0, -1e12),
    (0.0, 2.0, 0.1, SCALE, -5.0),
    (0.5, 0.0, 0.0, SCALE, 1.0),                  # v2 = 0, mu above the target
    (0.5, 0.0, 0.0, SCALE, -1.0),                 # v2 = 0, mu below it
    (0.5, 0.2, -0.3, SCALE, 2.0),                 # v2 < 0
]
# (values [S], the sample whose row is -inf or None): the cases 'mean_of_logs' is judged on
COMBINE_CASES = [([-3.0, -40.0, -5.5], None), ([-700.0, -2.0], None), ([0.25], None), ([-1.0, -np.inf, -2.0], 1), ([-np.inf, -np.inf], 0)]


def scalar_case_target(case):
  mu, var, noise, scale, u = case
  v2 = (var + noise) * scale
  return mu - u * (np.sqrt(v2) if v2 > 0 else 1.0)


# ---- the cases of the GPU tier ----------------------------------------------------------------------------------------------------
class Case(NamedTuple):
  kname: str
  mname: str
  ns: tuple       # observations per sample (S = len(ns))
  d: int
  M: int
  dtype: str
  feats: tuple = ()        # the MLP stack (mean and, with mlp_k, kernel)
  mlp_k: bool = False

  @property
  def id(self):
    f = ('-f' + 'x'.join(map(str, self.feats)) + ('k' if self.mlp_k else 'm')) if self.feats else ''
    return f'{self.kname}-{self.mname}-n{"_".join(map(str, self.ns))}-d{self.d}-M{self.M}{f}-{self.dtype}'

  @property
  def S(self):
    return len(self.ns)


CASES = [
    Case('squared_exponential', 'constant', (5,), 1, 7, 'fp64'),
    Case('matern32', 'zero', (128,), 3, 9, 'fp64'),
    Case('matern52', 'linear', (128, 128, 128), 17, 24, 'fp64'),
    Case('dot_product', 'constant', (129,), 3, 9, 'fp64'),
    Case('squared_exponential', 'linear', (300, 300, 300), 3, 9, 'fp64'),
    Case('matern32', 'constant', (5, 300, 129), 1, 9, 'fp64'),            # one call mixing one-block and blocked caches
    Case('dot_product', 'linear', (300,), 17, 5, 'fp64'),
    Case('matern52', 'linear_mlp', (128,), 3, 9, 'fp64', (8, 8), True),   # the one-launch route with the forward and backward pass
    Case('matern52', 'linear_mlp', (129,), 3, 9, 'fp64', (8, 8), True),   # five launches per chunk
    Case('squared_exponential', 'linear_mlp', (300,), 3, 9, 'fp64', (4, 5), False),   # a linear_mlp mean only
    Case('squared_exponential', 'constant', (128, 5, 129), 3, 9, 'fp32'),
    Case('matern52', 'linear', (129,), 17, 24, 'fp32'),
    Case('dot_product', 'zero', (300,), 1, 9, 'fp32'),
    Case('matern32', 'linear_mlp', (5,), 3, 9, 'fp32', (8, 8), True),
]
U0 = -2.0        # where query 0 of every sample sits; the other queries sit wherever their posterior puts them


def np_dtype(case):
  return np.float64 if case.dtype == 'fp64' else np.float32


def config(case):
  return {'mlp_features': tuple(case.feats)} if case.feats else {}


def _model(rng, case):
  if not case.feats:
    return helpers.make_model(rng, case.mname, False, case.d)
  model = helpers.mlp_model(rng, case.d, case.feats, case.kname, 'ard')
  if not case.mlp_k:      # the kernel sees the raw inputs
    model['lengthscale'] = helpers.lengthscale(rng, case.d, 'ard')
  return model


@functools.lru_cache(maxsize=None)
def problem(case, seed=83):
  """The S (model, observations) pairs of a case, the shared queries, the oracle's fp64 posterior on the same (dtype-rounded) numbers
  and targets t_s = mu_s(q0) - U0 sd_s(q0) (noise included, as hbo_logei_grad_samples is called).  No device.  Shared: do not write."""
  dt = np_dtype(case)
  rng = np.random.default_rng([seed, len(case.id), case.d, case.M, len(case.feats)])
  xq = np.ascontiguousarray(rng.uniform(size=(case.M, case.d)).astype(dt))
  smp = []
  for n in case.ns:
    model_t = mc._cast(_model(rng, case), dt)
    po = o.GPParams(model=mc._cast(model_t, np.float64), config=config(case))
    x, y = helpers.synthetic_task(rng, n, case.d, dtype=dt)
    smp.append(types.SimpleNamespace(model_t=model_t, po=po, x=x, y=y, ko=getattr(o, case.kname + ('_mlp' if case.mlp_k else '')),
                                     mo=getattr(o, case.mname), noise=float(np.squeeze(o.retrieve_params(po, ['noise_variance'], WFO)[0]))))
  p = types.SimpleNamespace(case=case, xq=xq, smp=smp, dtype=np.dtype(dt))
  for sm in smp:
    sm.mu, sm.var, sm.dmu, sm.dsd = mc.posterior(sm, xq, sm.noise, SCALE)
    sm.sd = np.sqrt((sm.var + sm.noise) * SCALE)
  p.targets = np.array([sm.mu[0] - U0 * sm.sd[0] for sm in smp])
  p.noises = [sm.noise for sm in smp]
  return p


def oracle_value_and_grad(sm, xq, target, add_noise=None, scale=SCALE, mutant=None):
  """(value [M], gradient [M, D], u [M]) of one sample's LogEI from the oracle's posterior and its derivative:
  d value / dx = a_mu d mu / dx + a_sd d sd / dx, a_sd = a_var * 2 sd / scale."""
  add_noise = sm.noise if add_noise is None else add_noise
  mu, var, dmu, dsd = mc.posterior(sm, xq, add_noise, scale)
  val, grad = np.zeros(mu.size), np.zeros_like(dmu)
  sd = np.sqrt((var + add_noise) * scale)
  for q in range(mu.size):
    v, amu, avar = scalars(mu[q], var[q], add_noise, scale, target, mutant)
    val[q], grad[q] = v, amu * dmu[q] + (avar * 2.0 * sd[q] / scale) * dsd[q]
  return val, grad, (mu - target) / sd


# ---- the bounds of the GPU tier -----------------------------------------------------------------------------------------------------
posterior_tolerances = mc.posterior_tolerances


def value_bound(u, sd, v_plus_noise, dtype, d_mu=0.0, d_v=0.0, value=None):
  """The absolute bound of one query's value at u: DEVICE_FACTOR (C_VALUE unit(u) + eps64 |log sd|), plus what the posterior's own error
  moves it by, to first order -- |d value / d mu| d_mu + |d value / d var| d_v = (cdf / h) / sd d_mu + (pdf / h) / (2 (var + add_noise)) d_v
  (0 when the reference reads the device's own mu, var) --; an fp32 result adds the one rounding of the output, eps32 / 2 of the value."""
  logh, cdf_h, pdf_h = exact_terms(float(u))
  b = DEVICE_FACTOR * (C_VALUE * unit(u) + EPS64 * abs(np.log(sd))) + cdf_h / sd * d_mu + pdf_h / (2.0 * v_plus_noise) * d_v
  if np.dtype(dtype) == np.float32:
    b += 0.5 * EPS32 * abs(np.log(sd) + logh if value is None else value)
  return float(b)


def grad_tol(u, dtype):
  """Relative to the query's largest gradient component: mes_cases.grad_tol with (1 + u^2) in the place of its gamma term -- fp64
  1e-7 (1 + u^2); fp32 2e-2 (1 + u^2), for queries with |u| <= 3.25 only."""
  return (1e-7 if np.dtype(dtype) == np.float64 else 2e-2) * (1.0 + float(u) * float(u))


# ---- the flat tail -------------------------------------------------------------------------------------------------------------------
FLAT_SEED = 3     # chosen on the CPU by test_logei_cases_host.py::test_the_flat_tail_premise's own search order: the first seed that holds


@functools.lru_cache(maxsize=None)
def flat_tail_problem(seed=FLAT_SEED):
  """Squared-exponential kernel, constant mean, n = 6 observations in [0.55, 0.95]^2 and a start near the opposite corner, where
  u = (mu - max y) / sd lies between -14 and -10: EI and its gradient are about 1e-25 there.  One sample (S = 1), fp64."""
  rng = np.random.default_rng([seed, 977])
  d = 2
  model = helpers.make_model(rng, 'constant', False, d)
  model.update(lengthscale=helpers.inv_softplus(np.full(d, 0.25)), signal_variance=helpers.inv_softplus(0.006),
               noise_variance=helpers.inv_softplus(1e-4), constant=np.array(0.0))
  x = rng.uniform(0.55, 0.95, size=(6, d))
  y = (1.0 + 0.3 * np.sin(5.0 * x[:, :1]) + 0.2 * x[:, 1:2])
  po = o.GPParams(model=mc._cast(model, np.float64), config={})
  sm = types.SimpleNamespace(model_t=mc._cast(model, np.float64), po=po, x=x, y=y, ko=o.squared_exponential, mo=o.constant,
                             noise=float(np.squeeze(o.retrieve_params(po, ['noise_variance'], WFO)[0])))
  case = Case('squared_exponential', 'constant', (6,), d, 1, 'fp64')
  return types.SimpleNamespace(case=case, smp=[sm], dtype=np.dtype(np.float64), target=float(np.max(y)), x0=np.array([0.5, 0.45]),
                               lo=np.zeros(d), hi=np.ones(d), noises=[sm.noise])


def flat_tail_logei(p):
  """x [D] -> (vals [1], grads [1, D]): the oracle's LogEI of the flat-tail problem, for acq_opt_oracle.minimise."""
  sm = p.smp[0]

  def vg(x):
    v, g, _ = oracle_value_and_grad(sm, np.asarray(x, dtype=np.float64)[None, :], p.target)
    return v, g
  return vg


def flat_tail_ei(p):
  sm = p.smp[0]

  def vg(x):
    v, g = o.acquisition_value_and_grad('ei', sm.mo, sm.ko, sm.po, sm.x, sm.y, np.asarray(x, dtype=np.float64)[None, :], p.target, WFO,
                                        add_noise=sm.noise, scale=SCALE)
    return np.array([float(v[0, 0])]), np.asarray(g, dtype=np.float64).reshape(1, -1)
  return vg


@functools.lru_cache(maxsize=None)
def flat_tail_reference():
  """(the oracle-driven run of acq_opt_oracle.minimise on LogEI from the start, SciPy's end point from the same start with its
  tolerances tightened to the maximiser itself, their distance in the max norm).  Shared by both tiers."""
  import scipy.optimize
  import acq_opt_oracle as ao
  p = flat_tail_problem()
  vg = flat_tail_logei(p)
  run = ao.minimise(vg, p.x0, p.lo, p.hi)

  def f(x):
    v, g = vg(x)
    return -float(v[0]), -g[0]
  res = scipy.optimize.minimize(f, p.x0, jac=True, method='L-BFGS-B', bounds=list(zip(p.lo, p.hi)), options=dict(gtol=1e-10, ftol=1e-15))
  return run, np.asarray(res.x, dtype=np.float64), float(np.max(np.abs(run.x - res.x))), float(-res.fun)
