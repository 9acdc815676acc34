"""CPU side of the tests of max-value entropy search (csrc/kernfun.h: mes_terms, mes_scalars_block; csrc/mes.hip: hbo_acq_mes,
hbo_mes_grad_samples, hbo_mes_maximize; acfun.MaxValueEntropySearch).  Shared by tests/test_mes_cases_host.py (this file judged on
its own, no device) and tests/test_gpu_mes.py (the device against it).

  exact_terms(g)        h, h' and the scales of their un-cancelled terms from mpmath, at a precision raised until doubling it changes
                        nothing; log cdf is log1p(-ncdf(-g)) for g > 0
  stable_terms(g)       the float64 restatement of the stable forms (SciPy erfcx, log_ndtr): what the device evaluates
  C_VALUE, C_SLOPE      that restatement's worst error against mpmath on [-30, 38.5], in units of eps * scale (measured by
                        test_mes_cases_host.py::test_restatement_against_mpmath); the device gets DEVICE_FACTOR = 8 times them
  scalars / exact_scalars   value, a_mu, a_var of one query from mu, var and the maxima: float64 (with a mutant on request) / mpmath
  posterior / oracle_value_and_grad   the oracle's posterior, and MES value + d value / d x from the oracle's posterior and its derivative
  value_bound, grad_tol the bounds of the GPU tier
  MUTANTS, CLAMP_MUTANTS   one failure each
  CASES                 the shapes of the GPU tier
"""
import functools
import types
from typing import NamedTuple

import mpmath as mp
import numpy as np
from scipy import special

import helpers
from oracle import hyperbo_oracle as o

WFO = o.DEFAULT_WARP_FUNC
EPS64, EPS32 = 2.0**-52, 2.0**-23
SCALE = 1.5                       # T / (T - 1) of three sub-datasets
GAMMAS = (-30.0, -8.0, -3.0, -0.5, 0.0, 0.7, 3.0, 8.3, 20.0, 38.0)   # the epilogue tests' gammas
GAMMAS_FP32 = tuple(g for g in GAMMAS if g <= 8.3)                  # h(8.3) = 2e-16 is a normal float; h(20) = 2e-88 is not
C_VALUE, C_SLOPE = 4.0, 3.0       # measured 3.10 (gamma 0.15) and 1.95 (gamma 2.65); test_restatement_against_mpmath asserts
                                  # measured <= C <= 2 * measured
DEVICE_FACTOR = 8.0               # the margin test_gpu_acq_tails.py gives the device's exp / erfc over the host's libm
QUANTUM = 2.0**-1074              # the spacing of float64 below 2^-1022: where pdf(gamma) is a denormal (gamma > 37.6) r is good to a
                                  # quantum, not to eps, and h' multiplies it by (1 + gamma^2) / 2


C_TAIL = 4.0                      # measured 3.09 (gamma 0.15), as C_VALUE is


def value_term_bound(g, h, value_scale, factor=1.0):
  """The absolute bound of one term h(gamma) in float64: factor * C_VALUE * eps64 * (gamma^2 / 2 + |log cdf| + |gamma r| / 2) -- and,
  for gamma >= 0, no more than factor * C_TAIL * eps64 * (1 + gamma^2) * h: there gamma r / 2 and -log cdf are both positive, nothing
  cancels, and the only amplified rounding is that of erfc's argument (relative gamma^2 eps in cdf(-gamma)).  The first bound alone
  is 1e3 (gamma = 8.3) to 1e300 (38) times the value itself and would pass a result that has lost every digit."""
  b = factor * C_VALUE * EPS64 * value_scale
  if g >= 0.0:
    b = min(b, factor * C_TAIL * (EPS64 * (1.0 + g * g) * h + (1.0 + g) * QUANTUM))
  return b


def slope_unit(g, slope_scale):
  """What one unit of C_SLOPE is at gamma = g: eps64 * the un-cancelled scale, or the quantum's share where that has underflowed."""
  return EPS64 * slope_scale + (1.0 + g * g) * QUANTUM


# ---- the reference --------------------------------------------------------------------------------------------------------------
def _mp_terms(g, dps):
  with mp.workdps(dps):
    g = mp.mpf(g)
    logcdf = mp.log1p(-mp.ncdf(-g)) if g > 0 else mp.log(mp.ncdf(g))
    r = mp.exp(-g * g / 2 - logcdf) / mp.sqrt(2 * mp.pi)
    h = g * r / 2 - logcdf
    dh = -(r / 2) * (1 + g * g + g * r)
    sh = g * g / 2 + abs(logcdf) + abs(g * r) / 2
    sdh = (r / 2) * (1 + g * g + abs(g * r))
    return h, dh, sh, sdh


@functools.lru_cache(maxsize=None)
def exact_terms(g):
  """(h, h', value scale, slope scale) at gamma = g as floats, correctly rounded: the precision is doubled from 50 digits until two
  successive results agree to 1e-25 relatively (at 60 digits a literal 1 - ncdf(-20) is already 1)."""
  g = float(g)
  if g == np.inf:
    return 0.0, 0.0, np.inf, 0.0
  if g == -np.inf:
    return np.inf, 0.0, np.inf, np.inf
  dps, prev = 50, None
  while True:
    cur = _mp_terms(g, dps)
    if prev is not None and all(abs(a - b) <= mp.mpf(10)**-25 * abs(b) for a, b in zip(prev[:2], cur[:2])):
      return tuple(float(v) for v in cur)
    prev, dps = cur, 2 * dps
    assert dps <= 6400, g


def _pdf(g):
  """pdf(g) with g^2 taken exactly: g = gh + gl with gh of 24 bits, so gh^2 is exact and exp(-gh^2 / 2) exp(-(2 gh gl + gl^2) / 2) loses
  nothing to the rounding of the square (which alone costs g^2 / 2 ulp: 700 at g = 37).  The device takes the residual from an fma."""
  gh = g.astype(np.float32).astype(np.float64)
  gl = g - gh
  return np.exp(-0.5 * gh * gh) * np.exp(-gh * gl - 0.5 * gl * gl) / np.sqrt(2.0 * np.pi)


def stable_terms(g):
  """(h, h') in float64 by the stable forms, elementwise: gamma >= 0 through log_ndtr (log1p(-ndtr(-g))) and r = pdf / ndtr; gamma < 0
  through erfcx: r = sqrt(2 / pi) / erfcx(-g / sqrt 2), log cdf = log(erfcx / 2) - g^2 / 2, with r + g formed first."""
  g = np.asarray(g, dtype=np.float64)
  h, dh = np.empty_like(g), np.empty_like(g)
  neg = g < 0
  with np.errstate(all='ignore'):
    gn = g[neg]
    e = special.erfcx(-gn / np.sqrt(2.0))
    r = np.sqrt(2.0 / np.pi) / e
    rg = gn * (r + gn)
    h[neg], dh[neg] = 0.5 * rg - np.log(0.5 * e), -0.5 * r * (1.0 + rg)
    gp = g[~neg]
    r = _pdf(gp) / special.ndtr(gp)
    h[~neg] = 0.5 * gp * r - special.log_ndtr(gp)
    dh[~neg] = np.where(r == 0.0, -0.0, -0.5 * r * (1.0 + gp * gp + gp * r))
  h = np.where(g == -np.inf, np.inf, np.where(g == np.inf, 0.0, h))
  dh = np.where(np.isinf(g), -0.0, dh)
  return np.where(h < 0.0, 0.0, h), dh


# ---- the scalar step of one query ---------------------------------------------------------------------------------------------------
def _literal_logcdf(g):
  with np.errstate(all='ignore'):
    r = np.exp(-0.5 * g * g) / np.sqrt(2 * np.pi) / special.ndtr(g)
    lc = np.log(special.ndtr(g))
    return 0.5 * g * r - lc, -0.5 * r * (1 + g * g + g * r)


def _literal_one_minus(g):
  with np.errstate(all='ignore'):
    cdf = 1.0 - special.ndtr(-g)
    r = np.exp(-0.5 * g * g) / np.sqrt(2 * np.pi) / cdf
    return 0.5 * g * r - np.log(cdf), -0.5 * r * (1 + g * g + g * r)


def _missing_half(g):
  h, dh = stable_terms(g)
  with np.errstate(all='ignore'):
    r = np.where(g < 0, np.sqrt(2 / np.pi) / special.erfcx(-g / np.sqrt(2)), np.exp(-0.5 * g * g) / np.sqrt(2 * np.pi) / special.ndtr(g))
  return h + 0.5 * g * r, dh           # h = gamma r - log cdf


def scalars(mu, var, add_noise, scale, ystar, mutant=None):
  """(value, a_mu, a_var) of one query in float64, as include/hbo.h states them.  mutant: a key of MUTANTS."""
  ystar = np.asarray(ystar, dtype=np.float64)
  k = ystar.size
  v2 = (var + add_noise) * scale
  if v2 <= 0.0 and mutant != 'no_v2_rule':
    return 0.0, 0.0, 0.0
  with np.errstate(all='ignore'):
    sd = np.sqrt(v2)
    g = (ystar - mu) / sd
    terms = {'literal_log_cdf': _literal_logcdf, 'literal_one_minus_cdf': _literal_one_minus, 'missing_half': _missing_half}.get(mutant, stable_terms)
    h, dh = terms(g)
    div = 1.0 if mutant == 'sum_not_mean' else float(k)
    val, amu = np.sum(h) / div, -np.sum(dh) / div / sd
    asd = -np.sum(dh * g) / div / sd
    if mutant == 'dgamma_dsd_sign':
      asd = -asd
    avar = asd / (2.0 * sd) * (1.0 if mutant == 'scale_dropped' else scale)
  return float(val), float(amu), float(avar)


def exact_scalars(mu, var, add_noise, scale, ystar):
  """scalars() from exact_terms, with the absolute bounds of the device's three results beside them (DEVICE_FACTOR * C * eps64 * the
  scales of the un-cancelled terms): ((value, a_mu, a_var), (b_value, b_amu, b_avar))."""
  v2 = (var + add_noise) * scale
  if v2 <= 0.0:
    return (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
  sd = float(np.sqrt(v2))
  g = [float((y - mu) / sd) for y in np.ravel(ystar)]
  t = [exact_terms(x) for x in g]
  k = float(len(g))
  val, amu = sum(x[0] for x in t) / k, -sum(x[1] for x in t) / k / sd
  asd = -sum(x[1] * gg for x, gg in zip(t, g)) / k / sd
  bv = sum(value_term_bound(gg, x[0], x[2], DEVICE_FACTOR) for x, gg in zip(t, g)) / k
  bm = DEVICE_FACTOR * C_SLOPE * sum(slope_unit(gg, x[3]) for x, gg in zip(t, g)) / k / sd
  bs = DEVICE_FACTOR * C_SLOPE * sum(slope_unit(gg, x[3]) * abs(gg) for x, gg in zip(t, g)) / k / sd
  f = scale / (2.0 * sd)
  return (val, amu, asd * f), (bv, bm, bs * f)


MUTANTS = ('literal_log_cdf', 'literal_one_minus_cdf', 'missing_half', 'sum_not_mean', 'dgamma_dsd_sign', 'scale_dropped', 'no_v2_rule')

# (mu, var, add_noise, scale, gammas of the maxima): the scalar-step cases the mutants are judged on
SCALAR_CASES = [
    (0.3, 0.8, 0.0, SCALE, GAMMAS),
    (-1.2, 0.05, 0.01, SCALE, (8.3, 20.0, 38.0)),
    (0.1, 0.4, 0.0, 1.0, (0.7,)),
    (0.0, 2.0, 0.1, SCALE, (-3.0, -0.5, 3.0, 8.3)),
    (0.5, 0.0, 0.0, SCALE, (1.0, 2.0)),                 # v2 = 0
    (0.5, 0.2, -0.3, SCALE, (1.0, 2.0)),                # v2 < 0
]


def scalar_case_maxima(case):
  mu, var, noise, scale, gammas = case
  v2 = (var + noise) * scale
  sd = np.sqrt(v2) if v2 > 0 else 1.0
  return mu + np.asarray(gammas) * sd


def clamp_maxima(ystar, y_observed, mutant=None):
  """max_value_samples' last step: no maximum below the incumbent."""
  ystar = np.asarray(ystar, dtype=np.float64)
  if mutant == 'no_clamp' or y_observed is None or np.size(y_observed) == 0:
    return ystar
  return np.maximum(ystar, float(np.max(y_observed)))


CLAMP_MUTANTS = ('no_clamp',)


# ---- the cases of the GPU tier ----------------------------------------------------------------------------------------------------
class Case(NamedTuple):
  kname: str
  mname: str
  ns: tuple       # observations per sample (S = len(ns))
  d: int
  K: int
  M: int
  dtype: str

  @property
  def id(self):
    return f'{self.kname}-{self.mname}-n{"_".join(map(str, self.ns))}-d{self.d}-K{self.K}-M{self.M}-{self.dtype}'

  @property
  def S(self):
    return len(self.ns)


CASES = [
    Case('squared_exponential', 'constant', (1,), 1, 1, 1, 'fp64'),
    Case('matern32', 'zero', (5,), 3, 7, 9, 'fp64'),
    Case('matern52', 'linear', (127, 127, 127), 17, 64, 37, 'fp64'),
    Case('dot_product', 'constant', (128,), 3, 65, 9, 'fp64'),
    Case('squared_exponential', 'linear', (129,), 17, 256, 9, 'fp64'),
    Case('matern52', 'zero', (300, 300, 300), 3, 7, 37, 'fp64'),
    Case('matern32', 'constant', (100, 300, 100), 1, 65, 9, 'fp64'),      # one call mixing n = 100 and n = 300
    Case('dot_product', 'linear', (300,), 17, 64, 1, 'fp64'),
    Case('squared_exponential', 'constant', (128, 5, 127), 3, 256, 9, 'fp32'),
    Case('matern52', 'linear', (129,), 3, 7, 37, 'fp32'),
    Case('dot_product', 'zero', (300,), 1, 65, 9, 'fp32'),
]


def np_dtype(case):
  return np.float64 if case.dtype == 'fp64' else np.float32


def _cast(t, dtype):
  return {k: _cast(v, dtype) for k, v in t.items()} if isinstance(t, dict) else np.asarray(t, dtype=dtype)


@functools.lru_cache(maxsize=None)
def problem(case, seed=71):
  """The S (model, observations) pairs of a case, the shared queries and the oracle's fp64 posterior on the same (dtype-rounded) numbers,
  and maxima y*[s, k] = mu_s(q0) + gamma_k sd_s(q0) with gamma spread over [-3, 6] (fp32: [0, 3]) at query q0 = 0 (the other queries sit
  wherever their posterior puts them).  No device.  Computed once per case and shared: do not write to it."""
  dt = np_dtype(case)
  rng = np.random.default_rng([seed, len(case.id), case.d, case.K, case.M])
  xq = np.ascontiguousarray(rng.uniform(size=(case.M, case.d)).astype(dt))
  smp = []
  for s, n in enumerate(case.ns):
    model_t = _cast(helpers.make_model(rng, case.mname, False, case.d), dt)
    po = o.GPParams(model=_cast(model_t, np.float64), config={})
    x, y = helpers.synthetic_task(rng, n, case.d, dtype=dt)
    smp.append(types.SimpleNamespace(model_t=model_t, po=po, x=x, y=y, ko=getattr(o, case.kname), mo=getattr(o, case.mname),
                                     noise=float(np.squeeze(o.retrieve_params(po, ['noise_variance'], WFO)[0]))))
  p = types.SimpleNamespace(case=case, xq=xq, smp=smp, dtype=np.dtype(dt))
  lo, hi = (-3.0, 6.0) if case.dtype == 'fp64' else (0.0, 3.0)
  p.gam0 = np.linspace(lo, hi, case.K) if case.K > 1 else np.array([0.7])
  for sm in smp:
    sm.mu, sm.var, sm.dmu, sm.dsd = posterior(sm, xq, 0.0, SCALE)
    sm.sd = np.sqrt(sm.var * SCALE)
  p.ystar = np.ascontiguousarray(np.stack([sm.mu[0] + p.gam0 * sm.sd[0] for sm in smp]))
  return p


def zero_variance_problem(n, dtype):
  """A problem whose posterior variance is exactly 0 at query 0 with add_noise = 0, from the products themselves: a dot-product kernel
  with dot_prod_bias = 0 (the bias is not warped) and the query x = 0, so k(x, x) = 0 and k(x, X) = 0 in any precision.  The other
  queries keep a positive variance.  Only what the device side reads is filled in (case, dtype, xq, ystar, smp[0].model_t / x / y)."""
  base = problem(Case('dot_product', 'constant', (n,), 3, 7, 9, dtype))
  sm = base.smp[0]
  model_t = dict(sm.model_t, dot_prod_bias=np.zeros((), dtype=base.dtype))
  xq = base.xq.copy()
  xq[0] = 0
  return types.SimpleNamespace(case=base.case, dtype=base.dtype, xq=xq, ystar=base.ystar,
                               smp=[types.SimpleNamespace(model_t=model_t, x=sm.x, y=sm.y)])


def posterior(sm, xq, add_noise, scale):
  """The oracle's mu [M], var [M] and their derivatives d mu / dx, d sd / dx [M, D] (sd = sqrt((var + add_noise) scale)): UCB is linear
  in its parameter, so its oracle gradient at beta = 0 is d mu / dx and the difference to beta = 1 is d sd / dx."""
  x64, y64, xq64 = sm.x.astype(np.float64), sm.y.astype(np.float64), np.asarray(xq, dtype=np.float64)
  mu, var = o.predict(sm.mo, sm.ko, sm.po, x64, y64, xq64, WFO)
  _, g0 = o.acquisition_value_and_grad('ucb', sm.mo, sm.ko, sm.po, x64, y64, xq64, 0.0, WFO, add_noise=add_noise, scale=scale)
  _, g1 = o.acquisition_value_and_grad('ucb', sm.mo, sm.ko, sm.po, x64, y64, xq64, 1.0, WFO, add_noise=add_noise, scale=scale)
  return np.ravel(mu).astype(np.float64), np.ravel(var).astype(np.float64), g0, g1 - g0


def oracle_value_and_grad(sm, xq, ystar, add_noise=0.0, scale=SCALE, mutant=None):
  """(value [M], gradient [M, D], gammas [M, K]) of the MES value of one sample from the oracle's posterior and its derivative:
  d value / dx = a_mu d mu / dx + a_sd d sd / dx, a_sd = a_var * 2 sd / scale."""
  mu, var, dmu, dsd = posterior(sm, xq, add_noise, scale)
  val, grad = np.zeros(mu.size), np.zeros_like(dmu)
  sd = np.sqrt((var + add_noise) * scale)
  for q in range(mu.size):
    v, amu, avar = scalars(mu[q], var[q], add_noise, scale, ystar, mutant)
    asd = avar * 2.0 * sd[q] / scale
    val[q], grad[q] = v, amu * dmu[q] + asd * dsd[q]
  return val, grad, (np.asarray(ystar)[None, :] - mu[:, None]) / sd[:, None]


# ---- the bounds of the GPU tier -----------------------------------------------------------------------------------------------------
def posterior_tolerances(dtype, mu, var):
  """(d_mu, d_v): what test_gpu_parity.py holds the posterior to -- fp64 1e-9 of max |mu|, max |var|; fp32 5e-4 (of max(max |mu|, 1))
  and 1e-4."""
  if np.dtype(dtype) == np.float64:
    return 1e-9 * np.max(np.abs(mu)), 1e-9 * np.max(np.abs(var))
  return 5e-4 * max(np.max(np.abs(mu)), 1.0), 1e-4 * np.max(np.abs(var))


def value_bound(gammas, sd, v_plus_noise, dtype, d_mu=0.0, d_v=0.0):
  """The absolute bound of one query's value whose maxima sit at `gammas`: the mean over k of
    value_term_bound(gamma, factor = DEVICE_FACTOR)  +  |h'(gamma)| * d_gamma,
  d_gamma = d_mu / sd + |gamma| d_v / (2 (var + add_noise)) (the posterior term; 0 when the reference reads the device's own mu, var);
  an fp32 result adds the one rounding of the output, eps32 / 2 of the value."""
  t = [exact_terms(float(g)) for g in gammas]
  b = np.mean([value_term_bound(float(g), x[0], x[2], DEVICE_FACTOR) + abs(x[1]) * (d_mu / sd + abs(float(g)) * d_v / (2.0 * v_plus_noise))
               for x, g in zip(t, gammas)])
  if np.dtype(dtype) == np.float32:   # (or, below 2^-126, half a quantum of the format: the value may round to 0)
    b += max(0.5 * EPS32 * np.mean([x[0] for x in t]), 2.0**-150)
  return float(b)


def grad_tol(gammas, dtype):
  """Relative to the query's largest gradient component: fp64 1e-7 (1 + gamma^2), the existing acquisition-gradient bound, with the
  MEAN of gamma_k^2 over the query's maxima -- the gradient is a mean over k of terms that each carry (1 + gamma_k^2), so one far
  maximum does not loosen the bound of the whole query; fp32 2e-2 (1 + gamma^2) (test_gpu_acq_tails.py), for queries with every
  |gamma| <= 3.25 only."""
  g2 = float(np.mean(np.square(gammas)))
  return (1e-7 if np.dtype(dtype) == np.float64 else 2e-2) * (1.0 + g2)
