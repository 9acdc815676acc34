"""EI / PI / UCB per query in the tails (run with `-m gpu` on an MI355X): the device epilogues against an 80-digit mpmath
reference (acq_oracle.exact_ei), RELATIVELY and PER QUERY, never max-norm.

Why: every other EI comparison of the suite is a max-norm one over queries at gamma = (target - mu) / sd in about [-3, 4].  A query
whose EI is 1e-12 can be wrong by a factor of a thousand there and no test moves -- and after a few dozen observations every remaining
candidate of a BO run is several standard deviations below the incumbent, so the ORDER of tiny EI values decides the next point.

How the tail is reached: the target is a parameter of hbo_acq / hbo_acq_grad / hbo_acq_samples (`acfun_callback` in the Python
layer).  For a fixed model and fixed queries, target_k = mu_q + gamma_k * sd_q (from the oracle's posterior) puts a chosen query at a
chosen gamma and the others wherever their mu, sd put them; every query of every call is checked at its OWN gamma.

Bounds (acq_oracle.C_HOST = 4 is measured on the CPU by test_acq_host.py::test_stable_form_constant):
  (a) epilogue alone, reference = exact_ei of the device's own mu, var (hbo_predict: same routine, bit-identical calls) and
      sd = sqrt((var + add_noise) * scale) formed in the model dtype as the kernel forms it:
        fp64  8 * C_HOST * (1 + gamma**4) * 2**-52   (the 8: margin for the device's exp / erfc over the host libm)
        fp32  (5 * (gamma**2 + 2) + 1) * 2**-24 + the fp64 term   (gamma from 5 fp32 roundings, |d ln EI / d ln gamma| <= gamma**2 + 2,
              one rounding of the output), gamma <= 12 (EI(13) is not a normal float)
      PI, UCB: 4 ulp of the model dtype.
  posterior term (b, d: two routes to mu, var, or the oracle's posterior): d_gamma = d_mu / sd + |gamma| d_v / (2 v2),
      |d ln EI / d gamma| <= gamma + 2 (gamma >= 0; <= 1.25 below 0), d ln sd = d_v / (2 v2); d_mu, d_v are the tolerances the suite
      holds the posterior to: fp64 1e-9 of max |mu|, max |var| (test_gpu_parity.py::test_factor_predict_acquisition_vs_oracle), fp32
      5e-4 (of max(max |mu|, 1)) and 1e-4 (test_gpu_parity.py::test_fp32_registry_value_grad_posterior_vs_oracle).
  (d) gradient per query: max_d |g - g_ref| <= tol * max_d |g_ref|, tol = 1e-7 * (1 + gamma**2) in fp64
      (test_acquisition_value_and_grad_vs_oracle's 1e-7; Phi(u), phi(u) have relative sensitivity ~gamma**2 to u), 2e-2 * (1 + gamma**2)
      in fp32 (test_acquisition_grad_fp32_and_many_queries' 2e-2) at gamma in {0, 2, 3} only: beyond, an fp32 bound says nothing.

Worst ratios to the bounds observed on an MI355X (each test prints its own with -s and appends it to $HBO_GRAD_LOG when set):
  (a) EI fp64 0.10 (gamma 0.7; i.e. 0.8 of the host constant: the device's exp / erfc need none of the factor 8), EI fp32 0.39
      (gamma 8.3), PI / UCB 0.25 (1 ulp of the 4);  (b) fp64 1.3e-3 (gamma 36.3), fp32 9.7e-3 (gamma 2.0), through acfun 1.3e-3 (GP),
      3.9e-4 (HGP of 3);  (c) no pair left out, fp64 and fp32;  (d) fp64 1.1e-7, fp32 EI 1.8e-3, PI 3.6e-3.
  Two hbo_predict calls returned identical bits in every case of (a).
With the literal form (pdf(g) - g * (1 - cdf(g))) * sd in post_epilogue_kernel (tried once, by hand): (a) fails in fp64 for every case --
ratios just above 1 from gamma 3.1 to 4, 10-1000 at 5, 1e5 and negative values at 8 -- and in fp32 from gamma 6.2; (b) fails in fp64
from gamma 5.4; (c) fails on the sign (EI of -3e-17 .. -1.5e-16 at gamma 8.1 - 8.3) in fp64 and fp32; everything below gamma 3 passes."""
import os
import types

import numpy as np
import pytest

import acq_oracle as ao
import helpers
from oracle import hyperbo_oracle as o

pytestmark = pytest.mark.gpu
WFO = o.DEFAULT_WARP_FUNC
CASES = [('squared_exponential', False, 'constant'), ('matern52', True, 'linear_mlp'), ('dot_product', False, 'linear')]
CASE_IDS = ['se-constant', 'matern52_mlp-linear_mlp', 'dot-linear']
SCALE = 1.5           # T / (T - 1) of three sub-datasets (gp.py:607-619)
ACQ_EI, ACQ_PI, ACQ_UCB = 0, 1, 2
_WORST = {}


def _native():
  from hyperbo_amd import _model as hmodel
  from hyperbo_amd import _native as nat
  from hyperbo_amd.basics import definitions as defs, linalg
  from hyperbo_amd.bo_utils import acfun
  from hyperbo_amd.gp_utils import gp, kernel, mean, utils
  return types.SimpleNamespace(hmodel=hmodel, nat=nat, defs=defs, linalg=linalg, acfun=acfun, gp=gp, kernel=kernel, mean=mean, utils=utils)


def _cast(t, dtype):
  return {k: _cast(v, dtype) for k, v in t.items()} if isinstance(t, dict) else np.asarray(t, dtype=dtype)


def _record(label, ratio, where):
  """Worst ratio to a bound per label: printed (-s) and appended to $HBO_GRAD_LOG."""
  if ratio > _WORST.get(label, (-1.0, None))[0]:
    _WORST[label] = (ratio, where)
  print(f'\nacq tails: {label}: worst ratio to the bound {ratio:.3e} at {where}')
  log = os.environ.get('HBO_GRAD_LOG')
  if log:
    with open(log, 'a') as f:
      f.write(f'{ratio:.3e} acq_tails {label} at {where} {os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]}\n')


def _oracle_case(kname, mlp, mname, n_obs, m_q, dtype, seed):
  """One model, its observations, its queries, and the oracle's fp64 posterior on the same (dtype-rounded) numbers: no device."""
  rng = np.random.default_rng(seed)
  d = 3
  model_t = _cast(helpers.make_model(rng, mname, mlp, d), dtype)
  cfg = {'mlp_features': helpers.MLP_FEATURES}
  po = o.GPParams(model=_cast(model_t, np.float64), config=dict(cfg))
  x, y = helpers.synthetic_task(rng, max(n_obs, 1), d, dtype=dtype)
  xq = np.ascontiguousarray(rng.uniform(size=(m_q, d)).astype(dtype))
  ko, mo = getattr(o, kname + ('_mlp' if mlp else '')), getattr(o, mname)
  x64, y64, xq64 = x.astype(np.float64), y.astype(np.float64), xq.astype(np.float64)
  mu_o, var_o = o.predict(mo, ko, po, x64 if n_obs else None, y64 if n_obs else None, xq64, WFO)
  noise = float(np.squeeze(o.retrieve_params(po, ['noise_variance'], WFO)[0]))
  c = types.SimpleNamespace(d=d, dtype=np.dtype(dtype), model_t=model_t, po=po, x=x, y=y, x64=x64, y64=y64, xq=xq, xq64=xq64, ko=ko, mo=mo,
                            n_obs=n_obs, m_q=m_q, noise=noise, cfg=cfg, h=None,
                            mu_o=np.asarray(mu_o, dtype=np.float64).ravel(), var_o=np.asarray(var_o, dtype=np.float64).ravel())
  c.sd_o = np.sqrt((c.var_o + noise) * SCALE)
  return c


def _case(gpu_ctx, kname, mlp, mname, n_obs, m_q, dtype, seed=61):
  """_oracle_case plus the device side: the hbo_model and, with observations, the factorised cache."""
  c = _oracle_case(kname, mlp, mname, n_obs, m_q, dtype, seed)
  nv = _native()
  pn = nv.defs.GPParams(model=c.model_t, config=dict(c.cfg))
  kn, mn = getattr(nv.kernel, kname + ('_mlp' if mlp else '')), getattr(nv.mean, mname)
  wf = nv.utils.DEFAULT_WARP_FUNC
  c.nv = nv
  c.h = nv.linalg.factor(mn, kn, pn, c.x, c.y, wf) if n_obs else None
  c.bm = nv.hmodel.BuiltModel(mn, kn, pn, wf, dtype, c.d)
  c.ctx = c.h.ctx if c.h is not None else gpu_ctx
  c.hh = c.h.handle if c.h is not None else None
  return c


def _close(c):
  if c.h is not None:
    c.h.close()


def _predict(c):
  nat = c.nv.nat
  mu, var = np.empty((c.m_q, 1), dtype=c.dtype), np.empty((c.m_q, 1), dtype=c.dtype)
  c.ctx.check(nat.lib().hbo_predict(c.ctx.handle, c.bm.ref(), c.hh, nat.ptr(c.xq), c.m_q, 0, nat.ptr(mu), nat.ptr(var)))
  return mu[:, 0], var[:, 0]


def _acq(c, acq_id, param):
  nat = c.nv.nat
  out = np.empty((c.m_q, 1), dtype=c.dtype)
  c.ctx.check(nat.lib().hbo_acq(c.ctx.handle, c.bm.ref(), c.hh, nat.ptr(c.xq), c.m_q, acq_id, float(param), c.noise, SCALE, nat.ptr(out)))
  return out[:, 0]


def _acq_grad(c, acq_id, param):
  nat = c.nv.nat
  out = np.empty((c.m_q, 1), dtype=c.dtype)
  grad = np.zeros((c.m_q, c.d), dtype=np.float64)
  c.ctx.check(nat.lib().hbo_acq_grad(c.ctx.handle, c.bm.ref(), c.hh, nat.ptr(c.xq), c.m_q, acq_id, float(param), c.noise, SCALE, nat.ptr(out),
                                     grad.ctypes.data_as(nat.C.POINTER(nat.C.c_double))))
  return out[:, 0], grad


def _device_sd(c, var):
  """sd as post_epilogue_kernel forms it: (var + (T)add_noise) * (T)scale, sqrt, all in the model dtype."""
  t = c.dtype.type
  return np.sqrt((var + t(c.noise)) * t(SCALE))


def _target(c, q, gamma):
  """The target that puts query q at gamma under the oracle's posterior, rounded to the model dtype (the kernel casts it)."""
  return float(c.dtype.type(c.mu_o[q] + gamma * c.sd_o[q]))


def _gammas(dtype):
  return [g for g in ao.GAMMAS if np.dtype(dtype) == np.float64 or g <= 12.0]


def _window(dtype):
  """The gammas a query is checked at: the sweep's [-10, 37] (fp32: <= 12) widened by 0.25, so that the query AIMED at 37 (or 12) is
  checked when the device's posterior puts it a hair beyond; EI(37.25) = 7e-306 and, in fp32, EI(12.25) = 7e-36 are still normal."""
  return -10.25, (37.25 if np.dtype(dtype) == np.float64 else 12.25)


def _epilogue_bound(gamma, dtype):
  b = 8.0 * ao.fp64_bound(gamma)
  if np.dtype(dtype) == np.float32:
    b += (5.0 * (gamma * gamma + 2.0) + 1.0) * ao.EPS32
  return b


def _posterior_term(c, gamma, sd, two_routes):
  """Relative move of EI when mu, var move by the tolerances the suite holds the posterior to (module docstring).  two_routes: both
  sides are device routes, each within the tolerance of the true posterior, so they are within twice the tolerance of each other."""
  if c.dtype == np.float64:   # test_gpu_parity.py::test_factor_predict_acquisition_vs_oracle: rel_err(mu), rel_err(var) < 1e-9
    d_mu, d_v = 1e-9 * np.max(np.abs(c.mu_o)), 1e-9 * np.max(np.abs(c.var_o))
  else:                       # test_gpu_parity.py::test_fp32_registry_value_grad_posterior_vs_oracle: e_mu <= 5e-4, e_var <= 1e-4
    d_mu, d_v = 5e-4 * max(np.max(np.abs(c.mu_o)), 1.0), 1e-4 * np.max(np.abs(c.var_o))
  if two_routes:
    d_mu, d_v = 2 * d_mu, 2 * d_v
  v2 = sd * sd / SCALE     # d_v is an error of var; v2 = (var + noise) * scale moves by scale * d_v, relative d_v * scale / v2
  rel_v = d_v / (2.0 * v2)
  d_gamma = d_mu / sd + abs(gamma) * rel_v
  return d_gamma * (max(gamma, 0.0) + 2.0) + rel_v


# ---- (a) the epilogue alone, per query -------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['fp64', 'fp32'])
@pytest.mark.parametrize('m_q', [7, 1500])
@pytest.mark.parametrize('n_obs', [0, 150, 300])
@pytest.mark.parametrize('kname,mlp,mname', CASES, ids=CASE_IDS)
def test_epilogue_per_query_vs_mpmath(gpu_ctx, kname, mlp, mname, n_obs, m_q, dtype):
  """hbo_acq's EI / PI / UCB of every query against the exact value of the device's own mu, var.  n_obs = 0: prior branch
  (cache == NULL); 300 observations: more than one 128-row block (the mupart branch); 1500 queries: more than one query pass.
  Worst ratio to the bound on an MI355X: fp64 0.10, fp32 0.39, PI / UCB 0.25 of the 4 ulp (module docstring)."""
  c = _case(gpu_ctx, kname, mlp, mname, n_obs, m_q, dtype)
  try:
    mu, var = _predict(c)
    mu2, var2 = _predict(c)
    # identical calls are bit-identical (hbo.h): hbo_acq's own mu, var are then the ones read here
    assert mu.tobytes() == mu2.tobytes() and var.tobytes() == var2.tobytes()
    assert np.isfinite(mu).all() and (var + c.dtype.type(c.noise) > 0).all()
    sd = _device_sd(c, var)
    lo, hi = _window(dtype)
    eps = float(np.finfo(c.dtype).eps)
    mu_l, sd_l = mu.astype(np.longdouble), sd.astype(np.longdouble)
    bad, reached, worst, worst_pu = [], set(), (0.0, None), 0.0
    for k, g in enumerate(_gammas(dtype)):
      qk = (k * 5) % m_q
      target = _target(c, qk, g)
      ei = _acq(c, ACQ_EI, target)
      assert ei.dtype == c.dtype
      gam = ((np.longdouble(target) - mu_l) / sd_l).astype(np.float64)     # each query's own gamma (80-bit: exact enough for a bound)
      for q in np.flatnonzero((gam >= lo) & (gam <= hi)):
        gq = float(gam[q])
        if q == qk and abs(gq - g) <= 0.25:
          reached.add(g)
        r = ao.rel_to(ei[q], ao.exact_ei(mu[q], sd[q], target)) / _epilogue_bound(gq, dtype) if np.isfinite(ei[q]) else np.inf
        if r > worst[0]:
          worst = (r, (g, int(q), round(gq, 3)))
        if not r <= 1.0:
          bad.append((g, int(q), round(gq, 3), float(ei[q]), r))
      # PI = (mu - target) / sd and UCB = mu + beta * sd (beta = this gamma): one or two roundings from mu, sd -> 4 ulp; reference in
      # 80-bit long double (2**-64, far below 4 ulp of either dtype)
      pi = _acq(c, ACQ_PI, target).astype(np.longdouble)
      pi_x = (mu_l - np.longdouble(target)) / sd_l
      ucb = _acq(c, ACQ_UCB, g).astype(np.longdouble)
      ucb_x = mu_l + np.longdouble(g) * sd_l
      r_pi = np.max(np.abs(pi - pi_x) / (4 * eps * np.maximum(np.abs(pi_x), np.finfo(c.dtype).tiny)))
      r_ucb = np.max(np.abs(ucb - ucb_x) / (4 * eps * np.maximum(np.abs(mu_l), np.abs(np.longdouble(g) * sd_l))))
      worst_pu = max(worst_pu, float(r_pi), float(r_ucb))
      assert r_pi <= 1.0 and r_ucb <= 1.0, (g, float(r_pi), float(r_ucb))
    _record(f'{c.dtype.name} epilogue EI', worst[0], f'(gamma aimed, query, gamma) = {worst[1]} {kname} n={n_obs} M={m_q}')
    _record(f'{c.dtype.name} epilogue PI/UCB (of 4 ulp)', worst_pu, f'{kname} n={n_obs} M={m_q}')
    assert not bad, (f'{len(bad)} queries beyond the bound, smallest gamma {min(b[2] for b in bad)}; first (gamma aimed, query, gamma, EI, '
                     f'ratio): {bad[:5]}')
    assert reached == set(_gammas(dtype)), sorted(set(_gammas(dtype)) - reached)
  finally:
    _close(c)


# ---- (b) the two entry points agree ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['fp64', 'fp32'])
@pytest.mark.parametrize('n_obs', [0, 150, 300])
@pytest.mark.parametrize('kname,mlp,mname', CASES, ids=CASE_IDS)
def test_acq_and_acq_grad_values_agree_per_query(gpu_ctx, kname, mlp, mname, n_obs, dtype):
  """hbo_acq's value and the value hbo_acq_grad returns, same model, queries and target, per query.  The kernels reach mu, var by
  different routes (model-dtype sums over the product's column squares / double sums over l = W k), so the bound is the posterior
  term (two routes) plus the epilogue bound of either side.  fp32: gamma <= 3 (beyond ~4 the posterior term is of order one)."""
  c = _case(gpu_ctx, kname, mlp, mname, n_obs, 7, dtype, seed=62)
  try:
    mu, var = _predict(c)
    sd = _device_sd(c, var)
    top = 37.25 if c.dtype == np.float64 else 3.25
    gammas = [g for g in ao.GAMMAS if g <= top]
    bad, reached, worst = [], set(), (0.0, None)
    for k, g in enumerate(gammas):
      qk = (k * 5) % 7
      target = _target(c, qk, g)
      a = _acq(c, ACQ_EI, target)
      b, _ = _acq_grad(c, ACQ_EI, target)
      for q in range(7):
        gq = ao.exact_gamma(mu[q], sd[q], target)
        if not -10.25 <= gq <= top:
          continue
        if q == qk and abs(gq - g) <= 0.25:
          reached.add(g)
        bound = _posterior_term(c, gq, float(sd[q]), True) + 2 * _epilogue_bound(gq, dtype)
        r = abs(float(a[q]) - float(b[q])) / (bound * max(abs(float(a[q])), abs(float(b[q])), 1e-300)) \
            if np.isfinite(a[q]) and np.isfinite(b[q]) else np.inf
        if r > worst[0]:
          worst = (r, (g, q, round(gq, 3)))
        if not r <= 1.0:
          bad.append((g, q, round(gq, 3), float(a[q]), float(b[q]), r))
    _record(f'{c.dtype.name} hbo_acq vs hbo_acq_grad value', worst[0], f'{worst[1]} {kname} n={n_obs}')
    assert not bad, f'{len(bad)} queries disagree, smallest gamma {min(b_[2] for b_ in bad)}; first: {bad[:5]}'
    assert reached == set(gammas), sorted(set(gammas) - reached)
  finally:
    _close(c)


@pytest.mark.parametrize('n_samples', [1, 3], ids=['gp', 'hgp3'])
def test_python_value_and_grad_value_agrees_with_the_acquisition(gpu_ctx, n_samples):
  """acfun.expected_improvement(...) against .value_and_grad(...)[0] with the target given through `acfun_callback`: a GP
  (hbo_acq / hbo_acq_grad) and an HGP of 3 parameter samples (hbo_acq_samples / the mean of the per-sample hbo_acq_grad values).
  The bound of a mean over samples is the mean of the samples' bounds times their EI (from the oracle's posterior per sample)."""
  nv = _native()
  kname, mname, d, n, m_q = 'squared_exponential', 'constant', 3, 150, 7
  rng = np.random.default_rng(63)
  samples = [helpers.make_model(np.random.default_rng(400 + i), mname, False, d) for i in range(n_samples)]
  x, y = helpers.synthetic_task(rng, n, d)
  x2, y2 = helpers.synthetic_task(rng, 20, d)
  xq = rng.uniform(size=(m_q, d))
  ds = {0: nv.defs.SubDataset(x, y), 1: nv.defs.SubDataset(x2, y2), 2: nv.defs.SubDataset(x2[:5], y2[:5])}   # scale 3 / 2
  params = nv.defs.GPParams(model=samples[0], samples=samples if n_samples > 1 else [], config={})
  cls = nv.gp.HGP if n_samples > 1 else nv.gp.GP
  model = cls(ds, nv.mean.constant, nv.kernel.squared_exponential, params, nv.utils.DEFAULT_WARP_FUNC)
  post = []
  for smp in samples:
    po = o.GPParams(model=smp, config={})
    mu, var = o.predict(o.constant, o.squared_exponential, po, x, y, xq, WFO)
    noise = float(np.squeeze(o.retrieve_params(po, ['noise_variance'], WFO)[0]))
    mu, var = np.ravel(mu), np.ravel(var)
    c = types.SimpleNamespace(dtype=np.dtype(np.float64), mu_o=mu, var_o=var)
    post.append((c, mu, np.sqrt((var + noise) * SCALE)))
  fn = nv.acfun.expected_improvement
  bad, worst, reached = [], (0.0, None), set()
  for k, g in enumerate(ao.GAMMAS):
    qk = (k * 5) % m_q
    # the sample that needs the smallest (gamma < 0: largest) target sits at gamma; the other samples between it and 0
    target = float((min if g >= 0 else max)(mu[qk] + g * sd[qk] for _, mu, sd in post))
    a = fn(model=model, sub_dataset_key=0, x_queries=xq, acfun_callback=lambda m_, k_: target)
    b, _ = fn.value_and_grad(model=model, sub_dataset_key=0, x_queries=xq, acfun_callback=lambda m_, k_: target)
    assert a.shape == (m_q, 1) and b.shape == (m_q, 1)
    for q in range(m_q):
      gs = [ao.exact_gamma(mu[q], sd[q], target) for _, mu, sd in post]
      if not all(-10.25 <= gq <= 37.25 for gq in gs):    # (_window: a sample aimed at 37 may sit an ulp beyond)
        continue
      if q == qk and min(abs(gq - g) for gq in gs) <= 1e-6:
        reached.add(g)
      absb = np.mean([(_posterior_term(c, gq, float(sd[q]), True) + 2 * _epilogue_bound(gq, np.float64)) * float(ao.exact_ei(mu[q], sd[q], target))
                      for gq, (c, mu, sd) in zip(gs, post)])
      absb *= 1.0 + 1e-6    # (the bounds are relative to the device's values; the oracle's EI stands in for them)
      r = abs(float(a[q, 0]) - float(b[q, 0])) / absb if np.isfinite(a[q, 0]) and np.isfinite(b[q, 0]) else np.inf
      if r > worst[0]:
        worst = (r, (g, q, [round(v, 3) for v in gs]))
      if not r <= 1.0:
        bad.append((g, q, [round(v, 3) for v in gs], float(a[q, 0]), float(b[q, 0]), r))
  nv.acfun.drop_sample_caches(model)
  _record(f'fp64 acfun value vs value_and_grad ({n_samples} sample(s))', worst[0], str(worst[1]))
  assert not bad, f'{len(bad)} queries disagree; first: {bad[:5]}'
  assert reached == set(ao.GAMMAS), sorted(set(ao.GAMMAS) - reached)


# ---- (c) sign and order ----------------------------------------------------------------------------------------------------
def _tail_candidates(c_pool, count=200, lo=6.0, hi=12.0, margin=0.2):
  """`count` candidates of a pool of uniform draws that one target puts at gamma in [lo + margin, hi - margin] under the oracle's
  posterior: the target is the pool's largest mu plus (lo + margin) of the largest sd, so no candidate sits below lo + margin; of
  those below hi - margin, `count` spread evenly over the range are kept (a selection by the posterior, not a construction)."""
  target = float(c_pool.dtype.type(np.max(c_pool.mu_o) + (lo + margin) * np.max(c_pool.sd_o)))
  gam = (target - c_pool.mu_o) / c_pool.sd_o
  idx = np.flatnonzero((gam >= lo + margin) & (gam <= hi - margin))
  if idx.size > count:    # spread over the whole range: every (size / count)-th of them in the order of gamma, back in the order of the draw
    idx = np.sort(idx[np.argsort(gam[idx], kind='stable')][np.linspace(0, idx.size - 1, count).astype(int)])
  return target, idx


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['fp64', 'fp32'])
def test_sign_and_order_of_200_tail_candidates(gpu_ctx, dtype):
  """One call, one target, 200 candidates all at gamma in [6, 12]: every EI is > 0 and finite, the device's ordering of the candidates
  is the ordering of exact_ei on the device's own mu, var, argmax included.  A pair is left out only when its exact values are closer
  than the sum of its two bounds of (a): at most 2 of the 199 adjacent pairs.  fp64 also: at gamma = 40, 0 or a denormal."""
  c = _case(gpu_ctx, 'squared_exponential', False, 'constant', 150, 4000, dtype, seed=64)
  try:
    target, idx = _tail_candidates(c)
    assert idx.size == 200
    c.xq = np.ascontiguousarray(c.xq[idx]); c.m_q = 200
    mu, var = _predict(c)
    sd = _device_sd(c, var)
    gam = np.array([ao.exact_gamma(m, s, target) for m, s in zip(mu, sd)])
    assert gam.min() >= 5.5 and gam.max() <= 12.5, (gam.min(), gam.max())     # still in the tail on the device's own posterior
    ei = _acq(c, ACQ_EI, target)
    assert np.isfinite(ei).all() and (ei > 0).all(), (ei[~(ei > 0)], gam[~(ei > 0)])
    exact = [ao.exact_ei(m, s, target) for m, s in zip(mu, sd)]
    order = sorted(range(200), key=lambda i: exact[i], reverse=True)
    left_out, wrong = 0, []
    for i, j in zip(order[:-1], order[1:]):
      if exact[i] - exact[j] <= _epilogue_bound(gam[i], dtype) * exact[i] + _epilogue_bound(gam[j], dtype) * exact[j]:
        left_out += 1
      elif not ei[i] > ei[j]:
        wrong.append((i, j, gam[i], gam[j], float(ei[i]), float(ei[j])))
    assert left_out <= 2, left_out
    assert not wrong, f'{len(wrong)} adjacent pairs out of order, smallest gamma {min(w[2] for w in wrong)}; first: {wrong[:5]}'
    assert int(np.argmax(ei)) == order[0]
    if left_out == 0:
      assert list(np.argsort(-ei.astype(np.float64), kind='stable')) == order
    print(f'\nacq tails: {c.dtype.name} order: gamma in [{gam.min():.2f}, {gam.max():.2f}], pairs left out {left_out}')
    if c.dtype == np.float64:
      t40 = float(mu[0] + 40.0 * sd[0])
      z = _acq(c, ACQ_EI, t40)[0]
      assert z == z and 0.0 <= z < np.finfo(np.float64).tiny * sd[0], z
  finally:
    _close(c)


# ---- (d) the gradient in the tail, per query -------------------------------------------------------------------------------
@pytest.mark.parametrize('kname,mlp,mname', CASES, ids=CASE_IDS)
def test_tail_gradient_per_query_fp64(gpu_ctx, kname, mlp, mname):
  """d EI / d x from hbo_acq_grad against o.acquisition_value_and_grad at gamma in {5, 8, 12, 20}, each query against ITS OWN largest
  gradient component (a bound relative to the largest gradient of the batch is one a tail query never reaches)."""
  c = _case(gpu_ctx, kname, mlp, mname, 150, 7, np.float64, seed=65)
  try:
    bad, worst, reached = [], (0.0, None), set()
    for k, g in enumerate((5.0, 8.0, 12.0, 20.0)):
      qk = (k * 5) % 7
      target = _target(c, qk, g)
      _, grad = _acq_grad(c, ACQ_EI, target)
      _, gref = o.acquisition_value_and_grad('ei', c.mo, c.ko, c.po, c.x64, c.y64, c.xq64, target, WFO, add_noise=c.noise, scale=SCALE)
      for q in range(7):
        gq = float((target - c.mu_o[q]) / c.sd_o[q])
        if not -10.0 <= gq <= 20.25:
          continue
        if q == qk:
          reached.add(g)
        tol = 1e-7 * (1.0 + gq * gq)
        r = np.max(np.abs(grad[q] - gref[q])) / (tol * np.max(np.abs(gref[q]))) if np.isfinite(grad[q]).all() else np.inf
        if float(r) > worst[0]:
          worst = (float(r), (g, q, round(gq, 3)))
        if not r <= 1.0:
          bad.append((g, q, round(gq, 3), grad[q].tolist(), gref[q].tolist(), float(r)))
    _record('fp64 tail gradient', worst[0], f'{worst[1]} {kname}')
    assert not bad, bad[:3]
    assert reached == {5.0, 8.0, 12.0, 20.0}
  finally:
    _close(c)


@pytest.mark.parametrize('acq', ['ei', 'pi'])
@pytest.mark.parametrize('kname,mlp,mname', CASES, ids=CASE_IDS)
def test_gradient_per_query_fp32(gpu_ctx, kname, mlp, mname, acq):
  """fp32, EI and PI (the suite had UCB only), per query, at gamma in {0, 2, 3}: 2e-2 * (1 + gamma**2)."""
  c = _case(gpu_ctx, kname, mlp, mname, 150, 7, np.float32, seed=66)
  try:
    bad, worst, reached = [], (0.0, None), set()
    for k, g in enumerate((0.0, 2.0, 3.0)):
      qk = (k * 5) % 7
      target = _target(c, qk, g)
      val, grad = _acq_grad(c, ACQ_EI if acq == 'ei' else ACQ_PI, target)
      assert val.dtype == np.float32 and grad.dtype == np.float64
      _, gref = o.acquisition_value_and_grad(acq, c.mo, c.ko, c.po, c.x64, c.y64, c.xq64, target, WFO, add_noise=c.noise, scale=SCALE)
      for q in range(7):
        gq = float((target - c.mu_o[q]) / c.sd_o[q])
        if not -3.25 <= gq <= 3.25:
          continue
        if q == qk:
          reached.add(g)
        tol = 2e-2 * (1.0 + gq * gq)
        r = np.max(np.abs(grad[q] - gref[q])) / (tol * np.max(np.abs(gref[q]))) if np.isfinite(grad[q]).all() else np.inf
        if float(r) > worst[0]:
          worst = (float(r), (g, q, round(gq, 3)))
        if not r <= 1.0:
          bad.append((g, q, round(gq, 3), grad[q].tolist(), gref[q].tolist(), float(r)))
    _record(f'fp32 gradient {acq}', worst[0], f'{worst[1]} {kname}')
    assert not bad, bad[:3]
    assert reached == {0.0, 2.0, 3.0}
  finally:
    _close(c)
