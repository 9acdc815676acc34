"""tests/logei_cases.py judged on its own, and the host side of log expected improvement: no device.  The restatement of
csrc/kernfun.h: logei_terms against mpmath (the constants of the bounds are MEASURED here), the mutants, the rules, the S-sample
combination, the argument checks of the three new entry points, and the premise of the feature: a start on the flat tail of EI where
EI's maximiser stops without moving and LogEI's does not."""
import ctypes as C
import os

import mpmath as mp
import numpy as np
import pytest

import acq_opt_oracle as ao
import logei_cases as lc
from hyperbo_amd import _native as nat
from hyperbo_amd.bo_utils import acfun, bayesopt

# u in [-1, 40] and -u in [1, 3e7] (log-spaced), the neighbours of the two switch points, and U itself
GRID = np.unique(np.concatenate([np.arange(-1.0, 40.0 + 1e-9, 0.025), -np.logspace(0.0, np.log10(3e7), 1200), np.array(lc.U),
                                 [np.nextafter(-1.0, 0.0), np.nextafter(-1.0, -2.0), -lc.SERIES_U, np.nextafter(-lc.SERIES_U, 0.0),
                                  np.nextafter(-lc.SERIES_U, -1e3)]]))


def test_restatement_against_mpmath():
  """The worst error of stable_terms against exact_terms over the grid, in units of eps64 (1 + u^2): C_VALUE, C_CDF and C_PDF are
  these numbers rounded up, by less than a factor of two; the device's bound is DEVICE_FACTOR = 8 times them, so the restatement sits
  at or below an eighth of it.  No result is non-finite."""
  got = lc.stable_terms(GRID)
  assert all(np.all(np.isfinite(g)) for g in got)
  worst, where = [0.0, 0.0, 0.0], [None] * 3
  for i, u in enumerate(GRID):
    r = lc.term_ratios(u, [g[i] for g in got])
    for k, c in enumerate((lc.C_VALUE, lc.C_CDF, lc.C_PDF)):
      if r[k] * c > worst[k]:
        worst[k], where[k] = r[k] * c, float(u)
  print(f'\nlogei: measured constants (value, cdf / h, pdf / h): {worst[0]:.3f} at u = {where[0]}, {worst[1]:.3f} at {where[1]}, {worst[2]:.3f} at {where[2]}')
  for w, c in zip(worst, (lc.C_VALUE, lc.C_CDF, lc.C_PDF)):
    assert w <= c <= 2.0 * w, (worst, where)


def test_every_u_of_the_list_and_both_sides_of_the_switch_points():
  """Each u of U, and the last float on either side of u = -1 and u = -SERIES_U: inside a quarter of the device's bounds, and the two
  forms agree across each switch to the same bounds (the function is continuous; a wrong constant in either form would show here)."""
  pts = list(lc.U) + [np.nextafter(-1.0, 0.0), np.nextafter(-1.0, -2.0), -lc.SERIES_U, np.nextafter(-lc.SERIES_U, -1e3)]
  for u in pts:
    r = lc.term_ratios(u, [float(t) for t in lc.stable_terms(np.float64(u))])
    assert max(r) <= 0.25 * lc.DEVICE_FACTOR, (u, r)
  assert -1.0 - 2.0**-40 in lc.U and -1.0 in lc.U and min(lc.U) == -3e7 and max(lc.U) == 1e3
  for a, b in ((np.nextafter(-1.0, 0.0), -1.0), (-lc.SERIES_U, np.nextafter(-lc.SERIES_U, -1e3))):
    ta, tb = lc.stable_terms(np.float64(a)), lc.stable_terms(np.float64(b))
    assert abs(ta[0] - tb[0]) <= 2 * lc.C_VALUE * lc.unit(a)
    assert abs(ta[1] - tb[1]) <= 2 * lc.C_CDF * lc.unit(a) * abs(ta[1]) and abs(ta[2] - tb[2]) <= 2 * lc.C_PDF * lc.unit(a) * abs(ta[2])


def test_limits_and_nan():
  for u, want in ((np.inf, (np.inf, 0.0, 0.0)), (-np.inf, (-np.inf, np.inf, np.inf))):
    got = tuple(float(t) for t in lc.stable_terms(np.float64(u)))
    assert got == want == lc.exact_terms(u), (u, got)
  assert all(np.isnan(float(t)) for t in lc.stable_terms(np.float64(np.nan)))
  # finite for every finite u whose square does not overflow
  for u in (-1e8, -1e12, -1e100, -1e154):
    assert all(np.isfinite(float(t)) for t in lc.stable_terms(np.float64(u))), u


def _ratios(case, mutant=None):
  mu, var, noise, scale, _ = case
  t = lc.scalar_case_target(case)
  got = lc.scalars(mu, var, noise, scale, t, mutant)
  exact, bound = lc.exact_scalars(mu, var, noise, scale, t)
  out = []
  for g, e, b in zip(got, exact, bound):
    if not (np.isfinite(g) and np.isfinite(e)):
      out.append(0.0 if g == e else np.inf)
    else:
      out.append(abs(g - e) / b if b > 0 else (0.0 if g == e else np.inf))
  return out


def test_the_scalar_step_restated_is_inside_a_quarter_of_the_device_bounds():
  for case in lc.SCALAR_CASES:
    assert max(_ratios(case)) <= 0.25, (case, _ratios(case))


@pytest.mark.parametrize('mutant', lc.MUTANTS)
def test_every_mutant_is_rejected_by_some_case(mutant):
  if mutant == 'mean_of_logs':
    hit = []
    for vals, _ in lc.COMBINE_CASES:
      got, exact = lc.combine(vals, mutant=mutant)[0], lc.exact_combine(vals)[0]
      hit.append(not (got == exact or abs(got - exact) <= 8 * lc.EPS64 * (1.0 + abs(exact))))
    assert any(hit) and not hit[2]          # S = 1: the two rules coincide
    return
  assert any(max(_ratios(case, mutant)) > 1.0 for case in lc.SCALAR_CASES), mutant


def test_exact_slopes_against_central_differences_of_the_exact_value():
  """a_mu and a_var of exact_scalars against central differences of the mpmath value in mu and in var (400 digits, step 1e-20: the
  slope in var is 1e-316 at u = 40, a difference of 1e-336 in a value of order one)."""
  for case in lc.SCALAR_CASES[:len(lc.U)] + lc.SCALAR_CASES[len(lc.U) + 2:len(lc.U) + 3]:
    mu, var, noise, scale, u = case
    if abs(u) > 1e5:
      continue
    t = lc.scalar_case_target(case)
    with mp.workdps(400):
      def value(m, v):
        sd = mp.sqrt((v + mp.mpf(noise)) * mp.mpf(scale))
        uu = (m - mp.mpf(t)) / sd
        return mp.log(sd) + mp.log(mp.npdf(uu) + uu * mp.ncdf(uu))
      hm, hv = mp.mpf(10)**-20, mp.mpf(10)**-20
      dmu = (value(mp.mpf(mu) + hm, mp.mpf(var)) - value(mp.mpf(mu) - hm, mp.mpf(var))) / (2 * hm)
      dvar = (value(mp.mpf(mu), mp.mpf(var) + hv) - value(mp.mpf(mu), mp.mpf(var) - hv)) / (2 * hv)
    (_, amu, avar), _ = lc.exact_scalars(mu, var, noise, scale, t)
    assert abs(amu - float(dmu)) <= 1e-12 * abs(float(dmu)) and abs(avar - float(dvar)) <= 1e-12 * abs(float(dvar)), (case, amu, dmu, avar, dvar)


def test_the_rules():
  s = lc.scalars
  assert s(0.5, 0.0, 0.0, 1.5, 0.25) == (float(np.log(0.25)), 4.0, 0.0)                 # v2 = 0, mu above the target
  assert s(0.5, 0.0, 0.0, 1.5, 0.5) == (-np.inf, 0.0, 0.0) and s(0.5, 0.2, -0.3, 1.5, 0.75) == (-np.inf, 0.0, 0.0)
  assert all(np.isnan(v) for v in s(0.5, np.nan, 0.0, 1.5, 0.25)) and all(np.isnan(v) for v in s(0.5, 0.1, np.nan, 1.5, 0.25))
  assert s(0.0, 1.0, 0.0, 1.0, 1e300) == (-np.inf, 0.0, 0.0)                           # u^2 overflows: -inf carries no slope
  v, amu, avar = s(0.0, 1.0, 0.0, 1.0, -1e300)
  assert np.isfinite(v) and amu >= 0.0 and avar == 0.0
  assert lc.exact_scalars(0.5, 0.0, 0.0, 1.5, 0.5)[0] == (-np.inf, 0.0, 0.0)
  # the host route of acfun is the same function
  mu, sd = np.array([0.3, -2.0, 0.5, 0.5, 0.1]), np.array([0.9, 1e-3, 0.0, 0.0, np.nan])
  got = acfun.log_expected_improvement_sub(mu, sd, 0.4)
  want = [s(m, v * v, 0.0, 1.0, 0.4)[0] for m, v in zip(mu[:2], sd[:2])]
  assert np.allclose(got[:2], want, rtol=1e-14, atol=0) and got[2] == np.log(0.5 - 0.4) and np.isnan(got[4])
  assert acfun.log_expected_improvement_sub(0.3, 0.0, 0.4) == -np.inf
  for u in lc.U:
    a, b = acfun.logei_terms_host(np.float64(u)), lc.stable_terms(np.float64(u))
    assert all(float(x) == float(y) for x, y in zip(a, b)), u
  assert acfun.LOGEI_SERIES_U == lc.SERIES_U
  src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'hyperbo_amd', 'csrc', 'kernfun.h')).read()
  assert f'#define LOGEI_SERIES_U {lc.SERIES_U}' in src


def test_combine_against_mpmath():
  rng = np.random.default_rng(5)
  for vals, dead in lc.COMBINE_CASES:
    grads = rng.normal(size=(len(vals), 3))
    if dead is not None:
      grads[dead] = 0.0
    val, grad = lc.combine(vals, grads)
    ev, eg = lc.exact_combine(vals, grads)
    if np.isfinite(ev):
      assert abs(val - ev) <= 4 * lc.EPS64 * (1.0 + abs(ev)) and np.all(np.abs(grad - eg) <= 8 * lc.EPS64 * np.max(np.abs(grads))), (vals, val, ev)
    else:
      assert val == ev == -np.inf and np.all(grad == 0.0)
    hv, hg = acfun.logei_combine(np.asarray(vals)[:, None], grads[:, None, :])
    assert (hv[0] == val or abs(hv[0] - val) <= 2 * lc.EPS64 * abs(val)) and np.allclose(hg[0], grad, rtol=1e-15, atol=1e-300)
  # a -inf row among finite ones is the combination of the others shifted by log((S - 1) / S)
  assert abs(lc.combine([-1.0, -np.inf, -2.0])[0] - (lc.combine([-1.0, -2.0])[0] + np.log(2.0 / 3.0))) <= 4 * lc.EPS64
  # S = 1 returns its input to the bit, value and gradient
  g = rng.normal(size=(1, 5))
  for v in (0.1234567, -745.5, 1e-300, -3e14):
    val, grad = lc.combine([v], g)
    assert val == v and grad.tobytes() == g[0].tobytes()
    hv, hg = acfun.logei_combine(np.array([[v]]), g[:, None, :])
    assert hv[0] == v and hg[0].tobytes() == g[0].tobytes()
  assert np.isnan(lc.combine([0.5, np.nan])[0]) and np.isnan(acfun.logei_combine(np.array([[0.5], [np.nan]]))[0])
  assert acfun.logei_combine(np.array([[-np.inf], [-np.inf]]))[0] == -np.inf


def test_the_cases_cover_the_edges():
  cs = lc.CASES
  assert {n for c in cs for n in c.ns} == {5, 128, 129, 300} and {c.d for c in cs} == {1, 3, 17} and {c.S for c in cs} == {1, 3}
  assert {c.kname for c in cs} == {'squared_exponential', 'matern32', 'matern52', 'dot_product'}
  assert {c.mname for c in cs} == {'zero', 'constant', 'linear', 'linear_mlp'} and {c.dtype for c in cs} == {'fp64', 'fp32'}
  assert max(c.M for c in cs) <= 24 and len({c.id for c in cs}) == len(cs)
  assert any(c.feats == (8, 8) and c.mlp_k for c in cs) and any(c.feats and not c.mlp_k for c in cs)
  assert any(min(c.ns) <= 128 < max(c.ns) for c in cs)


# ---- the host side of the feature --------------------------------------------------------------------------------------------------
NEW = ('hbo_acq_logei', 'hbo_logei_grad_samples', 'hbo_logei_maximize', 'hbo_probe_logei_grad_samples64')


def test_entry_points_are_exported_bound_and_documented():
  for name in NEW:
    assert name in nat.SIGNATURES, name
    f = getattr(nat.lib(), name)
    res, args = nat.SIGNATURES[name]
    assert f.restype is res and list(f.argtypes) == args, name
  sib, mine = nat.SIGNATURES['hbo_acq_grad_samples_mlp'][1], nat.SIGNATURES['hbo_logei_grad_samples'][1]
  assert mine == sib[:6] + sib[7:]                                  # targets [S] in the place of acq_id, params
  sib, mine = nat.SIGNATURES['hbo_acq_maximize_mlp'][1], nat.SIGNATURES['hbo_logei_maximize'][1]
  assert mine == sib[:8] + sib[9:]
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  hbo, tune = (open(os.path.join(root, 'include', f)).read() for f in ('hbo.h', 'hbo_tune.h'))
  for name in NEW[:3]:
    assert f'int {name}(' in hbo, name
  assert 'int hbo_probe_logei_grad_samples64(' in tune
  for f in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
    assert 'hbo_acq_logei' in open(os.path.join(root, f)).read(), f
  assert 'logei.hip' in open(os.path.join(root, 'hyperbo_amd', 'csrc', 'Makefile')).read()
  assert acfun.log_ei is acfun.log_expected_improvement and acfun.log_ei.__name__ == 'log_ei'


def test_argument_errors_come_before_any_device_call():
  err = lambda: (nat.lib().hbo_last_error(None) or b'').decode()
  pd = C.POINTER(C.c_double)
  xq, out, grad = np.zeros((1, 2)), np.full((1, 1), 7.0), np.full((1, 1, 2), 7.0)
  models, caches, nse = (nat.Model * 1)(), (C.c_void_p * 1)(), (C.c_double * 1)()
  tg = np.array([0.5])
  tp = lambda a: None if a is None else a.ctypes.data_as(pd)
  lib = nat.lib()
  # hbo_acq_logei
  acq = lambda t=0.5, m=models, o=out: lib.hbo_acq_logei(None, m, None, nat.ptr(xq), 1, t, 0.0, 1.0, nat.ptr(o))
  assert acq(m=None) == nat.HBO_ERR_ARG and 'hbo_acq_logei: null argument' in err()
  assert acq(o=None) == nat.HBO_ERR_ARG and 'null argument' in err()
  for v in (np.nan, np.inf, -np.inf):
    assert acq(t=v) == nat.HBO_ERR_ARG and 'not finite' in err()
  assert acq() == nat.HBO_ERR_ARG and 'hbo_acq_logei: ctx is null' in err()
  # hbo_logei_grad_samples: its own checks, then those of hbo_acq_grad_samples_mlp
  gs = lambda S=1, t=tg, m=models: lib.hbo_logei_grad_samples(None, m, S, caches, nat.ptr(xq), 1, tp(t), nse, 1.0, nat.ptr(out), tp(grad))
  assert gs(t=None) == nat.HBO_ERR_ARG and 'hbo_logei_grad_samples: null argument' in err()
  assert gs(m=None) == nat.HBO_ERR_ARG and 'null argument' in err()
  assert gs(S=4097) == nat.HBO_ERR_ARG and '1 <= S <= 4096' in err()
  assert gs(t=np.array([np.nan])) == nat.HBO_ERR_ARG and 'not finite' in err()
  assert gs() == nat.HBO_ERR_ARG and 'hbo_logei_grad_samples: ctx is null' in err()
  v64 = np.full((1, 1), 7.0)
  probe = lambda chunk, v: lib.hbo_probe_logei_grad_samples64(None, models, 1, caches, nat.ptr(xq), 1, tp(tg), nse, 1.0, nat.ptr(out), tp(grad), 1, chunk, v)
  assert probe(0, None) == nat.HBO_ERR_ARG and 'val64_out is null' in err()
  assert probe(-1, tp(v64)) == nat.HBO_ERR_ARG and 'chunk_queries < 0' in err()
  # hbo_logei_maximize
  opts = nat.AcqOptOpts(**acfun.ACQ_OPT_DEFAULTS)
  ns = lib.hbo_acq_opt_state_doubles(2, opts.memory)
  state, x, val, status = np.zeros((1, ns)), np.full((1, 2), 7.0), np.full(1, 7.0), np.full(1, 7, dtype=np.int32)
  mx = lambda S=1, t=tg: lib.hbo_logei_maximize(None, models, S, caches, nat.ptr(xq), 1, None, None, tp(t), nse, 1.0, C.byref(opts), nat.ptr(state), 1,
                                                nat.ptr(x), nat.ptr(val), nat.ptr(status), None)
  assert mx(t=None) == nat.HBO_ERR_ARG and 'hbo_logei_maximize: null argument' in err()
  assert mx(S=0) == nat.HBO_ERR_ARG and 'hbo_logei_maximize: 1 <= S <= 4096' in err()
  assert mx(t=np.array([np.inf])) == nat.HBO_ERR_ARG and 'not finite' in err()
  assert mx() == nat.HBO_ERR_ARG and 'hbo_logei_maximize: ctx is null' in err()
  for a in (out, grad, v64, x, val):
    assert np.all(a == 7.0)                               # no output was touched
  assert np.all(status == 7) and not state.any()


def test_the_existing_entry_points_keep_refusing_a_fourth_acq_id():
  err = lambda: (nat.lib().hbo_last_error(None) or b'').decode()
  pd = C.POINTER(C.c_double)
  lib = nat.lib()
  xq, out, grad = np.zeros((1, 2)), np.full((1, 1), 7.0), np.full((1, 1, 2), 7.0)
  models, caches, nse, prm = (nat.Model * 1)(), (C.c_void_p * 1)(), (C.c_double * 1)(), (C.c_double * 1)()
  assert lib.hbo_acq(None, models, None, nat.ptr(xq), 1, 3, 0.0, 0.0, 1.0, nat.ptr(out)) == nat.HBO_ERR_ARG and 'bad acq_id' in err()
  for name in ('hbo_acq_grad_samples', 'hbo_acq_grad_samples_blocked', 'hbo_acq_grad_samples_mlp'):
    assert getattr(lib, name)(None, models, 1, caches, nat.ptr(xq), 1, 3, prm, nse, 1.0, nat.ptr(out), grad.ctypes.data_as(pd)) == nat.HBO_ERR_ARG, name
    assert 'bad acq_id' in err(), name
  opts = nat.AcqOptOpts(**acfun.ACQ_OPT_DEFAULTS)
  state, x, val, status = np.zeros((1, lib.hbo_acq_opt_state_doubles(2, opts.memory))), np.full((1, 2), 7.0), np.full(1, 7.0), np.full(1, 7, dtype=np.int32)
  for name in ('hbo_acq_maximize', 'hbo_acq_maximize_blocked', 'hbo_acq_maximize_mlp'):
    rc = getattr(lib, name)(None, models, 1, caches, nat.ptr(xq), 1, None, None, 3, prm, nse, 1.0, C.byref(opts), nat.ptr(state), 1, nat.ptr(x),
                            nat.ptr(val), nat.ptr(status), None)
    assert rc == nat.HBO_ERR_ARG and 'bad acq_id' in err(), name
  assert np.all(out == 7.0) and np.all(grad == 7.0) and np.all(x == 7.0)


def test_the_device_loop_names_log_ei_as_outside_its_registry():
  import types
  model = types.SimpleNamespace(params=types.SimpleNamespace(config={}), cov_func=None, dataset={})
  msg = bayesopt._bo_on_device_unmet(model, 't', types.SimpleNamespace(x=np.zeros((3, 2)), y=np.zeros((3, 1))), acfun.log_ei)
  assert msg is not None and 'log_ei' in msg and 'registry' in msg
  assert acfun.log_ei not in acfun._BO_DEVICE


# ---- the premise ---------------------------------------------------------------------------------------------------------------------
def test_the_flat_tail_premise():
  """At the start of logei_cases.flat_tail_problem u lies between -14 and -10.  EI's projected-gradient measure from the oracle is
  below pgtol = 1e-5 there, so the optimiser of csrc/acq_opt_ctl.h (acq_opt_oracle.minimise) stops CONVERGED on its first evaluation,
  where it started.  Driven by the oracle's LogEI the same optimiser leaves the start and ends at the point SciPy's L-BFGS-B reaches on
  the oracle's LogEI from that start (tolerances tightened so that SciPy's end is the maximiser itself): within 1e-4, which is what
  ftol = 2.2e-9 of |f| = 5 leaves under a curvature of order 1e2 (dx ~ sqrt(2 * 1e-8 / 1e2)); the measured distance is 2.4e-7."""
  p = lc.flat_tail_problem()
  _, _, u = lc.oracle_value_and_grad(p.smp[0], p.x0[None, :], p.target)
  assert -14.0 < u[0] < -10.0, u
  ei, logei = lc.flat_tail_ei(p), lc.flat_tail_logei(p)
  ve, ge = ei(p.x0)
  assert ao.pg_measure(p.x0, -ge[0], p.lo, p.hi) < ao.DEFAULTS['pgtol'] and 0.0 <= ve[0] < 1e-20
  run_ei = ao.minimise(ei, p.x0, p.lo, p.hi)
  assert run_ei.status == ao.CONVERGED and len(run_ei.log) == 1 and np.array_equal(run_ei.x, p.x0)
  run, x_scipy, dist, v_scipy = lc.flat_tail_reference()
  assert run.status in (ao.CONVERGED, ao.FTOL) and np.max(np.abs(run.x - p.x0)) > 0.1 and len(run.log) > 5
  print(f'\nlogei: flat tail: u = {u[0]:.3f}, EI {ve[0]:.3e}; LogEI {len(run.log)} evaluations, status {run.status}, end {run.x}, SciPy {x_scipy}, distance {dist:.3e}')
  assert dist <= 1e-4 and v_scipy >= -run.f - 1e-8
  assert -run.f > float(logei(p.x0)[0][0]) + 10.0           # EI grew by a factor of e^10 at least
