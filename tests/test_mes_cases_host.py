"""CPU tier of max-value entropy search: tests/mes_cases.py judged on its own -- the float64 restatement of the stable forms against
mpmath (which also MEASURES the constants of the GPU tier's bounds), h >= 0 and monotone, every mutant outside the bounds on some
case, the oracle's gradient against central differences -- and the host side of the feature: max_value_samples' clamp and the
ValueErrors on stubs, the bindings, and the argument checks of the three entry points, which run before any device call."""
import ctypes as C
import os

import numpy as np
import pytest

import mes_cases as mc
from hyperbo_amd import _native as nat
from hyperbo_amd.basics import definitions as defs
from hyperbo_amd.bo_utils import acfun
from hyperbo_amd.gp_utils import gp, kernel, mean

GRID = np.round(np.arange(-30.0, 38.5 + 1e-9, 0.05), 2)


def test_restatement_against_mpmath():
  """On gamma in [-30, 38.5], 0.05 apart: the worst error of the restatement in units of eps64 * (the scale of the un-cancelled terms)
  IS the constant of the bounds (C_VALUE, C_SLOPE; C_TAIL in units of eps64 (1 + gamma^2) h for gamma >= 0): measured <= C <= 2 measured."""
  h, dh = mc.stable_terms(GRID)
  assert np.all(np.isfinite(h)) and np.all(np.isfinite(dh))
  cv = cs = ct = 0.0
  for g, hv, dv in zip(GRID, h, dh):
    eh, ed, sh, sdh = mc.exact_terms(float(g))
    cv = max(cv, abs(hv - eh) / (mc.EPS64 * sh))
    cs = max(cs, abs(dv - ed) / mc.slope_unit(g, sdh))
    if g >= 0:
      ct = max(ct, abs(hv - eh) / (mc.EPS64 * (1.0 + g * g) * eh + (1.0 + g) * mc.QUANTUM))
  print(f'\nmes host: restatement against mpmath: value {cv:.3f}, slope {cs:.3f}, positive tail {ct:.3f}')
  for measured, const in ((cv, mc.C_VALUE), (cs, mc.C_SLOPE), (ct, mc.C_TAIL)):
    assert measured <= const <= 2.0 * measured, (measured, const)
  h, dh = mc.stable_terms(np.array([-np.inf, np.inf]))
  assert h[0] == np.inf and h[1] == 0.0 and dh[0] == 0.0 and dh[1] == 0.0
  assert mc.exact_terms(np.inf)[:2] == (0.0, 0.0) and mc.exact_terms(-np.inf)[:2] == (np.inf, 0.0)
  assert np.all(np.isnan(mc.stable_terms(np.array([np.nan]))[0]))


def test_reference_precision_is_raised_until_it_stops_mattering():
  """At 60 digits a literal 1 - ncdf(-20) is 1; the reference must not depend on its starting precision."""
  with mc.mp.workdps(60):
    assert 1 - mc.mp.ncdf(-20) == 1
  a = mc.exact_terms(20.0)
  b = tuple(float(v) for v in mc._mp_terms(20.0, 400))
  assert a == b and a[0] > 0.0


def test_h_is_nonnegative_and_monotone():
  h, dh = mc.stable_terms(GRID)
  assert np.all(h >= 0.0) and np.all(dh <= 0.0)
  exact = np.array([mc.exact_terms(float(g))[0] for g in GRID])
  assert np.all(exact > 0.0) and np.all(np.diff(exact) < 0.0)
  # the restatement decreases too, up to the bound of either neighbour
  slack = np.array([mc.value_term_bound(float(g), e, mc.exact_terms(float(g))[2]) for g, e in zip(GRID, exact)])
  assert np.all(np.diff(h) <= slack[1:] + slack[:-1])
  assert mc.stable_terms(np.array([60.0]))[0][0] == 0.0          # 0 by underflow, never negative


def _ratios(case, mutant=None):
  mu, var, noise, scale, _ = case
  ys = mc.scalar_case_maxima(case)
  exact, bound = mc.exact_scalars(mu, var, noise, scale, ys)
  got = mc.scalars(mu, var, noise, scale, ys, mutant)
  return [(0.0 if a == e else np.inf) if b == 0.0 else (abs(a - e) / b if np.isfinite(a) else np.inf) for a, e, b in zip(got, exact, bound)]


def test_the_scalar_step_restated_is_inside_the_device_bounds():
  for case in mc.SCALAR_CASES:
    assert max(_ratios(case)) <= 1.0 / mc.DEVICE_FACTOR + 1e-12, (case, _ratios(case))


@pytest.mark.parametrize('mutant', mc.MUTANTS)
def test_every_mutant_is_rejected_by_some_case(mutant):
  worst = max(max(_ratios(case, mutant)) for case in mc.SCALAR_CASES)
  assert worst > 1.0, (mutant, worst)


def test_the_clamp_mutant_is_rejected():
  ys, y = np.array([0.1, 0.9]), np.array([[0.2], [0.5]])
  assert np.array_equal(mc.clamp_maxima(ys, y), [0.5, 0.9]) and np.array_equal(mc.clamp_maxima(ys, None), ys)
  assert not np.array_equal(mc.clamp_maxima(ys, y, 'no_clamp'), mc.clamp_maxima(ys, y))
  # what the clamp prevents: gamma < 0 at the incumbent, whose MES value would then be the pool's largest
  assert mc.stable_terms(np.array([(0.1 - 0.5) / 0.05]))[0][0] > mc.stable_terms(np.array([0.0]))[0][0]


def test_oracle_gradient_against_central_differences():
  case = mc.Case('matern52', 'linear', (20,), 3, 7, 4, 'fp64')
  p = mc.problem(case)
  sm = p.smp[0]
  val, grad, gam = mc.oracle_value_and_grad(sm, p.xq, p.ystar[0])
  assert np.all(val >= 0.0) and gam.shape == (4, 7)
  step = 1e-6
  for q in range(case.M):
    for d in range(case.d):
      xp, xm = p.xq.copy(), p.xq.copy()
      xp[q, d] += step; xm[q, d] -= step
      fd = (mc.oracle_value_and_grad(sm, xp, p.ystar[0])[0][q] - mc.oracle_value_and_grad(sm, xm, p.ystar[0])[0][q]) / (2 * step)
      assert abs(fd - grad[q, d]) <= 1e-6 * max(np.max(np.abs(grad[q])), 1e-12), (q, d, fd, grad[q, d])


def test_the_cases_cover_the_edges():
  cs = mc.CASES
  assert {n for c in cs for n in c.ns} >= {1, 5, 127, 128, 129, 300} and {c.d for c in cs} == {1, 3, 17}
  assert {c.K for c in cs} == {1, 7, 64, 65, 256} and {c.S for c in cs} == {1, 3} and {c.M for c in cs} == {1, 9, 37}
  assert {c.kname for c in cs} == {'squared_exponential', 'matern32', 'matern52', 'dot_product'}
  assert {c.mname for c in cs} == {'zero', 'constant', 'linear'} and {c.dtype for c in cs} == {'fp64', 'fp32'}
  assert any(set(c.ns) == {100, 300} for c in cs) and len({c.id for c in cs}) == len(cs)


# ---- the host side of the feature --------------------------------------------------------------------------------------------------
NEW = ('hbo_acq_mes', 'hbo_mes_grad_samples', 'hbo_mes_maximize', 'hbo_probe_mes_grad_samples64')


def test_entry_points_are_exported_bound_and_documented():
  for name in NEW:
    assert name in nat.SIGNATURES, name
    f = getattr(nat.lib(), name)
    res, args = nat.SIGNATURES[name]
    assert f.restype is res and list(f.argtypes) == args, name
  blocked, mes = nat.SIGNATURES['hbo_acq_grad_samples_blocked'][1], nat.SIGNATURES['hbo_mes_grad_samples'][1]
  assert mes == blocked[:6] + [C.POINTER(C.c_double), C.c_int32] + blocked[8:]          # ystar, K in the place of acq_id, params
  blocked, mes = nat.SIGNATURES['hbo_acq_maximize_blocked'][1], nat.SIGNATURES['hbo_mes_maximize'][1]
  assert mes == blocked[:8] + [C.POINTER(C.c_double), C.c_int32] + blocked[10:]
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  hbo, tune = (open(os.path.join(root, 'include', f)).read() for f in ('hbo.h', 'hbo_tune.h'))
  for name in NEW[:3]:
    assert f'int {name}(' in hbo, name
  assert 'int hbo_probe_mes_grad_samples64(' in tune and '#define HBO_MES_MAX_K 256' in hbo and nat.MES_MAX_K == 256
  doc = hbo[:hbo.index('int hbo_mes_grad_samples(')].rsplit('/*', 1)[1]
  assert 'atomics' in doc and 'order' in doc
  for f in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
    assert 'hbo_acq_mes' in open(os.path.join(root, f)).read(), f


def test_argument_errors_come_before_any_device_call():
  err = lambda: (nat.lib().hbo_last_error(None) or b'').decode()
  pd = C.POINTER(C.c_double)
  xq, out, grad = np.zeros((1, 2)), np.full((1, 1), 7.0), np.full((1, 1, 2), 7.0)
  models, caches, nse = (nat.Model * 1)(), (C.c_void_p * 1)(), (C.c_double * 1)()
  ys = np.array([[0.5, 0.7]])
  yp = lambda a: None if a is None else a.ctypes.data_as(pd)
  lib = nat.lib()
  # hbo_acq_mes
  acq = lambda y=ys, k=2, m=models: lib.hbo_acq_mes(None, m, None, nat.ptr(xq), 1, yp(y), k, 0.0, 1.0, nat.ptr(out))
  assert acq(y=None) == nat.HBO_ERR_ARG and 'hbo_acq_mes: null argument' in err()
  assert acq(m=None) == nat.HBO_ERR_ARG and 'null argument' in err()
  for k in (0, -1, 257):
    assert acq(k=k) == nat.HBO_ERR_ARG and '1 <= K <= 256' in err()
  for v in (np.nan, np.inf, -np.inf):
    assert acq(y=np.array([[0.5, v]])) == nat.HBO_ERR_ARG and 'not finite' in err()
  assert acq() == nat.HBO_ERR_ARG and 'hbo_acq_mes: ctx is null' in err()
  # hbo_mes_grad_samples: its own checks, then those of hbo_acq_grad_samples_blocked
  gs = lambda S=1, y=ys, k=2, m=models: lib.hbo_mes_grad_samples(None, m, S, caches, nat.ptr(xq), 1, yp(y), k, nse, 1.0, nat.ptr(out), yp(grad))
  assert gs(y=None) == nat.HBO_ERR_ARG and 'hbo_mes_grad_samples: null argument' in err()
  assert gs(m=None) == nat.HBO_ERR_ARG and 'null argument' in err()
  assert gs(S=4097) == nat.HBO_ERR_ARG and '1 <= S <= 4096' in err()
  assert gs(k=0) == nat.HBO_ERR_ARG and gs(k=257) == nat.HBO_ERR_ARG and '1 <= K <= 256' in err()
  assert gs(y=np.array([[np.nan, 0.1]])) == nat.HBO_ERR_ARG and 'not finite' in err()
  assert gs() == nat.HBO_ERR_ARG and 'hbo_mes_grad_samples: ctx is null' in err()
  v64 = np.full((1, 1), 7.0)
  probe = lambda chunk, v: lib.hbo_probe_mes_grad_samples64(None, models, 1, caches, nat.ptr(xq), 1, yp(ys), 2, nse, 1.0, nat.ptr(out), yp(grad), 1, chunk, v)
  assert probe(0, None) == nat.HBO_ERR_ARG and 'val64_out is null' in err()
  assert probe(-1, yp(v64)) == nat.HBO_ERR_ARG and 'chunk_queries < 0' in err()
  # hbo_mes_maximize
  opts = nat.AcqOptOpts(**acfun.ACQ_OPT_DEFAULTS)
  ns = lib.hbo_acq_opt_state_doubles(2, opts.memory)
  state, x, val, status = np.zeros((1, ns)), np.full((1, 2), 7.0), np.full(1, 7.0), np.full(1, 7, dtype=np.int32)
  mx = lambda S=1, y=ys, k=2: lib.hbo_mes_maximize(None, models, S, caches, nat.ptr(xq), 1, None, None, yp(y), k, nse, 1.0, C.byref(opts), nat.ptr(state), 1,
                                                   nat.ptr(x), nat.ptr(val), nat.ptr(status), None)
  assert mx(y=None) == nat.HBO_ERR_ARG and 'hbo_mes_maximize: null argument' in err()
  assert mx(S=0) == nat.HBO_ERR_ARG and 'hbo_mes_maximize: 1 <= S <= 4096' in err()
  assert mx(k=300) == nat.HBO_ERR_ARG and '1 <= K <= 256' in err()
  assert mx(y=np.array([[0.1, np.inf]])) == nat.HBO_ERR_ARG and 'not finite' in err()
  assert mx() == nat.HBO_ERR_ARG and 'hbo_mes_maximize: ctx is null' in err()
  for a in (out, grad, v64, x, val):
    assert np.all(a == 7.0)                               # no output was touched
  assert np.all(status == 7) and not state.any()
  # the old entry points keep refusing a fourth acq_id
  prm = (C.c_double * 1)()
  assert lib.hbo_acq(None, models, None, nat.ptr(xq), 1, 3, 0.0, 0.0, 1.0, nat.ptr(out)) == nat.HBO_ERR_ARG and 'bad acq_id' in err()
  assert lib.hbo_acq_grad_samples_blocked(None, models, 1, caches, nat.ptr(xq), 1, 3, prm, nse, 1.0, nat.ptr(out), yp(grad)) == nat.HBO_ERR_ARG
  assert 'bad acq_id' in err()


class _Draws:
  """Stands in for pathwise.PathDraws: path k of the pool scores `pool[:, k]`, and refines to `refined[k]` from any start."""

  def __init__(self, pool, refined):
    self.pool, self.refined, self.starts = np.asarray(pool, dtype=np.float64), np.asarray(refined, dtype=np.float64), None

  def values(self, xc):
    return self.pool[:np.shape(xc)[0]]

  def maximize(self, x0, bounds=None, opts=None):
    self.starts = np.asarray(x0)
    s, r = self.starts.shape[:2]
    val = np.tile(self.refined[:, None], (1, r))
    val[:, 1:] = np.nan                                   # only the first start of a path ends with a finite value
    return self.starts.copy(), val, {}


def _stub(n, y=None, hgp=False, d=2):
  ds = {'t': defs.SubDataset(np.zeros((n, d)), np.zeros((n, 1)) if y is None else np.asarray(y, dtype=np.float64).reshape(n, 1))}
  params = defs.GPParams(model={'constant': 1.0}, samples=[{'constant': 1.0}] * 2 if hgp else None, config={})
  return (gp.HGP if hgp else gp.GP)(ds, mean.constant, kernel.matern52, params)


def test_max_value_samples_takes_pool_refinement_and_incumbent():
  xc = np.array([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]])
  pool = np.array([[0.2, 1.0, -3.0], [0.7, 0.1, -2.0], [0.4, 0.3, -2.5]])          # [M, K]
  model = _stub(3, y=[0.3, 0.65, -1.0])
  seen = {}

  def draw_paths(key_, num_samples, num_features, key):
    seen.update(k=num_samples, f=num_features, key=key)
    seen['draws'] = _Draws(pool, [0.6, 1.5, -1.9])
    return seen['draws']
  model.draw_paths = draw_paths
  ys = acfun.max_value_samples(model, 't', xc, num_maxima=3, key=5, num_features=64, starts=2)
  assert ys.dtype == np.float64 and seen['k'] == 3 and seen['f'] == 64 and seen['key'] == 5
  # path 0: pool 0.7 beats its refinement 0.6; path 1: refined 1.5; path 2: -1.9 is below the incumbent 0.65 -- the clamp
  assert np.array_equal(ys, [0.7, 1.5, 0.65])
  assert np.array_equal(ys, mc.clamp_maxima([0.7, 1.5, -1.9], model.dataset['t'].y))
  # the starts: per path the two best candidates, best first, stable
  assert seen['draws'].starts.shape == (3, 2, 2) and np.array_equal(seen['draws'].starts[0], xc[[1, 2]]) and np.array_equal(seen['draws'].starts[2], xc[[1, 2]])
  # unrefined: the pool maxima, clamped; without observations: no clamp
  assert np.array_equal(acfun.max_value_samples(model, 't', xc, num_maxima=3, key=5, refine=False), [0.7, 1.0, 0.65])
  assert seen['draws'].starts is None
  empty = _stub(0)
  empty.draw_paths = draw_paths
  assert np.array_equal(acfun.max_value_samples(empty, 't', xc, num_maxima=3, key=5, refine=False), [0.7, 1.0, -2.0])


def test_value_errors():
  xc = np.zeros((3, 2))
  for fn in (lambda m: acfun.max_value_samples(m, 't', xc, key=1), lambda m: acfun.mes(m, 't', xc, key=1),
             lambda m: acfun.mes.value_and_grad(model=m, sub_dataset_key='t', x_queries=xc, maxima=[1.0]),
             lambda m: acfun.mes.maximize(model=m, sub_dataset_key='t', x_init=xc, maxima=[1.0]),
             lambda m: acfun.mes.suggest(model=m, sub_dataset_key='t', x_candidates=xc, key=1)):
    with pytest.raises(ValueError, match='not for an HGP'):
      fn(_stub(3, hgp=True))
  model = _stub(3)
  with pytest.raises(ValueError, match='batch_size|one point'):
    acfun.mes.suggest(model=model, sub_dataset_key='t', x_candidates=xc, key=1, batch_size=2)
  for k in (0, 257):
    with pytest.raises(ValueError, match='num_maxima'):
      acfun.max_value_samples(model, 't', xc, num_maxima=k, key=1)
  with pytest.raises(ValueError, match='x_candidates'):
    acfun.max_value_samples(model, 't', np.zeros(3), key=1)
  for bad in ([], [np.nan], [np.inf, 1.0], np.zeros(257)):
    with pytest.raises(ValueError, match='maxima'):
      acfun.MaxValueEntropySearch._given(bad)
  # without observations the gradient and the maximiser refuse in Python, with the entry points' code, before any device call
  for fn in (lambda m: acfun.mes.value_and_grad(model=m, sub_dataset_key='t', x_queries=xc, maxima=[1.0]),
             lambda m: acfun.mes.maximize(model=m, sub_dataset_key='t', x_init=xc, maxima=[1.0]),
             lambda m: acfun.mes.maximize(model=m, sub_dataset_key='missing', x_init=xc, maxima=[1.0])):
    with pytest.raises(nat.HboError, match='no observations') as e:
      fn(_stub(0))
    assert e.value.code == nat.HBO_ERR_UNSUPPORTED
  assert acfun.mes.__name__ == 'mes' and acfun.max_value_entropy_search is acfun.mes
  assert acfun.mes.with_noise is False and acfun.MaxValueEntropySearch(with_noise=True).with_noise is True
  from hyperbo_amd.bo_utils import bayesopt
  assert 'not one of the native' in bayesopt._bo_on_device_unmet(model, 't', defs.SubDataset(xc, np.zeros((3, 1))), acfun.mes)
