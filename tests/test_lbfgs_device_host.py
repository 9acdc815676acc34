"""config['lbfgs_on_device'] (hbo_train_lbfgs), the parts that need no device: the L-BFGS control code (csrc/lbfgs_ctl.h) driven
through its host hook hbo_probe_lbfgs_ctl against lbfgs.lbfgs on analytic functions, its state across copies, the argument checks
hbo_train_lbfgs makes before any HIP call, the eligibility rules and the untouched host branch."""
import ctypes as C

import numpy as np
import pytest

import train_device_cases as cases

# Hook and host driver take the same decisions from the same numbers; they differ only in how a dot product is summed: 256 strided
# partial sums and a tree without fused multiply-adds against BLAS ddot (test_hook_is_the_host_driver_bit_for_bit_with_its_own_dots
# removes that difference and gets identical bits).  Largest deviation of any evaluated point or value over the cases below,
# |hook - host| / (|host| + 1), measured on the CPU tier's machine: 1.57e-8, on Rosenbrock from (-1.2, 1) with alpha 1 -- the curved
# valley carries a last-bit difference of step 5 (8.6e-16) up by a factor of about two per main step over 25 steps; every other case
# stays below 1e-14, the P = 300 quadratic at 2.4e-15.  The bound is 10 x the largest measurement.
HOOK_RTOL = 1.6e-7


def _mods():
  from hyperbo_amd import _native as nat
  from hyperbo_amd.basics import definitions as defs, lbfgs
  from hyperbo_amd.gp_utils import gp, objectives, utils
  return nat, defs, lbfgs, gp, objectives, utils


def _opts(nat, **kw):
  d = dict(memory=10, ls_steps=50, max_iters=100, alpha=1.0, tol=1e-6, c1=1e-4, c2=0.9, grow=2.1, tau=0.5)
  d.update(kw)
  return nat.LbfgsOpts(**d)


def rosenbrock(x):
  a, b = x[0], x[1]
  return (1 - a)**2 + 100 * (b - a * a)**2, np.array([-2 * (1 - a) - 400 * a * (b - a * a), 200 * (b - a * a)])


QUAD_LAM = np.linspace(1.0, 40.0, 300)


def quadratic(x):
  return 0.5 * float(np.sum(QUAD_LAM * x * x)), QUAD_LAM * x


def nan_everywhere(x):
  return float('nan'), np.full(x.size, np.nan)


BALL_C, BALL_LAM = np.array([0.9, 0.2]), np.array([1.0, 3.0])


def ball(x):
  """An anisotropic bowl, infinite outside the unit ball."""
  if float(x @ x) >= 1.0:
    return float('inf'), np.full(x.size, np.nan)
  return float(np.sum(BALL_LAM * (x - BALL_C)**2)), 2 * BALL_LAM * (x - BALL_C)


def run_hook(f, x0, copy_every=0, **kw):
  """The hook driven like the device loop: [(kind, iter, alpha, point, value)], the iterate, the status."""
  nat, *_ = _mods()
  o = _opts(nat, **kw)
  P = x0.size
  state = np.zeros(nat.lib().hbo_lbfgs_state_doubles(P, o.memory))
  point, x_next, x_iter = x0.astype(np.float64).copy(), np.zeros(P), np.zeros(P)
  ev, status = nat.LbfgsEval(), C.c_int32(0)
  out = []
  for n in range(100000):
    if copy_every and n % copy_every == 0:
      state = state.copy()
    v, g = f(point)
    g = np.ascontiguousarray(g, dtype=np.float64)
    rc = nat.lib().hbo_probe_lbfgs_ctl(nat.ptr(state), P, C.byref(o), nat.ptr(point) if n == 0 else None, float(v), nat.ptr(g),
                                       nat.ptr(x_next), nat.ptr(x_iter), C.byref(ev), C.byref(status))
    assert rc == nat.HBO_OK, (nat.lib().hbo_last_error(None) or b'').decode()
    out.append((ev.kind, ev.iter, ev.alpha, point.copy(), ev.value))
    if status.value != nat.LBFGS_RUNNING:
      return out, x_iter.copy(), status.value
    point = x_next.copy()
  raise AssertionError('the hook never stopped')


def run_host(f, x0, monkeypatch, **kw):
  """lbfgs.lbfgs on the same function: the same list (alpha left out), the returned parameters, the callback steps."""
  nat, defs, lbfgs, *_ = _mods()
  o = dict(memory=10, ls_steps=50, steps=kw.pop('max_iters', 100), alpha=1.0, tol=1e-6)
  o.update(kw)
  out, steps, in_search = [], [], [False]
  orig = lbfgs.backtracking_linesearch

  def searching(*a, **k):
    in_search[0] = True
    try:
      return orig(*a, **k)
    finally:
      in_search[0] = False
  monkeypatch.setattr(lbfgs, 'backtracking_linesearch', searching)
  main = [0]

  def vg(p):
    v, g = f(p['x'])
    if in_search[0]:
      kind, it = nat.LBFGS_LINE_SEARCH, main[0]
    elif not out:
      kind, it = nat.LBFGS_START, 0
    else:
      main[0] += 1
      kind, it = nat.LBFGS_MAIN, main[0]
    out.append((kind, it, None, p['x'].copy(), v))
    return v, {'x': g}
  _, params, _ = lbfgs.lbfgs(None, {'x': x0.astype(np.float64)}, val_and_grad_fn=vg, callback=lambda step, model_params, loss: steps.append(step), **o)
  monkeypatch.setattr(lbfgs, 'backtracking_linesearch', orig)
  return out, params['x'], steps


def deviation(got, want):
  """max |got - want| / (|want| + 1) over the points and values of two evaluation lists (non-finite entries must coincide)."""
  worst = 0.0
  for (_, _, _, xp, v), (_, _, _, xh, vh) in zip(got, want):
    a, b = np.append(xp, v), np.append(xh, vh)
    fin = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), fin)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)])
    if fin.any():
      worst = max(worst, float(np.max(np.abs(a[fin] - b[fin]) / (np.abs(b[fin]) + 1))))
  return worst


def compare(f, x0, monkeypatch, **kw):
  hook, x_hook, status = run_hook(f, x0, **kw)
  host, x_host, steps = run_host(f, x0, monkeypatch, **kw)
  assert [(k, i) for k, i, *_ in hook] == [(k, i) for k, i, *_ in host]
  dev = deviation(hook, host)
  end = float(np.max(np.abs(x_hook - x_host) / (np.abs(x_host) + 1)))
  print(f'hook vs host: {len(hook)} evaluations, status {status}, deviation {dev:.3g}, final {end:.3g}')
  assert dev <= HOOK_RTOL and end <= HOOK_RTOL
  return hook, x_hook, status, steps


ROSEN_X0 = np.array([-1.2, 1.0])


def test_hook_rosenbrock(monkeypatch):
  nat, *_ = _mods()
  hook, x, status, steps = compare(rosenbrock, ROSEN_X0, monkeypatch, max_iters=25, tol=1e-14)
  assert steps[:3] == [0, 1, 2] and status in (nat.LBFGS_STEPS_DONE, nat.LBFGS_CONVERGED, nat.LBFGS_NO_PROGRESS, nat.LBFGS_INSTABILITY)
  assert status == nat.LBFGS_STEPS_DONE and rosenbrock(x)[0] < 1e-2 * rosenbrock(ROSEN_X0)[0]


def test_hook_rosenbrock_growing_probes(monkeypatch):
  hook, *_ = compare(rosenbrock, ROSEN_X0, monkeypatch, max_iters=25, tol=1e-14, alpha=0.02)
  grew = [b[2] / a[2] for a, b in zip(hook, hook[1:]) if a[0] == b[0] == 2 and a[1] == b[1]]
  assert any(abs(r - 2.1) < 1e-12 for r in grew), 'no probe took the x 2.1 branch'


def test_hook_quadratic_spans_partial_sums_and_wraps_the_ring(monkeypatch):
  nat, *_ = _mods()
  x0 = np.cos(np.arange(300.0)) + 1.5
  hook, x, status, steps = compare(quadratic, x0, monkeypatch, max_iters=25, tol=1e-30)
  assert max(steps) > 10 and status == nat.LBFGS_STEPS_DONE   # more main steps than the ring holds pairs
  assert quadratic(x)[0] < 1e-6 * quadratic(x0)[0]


def test_hook_nan_everywhere_makes_no_progress(monkeypatch):
  nat, *_ = _mods()
  hook, x, status, steps = compare(nan_everywhere, ROSEN_X0, monkeypatch, max_iters=5)
  assert len(hook) == 1 + 50 and status == nat.LBFGS_NO_PROGRESS and steps == [0]
  assert np.array_equal(x, ROSEN_X0)


def test_hook_shrinks_through_non_finite_probes(monkeypatch):
  hook, x, status, steps = compare(ball, np.array([-0.5, 0.0]), monkeypatch, max_iters=12, alpha=5.0, tol=1e-20)
  assert any(k == 2 and not np.isfinite(v) for k, _, _, _, v in hook), 'no probe left the ball'
  assert np.isfinite(ball(x)[0]) and ball(x)[0] < 1e-3


def test_hook_exhausted_search_at_the_start(monkeypatch):
  nat, *_ = _mods()
  hook, x, status, steps = compare(rosenbrock, ROSEN_X0, monkeypatch, max_iters=25, tol=1e-14, ls_steps=2)
  # both probes fail Armijo with finite values: the search runs out and returns (last value, alpha halved once more); lbfgs() finds the
  # value above the start's and stops where it started
  assert [k for k, *_ in hook] == [0, 2, 2] and all(np.isfinite(v) for *_, v in hook) and hook[2][4] >= hook[0][4]
  assert status == nat.LBFGS_NO_PROGRESS and np.array_equal(x, ROSEN_X0)


def test_hook_exhausted_search_moves_by_the_unevaluated_step(monkeypatch):
  hook, *_ = compare(rosenbrock, np.array([2.0, 2.0]), monkeypatch, max_iters=25, tol=1e-14, ls_steps=2, alpha=0.02)
  # a search that ran out of probes moves by the alpha already modified after its last probe: the next main evaluation is then at a
  # point no probe evaluated, further along d by that factor
  quirk = [i for i in range(2, len(hook)) if hook[i][0] == 1 and hook[i - 1][0] == 2 and hook[i - 2][0] == 2 and hook[i - 2][1] == hook[i - 1][1]
           and not np.array_equal(hook[i][3], hook[i - 1][3])]
  assert quirk, 'no exhausted search in this run'
  i = quirk[0]
  x_it, probe, moved = hook[i - 3][3], hook[i - 1][3], hook[i][3]   # the main evaluation before the search is at the iterate
  assert hook[i - 3][0] == 1
  np.testing.assert_allclose(moved - x_it, 2.1 * (probe - x_it), rtol=1e-9)


def fixed_order_dot(a, b):
  """csrc/lbfgs_ctl.h: hbo_lbfgs_dot in NumPy."""
  prod = np.zeros(-(-a.size // 256) * 256)
  prod[:a.size] = np.asarray(a, dtype=np.float64).ravel() * np.asarray(b, dtype=np.float64).ravel()
  acc = np.zeros(256)
  for row in prod.reshape(-1, 256):
    acc = acc + row
  s = 128
  while s:
    acc[:s] = acc[:s] + acc[s:2 * s]
    s //= 2
  return acc[0]


@pytest.mark.parametrize('f,x0,kw', [(rosenbrock, ROSEN_X0, dict(max_iters=25, tol=1e-14)),
                                     (rosenbrock, ROSEN_X0, dict(max_iters=25, tol=1e-14, alpha=0.02)),
                                     (rosenbrock, np.array([2.0, 2.0]), dict(max_iters=25, tol=1e-14, ls_steps=2, alpha=0.02)),
                                     (quadratic, np.cos(np.arange(300.0)) + 1.5, dict(max_iters=25, tol=1e-30)),
                                     (ball, np.array([-0.5, 0.0]), dict(max_iters=12, alpha=5.0, tol=1e-20))],
                         ids=['rosenbrock', 'rosenbrock-grow', 'rosenbrock-exhausted', 'quadratic', 'ball'])
def test_hook_is_the_host_driver_bit_for_bit_with_its_own_dots(monkeypatch, f, x0, kw):
  nat, defs, lbfgs, *_ = _mods()
  hook, x_hook, _ = run_hook(f, x0, **kw)
  monkeypatch.setattr(lbfgs.np, 'vdot', fixed_order_dot)
  host, x_host, _ = run_host(f, x0, monkeypatch, **kw)
  monkeypatch.undo()
  _same([(k, i, 0.0, x, v) for k, i, _, x, v in hook], [(k, i, 0.0, x, v) for k, i, _, x, v in host])
  assert np.array_equal(x_hook, x_host)


@pytest.mark.parametrize('memory', [1, 3])
def test_hook_is_the_host_driver_bit_for_bit_with_a_short_ring(monkeypatch, memory):
  """memory 1 (every pair overwrites the only slot) and 3: the ring wraps from the second / fourth main step on (the P = 300 quadratic)."""
  nat, defs, lbfgs, *_ = _mods()
  f, x0, kw = quadratic, np.cos(np.arange(300.0)) + 1.5, dict(max_iters=25, tol=1e-30, memory=memory)
  hook, x_hook, _ = run_hook(f, x0, **kw)
  monkeypatch.setattr(lbfgs.np, 'vdot', fixed_order_dot)
  host, x_host, _ = run_host(f, x0, monkeypatch, **kw)
  monkeypatch.undo()
  assert max(i for k, i, *_ in hook if k == nat.LBFGS_MAIN) >= 8
  _same([(k, i, 0.0, x, v) for k, i, _, x, v in hook], [(k, i, 0.0, x, v) for k, i, _, x, v in host])
  assert np.array_equal(x_hook, x_host)


def test_hook_converged_at_start(monkeypatch):
  nat, *_ = _mods()
  hook, x, status, steps = compare(rosenbrock, np.array([1.0, 1.0]), monkeypatch)
  assert len(hook) == 1 and status == nat.LBFGS_CONVERGED_AT_START and steps == [0]


def test_hook_one_iteration(monkeypatch):
  nat, *_ = _mods()
  hook, x, status, steps = compare(rosenbrock, ROSEN_X0, monkeypatch, max_iters=1, tol=1e-14)
  assert status == nat.LBFGS_STEPS_DONE and steps == [0, 1]


def _same(a, b):
  assert len(a) == len(b)
  for (k, i, al, x, v), (k2, i2, al2, x2, v2) in zip(a, b):
    assert (k, i) == (k2, i2)
    assert np.array_equal(np.array([al, v]), np.array([al2, v2]), equal_nan=True) and np.array_equal(x, x2, equal_nan=True)


@pytest.mark.parametrize('f,x0,kw', [(rosenbrock, ROSEN_X0, dict(max_iters=25, tol=1e-14)),
                                     (quadratic, np.cos(np.arange(300.0)) + 1.5, dict(max_iters=14, tol=1e-30)),
                                     (nan_everywhere, ROSEN_X0, dict(max_iters=3))], ids=['rosenbrock', 'quadratic', 'nan'])
def test_state_survives_a_round_trip(f, x0, kw):
  base = run_hook(f, x0, **kw)
  for every in (1, 7):
    other = run_hook(f, x0, copy_every=every, **kw)
    _same(base[0], other[0])
    assert np.array_equal(base[1], other[1]) and base[2] == other[2]


def _lbfgs_args(nat, P=3, evals=2):
  leaves = (nat.TrainLeaf * P)()
  for i in range(P):
    leaves[i].target = nat.TRAIN_NONE
  o = _opts(nat)
  return dict(leaves=leaves, P=P, opts=o, x=np.zeros(P), state=np.zeros(nat.lib().hbo_lbfgs_state_doubles(P, o.memory)), evals=evals,
              log=(nat.LbfgsEval * evals)())


def _call(nat, model, a, ds=None, drop=()):
  done, status = C.c_int32(0), C.c_int32(0)
  arg = lambda name, v: None if name in drop else v
  return nat.lib().hbo_train_lbfgs(None, C.byref(model) if model is not None else None, ds, a['leaves'], a['P'],
                                   arg('opts', C.byref(a['opts'])), nat.ptr(a['x']), arg('state', nat.ptr(a['state'])), a['evals'],
                                   arg('log', a['log']), None, None, arg('evals_done', C.byref(done)), arg('status', C.byref(status)))


def test_train_lbfgs_rejects_bad_arguments_before_any_device_call():
  from hyperbo_amd import _model
  nat, defs, lbfgs, gp, objectives, utils = _mods()
  mean_func, cov_func = cases.funcs('squared_exponential', 'constant')
  params = defs.GPParams(model=cases.model_of('squared_exponential', 'constant'), config={})
  m = _model.BuiltModel(mean_func, cov_func, params, utils.DEFAULT_WARP_FUNC, np.float64, cases.D).struct
  err = lambda: (nat.lib().hbo_last_error(None) or b'').decode()

  def expect(rc, text):
    assert rc == nat.HBO_ERR_ARG, (rc, err())
    assert text in err(), err()

  expect(_call(nat, None, _lbfgs_args(nat)), 'model is null')
  a = _lbfgs_args(nat); a['P'] = 0
  expect(_call(nat, m, a), 'P must be positive')
  a = _lbfgs_args(nat); a['evals'] = 0
  expect(_call(nat, m, a), 'evals must be positive')
  for name in ('state', 'log', 'evals_done', 'status'):
    expect(_call(nat, m, _lbfgs_args(nat), drop=(name,)), 'null array argument')
  expect(_call(nat, m, _lbfgs_args(nat), drop=('opts',)), 'opts is null')
  for field, val, text in (('memory', 0, 'memory'), ('ls_steps', 0, 'ls_steps'), ('max_iters', 0, 'max_iters'), ('alpha', float('nan'), 'numbers'),
                           ('tol', float('nan'), 'numbers'), ('tau', float('nan'), 'numbers')):
    a = _lbfgs_args(nat)
    setattr(a['opts'], field, val)
    expect(_call(nat, m, a), text)
  a = _lbfgs_args(nat); a['state'][0] = 7.0
  expect(_call(nat, m, a), 'state is neither')
  for field, val, text in (('warp', 7, 'unknown warp'), ('target', 40, 'unknown target'), ('round_f32', 2, 'round_f32'),
                           ('index', 9, 'outside its target')):
    a = _lbfgs_args(nat)
    if field == 'index':
      a['leaves'][0].target = nat.TRAIN_LENGTHSCALE
    setattr(a['leaves'][0], field, val)
    expect(_call(nat, m, a), text)
  a = _lbfgs_args(nat)
  a['leaves'][1].target = nat.TRAIN_DOT_PROD_SIGMA   # an SE model has no dot-product sigma
  expect(_call(nat, m, a), 'does not read its target')
  # every leaf valid: the next thing missing is the dataset
  a = _lbfgs_args(nat)
  a['leaves'][0].target = nat.TRAIN_NOISE_VARIANCE
  a['leaves'][0].warp = nat.TRAIN_WARP_SOFTPLUS_EPS
  expect(_call(nat, m, a), 'dataset is null')
  assert nat.lib().hbo_lbfgs_state_doubles(0, 10) == 0 and nat.lib().hbo_lbfgs_state_doubles(3, 0) == 0
  assert nat.lib().hbo_lbfgs_state_doubles(3, 10) >= 5 * 3 + 2 * 10 * 3


def _gp(sizes=(60, 80), warp=None, **config):
  nat, defs, lbfgs, gp, objectives, utils = _mods()
  mean_func, cov_func = cases.funcs('squared_exponential', 'constant')
  cfg = {'method': 'lbfgs', 'batch_size': 100, 'max_training_step': 5, 'objective': objectives.nll}
  cfg.update(config)
  w = dict(utils.DEFAULT_WARP_FUNC)
  w.update(warp or {})
  return gp.GP(cases.dataset(list(sizes)), mean_func, cov_func, defs.GPParams(model=cases.model_of('squared_exponential', 'constant'), config=cfg), w)


@pytest.mark.parametrize('case,match', [
    ({'objective': 'ekl'}, 'not obj.nll'),
    ({'priors': {}}, 'priors'),
    ({'warp': {'noise_variance': np.exp}}, 'closed set'),
    ({'comm': object()}, 'comm'),
    ({'sizes': [60, 129], 'batch_size': 200}, '> 128'),
    ({'sizes': [60, 400], 'batch_size': 200}, '> 128'),
])
def test_ineligible_configurations_raise(case, match):
  nat, defs, lbfgs, gp, objectives, utils = _mods()
  g = _gp(lbfgs_on_device=True, **case)
  if isinstance(g.params.config['objective'], str):
    g.params.config['objective'] = getattr(objectives, g.params.config['objective'])
  with pytest.raises(ValueError, match='lbfgs_on_device: .*' + match):
    g.train(key=0)


@pytest.mark.parametrize('config', [{}, {'lbfgs_on_device': False}])
def test_host_branch_unchanged_without_the_key(monkeypatch, config):
  nat, defs, lbfgs, gp, objectives, utils = _mods()
  calls = []

  def spy(fn, params, **kw):
    calls.append(kw)
    return 0.0, params, None
  monkeypatch.setattr(lbfgs, 'lbfgs', spy)
  monkeypatch.setattr(gp, '_infer_lbfgs_on_device', lambda *a, **k: pytest.fail('the device loop ran without its key'))
  g = _gp(alpha=0.5, **config)
  before = g.params.model
  g.train(key=0)
  assert len(calls) == 1 and g.params.model is before
  assert calls[0]['steps'] == 5 and calls[0]['alpha'] == 0.5 and callable(calls[0]['val_and_grad_fn']) and calls[0]['callback'] is None
  assert set(calls[0]) == {'steps', 'alpha', 'val_and_grad_fn', 'callback'}


def test_the_key_enters_the_device_loop(monkeypatch):
  nat, defs, lbfgs, gp, objectives, utils = _mods()
  monkeypatch.setattr(lbfgs, 'lbfgs', lambda *a, **k: pytest.fail('the host driver ran'))
  seen = []
  monkeypatch.setattr(gp, '_infer_lbfgs_on_device', lambda *a: seen.append(a) or a[2])
  g = _gp(lbfgs_on_device=True)
  g.train(key=0)
  assert len(seen) == 1
