"""GPU tier: config['lbfgs_on_device'] (hbo_train_lbfgs) against the host L-BFGS driver of infer_parameters -- the same callback
steps, the same number of evaluations between main steps (every Armijo, curvature and progress decision falls the same way), the same
losses and parameters at every main step and at the end, non-finite probes at the same positions, the host driver's behaviour on NaN,
bit-identical runs however they are cut into calls, no evaluation from Python, and hbo_train_lbfgs itself against its control code driven
from the host (hbo_probe_lbfgs_ctl) to the bit with rings of 1 and 3 pairs."""
import ctypes as C

import numpy as np
import pytest

import train_device_cases as cases

pytestmark = pytest.mark.gpu

SIZES = [128, 127, 65, 64, 17, 5]   # a full block, one short of it, both sides of 64, two small tasks
STEPS = 14                          # the ring of 10 pairs wraps

# Each bound is 10 x the largest deviation measured on the MI355X against the host driver over the cases of its class: losses
# |device - host| / |host|, parameters |device - host| / (|host| + 1e-6), at every main step and at the end (the figures are also in
# profiles/train_device.md).  The two loops take the same decisions from the same evaluation; they differ in the summation order of
# the dot products and in the last bit of the warps (ocml on the device, libm on the host), and L-BFGS carries that along.
# fp64 without an MLP (test 1 and the non-finite probes): losses 3.3e-14, parameters 1.78e-11 (both with alpha 10 through 18 non-finite
# probes; the plain 14-step runs: 3.0e-15 / 8.6e-12).  The losses are at rounding; the parameters part further along the flat
# directions of the likelihood, three orders below the 1e-8 that would want an explanation.
RTOL64 = 1.8e-10
# fp64 on an MLP basis (its weight gradient is summed with atomics, so two runs of one driver already part): losses 1.1e-15,
# parameters 2.99e-11 (SE on the (6, 33) basis, P = 330)
RTOL64_MLP = 3e-10
# fp32: losses 2.2e-7 (SE + constant), 4.1e-7 (Matern 5/2 on the MLP basis); parameters 5.8e-4, 1.16e-3
RTOL32_LOSS = 4.1e-6
RTOL32_PARAM = 1.2e-2


def _mods():
  from hyperbo_amd import _native as nat
  from hyperbo_amd.basics import definitions as defs, lbfgs
  from hyperbo_amd.gp_utils import gp, objectives, utils
  return nat, defs, lbfgs, gp, objectives, utils


class Result:
  """One training run: log [(step, loss, flat params, evaluations made so far)], the final flat params, the value of every
  evaluation in order, the DeviceDataset.evaluate calls Python made and (device) the status."""


def _run(kname, mname, data, on_device, monkeypatch, steps=STEPS, alpha=None, dtype=np.float64, warp=None, model=None, key=7):
  nat, defs, lbfgs, gp, objectives, utils = _mods()
  mean_func, cov_func = cases.funcs(kname, mname)
  config = {'method': 'lbfgs', 'batch_size': 129, 'max_training_step': steps, 'objective': objectives.nll}
  if alpha is not None:
    config['alpha'] = alpha
  if on_device:
    config['lbfgs_on_device'] = True
    config['lbfgs_eval_log'] = {}
  m = model if model is not None else cases.model_of(kname, mname, dtype=dtype)
  m = {k: (dict(v) if isinstance(v, dict) else v) for k, v in m.items()}
  g = gp.GP(data, mean_func, cov_func, defs.GPParams(model=m, config=config), warp if warp is not None else utils.DEFAULT_WARP_FUNC)
  r = Result()
  r.log, r.values = [], []
  orig = objectives.DeviceDataset.evaluate

  def counting(self, *a, **k):
    out = orig(self, *a, **k)
    r.values.append(out[0] / self.num_tasks)
    return out
  monkeypatch.setattr(objectives.DeviceDataset, 'evaluate', counting)
  try:
    g.train(key=key, callback=lambda step, model_params, loss: r.log.append((step, loss, lbfgs.tree_flatten(model_params)[0], len(r.values))))
  finally:
    monkeypatch.setattr(objectives.DeviceDataset, 'evaluate', orig)
  r.final = lbfgs.tree_flatten(g.params.model)[0]
  r.python_evaluations = len(r.values)
  r.status = None
  if on_device:
    r.evals = config['lbfgs_eval_log']['evals']
    r.status = config['lbfgs_eval_log']['status']
    r.values = [v for _, _, _, v in r.evals]
    # evaluations made up to and including each recorded step, as the host's callback sees them
    recorded = [j + 1 for j, (kind, _, _, _) in enumerate(r.evals) if kind in (nat.LBFGS_START, nat.LBFGS_MAIN)]
    if r.status == nat.LBFGS_CONVERGED:
      recorded = recorded[:-1]
    assert len(recorded) == len(r.log)
    r.log = [(s, l, x, n) for (s, l, x, _), n in zip(r.log, recorded)]
  return r


def _deviation(host, dev):
  """(largest relative loss deviation, largest parameter deviation) after checking that both runs took the same path."""
  assert [s for s, *_ in dev.log] == [s for s, *_ in host.log]
  assert [n for *_, n in dev.log] == [n for *_, n in host.log], 'a line search took another number of probes'
  assert len(dev.values) == len(host.values)
  hl, dl = np.array([l for _, l, _, _ in host.log]), np.array([l for _, l, _, _ in dev.log])
  hx, dx = np.array([x for _, _, x, _ in host.log] + [host.final]), np.array([x for _, _, x, _ in dev.log] + [dev.final])
  assert np.array_equal(np.isfinite(hl), np.isfinite(dl))
  fin = np.isfinite(hl)
  loss = float(np.max(np.abs(dl[fin] - hl[fin]) / np.abs(hl[fin]))) if fin.any() else 0.0
  param = float(np.max(np.abs(dx - hx) / (np.abs(hx) + 1e-6)))
  return loss, param


def _compare(host, dev, rtol_loss, rtol_param, what):
  loss, param = _deviation(host, dev)
  print(f'{what}: {len(host.log)} main steps, {len(host.values)} evaluations, status {dev.status}; deviation loss {loss:.3g} param {param:.3g}')
  assert loss <= rtol_loss and param <= rtol_param, (loss, param)


FP64_CASES = [
    ('squared_exponential', 'constant', cases.D, cases.FEATS, STEPS, None),
    ('matern32', 'linear', cases.D, cases.FEATS, STEPS, None),
    ('squared_exponential_kumar', 'constant', cases.D, cases.FEATS, STEPS, None),
    ('matern52_mlp', 'linear_mlp', cases.D, cases.FEATS, STEPS, None),
    ('squared_exponential_mlp', 'linear_mlp', cases.D, (6, 33), STEPS, None),   # P = 330
    ('matern52', 'linear', 33, cases.FEATS, STEPS, None),
    ('dot_product', 'zero', cases.D, cases.FEATS, 10, None),
    ('squared_exponential', 'constant', cases.D, cases.FEATS, STEPS, 0.02),     # growing probes
    ('squared_exponential', 'constant', cases.D, cases.FEATS, STEPS, 50.0),     # shrinking probes
]


@pytest.mark.parametrize('kname,mname,d,feats,steps,alpha', [pytest.param(*c, id=f'{c[0]}-{c[1]}-d{c[2]}-f{c[3][-1]}-a{c[5]}') for c in FP64_CASES])
def test_device_lbfgs_matches_host_driver_fp64(gpu_ctx, monkeypatch, kname, mname, d, feats, steps, alpha):
  data = cases.dataset(SIZES, d=d)
  model = cases.model_of(kname, mname, d=d, feats=feats)
  host = _run(kname, mname, data, False, monkeypatch, steps=steps, alpha=alpha, model=model)
  dev = _run(kname, mname, data, True, monkeypatch, steps=steps, alpha=alpha, model=model)
  assert len(host.log) >= 2
  mlp = kname.endswith('_mlp') or mname == 'linear_mlp'
  rtol = RTOL64_MLP if mlp else RTOL64
  _compare(host, dev, rtol, rtol, f'fp64 {kname}+{mname} d{d} f{feats[-1]} alpha {alpha}')


@pytest.mark.parametrize('kname,mname', [('squared_exponential', 'constant'), ('matern52_mlp', 'linear_mlp')])
def test_device_lbfgs_matches_host_driver_fp32(gpu_ctx, monkeypatch, kname, mname):
  data = cases.dataset(SIZES, dtype=np.float32)
  host = _run(kname, mname, data, False, monkeypatch, dtype=np.float32)
  dev = _run(kname, mname, data, True, monkeypatch, dtype=np.float32)
  assert len(host.log) >= 2
  _compare(host, dev, RTOL32_LOSS, RTOL32_PARAM, f'fp32 {kname}+{mname}')


@pytest.mark.parametrize('alpha', [1.0, 10.0])
def test_device_lbfgs_non_finite_probes_fall_where_the_hosts_do(gpu_ctx, monkeypatch, alpha):
  nat, defs, lbfgs, gp, objectives, utils = _mods()
  # an identity-warped noise variance: long probes drive it below zero and the Gram matrix stops being positive definite
  warp = dict(utils.DEFAULT_WARP_FUNC, noise_variance=utils.identity_warp)
  data = cases.dataset(SIZES)
  model = cases.model_of('squared_exponential', 'constant')
  model['noise_variance'] = np.array(0.3)
  model['lengthscale'] = np.full(cases.D, -1.0)
  host = _run('squared_exponential', 'constant', data, False, monkeypatch, steps=12, alpha=alpha, warp=warp, model=model)
  dev = _run('squared_exponential', 'constant', data, True, monkeypatch, steps=12, alpha=alpha, warp=warp, model=model)
  bad = [i for i, v in enumerate(host.values) if not np.isfinite(v)]
  print(f'alpha {alpha}: {len(bad)} non-finite evaluations of {len(host.values)}')
  assert bad, 'the host driver saw no non-finite evaluation: the case tests nothing'
  assert [i for i, v in enumerate(dev.values) if not np.isfinite(v)] == bad
  _compare(host, dev, RTOL64, RTOL64, f'non-finite probes, alpha {alpha}')


def test_device_lbfgs_nan_at_the_start_returns_the_initial_parameters(gpu_ctx, monkeypatch):
  nat, defs, lbfgs, gp, objectives, utils = _mods()
  data = cases.dataset(SIZES)
  x = data[2].x.copy(); x[3, 1] = np.nan
  data[2] = type(data[2])(x, data[2].y)
  start = lbfgs.tree_flatten(cases.model_of('squared_exponential', 'constant'))[0]
  host = _run('squared_exponential', 'constant', data, False, monkeypatch)
  dev = _run('squared_exponential', 'constant', data, True, monkeypatch)
  for r in (host, dev):
    assert np.array_equal(r.final, start)
    assert [s for s, *_ in r.log] == [0] and np.isnan(r.log[0][1])
    assert len(r.values) == 1 + 50 and all(np.isnan(v) for v in r.values)
  assert [k for k, *_ in dev.evals] == [nat.LBFGS_START] + [nat.LBFGS_LINE_SEARCH] * 50
  assert dev.status == nat.LBFGS_NO_PROGRESS


def _bits(r):
  return ([(k, i) for k, i, _, _ in r.evals], np.array([[a, v] for _, _, a, v in r.evals]), np.array([x for _, _, x, _ in r.log]), r.final)


def test_device_lbfgs_segments_do_not_change_a_bit(gpu_ctx, monkeypatch):
  nat, defs, lbfgs, gp, objectives, utils = _mods()
  data = cases.dataset(SIZES)
  runs = []
  for seg in (7, 1000, 1000):
    monkeypatch.setattr(gp, 'LBFGS_SEGMENT', seg)
    runs.append(_bits(_run('squared_exponential', 'constant', data, True, monkeypatch)))
  assert len(runs[0][0]) > 2 * 7   # the short segments cut the run more than once
  for other in runs[1:]:
    assert other[0] == runs[0][0]
    for a, b in zip(other[1:], runs[0][1:]):
      assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize('memory', [1, 3])
def test_device_loop_is_the_host_driven_hook_to_the_bit_with_a_short_ring(gpu_ctx, memory):
  """hbo_train_lbfgs called directly, SE + constant on SIZES, memory 1 (every pair overwrites the only slot) and 3: one call of 32
  evaluations against a host loop that makes them one call each and hands the value and the chained gradient the device left in
  the state to the one-thread hook.  Log entries, next points and the whole state agree to the bit after every evaluation."""
  from hyperbo_amd import _model
  nat, defs, lbfgs, gp, objectives, utils = _mods()
  mean_func, cov_func = cases.funcs('squared_exponential', 'constant')
  template = cases.model_of('squared_exponential', 'constant')
  x0, unflatten = lbfgs.tree_flatten(template)
  P, evals = x0.size, 32
  opts = nat.LbfgsOpts(memory=memory, ls_steps=50, max_iters=STEPS, alpha=1.0, tol=1e-6, c1=1e-4, c2=0.9, grow=2.1, tau=0.5)
  ns = nat.lib().hbo_lbfgs_state_doubles(P, memory)
  full = objectives.DeviceDataset(cases.dataset(SIZES))

  def call(point, x, state, k):
    bm = _model.BuiltModel(mean_func, cov_func, defs.GPParams(model=unflatten(point), config={}), utils.DEFAULT_WARP_FUNC, full.dtype, full.input_dim)
    leaves, n = _model.train_leaf_map(bm, template)
    assert n == P
    log, x_next, done, st = (nat.LbfgsEval * k)(), np.empty(P), C.c_int32(0), C.c_int32(0)
    full.ctx.check(nat.lib().hbo_train_lbfgs(full.ctx.handle, bm.ref(), full._h, leaves, P, C.byref(opts), nat.ptr(x), nat.ptr(state), k, log,
                                             None, nat.ptr(x_next), C.byref(done), C.byref(st)), allow_not_pd=False)
    return log, x_next, done.value, st.value
  try:
    x_one, state_one = x0.copy(), np.zeros(ns)
    log_one, next_one, done_one, status_one = call(x0, x_one, state_one, evals)
    x_dev, state_dev, state_hook, point = x0.copy(), np.zeros(ns), np.zeros(ns), x0.copy()
    x_next, x_iter, ev, st = np.empty(P), np.empty(P), nat.LbfgsEval(), C.c_int32(0)
    made, mains = 0, 0
    for e in range(evals):
      log, point, done, status = call(point, x_dev, state_dev, 1)
      assert done == 1
      grad = state_dev[16 + 5 * P:16 + 6 * P].copy()                       # hbo_lbfgs_view.g: the gradient of the point just evaluated
      rc = nat.lib().hbo_probe_lbfgs_ctl(nat.ptr(state_hook), P, C.byref(opts), nat.ptr(x0) if e == 0 else None, float(log[0].value), nat.ptr(grad),
                                         nat.ptr(x_next), nat.ptr(x_iter), C.byref(ev), C.byref(st))
      assert rc == nat.HBO_OK, (nat.lib().hbo_last_error(None) or b'').decode()
      assert bytes(ev) == bytes(log[0]) == bytes(log_one[e]), e
      assert state_hook.tobytes() == state_dev.tobytes() and x_next.tobytes() == point.tobytes() and x_iter.tobytes() == x_dev.tobytes(), e
      assert st.value == status
      made += 1
      mains = max(mains, ev.iter if ev.kind == nat.LBFGS_MAIN else 0)
      if status != nat.LBFGS_RUNNING:
        break
    assert mains >= 5                                                      # pairs 1 .. 4 at least: a ring of 3 has wrapped and been used
    assert done_one == made and status_one == status and state_one.tobytes() == state_hook.tobytes()
    assert next_one.tobytes() == point.tobytes() and x_one.tobytes() == x_dev.tobytes()
  finally:
    full.close()


def test_device_lbfgs_evaluates_nothing_from_python(gpu_ctx, monkeypatch):
  data = cases.dataset(SIZES)
  dev = _run('squared_exponential', 'constant', data, True, monkeypatch)
  assert dev.python_evaluations == 0 and len(dev.evals) > STEPS
  host = _run('squared_exponential', 'constant', data, False, monkeypatch)
  assert host.python_evaluations == len(dev.evals)   # the host driver: one DeviceDataset.evaluate per evaluation


def test_device_lbfgs_refuses_the_blocked_regime(gpu_ctx, monkeypatch):
  nat, defs, lbfgs, gp, objectives, utils = _mods()
  ctx = nat.default_context()
  data = cases.dataset(SIZES)
  ctx.set_option('small_fused', 0)
  try:
    with pytest.raises(ValueError, match='small_fused'):
      _run('squared_exponential', 'constant', data, True, monkeypatch, steps=3)
  finally:
    ctx.set_option('small_fused', 1)
