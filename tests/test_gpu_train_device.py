"""GPU tier: config['adam_on_device'] (hbo_train_adam) against the host Adam driver of infer_parameters -- the same per-step losses
(through `callback`), the same parameters at every step and at the end, the same batches for the same key, the host driver's rules
for non-finite losses, and no per-step evaluation from Python."""
import numpy as np
import pytest

import train_device_cases as cases

pytestmark = pytest.mark.gpu

RTOL64 = 1e-10
# with an MLP basis the evaluation itself is not bit-reproducible: the weight gradient of a dense layer is summed with atomics
# (mlp.hip: dense_bwd_w_kernel), so two host-driver runs already part in the last bits and Adam carries that along.  Measured on
# the MI355X over 200 steps, device vs host: 3.7e-10 relative (1.1e-11 absolute) on parameters near 0.03.
RTOL64_MLP = 1e-8
# fp32: 10 x the largest deviation measured on the MI355X over these 200-step runs.  Losses, relative: 1.9e-7 (SE + constant),
# 1.1e-7 (Matern 5/2 on the MLP basis + linear_mlp).  Parameters at every step, |device - host| / (|host| + 1e-6): 1.6e-5 (SE),
# 5.4e-4 (MLP: small biases and weights moved by Adam steps of 1e-2).  The warps of the device (ocml) and the host (libm) differ in
# the last ulp and the fp32 evaluation carries that apart.
RTOL32_LOSS = 2e-6
RTOL32_PARAM = {'squared_exponential': 1.6e-4, 'matern52_mlp': 5.4e-3}


def _mods():
  from hyperbo_amd import _native as nat
  from hyperbo_amd.basics import definitions as defs, lbfgs
  from hyperbo_amd.gp_utils import gp, objectives, utils
  return nat, defs, lbfgs, gp, objectives, utils


def _run(kname, mname, data, on_device, steps=200, lr=1e-2, batch_size=129, key=7, dtype=np.float64, warp=None, model=None):
  nat, defs, lbfgs, gp, objectives, utils = _mods()
  mean_func, cov_func = cases.funcs(kname, mname)
  config = {'method': 'adam', 'batch_size': batch_size, 'max_training_step': steps, 'learning_rate': lr, 'objective': objectives.nll}
  if on_device:
    config['adam_on_device'] = True
  m = model if model is not None else cases.model_of(kname, mname, dtype=dtype)
  m = {k: (dict(v) if isinstance(v, dict) else v) for k, v in m.items()}
  g = gp.GP(data, mean_func, cov_func, defs.GPParams(model=m, config=config), warp if warp is not None else utils.DEFAULT_WARP_FUNC)
  log = []
  g.train(key=key, callback=lambda i, mp, loss: log.append((i, loss, lbfgs.tree_flatten(mp)[0])))
  return log, lbfgs.tree_flatten(g.params.model)[0]


def _sizes(tasks=24, lo=60, hi=128, seed=5):
  return [int(v) for v in np.random.default_rng(seed).integers(lo, hi + 1, size=tasks)]


def _compare(host, dev, rtol, atol=1e-12):
  (hlog, hfin), (dlog, dfin) = host, dev
  assert [i for i, _, _ in dlog] == [i for i, _, _ in hlog]
  np.testing.assert_allclose([l for _, l, _ in dlog], [l for _, l, _ in hlog], rtol=rtol, atol=0)
  np.testing.assert_allclose(np.array([x for _, _, x in dlog]), np.array([x for _, _, x in hlog]), rtol=rtol, atol=atol)
  np.testing.assert_allclose(dfin, hfin, rtol=rtol, atol=atol)


@pytest.mark.parametrize('kname,mname,d,feats', [pytest.param(k, mu, cases.D, cases.FEATS, id=f'{k}-{mu}') for k, mu in cases.FAMILIES] +
                         [pytest.param(k, mu, d, f, id=f'{k}-{mu}-d{d}-f{f[-1]}') for k, mu, d, f in cases.WIDE_FAMILIES])
def test_device_adam_matches_host_driver_fp64(gpu_ctx, kname, mname, d, feats):
  data = cases.dataset(_sizes(), d=d)
  model = cases.model_of(kname, mname, d=d, feats=feats)
  host = _run(kname, mname, data, False, model=model)
  dev = _run(kname, mname, data, True, model=model)
  assert len(host[0]) == 200
  mlp = kname.endswith('_mlp') or mname == 'linear_mlp'
  _compare(host, dev, RTOL64_MLP if mlp else RTOL64, atol=1e-10 if mlp else 1e-12)


@pytest.mark.parametrize('kname,mname', [('squared_exponential', 'constant'), ('matern52_mlp', 'linear_mlp')])
def test_device_adam_matches_host_driver_fp32(gpu_ctx, kname, mname):
  data = cases.dataset(_sizes(), dtype=np.float32)
  host = _run(kname, mname, data, False, dtype=np.float32)
  dev = _run(kname, mname, data, True, dtype=np.float32)
  assert len(host[0]) == 200
  (hlog, hfin), (dlog, dfin) = host, dev
  assert [i for i, _, _ in dlog] == [i for i, _, _ in hlog]
  np.testing.assert_allclose([l for _, l, _ in dlog], [l for _, l, _ in hlog], rtol=RTOL32_LOSS, atol=0)
  hx, dx = np.array([x for _, _, x in hlog] + [hfin]), np.array([x for _, _, x in dlog] + [dfin])
  assert np.max(np.abs(dx - hx) / (np.abs(hx) + 1e-6)) <= RTOL32_PARAM[kname]


def test_device_adam_resampled_batches_match(gpu_ctx):
  sizes = [400] * 23 + [80]   # one task smaller than the batch: kept whole every step
  data = cases.dataset(sizes)
  host = _run('squared_exponential', 'constant', data, False, batch_size=100, key=11)
  dev = _run('squared_exponential', 'constant', data, True, batch_size=100, key=11)
  _compare(host, dev, RTOL64)
  other = _run('squared_exponential', 'constant', data, True, batch_size=100, key=12)
  assert other[0][1][1] != dev[0][1][1]   # another key, other batches


def test_device_adam_crosses_a_segment_boundary(gpu_ctx):
  from hyperbo_amd.gp_utils import gp
  assert gp.ADAM_SEGMENT < 300
  data = cases.dataset(_sizes())
  host = _run('matern32', 'linear', data, False, steps=300)
  dev = _run('matern32', 'linear', data, True, steps=300)
  assert len(dev[0]) == 300
  _compare(host, dev, RTOL64)


def test_device_adam_nan_at_step_zero_raises(gpu_ctx):
  data = cases.dataset(_sizes(tasks=4))
  x = data[2].x.copy(); x[3, 1] = np.nan
  data[2] = type(data[2])(x, data[2].y)
  for on_device in (False, True):
    with pytest.raises(ValueError, match='NaN'):
      _run('squared_exponential', 'constant', data, on_device, steps=5)


def test_device_adam_stops_where_the_host_driver_stops(gpu_ctx):
  nat, defs, lbfgs, gp, objectives, utils = _mods()
  # an identity-warped noise variance: large steps drive it below zero and the Gram matrix stops being positive definite
  warp = dict(utils.DEFAULT_WARP_FUNC, noise_variance=utils.identity_warp)
  data = cases.dataset(_sizes(tasks=6))
  model = cases.model_of('squared_exponential', 'constant')
  model['noise_variance'] = np.array(0.3)
  model['lengthscale'] = np.full(cases.D, -1.0)
  stopped = None
  for lr in (0.05, 0.1, 0.3, 1.0):
    host = _run('squared_exponential', 'constant', data, False, steps=60, lr=lr, warp=warp, model=model)
    if 0 < len(host[0]) < 60:
      stopped = lr
      break
  assert stopped is not None, 'the host driver never stopped early: the case does not test the halt'
  dev = _run('squared_exponential', 'constant', data, True, steps=60, lr=stopped, warp=warp, model=model)
  assert len(dev[0]) == len(host[0])
  _compare(host, dev, RTOL64)


def test_device_adam_evaluates_from_python_only_once(gpu_ctx, monkeypatch):
  nat, defs, lbfgs, gp, objectives, utils = _mods()
  calls = []
  orig = objectives.DeviceDataset.evaluate

  def spy(self, *a, **k):
    calls.append(1)
    return orig(self, *a, **k)
  monkeypatch.setattr(objectives.DeviceDataset, 'evaluate', spy)
  data = cases.dataset(_sizes(tasks=8))
  log, _ = _run('squared_exponential', 'constant', data, True, steps=50)
  assert len(log) == 50
  assert len(calls) == 1   # the final evaluation at the updated parameters
  calls.clear()
  _run('squared_exponential', 'constant', data, False, steps=50)
  assert len(calls) == 51


def test_device_adam_refuses_the_blocked_regime(gpu_ctx):
  nat, defs, lbfgs, gp, objectives, utils = _mods()
  ctx = nat.default_context()
  data = cases.dataset(_sizes(tasks=4))
  ctx.set_option('small_fused', 0)
  try:
    with pytest.raises(ValueError, match='small_fused'):
      _run('squared_exponential', 'constant', data, True, steps=3)
  finally:
    ctx.set_option('small_fused', 1)
