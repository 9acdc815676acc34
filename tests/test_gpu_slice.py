"""GPU tier: the batched value-only NLL of S hyper-parameter samples (hbo_nll_samples) and the slice sampler built on it
(infer_parameters(method='slice_sample'), HGP.train, an HGP in simulated_bayesopt)."""
import ctypes as C

import numpy as np
import pytest

import helpers
import slice_oracle
from oracle import hyperbo_oracle as o

pytestmark = pytest.mark.gpu
WFO = o.DEFAULT_WARP_FUNC


def _native():
  from hyperbo_amd import _model, _native as nat
  from hyperbo_amd.basics import definitions as defs
  from hyperbo_amd.gp_utils import gp, kernel, mean, objectives, utils
  return nat, _model, defs, gp, kernel, mean, objectives, utils


SHAPES = {'fused': [100] * 24, 'blocked': [90, 300]}


def _dataset(sizes, d, dtype, seed=1):
  rng = np.random.default_rng(seed)
  return {i: helpers.synthetic_task(rng, n, d, dtype=dtype) for i, n in enumerate(sizes)}


def _samples(mname, mlp, d, dtype, count, seed=2):
  """`count` params.model dicts of one family: the same structure, different values."""
  out = []
  for s in range(count):
    rng = np.random.default_rng(seed + 31 * s)
    m = helpers.make_model(rng, mname, mlp, d, dtype)
    m['signal_variance'] = np.array(0.3 + 0.2 * rng.normal(), dtype=dtype)
    m['noise_variance'] = np.array(-2.0 + 0.3 * rng.normal(), dtype=dtype)
    m['constant'] = np.array(0.4 + rng.normal(), dtype=dtype)
    m['dot_prod_sigma'] = np.array(0.7 + 0.1 * rng.normal(), dtype=dtype)
    out.append(m)
  return out


def _call(ctx, dev, built):
  nat = _native()[0]
  structs = (nat.Model * len(built))(*[b.struct for b in built])
  tot = np.full(len(built), -1.0)
  pt = np.full((len(built), dev.num_tasks), -1.0)
  rc = nat.lib().hbo_nll_samples(ctx.handle, structs, len(built), dev._h, tot.ctypes.data_as(C.POINTER(C.c_double)),
                                 pt.ctypes.data_as(C.POINTER(C.c_double)))
  return rc, tot, pt


def _solo(ctx, dev, b):
  nat = _native()[0]
  tot = C.c_double(-1.0)
  pt = (C.c_double * dev.num_tasks)()
  rc = nat.lib().hbo_nll(ctx.handle, b.ref(), dev._h, C.byref(tot), pt, None)
  return rc, tot.value, np.array(list(pt))


def _family(kname, mlp, mname, d, dtype, count, warp=True):
  nat, _model, defs, gp, kernel, mean, objectives, utils = _native()
  kn = getattr(kernel, kname + ('_mlp' if mlp else ''))
  mf = getattr(mean, mname)
  cfg = {'mlp_features': helpers.MLP_FEATURES}
  models = _samples(mname, mlp, d, dtype, count)
  wf = utils.DEFAULT_WARP_FUNC if warp else None
  built = [_model.BuiltModel(mf, kn, defs.GPParams(model=m, config=dict(cfg)), wf, dtype, d) for m in models]
  return kn, mf, cfg, models, built


@pytest.mark.parametrize('shape', ['fused', 'blocked'])
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('mname', helpers.MEANS)
@pytest.mark.parametrize('mlp', [False, True])
@pytest.mark.parametrize('kname', helpers.KERNELS)
@pytest.mark.parametrize('S', [1, 3, 17])
def test_nll_samples_vs_nll_and_oracle(gpu_ctx, S, kname, mlp, mname, dtype, shape):
  nat, _model, defs, gp, kernel, mean, objectives, utils = _native()
  d = 3
  data = _dataset(SHAPES[shape], d, dtype)
  dev = objectives.DeviceDataset({k: defs.SubDataset(x, y) for k, (x, y) in data.items()}, ctx=gpu_ctx)
  try:
    kn, mf, cfg, models, built = _family(kname, mlp, mname, d, dtype, S)
    rc, tot, pt = _call(gpu_ctx, dev, built)
    assert rc == nat.HBO_OK
    tol_nll, tol_o = (1e-12, 1e-10) if dtype == np.float64 else (1e-5, 1e-5)
    for s in range(S):
      rc1, tot1, pt1 = _solo(gpu_ctx, dev, built[s])
      assert rc1 == nat.HBO_OK
      assert abs(tot[s] - tot1) <= tol_nll * abs(tot1)
      np.testing.assert_allclose(pt[s], pt1, rtol=tol_nll, atol=0)
    dso = {k: o.SubDataset(x.astype(np.float64), y.astype(np.float64)) for k, (x, y) in data.items()}
    ko = getattr(o, kname + ('_mlp' if mlp else ''))
    for s in sorted({0, S // 2, S - 1}):
      m64 = helpers.unflatten_like(models[s], helpers.flatten(models[s]))
      vo = o.neg_log_marginal_likelihood(getattr(o, mname), ko, o.GPParams(model=m64, config=dict(cfg)), dso, WFO)
      assert abs(tot[s] / len(data) - vo) <= tol_o * abs(vo), (s, tot[s] / len(data), vo)
  finally:
    dev.close()


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('kname,mlp,mname', [('squared_exponential', False, 'constant'), ('matern52', True, 'linear_mlp'),
                                             ('dot_product', False, 'linear'), ('matern32', False, 'linear_mlp')])
def test_fused_batch_independence_bitwise(gpu_ctx, kname, mlp, mname, dtype):
  """A sample's per-task values do not depend on the other samples of the call: alone, in a batch of 17, in reverse order."""
  nat, _model, defs, gp, kernel, mean, objectives, utils = _native()
  d = 3
  data = _dataset(SHAPES['fused'], d, dtype)
  dev = objectives.DeviceDataset({k: defs.SubDataset(x, y) for k, (x, y) in data.items()}, ctx=gpu_ctx)
  try:
    _, _, _, _, built = _family(kname, mlp, mname, d, dtype, 17)
    rc, tot, pt = _call(gpu_ctx, dev, built)
    assert rc == nat.HBO_OK
    rc_r, tot_r, pt_r = _call(gpu_ctx, dev, built[::-1])
    assert rc_r == nat.HBO_OK
    assert np.array_equal(tot_r[::-1], tot) and np.array_equal(pt_r[::-1], pt)
    for s in (0, 5, 16):
      rc1, tot1, pt1 = _call(gpu_ctx, dev, [built[s]])
      assert rc1 == nat.HBO_OK and np.array_equal(tot1[0], tot[s]) and np.array_equal(pt1[0], pt[s])
    rc2, tot2, pt2 = _call(gpu_ctx, dev, built)   # identical calls: identical bits
    assert np.array_equal(tot2, tot) and np.array_equal(pt2, pt)
  finally:
    dev.close()


@pytest.mark.parametrize('shape', ['fused', 'blocked'])
def test_non_pd_sample_is_nan_alone(gpu_ctx, shape):
  """Unwarped parameters, one sample with a negative noise variance: its Gram matrices are not PD.  Its row is NaN, the call
  returns HBO_NOT_PD, and every other row is bit-identical to the same call without the bad sample."""
  nat, _model, defs, gp, kernel, mean, objectives, utils = _native()
  d = 3
  data = _dataset(SHAPES[shape], d, np.float64)
  dev = objectives.DeviceDataset({k: defs.SubDataset(x, y) for k, (x, y) in data.items()}, ctx=gpu_ctx)
  try:
    models = []
    for s in range(4):
      models.append({'lengthscale': np.full(d, 0.5 + 0.1 * s), 'signal_variance': np.array(1.0 + 0.1 * s),
                     'noise_variance': np.array(-50.0 if s == 2 else 0.1), 'constant': np.array(0.1 * s)})
    built = [_model.BuiltModel(mean.constant, kernel.squared_exponential, defs.GPParams(model=m), None, np.float64, d) for m in models]
    rc, tot, pt = _call(gpu_ctx, dev, built)
    assert rc == nat.HBO_NOT_PD
    assert np.isnan(tot[2]) and np.isnan(pt[2]).all()
    good = [0, 1, 3]
    rc_g, tot_g, pt_g = _call(gpu_ctx, dev, [built[s] for s in good])
    assert rc_g == nat.HBO_OK and np.all(np.isfinite(tot_g))
    if shape == 'fused':
      assert np.array_equal(tot[good], tot_g) and np.array_equal(pt[good], pt_g)
    else:
      np.testing.assert_allclose(tot[good], tot_g, rtol=1e-12, atol=0)
    for i, s in enumerate(good):
      rc1, tot1, _ = _solo(gpu_ctx, dev, built[s])
      assert rc1 == nat.HBO_OK and abs(tot1 - tot[s]) <= 1e-12 * abs(tot1)
  finally:
    dev.close()


def test_unsupported_and_mixed_families(gpu_ctx):
  nat, _model, defs, gp, kernel, mean, objectives, utils = _native()
  d = 3
  data = _dataset([40, 50], d, np.float64)
  dev = objectives.DeviceDataset({k: defs.SubDataset(x, y) for k, (x, y) in data.items()}, ctx=gpu_ctx)
  try:
    _, _, _, _, built = _family('squared_exponential', False, 'constant', d, np.float64, 3)
    structs = (nat.Model * 3)(*[b.struct for b in built])
    structs[1].input_warp = 1   # a Kumaraswamy sample
    tot = np.zeros(3)
    rc = nat.lib().hbo_nll_samples(gpu_ctx.handle, structs, 3, dev._h, tot.ctypes.data_as(C.POINTER(C.c_double)), None)
    assert rc == nat.HBO_ERR_UNSUPPORTED
    _, _, _, _, other = _family('matern52', False, 'constant', d, np.float64, 1)
    rc, _, _ = _call(gpu_ctx, dev, built[:2] + other)
    assert rc == nat.HBO_ERR_ARG
    _, _, _, _, mlp_a = _family('squared_exponential', True, 'constant', d, np.float64, 2)
    cfg_b = {'mlp_features': (4, 6)}
    m_b = helpers.make_model(np.random.default_rng(9), 'constant', True, d)
    m_b['mlp_params']['Dense_1'] = {'kernel': np.ones((4, 6)) * 0.1, 'bias': np.zeros(6)}
    m_b['lengthscale'] = np.ones(6)
    b_b = _model.BuiltModel(mean.constant, kernel.squared_exponential_mlp, defs.GPParams(model=m_b, config=cfg_b), utils.DEFAULT_WARP_FUNC,
                            np.float64, d)
    rc, _, _ = _call(gpu_ctx, dev, mlp_a + [b_b])
    assert rc == nat.HBO_ERR_ARG
    assert _call(gpu_ctx, dev, mlp_a)[0] == nat.HBO_OK
  finally:
    dev.close()


def test_log_densities_apply_priors_per_sample(gpu_ctx):
  nat, _model, defs, gp, kernel, mean, objectives, utils = _native()
  from hyperbo_amd.gp_utils import priors
  d = 2
  data = {k: defs.SubDataset(x, y) for k, (x, y) in _dataset([30, 40, 50], d, np.float64).items()}
  cfg = {'priors': priors.DEFAULT_PRIORS}
  models = _samples('constant', False, d, np.float64, 5)
  got = objectives.nll_log_densities(mean.constant, kernel.matern32, cfg, models, data, utils.DEFAULT_WARP_FUNC)
  for s, m in enumerate(models):
    ref = objectives.neg_log_marginal_likelihood(mean.constant, kernel.matern32, defs.GPParams(model=m, config=cfg), data,
                                                 utils.DEFAULT_WARP_FUNC)
    assert abs(got[s] + ref) <= 1e-12 * abs(ref)


def test_infer_parameters_slice_sample_equals_restatement(gpu_ctx):
  """infer_parameters(method='slice_sample') on the device against the sequential restatement (tests/slice_oracle.py) driven by
  the oracle NLL with the same priors: every kept sample to 1e-8."""
  nat, _model, defs, gp, kernel, mean, objectives, utils = _native()
  from hyperbo_amd.gp_utils import priors
  d = 2
  raw = _dataset([40, 60, 25], d, np.float64, seed=4)
  model = {'constant': np.array(0.1), 'lengthscale': np.zeros(d), 'signal_variance': np.array(0.0), 'noise_variance': np.array(-3.0)}
  cfg = {'method': 'slice_sample', 'burnin': 3, 'nsamples': 4, 'slice_chains': 3, 'priors': priors.DEFAULT_PRIORS,
         'max_training_step': 0, 'batch_size': 10}
  params = defs.GPParams(model={k: v.copy() for k, v in model.items()}, config=dict(cfg))
  seen = []
  out = gp.infer_parameters(mean.constant, kernel.squared_exponential, params, {k: defs.SubDataset(x, y) for k, (x, y) in raw.items()},
                            warp_func=utils.DEFAULT_WARP_FUNC, key=123, callback=lambda i, m, loss: seen.append(loss))
  assert len(out.samples) == 12 and out.cache == {}
  for smp in out.samples:
    assert set(smp) == set(model)
    for k in model:
      assert np.shape(smp[k]) == np.shape(model[k]) and np.asarray(smp[k]).dtype == np.asarray(model[k]).dtype
  assert all(np.array_equal(out.model[k], out.samples[-1][k]) for k in model)
  assert seen and all(np.isfinite(seen))
  dso = {k: o.SubDataset(x, y) for k, (x, y) in raw.items()}
  po_cfg = {'priors': {'noise_variance': priors.noise_prior, 'signal_variance': priors.lognormal_prior, 'constant': priors.constant_prior}}

  def log_density(x):
    p = o.GPParams(model=helpers.unflatten_like(model, x), config=po_cfg)
    return -o.neg_log_marginal_likelihood(o.constant, o.squared_exponential, p, dso, WFO)
  ref = slice_oracle.slice_sample(log_density, helpers.flatten(model), np.random.default_rng(123), 3, 3, 4)
  got = np.array([helpers.flatten(s) for s in out.samples])
  np.testing.assert_allclose(got, ref, rtol=0, atol=1e-8)


MIRROR_KERNELS = ['squared_exponential', 'matern32', 'matern52', 'matern32_mlp', 'matern52_mlp', 'squared_exponential_mlp',
                  'dot_product_mlp']


@pytest.mark.parametrize('kname', MIRROR_KERNELS)
def test_mirror_of_reference_slice_sampling_test(gpu_ctx, kname):
  """hyperbo/gp_utils/slice_sampling_test.py:56-153 with NumPy draws: an HGP with mean.linear_mlp and mlp_features (8,) over ten
  sampled sub-datasets, trained by slice sampling; two predictions (nsamples 1 x the default two chains) and a lower HGP.stats NLL
  than at the start.  burnin 20 instead of the reference's 1: one transition from the initial point moves a chain only as far as
  one random slice allows, and whether that already lowers the NLL is a matter of luck; a claim tested with a fixed seed needs the
  chains to have reached the bulk of the posterior, which 20 transitions do for all seven kernels."""
  nat, _model, defs, gp, kernel, mean, objectives, utils = _native()
  from hyperbo_amd.gp_utils import priors
  cov_func = getattr(kernel, kname)
  rng = np.random.default_rng(0)
  n, nq = 6, 3
  vx = rng.normal(size=(n, 2))
  qx = rng.normal(size=(nq, 2))
  params = defs.GPParams(model={'constant': 5., 'lengthscale': .1, 'signal_variance': 1.0, 'noise_variance': 0.01})
  if kname.endswith('_mlp'):
    params.config['mlp_features'] = (8,)
    params.model['mlp_params'] = {'Dense_0': {'kernel': rng.normal(size=(2, 8)) / np.sqrt(2), 'bias': np.zeros(8)}}
    params.model['lengthscale'] = np.full(8, .1)
    if kname == 'dot_product_mlp':
      params.model['dot_prod_sigma'] = 0.5
      params.model['dot_prod_bias'] = 0.
  else:
    params.model['lengthscale'] = np.full(2, .1)
  dataset = [(vx, gp.sample_from_gp(i, mean.constant, cov_func, params, vx)) for i in range(10)]
  nsamples = 1
  init_params = defs.GPParams(
      model={'constant': 5.1, 'lengthscale': np.array([0., 0.]), 'signal_variance': 0., 'noise_variance': -4.},
      config={'method': 'slice_sample', 'burnin': 20, 'nsamples': nsamples, 'max_training_step': 0, 'logging_interval': 1,
              'priors': priors.DEFAULT_PRIORS, 'mlp_features': (8,), 'batch_size': 100})
  if kname in ('squared_exponential_mlp', 'matern32_mlp', 'matern52_mlp'):
    init_params.model['lengthscale'] = np.array([0.] * 8)
  elif kname == 'dot_product_mlp':
    init_params.model['dot_prod_sigma'] = 1.
    init_params.model['dot_prod_bias'] = 0.
  model = gp.HGP(dataset=dataset, mean_func=mean.linear_mlp, cov_func=cov_func, params=init_params,
                 warp_func=utils.DEFAULT_WARP_FUNC)
  model.initialize_params(1)
  init_nll = model.stats(verbose=False)[0]
  model.train()
  inferred_nll = model.stats(verbose=False)[0]
  assert init_nll > inferred_nll, (init_nll, inferred_nll)
  predictions = model.predict(qx, 0, True, True)
  assert len(predictions) == nsamples * 2
  for mu, cov in predictions:
    assert mu.shape == (nq, 1) and cov.shape == (nq, nq)


def test_slice_sampled_hgp_in_simulated_bayesopt(gpu_ctx, monkeypatch):
  """An HGP trained by slice sampling drives simulated_bayesopt with EI: the acquisition goes through hbo_acq_samples over all
  nsamples x chains samples."""
  nat, _model, defs, gp, kernel, mean, objectives, utils = _native()
  from hyperbo_amd.bo_utils import acfun, bayesopt
  from hyperbo_amd.gp_utils import priors
  rng = np.random.default_rng(8)
  d = 2
  f = lambda xx: -np.sum((np.atleast_2d(xx) - 0.3)**2, axis=1, keepdims=True)
  x0 = rng.uniform(size=(4, d))
  ds = {'hist0': defs.SubDataset(*helpers.synthetic_task(rng, 30, d)), 'hist1': defs.SubDataset(*helpers.synthetic_task(rng, 25, d)),
        'test': defs.SubDataset(x0, f(x0))}
  cfg = {'method': 'slice_sample', 'burnin': 2, 'nsamples': 3, 'priors': priors.DEFAULT_PRIORS, 'objective': 'nll'}
  model = gp.HGP(ds, mean.constant, kernel.matern52,
                 defs.GPParams(model={'constant': 0., 'lengthscale': np.zeros(d), 'signal_variance': 0., 'noise_variance': -3.},
                               config=cfg), utils.DEFAULT_WARP_FUNC)
  model.train(key=5)
  assert len(model.params.samples) == 6
  lib = nat.lib()
  orig = lib.hbo_acq_samples
  counts = []

  def spy(*args):
    counts.append(args[2])
    return orig(*args)
  monkeypatch.setattr(lib, 'hbo_acq_samples', spy)
  pool = defs.SubDataset(rng.uniform(size=(50, d)), None)
  pool = defs.SubDataset(pool.x, f(pool.x))
  out = bayesopt.simulated_bayesopt(model, 'test', pool, acfun.expected_improvement, iters=3)
  assert out.x.shape == (7, d) and out.y.shape == (7, 1)
  assert counts and sum(counts) % 6 == 0 and all(c <= 6 for c in counts)
  assert sum(counts) >= 3 * 6
