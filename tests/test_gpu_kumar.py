"""Kumaraswamy input-warped kernels (*_kumar) on the MI355X: Gram, objectives with the a / b gradient leaves, posterior,
acquisition, training, and the rejections, against the oracle's kernels composed with a NumPy KumarWarp (tests/kumar_oracle.py)."""
import copy

import numpy as np
import pytest

import helpers
import kumar_oracle as ko
from oracle import hyperbo_oracle as o

pytestmark = pytest.mark.gpu
WFO = o.DEFAULT_WARP_FUNC
FP64_GRAM_TOL = 1e-13
FP64_GRAD_TOL = 1e-10     # per leaf, as tests/test_gpu_parity.py
FP32_GRAM_TOL = 2e-5
BASES = ['squared_exponential', 'matern32', 'matern52', 'dot_product']


def _native():
  from hyperbo_amd import _native as nat
  from hyperbo_amd.basics import definitions as defs
  from hyperbo_amd.bo_utils import acfun
  from hyperbo_amd.gp_utils import gp, kernel, mean, objectives, utils
  return nat, defs, acfun, gp, kernel, mean, objectives, utils


def _model(rng, d, mname='constant', kumar=True, spread=1.5):
  m = helpers.make_model(rng, mname, False, d)
  if kumar:
    m['kumar_params'] = {'a': rng.uniform(-spread, spread, size=d), 'b': rng.uniform(-spread, spread, size=d)}
  return m


def _x(rng, n, d, dtype=np.float64):
  x = rng.uniform(size=(n, d))
  x.flat[::7] = 0.0
  x.flat[3::11] = 1.0
  return x.astype(dtype)


def _warped_dataset(ds, kp):
  return {k: o.SubDataset(ko.warp(v.x, kp['a'], kp['b']), v.y, v.aligned) for k, v in ds.items()}


def _without_kumar(model):
  m = dict(model); m.pop('kumar_params', None)
  return m


# ---- identity anchor -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('base', BASES)
def test_identity_warp_equals_the_plain_kernel_bit_for_bit(gpu_ctx, base):
  nat, defs, _, gp, kernel, mean, objectives, utils = _native()
  rng = np.random.default_rng(1)
  d = 5
  model = _model(rng, d, kumar=False)
  p = defs.GPParams(model=dict(model))
  kernel.init_kumar_warp_with_shape(None, p, (1, d))
  pp = defs.GPParams(model=dict(model))
  x = _x(rng, 150, d); x2 = _x(rng, 40, d)
  kk, kp = getattr(kernel, base + '_kumar'), getattr(kernel, base)
  wf = utils.DEFAULT_WARP_FUNC
  np.testing.assert_array_equal(kk(p, x, warp_func=wf), kp(pp, x, warp_func=wf))
  np.testing.assert_array_equal(kk(p, x, x2, warp_func=wf), kp(pp, x, x2, warp_func=wf))
  np.testing.assert_array_equal(kk(p, x, warp_func=wf, diag=True), kp(pp, x, warp_func=wf, diag=True))
  for n in (100, 300):   # the fused single-workgroup path and the blocked one
    ds = {i: defs.SubDataset(*helpers.synthetic_task(rng, n, d)) for i in range(2)}
    vk, gk = objectives.nll_value_and_grad(mean.constant, kk, p, ds, wf)
    vp, gpl = objectives.nll_value_and_grad(mean.constant, kp, pp, ds, wf)
    assert vk == vp
    for key in gpl:
      np.testing.assert_array_equal(gk[key], gpl[key], err_msg=key)
  y = np.sin(x[:, :1])
  mk, vk = gp.predict(mean.constant, kk, p, x, y, x2, wf)
  mp, vp = gp.predict(mean.constant, kp, pp, x, y, x2, wf)
  np.testing.assert_array_equal(mk, mp); np.testing.assert_array_equal(vk, vp)


# ---- Gram -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('base', BASES)
@pytest.mark.parametrize('d', [1, 16, 64])
@pytest.mark.parametrize('dtype,tol', [(np.float64, FP64_GRAM_TOL), (np.float32, FP32_GRAM_TOL)])
def test_gram_vs_oracle_on_warped_inputs(gpu_ctx, base, d, dtype, tol):
  nat, defs, _, _, kernel, _, _, utils = _native()
  rng = np.random.default_rng(d)
  model = _model(rng, d)
  model['lengthscale'] = np.abs(model['lengthscale']) + 0.5 * np.sqrt(d)
  kp = model['kumar_params']
  x1, x2 = _x(rng, 200, d), _x(rng, 130, d)
  pn = defs.GPParams(model=copy.deepcopy(model))
  kn = getattr(kernel, base + '_kumar'); kb = getattr(o, base)
  po = o.GPParams(model=_without_kumar(model))
  w1, w2 = ko.warp(x1, kp['a'], kp['b']), ko.warp(x2, kp['a'], kp['b'])
  for got, ref in [(kn(pn, x1.astype(dtype), warp_func=utils.DEFAULT_WARP_FUNC), kb(po, w1, warp_func=WFO)),
                   (kn(pn, x1.astype(dtype), x2.astype(dtype), warp_func=utils.DEFAULT_WARP_FUNC), kb(po, w1, w2, warp_func=WFO)),
                   (kn(pn, x1.astype(dtype), warp_func=utils.DEFAULT_WARP_FUNC, diag=True), kb(po, w1, warp_func=WFO, diag=True))]:
    assert got.dtype == dtype and got.shape == ref.shape
    assert helpers.rel_err(got, ref) < tol


# ---- objectives ------------------------------------------------------------------------------------------------------
def _fd_ab(fn, model, h=1e-5):
  out = {}
  for key in ('a', 'b'):
    g = np.zeros_like(model['kumar_params'][key])
    for i in range(g.size):
      mp = copy.deepcopy(model); mm = copy.deepcopy(model)
      mp['kumar_params'][key][i] += h; mm['kumar_params'][key][i] -= h
      g[i] = (fn(mp) - fn(mm)) / (2 * h)
    out[key] = g
  return out


@pytest.mark.parametrize('sizes', [(300, 129, 64), (100,) * 24])
def test_nll_value_and_grad_se_kumar_fp64(gpu_ctx, sizes):
  nat, defs, _, _, kernel, mean, objectives, utils = _native()
  rng = np.random.default_rng(len(sizes))
  d = 6
  model = _model(rng, d)
  dso = {i: o.SubDataset(_x(rng, n, d), np.sin(3 * rng.uniform(size=(n, 1)))) for i, n in enumerate(sizes)}
  dsn = {k: defs.SubDataset(v.x, v.y) for k, v in dso.items()}
  gpu_ctx.profile_enable(1)
  try:
    vn, gn = objectives.nll_value_and_grad(mean.constant, kernel.squared_exponential_kumar, defs.GPParams(model=copy.deepcopy(model)), dsn,
                                           utils.DEFAULT_WARP_FUNC)
    stages = gpu_ctx.profile_get()
  finally:
    gpu_ctx.profile_enable(0)
  if len(sizes) == 24:
    assert 'small_eval' in stages and 'kumar_forward' in stages and 'kumar_backward' in stages, sorted(stages)
  po = o.GPParams(model=_without_kumar(model))
  vo, go = o.nll_value_and_grad(o.constant, o.squared_exponential, po, _warped_dataset(dso, model['kumar_params']), WFO)
  assert abs(vn - vo) <= 1e-10 * abs(vo)
  ga, gb = ko.se_nll_ab_grad(model, dso)
  go['kumar_params'] = {'a': ga, 'b': gb}
  helpers.assert_grad_close(gn, go, FP64_GRAD_TOL)


@pytest.mark.parametrize('base', BASES)
def test_nll_with_linear_mean_sees_raw_x(gpu_ctx, base):
  """All leaves against fp64 central differences of the oracle (kernel on w(x), linear mean on raw x).  The FD reference
  carries ~1e-9 relative truncation + rounding error at h = 1e-5 (measured against the analytic SE gradient above); 1e-6 per
  leaf leaves room for it."""
  nat, defs, _, _, kernel, mean, objectives, utils = _native()
  rng = np.random.default_rng(5)
  d = 3
  model = _model(rng, d, mname='linear')
  dso = {i: o.SubDataset(_x(rng, n, d), np.sin(3 * rng.uniform(size=(n, 1)))) for i, n in enumerate((150, 40))}
  dsn = {k: defs.SubDataset(v.x, v.y) for k, v in dso.items()}
  okern = ko.kumar_kernel(getattr(o, base))
  vn, gn = objectives.nll_value_and_grad(mean.linear, getattr(kernel, base + '_kumar'), defs.GPParams(model=copy.deepcopy(model)), dsn,
                                         utils.DEFAULT_WARP_FUNC)
  f = lambda mdl: o.neg_log_marginal_likelihood(o.linear, okern, o.GPParams(model=mdl), dso, WFO)
  vo = f(model)
  assert abs(vn - vo) <= 1e-10 * abs(vo)
  ab = _fd_ab(f, model)
  np.testing.assert_allclose(gn['kumar_params']['a'], ab['a'], rtol=1e-6, atol=1e-6 * np.max(np.abs(ab['a'])))
  np.testing.assert_allclose(gn['kumar_params']['b'], ab['b'], rtol=1e-6, atol=1e-6 * np.max(np.abs(ab['b'])))
  h = 1e-6
  for key in ('bias', 'kernel'):
    lm = model['linear_mean'][key]
    for i in range(lm.size):
      mp = copy.deepcopy(model); mm = copy.deepcopy(model)
      mp['linear_mean'][key].flat[i] += h; mm['linear_mean'][key].flat[i] -= h
      fd = (f(mp) - f(mm)) / (2 * h)
      assert abs(gn['linear_mean'][key].flat[i] - fd) <= 1e-6 * max(1.0, abs(fd))


@pytest.mark.parametrize('kind', ['ekl', 'euc'])
@pytest.mark.parametrize('base', ['squared_exponential', 'dot_product'])
def test_divergence_value_and_grad(gpu_ctx, kind, base):
  nat, defs, _, _, kernel, mean, objectives, utils = _native()
  rng = np.random.default_rng(9)
  d = 3
  model = _model(rng, d, spread=1.0)
  dso = {i: o.SubDataset(_x(rng, n, d), rng.normal(size=(n, 4)), aligned=1) for i, n in enumerate((60, 140))}
  dsn = {k: defs.SubDataset(v.x, v.y, v.aligned) for k, v in dso.items()}
  fn = objectives.ekl_value_and_grad if kind == 'ekl' else objectives.euc_value_and_grad
  vn, gn = fn(mean.constant, getattr(kernel, base + '_kumar'), defs.GPParams(model=copy.deepcopy(model)), dsn, utils.DEFAULT_WARP_FUNC)
  po = o.GPParams(model=_without_kumar(model))
  vo, go = o.divergence_value_and_grad(kind, o.constant, getattr(o, base), po, _warped_dataset(dso, model['kumar_params']), WFO)
  assert abs(vn - vo) <= 1e-9 * abs(vo)
  go = {k: v for k, v in go.items()}
  gn_rest = {k: v for k, v in gn.items() if k != 'kumar_params'}
  helpers.assert_grad_close(gn_rest, go, 1e-8)
  f = lambda mdl: o.divergence_value_and_grad(kind, o.constant, getattr(o, base), o.GPParams(model=_without_kumar(mdl)),
                                              _warped_dataset(dso, mdl['kumar_params']), WFO)[0]
  ab = _fd_ab(f, model)
  for key in ('a', 'b'):
    np.testing.assert_allclose(gn['kumar_params'][key], ab[key], rtol=1e-6, atol=1e-6 * np.max(np.abs(ab[key])))


def test_fp32_nll_grad_against_fp64(gpu_ctx):
  nat, defs, _, _, kernel, mean, objectives, utils = _native()
  rng = np.random.default_rng(12)
  d = 4
  model = _model(rng, d, spread=1.0)
  ds64 = {i: defs.SubDataset(_x(rng, n, d), np.sin(3 * rng.uniform(size=(n, 1)))) for i, n in enumerate((200, 90))}
  ds32 = {k: defs.SubDataset(v.x.astype(np.float32), v.y.astype(np.float32)) for k, v in ds64.items()}
  p = lambda: defs.GPParams(model=copy.deepcopy(model))
  v64, g64 = objectives.nll_value_and_grad(mean.constant, kernel.matern52_kumar, p(), ds64, utils.DEFAULT_WARP_FUNC)
  v32, g32 = objectives.nll_value_and_grad(mean.constant, kernel.matern52_kumar, p(), ds32, utils.DEFAULT_WARP_FUNC)
  assert abs(v32 - v64) <= 1e-3 * abs(v64)
  helpers.assert_grad_close(g32, g64, 2.5e-3, floor_rel=1e-2)


def test_cfg2_full_size_se_kumar_and_bit_identical_repeats(gpu_ctx):
  nat, defs, _, _, kernel, mean, objectives, utils = _native()
  rng = np.random.default_rng(2)
  n, d = 8192, 16
  model = _model(rng, d, spread=1.0)
  model['lengthscale'] = np.full(d, 1.0)
  x = _x(rng, n, d)
  y = np.sin(2 * np.pi * x @ rng.normal(size=(d, 1)) / 4) + 0.1 * rng.normal(size=(n, 1))
  dso = {0: o.SubDataset(x, y)}
  dsn = {0: defs.SubDataset(x, y)}
  p = lambda: defs.GPParams(model=copy.deepcopy(model))
  v1, g1 = objectives.nll_value_and_grad(mean.constant, kernel.squared_exponential_kumar, p(), dsn, utils.DEFAULT_WARP_FUNC)
  v2, g2 = objectives.nll_value_and_grad(mean.constant, kernel.squared_exponential_kumar, p(), dsn, utils.DEFAULT_WARP_FUNC)
  assert v1 == v2
  for (path, a), (_, b) in zip(helpers.tree_leaves(g1), helpers.tree_leaves(g2)):
    np.testing.assert_array_equal(a, b, err_msg=path)
  vo, go = o.nll_value_and_grad(o.constant, o.squared_exponential, o.GPParams(model=_without_kumar(model)),
                                _warped_dataset(dso, model['kumar_params']), WFO)
  assert abs(v1 - vo) <= 1e-10 * abs(vo)
  ga, gb = ko.se_nll_ab_grad(model, dso)
  go['kumar_params'] = {'a': ga, 'b': gb}
  helpers.assert_grad_close(g1, go, FP64_GRAD_TOL)


def test_sharded_objective_carries_the_kumar_leaves(gpu_ctx):
  """hbo_objective_sharded: the device-side scatter of two shards, summed, equals hbo_objective on their union (2 D leaves
  included); with a one-rank RCCL communicator the all-reduced result equals the local one."""
  nat, defs, _, _, kernel, mean, objectives, utils = _native()
  from hyperbo_amd import parallel
  rng = np.random.default_rng(4)
  d = 5
  model = _model(rng, d)
  ds = {i: defs.SubDataset(_x(rng, n, d), rng.normal(size=(n, 1))) for i, n in enumerate((140, 60, 100, 300))}
  p = defs.GPParams(model=copy.deepcopy(model))
  kn = kernel.matern32_kumar
  full = objectives._as_device(ds, True)[0]
  sa = objectives._as_device({k: ds[k] for k in (0, 1)}, True)[0]
  sb = objectives._as_device({k: ds[k] for k in (2, 3)}, True)[0]
  try:
    s0, _, g0, bm = full.evaluate(mean.constant, kn, p, utils.DEFAULT_WARP_FUNC, want_grad=True)
    s1, c1, g1, _ = sa.evaluate_sharded(mean.constant, kn, p, utils.DEFAULT_WARP_FUNC)
    s2, c2, g2, _ = sb.evaluate_sharded(mean.constant, kn, p, utils.DEFAULT_WARP_FUNC)
  finally:
    for dv in (full, sa, sb):
      dv.close()
  ao, bo = bm.kumar_offsets
  assert c1 + c2 == 4 and len(g0) == bm.layout.total and bo == len(g0) - d
  assert abs((s1 + s2) - s0) <= 1e-12 * abs(s0)
  np.testing.assert_allclose(np.asarray(g1) + np.asarray(g2), g0, rtol=1e-11, atol=1e-12 * np.max(np.abs(g0)))
  assert np.any(np.asarray(g0)[ao:] != 0)
  comm = parallel.RcclComm(gpu_ctx, 0, 1, lambda b: b)
  try:
    v1, gr1 = objectives.nll_value_and_grad(mean.constant, kn, defs.GPParams(model=copy.deepcopy(model)), ds, utils.DEFAULT_WARP_FUNC, comm=comm)
  finally:
    comm.close()
  v0, gr0 = objectives.nll_value_and_grad(mean.constant, kn, defs.GPParams(model=copy.deepcopy(model)), ds, utils.DEFAULT_WARP_FUNC)
  assert v1 == v0
  for key in ('a', 'b'):
    np.testing.assert_array_equal(gr1['kumar_params'][key], gr0['kumar_params'][key])


# ---- posterior / acquisition -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('base', ['matern52', 'dot_product'])
def test_predict_append_and_acquisition(gpu_ctx, base):
  nat, defs, acfun, gp, kernel, mean, _, utils = _native()
  rng = np.random.default_rng(6)
  d = 3
  model = _model(rng, d, mname='linear', spread=1.0)
  kn = getattr(kernel, base + '_kumar'); okern = ko.kumar_kernel(getattr(o, base))
  x, y = _x(rng, 200, d), rng.normal(size=(200, 1))
  xq = rng.uniform(0.05, 0.95, size=(70, d))
  po = o.GPParams(model=model); pn = defs.GPParams(model=copy.deepcopy(model))
  wf = utils.DEFAULT_WARP_FUNC
  muo, varo = o.predict(o.linear, okern, po, x, y, xq, WFO)
  mun, varn = gp.predict(mean.linear, kn, pn, x, y, xq, wf)
  assert helpers.rel_err(mun, muo) < 1e-9 and helpers.rel_err(varn, varo) < 1e-9
  _, covo = o.predict(o.linear, okern, po, x, y, xq, WFO, full_cov=True)
  _, covn = gp.predict(mean.linear, kn, pn, x, y, xq, wf, full_cov=True)
  assert helpers.rel_err(covn, covo) < 1e-9
  # cache append (O(N^2) rows on the device) then predict
  from hyperbo_amd.basics import linalg
  from hyperbo_amd import _model as hmodel
  h = linalg.factor(mean.linear, kn, pn, x[:150], y[:150], wf)
  try:
    assert h.append(pn, x[150:], y[150:])
    bm = hmodel.BuiltModel(mean.linear, kn, pn, wf, np.float64, d)
    mu_c, var_c = np.empty((70, 1)), np.empty((70, 1))
    h.ctx.check(nat.lib().hbo_predict(h.ctx.handle, bm.ref(), h.handle, nat.ptr(xq), 70, 0, nat.ptr(mu_c), nat.ptr(var_c)))
  finally:
    h.close()
  assert helpers.rel_err(mu_c, muo) < 1e-8 and helpers.rel_err(var_c, varo) < 1e-8
  # acquisition functions through the GP object
  ds = {0: defs.SubDataset(x, y), 1: defs.SubDataset(x[:50], y[:50])}
  model_n = gp.GP(ds, mean.linear, kn, pn, wf)
  dso = {k: o.SubDataset(v.x, v.y) for k, v in ds.items()}
  mu_o, var_o = o.gp_predict_postprocess(po, dso, muo, varo, WFO, False, True, True)
  for name, sub_o, par in [('expected_improvement', o.expected_improvement_sub, float(np.max(y))),
                           ('probability_of_improvement', o.probability_of_improvement_sub, float(np.max(y)) + 0.1),
                           ('ucb', o.ucb_sub, 3.0)]:
    an = getattr(acfun, name)(model=model_n, sub_dataset_key=0, x_queries=xq)
    assert helpers.rel_err(an, sub_o(mu_o, np.sqrt(var_o), par)) < 1e-8, name
  # d acq / d x at interior queries against central differences of the acquisition
  for name in ('expected_improvement', 'ucb'):
    fn = getattr(acfun, name)
    val, grad = fn.value_and_grad(model=model_n, sub_dataset_key=0, x_queries=xq[:10])
    # (hbo_acq_grad's triangular mat-vecs against hbo_acq's streamed product: measured 1.3e-10 apart)
    assert helpers.rel_err(val, fn(model=model_n, sub_dataset_key=0, x_queries=xq[:10])) < 1e-8
    hh = 1e-6
    for j in range(d):
      e = np.zeros(d); e[j] = hh
      fd = (fn(model=model_n, sub_dataset_key=0, x_queries=xq[:10] + e) - fn(model=model_n, sub_dataset_key=0, x_queries=xq[:10] - e)) / (2 * hh)
      np.testing.assert_allclose(grad[:, j], fd[:, 0], rtol=1e-5, atol=1e-7 * max(1.0, np.max(np.abs(fd))), err_msg=f'{name} d{j}')


def test_streamed_kumar_posterior_chunks_match_single_pass(gpu_ctx):
  """A Kumaraswamy model streamed through two workspaces: the linear mean reads the raw queries, the covariance w(queries), which
  lives per workspace.  post_chunk = 128 cuts 300 queries into three chunks (the last ragged) through two alternating workspaces:
  mean, variance and EI with data, and mean, variance and UCB on the prior branch, must be finite and bit-identical to the
  one-pass run, fp64 and fp32; the fp64 one-pass mean and variance are within 1e-9 of the oracle."""
  nat, defs, acfun, gp, kernel, mean, _, utils = _native()
  rng = np.random.default_rng(14)
  d = 3
  model = _model(rng, d, mname='linear', spread=1.0)
  x, y = _x(rng, 200, d), rng.normal(size=(200, 1))
  xq = rng.uniform(0.05, 0.95, size=(300, d))
  muo, varo = o.predict(o.linear, ko.kumar_kernel(o.matern52), o.GPParams(model=model), x, y, xq, WFO)
  for dtype in (np.float64, np.float32):
    cast = lambda t: {k: cast(v) for k, v in t.items()} if isinstance(t, dict) else np.asarray(t, dtype=dtype)
    g = gp.GP({0: defs.SubDataset(x.astype(dtype), y.astype(dtype)), 1: defs.SubDataset(np.zeros((0, d), dtype), np.zeros((0, 1), dtype))},
              mean.linear, kernel.matern52_kumar, defs.GPParams(model=cast(model)), utils.DEFAULT_WARP_FUNC)
    q = xq.astype(dtype)
    ref = None
    try:
      for chunk in (65536, 128):
        gpu_ctx.set_option('post_chunk', chunk)
        p0, ei = g.predict(q, 0), acfun.expected_improvement(model=g, sub_dataset_key=0, x_queries=q)
        p1, ucb = g.predict(q, 1), acfun.ucb(model=g, sub_dataset_key=1, x_queries=q)
        flat = [p0[0], p0[1], ei, p1[0], p1[1], ucb]
        assert all(np.isfinite(a).all() for a in flat), chunk
        if ref is None:
          ref = flat
          if dtype == np.float64:
            mu, var = g.predict(q, 0, with_noise=False, unbiased=False)
            assert helpers.rel_err(mu, muo) < 1e-9 and helpers.rel_err(var, varo) < 1e-9
        else:
          for a, b in zip(flat, ref):
            assert np.array_equal(a, b), chunk
    finally:
      gpu_ctx.set_option('post_chunk', 8192)


# ---- training ------------------------------------------------------------------------------------------------------------
def test_gp_train_adam_moves_kumar_params_like_the_numpy_loop(gpu_ctx):
  """GP.train (Adam, full batches) against the same Adam loop in NumPy on the oracle NLL's gradient (analytic SE-kumar a / b
  leaves, oracle leaves on w(x) for the rest)."""
  nat, defs, _, gp, kernel, mean, objectives, utils = _native()
  rng = np.random.default_rng(8)
  d, steps, lr = 2, 20, 0.05
  model = _model(rng, d, spread=0.5)
  ds = {i: defs.SubDataset(*helpers.synthetic_task(rng, 60, d)) for i in range(4)}
  cfg = {'method': 'adam', 'batch_size': 1000, 'max_training_step': steps, 'learning_rate': lr}
  model_n = gp.GP(ds, mean.constant, kernel.squared_exponential_kumar, defs.GPParams(model=copy.deepcopy(model), config=dict(cfg)),
                  utils.DEFAULT_WARP_FUNC)
  init_nll, _ = model_n.neg_log_marginal_likelihood()
  model_n.train(key=0)
  nll, _ = model_n.neg_log_marginal_likelihood()
  assert np.isfinite(nll) and nll < init_nll
  # the same optimiser on the host
  dso = {k: o.SubDataset(v.x, v.y) for k, v in ds.items()}
  params = copy.deepcopy(model)
  leaves = lambda t: helpers.flatten(t)
  mom = np.zeros_like(leaves(params)); vel = np.zeros_like(mom)
  b1, b2, eps = 0.9, 0.999, 1e-8
  for t in range(1, steps + 1):
    _, go = o.nll_value_and_grad(o.constant, o.squared_exponential, o.GPParams(model=_without_kumar(params)),
                                 _warped_dataset(dso, params['kumar_params']), WFO)
    ga, gb = ko.se_nll_ab_grad(params, dso)
    go['kumar_params'] = {'a': ga, 'b': gb}
    g = leaves(go)
    mom = b1 * mom + (1 - b1) * g; vel = b2 * vel + (1 - b2) * g * g
    upd = (mom / (1 - b1 ** t)) / (np.sqrt(vel / (1 - b2 ** t)) + eps)
    params = helpers.unflatten_like(params, leaves(params) - lr * upd)
  for key in ('a', 'b'):
    np.testing.assert_allclose(np.asarray(model_n.params.model['kumar_params'][key], dtype=np.float64), params['kumar_params'][key],
                               rtol=1e-6, atol=1e-8)


# ---- rejections --------------------------------------------------------------------------------------------------------
def test_acq_samples_and_hgp_reject_kumar_models(gpu_ctx):
  nat, defs, acfun, gp, kernel, mean, _, utils = _native()
  from hyperbo_amd import _model as hmodel
  import ctypes as C
  rng = np.random.default_rng(10)
  d = 2
  model = _model(rng, d)
  x, y = _x(rng, 30, d), rng.normal(size=(30, 1))
  xq = rng.uniform(size=(5, d))
  bm = hmodel.BuiltModel(mean.constant, kernel.matern52_kumar, defs.GPParams(model=model), utils.DEFAULT_WARP_FUNC, np.float64, d)
  structs = (nat.Model * 2)(bm.struct, bm.struct)
  out = np.empty((2, 5))
  prm = (C.c_double * 2)(0.0, 0.0); nse = (C.c_double * 2)(0.1, 0.1)
  rc = nat.lib().hbo_acq_samples(gpu_ctx.handle, structs, 2, nat.ptr(x), 30, nat.ptr(y), 1, nat.ptr(xq), 5, nat.ACQ_EI, prm, nse, 1.0,
                                 out.ctypes.data_as(C.c_void_p))
  assert rc == nat.HBO_ERR_UNSUPPORTED and b'Kumaraswamy' in nat.lib().hbo_last_error(gpu_ctx.handle)
  # an MLP basis on a Kumaraswamy kernel is refused by the entry points too
  bm.struct.kernel_uses_mlp = 1
  g = np.empty((30, 30))
  rc = nat.lib().hbo_gram(gpu_ctx.handle, bm.ref(), nat.ptr(x), 30, None, 30, 0, nat.ptr(g))
  assert rc == nat.HBO_ERR_UNSUPPORTED
  bm.struct.kernel_uses_mlp = 0
  # the HGP path of the Python API raises the same error
  ds = {0: defs.SubDataset(x, y)}
  samples = [copy.deepcopy(model), copy.deepcopy(model)]
  hgp = gp.HGP(ds, mean.constant, kernel.matern52_kumar, defs.GPParams(model=copy.deepcopy(model), samples=samples), utils.DEFAULT_WARP_FUNC) \
      if hasattr(gp, 'HGP') else None
  if hgp is not None:
    with pytest.raises(nat.HboError) as e:
      acfun.expected_improvement(model=hgp, sub_dataset_key=0, x_queries=xq)
    assert e.value.code == nat.HBO_ERR_UNSUPPORTED
    with pytest.raises(nat.HboError):
      acfun.expected_improvement.value_and_grad(model=hgp, sub_dataset_key=0, x_queries=xq)
    assert getattr(hgp, '_hbo_sample_caches', None) is None
