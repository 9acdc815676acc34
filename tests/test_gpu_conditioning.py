"""The fp32 Gram of the stationary covariances on the matrix cores (csrc/gram.hip: gram_mfma_kernel) where its expansion
u = |a|^2 + |b|^2 - 2 a.b is badly conditioned: small length-scales, inputs far from the origin, exact and near duplicates.
Every case is checked against the fp64 oracle on the fp32-rounded inputs (only the kernel's arithmetic is judged) and, where the
issue is the Gram itself, against the direct form sum (a - b)^2 computed on a context of its own (hbo_tune gram_mfma = 0), so that
the default context is never changed.  Run with `-m gpu`.
"""
import os

import numpy as np
import pytest

import helpers
from oracle import hyperbo_oracle as o

pytestmark = pytest.mark.gpu
WFO = o.DEFAULT_WARP_FUNC
GRAM_TOL = 2e-5          # per entry, relative to the signal variance
FP32_GRAD_TOL = 2.5e-3   # as tests/test_gpu_parity.py
KERNELS = ['squared_exponential', 'matern32', 'matern52']


def _native():
  from hyperbo_amd import _model, _native as nat
  from hyperbo_amd.basics import definitions as defs
  from hyperbo_amd.bo_utils import acfun
  from hyperbo_amd.gp_utils import gp, kernel, mean, objectives, utils
  return nat, _model, defs, acfun, gp, kernel, mean, objectives, utils


@pytest.fixture(scope='module')
def direct_ctx(gpu_ctx):
  """A second context whose fp32 Gram matrices always take the direct form; the default context is never changed."""
  nat = _native()[0]
  ctx = nat.Context(gpu_ctx.device)
  ctx.set_option('poison', 1)
  ctx.set_option('gram_mfma', 0)
  yield ctx
  ctx.close()


def _gram(ctx, kfun, params, x1, x2=None, diag=False):
  """kernel.<name>(params, x1, x2, diag=diag) evaluated on `ctx` (the library's kernels use the default context)."""
  nat, _model, _, _, _, _, mean, _, utils = _native()
  n1 = x1.shape[0]
  n2 = n1 if x2 is None else x2.shape[0]
  out = np.empty((n1,) if diag else (n1, n2), dtype=x1.dtype)
  bm = _model.BuiltModel(mean.zero, kfun, params, utils.DEFAULT_WARP_FUNC, x1.dtype, x1.shape[1])
  ctx.check(nat.lib().hbo_gram(ctx.handle, bm.ref(), nat.ptr(x1), n1, nat.ptr(x2), n2, int(diag), nat.ptr(out)), allow_not_pd=False)
  return out


def _lengthscales(rng, scale, d):
  return (scale * np.exp(rng.uniform(-0.3, 0.3, size=d))).astype(np.float32)


def _rows(rng, n, d, data, offset):
  z = rng.uniform(-1, 1, size=(n, d)) if data == 'uniform' else np.tanh(rng.normal(size=(n, d)))
  return z + offset


def _hard_data(rng, d, ls, data, offset, n1=300, n2=150):
  """x1 (n1 x d), x2 (n2 x d) in fp32 with exact duplicates inside x1 and across the sets, and near duplicates spaced 1e-3 and
  1e-5 length-scales apart; neither size is a multiple of the 128-tile."""
  x1 = _rows(rng, n1, d, data, offset)
  x2 = _rows(rng, n2, d, data, offset)
  x1[n1 - 20:] = x1[:20]                                                  # exact duplicates inside x1
  x1[n1 - 40:n1 - 20] = x1[20:40] + 1e-3 * ls * rng.normal(size=(20, d))  # near duplicates inside x1
  x2[:20] = x1[:20]                                                       # exact duplicates across the sets
  x2[20:40] = x1[20:40] + 1e-3 * ls * rng.normal(size=(20, d))
  x2[40:60] = x1[40:60] + 1e-5 * ls * rng.normal(size=(20, d))
  return x1.astype(np.float32), x2.astype(np.float32)


def _params(ls, sv=0.8, noise=1e-2):
  defs = _native()[2]
  model = {'lengthscale': helpers.inv_softplus(ls).astype(np.float32), 'signal_variance': np.float32(helpers.inv_softplus(sv)),
           'noise_variance': np.float32(helpers.inv_softplus(noise)), 'constant': np.float32(0.1)}
  return model, defs.GPParams(model=model), o.GPParams(model=helpers.unflatten_like(model, helpers.flatten(model)))


def _sv(model):
  return float(np.log1p(np.exp(np.float64(model['signal_variance']))))


def _log(line):
  if os.environ.get('HBO_GRAD_LOG'):
    with open(os.environ['HBO_GRAD_LOG'], 'a') as f_:
      f_.write(line + '\n')


# ---- (a) Gram entries -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('data', ['uniform', 'tanh'])
@pytest.mark.parametrize('offset', [0.0, 10.0, 1000.0])
@pytest.mark.parametrize('scale', [0.05, 0.1, 0.3, 2.0])
@pytest.mark.parametrize('d', [32, 64, 65])
@pytest.mark.parametrize('kname', KERNELS)
def test_fp32_gram_entries_small_lengthscales_and_offsets(gpu_ctx, direct_ctx, kname, d, scale, offset, data):
  kernel = _native()[5]
  rng = np.random.default_rng([d, int(scale * 100), int(offset), len(data), len(kname)])
  ls = _lengthscales(rng, scale, d)
  x1, x2 = _hard_data(rng, d, ls, data, offset)
  model, pn, po = _params(ls)
  sv = _sv(model)
  kn, ko = getattr(kernel, kname), getattr(o, kname)
  x1d, x2d = x1.astype(np.float64), x2.astype(np.float64)
  ref = {'sym': ko(po, x1d, warp_func=WFO), 'cross': ko(po, x1d, x2d, warp_func=WFO)}
  ref['diag'] = np.diag(ref['sym'])
  errs = {}
  for form, ctx in (('mfma', gpu_ctx), ('direct', direct_ctx)):
    got = {'sym': _gram(ctx, kn, pn, x1), 'cross': _gram(ctx, kn, pn, x1, x2), 'diag': _gram(ctx, kn, pn, x1, diag=True)}
    for k, g in got.items():
      assert g.dtype == np.float32 and g.shape == ref[k].shape
      assert np.all(np.isfinite(g)), (form, k)
      errs[form, k] = float(np.max(np.abs(g.astype(np.float64) - ref[k]))) / sv
    if form == 'mfma':
      gs = got['sym']
      assert np.array_equal(gs, gs.T)                                 # exactly symmetric
      assert np.linalg.eigvalsh(gs.astype(np.float64)).min() > -1e-5   # PSD
  _log('0 tol=gramcond %s d=%d ls=%g off=%g %s max|dK|/sv: mfma %.3e %.3e %.3e direct %.3e %.3e %.3e' % (
      (kname, d, scale, offset, data) + tuple(errs[f, k] for f in ('mfma', 'direct') for k in ('sym', 'cross', 'diag'))))
  for k in ('sym', 'cross', 'diag'):
    assert errs['mfma', k] <= GRAM_TOL, (k, errs)
    assert errs['mfma', k] <= 2 * errs['direct', k] + 1e-6, (k, errs)


# ---- (b) the call sites of the Gram ---------------------------------------------------------------------------------------------
HARD = [(32, 0.1, 10.0, 'tanh'), (64, 0.3, 10.0, 'uniform'), (65, 0.05, 0.0, 'tanh'), (64, 2.0, 10.0, 'tanh')]


def _task(rng, n, d, ls, data, offset):
  x, _ = _hard_data(rng, d, ls, data, offset, n1=n, n2=64)
  w = rng.normal(size=(d, 1))
  y = np.sin((x - offset) @ w) + 0.1 * rng.normal(size=(n, 1))
  return x, y.astype(np.float32)


@pytest.mark.parametrize('d,scale,offset,data', HARD)
@pytest.mark.parametrize('kname', KERNELS)
def test_fp32_nll_and_grad_blocked_path(gpu_ctx, kname, d, scale, offset, data):
  """The blocked objective (n > 128: the batched Gram of objective.hip) against the fp64 oracle, and at n <= 128 the blocked
  evaluation (small_fused = 0) against the single-workgroup one (small.hip, direct form)."""
  _, _, defs, _, _, kernel, mean, objectives, utils = _native()
  rng = np.random.default_rng([d, int(scale * 100), int(offset), len(kname)])
  ls = _lengthscales(rng, scale, d)
  model, pn, po = _params(ls)
  kn, ko = getattr(kernel, kname), getattr(o, kname)
  x, y = _task(rng, 300, d, ls, data, offset)
  xs, ys = _task(rng, 120, d, ls, data, offset)
  ds = {0: defs.SubDataset(x, y), 1: defs.SubDataset(x[:170], y[:170])}
  dso = {k: o.SubDataset(v.x.astype(np.float64), v.y.astype(np.float64)) for k, v in ds.items()}
  v, g = objectives.nll_value_and_grad(mean.constant, kn, pn, ds, utils.DEFAULT_WARP_FUNC)
  vo, go = o.nll_value_and_grad(o.constant, ko, po, dso, WFO)
  assert np.isfinite(v) and abs(v - vo) <= 2e-4 * abs(vo), (v, vo)
  helpers.assert_grad_close(g, go, FP32_GRAD_TOL, label='nll blocked %s d=%d ls=%g' % (kname, d, scale))
  dss = {0: defs.SubDataset(xs, ys)}
  dsso = {0: o.SubDataset(xs.astype(np.float64), ys.astype(np.float64))}
  vso = o.neg_log_marginal_likelihood(o.constant, ko, po, dsso, WFO)
  v_small = objectives.neg_log_marginal_likelihood(mean.constant, kn, pn, dss, utils.DEFAULT_WARP_FUNC)
  try:
    gpu_ctx.set_option('small_fused', 0)
    v_blocked = objectives.neg_log_marginal_likelihood(mean.constant, kn, pn, dss, utils.DEFAULT_WARP_FUNC)
  finally:
    gpu_ctx.set_option('small_fused', 1)
  assert abs(v_small - vso) <= 2e-4 * abs(vso) and abs(v_blocked - vso) <= 2e-4 * abs(vso), (v_small, v_blocked, vso)
  assert abs(v_blocked - v_small) <= 2e-4 * abs(vso), (v_blocked, v_small)


@pytest.mark.parametrize('d,scale,offset,data', HARD)
@pytest.mark.parametrize('kname', KERNELS)
def test_fp32_predict_at_training_points_one_and_two_buffers(gpu_ctx, kname, d, scale, offset, data):
  """gp.predict through the factor cache, at the training inputs and at near duplicates of them: M below the posterior chunk
  (one buffer, the cross Gram on the matrix cores) and above it (two buffers, direct-form cross Gram) agree with each other and
  with the oracle; the prior's full covariance (no observations) too."""
  _, _, _, _, gp, kernel, mean, _, utils = _native()
  rng = np.random.default_rng([d, int(scale * 100), int(offset), len(kname), 7])
  ls = _lengthscales(rng, scale, d)
  model, pn, po = _params(ls)
  kn, ko = getattr(kernel, kname), getattr(o, kname)
  x, y = _task(rng, 200, d, ls, data, offset)
  xq = np.concatenate([x[:100], x[100:200] + (1e-3 * ls * rng.normal(size=(100, d))).astype(np.float32)]).astype(np.float32)
  xd, yd, xqd = x.astype(np.float64), y.astype(np.float64), xq.astype(np.float64)
  muo, varo = o.predict(o.constant, ko, po, xd, yd, xqd, WFO)
  vscale = np.max(np.abs(varo)) + _sv(model) * 1e-3
  outs = []
  try:
    for chunk in (8192, 128):   # 200 candidates: one chunk / two chunks in flight
      gpu_ctx.set_option('post_chunk', chunk)
      mu, var = gp.predict(mean.constant, kn, pn, x, y, xq, utils.DEFAULT_WARP_FUNC)
      assert np.all(np.isfinite(mu)) and np.all(np.isfinite(var))
      assert helpers.rel_err(mu, muo) < 2e-4, chunk
      assert np.max(np.abs(var - varo)) <= 5e-3 * vscale, chunk
      outs.append((mu, var))
  finally:
    gpu_ctx.set_option('post_chunk', 8192)
  assert helpers.rel_err(outs[0][0], outs[1][0]) < 2e-4
  assert np.max(np.abs(outs[0][1] - outs[1][1])) <= 5e-3 * vscale
  # the prior branch with full_cov: the Gram of the queries themselves
  _, covo = o.predict(o.constant, ko, po, np.zeros((0, d)), np.zeros((0, 1)), xqd, WFO, full_cov=True)
  _, cov = gp.predict(mean.constant, kn, pn, np.zeros((0, d), np.float32), np.zeros((0, 1), np.float32), xq, utils.DEFAULT_WARP_FUNC,
                      full_cov=True)
  assert np.array_equal(cov, cov.T)
  assert np.max(np.abs(cov - covo)) <= GRAM_TOL * _sv(model)


def test_fp32_hgp_samples_with_lengthscales_ten_times_apart(gpu_ctx):
  """The batched Gram of S parameter samples (cache.hip, model_stride 1) when the samples' length-scales differ by 10x, on
  offset inputs with duplicates: every sample's UCB against the oracle."""
  _, _, defs, acfun, gp, kernel, mean, _, utils = _native()
  rng = np.random.default_rng(41)
  d = 64
  base = _lengthscales(rng, 1.0, d)
  samples = [_params(base * f, sv=0.5 + 0.2 * i)[0] for i, f in enumerate((0.1, 0.3, 1.0))]
  x, y = _task(rng, 150, d, 0.1 * base, 'tanh', 10.0)
  xq = np.concatenate([x[:10], _rows(rng, 10, d, 'tanh', 10.0).astype(np.float32)]).astype(np.float32)
  hgp = gp.HGP({0: defs.SubDataset(x, y)}, mean.constant, kernel.squared_exponential, defs.GPParams(model=samples[0], samples=samples),
               utils.DEFAULT_WARP_FUNC)
  vals = acfun.hgp_sample_values(hgp, 0, xq, 2, 3.0)
  assert vals.dtype == np.float32 and np.all(np.isfinite(vals))
  dso = {0: o.SubDataset(x.astype(np.float64), y.astype(np.float64))}
  for s_, smp in enumerate(samples):
    po = o.GPParams(model={k_: np.asarray(v_, dtype=np.float64) for k_, v_ in smp.items()})
    mu, var = o.predict(o.constant, o.squared_exponential, po, x.astype(np.float64), y.astype(np.float64), xq.astype(np.float64), WFO)
    mu, var = o.gp_predict_postprocess(po, dso, mu, var, WFO, False, True, True)
    assert helpers.rel_err(vals[s_], o.ucb_sub(mu, np.sqrt(var), 3.0)) < 5e-3, s_


@pytest.mark.parametrize('feats', [(16, 32), (16, 64)])
def test_fp32_mlp_kernel_with_wide_last_layer(gpu_ctx, feats):
  """An MLP kernel whose last layer has 32 / 64 features reaches the matrix-core Gram (helpers.MLP_FEATURES does not): Gram and
  NLL value and gradient against the oracle, with small output length-scales."""
  _, _, defs, _, _, kernel, mean, objectives, utils = _native()
  rng = np.random.default_rng(feats[-1])
  d = 6
  ls = _lengthscales(rng, 0.3, feats[-1])
  model = _params(ls)[0]
  fin, mlp = d, {}
  for l, f in enumerate(feats):
    mlp[f'Dense_{l}'] = {'kernel': (rng.normal(size=(fin, f)) * 0.7).astype(np.float32), 'bias': (rng.normal(size=f) * 0.1).astype(np.float32)}
    fin = f
  model['mlp_params'] = mlp
  cfg = {'mlp_features': feats}
  pn = defs.GPParams(model=model, config=dict(cfg))
  po = o.GPParams(model=helpers.unflatten_like(model, helpers.flatten(model)), config=dict(cfg))
  x, y = _task(rng, 200, d, 0.05, 'uniform', 0.0)
  xd = x.astype(np.float64)
  g = kernel.matern52_mlp(pn, x, warp_func=utils.DEFAULT_WARP_FUNC)
  assert np.max(np.abs(g - o.matern52_mlp(po, xd, warp_func=WFO))) <= GRAM_TOL * _sv(model)
  ds = {0: defs.SubDataset(x, y)}
  v, gr = objectives.nll_value_and_grad(mean.constant, kernel.matern52_mlp, pn, ds, utils.DEFAULT_WARP_FUNC)
  vo, go = o.nll_value_and_grad(o.constant, o.matern52_mlp, po, {0: o.SubDataset(xd, y.astype(np.float64))}, WFO)
  assert abs(v - vo) <= 2e-4 * abs(vo), (v, vo)
  helpers.assert_grad_close(gr, go, FP32_GRAD_TOL, label='nll mlp %s' % (feats,))


# ---- (c) close to not positive definite -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('kname', KERNELS)
def test_fp32_near_duplicates_small_noise_nll_stays_finite(gpu_ctx, direct_ctx, kname):
  """Near duplicates and a small noise variance: where the fp64 oracle and the fp32 direct form factor and give a finite NLL, the
  default fp32 path does too (a NaN is what the expansion's absolute error in u can cause), within the fp32 tolerance."""
  _, _, defs, _, _, kernel, mean, objectives, utils = _native()
  rng = np.random.default_rng(len(kname))
  d = 64
  ls = _lengthscales(rng, 0.3, d)
  model, pn, po = _params(ls, sv=1.0, noise=1e-3)
  kn, ko = getattr(kernel, kname), getattr(o, kname)
  x, y = _task(rng, 300, d, ls, 'tanh', 10.0)
  ds = {0: defs.SubDataset(x, y)}
  vo = o.neg_log_marginal_likelihood(o.constant, ko, po, {0: o.SubDataset(x.astype(np.float64), y.astype(np.float64))}, WFO)
  assert np.isfinite(vo)
  dev = objectives.DeviceDataset(ds, ctx=direct_ctx)
  try:
    vd = objectives.neg_log_marginal_likelihood(mean.constant, kn, pn, dev, utils.DEFAULT_WARP_FUNC)
  finally:
    dev.close()
  assert np.isfinite(vd), 'precondition: the direct form factors this data'
  v = objectives.neg_log_marginal_likelihood(mean.constant, kn, pn, ds, utils.DEFAULT_WARP_FUNC)
  _log('0 tol=nllcond %s nll rel. error vs fp64: default %.3e direct %.3e' % (kname, abs(v - vo) / abs(vo), abs(vd - vo) / abs(vo)))
  assert np.isfinite(v)
  assert abs(v - vo) <= max(2e-4, 2 * abs(vd - vo) / abs(vo)) * abs(vo), (v, vd, vo)


# ---- (d) the gram_mfma setting belongs to one context -------------------------------------------------------------------------------
def test_gram_mfma_setting_does_not_leak_between_contexts(gpu_ctx):
  nat, _, _, _, _, kernel, _, _, _ = _native()
  rng = np.random.default_rng(5)
  d = 64
  ls = _lengthscales(rng, 2.0, d)
  x1, x2 = _hard_data(rng, d, ls, 'tanh', 0.0)
  pn = _params(ls)[1]
  before = _gram(gpu_ctx, kernel.matern52, pn, x1, x2)
  other = nat.Context(gpu_ctx.device)
  try:
    other.set_option('gram_mfma', 0)
    direct = _gram(other, kernel.matern52, pn, x1, x2)
    after = _gram(gpu_ctx, kernel.matern52, pn, x1, x2)
  finally:
    other.close()
  assert np.array_equal(before, after)
  assert not np.array_equal(before, direct)   # the two contexts did take different forms
