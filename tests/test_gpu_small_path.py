"""The single-workgroup evaluation (csrc/small.hip) -- the whole NLL and its gradient in one workgroup per task, taken whenever every
task of a batch has n <= 128: the reference's training regime, the fused NLL of the slice sampler and every step of the device Adam
loop.  Its gradient is checked PER LEAF (helpers.assert_grad_close) against the fp64 oracle on the same (fp32-rounded) inputs and,
in fp64, against the blocked pipeline on the same batch (hbo_tune small_fused = 0): the kernel x basis x mean registry on one
ragged batch, feature widths on both sides of the 16-feature chunks of the length-scale gradient, Kumaraswamy warps wider than a
chunk, and the training batch shape.  Every evaluation runs with profiling on and asserts that small_eval ran and potrf did not
(a runtime that quietly takes the blocked path fails here instead of passing).  Run with `-m gpu`."""
import numpy as np
import pytest

import helpers
import kumar_oracle as ko
from oracle import hyperbo_oracle as o

pytestmark = pytest.mark.gpu
WFO = o.DEFAULT_WARP_FUNC
# Per-leaf bounds (helpers.assert_grad_close) and the worst leaf measured on the MI355X over this file, as a fraction of its bound:
FP64_GRAD_TOL = 1e-10      # fp64 against the oracle, as tests/test_gpu_parity.py; worst 3.1e-3
FP32_GRAD_TOL = 2.5e-3     # fp32 against the fp64 oracle on the fp32-rounded inputs; worst 9.4e-2
BLOCKED_GRAD_TOL = 1e-11   # fp64 against the blocked pipeline (another summation order: rounding, not bits); worst 2.9e-2
FP64_VALUE_TOL = 1e-10     # relative, against the oracle
FP32_VALUE_TOL = 2e-4
BLOCKED_VALUE_TOL = 1e-12  # fp64, relative, against the blocked pipeline
STATIONARY = ['squared_exponential', 'matern32', 'matern52']


def _native():
  from hyperbo_amd.basics import definitions as defs
  from hyperbo_amd.gp_utils import kernel, mean, objectives, utils
  return defs, kernel, mean, objectives, utils


def _cast(tree, dtype):
  return {k: _cast(v, dtype) for k, v in tree.items()} if isinstance(tree, dict) else np.asarray(tree, dtype=dtype)


def _tols(dtype):
  return (FP64_VALUE_TOL, FP64_GRAD_TOL) if dtype == np.float64 else (FP32_VALUE_TOL, FP32_GRAD_TOL)


def _small(ctx, fn, *stages):
  """fn() with profiling on: the single-workgroup evaluation ran (with `stages`), the blocked pipeline did not."""
  ctx.profile_enable(1)
  try:
    out = fn()
    seen = ctx.profile_get()
  finally:
    ctx.profile_enable(0)
  assert 'small_eval' in seen and 'potrf' not in seen, sorted(seen)
  for s in stages:
    assert s in seen, (s, sorted(seen))
  return out


def _blocked(ctx, fn):
  """fn() on the blocked pipeline (small_fused = 0) of the same batch."""
  ctx.set_option('small_fused', 0)
  ctx.profile_enable(1)
  try:
    out = fn()
    seen = ctx.profile_get()
  finally:
    ctx.set_option('small_fused', 1)
    ctx.profile_enable(0)
  assert 'potrf' in seen and 'small_eval' not in seen, sorted(seen)
  return out


def _backward_stages(mlp_kernel, mname):
  return ('mlp_backward',) if mlp_kernel or mname == 'linear_mlp' else ()


def _check_nll_and_grad(ctx, mn, kn, pn, dsn, mo, ko_, po, dso, dtype, label, stages=(), blocked=None, exclude=True):
  """Value, every task's value (return_key2nll) and the gradient per leaf of the single-workgroup evaluation against the oracle;
  with `blocked` (fp64) the gradient per leaf and the value against the blocked pipeline too."""
  objectives, utils = _native()[3:]
  wf = utils.DEFAULT_WARP_FUNC
  vtol, gtol = _tols(dtype)
  v, g = _small(ctx, lambda: objectives.nll_value_and_grad(mn, kn, pn, dsn, wf, exclude_aligned=exclude), *stages)
  t, k2n = _small(ctx, lambda: objectives.neg_log_marginal_likelihood(mn, kn, pn, dsn, wf, exclude_aligned=exclude, return_key2nll=True))
  vo, go = o.nll_value_and_grad(mo, ko_, po, dso, WFO, exclude_aligned=exclude)
  to, k2o = o.neg_log_marginal_likelihood(mo, ko_, po, dso, WFO, exclude_aligned=exclude, return_key2nll=True)
  assert np.isfinite(v) and abs(v - vo) <= vtol * max(abs(vo), 1.0), (label, v, vo)
  assert abs(t - to) <= vtol * max(abs(to), 1.0), (label, t, to)
  assert sorted(k2n, key=str) == sorted(k2o, key=str), (label, sorted(k2n, key=str), sorted(k2o, key=str))
  for k in k2o:
    assert abs(k2n[k] - k2o[k]) <= vtol * max(abs(k2o[k]), 1.0), (label, k, k2n[k], k2o[k])
  helpers.assert_grad_close(g, go, gtol, label=label + ' vs oracle')
  if blocked:
    vb, gb = _blocked(ctx, lambda: objectives.nll_value_and_grad(mn, kn, pn, dsn, wf, exclude_aligned=exclude))
    assert abs(v - vb) <= BLOCKED_VALUE_TOL * max(abs(vb), 1.0), (label, v, vb)
    helpers.assert_grad_close(g, gb, BLOCKED_GRAD_TOL, label=label + ' vs blocked')
  return g, go


def _batch(rng, sizes, d, dtype, multi_y=None, aligned=None):
  """Host datasets for the device (dtype) and the oracle (the same values in fp64)."""
  defs = _native()[0]
  dso, dsn = {}, {}
  for n in sizes:
    x, y = helpers.synthetic_task(rng, n, d, m=(3 if n == multi_y else 1), dtype=dtype)
    al = 1 if n == aligned else None
    dso[n] = o.SubDataset(x.astype(np.float64), y.astype(np.float64), al)
    dsn[n] = defs.SubDataset(x, y, al)
  return dso, dsn


# ---- 1. the registry on one ragged batch ----------------------------------------------------------------------------------------
REGISTRY_SIZES = [1, 2, 15, 16, 17, 33, 64, 100, 127, 128]


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['fp64', 'fp32'])
@pytest.mark.parametrize('mname', helpers.MEANS)
@pytest.mark.parametrize('mlp', [False, True], ids=['plain', 'mlp'])
@pytest.mark.parametrize('kname', helpers.KERNELS)
def test_registry_per_leaf_vs_oracle_and_blocked(gpu_ctx, kname, mlp, mname, dtype):
  """Every kernel x {plain, MLP basis} x mean: one batch across the 16-row leaf boundaries up to the 128-point limit, a task with
  three columns of y (100 points) and an aligned task (33 points), with and without exclude_aligned."""
  defs, kernel, mean, _, _ = _native()
  rng = np.random.default_rng([helpers.KERNELS.index(kname), int(mlp), helpers.MEANS.index(mname), int(dtype == np.float32)])
  d = 3
  model = _cast(helpers.make_model(rng, mname, mlp, d), dtype)
  cfg = {'mlp_features': helpers.MLP_FEATURES}
  po, pn = o.GPParams(model=_cast(model, np.float64), config=dict(cfg)), defs.GPParams(model=model, config=dict(cfg))
  dso, dsn = _batch(rng, REGISTRY_SIZES, d, dtype, multi_y=100, aligned=33)
  suffix = '_mlp' if mlp else ''
  kn, ko_ = getattr(kernel, kname + suffix), getattr(o, kname + suffix)
  mn, mo = getattr(mean, mname), getattr(o, mname)
  for exclude in (True, False):
    _check_nll_and_grad(gpu_ctx, mn, kn, pn, dsn, mo, ko_, po, dso, dtype, f'registry exclude_aligned={exclude}',
                        stages=_backward_stages(mlp, mname), blocked=dtype == np.float64, exclude=exclude)


# ---- 2. feature widths across the 16-feature chunks of the length-scale gradient ------------------------------------------------
WIDTH_SIZES = [128, 90, 33, 2]
WIDTHS = [15, 16, 17, 31, 32, 33, 64, 65, 256]   # 256: HBO_MAX_FEATURE_DIM


@pytest.mark.parametrize('ls', ['ard', 'scalar'])
@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['fp64', 'fp32'])
@pytest.mark.parametrize('kname', STATIONARY)
@pytest.mark.parametrize('d', WIDTHS)
def test_input_width_per_leaf(gpu_ctx, d, kname, dtype, ls):
  """Plain inputs of d features, a linear mean on them (its d weights: the strided per-wave loop of the mean leaves).  fp32 is
  compared with the oracle only: from 32 features the blocked path takes the matrix-core Gram, this path the direct form."""
  defs, kernel, mean, _, _ = _native()
  rng = np.random.default_rng([d, STATIONARY.index(kname), int(dtype == np.float32), int(ls == 'scalar')])
  model = _cast({'lengthscale': helpers.lengthscale(rng, d, ls), 'signal_variance': helpers.inv_softplus(0.8),
                 'noise_variance': helpers.inv_softplus(0.1),
                 'linear_mean': {'kernel': rng.normal(size=(d, 1)) / np.sqrt(d), 'bias': rng.normal(size=1)}}, dtype)
  po, pn = o.GPParams(model=_cast(model, np.float64)), defs.GPParams(model=model)
  dso, dsn = _batch(rng, WIDTH_SIZES, d, dtype)
  g, _ = _check_nll_and_grad(gpu_ctx, mean.linear, getattr(kernel, kname), pn, dsn, o.linear, getattr(o, kname), po, dso, dtype,
                             f'width d={d} {ls}', blocked=dtype == np.float64)
  assert g['lengthscale'].shape == ((d,) if ls == 'ard' else (1,))


# (last layer, kernel, length-scale): the dot product at 33 features only -- it has no length-scale, its features' gradient is all
# grad_feat_kernel's
MLP_WIDTH_CASES = [(f, k, ls) for f in (17, 33, 64) for k in STATIONARY for ls in ('ard', 'scalar')] + [(33, 'dot_product', 'none')]


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['fp64', 'fp32'])
@pytest.mark.parametrize('flast,kname,ls', MLP_WIDTH_CASES)
def test_mlp_last_layer_width_per_leaf(gpu_ctx, flast, kname, ls, dtype):
  """MLP basis (5 -> 12 -> flast features) under the kernel and a linear_mlp mean: the length-scale leaves come out of the
  chunked sum of small.hip, the feature gradient out of grad_feat_kernel / grad_feat_mean into the MLP backward."""
  defs, kernel, mean, _, _ = _native()
  rng = np.random.default_rng([flast, (STATIONARY + ['dot_product']).index(kname), int(dtype == np.float32), int(ls == 'scalar'), 7])
  d, feats = 5, (12, flast)
  model = _cast(helpers.mlp_model(rng, d, feats, kname, ls), dtype)
  cfg = {'mlp_features': feats}
  po, pn = o.GPParams(model=_cast(model, np.float64), config=dict(cfg)), defs.GPParams(model=model, config=dict(cfg))
  dso, dsn = _batch(rng, WIDTH_SIZES, d, dtype)
  _check_nll_and_grad(gpu_ctx, mean.linear_mlp, getattr(kernel, kname + '_mlp'), pn, dsn, o.linear_mlp, getattr(o, kname + '_mlp'),
                      po, dso, dtype, f'mlp width {flast} {ls}', stages=('mlp_backward',), blocked=dtype == np.float64)


# ---- 3. Kumaraswamy warps wider than a chunk ------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [17, 40])
def test_se_kumar_per_leaf_fp64(gpu_ctx, d):
  """squared_exponential_kumar + constant mean on a batch of small tasks: every leaf, the a / b leaves included, against the oracle
  on the warped inputs and the analytic a / b gradient (as test_gpu_kumar.py at d = 6), and against the blocked pipeline."""
  defs, kernel, mean, objectives, utils = _native()
  rng = np.random.default_rng([d, 17])
  model = helpers.make_model(rng, 'constant', False, d)
  model['lengthscale'] = helpers.lengthscale(rng, d, 'ard')
  model['kumar_params'] = {'a': rng.uniform(-1.5, 1.5, size=d), 'b': rng.uniform(-1.5, 1.5, size=d)}
  dso = {}
  for n in (128, 100, 64, 17, 1):
    x = rng.uniform(size=(n, d))
    x.flat[::7] = 0.0
    x.flat[3::11] = 1.0
    dso[n] = o.SubDataset(x, np.sin(3 * rng.uniform(size=(n, 1))))
  dsn = {k: defs.SubDataset(v.x, v.y) for k, v in dso.items()}
  pn = defs.GPParams(model=model)
  wf = utils.DEFAULT_WARP_FUNC
  fn = lambda: objectives.nll_value_and_grad(mean.constant, kernel.squared_exponential_kumar, pn, dsn, wf)
  v, g = _small(gpu_ctx, fn, 'kumar_forward', 'kumar_backward')
  kp = model['kumar_params']
  warped = {k: o.SubDataset(ko.warp(s.x, kp['a'], kp['b']), s.y) for k, s in dso.items()}
  po = o.GPParams(model={k: v_ for k, v_ in model.items() if k != 'kumar_params'})
  vo, go = o.nll_value_and_grad(o.constant, o.squared_exponential, po, warped, WFO)
  ga, gb = ko.se_nll_ab_grad(model, dso)
  go['kumar_params'] = {'a': ga, 'b': gb}
  assert abs(v - vo) <= FP64_VALUE_TOL * abs(vo), (v, vo)
  helpers.assert_grad_close(g, go, FP64_GRAD_TOL, label=f'kumar d={d} vs oracle')
  vb, gb_ = _blocked(gpu_ctx, fn)
  assert abs(v - vb) <= BLOCKED_VALUE_TOL * abs(vb), (v, vb)
  helpers.assert_grad_close(g, gb_, BLOCKED_GRAD_TOL, label=f'kumar d={d} vs blocked')


# ---- 4. the training batch shape ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kname,mlp,mname,dtype', [('matern52', False, 'linear', np.float64),
                                                   ('squared_exponential', True, 'linear_mlp', np.float64),
                                                   ('matern32', False, 'constant', np.float32)],
                         ids=['matern52-linear-fp64', 'squared_exponential_mlp-linear_mlp-fp64', 'matern32-constant-fp32'])
def test_training_batch_shape(gpu_ctx, kname, mlp, mname, dtype):
  """64 tasks of 100 points (cfg 4's task count at the training batch size) with tasks of 1 and 2 points: the total, every task's
  value and the gradient per leaf against the oracle."""
  defs, kernel, mean, _, _ = _native()
  rng = np.random.default_rng([helpers.KERNELS.index(kname), int(mlp), helpers.MEANS.index(mname), 64])
  d = 4
  model = _cast(helpers.make_model(rng, mname, mlp, d), dtype)
  cfg = {'mlp_features': helpers.MLP_FEATURES}
  po, pn = o.GPParams(model=_cast(model, np.float64), config=dict(cfg)), defs.GPParams(model=model, config=dict(cfg))
  dso, dsn = {}, {}
  for k, n in enumerate([100] * 32 + [1] + [100] * 32 + [2]):
    x, y = helpers.synthetic_task(rng, n, d, dtype=dtype)
    dso[k] = o.SubDataset(x.astype(np.float64), y.astype(np.float64))
    dsn[k] = defs.SubDataset(x, y)
  suffix = '_mlp' if mlp else ''
  _check_nll_and_grad(gpu_ctx, getattr(mean, mname), getattr(kernel, kname + suffix), pn, dsn, getattr(o, mname),
                      getattr(o, kname + suffix), po, dso, dtype, 'batch 64 x 100', stages=_backward_stages(mlp, mname))
