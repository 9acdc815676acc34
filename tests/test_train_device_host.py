"""config['adam_on_device'] (hbo_train_adam), the parts that need no device: the leaf map of every model family restated in NumPy
against BuiltModel (warped fields and the chain rule of unflatten_grad), the eligibility rules of the Python driver and the
argument checks hbo_train_adam makes before any HIP call."""
import ctypes as C

import numpy as np
import pytest

import train_device_cases as cases


def _mods():
  from hyperbo_amd import _model, _native as nat
  from hyperbo_amd.basics import definitions as defs, lbfgs
  from hyperbo_amd.gp_utils import gp, objectives, utils
  return _model, nat, defs, lbfgs, gp, objectives, utils


def _built(kname, mname, dtype=np.float64, leaf_dtype=np.float64):
  _model, nat, defs, lbfgs, gp, objectives, utils = _mods()
  mean_func, cov_func = cases.funcs(kname, mname)
  model = cases.model_of(kname, mname, dtype=leaf_dtype)
  params = defs.GPParams(model=model, config={})
  bm = _model.BuiltModel(mean_func, cov_func, params, utils.DEFAULT_WARP_FUNC, dtype, cases.D)
  return bm, model


def _np_warp(code, t):
  _model, nat, defs, lbfgs, gp, objectives, utils = _mods()
  return {nat.TRAIN_WARP_IDENTITY: lambda v: v, nat.TRAIN_WARP_SOFTPLUS: utils.softplus_warp,
          nat.TRAIN_WARP_SOFTPLUS_EPS: utils.DEFAULT_SOFTPLUS, nat.TRAIN_WARP_SQUAREPLUS: utils.squareplus_warp}[code](t)


def _np_slope(code, t):
  _model, nat, defs, lbfgs, gp, objectives, utils = _mods()
  fn = {nat.TRAIN_WARP_IDENTITY: utils.identity_warp, nat.TRAIN_WARP_SOFTPLUS: utils.softplus_warp,
        nat.TRAIN_WARP_SOFTPLUS_EPS: utils.DEFAULT_SOFTPLUS, nat.TRAIN_WARP_SQUAREPLUS: utils.squareplus_warp}[code]
  return utils.warp_derivative(fn, t)


def _apply_map(bm, model, leaves, P):
  """What adam_step_kernel writes, in NumPy: the scalar fields and the arrays (in the model dtype) of hbo_model."""
  _model, nat, defs, lbfgs, gp, objectives, utils = _mods()
  x, _ = lbfgs.tree_flatten(model)
  assert P == x.size
  s = bm.struct
  sc = {nat.TRAIN_SIGNAL_VARIANCE: s.signal_variance, nat.TRAIN_NOISE_VARIANCE: s.noise_variance, nat.TRAIN_CONSTANT: s.constant,
        nat.TRAIN_DOT_PROD_SIGMA: s.dot_prod_sigma, nat.TRAIN_DOT_PROD_BIAS: s.dot_prod_bias, nat.TRAIN_LINEAR_BIAS: s.linear_bias}
  arrays = {}
  for i in range(P):
    lf = leaves[i]
    xr = np.float64(np.float32(x[i])) if lf.round_f32 else x[i]
    w = float(_np_warp(lf.warp, np.asarray(xr)))
    if lf.target in sc:
      sc[lf.target] = w
    elif lf.target != nat.TRAIN_NONE:
      arrays.setdefault((lf.target, lf.layer), {})[lf.index] = w
  return sc, arrays


def _struct_arrays(bm):
  _model, nat, defs, lbfgs, gp, objectives, utils = _mods()
  s = bm.struct
  dt = np.float64 if s.dtype == nat.F64 else np.float32
  ctype = C.c_double if s.dtype == nat.F64 else C.c_float

  def read(ptr, n):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,)).astype(dt).copy()
  out = {}
  if s.kernel_id != nat.KERNEL_DOT:
    out[(nat.TRAIN_LENGTHSCALE, 0)] = read(s.lengthscale, s.n_lengthscale)
  if s.mean_id in (nat.MEAN_LINEAR, nat.MEAN_LINEAR_MLP):
    out[(nat.TRAIN_LINEAR_KERNEL, 0)] = read(s.linear_kernel, bm.mlp_out if s.mean_id == nat.MEAN_LINEAR_MLP else s.input_dim)
  for l, (ws, bs) in enumerate(bm.mlp_shapes):
    out[(nat.TRAIN_MLP_KERNEL, l)] = read(s.mlp_kernel[l], int(np.prod(ws)))
    out[(nat.TRAIN_MLP_BIAS, l)] = read(s.mlp_bias[l], int(np.prod(bs)))
  if bm.uses_kumar:
    out[(nat.TRAIN_KUMAR_A, 0)] = read(bm.kstruct.kumar_a, s.input_dim)
    out[(nat.TRAIN_KUMAR_B, 0)] = read(bm.kstruct.kumar_b, s.input_dim)
  return out


@pytest.mark.parametrize('kname,mname', cases.FAMILIES)
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_leaf_map_gives_the_fields_of_built_model(kname, mname, dtype):
  _model, nat, defs, lbfgs, gp, objectives, utils = _mods()
  bm, model = _built(kname, mname, dtype)
  leaves, P = _model.train_leaf_map(bm, model)
  sc, arrays = _apply_map(bm, model, leaves, P)
  s = bm.struct
  for tgt, val in sc.items():
    name = {nat.TRAIN_SIGNAL_VARIANCE: 'signal_variance', nat.TRAIN_NOISE_VARIANCE: 'noise_variance', nat.TRAIN_CONSTANT: 'constant',
            nat.TRAIN_DOT_PROD_SIGMA: 'dot_prod_sigma', nat.TRAIN_DOT_PROD_BIAS: 'dot_prod_bias', nat.TRAIN_LINEAR_BIAS: 'linear_bias'}[tgt]
    assert getattr(s, name) == val, name
  got = _struct_arrays(bm)
  assert set(arrays) == set(got)
  dt = np.float64 if dtype == np.float64 else np.float32
  for key, vals in arrays.items():
    assert sorted(vals) == list(range(got[key].size)), key
    mine = np.array([vals[i] for i in range(got[key].size)]).astype(dt)
    np.testing.assert_array_equal(mine, got[key], err_msg=str(key))


def test_leaf_map_marks_float32_leaves_and_unread_leaves():
  _model, nat, defs, lbfgs, gp, objectives, utils = _mods()
  bm, model = _built('dot_product', 'zero', leaf_dtype=np.float32)
  model['unused'] = np.zeros(3)
  leaves, P = _model.train_leaf_map(bm, model)
  x, _ = lbfgs.tree_flatten(model)
  assert P == x.size
  rows = [(leaves[i].target, leaves[i].round_f32) for i in range(P)]
  assert (nat.TRAIN_NOISE_VARIANCE, 1) in rows
  assert rows.count((nat.TRAIN_NONE, 1)) == 1    # signal_variance: the dot-product kernel does not read it
  assert rows.count((nat.TRAIN_NONE, 0)) == 3    # 'unused'


@pytest.mark.parametrize('kname,mname', cases.FAMILIES)
def test_chained_gradient_equals_unflatten_grad(kname, mname):
  _model, nat, defs, lbfgs, gp, objectives, utils = _mods()
  bm, model = _built(kname, mname)
  leaves, P = _model.train_leaf_map(bm, model)
  x, _ = lbfgs.tree_flatten(model)
  rng = np.random.default_rng(3)
  flat = rng.normal(size=bm.layout.total)
  want, _ = lbfgs.tree_flatten(bm.unflatten_grad(flat))
  lay = bm.layout
  ka, kb = bm.kumar_offsets if bm.uses_kumar else (-1, -1)
  got = np.zeros(P)
  for i in range(P):
    lf = leaves[i]
    base = {nat.TRAIN_LENGTHSCALE: lay.lengthscale, nat.TRAIN_SIGNAL_VARIANCE: lay.signal_variance,
            nat.TRAIN_NOISE_VARIANCE: lay.noise_variance, nat.TRAIN_CONSTANT: lay.constant, nat.TRAIN_DOT_PROD_SIGMA: lay.dot_prod_sigma,
            nat.TRAIN_DOT_PROD_BIAS: lay.dot_prod_bias, nat.TRAIN_LINEAR_KERNEL: lay.linear_kernel, nat.TRAIN_LINEAR_BIAS: lay.linear_bias,
            nat.TRAIN_MLP_KERNEL: lay.mlp_kernel[lf.layer], nat.TRAIN_MLP_BIAS: lay.mlp_bias[lf.layer], nat.TRAIN_KUMAR_A: ka,
            nat.TRAIN_KUMAR_B: kb}.get(lf.target, -1)
    if lf.target == nat.TRAIN_NONE:
      continue
    assert base >= 0
    got[i] = flat[base + lf.index] * float(_np_slope(lf.warp, np.asarray(x[i])))
  np.testing.assert_array_equal(got, want)


def _eligibility_case(**over):
  _model, nat, defs, lbfgs, gp, objectives, utils = _mods()
  mean_func, cov_func = cases.funcs('squared_exponential', 'constant')
  config = {'method': 'adam', 'batch_size': 100, 'max_training_step': 5, 'learning_rate': 1e-3, 'objective': objectives.nll,
            'adam_on_device': True}
  config.update(over.pop('config', {}))
  model = cases.model_of('squared_exponential', 'constant')
  warp = dict(utils.DEFAULT_WARP_FUNC)
  warp.update(over.pop('warp', {}))
  sizes = over.pop('sizes', [60, 80])
  return gp.GP(cases.dataset(sizes), mean_func, cov_func, defs.GPParams(model=model, config=config), warp)


@pytest.mark.parametrize('case,match', [
    ({'config': {'objective': 'ekl'}}, 'not obj.nll'),
    ({'config': {'priors': {}}}, 'priors'),
    ({'warp': {'noise_variance': np.exp}}, 'closed set'),
    ({'config': {'comm': object()}}, 'comm'),
    ({'sizes': [60, 129], 'config': {'batch_size': 200}}, '> 128'),
    ({'sizes': [60, 400], 'config': {'batch_size': 200}}, '> 128'),
])
def test_ineligible_configurations_raise(case, match):
  g = _eligibility_case(**case)
  if isinstance(g.params.config['objective'], str):
    from hyperbo_amd.gp_utils import objectives
    g.params.config['objective'] = getattr(objectives, g.params.config['objective'])
  with pytest.raises(ValueError, match=match):
    g.train(key=0)


def test_eligibility_accepts_the_fused_regime():
  _model, nat, defs, lbfgs, gp, objectives, utils = _mods()
  g = _eligibility_case(sizes=[60, 400])   # batch_size 100: the 400-point task is sub-sampled to 100
  assert gp._adam_on_device_unmet(g.mean_func, g.cov_func, g.params, g.dataset, g.warp_func, objectives.nll) is None


def _train_args(nat, P=3, steps=2):
  leaves = (nat.TrainLeaf * P)()
  for i in range(P):
    leaves[i].target = nat.TRAIN_NONE
  arr = lambda n: np.zeros(n)
  return dict(leaves=leaves, P=P, x=arr(P), m=arr(P), v=arr(P), b1=arr(steps), b2=arr(steps), steps=steps, losses=arr(steps))


def _call(nat, model, a, ds=None, counts=None, rows=None, done=True):
  d = C.c_int32(0)
  return nat.lib().hbo_train_adam(None, C.byref(model) if model is not None else None, ds, a['leaves'], a['P'], nat.ptr(a['x']),
                                  nat.ptr(a['m']), nat.ptr(a['v']), nat.ptr(a['b1']), nat.ptr(a['b2']), a['steps'], 1e-3, 0.9, 0.999,
                                  1e-8, counts, rows, nat.ptr(a['losses']), None, C.byref(d) if done else None)


def test_train_adam_rejects_bad_arguments_before_any_device_call():
  _model, nat, defs, lbfgs, gp, objectives, utils = _mods()
  bm, model = _built('squared_exponential', 'constant')
  m = bm.struct
  err = lambda: (nat.lib().hbo_last_error(None) or b'').decode()

  def expect(rc, text):
    assert rc == nat.HBO_ERR_ARG, (rc, err())
    assert text in err(), err()

  expect(_call(nat, None, _train_args(nat)), 'model is null')
  a = _train_args(nat); a['P'] = 0
  expect(_call(nat, m, a), 'P must be positive')
  a = _train_args(nat); a['steps'] = 0
  expect(_call(nat, m, a), 'steps must be positive')
  expect(_call(nat, m, _train_args(nat), done=False), 'null array argument')
  expect(_call(nat, m, _train_args(nat), counts=nat.ptr(np.zeros(2, dtype=np.int64))), 'both given or both null')
  for field, val, text in (('warp', 7, 'unknown warp'), ('target', 40, 'unknown target'), ('round_f32', 2, 'round_f32'),
                           ('index', 9, 'outside its target')):
    a = _train_args(nat)
    if field == 'index':
      a['leaves'][0].target = nat.TRAIN_LENGTHSCALE
    setattr(a['leaves'][0], field, val)
    expect(_call(nat, m, a), text)
  a = _train_args(nat)
  a['leaves'][1].target = nat.TRAIN_DOT_PROD_SIGMA   # an SE model has no dot-product sigma
  expect(_call(nat, m, a), 'does not read its target')
  a = _train_args(nat)
  a['leaves'][1].target = nat.TRAIN_MLP_KERNEL       # nor an MLP
  expect(_call(nat, m, a), 'outside its target')
  # every leaf valid: the next thing missing is the dataset, then the context
  a = _train_args(nat)
  a['leaves'][0].target = nat.TRAIN_NOISE_VARIANCE
  a['leaves'][0].warp = nat.TRAIN_WARP_SOFTPLUS_EPS
  expect(_call(nat, m, a), 'dataset is null')
