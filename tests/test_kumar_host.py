"""Kumaraswamy input-warped kernels (*_kumar): host-side pieces that need no device -- the Python surface, the ABI structs and
gradient layout, the rejections that happen before any device work, and the NumPy derivatives the GPU tests rely on."""
import ctypes as C

import numpy as np
import pytest

import kumar_oracle as ko

BASES = ['squared_exponential', 'matern32', 'matern52', 'dot_product']


@pytest.mark.parametrize('base', BASES)
def test_kumar_kernels_exist_with_the_base_name(base):
  from hyperbo_amd.gp_utils import kernel
  k = getattr(kernel, base + '_kumar')
  assert k.__name__ == base and 'mlp' not in k.__name__   # functools.wraps in the reference
  assert k.uses_kumar and not k.uses_mlp
  assert k.kernel_id == getattr(kernel, base).kernel_id
  assert not getattr(kernel, base).uses_kumar


def test_model_kumar_struct_size():
  from hyperbo_amd import _native as nat
  assert C.sizeof(nat.ModelKumar) == C.sizeof(nat.Model) + 16
  assert nat.WARP_KUMAR == 1 and nat.WARP_NONE == 0
  assert C.sizeof(nat.Model) == 264 and C.sizeof(nat.GradLayout) == 100   # unchanged


def _kumar_model(d=16, mean_id=None, kernel_id=0, warp=1, mlp=False):
  from hyperbo_amd import _native as nat
  ls = np.ones(d); a = np.ones(d); b = np.ones(d)
  mk = nat.ModelKumar()
  m = mk.base
  m.kernel_id, m.mean_id, m.dtype, m.input_dim = kernel_id, nat.MEAN_CONSTANT if mean_id is None else mean_id, nat.F64, d
  m.n_lengthscale = d; m.lengthscale = nat.ptr(ls).value; m.input_warp = warp
  if mlp:
    m.kernel_uses_mlp = 1; m.n_layers = 1; m.features[0] = 4
  mk.kumar_a = nat.ptr(a).value; mk.kumar_b = nat.ptr(b).value
  return mk, (ls, a, b)


def test_grad_layout_of_a_kumar_model():
  from hyperbo_amd import _native as nat
  d = 16
  mk, keep = _kumar_model(d)
  plain = nat.Model(); C.memmove(C.byref(plain), C.byref(mk.base), C.sizeof(nat.Model)); plain.input_warp = 0
  lp, lk = nat.GradLayout(), nat.GradLayout()
  assert nat.lib().hbo_grad_layout_of(C.byref(plain), C.byref(lp)) == nat.HBO_OK
  ref = C.cast(C.pointer(mk), C.POINTER(nat.Model))
  assert nat.lib().hbo_grad_layout_of(ref, C.byref(lk)) == nat.HBO_OK
  assert lp.total == d + 3   # lengthscale, signal, noise, constant
  assert lk.total == lp.total + 2 * d
  for f in ('lengthscale', 'signal_variance', 'noise_variance', 'constant'):
    assert getattr(lk, f) == getattr(lp, f)
  ao, bo = C.c_int32(), C.c_int32()
  assert nat.lib().hbo_grad_layout_kumar_of(ref, C.byref(ao), C.byref(bo)) == nat.HBO_OK
  assert (ao.value, bo.value) == (lk.total - 2 * d, lk.total - d)
  assert nat.lib().hbo_grad_layout_kumar_of(C.byref(plain), C.byref(ao), C.byref(bo)) == nat.HBO_OK
  assert (ao.value, bo.value) == (-1, -1)


def test_kumar_with_mlp_and_unknown_warp_are_rejected_before_device_work():
  from hyperbo_amd import _native as nat
  lay = nat.GradLayout()
  mk, keep = _kumar_model(mlp=True)
  assert nat.lib().hbo_grad_layout_of(C.cast(C.pointer(mk), C.POINTER(nat.Model)), C.byref(lay)) == nat.HBO_ERR_UNSUPPORTED
  assert b'MLP' in nat.lib().hbo_last_error(None)
  mk, keep = _kumar_model(warp=7)
  assert nat.lib().hbo_grad_layout_of(C.cast(C.pointer(mk), C.POINTER(nat.Model)), C.byref(lay)) == nat.HBO_ERR_UNSUPPORTED
  mk, keep = _kumar_model()
  mk.kumar_b = None
  assert nat.lib().hbo_grad_layout_of(C.cast(C.pointer(mk), C.POINTER(nat.Model)), C.byref(lay)) == nat.HBO_ERR_ARG


def test_built_model_rejections_and_missing_kumar_params():
  from hyperbo_amd import _model, _native as nat
  from hyperbo_amd.basics import definitions as defs
  from hyperbo_amd.gp_utils import kernel, mean, utils
  model = {'lengthscale': np.zeros(3), 'signal_variance': 0.0, 'noise_variance': -2.0, 'constant': 0.0}
  with pytest.raises(ValueError, match='init_kumar_warp_with_shape'):
    _model.BuiltModel(mean.constant, kernel.matern52_kumar, defs.GPParams(model=dict(model)), utils.DEFAULT_WARP_FUNC, np.float64, 3)
  p = defs.GPParams(model=dict(model))
  kernel.init_kumar_warp_with_shape(None, p, (10, 3))
  bm = _model.BuiltModel(mean.constant, kernel.matern52_kumar, p, utils.DEFAULT_WARP_FUNC, np.float64, 3)
  assert bm.struct.input_warp == nat.WARP_KUMAR and bm.layout.total == 3 + 3 + 6
  # the chain rule of squareplus on the 2 D leaves
  p.model['kumar_params'] = {'a': np.array([-1.0, 0.0, 2.0]), 'b': np.array([0.5, -0.5, 1.5])}
  bm = _model.BuiltModel(mean.constant, kernel.matern52_kumar, p, utils.DEFAULT_WARP_FUNC, np.float64, 3)
  flat = np.arange(bm.layout.total, dtype=np.float64)
  g = bm.unflatten_grad(flat)
  ao, bo = bm.kumar_offsets
  np.testing.assert_allclose(g['kumar_params']['a'], flat[ao:ao + 3] * ko.squareplus_grad(p.model['kumar_params']['a']), rtol=1e-15)
  np.testing.assert_allclose(g['kumar_params']['b'], flat[bo:bo + 3] * ko.squareplus_grad(p.model['kumar_params']['b']), rtol=1e-15)


def test_init_kumar_warp_with_shape_gives_zeros():
  from hyperbo_amd.basics import definitions as defs
  from hyperbo_amd.gp_utils import kernel
  p = defs.GPParams(model={})
  kernel.init_kumar_warp_with_shape(None, p, (7, 16))
  kp = p.model['kumar_params']
  assert set(kp) == {'a', 'b'}
  for v in kp.values():
    assert np.shape(v) == (16,) and not np.any(v)
  np.testing.assert_array_equal(ko.squareplus(kp['a']), np.ones(16))   # identity warp


def test_numpy_derivatives_against_central_differences():
  rng = np.random.default_rng(0)
  x = rng.uniform(0.02, 0.98, size=200)
  a = ko.squareplus(rng.uniform(-1.5, 1.5, size=200)); b = ko.squareplus(rng.uniform(-1.5, 1.5, size=200))
  w = lambda x_, a_, b_: 1.0 - (1.0 - x_ ** a_) ** b_
  h = 1e-6
  da, db = ko.dw_dab(x, a, b)
  np.testing.assert_allclose(da, (w(x, a + h, b) - w(x, a - h, b)) / (2 * h), rtol=1e-6, atol=1e-9)
  np.testing.assert_allclose(db, (w(x, a, b + h) - w(x, a, b - h)) / (2 * h), rtol=1e-6, atol=1e-9)
  np.testing.assert_allclose(ko.dw_dx(x, a, b), (w(x + h, a, b) - w(x - h, a, b)) / (2 * h), rtol=1e-6, atol=1e-9)
  da0, db0 = ko.dw_dab(np.array([0.0, 1.0]), np.array([0.7, 1.3]), np.array([0.6, 2.0]))
  assert np.all(da0 == 0) and np.all(db0 == 0)
