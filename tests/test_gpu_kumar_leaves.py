"""The Kumaraswamy warp of csrc/kumar.hip on an MI355X (run with `-m gpu`) against tests/kumar_cases.py:

  * the element-wise kernels through the test hook hbo_probe_kumar_warp (include/hbo_tune.h: launch_kumar_forward in its gradient form,
    launch_kumar_chain_dx on a cotangent of ones), one call per dtype over the [211, 36] grid: w, dw/da, dw/db, dw/dx per element
    against mpmath within REL_FACTOR x the NumPy restatement's own error + FLOOR_C eps_T S, and the exact identities (w in {0, 1} and
    dw/da = dw/db = 0 at x in {0, 1}; w == x bit for bit with a = b = 1);
  * cases A-F through objectives.nll_value_and_grad: per-task values (1e-10 fp64, 2e-4 fp32), every leaf against the analytic reference
    (FP64_GRAD_TOL = 1e-10 / FP32_GRAD_TOL = 2.5e-3 per leaf, helpers.assert_grad_close with its default floor_rel and the a / b leaves'
    own term scales), the route of group B from the profile stages, two identical calls bit-identical (no float atomics);
  * d acq / d x of EI and UCB for the four families at 12 queries, interior ones and x in {0, 1} in columns with a, b > 1.

RATIOS_MEASURED: error over bound as measured on an MI355X (also in profiles/kumar_errors.md).
"""
import ctypes as C

import numpy as np
import pytest

import helpers
import kumar_cases as kc
import kumar_oracle as ko
from hyperbo_amd import _model as hmodel
from hyperbo_amd import _native as nat
from hyperbo_amd.basics import definitions as defs
from hyperbo_amd.bo_utils import acfun
from hyperbo_amd.gp_utils import gp, kernel, mean, objectives, utils
from oracle import hyperbo_oracle as o

pytestmark = pytest.mark.gpu
WF = utils.DEFAULT_WARP_FUNC
WFO = o.DEFAULT_WARP_FUNC

# worst error / bound.  element-wise: per quantity (w, dw/da, dw/db, dw/dx); groups: (per-task value, gradient leaf)
RATIOS_MEASURED = {
    'element-wise fp64': (0.15, 0.032, 0.034, 0.049),    # w at a = b = 8; dw/dx at b = 8
    'element-wise fp32': (0.13, 0.034, 0.035, 0.14),
    'A': (6.0e-5, 3.0e-3),
    'B': (7.1e-5, 3.4e-3),
    'C': (1.8e-5, 2.4e-3),
    'D': (7.2e-5, 1.1e-3),
    'E': (7.2e-3, 2.8e-2),             # fp32
    'F': (4.4e-3, 4.4e-2),             # the fp32 twins; fp64: 3.3e-5, 1.4e-3
    'acq': (0.0, 2.9e-6),              # of 1e-7 max(max |g|, 1e-3): the dot product; the stationary families 4e-8 .. 9e-8
}

_WORST = {}


def _note(group, value=0.0, grad=0.0):
  w = _WORST.setdefault(group, [0.0, 0.0])
  w[0], w[1] = max(w[0], value), max(w[1], grad)


# ---- element-wise --------------------------------------------------------------------------------------------------------------------
def _probe(ctx, dtype):
  """One hbo_probe_kumar_warp call over the grid: quantity -> [211, 36]."""
  ra, rb, a, b = kc.grid_ab(dtype)
  x = np.ascontiguousarray(kc.grid_x(dtype))
  dt = kc.np_dtype(dtype)
  d = x.shape[1]
  model = {'lengthscale': np.zeros(d), 'signal_variance': np.array(0.0), 'noise_variance': np.array(0.0), 'constant': np.array(0.0),
           'kumar_params': {'a': ra, 'b': rb}}
  bm = hmodel.BuiltModel(mean.constant, kernel.squared_exponential_kumar, defs.GPParams(model=kc.cast(model, dt)), WF, dt, d)
  # the device reads the warped a, b the reference was computed at
  got_a = np.ctypeslib.as_array(C.cast(bm.kstruct.kumar_a, C.POINTER(C.c_double if dt == np.float64 else C.c_float)), shape=(d,))
  got_b = np.ctypeslib.as_array(C.cast(bm.kstruct.kumar_b, C.POINTER(C.c_double if dt == np.float64 else C.c_float)), shape=(d,))
  assert np.array_equal(got_a, a) and np.array_equal(got_b, b)
  w = np.full(x.shape, np.nan, dtype=dt)
  da, db, dx = (np.full(x.shape, np.nan) for _ in range(3))
  dp = lambda arr: arr.ctypes.data_as(C.POINTER(C.c_double))
  ctx.check(nat.lib().hbo_probe_kumar_warp(ctx.handle, bm.ref(), nat.ptr(x), x.shape[0], nat.ptr(w), dp(da), dp(db), dp(dx)), allow_not_pd=False)
  return {'w': w, 'da': da, 'db': db, 'dx': dx}


@pytest.mark.parametrize('dtype', ['fp64', 'fp32'])
def test_warp_and_its_derivatives_per_element(gpu_ctx, dtype):
  got = _probe(gpu_ctx, dtype)
  x = kc.grid_x(dtype)
  _, _, a, b = kc.grid_ab(dtype)
  er = kc.elem_reference(dtype)
  assert got['w'].dtype == x.dtype
  # the exact identities
  assert np.all(got['w'][0] == 0) and np.all(got['w'][10] == 1)
  for q in ('da', 'db'):
    assert np.all(got[q][0] == 0) and np.all(got[q][10] == 0), q
  col = int(np.flatnonzero((a == 1) & (b == 1))[0])
  assert np.array_equal(got['w'][:, col], x[:, col])
  # everything finite except dw/dx where it is infinite: those entries are left out of the comparison (the device answers +inf or,
  # where its exp2 saturates, a number beyond 1e300 / 1e30; never NaN)
  assert all(np.isfinite(got[q]).all() for q in ('w', 'da', 'db'))
  assert np.isfinite(got['dx'][er.dx_finite]).all() and int((~er.dx_finite).sum()) == kc.DX_LEFT_OUT
  assert np.all(got['dx'][~er.dx_finite] > (1e300 if dtype == 'fp64' else 1e30))
  ratios = kc.elem_ratios(dtype, got)
  print(f'KUMAR element-wise {dtype}: ' + ' '.join(f'{q} {r:.3e}' for q, (r, _) in ratios.items()))
  _WORST['element-wise ' + dtype] = [ratios[q][0] for q in kc.QUANTITIES]
  for q, (r, at) in ratios.items():
    assert r <= 1.0, (q, r, at, None if at is None else (float(x[at]), float(a[at[1]]), float(b[at[1]]), float(got[q][at]), er.ref[q][at]))


def test_probe_rejects_bad_arguments(gpu_ctx):
  lib = nat.lib()
  d = 2
  model = {'lengthscale': np.zeros(d), 'signal_variance': np.array(0.0), 'noise_variance': np.array(0.0), 'constant': np.array(0.0),
           'kumar_params': {'a': np.zeros(d), 'b': np.zeros(d)}}
  bm = hmodel.BuiltModel(mean.constant, kernel.matern32_kumar, defs.GPParams(model=model), WF, np.float64, d)
  plain = hmodel.BuiltModel(mean.constant, kernel.matern32, defs.GPParams(model=model), WF, np.float64, d)
  x = np.full((3, d), 0.5)
  w, da, db, dx = (np.zeros((3, d)) for _ in range(4))
  dp = lambda arr: arr.ctypes.data_as(C.POINTER(C.c_double))
  call = lambda m, xx, n, ww, aa, bb, gg: lib.hbo_probe_kumar_warp(gpu_ctx.handle, m, xx, n, ww, aa, bb, gg)
  assert call(bm.ref(), nat.ptr(x), 3, nat.ptr(w), dp(da), dp(db), dp(dx)) == nat.HBO_OK and np.all(w == 0.5)     # a = b = 1
  assert call(plain.ref(), nat.ptr(x), 3, nat.ptr(w), dp(da), dp(db), dp(dx)) == nat.HBO_ERR_ARG
  assert b'Kumaraswamy' in lib.hbo_last_error(gpu_ctx.handle)
  for n in (0, -1):
    assert call(bm.ref(), nat.ptr(x), n, nat.ptr(w), dp(da), dp(db), dp(dx)) == nat.HBO_ERR_ARG
  assert call(None, nat.ptr(x), 3, nat.ptr(w), dp(da), dp(db), dp(dx)) == nat.HBO_ERR_ARG
  assert call(bm.ref(), None, 3, nat.ptr(w), dp(da), dp(db), dp(dx)) == nat.HBO_ERR_ARG
  assert call(bm.ref(), nat.ptr(x), 3, None, dp(da), dp(db), dp(dx)) == nat.HBO_ERR_ARG
  assert call(bm.ref(), nat.ptr(x), 3, nat.ptr(w), None, dp(db), dp(dx)) == nat.HBO_ERR_ARG
  assert call(bm.ref(), nat.ptr(x), 3, nat.ptr(w), dp(da), None, dp(dx)) == nat.HBO_ERR_ARG
  assert call(bm.ref(), nat.ptr(x), 3, nat.ptr(w), dp(da), dp(db), None) == nat.HBO_ERR_ARG


# ---- NLL and its leaves ----------------------------------------------------------------------------------------------------------------
def _funcs(case):
  return getattr(mean, case.mname), getattr(kernel, case.kname + '_kumar')


def _evaluate(case, ctx):
  """(per-task values in the case's order, mean value, gradient tree of the mean, profile stages) of one value + gradient call."""
  mf, cf = _funcs(case)
  ds = {k: defs.SubDataset(x, y) for k, (x, y) in enumerate(kc.inputs(case).tasks)}
  dev = objectives.DeviceDataset(ds, ctx=ctx)
  try:
    assert dev.dtype == case.np_dtype
    ctx.profile_enable(1)
    try:
      total, per, g, bm = dev.evaluate(mf, cf, defs.GPParams(model=kc.inputs(case).model), WF, want_grad=True, per_task=True)
      stages = ctx.profile_get()
    finally:
      ctx.profile_enable(0)
  finally:
    dev.close()
  t = len(case.tasks)
  return [per[k] for k in range(t)], total / t, bm.unflatten_grad(g / t), stages


@pytest.mark.parametrize('case', kc.CASES, ids=lambda c: c.id)
def test_nll_values_and_every_leaf(gpu_ctx, case):
  ref = kc.reference(case)
  per, value, grad, stages = _evaluate(case, gpu_ctx)
  assert 'kumar_forward' in stages and 'kumar_backward' in stages, sorted(stages)
  if case.group == 'B':
    # the single-workgroup evaluation up to one block, the blocked pipeline beyond
    small = case.tasks[0] <= kc.TILE
    assert ('small_eval' in stages) == small and ('potrf' in stages) == (not small), sorted(stages)
  vr = max(abs(got - tr.value) / (case.value_tol * abs(tr.value)) for got, tr in zip(per, ref.tasks))
  gr, leaf = kc.grad_ratio(grad, ref.grad, case.grad_tol, ref.leaf_scales)
  print(f'KUMAR {case.id}: value {vr:.3e} grad {gr:.3e} ({leaf})')
  _note(case.group, vr, gr)
  assert all(np.isfinite(v) for v in per) and vr <= 1.0, (per, [tr.value for tr in ref.tasks])
  assert abs(value - ref.value) <= case.value_tol * abs(ref.value)
  helpers.assert_grad_close(grad, ref.grad, case.grad_tol, label=case.id, leaf_scales=ref.leaf_scales)
  # the public entry point, a second evaluation on a dataset of its own: the same bits
  mf, cf = _funcs(case)
  ds = {k: defs.SubDataset(x, y) for k, (x, y) in enumerate(kc.inputs(case).tasks)}
  v2, g2 = objectives.nll_value_and_grad(mf, cf, defs.GPParams(model=kc.inputs(case).model), ds, WF)
  assert v2 == value
  for (path, g_a), (_, g_b) in zip(helpers.tree_leaves(grad), helpers.tree_leaves(g2)):
    np.testing.assert_array_equal(g_a, g_b, err_msg=path)


# ---- d acquisition / d x ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kname', helpers.KERNELS)
def test_acquisition_gradient_through_the_warp(gpu_ctx, kname):
  model, x, y, xo, yo, xq = kc.acq_inputs(kname)
  kp = model['kumar_params']
  a, b = ko.squareplus(kp['a']), ko.squareplus(kp['b'])
  assert np.all(a[:4] > 1) and np.all(b[:4] > 1) and np.sum(xq == 0) == 6 and np.sum(xq == 1) == 6
  m = gp.GP({'t': defs.SubDataset(x, y), 'other': defs.SubDataset(xo, yo)}, mean.constant, getattr(kernel, kname + '_kumar'),
            defs.GPParams(model=model), WF)
  po = o.GPParams(model={k: v for k, v in model.items() if k != 'kumar_params'})
  noise = float(np.squeeze(o.retrieve_params(po, ['noise_variance'], WFO)[0]))
  wx, wq = ko.warp(x, kp['a'], kp['b']), ko.warp(xq, kp['a'], kp['b'])
  dwdx = ko.dw_dx(xq, a, b)
  assert np.isfinite(dwdx).all() and np.all(dwdx[xq == 0] == 0) and np.all(dwdx[xq == 1] == 0)
  worst = 0.0
  for acq, fn, param in (('ei', acfun.expected_improvement, float(np.max(y))), ('ucb', acfun.ucb, 3.0)):
    val, grad = fn.value_and_grad(model=m, sub_dataset_key='t', x_queries=xq)
    vo, go = o.acquisition_value_and_grad(acq, o.constant, getattr(o, kname), po, wx, y, wq, param, WFO, add_noise=noise, scale=2.0)
    go = go * dwdx
    assert np.all(np.isfinite(grad))
    np.testing.assert_allclose(val, vo, rtol=1e-8, atol=1e-10)
    # the tolerance of test_matern_with_duplicated_training_rows (tests/test_gpu_parity.py)
    bound = 1e-7 * max(np.max(np.abs(go)), 1e-3)
    worst = max(worst, float(np.max(np.abs(grad - go))) / bound)
    assert np.max(np.abs(grad - go)) <= bound, (acq, np.max(np.abs(grad - go)), bound)
    assert np.all(grad[xq == 0] == 0) and np.all(grad[xq == 1] == 0)      # dw/dx = 0 there, exactly
  print(f'KUMAR acq {kname}: grad {worst:.3e}')
  _note('acq', grad=worst)


def test_zz_print_measured_ratios():
  """Last in the file: what this run measured, beside RATIOS_MEASURED (python -m pytest tests/test_gpu_kumar_leaves.py -m gpu -s)."""
  for group in sorted(_WORST):
    print(f'KUMAR RATIOS {group}: ' + ' '.join(f'{v:.2e}' for v in _WORST[group]) + f'   (recorded: {RATIOS_MEASURED.get(group)})')
