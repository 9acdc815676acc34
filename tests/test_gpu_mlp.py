"""The MLP basis on an MI355X (run with `-m gpu`) at layer widths up to 256 (HBO_MAX_FEATURE_DIM), depths 1 .. 8 and batches of more than
one 256-row chunk, PER LEAF -- every Dense_l/kernel and Dense_l/bias is its own leaf -- against tests/mlp_cases.py (judged on its own by
tests/test_mlp_cases_host.py).  The four implementations, each with its own forward and backward pass:

  the batched layers of the objectives (csrc/mlp.hip from csrc/objective.hip)    test_blocked_objective_*, test_divergence_*
  the single-workgroup evaluation (csrc/small.hip) into the MLP backward          test_single_workgroup_*
  the per-task query side (dense_tanh_kernel; dense_bwd_* from hbo_acq_grad)      test_gram_*, test_predict_*, test_query_side_backward_*
  per-sample weight sets (model_weights of dense_tanh_batch_kernel)               test_per_sample_weights_*

Bounds: mlp_cases.py (the project's own; an MLP leaf's floor is min(1e-3 max|g|, its un-cancelled term scale)).  No weight gradient is
compared bit for bit: they are summed with fp64 atomics.  Every test prints its worst ratio to a bound as an `MLPERR` line (-s);
profiles/mlp_errors.md holds what an MI355X gave, per case and dtype.  Worst fractions of a bound there:

                         fp64      fp32
  blocked: value / leaf  1.8e-4 / 2.0e-2   4.3e-2 / 1.4e-1 (lengthscale; worst MLP leaf 3.9e-2)
  small: value / leaf    6.3e-5 / 4.8e-3   1.7e-2 / 4.6e-2; against the blocked pipeline (fp64) 3.0e-2
  EKL: value / leaf      3.0e-6 / 1.9e-4   1.2e-1 / 1.9e-3
  Gram entry             5.6e-2            1.6e-1
  predict: mean / var    1.4e-4 / 2.1e-6   3.3e-1 / 1.7e-4
  acq_grad: value        3.8e-5            2.3e-2
  acq_grad: gradient     9.2e-4            7.9e-1: UCB, (193, 1) on d = 256, M = 1025, the query whose gradient is the smallest of the
                                           1025 (one last-layer column: all of d acq / dx vanishes where d acq / d f changes sign; the
                                           bound is relative to the query's own gradient); every other case <= 5.4e-2
  samples: alone/oracle  0 / 4.1e-5        0 / 1.7e-1
With dense_bwd_w_batch_kernel's column loop stopped at 64 (a scratch build), all 72 blocked and single-workgroup runs with a layer wider
than 64 fail, fp64 and fp32."""
import numpy as np
import pytest

import acq_grad_cases as G
import helpers
import mlp_cases as mc
import test_gpu_acq_grad_shapes as ags
import test_gpu_slice as slice_tier
import test_gpu_small_path as sp
from oracle import hyperbo_oracle as o

pytestmark = pytest.mark.gpu
WFO = o.DEFAULT_WARP_FUNC
IDS = lambda c: c.id
DTYPES = pytest.mark.parametrize('dtype', mc.DTYPES)
GRAM_TOL = {'fp64': 1e-13, 'fp32': 2e-5}          # tests/test_gpu_parity.py: test_gram_vs_oracle
# posterior mean and variance, tests/test_gpu_parity.py: fp64 1e-9 (test_factor_predict_acquisition_vs_oracle); fp32 2e-4 on values and
# 5e-3 on variances (its docstring).  Per query, the variance relative to the prior variance, the mean to max(prior sd, max |mean|)
PREDICT_TOL = {'fp64': (1e-9, 1e-9), 'fp32': (2e-4, 5e-3)}
QUERY_COUNTS = (1, 255, 257)
ACQ_COUNTS = (1, 257, 1025)                       # 1025: a second 1024-query pass re-uses d_t0 / d_t1 and the activations' buffers
ACQS = ('ei', 'ucb')
EKL = 1                                           # include/hbo.h: HBO_OBJ_EKL
NARROW, WIDE = mc.BY_FEATS[(12, 1)], mc.BY_FEATS[(256, 256)]


def _native():
  from hyperbo_amd import _model, _native as nat
  from hyperbo_amd.basics import definitions as defs
  from hyperbo_amd.gp_utils import gp, kernel, mean, objectives, utils
  return nat, _model, defs, gp, kernel, mean, objectives, utils


def _err(what, case_id, dtype, ratio, where=''):
  print(f'\nMLPERR|{what}|{case_id}|{dtype}|{ratio:.3e}|{where}')


def _profiled(ctx, fn, small_fused):
  """fn() with profiling on and hbo_tune small_fused as given; (result, the stages that ran)."""
  ctx.set_option('small_fused', small_fused)
  ctx.profile_enable(1)
  try:
    out = fn()
    seen = set(ctx.profile_get())
  finally:
    ctx.set_option('small_fused', 1)
    ctx.profile_enable(0)
  return out, seen


def _funcs(case):
  _, _, _, _, kernel, mean, _, _ = _native()
  return mean.linear_mlp, getattr(kernel, case.kname + '_mlp')


def _params(case, model):
  return _native()[2].GPParams(model=model, config=mc.config(case))


def _dataset(case, sizes, dtype):
  defs = _native()[2]
  return {x.shape[0]: defs.SubDataset(x, y) for x, y in mc.inputs(case, sizes, dtype).tasks}


def _nll(ctx, case, sizes, dtype, small_fused):
  """(value, gradient tree, per-task values by size) of one evaluation, with the stages asserted: the blocked pipeline with the batched MLP
  backward (small_fused = 0) or the single-workgroup evaluation (1)."""
  objectives, utils = _native()[6:]
  mn, kn = _funcs(case)
  pn, wf = _params(case, mc.inputs(case, sizes, dtype).model), utils.DEFAULT_WARP_FUNC
  ds = objectives.DeviceDataset(_dataset(case, sizes, dtype), ctx=ctx)       # resident on `ctx`: both calls below run there
  try:
    (v, g), seen = _profiled(ctx, lambda: objectives.nll_value_and_grad(mn, kn, pn, ds, wf), small_fused)
    (t, k2n), seen2 = _profiled(ctx, lambda: objectives.neg_log_marginal_likelihood(mn, kn, pn, ds, wf, return_key2nll=True), small_fused)
  finally:
    ds.close()
  for s in (seen, seen2):
    if small_fused:
      assert 'small_eval' in s and 'potrf' not in s, sorted(s)
    else:
      assert 'potrf' in s and 'small_eval' not in s, sorted(s)
  assert 'mlp_backward' in seen, sorted(seen)
  return v, g, t, k2n


def _check_nll(ctx, case, sizes, dtype, small_fused, what):
  """Value, every task's value and the gradient per leaf against the oracle."""
  ref = mc.reference(case, sizes, dtype)
  vtol, gtol = mc.tols(dtype)
  v, g, t, k2n = _nll(ctx, case, sizes, dtype, small_fused)
  assert sorted(k2n) == sorted(mc.SIZES[sizes])
  vr = max([mc.value_ratio(v, ref.value, vtol), mc.value_ratio(t, ref.value, vtol)] +
           [mc.value_ratio(k2n[n], pv, vtol) for n, pv in zip(mc.SIZES[sizes], ref.per_task)])
  ratios = mc.leaf_ratios(g, ref.grad, gtol, ref.scales)
  worst, leaf = mc.worst_leaf(ratios)
  worst_mlp, leaf_mlp = mc.worst_leaf({p: ratios[p] for p in mc.mlp_leaf_paths(case)})
  _err(what + ' value', f'{case.id} {sizes}', dtype, vr)
  _err(what + ' leaf', f'{case.id} {sizes}', dtype, worst, leaf)
  _err(what + ' mlp leaf', f'{case.id} {sizes}', dtype, worst_mlp, leaf_mlp)
  assert vr <= 1.0, (case.id, sizes, dtype, v, t, ref.value, k2n, ref.per_task)
  helpers.assert_grad_close(g, ref.grad, gtol, label=f'{what} {case.id} {sizes} {dtype}', leaf_scales=ref.scales)
  assert worst <= 1.0
  return v, g


# ---- 1. the objectives ----------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize('case', mc.CASES, ids=IDS)
def test_blocked_objective_per_leaf(gpu_ctx, case, dtype):
  """Three row chunks of the weight gradient, tasks that leave after the first and the second; every thread count of
  dense_bwd_w_batch_kernel; dF / dtmp alternate over 1, 2, 3 and 8 layers."""
  _check_nll(gpu_ctx, case, 'blocked', dtype, 0, 'blocked')


@DTYPES
@pytest.mark.parametrize('case', mc.CASES, ids=IDS)
def test_single_workgroup_per_leaf(gpu_ctx, case, dtype):
  """small.hip's forward pass and grad_feat_kernel into the MLP backward, at widths 65 .. 256; in fp64 also against the blocked pipeline
  on the same batch (another summation order: rounding, not bits)."""
  v, g = _check_nll(gpu_ctx, case, 'small', dtype, 1, 'small')
  if dtype == 'fp64':
    vb, gb, _, _ = _nll(gpu_ctx, case, 'small', dtype, 0)
    ref = mc.reference(case, 'small', dtype)
    worst, leaf = mc.worst_leaf(mc.leaf_ratios(g, gb, sp.BLOCKED_GRAD_TOL, ref.scales))
    _err('small vs blocked leaf', f'{case.id} small', dtype, worst, leaf)
    _err('small vs blocked value', f'{case.id} small', dtype, mc.value_ratio(v, vb, sp.BLOCKED_VALUE_TOL))
    assert abs(v - vb) <= sp.BLOCKED_VALUE_TOL * max(abs(vb), 1.0), (v, vb)
    helpers.assert_grad_close(g, gb, sp.BLOCKED_GRAD_TOL, label=f'{case.id} small vs blocked', leaf_scales=ref.scales)


@DTYPES
@pytest.mark.parametrize('order', ['wide-first', 'narrow-first'])
def test_both_paths_in_one_context(gpu_ctx, order, dtype):
  """Workspaces and d_mlp_w only grow: a narrow model after a wide one (and the reverse), on both paths of one context, each against its
  own reference."""
  nat = _native()[0]
  first, second = (WIDE, NARROW) if order == 'wide-first' else (NARROW, WIDE)
  ctx = nat.Context(gpu_ctx.device)       # a context of its own: what grows, grows here, in this order
  try:
    ctx.set_option('poison', 1)
    for case, sizes, fused in ((first, 'blocked', 0), (second, 'small', 1), (first, 'small', 1), (second, 'blocked', 0), (first, 'blocked', 0)):
      _check_nll(ctx, case, sizes, dtype, fused, f'one context {order}')
  finally:
    ctx.close()


@DTYPES
def test_divergence_objective_on_a_wide_last_layer(gpu_ctx, dtype):
  """EKL on (12, 129) with one aligned task of 130 points: value-only and value + gradient calls, the bounds of test_gpu_divergence.py."""
  nat, _, defs, _, _, _, objectives, utils = _native()
  case = mc.EKL_CASE
  model, x, y = mc.ekl_inputs(dtype)
  vo, go, scale, bound = mc.ekl_reference(dtype)
  mn, kn = _funcs(case)
  dev = objectives.DeviceDataset({0: defs.SubDataset(x, y, aligned=0)}, only_aligned=True, ctx=gpu_ctx)
  try:
    assert dev.dtype == mc.np_dtype(dtype)
    t0, p0, _, _ = dev.evaluate(mn, kn, _params(case, model), utils.DEFAULT_WARP_FUNC, want_grad=False, per_task=True, objective=EKL)
    t1, p1, g, bm = dev.evaluate(mn, kn, _params(case, model), utils.DEFAULT_WARP_FUNC, want_grad=True, per_task=True, objective=EKL)
    grad = bm.unflatten_grad(g)
  finally:
    dev.close()
  vr = max(abs(v - vo) / bound if np.isfinite(v) else np.inf for v in (t0, t1, p0[0], p1[0]))
  ratios = mc.leaf_ratios(grad, go, mc.tols(dtype)[1])
  _err('ekl value', case.id, dtype, vr)
  _err('ekl leaf', case.id, dtype, *mc.worst_leaf(ratios))
  assert vr <= 1.0, (t0, t1, vo, bound)
  helpers.assert_grad_close(grad, go, mc.tols(dtype)[1], label=f'ekl {case.id} {dtype}')


# ---- 2. the forward pass alone --------------------------------------------------------------------------------------------------------
def _prior_variance(case, po, feat):
  return np.asarray(getattr(o, case.kname)(po, feat, warp_func=WFO, diag=True), dtype=np.float64)


@DTYPES
@pytest.mark.parametrize('case', mc.CASES, ids=IDS)
def test_gram_per_entry(gpu_ctx, case, dtype):
  """hbo_gram through dense_tanh_kernel: the symmetric Gram of the 257-point task and its cross Gram with the 129-point one, per entry
  relative to the signal variance (the dot product: to the largest prior variance); two calls give the same bits."""
  utils = _native()[7]
  model, tasks = mc.inputs(case, 'blocked', dtype)
  x1, x2 = tasks[3][0], tasks[0][0]
  assert (x1.shape[0], x2.shape[0]) == (257, 129)
  kn, ko = _funcs(case)[1], mc.oracle_funcs(case)[1]
  pn, po = _params(case, model), mc.oracle_params(case, model)
  x1o, x2o = x1.astype(np.float64), x2.astype(np.float64)
  scale = float(np.max(_prior_variance(case, po, o.mlp_apply(po.model['mlp_params'], x1o))))
  worst = 0.0
  for args, argso in (((x1,), (x1o,)), ((x1, x2), (x1o, x2o))):
    got = kn(pn, *args, warp_func=utils.DEFAULT_WARP_FUNC)
    again = kn(pn, *args, warp_func=utils.DEFAULT_WARP_FUNC)
    ref = ko(po, *argso, warp_func=WFO)
    assert got.shape == ref.shape and got.dtype == mc.np_dtype(dtype) and np.isfinite(got).all()
    assert got.tobytes() == again.tobytes()
    worst = max(worst, float(np.max(np.abs(got.astype(np.float64) - ref))) / (GRAM_TOL[dtype] * scale))
  _err('gram entry', case.id, dtype, worst)
  assert worst <= 1.0


_PREDICT_REF = {}


def _predict_reference(case, dtype):
  """Posterior mean and variance of the 257-point task at the first 257 points of the 513-point one: once per case and dtype (queries are
  independent: the smaller counts are its leading rows)."""
  key = (case, dtype)
  if key not in _PREDICT_REF:
    model, tasks = mc.inputs(case, 'blocked', dtype)
    (x, y), xq = tasks[3], tasks[4][0][:max(QUERY_COUNTS)]
    mo, ko = mc.oracle_funcs(case)
    po = mc.oracle_params(case, model)
    mu, var = o.predict(mo, ko, po, x.astype(np.float64), y.astype(np.float64), xq.astype(np.float64), WFO)
    prior = _prior_variance(case, po, o.mlp_apply(po.model['mlp_params'], xq.astype(np.float64)))
    _PREDICT_REF[key] = (mu[:, 0], var[:, 0], prior)
  return _PREDICT_REF[key]


@DTYPES
@pytest.mark.parametrize('case', mc.CASES, ids=IDS)
def test_predict_per_query(gpu_ctx, case, dtype):
  """gp.predict at M = 1, 255 and 257 queries (query_features: one dense_tanh_kernel launch per layer over all queries), per query; two
  calls give the same bits."""
  _, _, _, gp, _, _, _, utils = _native()
  model, tasks = mc.inputs(case, 'blocked', dtype)
  (x, y), xq_all = tasks[3], tasks[4][0]
  mu_o, var_o, prior = _predict_reference(case, dtype)
  mn, kn = _funcs(case)
  pn = _params(case, model)
  mtol, vtol = PREDICT_TOL[dtype]
  mscale = max(float(np.max(np.abs(mu_o))), float(np.sqrt(np.max(prior))))
  worst = [0.0, 0.0]
  for M in QUERY_COUNTS:
    xq = np.ascontiguousarray(xq_all[:M])
    mu, var = gp.predict(mn, kn, pn, x, y, xq, utils.DEFAULT_WARP_FUNC)
    mu2, var2 = gp.predict(mn, kn, pn, x, y, xq, utils.DEFAULT_WARP_FUNC)
    assert mu.shape == (M, 1) and var.shape == (M, 1) and np.isfinite(mu).all() and np.isfinite(var).all()
    assert mu.tobytes() == mu2.tobytes() and var.tobytes() == var2.tobytes()
    rm = np.abs(mu[:, 0].astype(np.float64) - mu_o[:M]) / (mtol * mscale)
    rv = np.abs(var[:, 0].astype(np.float64) - var_o[:M]) / (vtol * prior[:M])
    worst = [max(worst[0], float(rm.max())), max(worst[1], float(rv.max()))]
    assert rm.max() <= 1.0 and rv.max() <= 1.0, (case.id, dtype, M, int(np.argmax(rm)), float(rm.max()), int(np.argmax(rv)), float(rv.max()))
  _err('predict mean', case.id, dtype, worst[0])
  _err('predict variance', case.id, dtype, worst[1])


# ---- 3. the backward pass to the query -----------------------------------------------------------------------------------------------------
QUERY_FEATS = [(256,), (65,), (12, 193), (256, 33), (256, 256), (1, 256), (193, 1), (128, 193), (129, 65, 193), mc.DEPTH8]


def _acq_case(case, M, dtype, mlp_k=True):
  return G.Case('W', case.kname, mlp_k, 'linear_mlp', False, 150, M, case.d, tuple(case.feats), case.ls, dtype)


ACQ_CASES = ([_acq_case(mc.BY_FEATS[f], M, dt) for f in QUERY_FEATS for M in ACQ_COUNTS for dt in mc.DTYPES] +
             # a plain kernel on the raw inputs under the linear_mlp mean: the MLP backward starts from the mean's gradient alone (gmlp = d_t0)
             [_acq_case(mc.Case(5, (12, 129), 'matern52', 'ard'), M, dt, mlp_k=False) for M in ACQ_COUNTS for dt in mc.DTYPES])


@pytest.mark.parametrize('case', ACQ_CASES, ids=IDS)
def test_query_side_backward_per_query(gpu_ctx, case):
  """d acquisition / d x of EI and UCB from hbo_acq_grad, per query, with the bounds of tests/test_gpu_acq_grad_shapes.py; the weight
  gradient of launch_dense_bwd goes to a sink, the chain to d / dx is what is checked."""
  ref = G.reference(case)
  dev = ags._Device(gpu_ctx, case)
  try:
    for acq in ACQS:
      assert np.isfinite(ref.val[acq]).all() and np.isfinite(ref.grad[acq]).all() and G.checked(case, acq, ref).any(), (case.id, acq)
      val, grad = dev.acq_grad(acq, G.acq_param(acq, ref))
      (rv, qv), (rg, qg, gam) = G.worst(case, acq, ref, val, grad)
      _err(f'acq {acq} value', case.id, case.dtype, rv, f'query {qv}')
      _err(f'acq {acq} gradient', case.id, case.dtype, rg, f'query {qg} gamma {gam:.2f}')
      ags._judge(case, ref, acq, val, grad, label=f'wide MLP {case.dtype}')
  finally:
    dev.close()


# ---- 4. per-sample weight sets ---------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize('shape', sorted(mc.SAMPLE_SIZES))
@pytest.mark.parametrize('case', mc.SAMPLE_CASES, ids=IDS)
def test_per_sample_weights(gpu_ctx, case, shape, dtype):
  """hbo_nll_samples with three weight sets: every sample's total and per-task values equal hbo_nll with that sample alone and the oracle
  (tests/test_gpu_slice.py's tolerances); per task also the float64 restatement, which sample 0's weights for every sample miss."""
  nat, _model, defs, _, _, _, objectives, utils = _native()
  models, tasks = mc.sample_inputs(case, shape, dtype)
  mn, kn = _funcs(case)
  dt = mc.np_dtype(dtype)
  dev = objectives.DeviceDataset({k: defs.SubDataset(x, y) for k, (x, y) in enumerate(tasks)}, ctx=gpu_ctx)
  try:
    built = [_model.BuiltModel(mn, kn, _params(case, m), utils.DEFAULT_WARP_FUNC, dt, case.d) for m in models]
    rc, tot, pt = slice_tier._call(gpu_ctx, dev, built)
    assert rc == nat.HBO_OK and np.isfinite(tot).all() and np.isfinite(pt).all()
    tol_nll, tol_o = mc.SAMPLE_TOL[dtype]
    order = list(dev.device_order_keys)
    expect = mc.sample_values(case, shape, dtype)
    dso = {k: o.SubDataset(x.astype(np.float64), y.astype(np.float64)) for k, (x, y) in enumerate(tasks)}
    mo, ko = mc.oracle_funcs(case)
    worst = [0.0, 0.0]
    for s in range(mc.SAMPLE_COUNT):
      rc1, tot1, pt1 = slice_tier._solo(gpu_ctx, dev, built[s])
      assert rc1 == nat.HBO_OK
      worst[0] = max(worst[0], abs(tot[s] - tot1) / (tol_nll * abs(tot1)), float(np.max(np.abs(pt[s] - pt1) / (tol_nll * np.abs(pt1)))))
      vo = o.neg_log_marginal_likelihood(mo, ko, mc.oracle_params(case, models[s]), dso, WFO)
      per = np.array([expect[s][k] for k in order])
      worst[1] = max(worst[1], abs(tot[s] / len(tasks) - vo) / (tol_o * abs(vo)), float(np.max(np.abs(pt[s] - per) / (tol_o * np.abs(per)))))
    _err('samples vs alone', f'{case.id} {shape}', dtype, worst[0])
    _err('samples vs oracle', f'{case.id} {shape}', dtype, worst[1])
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst
  finally:
    dev.close()
