"""hbo_objective with HBO_OBJ_EKL / HBO_OBJ_EUC (csrc/objective.hip) on an MI355X (run with `-m gpu`) against tests/divergence_cases.py,
PER TASK: every case's value-only first call on a fresh dataset and its value + gradient call, each task's value against the oracle
within a bound relative to the task's own term scale S_k, the total as the ordered sum of the per-task values to the bit, the gradient
per leaf, the public objectives.ekl / objectives.euc mean; group D in addition task by task, sub-sampled on the device and under the
sweep options; the two EKL back ends (objective.hip: the one-sweep inverse / trtri + lauum) on the nine-block batch of group S, the
smallest at which the options can choose between them; a smaller case after the largest one against a fresh context; the degenerate
cases of group F.

Bounds (divergence_cases.py): fp64 value 1e-10 S_k, gradient FP64_GRAD_TOL per leaf; fp32 value 4 x the float32 restatement's own
error + 8 eps32 S_k, gradient FP32_GRAD_TOL per leaf; Kumaraswamy a / b leaves 1e-10 against the analytic reference (divergence_cases.ab_analytic).
RATIOS_MEASURED: error over bound, the worst task / leaf of each case group, as measured on an MI355X (also in
profiles/divergence_errors.md).
"""
from typing import NamedTuple

import numpy as np
import pytest

import divergence_cases as dc
import helpers
from hyperbo_amd import _native as nat
from hyperbo_amd.basics import definitions as defs
from hyperbo_amd.gp_utils import kernel, mean, objectives, utils

pytestmark = pytest.mark.gpu
WF = utils.DEFAULT_WARP_FUNC

# worst error / bound per case group: (per-task value, gradient leaf[, Kumaraswamy a / b leaf]), measured on an MI355X
RATIOS_MEASURED = {
    'A': (6.3e-6, 1.1e-3),             # value: (150, 1) EKL; gradient: noise_variance at (150, 126) EKL
    'B': (8.9e-6, 2.5e-4),             # value: (127, 3) EKL; gradient: constant at (257, 3) EKL
    'C': (2.2e-5, 1.8e-2, 6.0e-4),     # the plain dot product + zero, EKL: value at (129, 127), dot_prod_sigma at (129, 128); a / b (of 1e-10, analytic): dot_product_kumar (129, 128) EKL
    'D': (4.4e-5, 1.8e-3),             # dot_product_mlp + linear_mlp, EKL: task (300, 2); dot_prod_sigma
    'D alone': (4.4e-5, 9.6e-3),       # gradient: constant of (150, 127) alone, matern52 + constant, EKL
    'D sub-sampled': (3.5e-5, 8.7e-3),
    'D options': (4.4e-5, 1.8e-3),     # the numbers of 'D': below eight blocks the options choose nothing
    'E': (0.22, 2.0e-3),               # fp32.  value: task (140, 128) of the SE + zero batch, EKL (the single-task cases 4e-4 .. 0.06); gradient: noise_variance at (150, 128) EKL
    'F': (8.5e-6, 5.2e-4),
    'S': (1.5e-5, 3.2e-4),
    'S options': (1.5e-5, 3.2e-4),     # sweep = 0 and sweep = 2 alike; sweep_qs = 1: gradient 3.0e-4 (another leaf)
}

_WORST = {}      # group -> [value ratio, gradient ratio, a / b ratio] of this run (printed by the last test of the file)


def _note(group, value=0.0, grad=0.0, ab=0.0):
  w = _WORST.setdefault(group, [0.0, 0.0, 0.0])
  w[0], w[1], w[2] = max(w[0], value), max(w[1], grad), max(w[2], ab)


def _funcs(case):
  return getattr(mean, case.mname), getattr(kernel, case.kernel_name)


def _params(case):
  return defs.GPParams(model=dc.inputs(case).model, config=dc.config())


def _dataset(case, keep=None):
  return {k: defs.SubDataset(x, y, aligned=k) for k, (x, y) in enumerate(dc.inputs(case).tasks) if keep is None or k in keep}


class Run(NamedTuple):
  total0: float              # the first call on the fresh dataset: value only
  per0: dict                 # task index -> value
  total: float               # the value + gradient call
  per: dict
  grad: dict                 # d sum / d raw params.model
  order: list                # the dataset's order on the device (largest task first, stable)


def _evaluate_on(dev, case):
  mf, cf = _funcs(case)
  t0, p0, _, _ = dev.evaluate(mf, cf, _params(case), WF, want_grad=False, per_task=True, objective=case.obj_id)
  t1, p1, g, bm = dev.evaluate(mf, cf, _params(case), WF, want_grad=True, per_task=True, objective=case.obj_id)
  return Run(t0, p0, t1, p1, bm.unflatten_grad(g), list(dev.device_order_keys))


def _evaluate(case, ctx, keep=None):
  dev = objectives.DeviceDataset(_dataset(case, keep), only_aligned=True, ctx=ctx)
  try:
    assert dev.dtype == case.np_dtype
    return _evaluate_on(dev, case)
  finally:
    dev.close()


def _check(case, run, ref, label, bounds=None):
  """Every task of the run against `ref` (whose tasks are indexed like the case's); returns (value ratio, gradient ratio, a / b ratio)."""
  bounds = bounds or dc.value_bounds(case, ref)
  keys = sorted(run.per)
  assert sorted(run.per0) == keys and sorted(run.order) == keys
  vr = 0.0
  for k in keys:
    for name, got in (('value-only', run.per0[k]), ('value+grad', run.per[k])):
      assert np.isfinite(got), (label, k, name)
      vr = max(vr, abs(got - ref.values[k]) / bounds[k])
    vr = max(vr, abs(run.per0[k] - run.per[k]) / bounds[k])
  # the total is the sum of the per-task values in the dataset's order, to the bit
  for total, per in ((run.total0, run.per0), (run.total, run.per)):
    s = 0.0
    for k in run.order:
      s += per[k]
    assert s == total, (label, s, total)
  ref_grad = dc.tree_sum([ref.grads[k] for k in keys])
  rest = {k: v for k, v in run.grad.items() if k != 'kumar_params'}
  gr, leaf = dc.grad_ratio(rest, ref_grad, dc.grad_tol(case))
  ab = 0.0
  if case.kumar:
    assert len(keys) == len(case.tasks)
    ab = max(dc.ab_errors(run.grad['kumar_params'], dc.ab_analytic(case), dc.AB_TOL).values())
  print(f'DIVERGENCE {case.id} {label}: value {vr:.3e} grad {gr:.3e} ({leaf})' + (f' a/b {ab:.3e}' if case.kumar else ''))
  worst_task = max(keys, key=lambda k: max(abs(run.per0[k] - ref.values[k]), abs(run.per[k] - ref.values[k])) / bounds[k])
  assert vr <= 1.0, (label, 'task', case.tasks[worst_task], run.per0[worst_task], run.per[worst_task], ref.values[worst_task], bounds[worst_task])
  helpers.assert_grad_close(rest, ref_grad, dc.grad_tol(case), label=f'{case.id} {label}')
  assert ab <= 1.0, (label, run.grad['kumar_params'], dc.ab_analytic(case))
  return vr, gr, ab


@pytest.mark.parametrize('case', dc.CASES, ids=lambda c: c.id)
def test_every_task_matches_the_oracle(gpu_ctx, case):
  run = _evaluate(case, gpu_ctx)
  ref = dc.reference(case)
  _note(case.group, *_check(case, run, ref, 'batch'))
  # the public objective: the mean over the tasks of a fresh dataset's value-only call
  mf, cf = _funcs(case)
  fn = objectives.ekl if case.kind == 'ekl' else objectives.euc
  assert fn(mf, cf, _params(case), _dataset(case), WF) == run.total0 / len(case.tasks)
  if case.group == 'F':
    leaves, ref_leaves = dict(helpers.tree_leaves(run.grad)), dict(helpers.tree_leaves(ref.grad_sum))
    assert all(np.isfinite(v).all() for v in leaves.values())
    for path, r in ref_leaves.items():
      if r.size and np.all(r == 0):
        assert np.all(leaves[path] == 0), (path, leaves[path])


@pytest.mark.parametrize('case', dc.GROUP_D, ids=lambda c: c.id)
def test_mixed_batch_task_by_task_and_sub_sampled(gpu_ctx, case):
  ref = dc.reference(case)
  for k in range(len(case.tasks)):
    _note('D alone', *_check(case, _evaluate(case, gpu_ctx, keep={k}), ref, f'alone {case.tasks[k]}'))
  # rows gathered on the device (hbo_dataset_subsample carries the divergence rows of every column along)
  rows = dc.subsample_rows(case)
  batch = objectives.DeviceBatch(_dataset(case), ctx=gpu_ctx)
  sub = batch.subsample(rows)
  try:
    run = _evaluate_on(sub.get('aligned'), case)
  finally:
    sub.close(); batch.close()
  _note('D sub-sampled', *_check(case, run, dc.reference_subsampled(case), 'sub-sampled'))


SWEEP_OPTIONS = [{'sweep': 0}, {'sweep': 2}, {'sweep': 2, 'sweep_qs': 1}]
SWEEP_DEFAULTS = {'sweep': 1, 'sweep_qs': 0, 'lookahead': 1}     # tests/test_gpu_fuzz.py: DEFAULTS


def _evaluate_under(ctx, case, opts):
  """(_evaluate under the options, the stages of its value + gradient call); the defaults restored whatever happens."""
  try:
    for k, v in opts.items():
      ctx.set_option(k, v)
    ctx.profile_enable(1)
    run = _evaluate(case, ctx)
    stages = set(ctx.profile_get())
  finally:
    ctx.profile_enable(0)
    for k, v in SWEEP_DEFAULTS.items():
      ctx.set_option(k, v)
  return run, stages


@pytest.mark.parametrize('opts', SWEEP_OPTIONS, ids=lambda o_: ','.join(f'{k}={v}' for k, v in o_.items()))
@pytest.mark.parametrize('case', dc.GROUP_D, ids=lambda c: c.id)
def test_mixed_batch_under_the_sweep_options(gpu_ctx, case, opts):
  """The mixed batch under the options that choose the EKL back end, each run against the reference.  At three blocks they choose
  nothing -- sched.hip:use_sweep is false below eight blocks -- so every run takes the block-recursive inverse and K^-1 = W^T W
  (checked: a change of that threshold must bring this batch through the other back end with its eyes open); the back ends
  themselves are compared by test_both_inverse_back_ends_on_a_nine_block_batch."""
  run, stages = _evaluate_under(gpu_ctx, case, opts)
  if case.kind == 'ekl':
    assert 'lauum' in stages and 'sweep_tail' not in stages, stages
  _note('D options', *_check(case, run, dc.reference(case), 'options ' + str(opts)))


@pytest.mark.parametrize('opts', SWEEP_OPTIONS, ids=lambda o_: ','.join(f'{k}={v}' for k, v in o_.items()))
def test_both_inverse_back_ends_on_a_nine_block_batch(gpu_ctx, opts):
  """sweep = 0: the block-recursive inverse and K^-1 = W^T W after the chain; sweep = 2 (with look-ahead forced, as
  test_one_sweep_inverse_across_the_registry_and_objectives does): the one-sweep inverse behind the chain, in its default row groups
  and in groups of one block.  A full tile row and an nvec task -- whose extra rows read the W the sweep leaves -- ride beside the
  nine-block task; each run per task against the reference, and the stages show which back end ran."""
  case = next(c for c in dc.GROUP_S if c.kind == 'ekl')
  run, stages = _evaluate_under(gpu_ctx, case, dict(opts, lookahead=2))
  if opts['sweep']:
    assert 'sweep_tail' in stages and 'lauum' not in stages, stages
  else:
    assert 'lauum' in stages and 'sweep_tail' not in stages, stages
  _note('S options', *_check(case, run, dc.reference(case), 'options ' + str(opts)))


@pytest.mark.parametrize('kind', dc.KINDS)
def test_smaller_case_after_the_largest_equals_a_fresh_context(gpu_ctx, kind):
  """The workspaces are pooled, grow-only and poisoned (conftest: hbo_tune 'poison'): a case after a larger one of other shapes -- a full
  tile row after the mixed batch, then the first nvec shape -- must not read what that one left."""
  big = next(c for c in dc.GROUP_D if c.kind == kind and c.kname == 'matern52')
  smalls = [next(c for c in dc.GROUP_A if c.kind == kind and c.tasks == ((70, m),)) for m in (127, 128)]
  _evaluate(big, gpu_ctx)
  second = [_evaluate(c, gpu_ctx) for c in smalls]
  fresh = nat.Context(gpu_ctx.device)
  try:
    first = [_evaluate(c, fresh) for c in smalls]
  finally:
    fresh.close()
  for c, a, b in zip(smalls, second, first):
    assert np.isfinite(a.total) and (a.total0, a.per0, a.total, a.per) == (b.total0, b.per0, b.total, b.per), c.id
    ga, gb = helpers.flatten(a.grad), helpers.flatten(b.grad)
    assert np.isfinite(ga).all() and np.array_equal(ga, gb), c.id


def test_zz_worst_ratio_per_group():
  """Prints what this run measured per group (the source of RATIOS_MEASURED); asserts nothing the tests above have not."""
  for group in sorted(_WORST):
    v, g, ab = _WORST[group]
    print(f'DIVERGENCE group {group}: value {v:.3e} grad {g:.3e}' + (f' a/b {ab:.3e}' if ab else ''))
  assert all(max(w) <= 1.0 for w in _WORST.values())
