"""tests/divergence_cases.py judged on its own, on the CPU: the case list covers both sides of the column edge m + 1 = 128 and of the row
edge n = 128; the fp64 reference agrees with the longdouble restatement to a tenth of the bound the device is held to (a condition of the
cases, not a measurement of the device); every mutant of MUTANTS exceeds the GPU tier's bounds; the oracle's analytic gradient agrees
with central differences."""
import numpy as np
import pytest

import divergence_cases as dc
import helpers
from oracle import hyperbo_oracle as o

LD = np.longdouble


def _shapes(cases):
  return {t for c in cases for t in c.tasks}


def test_case_list_covers_the_edges_named_in_its_docstring():
  ids = [c.id for c in dc.CASES]
  assert len(set(ids)) == len(ids)
  assert all(len({c.kind for c in dc.CASES if c.data_id == d and c.dtype == t}) == 2 for d, t in {(c.data_id, c.dtype) for c in dc.CASES})   # both kinds, always
  assert _shapes(dc.GROUP_A) == {(n, m) for n in (70, 150) for m in (1, 2, 126, 127, 128, 129, 257)}
  assert _shapes(dc.GROUP_B) == {(n, m) for m in (3, 130) for n in (1, 2, 127, 128, 129, 257)}
  assert _shapes(dc.GROUP_C) == {(129, 127), (129, 128)}
  fams = {(c.kernel_name, c.mname) for c in dc.GROUP_C}
  assert fams == ({(k, 'zero') for k in helpers.KERNELS} | {(k + '_mlp', 'linear_mlp') for k in helpers.KERNELS} |
                  {('squared_exponential_kumar', 'constant'), ('matern52_kumar', 'linear'), ('dot_product_kumar', 'zero')})
  assert all({t for c in dc.GROUP_C if (c.kernel_name, c.mname) == f for t in c.tasks} == {(129, 127), (129, 128)} for f in fams)
  assert all(c.tasks == ((300, 2), (150, 127), (140, 128), (70, 257), (1, 130), (40, 1)) for c in dc.GROUP_D)
  assert {(c.kernel_name, c.mname) for c in dc.GROUP_D} == {('matern52', 'constant'), ('dot_product_mlp', 'linear_mlp')}
  e = [c for c in dc.GROUP_E]
  assert all(c.dtype == 'fp32' for c in e) and all(c.dtype == 'fp64' for c in dc.FP64_CASES)
  assert {c.tasks for c in e if c.kname == 'matern52' and not c.mlp} == {((150, 127),), ((150, 128),), ((150, 257),)}
  assert {c.tasks for c in e if c.mname == 'constant'} == {((n, m),) for n in (128, 129) for m in (3, 130)}
  assert {(c.kernel_name, c.mname) for c in e if len(c.tasks) > 1} == {('squared_exponential', 'zero'), ('matern52_mlp', 'linear_mlp')}
  assert {c.special for c in dc.GROUP_F} == {'zero_mean', 'identical', ''} and ((129, 1),) in {c.tasks for c in dc.GROUP_F}
  # both sides of m + 1 = 128 (the tile row: naug = 127, the FULL tile row naug = 128; the nvec path from m = 128) and of n = 128
  for group in (dc.GROUP_A, dc.GROUP_C, dc.GROUP_D):
    ms = {m for _, m in _shapes(group)}
    assert 127 in ms and 128 in ms
  ns = {n for n, _ in _shapes(dc.GROUP_B)}
  assert {127, 128, 129} <= ns and {1, 2, 257} <= ns
  assert (1, 130) in _shapes(dc.GROUP_B) and (1, 130) in _shapes(dc.GROUP_D)          # n = 1 on the nvec path
  assert all(n <= 300 and m <= 257 for n, m in _shapes(c for c in dc.CASES if c.group != 'S'))
  assert all(c.tasks == ((1030, 2), (150, 127), (140, 128)) for c in dc.GROUP_S)      # nine blocks: the one size beyond 300, for use_sweep


def test_inputs_are_seeded_by_the_id_and_shared_between_kinds_and_dtypes():
  a = dc.GROUP_A[0]
  assert dc.inputs(a) is dc.inputs(a._replace(kind='euc'))
  x64, y64 = dc.inputs(a).tasks[0]
  x32, y32 = dc.inputs(a._replace(dtype='fp32')).tasks[0]
  assert x32.dtype == np.float32 and np.array_equal(x32, x64.astype(np.float32)) and np.array_equal(y32, y64.astype(np.float32))
  b = dc.GROUP_A[2]
  assert b.data_id != a.data_id and not np.array_equal(dc.inputs(b).tasks[0][0][:1], x64[:1])


@pytest.mark.parametrize('case', [c for c in dc.GROUP_F if c.special], ids=lambda c: c.id)
def test_degenerate_cases_are_degenerate_exactly(case):
  ref = dc.reference(case)
  model, tasks = dc.inputs(case)
  for x, y in tasks:
    mu0 = np.array([sum(float(v) for v in row) / y.shape[1] for row in y])       # the sequential sum of hbo_dataset_create
    if case.special == 'zero_mean':
      assert np.all(mu0 == 0) and np.all(np.mean(y, axis=1) == 0)
    else:
      assert np.array_equal(mu0, y[:, 0]) and np.all(y - mu0[:, None] == 0)
  if case.special == 'zero_mean':
    assert ref.terms[0]['mahalanobis' if case.kind == 'ekl' else 'dnorm'] == 0.0
    mean_leaves = {'constant': ['constant'], 'linear_mlp': ['linear_mean/kernel', 'linear_mean/bias'], 'zero': []}[case.mname]
    leaves = dict(helpers.tree_leaves(ref.grad_sum))
    assert all(np.all(leaves[p] == 0) for p in mean_leaves), 'the reference gradient of the mean is exactly zero at d = 0'
    assert all(np.isfinite(v).all() for v in leaves.values())
  else:
    assert ref.terms[0]['tr'] == 0.0 if case.kind == 'ekl' else ref.terms[0]['fnorm'] > 0


@pytest.mark.parametrize('case', dc.FP64_CASES, ids=lambda c: c.id)
def test_fp64_reference_agrees_with_longdouble_to_a_tenth_of_the_bound(case):
  """A condition on the cases (their noise and length-scales), checked here: COND_BOUND * S_k per task, per term and for the value."""
  ref, ld = dc.reference(case), dc.reference_ld(case)
  for k, (terms, s) in enumerate(zip(ref.terms, ref.scales)):
    assert set(terms) == set(ld[k]) and all(v.dtype == LD for v in ld[k].values())
    errs = {name: float(abs(LD(terms[name]) - ld[k][name])) for name in terms}
    errs['value'] = float(abs(LD(ref.values[k]) - sum(ld[k].values())))
    assert s > 0 and all(e <= dc.COND_BOUND * s for e in errs.values()), (case.tasks[k], {n: e / s for n, e in errs.items()})
    # and the float64 restatement of the same formulas is within the bound: what the mutants are changed lines of
    assert abs(float(dc.restate_value(case, k, np.float64)) - ref.values[k]) <= 0.1 * dc.FP64_VALUE * s


@pytest.mark.parametrize('case', dc.GROUP_E, ids=lambda c: c.id)
def test_fp32_bounds_come_from_the_float32_restatement(case):
  """The float32 restatement is finite, its error is of fp32 size (not a broken restatement that would make any bound pass), and the
  fp64 reference on the rounded inputs agrees with longdouble far below the bound."""
  ref, ld, bounds, lv = dc.reference(case), dc.reference_ld(case), dc.value_bounds(case), dc.f32_levels(case)
  eps32 = float(np.finfo(np.float32).eps)
  for k, s in enumerate(ref.scales):
    n = case.tasks[k][0]
    assert np.isfinite(lv[k]) and lv[k] <= 64 * n * eps32 * s, (case.tasks[k], lv[k] / s)
    assert bounds[k] <= (4 * 64 * n + 8) * eps32 * s
    assert float(abs(LD(ref.values[k]) - sum(ld[k].values()))) <= 1e-3 * bounds[k]


MUTANT_CASES = ([c for c in dc.GROUP_A if c.tasks[0][0] == 70] + [c for c in dc.GROUP_D if c.kname == 'matern52'] + dc.GROUP_F +
                [c for c in dc.GROUP_E if c.tasks in (((150, 127),), ((150, 128),))])


@pytest.mark.parametrize('mutant', sorted(dc.MUTANTS))
def test_every_mutant_exceeds_a_bound(mutant):
  hit = {c.id: dc.mutant_ratio(c, mutant) for c in MUTANT_CASES if dc.applicable(c, mutant)}
  assert hit, 'no case the mutant applies to'
  print(f'DIVERGENCE mutant {mutant}: beyond the bound on {sum(r > 1 for r in hit.values())} of {len(hit)} cases, least ratio {min(hit.values()):.3g}')
  assert any(r > 1 for r in hit.values()), hit
  fp64 = {i: r for i, r in hit.items() if i.endswith('fp64')}
  if mutant not in ('no_guard',):
    assert all(r > 1 for r in fp64.values()), 'an applicable fp64 case does not see it: ' + str({i: r for i, r in fp64.items() if not r > 1})
  if mutant in ('row_127', 'cols_ge_128'):
    # the small shapes are enough: a single task with m <= 129 already shows a dropped row, in both kinds and in fp32
    small = {c.id: hit[c.id] for c in MUTANT_CASES if c.id in hit and len(c.tasks) == 1 and c.tasks[0][1] <= 129 and not c.special}
    assert {c.kind for c in MUTANT_CASES if c.id in small} == {'ekl', 'euc'} and all(r > 1 for r in small.values()), small
    assert mutant != 'row_127' or any(i.endswith('fp32') for i in small)
  if mutant == 'no_guard':
    assert all(r == np.inf for r in hit.values()), hit       # NaN in a mean leaf (the constant, the linear weights)


def test_no_guard_mutant_needs_a_mean_leaf():
  """Under the zero mean function d f / d mu reaches no leaf: only the cases whose mean has parameters can show a missing guard."""
  zm = [c for c in dc.GROUP_F if c.special == 'zero_mean' and c.kind == 'euc']
  assert {c.mname for c in zm} == {'zero', 'constant', 'linear_mlp'}


def _central_differences(case, h=1e-5):
  model64 = dc.cast(dc.inputs(case).model, np.float64)
  x, y = dc.inputs(case).tasks[0]
  flat = helpers.flatten(model64)
  g = np.zeros_like(flat)
  for i in range(flat.size):
    hi, lo = flat.copy(), flat.copy()
    hi[i] += h; lo[i] -= h
    g[i] = (dc.oracle_task(case, helpers.unflatten_like(model64, hi), x, y)[0] - dc.oracle_task(case, helpers.unflatten_like(model64, lo), x, y)[0]) / (2 * h)
  return helpers.unflatten_like(model64, g)


@pytest.mark.parametrize('case', [c for c in dc.GROUP_A if c.tasks in (((70, 127),), ((70, 128),))] +
                         [c for c in dc.GROUP_C if c.kname == 'dot_product' and c.mlp and c.tasks == ((129, 128),)], ids=lambda c: c.id)
def test_oracle_gradient_agrees_with_central_differences(case):
  """One case per kind on each side of the column edge (and the dot product on the MLP basis, whose leaves A does not have)."""
  fd = _central_differences(case)
  ratio, leaf = dc.grad_ratio(dc.reference(case).grads[0], fd, 1e-6)
  assert ratio <= 1.0, (leaf, ratio)


@pytest.mark.parametrize('case', [c for c in dc.GROUP_C if c.kumar and c.tasks == ((129, 128),)], ids=lambda c: c.id)
def test_ab_central_differences_are_stable_in_the_step(case):
  """The central differences the analytic a / b reference is held to (AB_FD_TOL) do not move by more than a tenth of that bound when the
  step is doubled."""
  ratios = dc.ab_errors(dc.ab_central_differences(case, 2 * dc.AB_FD_STEP), dc.ab_reference(case))
  assert max(ratios.values()) <= 0.1, ratios


@pytest.mark.parametrize('case', [c for c in dc.GROUP_C if c.kumar and c.tasks == ((129, 128),)], ids=lambda c: c.id)
def test_analytic_ab_leaves_agree_with_central_differences(case):
  """What the device's a / b leaves are held to (ab_analytic, at AB_TOL): the oracle's kernel adjoint through dK/dw and dw/da, dw/db,
  within AB_FD_TOL of the central differences.  The adjoint that captures d f / d K1 is the oracle's own: every other leaf comes out to
  the bit."""
  ratios = dc.ab_errors(dc.ab_analytic(case), dc.ab_reference(case))
  assert max(ratios.values()) <= 1.0, ratios
  model64 = dc.cast(dc.inputs(case).model, np.float64)
  x, y = dc.inputs(case).tasks[0]
  plain, hooked = dc.oracle_task(case, model64, x, y), dc.oracle_task(case, model64, x, y, dc._capturing_adjoint({}))
  assert plain[0] == hooked[0] and all(np.array_equal(a, b) for (_, a), (_, b) in zip(helpers.tree_leaves(plain[1]), helpers.tree_leaves(hooked[1])))


def test_value_bounds_are_per_task_and_relative_to_the_term_scale():
  case = dc.GROUP_D[0]
  ref, bounds = dc.reference(case), dc.value_bounds(case)
  assert len(bounds) == len(case.tasks) and all(b == dc.FP64_VALUE * s for b, s in zip(bounds, ref.scales))
  assert all(abs(sum(t.values()) - v) <= 1e-12 * s for t, v, s in zip(ref.terms, ref.values, ref.scales))
  sub = dc.reference_subsampled(case)
  rows = dc.subsample_rows(case)
  assert sorted(k for k, r in rows.items() if r is not None) == [0, 1, 2] and all(len(set(r.tolist())) == len(r) for r in rows.values() if r is not None)
  assert sub.values[3:] == ref.values[3:] and all(a != b for a, b in zip(sub.values[:3], ref.values[:3]))
