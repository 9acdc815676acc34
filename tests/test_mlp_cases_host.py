"""tests/mlp_cases.py judged on its own, on the CPU: the case table reaches every edge it names (the four thread counts of the weight-
gradient kernels from both sides, three row chunks with tasks ending in the first and the second, depths 1 / 2 / 3 / 8, one-column layers,
d = 1 and 256); tanh saturation stays under 10 % per layer; no MLP leaf of the reference is zero; the oracle agrees with the longdouble
restatement to 1 % of every fp64 bound; the float32 restatement stays under a quarter of every fp32 bound; every mutant of MUTANTS is
rejected by a bound of the GPU tier, and every MLP leaf of every case is the rejecting leaf of some mutant."""
import numpy as np
import pytest

import helpers
import mlp_cases as mc

LD = np.longdouble
RUNS = [(c, s) for c in mc.CASES for s in mc.SIZES]
RUN_IDS = [f'{c.id}-{s}' for c, s in RUNS]


def test_case_table_reaches_the_edges():
  ids = [c.id for c in mc.CASES]
  assert len(set(ids)) == len(ids) and len({c.feats for c in mc.CASES}) == len(ids)
  feats = {c.feats for c in mc.CASES}
  # last layers on both sides of each thread-count edge under a hidden layer of 12, hidden layers on the same edges over a last layer of 33
  assert {(12, f) for f in (1, 63, 64, 65, 128, 129, 192, 193, 256)} <= feats
  assert {(h, 33) for h in (65, 129, 193, 256)} <= feats and (256, 256) in feats
  assert [mc.threads(f) for f in (1, 63, 64, 65, 128, 129, 192, 193, 256)] == [64, 64, 64, 128, 128, 192, 192, 256, 256]
  for pos in (-1, 0):
    classes = {}
    for c in mc.CASES:
      if len(c.feats) == 2:
        classes.setdefault(mc.threads(c.feats[pos]), set()).add(c.feats[pos])
    assert sorted(classes) == [64, 128, 192, 256], (pos, classes)
    widths = set().union(*classes.values())
    assert all({e, e + 1} <= widths or pos == 0 for e in (64, 128, 192)) and {65, 129, 193, 256} <= widths
  # depths: 1 (no din on the only layer), 2, an odd depth with a hidden layer, 8 (HBO's limit) with alternating widths
  assert {(256,), (65,)} <= feats and (256, 1, 256, 1, 256, 1, 256, 192) in feats
  assert {len(c.feats) for c in mc.CASES} == {1, 2, 3, 8}
  assert any(len(c.feats) % 2 == 1 and len(c.feats) > 1 for c in mc.CASES)
  # one-column layers and the input widths 1 and 256
  assert mc.BY_FEATS[(1, 256)].d == 1 and mc.BY_FEATS[(193, 1)].d == 256 and (12, 1) in feats
  assert [c.kname for c in mc.CASES].count('dot_product') == 1 and mc.BY_FEATS[(128, 193)].kname == 'dot_product'
  assert {c.ls for c in mc.CASES} == {'ard', 'scalar', 'none'} and {c.kname for c in mc.CASES} == set(helpers.KERNELS)
  assert all(1 <= f <= 256 for c in mc.CASES for f in c.feats) and all(len(c.feats) <= 8 for c in mc.CASES)
  # row chunks: three of them; tasks that end in the first (at 129, one short of the edge, on the edge), the second and the third
  blocked, small = mc.SIZES['blocked'], mc.SIZES['small']
  assert set(blocked) == {129, 255, 256, 257, 513} and set(small) == {128, 90, 33, 2}
  assert max(mc.chunks(n) for n in blocked) == 3
  assert {n: mc.last_chunk(n) for n in blocked} == {129: 0, 255: 0, 256: 0, 257: 1, 513: 2}
  assert min(blocked) > mc.SMALL_LIMIT >= max(small) and len(set(blocked)) > 1 and len(set(small)) > 1
  assert max(max(v) for v in mc.SIZES.values()) == 513


def test_inputs_are_shared_between_dtypes_and_size_sets():
  c = mc.CASES[0]
  a, b = mc.inputs(c, 'blocked', 'fp64'), mc.inputs(c, 'blocked', 'fp32')
  assert mc.inputs(c, 'blocked', 'fp64') is a
  assert all(np.array_equal(x32, x64.astype(np.float32)) and x32.dtype == np.float32 for (x32, _), (x64, _) in zip(b.tasks, a.tasks))
  assert np.array_equal(helpers.flatten(mc.inputs(c, 'small', 'fp64').model), helpers.flatten(a.model))
  assert [x.shape[0] for x, _ in a.tasks] == list(mc.SIZES['blocked'])


@pytest.mark.parametrize('case,sizes', RUNS, ids=RUN_IDS)
def test_saturation_and_nonzero_leaves(case, sizes):
  for dtype in mc.DTYPES:
    ref = mc.reference(case, sizes, dtype)
    pooled = [np.concatenate([acts[l] for acts in ref.acts]) for l in range(len(case.feats) + 1)]      # per layer over the batch's rows
    assert max(mc.saturation(pooled)) < mc.SATURATION_SHARE, (dtype, mc.saturation(pooled))
    leaves = dict(helpers.tree_leaves(ref.grad))
    gmax = max(float(np.max(np.abs(v))) for v in leaves.values())
    for p in mc.mlp_leaf_paths(case):
      assert np.isfinite(leaves[p]).all() and np.max(np.abs(leaves[p])) > 0, p
      assert 0 < ref.scales[p] and np.max(np.abs(leaves[p])) <= ref.scales[p] * (1 + 1e-12), p
    small = {p: float(np.max(np.abs(leaves[p])) / gmax) for p in mc.mlp_leaf_paths(case) if np.max(np.abs(leaves[p])) < 1e-3 * gmax}
    print(f'MLP {case.id} {sizes} {dtype}: leaves under the 1e-3 floor: {small}')


@pytest.mark.parametrize('case,sizes', RUNS, ids=RUN_IDS)
def test_oracle_agrees_with_longdouble_to_a_hundredth_of_the_fp64_bounds(case, sizes):
  """Features, dW, db, din per task and the batch's MLP leaves, for the oracle's own dF; and the float64 restatement -- what the mutants
  are wrong variants of -- and the value from the features likewise."""
  ref, (model, tasks) = mc.reference(case, sizes, 'fp64'), mc.inputs(case, sizes, 'fp64')
  wts, share = mc.weights(model, LD), mc.REFERENCE_SHARE
  floor = 1e-3 * max(float(np.max(np.abs(v))) for _, v in helpers.tree_leaves(ref.grad)) * len(tasks)     # of a task's share of the mean
  per = []
  for k, (x, y) in enumerate(tasks):
    acts = mc.forward(wts, x, LD)
    grads, din, _ = mc.backward(wts, acts, ref.dF[k], LD)
    per.append(grads)
    for a, b in zip(acts, ref.acts[k]):
      assert float(np.max(np.abs(a - b))) <= share * mc.FP64_VALUE_TOL           # |feature| <= 1
    assert float(np.max(np.abs(din - ref.din[k]))) <= share * mc.FP64_GRAD_TOL * float(np.max(np.abs(ref.din[k])))
    _, _, dzs = mc.backward(mc.weights(model), ref.acts[k], ref.dF[k], np.float64)
    for l, (dW, db) in enumerate(grads):
      o_ = ref.task_mlp[k][f'Dense_{l}']
      tk = float(np.max(np.abs(ref.acts[k][l]).T @ np.abs(dzs[l])))        # the task's own T_leaf
      tb = float(np.max(np.abs(dzs[l]).sum(axis=0)))
      assert float(np.max(np.abs(dW - o_['kernel']))) <= share * mc.FP64_GRAD_TOL * max(float(np.max(np.abs(o_['kernel']))), min(tk, floor))
      assert float(np.max(np.abs(db - o_['bias']))) <= share * mc.FP64_GRAD_TOL * max(float(np.max(np.abs(o_['bias']))), min(tb, floor))
    v = mc.nll_from_features(case, model, ref.acts[k][-1], y)
    assert mc.value_ratio(v, ref.per_task[k], mc.FP64_VALUE_TOL) <= 10 * share, (k, v, ref.per_task[k])
  ld = mc.leaf_ratios(mc.with_mlp(ref.grad, mc.mlp_tree(per, len(tasks))), ref.grad, mc.FP64_GRAD_TOL, ref.scales)
  f64 = mc.leaf_ratios(mc.restated_tree(case, sizes, 'fp64'), ref.grad, mc.FP64_GRAD_TOL, ref.scales)
  print(f'MLP {case.id} {sizes}: oracle against longdouble {mc.worst_leaf(ld)}, float64 restatement {mc.worst_leaf(f64)}')
  assert max(ld.values()) <= share and max(f64.values()) <= share, (ld, f64)


@pytest.mark.parametrize('case,sizes', RUNS, ids=RUN_IDS)
def test_float32_yardstick_is_under_a_quarter_of_the_fp32_bounds(case, sizes):
  """The forward and backward pass in float32 throughout (the device sums its gradients in fp64: it can only do better) on the oracle's
  dF, per leaf; and the value from the float32 features."""
  ref, (model, tasks) = mc.reference(case, sizes, 'fp32'), mc.inputs(case, sizes, 'fp32')
  ratios = mc.leaf_ratios(mc.restated_tree(case, sizes, 'fp32', np.float32), ref.grad, mc.FP32_GRAD_TOL, ref.scales)
  wts = mc.weights(model, np.float32)
  vr = max(mc.value_ratio(mc.nll_from_features(case, model, mc.forward(wts, x, np.float32)[-1], y), v, mc.FP32_VALUE_TOL)
           for (x, y), v in zip(tasks, ref.per_task))
  print(f'MLP {case.id} {sizes}: float32 yardstick: leaf {mc.worst_leaf(ratios)}, value {vr:.3g}')
  assert max(ratios.values()) <= mc.YARDSTICK_SHARE, ratios
  assert vr <= mc.YARDSTICK_SHARE


_REJECTED = {}     # (case id, sizes, dtype) -> {leaf: mutant that rejects it}: filled by test_every_mutant_is_rejected, in file order


@pytest.mark.parametrize('mutant', [m for m in mc.MUTANTS if m != 'sample0_weights'])
def test_every_mutant_is_rejected(mutant):
  hit = {}
  for case, sizes in RUNS:
    if not mc.applicable(case, sizes, mutant):
      continue
    for dtype in mc.DTYPES:
      ratios = mc.mutant_ratios(case, sizes, dtype, mutant)
      hit[(case.id, sizes, dtype)] = max(ratios.values())
      if mutant not in mc.VALUE_MUTANTS:
        seen = _REJECTED.setdefault((case.id, sizes, dtype), {})
        for p, r in ratios.items():
          if r > 1:
            seen.setdefault(p, mutant)
  assert hit, 'no case the mutant applies to'
  print(f'MLP mutant {mutant}: beyond a bound on {sum(r > 1 for r in hit.values())} of {len(hit)} runs, least ratio {min(hit.values()):.3g}')
  assert any(r > 1 for r in hit.values()), hit
  assert any(r > 1 for k, r in hit.items() if k[2] == 'fp64') and (mutant == 'chunk_twice' or any(r > 1 for k, r in hit.items() if k[2] == 'fp32')), hit
  if mutant in ('pingpong_odd', 'pingpong_even'):
    assert all(r > 1 for r in hit.values()), hit


def test_the_column_mutants_are_seen_on_the_blocked_wide_cases_in_both_dtypes():
  """What the sensitivity check of the device tier rests on: a weight gradient that stops at column 64 fails every blocked case with a
  layer wider than 64, fp64 and fp32."""
  for case in mc.CASES:
    if max(case.feats) > 64:
      for dtype in mc.DTYPES:
        assert max(mc.mutant_ratios(case, 'blocked', dtype, 'cols_ge_64').values()) > 1, (case.id, dtype)


def test_sample0_weights_is_rejected():
  for case in mc.SAMPLE_CASES:
    for shape in mc.SAMPLE_SIZES:
      for dtype in mc.DTYPES:
        good, bad = mc.sample_values(case, shape, dtype), mc.sample_values(case, shape, dtype, 'sample0_weights')
        assert np.array_equal(good[0], bad[0])
        tol = mc.SAMPLE_TOL[dtype][1]
        assert all(np.all(np.abs(bad[s] - good[s]) > tol * np.abs(good[s])) for s in range(1, mc.SAMPLE_COUNT)), (case.id, shape, dtype)


def test_every_mlp_leaf_of_every_case_is_the_rejecting_leaf_of_some_mutant():
  """Reads what test_every_mutant_is_rejected recorded (same file, run before this one; run alone it recomputes)."""
  if not _REJECTED:
    for m in mc.MUTANTS:
      if m not in mc.VALUE_MUTANTS:
        test_every_mutant_is_rejected(m)
  for case, sizes in RUNS:
    for dtype in mc.DTYPES:
      seen = _REJECTED.get((case.id, sizes, dtype), {})
      missing = [p for p in mc.mlp_leaf_paths(case) if p not in seen]
      assert not missing, (case.id, sizes, dtype, missing)
  print('MLP leaf -> rejecting mutant, per run:')
  for key in sorted(_REJECTED):
    print('  ', key, {p.replace('mlp_params/', ''): m for p, m in _REJECTED[key].items()})


def test_leaf_ratios_is_the_rule_of_assert_grad_close():
  """On a case: both accept the reference and reject a mutant, with the same worst leaf.  On a made-up tree whose small leaf has terms
  1e-6 of the largest leaf: a leaf that is wholly wrong passes the default floor at the fp32 tolerance and fails with its term scale."""
  case, sizes = mc.BY_FEATS[(256, 1, 256, 1, 256, 1, 256, 192)], 'small'
  ref = mc.reference(case, sizes, 'fp64')
  bad = mc.restated_tree(case, sizes, 'fp64', mutant='no_bias_row')
  helpers.assert_grad_close(ref.grad, ref.grad, mc.FP64_GRAD_TOL, leaf_scales=ref.scales)
  ratio, leaf = mc.worst_leaf(mc.leaf_ratios(bad, ref.grad, mc.FP64_GRAD_TOL, ref.scales))
  with pytest.raises(AssertionError, match=leaf):
    helpers.assert_grad_close(bad, ref.grad, mc.FP64_GRAD_TOL, leaf_scales=ref.scales)
  assert ratio > 1
  tree = {'lengthscale': np.array([1.0, -0.5]), 'mlp_params': {'Dense_0': {'kernel': np.full((2, 3), 1e-6), 'bias': np.full(3, 0.2)}}}
  wrong = {'lengthscale': tree['lengthscale'], 'mlp_params': {'Dense_0': {'kernel': -tree['mlp_params']['Dense_0']['kernel'], 'bias': np.full(3, 0.2)}}}
  scales = {'mlp_params/Dense_0/kernel': 2e-6, 'mlp_params/Dense_0/bias': 0.5}
  helpers.assert_grad_close(wrong, tree, mc.FP32_GRAD_TOL)                          # 2e-6 <= 2.5e-3 * 1e-3: hidden under the floor
  with pytest.raises(AssertionError, match='Dense_0/kernel'):
    helpers.assert_grad_close(wrong, tree, mc.FP32_GRAD_TOL, leaf_scales=scales)
  r = mc.leaf_ratios(wrong, tree, mc.FP32_GRAD_TOL, scales)
  assert r['mlp_params/Dense_0/kernel'] == pytest.approx(2e-6 / (mc.FP32_GRAD_TOL * 2e-6)) and r['mlp_params/Dense_0/bias'] == 0 and r['lengthscale'] == 0
  assert mc.leaf_ratios(wrong, tree, mc.FP32_GRAD_TOL)['mlp_params/Dense_0/kernel'] == pytest.approx(2e-6 / (mc.FP32_GRAD_TOL * 1e-3))
  # a term scale above the floor changes nothing
  assert mc.leaf_ratios(wrong, tree, mc.FP32_GRAD_TOL, {'mlp_params/Dense_0/kernel': 0.5}) == mc.leaf_ratios(wrong, tree, mc.FP32_GRAD_TOL)
