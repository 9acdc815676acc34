"""CPU tier of the row-append tests: tests/append_cases.py judged on its own, so that tests/test_gpu_cache_append.py cannot pass
vacuously (as test_acq_grad_cases_host.py does for its tier):

  * the case list holds the shapes the tier is about: two, five and nine 128-row blocks, the append that ends at npad exactly and the
    row that no longer fits, a second 512-row chunk of W^T l, 60 single-row calls, the registry, Kumaraswamy, three target columns;
  * the NumPy restatement of append_row_kernel's recurrences that the mutants are made from IS the reference (the oracle's
    from-scratch factorisation) on every case and after every call, at the bounds of the GPU tier;
  * every mutant -- one changed line of the restatement each -- is at least MUTANT_FACTOR = 100 fp64 bounds away from the reference
    in some part after some call of EVERY fp64 case it applies to, and beyond 5e-4 of an array's largest entry on the fp32 cases (the GPU
    test asserts again that its measured fp32 / drift bounds see them: append_cases.unseen_mutants);
  * the reference in np.longdouble agrees with the fp64 oracle to a hundredth of the fp64 bounds: the reference's own error is not
    what the bounds measure."""
import numpy as np
import pytest

import append_cases as A

IDS = lambda c: c.id


def _worst(case, got, ref):
  w = {}
  for g, r in zip(got, ref):
    for k, v in A.ratios(g, r, case.n0).items():
      w[k] = max(w.get(k, 0.0), v)
  return w


def test_case_list_covers_what_the_gpu_tier_needs():
  ids = [c.id for c in A.CASES + A.FP32_CASES]
  assert len(set(ids)) == len(ids)
  blocks = lambda c: -(-c.n0 // A.TILE)
  assert all(blocks(c) >= 2 for c in A.CASES)                                       # no case is the one-block test again
  assert [(c.n0, c.calls) for c in A.TWO_BLOCKS] == [(129, (1,)), (200, (7, 1, 1))]
  assert (A.EDGE.n0, A.EDGE.calls) == (250, (6, 1)) and A.EDGE.sizes[0][1] == 256 and A.EDGE.in_place == [True, False]
  assert [(c.n0, c.calls) for c in A.FIVE_BLOCKS] == [(513, (3,)), (600, (40,))] and A.FIVE_BLOCKS[1].n_total == 640
  assert all(blocks(c) == 5 for c in A.FIVE_BLOCKS)                                 # npad = 640: a second 512-row chunk
  assert (A.NINE_BLOCKS.n0, A.NINE_BLOCKS.calls, A.NINE_BLOCKS.M) == (1030, (5,), 40) and blocks(A.NINE_BLOCKS) == 9
  assert A.DRIFT.n0 == 130 and A.DRIFT.calls == (1,) * 60
  assert all(all(c.in_place) for c in A.CASES + A.FP32_CASES if c.name != 'edge')   # everything else is appended in place
  reg = A.REGISTRY_CASES
  assert all((c.n0, c.calls) == (200, (5,)) for c in reg) and len(reg) == 6
  assert {c.kernel_name for c in reg} == {'squared_exponential', 'matern52_mlp', 'matern32', 'dot_product_mlp', 'squared_exponential_kumar', 'matern52'}
  assert {c.mname for c in reg} == {'constant', 'linear_mlp', 'linear', 'zero'} and [c.mcols for c in reg] == [1, 1, 1, 1, 1, 3]
  assert all(c.d == 3 and c.M == 40 for c in A.CASES)
  assert {(c.name, c.n0) for c in A.FP32_CASES} == {('two', 129), ('two', 200), ('five', 513), ('five', 600), ('drift', 130)}
  assert [(c.n0, c.calls[0]) for c in A.ONCE_CASES] == [(200, 7), (600, 40)]
  live = set()
  for c in A.CASES:
    live |= set(A.MUTANTS) - A.not_applicable(c)
  assert live == set(A.MUTANTS)                                                      # every mutant applies somewhere


@pytest.mark.parametrize('case', A.CASES + A.FP32_CASES, ids=IDS)
def test_inputs_are_what_the_checks_assume(case):
  model, x, y, xq = A.inputs(case)
  assert x.dtype == case.np_dtype and x.shape == (case.n_total, case.d) and y.shape == (case.n_total, case.mcols) and xq.shape == (case.M, case.d)
  assert np.array_equal(xq[:3], x[A.new_queries(case)]) and all(i >= case.n0 for i in A.new_queries(case))
  if case.mcols > 1:      # the appended targets differ per column
    assert all(np.abs(y[case.n0:, a] - y[case.n0:, 0]).min() > 1e-3 for a in range(1, case.mcols))
  ref = A.reference(case)
  assert len(ref) == len(case.calls) and [r.n for r in ref] == [n1 for _, n1 in case.sizes]
  for r in ref:
    assert np.isfinite(r.mu).all() and np.abs(r.mu).max() > 0.1 and r.var.min() > 0


@pytest.mark.parametrize('case', A.CASES + A.FP32_CASES, ids=IDS)
def test_the_restatement_is_the_reference(case):
  w = _worst(case, A.restate(case), A.reference(case))
  assert max(w.values()) <= 0.1, w       # (of the GPU tier's fp64 bounds)
  old = A.initial(case).chol
  assert np.array_equal(A.restate(case)[0].chol[:case.n0, :case.n0], old)            # an append leaves the old rows alone


@pytest.mark.parametrize('mutant', sorted(A.MUTANTS))
@pytest.mark.parametrize('case', A.CASES, ids=IDS)
def test_fp64_bounds_reject_every_mutant(case, mutant):
  if mutant in A.not_applicable(case):
    assert mutant in ('z', 'wtl_512', 'col0')
    # what not_applicable says, from the shape on its own: a single appended row, no row of W from 512 on, one target column
    assert {'z': case.n_total - case.n0 == 1, 'wtl_512': case.n_total <= 513, 'col0': case.mcols == 1}[mutant]
    return
  with np.errstate(invalid='ignore'):
    w = _worst(case, A.restate(case, mutant), A.reference(case))
  assert max(w.values()) >= A.MUTANT_FACTOR, (mutant, A.MUTANTS[mutant], w)


@pytest.mark.parametrize('case', A.FP32_CASES, ids=IDS)
def test_fp32_cases_see_every_mutant_well_above_fp32_rounding(case):
  """At a flat bound of 5e-4 of every array's largest entry -- what the suite allows an fp32 posterior mean or variance
  (test_posterior_at_few_candidates_split_along_k), several times what an fp32 factorisation of these sizes is off by -- every
  applicable mutant is still seen after some call.  The least visible: W^T l without the rows from 512 on at 513 +3, which moves kinvy
  by 8e-4 and nothing else by more than 7e-5."""
  flat = [{k: 5e-4 for k in A.PART_OF} for _ in case.calls]
  assert A.unseen_mutants(case, flat) == set()


@pytest.mark.parametrize('case', A.CASES, ids=IDS)
def test_longdouble_reference_agrees_with_the_fp64_oracle(case):
  assert np.finfo(np.longdouble).eps < 1e-18          # (x87 extended precision: 64-bit significand)
  ref = A.reference(case)
  calls = range(len(case.calls)) if len(case.calls) <= 3 else [0, len(case.calls) // 2, len(case.calls) - 1]
  for i in calls:
    r = A.ratios(ref[i], A.oracle_state_ld(case, case.sizes[i][1]), case.n0)
    assert max(r.values()) <= 0.01, (i, r)
