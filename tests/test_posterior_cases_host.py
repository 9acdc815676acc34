"""CPU tier of the streamed-posterior tests: tests/posterior_cases.py judged on its own, so that tests/test_gpu_posterior.py cannot pass
vacuously.  For every case of the exact tier (at 256 CUs, the MI355X's count):

  * the operands are integers, W is lower triangular, and the three sums that bound every partial sum of the route stay below 2^24: the
    result is exact in fp32 whatever the order;
  * the expected variance is r_q in {0, 1, 2, 3}, every value present where there are enough queries;
  * every 128 x 128 block of W is live: zeroing it changes colsq[i, q] for all but at most 1 % of the (block, query) pairs;
  * the route walked on the host (simulate: chunks, workspaces, K chunks, unrolled mean) gives the outputs of the definition (direct);
  * every mutant of the route changes an asserted output of the case that is named for it;
  * the host twin of post_plan puts every case on the route it is listed for.

Real-kernel tier: the two fp64 routes of the reference agree to a tenth of the bound applied to the device, per query and on every case,
and the heterogeneous queries span the orders of magnitude they are there for."""
import numpy as np
import pytest

import posterior_cases as P

CUS = 256
CASES = P.route_cases(CUS)
BY_NAME = {c.name: c for c in CASES}
IDS = lambda c: c.id
EXACT_FP32 = 2.0 ** 24


def _kchunk(case):
  return P.plan(case.n, case.M, case.post_chunk, CUS)['kchunk']


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_operands_are_exact_in_fp32(case):
  d = P.design(case.n, case.M)
  for a in (d.W, d.alpha, d.Kxq, d.mu0, d.r, d.kdiag):
    assert np.array_equal(a, np.rint(a)) and np.array_equal(a, a.astype(np.float32).astype(np.float64))
  assert not np.triu(d.W, 1).any() and np.all(np.isin(np.diag(d.W), (1.0, 2.0)))
  assert np.abs(d.W).max() == 2 and np.abs(d.Kxq).max() <= P.K_BOUND and np.abs(d.alpha).max() <= 3 and np.abs(d.mu0).max() <= 5
  v, s, m = P.magnitudes(d)
  print(f'{case.id}: max sum |W||Kxq| {v:g}, max sum colsq 2^{np.log2(s):.1f}, max sum |Kxq alpha| + |mu0| {m:g}')
  assert max(v, s, m) < EXACT_FP32
  # a bf16 / fp16 plane holds the operands whole: 8 and 11 significant bits
  assert np.abs(d.W).max() < 2 ** 8 and np.abs(d.Kxq).max() < 2 ** 8


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_expected_variance_is_r(case):
  d, ref = P.design(case.n, case.M), P.direct(case.n, case.M)
  assert np.array_equal(ref.var, d.r) and set(np.unique(d.r)) <= {0.0, 1.0, 2.0, 3.0}
  if case.M >= 100:
    assert set(np.unique(d.r)) == {0.0, 1.0, 2.0, 3.0}
  assert ref.colsq.shape == ref.mupart.shape == (d.nblk, case.M) and ref.mu.shape == ref.var.shape == (case.M,)
  assert np.array_equal(ref.mu, d.Kxq.T @ d.alpha + d.mu0)
  if case.M <= 512:   # the sparse product against the dense one
    assert np.array_equal(ref.colsq.sum(axis=0), ((d.W @ d.Kxq) ** 2).sum(axis=0))


@pytest.mark.parametrize('case', [c for c in CASES if c.M <= 512], ids=IDS)
def test_every_block_of_w_is_live(case):
  dead, total = P.dead_pairs(P.design(case.n, case.M))
  print(f'{case.id}: {dead} of {total} (block, query) pairs unchanged')
  assert dead <= 0.01 * total, f'{case.id}: {dead} of {total}'


@pytest.mark.parametrize('case', [c for c in CASES if c.route != 'resident' and c.name != 'plain_edge'], ids=IDS)
@pytest.mark.parametrize('dtype', ['fp64', 'fp32'])
def test_walked_route_gives_the_definition(case, dtype):
  out = P.simulate(case.n, case.M, case.post_chunk, _kchunk(case), dtype)
  assert out.differs(P.direct(case.n, case.M), True) == []


@pytest.mark.parametrize('mutant', P.MUTANTS)
@pytest.mark.parametrize('dtype', ['fp64', 'fp32'])
def test_mutant_is_seen_by_its_case(mutant, dtype):
  case = BY_NAME[P.MUTANT_CASE[mutant]]
  out = P.simulate(case.n, case.M, case.post_chunk, _kchunk(case), dtype, mutant)
  changed = out.differs(P.direct(case.n, case.M), case.single_chunk)
  print(f'{mutant} on {case.id} ({dtype}): changes {changed}')
  assert changed, f'{mutant} changes no asserted output of {case.id}'


def test_mutants_are_not_seen_everywhere():
  """The mutants are specific: where the route has no such step the outputs stay (a mutant that changed everything would prove nothing
  about the case named for it)."""
  one = BY_NAME['one_full']
  for mutant in ('ragged_k_dropped', 'squared_before_sum', 'mupart_tail_dropped', 'chunk_written_at_previous_q0',
                 'ragged_chunk_read_with_ldq_max', 'workspace_reused_one_chunk_early', 'colsq_row_reversed'):
    assert P.simulate(one.n, one.M, one.post_chunk, 0, 'fp64', mutant).differs(P.direct(one.n, one.M), True) == [], mutant
  k2 = BY_NAME['k2']   # 1100 = 8 * 128 + 76 rows: no scalar tail in any block
  assert P.simulate(k2.n, k2.M, k2.post_chunk, 2, 'fp64', 'mupart_tail_dropped').differs(P.direct(k2.n, k2.M), True) == []


@pytest.mark.parametrize('cus', [256, 304, 64])
def test_cases_reach_their_routes(cus):
  """The plan's host twin on the sizes the list derives from the CU count: every route of the issue is reached, on any device."""
  seen = set()
  for case in P.route_cases(cus):
    for dtype, form, kb in P.runs_of(case):
      p = P.plan(case.n, case.M, case.post_chunk, cus, dtype, form, kb)
      seen.add((case.route, p['form']))
      assert p['nchunks'] == -(-case.M // max(case.post_chunk, 128)) and p['nbuf'] == (2 if p['nchunks'] > 1 else 1)
      if case.route == 'splitk':
        assert p['kchunk'] == P.EXPECT_KCHUNK[case.name] and p['form'] == 0 and p['resident_chunks'] == 0
        assert p['nch'] == -(-(-(-case.n // 128)) // p['kchunk'])
      else:
        assert p['kchunk'] == 0 and p['resident_chunks'] == (1 if case.route == 'resident' else 0)
        want = 'mfma' if dtype == 'fp64' or form == 'mfma' else ('bf16x3' if form == 'bf16x3' or kb == 0 else 'f16x2')
        assert p['form'] == P.FORMS[want]
      if case.route != 'one_block':
        assert case.n > 128
  assert seen == {(r, f) for r in ('one_block', 'plain', 'resident') for f in (0, 1, 2)} | {('splitk', 0)}
  names = {c.name: c for c in P.route_cases(cus)}
  assert names['plain_streamed'].M > 3 * P.DEFAULT_CHUNK or cus < 256   # four chunks through two workspaces on the MI355X
  # both sides of the resident edge, one tile apart; the plain side of the split-K edge, one query beyond a tile boundary
  assert -(-names['resident'].M // 128) == names['plain_edge'].M // 128 + 1 and names['resident'].M % 128 == 128 - 57
  m = names['plain_streamed'].M
  assert P.plan(129, m - 1, P.DEFAULT_CHUNK, cus)['kchunk'] == 1 and P.plan(129, m, P.DEFAULT_CHUNK, cus)['kchunk'] == 0


def test_plan_twin_at_the_shapes_of_the_issue():
  assert P.plain_streamed_M(256) == 32641 and P.resident_Ms(256) == (14535, 14464)
  p = P.plan(129, 32641, 8192, 256)
  assert (p['nchunks'], p['nbuf'], p['kchunk'], p['direct_form']) == (4, 2, 0, 1)
  assert P.plan(100, 300, 128, 256)['nchunks'] == 3
  assert [P.plan(n, 130, 8192, 256)['kchunk'] for n in (300, 1100, 3100)] == [1, 2, 3]
  assert [P.plan(n, 130, 8192, 256)['nch'] for n in (300, 1100, 3100)] == [3, 5, 9]


# ---- real-kernel tier -------------------------------------------------------------------------------------------------------------
REAL = P.real_cases(CUS)


@pytest.mark.parametrize('case', REAL, ids=IDS)
def test_reference_gap_is_a_tenth_of_the_bound(case):
  """Per query and relative to the query's own terms, the gap between the oracle's Cholesky route and np.linalg.solve stays below a tenth
  of every bound the GPU test applies to the case."""
  ref = P.real_reference(case)
  assert all(np.isfinite(a).all() for a in (ref.mu, ref.var, ref.mu_scale, ref.var_scale)) and ref.mu_scale.min() > 0 and ref.var_scale.min() > 0
  g_mu, g_var = float(np.max(ref.gap_mu / ref.mu_scale)), float(np.max(ref.gap_var / ref.var_scale))
  print(f'{case.id}: route gap mu {g_mu:.1e} var {g_var:.1e}')
  for form in P.real_forms(case, CUS):
    c_mu, c_var = P.real_bounds(case, form)
    assert g_mu <= 0.1 * c_mu and g_var <= 0.1 * c_var, (case.id, form, g_mu, g_var)


@pytest.mark.parametrize('case', [c for c in REAL if c.dtype == 'fp64'], ids=IDS)
def test_queries_differ_by_orders_of_magnitude(case):
  """What a max-norm bound cannot see: the queries' own terms and results span orders of magnitude, and every kind of query stands in
  every 128-tile."""
  ref = P.real_reference(case)
  _, x, _, xq = P.real_inputs(case)
  copies = np.flatnonzero(np.arange(case.M) % 3 == 1)
  assert all((x == xq[q]).all(axis=1).any() for q in copies[:50])
  assert ref.mu_scale.max() >= 100 * ref.mu_scale.min()
  assert ref.var.max() >= 30 * ref.var.min() > 0
  if case.kname == 'dot_product':
    assert ref.var_scale.max() >= 1000 * ref.var_scale.min()
  else:   # far queries: the prior, to rounding; copies: far below it
    far = np.flatnonzero(np.arange(case.M) % 3 == 2)
    assert np.all(ref.var[far] >= 0.999 * ref.var.max()) and np.all(ref.var[copies] <= 0.5 * ref.var.max())


def test_real_forms_follow_the_plan():
  for case in REAL:
    forms = P.real_forms(case, CUS)
    if case.dtype == 'fp64' or case.n in (300, 1100):   # fp64; few queries over two or more blocks: split along K, GEMM_POST
      assert forms == ['mfma']
    else:
      assert forms == (['mfma', 'bf16x3'] if case.kname == 'dot_product' else ['mfma', 'bf16x3', 'f16x2'])
    assert set((case.dtype, f) for f in forms) <= set(P.REAL_BOUNDS)
