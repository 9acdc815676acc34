"""CPU tier of the hbo_acq_grad shape tests: tests/acq_grad_cases.py judged on its own, so that tests/test_gpu_acq_grad_shapes.py
cannot pass vacuously (as test_full_cov_host.py does for its tier).  On a sub-sample of the case list at the shapes of the list (the
GPU test asserts conditions 1 - 3 again for every case it runs):

  * the conditions under which a per-query bound means something: no fp64 query is left out; fp32 EI / PI leave out only queries
    beyond |gamma| = 3, at most one in nine, UCB none; every query's largest gradient component is at least 1e-8 of the case's
    largest; the Gram matrix of a stationary case is neither the identity nor all ones;
  * the NumPy restatement of the device's route (l = W k, beta = W^T l) that the mutants are made from IS the oracle: 1e-10;
  * every mutant -- one per failure the kernels could have -- is at least MUTANT_FACTOR = 100 fp64 bounds away from the reference on
    at least one query of every fp64 case it applies to.  In fp32, 100 bounds are 2 * (1 + gamma^2) times the query's largest gradient
    component, which no defect that leaves the gradient within twice its own size can reach: there every applicable mutant must be
    beyond the fp32 bound itself (FP32_MUTANT_FACTOR = 1) on the fp32 twin of every such case, except where
    acq_grad_cases.FP32_BLIND lists it by name -- (c) at ten cases (n = 257 and 513; n = 300 at d = 1 and 2), every one of them in
    the sub-sample and asserted to be inside the bound, so that the list stays true;
  * not_applicable() agrees with what each mutant's handle addresses (mask, row range, column), computed here on its own; condition 4
    holds for EVERY stationary case of the list, not only the sub-sample;
  * the oracle's gradient, never before compared with anything above d = 3, against central differences of the oracle's own value
    at widths 17, 40 (Kumaraswamy) and 256 and through four MLP layers: h = 1e-6, rtol 1e-5 (tests/test_gpu_kumar.py)."""
import numpy as np
import pytest

import acq_grad_cases as G
import kumar_oracle

IDS = lambda c: c.id


def _host_cases():
  """Every eighth fp64 / fp32 pair of each group (offset by the group, so that the widths differ), plus what the mutants and the
  finite differences need: the widest plain, MLP and Kumaraswamy cases, both passes, M = 1 with and without a half chunk."""
  fp64 = [c for c in G.CASES if c.dtype == 'fp64']
  picked = []
  for gi, grp in enumerate('ABCDEF'):
    members = [c for c in fp64 if c.group == grp]
    picked += members[gi % 8::8]
  def want(pred):
    picked.extend(c for c in fp64 if pred(c) and c not in picked)
  want(lambda c: c.group == 'A' and c.d in (129, 256) and c.kname in ('matern52', 'dot_product') and c.ls != 'scalar')
  want(lambda c: c.group == 'B' and c.feats in ((12, 256), (7, 40, 9, 33)) and c.mlp_k and c.mname == 'linear_mlp')
  want(lambda c: c.group == 'C' and c.M in (1, 1025) or (c.group == 'C' and c.M == 2049 and c.kumar))
  want(lambda c: c.group == 'D' and c.n in (1, 64, 129, 257, 513))
  want(lambda c: c.group == 'E' and c.d == 256 and c.kname == 'dot_product')
  want(lambda c: c.group == 'F' and c.d in (40, 256) and c.kname == 'squared_exponential')
  want(lambda c: bool(G.fp32_blind(c._replace(dtype='fp32'))))
  return picked


HOST64 = _host_cases()
HOST = [c for c64 in HOST64 for c in (c64, c64._replace(dtype='fp32'))]


def test_case_list_covers_what_the_gpu_tier_needs():
  ids = [c.id for c in G.CASES]
  assert len(set(ids)) == len(ids)
  assert all(c._replace(dtype='fp64') in G.CASES and c._replace(dtype='fp32') in G.CASES for c in G.CASES)   # every case has its twin
  assert set(HOST) <= set(G.CASES)
  a = [c for c in G.CASES if c.group == 'A']
  assert len(a) == 12 * 7 * 2 and {c.d for c in a} == {1, 2, 5, 16, 17, 32, 33, 64, 65, 128, 129, 256}
  assert {G.groups_of_reduction(c) for c in a} == {256, 128, 32, 16, 8, 4, 2, 1}     # with C / D's 64: every layout of the reduction
  assert all(c.n == 300 and c.M == 9 and c.mname == 'linear' for c in a)
  b = [c for c in G.CASES if c.group == 'B']
  assert {c.feats for c in b} == set(G.B_STACKS) and len(b) == (6 + 1) * 3 * 2 and all(c.d == 5 and c.n == 150 for c in b)
  assert {(c.mlp_k, c.mname) for c in b} == {(True, 'linear_mlp'), (True, 'linear'), (False, 'linear_mlp')}
  c_ = [c for c in G.CASES if c.group == 'C']
  assert {c.M for c in c_} == {1, 2, 8, 9, 1023, 1024, 1025, 2049} and len(c_) == 8 * 3 * 2
  assert {c.kernel_name for c in c_} == {'squared_exponential', 'matern52_mlp', 'squared_exponential_kumar'}
  d = [c for c in G.CASES if c.group == 'D']
  assert {c.n for c in d} == set(G.D_SIZES) and {c.M for c in d} == {1, 9} and len(d) == 15 * 2 * 2 * 2
  e = [c for c in G.CASES if c.group == 'E']
  assert all(c.n == 0 for c in e) and {c.d for c in e} == {17, 256, 5} and {c.M for c in e} == {1, 9}
  f = [c for c in G.CASES if c.group == 'F']
  assert {c.d for c in f} == {1, 17, 40, 256} and all(c.kumar for c in f) and len(f) == 4 * 3 * 2
  r = G.reuse_cases()
  assert (r[0].n, r[0].M, r[0].d) == (513, 1025, 64) and (r[1].n, r[1].M, r[1].d) == (2, 1, 1) and (r[2].n, r[2].d) == (0, 256)
  # every mutant is live somewhere in the sub-sample judged here
  live = set()
  for c in HOST64:
    live |= set(G.MUTANTS) - G.not_applicable(c)
  assert live == set(G.MUTANTS)


# (the largest re-use case, 1025 queries x 513 rows x 64 features, is left to the GPU test, which asserts the conditions of every case)
@pytest.mark.parametrize('case', HOST + G.reuse_cases()[1:], ids=IDS)
def test_conditions_hold(case):
  ref = G.reference(case)
  assert G.conditions(case, ref) == [], f'{case.id}: give the case another seed (acq_grad_cases.RESEED)'
  assert case.np_dtype(ref.target) == ref.target     # the target is a number of the model dtype
  for acq in G.ACQS:
    assert G.checked(case, acq, ref).any()
  if case.kname != 'dot_product' and case.n >= 2:
    assert G.gram_fraction(case) >= 0.5, case.id


@pytest.mark.parametrize('case', HOST64, ids=IDS)
def test_route_restates_the_oracle(case):
  ref = G.reference(case)
  for acq in G.ACQS:
    val, grad = G.route(case, acq, G.acq_param(acq, ref))
    assert np.max(np.abs(val - ref.val[acq])) <= 1e-10 * max(np.max(np.abs(ref.val[acq])), 1e-300), (case.id, acq)
    assert np.max(np.abs(grad - ref.grad[acq])) <= 1e-10 * np.max(np.abs(ref.grad[acq])), (case.id, acq)
    rv, rg = G.ratios(case, acq, ref, val, grad)      # and far inside the bounds the device is held to
    assert rv.max() <= 1e-2 and np.nanmax(rg) <= 1e-2, (case.id, acq, rv.max(), np.nanmax(rg))


@pytest.mark.parametrize('case', HOST, ids=IDS)
def test_every_mutant_is_outside_the_gpu_bound(case):
  """fp64: by MUTANT_FACTOR bounds.  fp32: by FP32_MUTANT_FACTOR, except the mutants fp32_blind() names, which are inside."""
  ref = G.reference(case)
  na, blind = G.not_applicable(case), G.fp32_blind(case)
  factor = G.MUTANT_FACTOR if case.dtype == 'fp64' else G.FP32_MUTANT_FACTOR
  assert not (blind & na) and (case.dtype == 'fp32' or not blind)
  for name, mutant in G.MUTANTS.items():
    if name in na:
      continue
    far = 0.0
    for acq in G.ACQS:
      val, grad = mutant(case, acq, G.acq_param(acq, ref))
      assert val.shape == (case.M,) and grad.shape == (case.M, case.d)
      rv, rg = G.ratios(case, acq, ref, val, grad)
      far = max(far, float(rv.max()), float(np.nanmax(rg)))
    if name in blind:
      assert far < factor, f'{case.id}: mutant ({name}) is seen ({far:.3g} bounds): take it off FP32_BLIND'
    else:
      assert far >= factor, f'{case.id}: mutant ({name}) is only {far:.3g} bounds away (needs {factor:g})'


def test_fp32_blind_list_is_judged_entry_by_entry():
  blind = [c for c in G.CASES if G.fp32_blind(c)]
  assert len(blind) == len(G.FP32_BLIND) == 10 and all(c.dtype == 'fp32' and c in HOST for c in blind)
  assert all(G.fp32_blind(c) == {'c'} and 'c' not in G.not_applicable(c) for c in blind)
  assert {c.n for c in blind} == {257, 300, 513} and {c.d for c in blind if c.n == 300} == {1, 2}


def test_not_applicable_agrees_with_what_the_mutants_address():
  """For every case of the list: what each mutant's handle touches, worked out here from the kernels' loops, is empty exactly where
  not_applicable() says so."""
  for c in G.CASES:
    na = G.not_applicable(c)
    kernel_term = c.n > 0 or c.kname == 'dot_product'              # the feature gradient has something in it
    assert ('a' in na) == (not (np.any(np.arange(c.fdim) >= 64) and kernel_term))
    fd = 1 << int(np.ceil(np.log2(c.fdim)))                          # acq_grad_kernel: FD, G, `for (ii = grp; ii < lim; ii += G)`
    last_group = [i0 + ii for i0 in range(0, c.n, 256) for ii in range(256 // fd - 1, min(256, c.n - i0), 256 // fd)]
    assert ('b' in na) == (not last_group)
    # tri_matmat_trans_kernel (M >= 2): 256-row chunks from 0 to npad; the rows of a chunk that ends beyond npad
    half = [r for rc in range(0, c.npad, 256) if rc + 256 > c.npad for r in range(rc, min(c.n, c.npad))]
    assert ('c' in na) == (not (half and c.M >= 2))
    assert ('d' in na) == (not (c.n > 0 and np.arange(c.M)[8:9].size))     # right-hand side 8 of the first group of 8
    assert ('e' in na) == (not np.arange(c.M)[1024:].size)                 # a second pass
    assert ('f' in na) == (not (c.n > 0 and c.M == 1))                     # launch_tri_matvec: m == 1 takes tri_matvec_kernel
    assert ('g' in na) == (not (c.kumar and np.arange(c.d)[1:].size))      # a column other than 0
    assert ('h' in na) == (not len(c.feats[:-1]))                          # a hidden layer


def test_gram_condition_holds_for_every_stationary_case():
  """Condition 4 over the whole list (fp64; the fp32 twin is the same matrix rounded): the Gram matrix is neither the identity nor
  all ones.  One Gram matrix per (shape, kernel): the observations do not depend on M."""
  seen = set()
  for c in G.CASES + G.reuse_cases():
    key = c._replace(M=1, dtype='fp64')
    if c.kname == 'dot_product' or c.n < 2 or c.dtype != 'fp64' or key in seen:
      continue
    assert G.gram_fraction(c) >= 0.5, c.id
    seen.add(key)
  assert len(seen) > 100


def _raw_value(case, acq, param, xq_raw):
  """The oracle's own value at raw queries (Kumaraswamy: the oracle sees w(x))."""
  if case.kumar:
    kp = G.inputs(case)[0]['kumar_params']
    xq_raw = kumar_oracle.warp(xq_raw, kp['a'], kp['b'])
  return G.oracle_value_and_grad(case, acq, param, xq=xq_raw)[0]


def _fd_case(group, **kw):
  found = [c for c in G.CASES if c.group == group and c.dtype == 'fp64' and all(getattr(c, k) == v for k, v in kw.items())]
  assert len(found) == 1, (group, kw, [c.id for c in found])
  return found[0]


FD_CASES = [_fd_case('A', d=17, kname='matern52', ls='ard'), _fd_case('A', d=256, kname='squared_exponential', ls='ard'),
            _fd_case('A', d=256, kname='dot_product'), _fd_case('B', feats=(7, 40, 9, 33), mlp_k=True, mname='linear_mlp'),
            _fd_case('F', d=40, kname='squared_exponential')]


@pytest.mark.parametrize('case', FD_CASES, ids=IDS)
def test_oracle_gradient_vs_central_differences(case):
  ref = G.reference(case)
  xq = G.inputs(case)[3].astype(np.float64)
  h = 1e-6
  rng = np.random.default_rng(case.d)
  # every coordinate; d = 256: 16 randomly chosen coordinates per query
  coords = np.stack([rng.choice(case.d, size=16, replace=False) if case.d > 64 else np.arange(case.d) for _ in range(case.M)])
  rows = np.arange(case.M)
  # every perturbed copy of the queries in one call (queries are independent): [coordinate k][+h, -h][query]
  stack = np.tile(xq, (coords.shape[1], 2, 1, 1))
  for k in range(coords.shape[1]):
    stack[k, 0, rows, coords[:, k]] += h
    stack[k, 1, rows, coords[:, k]] -= h
  for acq in G.ACQS:
    param = G.acq_param(acq, ref)
    v = _raw_value(case, acq, param, stack.reshape(-1, case.d)).reshape(coords.shape[1], 2, case.M)
    assert np.array_equal(_raw_value(case, acq, param, xq), ref.val[acq])      # the same function the reference is the gradient of
    for k in range(coords.shape[1]):
      fd = (v[k, 0] - v[k, 1]) / (2 * h)
      got = ref.grad[acq][rows, coords[:, k]]
      np.testing.assert_allclose(got, fd, rtol=1e-5, atol=1e-7 * max(1.0, np.max(np.abs(fd))), err_msg=f'{case.id} {acq} coordinate {k}')
