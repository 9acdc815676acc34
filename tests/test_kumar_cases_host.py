"""tests/kumar_cases.py judged on its own, on the CPU: the element-wise grid and its left-out entries, the NumPy restatement within
RESTATE_CAP eps_T S of the mpmath reference for every quantity (a condition on S, not a measurement of the device), the exact
identities at x in {0, 1} and a = b = 1; the analytic a / b reference against kumar_oracle.se_nll_ab_grad (SE) and central differences
of the oracle value (the other three families), its other leaves against the oracle on the warped inputs, the tiled form of the
contraction against the direct one; group F's u == 0 off the diagonal and its positive definite matrices; every mutant at least
MUTANT_FACTOR bounds away on a case of each tier it belongs to.  No GPU call."""
import copy

import mpmath
import numpy as np
import pytest

import helpers
import kumar_cases as kc
import kumar_oracle as ko
from oracle import hyperbo_oracle as o

WFO = o.DEFAULT_WARP_FUNC
DTYPES = ('fp64', 'fp32')


def test_case_list_covers_the_edges_named_in_its_docstring():
  ids = [c.id for c in kc.CASES]
  assert len(set(ids)) == len(ids)
  assert {(c.kname, c.d) for c in kc.GROUP_A} == {(k, d) for k in helpers.KERNELS for d in (1, 7, 8, 9, 16, 17)}
  assert all(c.tasks == (129, 40) and c.dtype == 'fp64' and c.ls == 'ard' for c in kc.GROUP_A)
  assert {(c.kname, c.tasks) for c in kc.GROUP_B} == {(k, (n,)) for k in helpers.KERNELS for n in (1, 2, 127, 128, 129, 257)}
  assert all(c.d == 9 for c in kc.GROUP_B + kc.GROUP_C + kc.GROUP_D)
  assert {c.kname for c in kc.GROUP_C} == set(helpers.KERNELS) and all(c.tasks == (257, 100, 1) for c in kc.GROUP_C)
  assert {(c.kname, c.ls, c.mname, c.m) for c in kc.GROUP_D} == {('matern52', 'scalar', 'constant', 1), ('matern52', 'ard', 'linear', 1),
                                                                ('matern52', 'ard', 'constant', 3), ('dot_product', 'ard', 'linear', 1),
                                                                ('dot_product', 'ard', 'constant', 3)}
  assert all(c.dtype == 'fp32' for c in kc.GROUP_E)
  assert {(c.kname, c.d, c.tasks) for c in kc.GROUP_E} == ({(k, d, (129, 40)) for k in helpers.KERNELS for d in (7, 9, 17)} |
                                                           {(k, 9, (257, 100, 1)) for k in helpers.KERNELS})
  assert {(c.kname, c.tasks, c.dtype) for c in kc.GROUP_F} == {(k, (n,), t) for k in ('matern32', 'matern52') for n in (40, 140) for t in DTYPES}
  assert all(c.d == 1 for c in kc.GROUP_F) and max(n for c in kc.CASES for n in c.tasks) == 257
  # inputs: seeded by the id, the fp32 ones the fp64 ones rounded once; zeros and ones planted; raw a, b in [-1.5, 1.5]
  a = kc.GROUP_A[3]
  x64, x32 = kc.inputs(a).tasks[0][0], kc.inputs(a._replace(group='E', dtype='fp32')).tasks[0][0]
  assert x32.dtype == np.float32 and np.any(x64 == 0) and np.any(x64 == 1)
  e = kc.GROUP_E[0]
  m64 = kc.inputs(e._replace(group='E', dtype='fp64')).model
  assert np.array_equal(kc.inputs(e).model['kumar_params']['a'], m64['kumar_params']['a'].astype(np.float32))
  assert all(np.all(np.abs(kc.inputs(c).model['kumar_params'][k]) <= 1.5) for c in kc.GROUP_A + kc.GROUP_C for k in ('a', 'b'))


# ---- element-wise ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_grid_and_the_left_out_entries(dtype):
  x = kc.grid_x(dtype)
  ra, rb, a, b = kc.grid_ab(dtype)
  dt = kc.np_dtype(dtype)
  assert x.shape == (211, 36) and x.dtype == dt and a.dtype == dt
  # squareplus(a - 1/a) is a to a few ulp, and exactly 1 for a = 1 (the identity column needs it)
  assert np.allclose(a.reshape(6, 6)[:, 0], kc.GRID_AB, rtol=4 * np.finfo(dt).eps, atol=0) and np.allclose(b[:6], kc.GRID_AB, rtol=4 * np.finfo(dt).eps, atol=0)
  assert int(np.sum(a == 1)) == 6 and int(np.sum(b == 1)) == 6 and np.array_equal(ko.squareplus(ra).astype(dt), a)
  assert np.all(x[0] == 0) and np.all(x[10] == 1) and np.all(x[9] == np.nextafter(dt(1), dt(0))) and np.all(x[1] == np.finfo(dt).tiny)
  er = kc.elem_reference(dtype)
  out = ~er.dx_finite
  # exactly: x = 0 where a < 1, x = 1 where b < 1; at most 2 of the 211 rows of a column, and nothing else
  expect = np.zeros_like(out)
  expect[0, a < 1] = True
  expect[10, b < 1] = True
  assert np.array_equal(out, expect) and int(out.sum()) == kc.DX_LEFT_OUT == 24 and int(out.sum(axis=0).max()) == 2
  assert all(mpmath.isfinite(v) for q in ('w', 'da', 'db') for v in er.ref[q].ravel())


@pytest.mark.parametrize('dtype', DTYPES)
def test_reference_identities_at_the_ends_and_at_a_b_1(dtype):
  er, x = kc.elem_reference(dtype), kc.grid_x(dtype)
  _, _, a, b = kc.grid_ab(dtype)
  for row, wv in ((0, 0), (10, 1)):
    assert all(v == wv for v in er.ref['w'][row]) and all(v == 0 for q in ('da', 'db') for v in er.ref[q][row])
    assert all(s == 0 for q in ('da', 'db') for s in er.scale[q][row])
  col = int(np.flatnonzero((a == 1) & (b == 1))[0])
  assert all(er.ref['w'][i, col] == mpmath.mpf(float(x[i, col])) for i in range(x.shape[0]))
  rest = kc.elem_restatement(dtype)
  assert np.array_equal(rest['w'][:, col], x[:, col]) and rest['w'].dtype == x.dtype
  for row, wv in ((0, 0.0), (10, 1.0)):
    assert np.all(rest['w'][row] == wv) and np.all(rest['da'][row] == 0) and np.all(rest['db'][row] == 0)


@pytest.mark.parametrize('dtype', DTYPES)
def test_restatement_stays_within_the_cap_of_eps_s(dtype):
  """If it does not, S is wrong: fix S, not the cap."""
  ratios = kc.elem_restatement_ratios(dtype)
  print(f'KUMAR restatement {dtype}: ' + ' '.join(f'{q} {r:.3g}' for q, (r, _) in ratios.items()))
  assert all(r <= kc.RESTATE_CAP for r, _ in ratios.values()), ratios
  assert all(r >= 0.05 for r, _ in ratios.values()), ('a scale this loose bounds nothing', ratios)
  # the restatement is inside its own bound by construction; the element-wise mutants are not
  assert all(r <= 0.25 for r, _ in kc.elem_ratios(dtype, kc.elem_restatement(dtype)).values())
  for mutant, q in (('vb_for_vb1', 'da'), ('h_fp32', 'da'), ('h_fp32', 'db')):
    r = kc.elem_ratios(dtype, kc.elem_mutant(dtype, mutant))[q][0]
    print(f'KUMAR element-wise mutant {mutant} {dtype} {q}: {r:.3g} bounds')
    assert r >= kc.MUTANT_FACTOR


def test_kumar_oracle_derivatives_agree_with_mpmath_on_the_interior():
  """kumar_oracle.dw_dab / dw_dx, which the gradient references contract with: within 1e-12 of the largest entry of each column's
  interior rows (x in [1e-3, 0.9] and the uniform draws; at 1 - 1e-6 NumPy's 1 - x^a has lost six digits: 2e-12)."""
  er, x = kc.elem_reference('fp64'), kc.grid_x('fp64').astype(np.float64)
  _, _, a, b = kc.grid_ab('fp64')
  da, db = ko.dw_dab(x, a, b)
  dx = ko.dw_dx(x, a, b)
  rows = np.r_[4:8, 11:211]
  for q, got in (('da', da), ('db', db), ('dx', dx)):
    ref = np.array([[float(v) for v in row] for row in er.ref[q][rows]])
    assert np.max(np.abs(got[rows] - ref) / np.max(np.abs(ref), axis=0)) <= 1e-12, q


# ---- the analytic reference --------------------------------------------------------------------------------------------------------
def _oracle_dataset(case):
  return {k: o.SubDataset(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)) for k, (x, y) in enumerate(kc.inputs(case).tasks)}


def _warped_dataset(case):
  kp = kc.inputs(case).model['kumar_params']
  return {k: o.SubDataset(ko.warp(s.x, kp['a'], kp['b']), s.y) for k, s in _oracle_dataset(case).items()}


def _leaf_close(got, ref, tol):
  got, ref = np.asarray(got, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel()
  return np.max(np.abs(got - ref)) <= tol * max(np.max(np.abs(ref)), 1e-300)


@pytest.mark.parametrize('case', [c for c in kc.GROUP_A + kc.GROUP_C if c.kname == 'squared_exponential'], ids=lambda c: c.id)
def test_analytic_ab_reproduces_se_nll_ab_grad(case):
  ga, gb = ko.se_nll_ab_grad(kc.cast(kc.inputs(case).model, np.float64), _oracle_dataset(case))
  ref = kc.reference(case).grad['kumar_params']
  assert _leaf_close(ref['a'], ga, kc.SE_AB_TOL) and _leaf_close(ref['b'], gb, kc.SE_AB_TOL)


@pytest.mark.parametrize('case', [c for c in kc.GROUP_A + kc.GROUP_C + kc.GROUP_D if c.mname == 'constant' and c.m == 1], ids=lambda c: c.id)
def test_other_leaves_and_value_reproduce_the_oracle_on_warped_inputs(case):
  model = {k: v for k, v in kc.cast(kc.inputs(case).model, np.float64).items() if k != 'kumar_params'}
  vo, go = o.nll_value_and_grad(o.constant, getattr(o, case.kname), o.GPParams(model=model), _warped_dataset(case), WFO)
  ref = kc.reference(case)
  assert abs(ref.value - vo) <= 1e-13 * abs(vo)
  rest = {k: v for k, v in ref.grad.items() if k != 'kumar_params'}
  helpers.assert_grad_close(rest, go, 1e-12)
  # per task: the values are the oracle's, task by task
  _, k2 = o.neg_log_marginal_likelihood(o.constant, getattr(o, case.kname), o.GPParams(model=model), _warped_dataset(case), WFO, return_key2nll=True)
  assert all(abs(ref.tasks[k].value - k2[k]) <= 1e-13 * abs(k2[k]) for k in k2)


FD_CASES = ([c for c in kc.GROUP_A if c.d == 9 and c.kname != 'squared_exponential'] + [c for c in kc.GROUP_D] +
            [c for c in kc.GROUP_F if c.dtype == 'fp64' and c.tasks == (40,)])


@pytest.mark.parametrize('case', FD_CASES, ids=lambda c: c.id)
def test_analytic_leaves_agree_with_central_differences(case):
  """Every leaf of the analytic reference (a, b and the rest, the linear mean on raw x included) against central differences of the
  oracle's NLL with the kernel composed with the warp, at the 1e-6 of tests/test_gpu_kumar.py."""
  model = kc.cast(kc.inputs(case).model, np.float64)
  ds = _oracle_dataset(case)
  kern = ko.kumar_kernel(getattr(o, case.kname))
  f = lambda mdl: o.neg_log_marginal_likelihood(getattr(o, case.mname), kern, o.GPParams(model=mdl), ds, WFO)
  ref = kc.reference(case)
  assert abs(f(model) - ref.value) <= 1e-12 * abs(ref.value)
  used = {'squared_exponential': ('lengthscale', 'signal_variance'), 'matern32': ('lengthscale', 'signal_variance'),
          'matern52': ('lengthscale', 'signal_variance'), 'dot_product': ('dot_prod_sigma', 'dot_prod_bias')}[case.kname]
  flat, h = helpers.flatten(model), 1e-5
  fd = np.zeros_like(flat)
  for i in range(flat.size):
    hi, lo = flat.copy(), flat.copy()
    hi[i] += h; lo[i] -= h
    fd[i] = (f(helpers.unflatten_like(model, hi)) - f(helpers.unflatten_like(model, lo))) / (2 * h)
  fd = helpers.unflatten_like(model, fd)
  got = copy.deepcopy(ref.grad)
  for path, r in helpers.tree_leaves(fd):
    g = dict(helpers.tree_leaves(got))[path]
    if path.split('/')[0] not in used + ('noise_variance', 'constant', 'linear_mean', 'kumar_params') or (path == 'constant' and case.mname != 'constant'):
      assert np.all(g == 0) and np.max(np.abs(r)) <= 1e-9, path     # a leaf the model does not read
      continue
    assert np.allclose(g, r, rtol=kc.AB_FD_TOL, atol=kc.AB_FD_TOL * max(np.max(np.abs(r)), 1e-3)), (path, g, r)


@pytest.mark.parametrize('case', [c for c in kc.GROUP_C] + [c for c in kc.GROUP_D if c.ls == 'scalar'] + [c for c in kc.GROUP_A if c.d == 17], ids=lambda c: c.id)
def test_tiled_form_of_the_contraction_equals_the_direct_one(case):
  """What the mutants are changed lines of: kumar_contract_kernel's per-tile sums reproduce sum_i d f / d w_i dw_i / da."""
  ref = kc.reference(case)
  tiled = kc._reference_of(case, mutant='tiled')           # any name that is no mutant: the tiled form as it stands
  for k in ('a', 'b'):
    scale = ref.leaf_scales[f'kumar_params/{k}']
    assert np.max(np.abs(tiled.grad['kumar_params'][k] - ref.grad['kumar_params'][k])) <= 1e-13 * scale, k


# ---- group F -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', kc.GROUP_F, ids=lambda c: c.id)
def test_warped_duplicates_put_u_zero_off_the_diagonal_of_a_positive_definite_matrix(case):
  x = kc.inputs(case).tasks[0][0]
  a, b = kc.warped_ab(case)
  assert a[0] == 8.0 and b[0] == 2.0 and x.dtype == case.np_dtype
  n = case.tasks[0]
  tiny = np.isin(x[:, 0], np.array(kc.F_TINY[case.dtype], dtype=case.np_dtype))
  assert int(tiny.sum()) == n // 3 and int(np.sum(x == 1)) == 2 and int(np.sum(x == np.nextafter(case.np_dtype(1), case.np_dtype(0)))) == 2
  assert len(np.unique(x[tiny])) == 3                      # distinct inputs ...
  w = ko.warp(x.astype(np.float64), kc.inputs(case).model['kumar_params']['a'].astype(np.float64), kc.inputs(case).model['kumar_params']['b'].astype(np.float64))
  assert np.all(w[tiny] == 0)                              # ... one warped value
  # in the model dtype x^a underflows as well: the device's own w is 0 there
  with np.errstate(under='ignore'):
    assert np.all(x[tiny] ** case.np_dtype(8) == 0)
  ref = kc.reference(case).tasks[0]
  assert ref.u_zero_offdiag >= (n // 3) * (n // 3 - 1)
  noise = float(o.default_softplus(np.float64(kc.inputs(case).model['noise_variance'])))
  assert ref.min_eig >= 0.9 * noise and np.isfinite(ref.value)
  assert all(np.isfinite(v).all() for _, v in helpers.tree_leaves(ref.grad))


# ---- mutants -------------------------------------------------------------------------------------------------------------------------
MUTANT_CASES = ([c for c in kc.GROUP_A if c.d in (1, 9, 17)] + [c for c in kc.GROUP_B if c.tasks[0] in (129, 257)] + kc.GROUP_C +
                [c for c in kc.GROUP_E if c.d in (9, 17)] + kc.GROUP_F)


@pytest.mark.parametrize('mutant', sorted(kc.MUTANTS))
def test_every_mutant_lies_ten_bounds_away_on_a_case_of_each_tier(mutant):
  hit = {c.id: kc.mutant_ratio(c, mutant) for c in MUTANT_CASES if kc.applicable(c, mutant) and c.dtype in kc.MUTANT_TIERS[mutant]}
  assert hit, 'no case the mutant applies to'
  for tier in kc.MUTANT_TIERS[mutant]:
    rs = {i: r for i, r in hit.items() if i.endswith(tier)}
    print(f'KUMAR mutant {mutant} {tier}: at least {kc.MUTANT_FACTOR:g} bounds away on {sum(r >= kc.MUTANT_FACTOR for r in rs.values())} of {len(rs)} cases, '
          f'largest {max(rs.values()):.3g}, least {min(rs.values()):.3g}')
    assert any(r >= kc.MUTANT_FACTOR for r in rs.values()), (tier, rs)
  if mutant == 'dkdu_unguarded':
    # only cases with u == 0 off the diagonal see it: group F (and d = 1 of group A, whose planted zeros repeat)
    assert all(r == np.inf for i, r in hit.items() if i.startswith('F-')), hit
    assert all(r <= 1e-3 for i, r in hit.items() if i.startswith('C-')), hit
  if mutant == 'drop_slot2':
    assert all(r >= kc.MUTANT_FACTOR for i, r in hit.items() if i.endswith('fp64')), hit
  if mutant == 'no_col_term':
    # the mixed batch and the one-task cases both show it, in every family
    fp64 = {i: r for i, r in hit.items() if i.endswith('fp64')}
    assert all(r >= kc.MUTANT_FACTOR for r in fp64.values()), fp64
  if mutant == 'drop_last_chunk':
    assert all(r >= kc.MUTANT_FACTOR for i, r in hit.items() if i.endswith('fp64') and '-d9-' in i), hit


def test_mutants_that_do_not_apply_change_nothing():
  c = kc.GROUP_B[2]          # n = 127: one tile
  assert not kc.applicable(c, 'no_col_term') and kc.mutant_ratio(c, 'no_col_term') <= 1e-3
  c = kc.GROUP_A[1]          # d = 7: one chunk
  assert not kc.applicable(c, 'drop_last_chunk') and kc.mutant_ratio(c, 'drop_last_chunk') <= 1e-3
