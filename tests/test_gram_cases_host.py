"""tests/gram_cases.py judged on its own, on the CPU: the table reaches every edge of gram_kernel / gram_mfma_kernel / kdiag_kernel it
claims to, the longdouble reference agrees with mpmath, the restatement of the kernel's arithmetic stays at or below half the per-entry
bound in both dtypes, every mutant is rejected in every group it is listed for, and every group rejects at least one.  No device."""
import mpmath as mp
import numpy as np
import pytest

import gram_cases as gc

LD = gc.LD


def _by_group(g):
  return [c for c in gc.CASES if c.group == g]


# ---- the table ------------------------------------------------------------------------------------------------------------------------
def test_table_reaches_the_feature_chunk_edges():
  w = {c.fdim for c in _by_group('A')}
  assert {1, gc.DC - 1, gc.DC, gc.DC + 1, 2 * gc.DC - 1, 2 * gc.DC, 2 * gc.DC + 1} <= w
  assert any(f > 4 * gc.DC and f % gc.DC for f in w)                      # four full chunks and a partial one
  assert any(f % gc.DC == 0 and f > 2 * gc.DC for f in w)                 # three full chunks, nothing partial
  for f in w:                                                            # every width: four kernels in fp64 and on the VALU kernel in fp32
    for dt in gc.DTYPES:
      assert {c.kname for c in _by_group('A') if c.fdim == f and c.dtype == dt and c.engine == 'valu'} == set(gc.KERNELS), (f, dt)
  mf = {c.fdim for c in _by_group('A') if c.engine == 'mfma'}
  assert mf == {f for f in w if f >= gc.MFMA_MIN_F}
  assert any(f & 3 for f in mf) and any(f & 3 == 0 for f in mf)          # the scalar and the float4 staging of gram_mfma_kernel
  assert all(c.ctx == 'direct' for c in _by_group('A') if c.dtype == 'fp32' and c.engine == 'valu')
  assert all(c.ctx == 'default' for c in gc.CASES if c.group != 'A')
  assert all((c.n1, c.n2) == (70, 130) for c in _by_group('A'))


def test_table_reaches_the_tile_edges():
  cross = {(c.n1, c.n2) for c in _by_group('B') if c.n2}
  sym = {c.n1 for c in _by_group('B') if not c.n2}
  assert {c.fdim for c in _by_group('B')} == {3, gc.DC + 1}
  assert {n1 for n1, _ in cross} >= {1, gc.GTR - 1, gc.GTR, gc.GTR + 1, gc.TILE, gc.TILE + 1}
  assert {n2 for _, n2 in cross} >= {1, gc.TILE - 1, gc.TILE, gc.TILE + 1, 2 * gc.TILE}
  assert any(n1 > 3 * gc.GTR and n2 > 2 * gc.TILE for n1, n2 in cross)   # more than one block both ways, neither a multiple
  assert sym >= {1, gc.GTR - 1, gc.GTR, gc.GTR + 1, gc.TILE - 1, gc.TILE, gc.TILE + 1, 3 * gc.GTR + 1} and max(sym) > 2 * gc.TILE
  for c in _by_group('B'):
    assert c.engine == 'valu'
  # the padded cross form: a single column, one column past a tile, and interior tiles
  d = {(c.n1, c.n2) for c in _by_group('D')}
  assert d == {(130, 1), (130, 129), (200, 300)}
  assert len(gc.interior_tiles(next(c for c in _by_group('D') if (c.n1, c.n2) == (200, 300)))) >= 4
  assert not gc.interior_tiles(next(c for c in _by_group('D') if (c.n1, c.n2) == (130, 1)))
  for shape in d:
    for dt in gc.DTYPES:
      for f in (3, gc.DC + 1):
        assert {c.direct_form for c in _by_group('D') if (c.n1, c.n2) == shape and c.dtype == dt and c.fdim == f} == {0, 1}
  assert {c.engine for c in _by_group('D') if c.fdim == 33} == {'valu', 'mfma'} and all(c.dtype == 'fp32' for c in _by_group('D') if c.fdim == 33)
  # the task form
  batch = [c for c in _by_group('E') if len(c.tasks) > 1]
  assert all(c.tasks == (1, 64, 65, 128, 129, 257, 300) for c in batch)
  assert {(c.fdim, c.dtype) for c in batch} == {(3, 'fp64'), (17, 'fp64'), (3, 'fp32'), (17, 'fp32'), (33, 'fp32'), (40, 'fp32')}
  assert {c.per_task for c in batch} == {False, True}
  assert all(c.engine == 'mfma' for c in batch if c.fdim >= gc.MFMA_MIN_F and c.kname != 'dot_product')
  single = [c for c in _by_group('E') if len(c.tasks) == 1]
  assert single and all(gc.round_up(c.tasks[0], gc.TILE) // gc.TILE == 5 for c in single)    # gridDim.x = 5: the rotation
  assert {c.n1 for c in _by_group('F')} == {1, 255, 256, 257} and {c.kname for c in _by_group('F')} == {'dot_product', 'matern32'}
  assert all(c.fdim == gc.DC + 1 for c in _by_group('F') if c.kname == 'dot_product')


def test_lengthscales_are_distinct_and_spread():
  for c in gc.CASES:
    if c.fdim == 1:
      continue
    for p in gc.inputs(c)[1]:
      ls = p['ls'].astype(np.float64)
      assert len(set(ls.tolist())) == c.fdim and ls.max() / ls.min() >= 4.0, c.id
      if c.fdim > gc.DC:
        assert np.all(ls[gc.DC:] != ls[:c.fdim - gc.DC])                 # feature d never shares a length-scale with d - 16
  for c in _by_group('E'):
    if c.per_task:
      ms = gc.inputs(c)[1]
      assert len({(m['sv'], m['noise'], float(m['ls'][0])) for m in ms}) == len(c.tasks)


def test_group_c_holds_duplicates_tails_and_offsets():
  assert {c.offset for c in _by_group('C')} == {0.0, 10.0, 1000.0} and {c.fdim for c in _by_group('C')} == {2, gc.DC + 1}
  for c in _by_group('C'):
    xs, models = gc.inputs(c)
    u = gc.pair_terms(xs[0], xs[1], gc.inv_ls64(models[0]))[0].astype(np.float64)
    graded = u[np.arange(c.n2) % gc.C_BASE, np.arange(c.n2)]
    assert np.sum(graded == 0) >= gc.C_BASE                               # exact duplicates
    if c.offset == 0:
      assert np.any((graded > 0) & (graded < 1e-15)) and np.any(np.abs(graded - 1) < 1e-3)
      assert graded.max() >= (1399.0 if c.dtype == 'fp64' else 169.0)     # SE: exp(-700) / exp(-85)


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def _mp_cov(kname, u, sv):
  if kname == 'squared_exponential':
    return sv * mp.exp(-u / 2)
  r = mp.sqrt((3 if kname == 'matern32' else 5) * u)
  return sv * (1 + r) * mp.exp(-r) if kname == 'matern32' else sv * (1 + r + r * r / 3) * mp.exp(-r)


def _mp(v):
  return mp.mpf(float(v))   # (every input is an fp32 or fp64 number: exact)


@pytest.mark.parametrize('dtype', gc.DTYPES)
@pytest.mark.parametrize('kname', gc.KERNELS)
def test_reference_against_mpmath(kname, dtype):
  assert np.finfo(LD).eps < 2e-19, 'np.longdouble is not the 80-bit format here'
  mp.mp.dps = 60
  group = 'C' if kname != 'dot_product' else 'A'
  case = next(c for c in gc.CASES if c.group == group and c.kname == kname and c.dtype == dtype and c.fdim == gc.DC + 1 and c.offset == 0)
  xs, models = gc.inputs(case)
  p, T = models[0], case.np_dtype
  ref, bound = gc.expected(case)
  if group == 'C':
    u = gc.pair_terms(xs[0], xs[1], gc.inv_ls64(p))[0].astype(np.float64)
    cols = np.arange(case.n2)
    graded = u[cols % gc.C_BASE, cols]
    picks = [int(np.argmin(np.abs(graded))), int(np.argmin(np.abs(np.log10(np.maximum(graded, 1e-300)) + 16))), int(np.argmin(np.abs(graded - 1))),
             int(np.argmax(graded))]
    entries = [(j % gc.C_BASE, j) for j in picks]
    assert graded[picks[0]] == 0 and graded[picks[1]] < 1e-15 and graded[picks[3]] > 1000
  else:
    entries = [(0, 0), (69, 129), (33, 64)]
  inv = gc.inv_ls64(p)
  for i, j in entries:
    a, b = xs[0][i], xs[1][j]
    if kname == 'dot_product':
      is2, b2 = gc.dot_coefs(p, T)
      want = sum(_mp(a[d]) * _mp(b[d]) for d in range(case.fdim)) * _mp(is2) + _mp(b2)
      scale = sum(abs(_mp(a[d]) * _mp(b[d])) for d in range(case.fdim)) * _mp(is2) + abs(want)
    else:
      uu = sum(((_mp(a[d]) - _mp(b[d])) * _mp(inv[d])) ** 2 for d in range(case.fdim))
      want = _mp_cov(kname, uu, _mp(T(p['sv'])))
      scale = want * (1 + mp.sqrt(5 * uu) + uu)
    got = mp.mpf(ref[i, j].astype(np.float64)) + mp.mpf(float(ref[i, j] - LD(ref[i, j].astype(np.float64))))   # the longdouble, exactly
    # the reference's own error: a few dozen longdouble roundings (2^-64 each), amplified by the exponential's argument
    assert abs(got - want) <= 64 * float(np.finfo(LD).eps) * scale, (kname, dtype, i, j, got, want)
    # ... which is nothing beside the bound it is used with
    assert abs(got - want) <= 1e-2 * bound[i, j], (kname, dtype, i, j, float(abs(got - want)), bound[i, j])


# ---- the bound: the restatement's own error is at most half of it --------------------------------------------------------------------
@pytest.mark.parametrize('group', 'ABCDEF')
def test_restatement_within_half_the_bound(group):
  worst = {}
  for case in _by_group(group):
    got = gc.fake(case)
    ratio = gc.judge(case, got)     # every structural assertion holds for the restatement's own buffers, too
    key = (case.dtype, case.kname)
    if ratio > worst.get(key, (0.0, ''))[0]:
      worst[key] = (ratio, case.id)
    assert ratio <= gc.RESTATE_SHARE, (case.id, ratio)
  print({k: '%.3f %s' % v for k, v in sorted(worst.items())})


def test_bound_is_not_slack_by_orders_of_magnitude():
  """the restatement's error reaches at least a hundredth of the bound somewhere in group A, in both dtypes and for every kernel"""
  for dt in gc.DTYPES:
    for k in gc.KERNELS:
      assert max(gc.judge(c, gc.fake(c)) for c in _by_group('A') if c.dtype == dt and c.kname == k) >= 0.01, (dt, k)


# ---- the mutants --------------------------------------------------------------------------------------------------------------------
def _mutant_case(mutant, group):
  pick = lambda **kw: next(c for c in _by_group(group) if all(getattr(c, k) == v for k, v in kw.items()))
  if mutant in ('ls_shift', 'drop_partial_chunk'):
    return pick(fdim=17, kname='matern52', dtype='fp64')
  if mutant == 'swap_row_halves':
    return pick(n1=200, n2=300, fdim=3, kname='squared_exponential', dtype='fp64', direct_form=0)
  if mutant == 'pt_col_vec2':
    return pick(fdim=17, kname='matern32', dtype='fp32', n1=(70 if group == 'A' else 65), n2=(130 if group == 'A' else 129))
  if mutant == 'one_entry_8x':
    return pick(n1=200, n2=300, fdim=17, kname='matern52', dtype='fp64')
  if mutant == 'flush_tails':
    return pick(kname='squared_exponential', dtype='fp64', fdim=2, offset=0.0)
  if mutant == 'matern_u0':
    return pick(kname='matern52', dtype='fp32', fdim=17, offset=10.0)
  if mutant in ('missing_pad_zeros', 'diag_term_in_cross'):
    return pick(n1=130, n2=129, fdim=17, kname='matern32', dtype='fp32', direct_form=0)
  if mutant == 'interior_shift':
    return pick(n1=200, n2=300, fdim=3, kname='dot_product', dtype='fp32', direct_form=1)
  if mutant == 'model0_for_all':
    return pick(tasks=gc.E_TASKS, per_task=True, fdim=17, kname='squared_exponential', dtype='fp64')
  if mutant in ('no_diag_term', 'pad_diag_zero', 'upper_tile_written'):
    return pick(tasks=gc.E_TASKS, per_task=False, fdim=3, kname='matern52', dtype='fp32')
  assert mutant == 'dot_diag_no_bias'
  return pick(kname='dot_product', dtype='fp32', n1=257)


@pytest.mark.parametrize('mutant', sorted(gc.MUTANTS))
def test_every_mutant_is_rejected_in_every_group_it_is_listed_for(mutant):
  for group in gc.MUTANTS[mutant]:
    case = _mutant_case(mutant, group)
    gc.judge(case, gc.fake(case))                       # the same buffers without the fault pass
    with pytest.raises(AssertionError):
      gc.judge(case, gc.fake(case, mutant))


def test_every_group_rejects_a_mutant():
  assert set(''.join(gc.MUTANTS.values())) == set('ABCDEF')


def test_comparison_is_per_entry():
  """the one-entry mutant is 8 bounds off in ONE entry of 60000 and would pass the suite's helpers.rel_err at the fp64 level"""
  import helpers
  case = _mutant_case('one_entry_8x', 'B')
  ref = gc.expected(case)[0].astype(np.float64)
  assert helpers.rel_err(gc.fake(case, 'one_entry_8x'), ref) < 1e-13


# ---- the hook's binding ---------------------------------------------------------------------------------------------------------------
def test_probe_gram_is_bound():
  import ctypes as C
  from hyperbo_amd import _native as nat
  res, args = nat.SIGNATURES['hbo_probe_gram']
  assert res is C.c_int and len(args) == 15
  assert args[10] is C.c_double and args[5] == C.POINTER(C.c_int64) and args[13] == C.POINTER(C.c_int64) and args[14] == C.POINTER(C.c_int64)
