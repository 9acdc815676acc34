"""tests/grad_contract_cases.py judged on its own, on the CPU: the table reaches what it claims to reach, the two references agree, the
restatement stays inside its share of the bound, and every mutant of the restatement fails the bound the device test applies
(tests/test_gpu_grad_contract.py judges with the same grad_contract_cases.judge / leaf_ratios).  No device."""
import numpy as np
import pytest

import grad_contract_cases as gc


def _ids(cases):
  return [c.id for c in cases]


def _worst(case, res):
  r = gc.leaf_ratios(case, res.grad, res.fro if case.obj == 'euc' else None)
  return max(float(np.max(r[0])), float(np.max(r[1]))) if isinstance(r, tuple) else float(np.max(r))


def test_the_table_reaches_its_edges():
  by = lambda g: [c for c in gc.CASES if c.group == g]
  assert {c.ns[0] for c in by('A')} == {1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 300}
  assert {c.fdim for c in by('B')} == {1, 15, 16, 17, 29, 30, 33, 64, 256} and {c.scalar_ls for c in by('B')} == {False, True}
  assert {c.nacc for c in by('B') if c.fdim in (29, 30)} == {32, 33}                       # the strip edge of grad_finalize_kernel
  assert {c.kname for c in by('C')} == set(gc.KERNELS)
  assert {c.ns for c in by('D')} == {(300, 1, 129, 128, 513, 64), (64, 513, 128, 129, 1, 300)}
  assert {(c.obj, c.nvec, c.ns[0]) for c in by('E') if not c.mlp} == {(o, v, n) for o in ('ekl', 'euc') for v in (1, 2, 3, 9) for n in (100, 129, 300)}
  assert any(c.mlp and c.obj == 'euc' for c in by('E'))
  assert {(c.mean, c.ns[0]) for c in by('F')} == {(m, n) for m in ('constant', 'linear', 'linear_mlp') for n in (255, 256, 257, 1023, 1025, 1300)}
  assert all(c.prereduced for c in by('G')) and {(c.ns, c.fdim) for c in by('G')} == {((3969,), 3), ((3969, 200), 30)}
  assert not any(c.prereduced for c in gc.CASES if c.group != 'G')
  g2 = next(c for c in by('G') if len(c.ns) == 2)
  assert {c.obj for c in by('G') if len(c.ns) == 2} == {'nll', 'euc'}
  assert g2.nacc > gc.QW and gc.nblk(200) * (gc.nblk(200) + 1) == 6 < gc.PRE_ROWS and gc.nblk(3969) == 32 and 3969 - 31 * 128 == 1
  assert all(c.mlp for c in by('H')) and {c.kname for c in by('H')} == set(gc.KERNELS)
  for dt in gc.DTYPES:                                                                        # fp64 and fp32 unless noted (the anchor)
    assert {c.data_key for c in gc.CASES if c.dtype == dt and c.group != 'N'} == {c.data_key for c in gc.CASES if c.group != 'N'}
  # duplicate rows across the 128-row edge in group C: u = 0 off the diagonal
  x = gc.inputs(next(c for c in by('C') if c.kname == gc.M32)).x[0]
  assert np.array_equal(x[128], x[127]) and np.array_equal(x[150], x[5])
  # every operand is representable in fp32, so one reference serves both dtypes
  for c in gc.CASES:
    if c.group == 'N' or c.dtype == 'fp32':
      continue
    inp = gc.inputs(c)
    for a in inp.x + inp.vecs + [s for s in inp.s if s is not None] + [inp.lh, inp.c, inp.model['lin_w']] + ([inp.model['ls']] if inp.model['ls'] is not None else []):
      assert np.array_equal(a, a.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize('cid', _ids(gc.GROUP_N))
def test_anchor_reference_is_the_oracles_nll_gradient(cid):
  """The hook's conventions are the objective's: G = lh K^-1 - c alpha alpha^T of a real NLL gives the oracle's kernel leaves."""
  case = gc.BY_ID[cid]
  ref, want, scale = gc.reference(case), gc.anchor_oracle_leaves(case), gc.leaf_scales(case)[0]
  kernel = scale > 0
  assert kernel.sum() == (3 if case.kname == gc.DOT else case.fdim + 2)
  err = np.abs(ref.grad[0] - want)
  assert np.all(err[kernel] <= gc.ANCHOR_TOL * scale[kernel]), (err / np.where(kernel, scale, 1)).astype(float)
  assert np.all(ref.grad[0][~kernel] == 0) and np.all(want[~kernel] == 0)


@pytest.mark.parametrize('cid', _ids(c for c in gc.CASES if c.group in gc.SHARE_GROUPS and c.dtype == 'fp64'))
def test_every_half_tile_carries_its_share(cid):
  """Of the un-cancelled scale of every slot it reaches (a tile off the diagonal has no trace, a one-point tile no pair at a distance):
  SHARE_MIN on grids of up to SHARE_MAX_TILES half tiles; the shares sum to 1, so beyond that SHARE_FAIR of an equal share."""
  case = gc.BY_ID[cid]
  ref = gc.reference(case)
  for k, n in enumerate(case.ns):
    tiles = gc.half_tiles(n)
    need = gc.SHARE_MIN if len(tiles) <= gc.SHARE_MAX_TILES else gc.SHARE_FAIR / len(tiles)
    for slot, ti, h, tj, (r0, r1), (c0, c1) in tiles:
      for q in range(case.nacc):
        if q == case.nacc - 1 and case.obj != 'euc':             # the Frobenius slot: read by EUC alone
          continue
        if q == 1:
          reach = ti == tj and max(r0, c0) < min(r1, c1)          # the trace: tiles that hold diagonal entries
        elif q in (0, case.nacc - 1) or case.kname == gc.DOT:
          reach = True
        else:
          reach = (r1 - r0) * (c1 - c0) > 1                       # a length-scale slot: some pair at a distance
        if not reach:
          assert ref.parts_abs[k][slot, q] == 0
          continue
        share = ref.parts_abs[k][slot, q] / ref.tots_abs[k][q]
        assert share >= need, (k, (ti, h, tj), q, float(share), need)


@pytest.mark.parametrize('cid', _ids(gc.CASES))
def test_restatement_stays_inside_its_share_of_the_bound(cid):
  case = gc.BY_ID[cid]
  rs = gc.restate(case)
  assert _worst(case, rs) <= gc.RESTATE_SHARE
  if case.mlp:
    ref = gc.reference(case)
    for k, b in enumerate(gc.df_bounds(case)):
      assert float(np.max(gc._ratio(rs.dF[k], ref.dF[k], b))) <= gc.RESTATE_SHARE   # pylint: disable=protected-access
  assert gc.judge(case, rs.grad, rs.parts, rs.fro, rs.dF) <= gc.RESTATE_SHARE


def test_c2_is_the_smallest_round_number():
  """C2 from gc.ROUND: with the round number below it the restatement leaves its share on some case."""
  worst = 0.0
  for case in gc.CASES:
    rs = gc.restate(case)
    r = gc.leaf_ratios(case, rs.grad, rs.fro if case.obj == 'euc' else None, gc.C1, gc.ROUND[gc.ROUND.index(gc.C2) - 1])
    worst = max(worst, max(float(np.max(r[0])), float(np.max(r[1]))) if isinstance(r, tuple) else float(np.max(r)))
  assert worst > gc.RESTATE_SHARE


_PAIRS = [(m, c.id) for m in gc.MUTANTS for c in gc.CASES if gc.applies(m, c) and c.group != 'N']


@pytest.mark.parametrize('mutant,cid', _PAIRS)
def test_every_mutant_fails_the_bound(mutant, cid):
  case = gc.BY_ID[cid]
  far = _worst(case, gc.restate(case, mutant))
  if (mutant, cid) in gc.WEAK:
    assert far > 1.0, 'a weak pair still fails the bound'
    assert far < gc.MUTANT_FACTOR, 'no longer weak: take it out of WEAK'
  else:
    assert far >= gc.MUTANT_FACTOR, far


def test_weak_table_is_small_and_keeps_out_of_a_and_g():
  assert all(k in set(_PAIRS) for k in gc.WEAK)
  assert len(gc.WEAK) <= 0.1 * len(_PAIRS)
  assert not any(gc.BY_ID[cid].group in ('A', 'G') or gc.BY_ID[cid].dtype == 'fp64' for _, cid in gc.WEAK)
  for m in gc.MUTANTS:
    assert any(mm == m for mm, _ in _PAIRS), m
