"""tests/inverse_cases.py judged on its own, on the CPU: the conditions under which tests/test_gpu_inverse.py may ask the device for the
exact integers -- (a) the designs are what they claim, (b) every block product the algorithms must perform contributes on every case
(zero exceptions, on the 128-grid and on the 64-grid of the small shapes), (c) every operand and partial sum fits fp32, bf16x3 and f16x2
exactly -- (d) the compare function finds a planted entry in its tile and nowhere else, and the real-valued family's yardstick lies well
inside the bound the device is held to.
"""
import ctypes as C
import zlib

import numpy as np
import pytest

from hyperbo_amd import _native as nat

import inverse_cases as ic
import split_oracle as so

KEYS = ic.all_task_keys()
KEY_IDS = ['n%d_s%d' % k for k in KEYS]


# ---- (a) -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', KEYS, ids=KEY_IDS)
def test_exact_cases_are_integer_factors_with_integer_inverses(key):
  c = ic.exact_case(*key)
  n, L, W = c['n'], c['L'], c['W']
  I = np.eye(n, dtype=np.int64)
  N = L - I
  N2 = so._mm(N, N)
  assert np.array_equal(np.diag(L), np.ones(n, np.int64)) and not np.triu(L, 1).any() and set(np.unique(L)) <= {-1, 0, 1}
  assert np.array_equal(so._mm(L, W), I) and not so._mm(N2, N2).any()          # L W = I, N^4 = 0
  assert np.array_equal(so._mm(L, L.T), c['A']) and np.array_equal(so._mm(W.T, W), c['Kinv'])
  assert np.array_equal(so._mm(L, c['z']), c['b']) and np.array_equal(so._mm(c['A'], c['x']), c['b'])
  assert c['b'].shape == (n, ic.M_RHS)


def test_tasks_of_a_batch_differ():
  """a tile taken from the neighbouring task is a wrong tile: no two tasks of a batch share a leading block of L, W or K^-1"""
  for name, ns in ic.BATCHES.items():
    cases = [ic.exact_case(n, ic.task_seed(k)) for k, n in enumerate(ns)]
    for i, a in enumerate(cases):
      for b in cases[i + 1:]:
        k = min(a['n'], b['n'], ic.TILE)
        if k < 8:
          continue   # (the one-point task)
        for key in ('L', 'W', 'Kinv'):
          assert not np.array_equal(a[key][:k, :k], b[key][:k, :k]), (name, a['n'], b['n'], key)


def test_exact_spd_of_split_oracle_is_unchanged():
  """tests/test_gpu_split_products.py depends on split_oracle.exact_spd as it stands: its output at n = 219, seed 0, by checksum"""
  A, L, W = so.exact_spd(219)
  assert A.dtype == L.dtype == W.dtype == np.int64
  assert (zlib.crc32(A.tobytes()), zlib.crc32(L.tobytes()), zlib.crc32(W.tobytes())) == (760097106, 4265546974, 399697132)
  assert np.count_nonzero(L) - 219 == 834            # at most per_row = 5 per row: the stock design, not the dense one


# ---- (b) -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', KEYS, ids=KEY_IDS)
def test_every_block_product_contributes(key):
  c = ic.exact_case(*key)
  for tile in (ic.TILE, ic.TILE // 2):
    zeros = ic.zero_triples(c, tile)
    assert zeros == [], 'n=%d seed=%d tile=%d: %d of %d block products contribute nothing: %s' % (
        key[0], key[1], tile, len(zeros), ic.count_triples(key[0], tile), zeros[:8])


def test_the_stock_design_does_not_meet_the_condition():
  """why the dense variant exists: split_oracle.exact_spd leaves block products with a ragged last block of one row empty"""
  A, L, W = so.exact_spd(897)
  assert len(ic.zero_triples(dict(n=897, L=L, W=W), ic.TILE)) > 0


# ---- (c) -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', KEYS, ids=KEY_IDS)
def test_exact_cases_fit_fp32_and_both_split_forms(key):
  """csrc/post3.hip's header: bf16x3 -- "an fp32 number is EXACTLY the sum of three bf16 numbers (24 significand bits = 8 + 8 + 8"), the
  six retained products "formed exactly by the bf16 MFMA (8 x 8 bit products) and accumulated in its fp32 accumulator": operands of at
  most 16 significant bits have no third plane, so nothing is dropped.  f16x2 -- "fp16 carries 11 bits, so TWO pieces hold 22 of an fp32
  number's 24 significand bits", "the three products h h' + h l' + l h' (each exact in the fp32 accumulator: 11 x 11 bits)": a
  factor-side operand (L, W, every S21) of at most 11 bits is its h plane alone, so no product has an l plane on both sides; z may
  use h + l (22 bits).  "entries below 2^-14 of that [the largest magnitude, mapped to [2^13, 2^14)] lose bits of l": every non-zero
  entry here is an integer >= 1 beside a maximum below 2^11, far above 2^-14 of it.  And every partial sum, in any order, is an
  integer below 2^24: exact in the fp32 accumulators and in fp32 storage (fp64: below 2^53)."""
  c = ic.exact_case(*key)
  r = ic.fit_report(c)
  assert r['factor_bits'] <= 11 and r['factor_max'] < 2 ** 11, r
  assert r['z_bits'] <= 16 and r['z_max'] < 2 ** 11, r
  assert r['sweep_bits'] <= 11 and r['sweep_max'] < 2 ** 11, r                     # the sweep's running matrix, qs in 1, 2, 4, 8
  assert r['reach'] < 2 ** 22 and r['out_max'] < 2 ** 22, r
  assert r['reach'] <= 2 ** 15, r                                                  # (what the issue's own check of the variant reached: <= 2^11 ... 2^15)
  # the f16x2 a-priori scale of L's blocks: |L_ij| <= sqrt(max A_ii)
  assert np.abs(c['L']).max() ** 2 <= r['a_diag_max']
  for k in ('A', 'L', 'W', 'Kinv', 'b', 'z', 'x'):
    assert so.is_fp32(c[k]), k


def test_not_pd_variant():
  c = ic.exact_case(1290, ic.task_seed(4))
  A, r = ic.not_pd_case(c, 2 * ic.TILE + 37)
  assert r // ic.TILE == 2 and np.array_equal(A[:r, :r], c['A'][:r, :r]) and (A != c['A']).sum() == 1
  # the rows before r factorise to the same integers; the Schur complement's pivot at r is -1
  L0 = c['L'][:r, :r]
  row = so._mm(A[r:r + 1, :r], np.linalg.inv(L0.astype(np.float64)).round().astype(np.int64).T)
  assert np.array_equal(row[0], c['L'][r, :r]) and int(A[r, r] - (row ** 2).sum()) == -1


# ---- (d) -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [129, 515, 1290])
def test_compare_tiles_finds_a_planted_entry_in_its_tile_only(n):
  c = ic.exact_case(n, 0)
  rng = np.random.default_rng(n)
  nb = -(-n // ic.TILE)
  for name, (want, mask) in ic.expected_outputs(c).items():
    got32 = want.astype(np.float32)
    assert not ic.compare_tiles(got32, want, mask).any() and not ic.compare_tiles(want.copy(), want, mask).any()
    nr, nc = -(-want.shape[0] // ic.TILE), -(-want.shape[1] // ic.TILE)
    for tr in range(nr):
      for tc in range(nc):
        r = rng.integers(tr * ic.TILE, min((tr + 1) * ic.TILE, want.shape[0])); q = rng.integers(tc * ic.TILE, min((tc + 1) * ic.TILE, want.shape[1]))
        for planted in (want[r, q] + 1, np.nan):
          got = want.copy(); got[r, q] = planted
          counts = ic.compare_tiles(got, want, mask)
          looked_at = mask is None or mask[r, q]
          expect = np.zeros((nr, nc), np.int64); expect[tr, tc] = int(looked_at)
          assert np.array_equal(counts, expect), (name, tr, tc, planted)
    if name in ('chol', 'w'):   # above the diagonal: zeros are part of what is compared
      assert not np.triu(want, 1).any()
      got = want.copy(); got[0, n - 1] = 1.0
      assert ic.compare_tiles(got, want, mask)[0, nb - 1] == 1
  # K^-1: tiles above the tile diagonal are scratch and not looked at, whole diagonal tiles are
  m = ic.lower_tile_mask(n)
  assert m[0, min(n, ic.TILE) - 1] and (n <= ic.TILE or not m[0, ic.TILE]) and m[n - 1, 0]


# ---- the option sets ---------------------------------------------------------------------------------------------------------------------
def test_option_sets_cover_what_the_tier_claims():
  sets = ic.OPTION_SETS
  names = [s.name for s in sets]
  assert len(set(names)) == len(names)
  vals = lambda k: {s.opts.get(k, ic.OPTION_DEFAULTS[k]) for s in sets}
  assert {0, 2} <= vals('lookahead') and {1, 2, 3, 4, 8} <= vals('potrf_group') and {0, 1} <= vals('overlap_trtri') and {12, 60} <= vals('trtri_at')
  assert {1, 2, 8} <= vals('sweep_qs') and {0, 4, -1} <= vals('small_nblk') and {0, 1 << 30} <= vals('sweep_big') and {0, 1, 2} <= vals('batch_bg')
  assert {0, 2} <= vals('split_f1') and {0, 1} <= vals('sweep_side') and 0 in vals('lauum_persist') and {0, 200} <= vals('trtri_free') and {0, 1} <= vals('cu_yield')
  assert any(s.opts.get('potrf_group') == 4 and s.opts.get('group_inner') == 2 for s in sets) and any(s.opts.get('potrf_group') == 8 and s.opts.get('group_inner') == 4 for s in sets)
  assert {s.beside for s in sets} == {0, 1}
  planned = lambda **kw: [s for s in sets if all(s.plan.get(k) == v for k, v in kw.items())]
  for qs in ic.SWEEP_QS:                                   # the sweep, each row-group size; one matrix and batches
    assert planned(sweep=1, qs=qs), qs
  single = lambda s: not isinstance(s.shapes[0], str)
  assert any(single(s) for s in planned(early=1)) and any(not single(s) for s in planned(early=1, tgran=4))
  assert planned(small_shape=0) and planned(small_shape=1)
  for bg in (0, 1, 2):
    assert any(not single(s) for s in planned(sweep=1, batch_bg=bg)), bg
  assert {s.forms[0] for s in sets if s.forms} == {0, 1, 2} and {s.forms[1] for s in sets if s.forms} >= {0, 1, 1 | 4, 2 | 8}
  assert any(s.forms and s.opts.get('trtri3_min_s') == 1 and s.opts.get('small_nblk') == 0 and single(s) for s in sets)
  # every (set, shape) fits the hook
  for s in sets:
    for shape in s.shapes:
      ns, seeds = ic.shape_ns(shape)
      assert 1 <= len(ns) <= 64 and all(1 <= n <= 4096 for n in ns) and all((n, sd) in KEYS for n, sd in zip(ns, seeds))
  assert len(ic.BATCHES['B3']) > 8 and all(260 <= n <= 520 for n in ic.BATCHES['B3'])


def test_binding_matches_the_header():
  res, args = nat.SIGNATURES['hbo_probe_factor_inverse']
  assert res is C.c_int and len(args) == 15
  assert C.sizeof(nat.ProbePlan) == 13 * 4


# ---- the real-valued family ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', ic.REAL_NS)
def test_real_reference_and_yardstick(n):
  """the longdouble reference reproduces K; LAPACK's float64 L, W and W^T W lie under a quarter of the bound the device is held to"""
  c = ic.real_case(n)
  L, W = c['ref']['chol'], c['ref']['w']
  assert L.dtype == np.longdouble and np.finfo(np.longdouble).eps < 1e-18
  k = min(n, 300)    # (longdouble products are slow: a leading and a trailing block)
  assert np.abs(L[:k] @ L[:k].T - c['K'][:k, :k]).max() < 1e-17 and np.abs(L[-k:] @ L[-k:].T - c['K'][-k:, -k:]).max() < 1e-17
  assert np.abs(L[-k:] @ W[:, -k:] - np.eye(n)[-k:, -k:]).max() < 1e-15 * np.abs(W).max()
  assert np.array_equal(c['ref']['kinv'][-1, -k:], (W[-1:, -1:].T @ W[-1:, -k:])[0])
  for name in ('chol', 'w', 'kinv'):
    bound, yard = ic.real_bound(c, name)
    print('n=%d %s: yardstick %.3e, bound %.3e' % (n, name, yard, bound))
    assert 0 < yard < 0.25 * bound
  # the per-tile error sees one wrong entry in its tile only
  got = np.array(c['yard']['w']); got[n - 1, 0] += 1e-3
  err = ic.tile_errors(got, c['ref']['w'], ic.real_masks(n)['w'])
  nb = -(-n // ic.TILE)
  assert err[nb - 1, 0] > 1e-6 and (np.delete(err.ravel(), (nb - 1) * nb) < 1e-11).all()
