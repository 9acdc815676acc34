"""CPU tier: the operand designs of tests/split_oracle.py are what tests/test_gpu_split_products.py takes them for -- representable,
exact in the retained product, exact in every partial sum the kernels of hyperbo_amd/csrc/post3.hip may form, and sensitive to every
mutant of the emulation -- so that the GPU tests cannot pass vacuously.  No GPU, no libhbo.

Quanta (weight of the lowest bit of any product) and measured headroom (bits a partial sum can reach over the quantum; the limit is
22 = fp32's 24 minus two), n = 384, 200 candidates:
  dense            bf16x3 quantum 1        8.0 bits      f16x2 (scaled by 2^12 2^12) quantum 2^24   8.0 bits
  pair(1,0) (0,1)  bf16x3 quantum 2^-9    11.0 bits
  pair(2,0) (0,2)  bf16x3 quantum 2^-18   20.0 bits
  pair(1,1)        bf16x3 quantum 2^-18   21.0 bits
  pair(1,0) (0,1)  f16x2  (scaled by 2^13 and 2^12 / 2^13) quantum 2^13   14.0 bits
"""
import numpy as np
import pytest
import torch

import split_oracle as so

SHAPES = ((100, 70), (300, 200), (384, 200))   # one ragged block; three blocks, ragged; three full blocks
_cache = {}


def designs(n, M):
  if (n, M) not in _cache:
    _cache[(n, M)] = {(d.name, d.form): d for d in so.all_designs(n, M)}
  return _cache[(n, M)]


DESIGN_KEYS = sorted(designs(100, 70))


def _ref_colsq(d):
  key = ('colsq', d.name, d.form, d.n, d.M)
  if key not in _cache:
    _cache[key] = so.colsq_of(so.emulate_V(d), d.n)
  return _cache[key]


# ---- the emulation itself ----------------------------------------------------------------------------------------------------------
def _random_fp32(rng, n, lo_exp, hi_exp):
  mant = 1 + rng.integers(0, 1 << 23, size=n) / float(1 << 23)
  return (rng.choice([-1.0, 1.0], size=n) * mant * np.exp2(rng.integers(lo_exp, hi_exp + 1, size=n))).astype(np.float32)


def test_bf16_cast_is_torchs():
  rng = np.random.default_rng(0)
  x = np.concatenate([_random_fp32(rng, 20000, -120, 120), np.float32([0, 1, -1, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20])])
  want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
  assert np.array_equal(so.bf16_rne(x), want)


def test_bf16_three_way_split_is_exact():
  """x0 + x1 + x2 == x for random fp32 values over the whole range in which it can hold: from 2^-110 (below, the third plane would need
  bits under bf16's smallest subnormal 2^-133; the residual is then at most half of that) up to the largest fp32 whose bf16 rounding
  is finite, (2 - 2^-8) 2^127 exclusive (above, bf16(x) is inf: the largest 0.2 % of the fp32 range has no bf16 split)."""
  rng = np.random.default_rng(1)
  top = np.nextafter(np.float32((2 - 2.0 ** -8) * 2.0 ** 127), np.float32(0))
  x = np.concatenate([_random_fp32(rng, 50000, -110, 126), np.float32([top, -top, 2.0 ** -110, (2 - 2.0 ** -23) * 2.0 ** -110])])
  x = x[np.abs(x) <= top]
  x0, x1, x2 = (p.astype(np.float64) for p in so.split3(x))
  assert np.array_equal(x0 + x1 + x2, x.astype(np.float64))
  # the smallest normal magnitudes: not exact, but off by no more than half a bf16 subnormal step
  tiny = _random_fp32(rng, 5000, -126, -111)
  t0, t1, t2 = (p.astype(np.float64) for p in so.split3(tiny))
  assert np.abs(t0 + t1 + t2 - tiny.astype(np.float64)).max() <= 2.0 ** -134


@pytest.mark.parametrize('amax_exp', [127, 0, -40])
def test_fp16_two_way_residual(amax_exp):
  """|x s - h - l| <= 2^-22 |x s| for the entries within 2^14 of the maximum, whatever the maximum's magnitude down to 2^-41
  (hbo_h2_scale_for clamps the exponent there, so that neither a scale nor a ratio of two scales leaves the fp32 range)."""
  rng = np.random.default_rng(200 + amax_exp)
  amax = np.float32(1.9 * 2.0 ** amax_exp)
  x = (_random_fp32(rng, 50000, amax_exp - 14, amax_exp - 1)).astype(np.float32)
  x = np.concatenate([x, [amax, -amax]]).astype(np.float32)
  s = so.h2_scale_for(amax)
  assert 2.0 ** 13 <= float(amax) * s < 2.0 ** 14
  h, l, y = (p.astype(np.float64) for p in so.split2h(x, s))
  assert np.isfinite(h).all() and np.all(np.abs(y - h - l) <= 2.0 ** -22 * np.abs(y))


def test_scale_twins_agree():
  for b in (1e-11, 0.3, 1.0, 2.0, 3.0, 8191.0, 8192.0, 1e20):
    assert so.h2_scale_for(b) == so.post2h_scale_for(b) and 2.0 ** 13 <= b * so.h2_scale_for(b) < 2.0 ** 14
  assert so.h2_scale_for(0) == so.post2h_scale_for(0) == 1.0 and so.h2_scale_for(np.inf) == 1.0
  assert so.h2_scale_for(1e-30) == 2.0 ** 54   # (the device twin clamps the exponent at -40; the host twin is only handed model bounds)


# ---- every design: representable, exact, with headroom -------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'n%d_M%d' % s)
@pytest.mark.parametrize('key', DESIGN_KEYS, ids=lambda k: '%s-%s' % k)
def test_design_is_representable_and_exact(key, shape):
  d = designs(*shape)[key]
  assert d.W.dtype == np.float32 and d.K.dtype == np.float32 and not np.triu(d.W, 1).any()
  a, b, sw, sk = so.planes_of(d)
  Wp, Kp = so._pad(d)
  # the planes add up to the operand
  assert np.array_equal(sum(a), Wp.astype(np.float64) * sw) and np.array_equal(sum(b), Kp.astype(np.float64) * sk)
  if d.form == 'f16x2':
    assert 2.0 ** 13 <= np.abs(Wp).max() * sw < 2.0 ** 14 and np.abs(Kp).max() <= d.k_bound and 2.0 ** 13 <= d.k_bound * sk < 2.0 ** 14
    assert all(np.abs(p).max() <= 65504 for p in a + b)
    # never wide on both sides at the same k: l l' is dropped by design
    assert not ((np.abs(a[1]).sum(axis=0) > 0) & (np.abs(b[1]).sum(axis=1) > 0)).any()
  i, j = d.own if d.own else (0, 0)
  assert (a[i] != 0)[Wp != 0].all() and (b[j] != 0)[Kp != 0].all(), 'the designated planes are non-zero in every non-zero entry'
  # the retained product is the exact product, V consists of the designated product alone
  V = so.exact_V(d)
  assert np.array_equal(so.emulate_V(d), V)
  assert np.array_equal((a[i] @ b[j] / (sw * sk))[:d.n], V)
  # partial sums, 16-blocks of k ascending, any order inside a block: two bits of headroom
  assert so.headroom_bits(d) <= 22.0
  # colsq: representable in fp32, and so is every partial sum of the (non-negative) squares; no output is zero
  cs = so.exact_colsq(d)
  q2 = (d.quantum if d.form == 'bf16x3' else d.quantum / (sw * sk)) ** 2
  assert so.is_fp32(cs) and cs.max() < 2.0 ** 24 * q2 and np.array_equal(np.rint(cs / q2) * q2, cs) and (cs > 0).all()


def test_resident_grid_shape_is_exact_too():
  """the largest GPU case (three blocks, enough candidates for a resident grid on 256 CUs): colsq still fits fp32"""
  for form in ('bf16x3', 'f16x2'):
    d = so.design_dense(384, 43800, form)
    cs = so.exact_colsq(d)
    assert so.is_fp32(cs) and cs.max() < 2.0 ** 24 and (cs > 0).all()
    assert np.abs(so.exact_V(d)).max() * 3 * 3 * 16 < 2.0 ** 22   # (a block adds at most 16 * 3 * 3 to a partial sum)


# ---- mutants -------------------------------------------------------------------------------------------------------------------------
def _killed(d, mutant, mask=None):
  return so.killed_fraction(_ref_colsq(d), so.colsq_of(so.emulate_V(d, mutant), d.n), mask)


def _tiles_with_full_range(d):
  """outputs of the row tiles whose K range ends inside the matrix (the last 16-block of a ragged last tile is padding)"""
  nblk = so.npad_of(d.n) // so.TILE
  mask = np.zeros((nblk, d.M), bool)
  mask[:d.n // so.TILE] = True
  return mask


@pytest.mark.parametrize('shape', SHAPES[1:], ids=lambda s: 'n%d_M%d' % s)
@pytest.mark.parametrize('key', DESIGN_KEYS, ids=lambda k: '%s-%s' % k)
def test_pair_designs_answer_to_their_own_product_only(key, shape):
  d = designs(*shape)[key]
  own = d.own if d.own else (0, 0)
  for p in d.pairs:
    assert _killed(d, ('drop', p)) == (1.0 if p == own else 0.0), p
  # the halves of a stage exchanged on the designated plane of either operand alone
  assert _killed(d, ('swap_halves', 'W', own[0])) >= 0.99 and _killed(d, ('swap_halves', 'K', own[1])) >= 0.99
  if d.form == 'f16x2':
    assert _killed(d, ('scale2', 'W')) == 1.0 and _killed(d, ('scale2', 'K')) == 1.0


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'n%d_M%d' % s)
@pytest.mark.parametrize('form', ['bf16x3', 'f16x2'])
def test_dense_answers_to_every_structural_mutant(form, shape):
  d = designs(*shape)[('dense', form)]
  assert _killed(d, ('drop_kblock', 'start')) >= 0.99
  if d.n >= so.TILE:
    assert _killed(d, ('drop_kblock', 'end'), _tiles_with_full_range(d)) >= 0.99
  assert _killed(d, ('swap_halves', 'W', 0)) >= 0.99 and _killed(d, ('swap_halves', 'K', 0)) >= 0.99


@pytest.mark.parametrize('form', ['bf16x3', 'f16x2'])
def test_every_plane_exchange_is_caught_by_some_design(form):
  """Two planes of one operand (or of both: emit8 writes both operands' planes) exchanged: a design whose other operand is narrow
  cannot see it (every a_i b_0 is retained), so each exchange is judged on the designs that can -- at least one must answer 100 %."""
  ds = [d for d in designs(300, 200).values() if d.form == form]
  npl = 3 if form == 'bf16x3' else 2
  for op in ('W', 'K', 'both'):
    for p in range(npl):
      for q in range(p + 1, npl):
        best = max(_killed(d, ('swap_planes', op, p, q)) for d in ds)
        assert best == 1.0, (op, p, q, best)


def test_range_design_meets_the_documented_loss_exactly():
  """f16x2, one entry 2^13 times the typical one: the emulation loses exactly what post3.hip's header says -- 2^-25 of the scaled
  operand per small entry -- and nothing else (all partial sums exact), so the bound the GPU test derives is attained, not slack."""
  d = so.design_range(300, 200)
  assert so.is_fp32(d.W) and so.h2_scale_for(np.abs(d.W).max()) == 2.0 ** -5 and so.headroom_bits(d) <= 22.0
  _, l, y = so.split2h(d.W, 2.0 ** -5)
  small = (d.W != 0) & (np.abs(d.W) < so.RANGE_BIG)
  assert np.all(np.abs(l[small]) == 2.0 ** -14) and np.all(np.abs(y[small]) < 2.0 ** -14 * np.abs(y).max())
  err = np.abs(so.emulate_V(d) - so.exact_V(d))
  bound = so.range_bounds(d)
  assert (err <= bound).all() and err.max() > 0.5 * bound.max()
  # a split that took its scale from the typical entries (not from the maximum over all blocks) would overflow fp16 on the large one
  assert not np.isfinite(so.split2h(np.float32(so.RANGE_BIG), so.h2_scale_for(so.RANGE_SMALL))[0])


# ---- the factorisation's exact inputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nblk', [2, 3, 5, 6, 7])
def test_spd_cases_fit_both_forms(nblk):
  n = 128 * nblk - 37
  for m, big in ((1, False), (5, False), (5, True)):
    c = so.spd_case(n, m, big)
    L, W = c['L'], c['W']
    assert np.array_equal(np.diag(L), np.ones(n, np.int64)) and not np.triu(L, 1).any() and set(np.unique(L)) <= {-1, 0, 1}
    assert np.array_equal(so._mm(c['A'], c['x']), c['b']) and np.array_equal(so._mm(L, c['z']), c['b'])
    r = so.spd_operand_report(c)
    # bf16x3: at most 16 significant bits on both sides.  f16x2: the factor side (L, W, every S21) fits the h plane (11 bits), so no
    # product has an l plane on both sides; z needs at most h + l (22 bits)
    assert r['factor_bits'] <= 11 and r['z_bits'] <= 16
    if big:
      assert r['z_bits'] > 11, 'the right-hand sides near 2^10 make the augmented rows use their second plane'
    # every partial sum and every result far below 2^24; max A_ii bounds the factor's entries (the f16x2 a-priori scale)
    assert r['reach'] < 2 ** 22 and r['out_max'] < 2 ** 22 and np.abs(L).max() ** 2 <= c['A'].diagonal().max()
