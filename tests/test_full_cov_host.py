"""CPU tier of the full-covariance tests: tests/full_cov_oracle.py judged on its own, so that tests/test_gpu_full_cov.py cannot pass
vacuously (as test_split_products_host.py and test_acq_host.py do for their tiers).  For every case of the list:

  * the inputs make the posterior correction most of EVERY 128-tile of the query grid (max |Kqq - cov| >= 0.5 max |Kqq| per tile),
    so that a tile that skipped it is wrong by the prior's scale;
  * two independent fp64 routes to the covariance agree to 1e-10 of max |cov|: the reference's own uncertainty is far below every
    bound applied to the device;
  * every mutant of the reference -- one per failure the kernels could have -- moves an entry by at least 100 x the bound the GPU test
    applies to that case and dtype.  A mutant whose failure cannot exist at a shape (one row has no pitch, one tile column has no
    second one, n = 128 has no padded rows) returns None there and full_cov_oracle.not_applicable() says so by the shape alone; a
    mutant that exists but is too weak is listed in full_cov_oracle.WEAK_FP32, at most one per case and none at n = M = 300;
  * the reference of a subset of the queries is the sub-matrix of the reference of all of them (the resident-grid test relies on it).

The resident-grid cases (n = 4096) are judged on the subset of queries the GPU test checks (four per 128-tile, 16 entries of every
tile); the mutants address tiles, blocks and pitches and are run at the edge shapes."""
import numpy as np
import pytest

import full_cov_oracle as F

SMALL = [c for c in F.CASES if c.group != 'resident']
IDS = lambda c: c.id


def _subset(case):
  return None if case.group != 'resident' else F.resident_subset(case.M)


def _tile_fractions(case, ref, idx):
  """Per 128-tile of the whole query grid: max |Kqq - cov| over the entries of the tile that are looked at, of max |Kqq|."""
  if idx is None:
    return F.tile_errors(ref.kqq, ref.cov) / np.max(np.abs(ref.kqq))
  t = idx // F.TILE
  nt = int(t.max()) + 1
  out = np.zeros((nt, nt))
  np.maximum.at(out, (t[:, None].repeat(len(t), 1), t[None, :].repeat(len(t), 0)), np.abs(ref.kqq - ref.cov))
  return out / np.max(np.abs(ref.kqq))


@pytest.mark.parametrize('case', F.CASES, ids=IDS)
def test_posterior_correction_is_most_of_every_tile(case):
  idx = _subset(case)
  frac = _tile_fractions(case, F.reference(case, idx), idx)
  assert frac.shape == (-(-case.M // F.TILE),) * 2
  worst = np.unravel_index(int(np.argmin(frac)), frac.shape)
  assert frac.min() >= F.CONDITION, f'{case.id}: tile {worst} holds only {frac.min():.3f} of max |Kqq|: give the case other inputs'


@pytest.mark.parametrize('case', F.CASES, ids=IDS)
def test_two_fp64_routes_agree(case):
  idx = _subset(case)
  ref = F.reference(case, idx)
  gap = np.max(np.abs(F.second_route(case, idx) - ref.cov)) / np.max(np.abs(ref.cov))
  assert gap <= F.ROUTE_GAP_TOL, f'{case.id}: {gap:.2e} (raise the case\'s noise variance)'
  assert np.array_equal(ref.cov.shape, (len(ref.mu),) * 2) and np.isfinite(ref.cov).all() and np.isfinite(ref.mu).all()


def test_fp32_yardstick_is_float32_arithmetic():
  """Of the order of the fp32 unit roundoff times a modest factor on the operands' scale: neither exact (it would measure nothing) nor
  large (it would excuse anything)."""
  for case in (c for c in SMALL if c.n == 300 and c.M == 300 and c.dtype == 'fp32'):
    ref = F.reference(case)
    y = F.fp32_yardstick(case)
    assert y.dtype == np.float32
    err = np.max(np.abs(y - ref.cov)) / np.max(np.abs(ref.kqq))
    assert 1e-8 < err < 1e-5, (case.id, err)


def _threshold(case, ref, gram_form='default'):
  tol, scale_name = F.cov_bound(case, gram_form)
  return F.MUTANT_FACTOR * tol * float(np.max(np.abs(ref.cov if scale_name == 'cov' else ref.kqq)))


@pytest.mark.parametrize('case', SMALL, ids=IDS)
def test_every_mutant_is_far_outside_the_gpu_bound(case):
  ref = F.reference(case)
  threshold = max(_threshold(case, ref, form) for form in (('default', 'direct') if case.group == 'wide' else ('default',)))
  na, weak = F.not_applicable(case), F.weak_mutants(case)
  assert len(weak) <= 1 and not (set(weak) & na)
  if case.n == 300 and case.M == 300:
    assert not weak and not na, 'every mutant must be live at n = M = 300'
  moved = {}
  for name, mutant in F.MUTANTS.items():
    out = mutant(case)
    assert (out is None) == (name in na), f'{case.id}: mutant ({name}) and not_applicable() disagree'
    if out is None:
      continue
    assert out.shape == ref.cov.shape
    moved[name] = float(np.max(np.abs(out - ref.cov)))
    if name in weak:
      assert moved[name] < threshold, f'{case.id}: mutant ({name}) is live ({moved[name]:.3e} >= {threshold:.3e}): take it off WEAK_FP32'
    else:
      assert moved[name] >= threshold, f'{case.id}: mutant ({name}) moves no entry by more than {moved[name]:.3e} < {threshold:.3e}'
  if case.M > 1 and case.dtype == 'fp64':   # the pitch error the other way
    assert np.max(np.abs(F.mutant_d(case, -32) - ref.cov)) >= threshold


@pytest.mark.parametrize('case', F.CASES, ids=IDS)
def test_reference_of_a_subset_is_the_submatrix(case):
  rng = np.random.default_rng(case.M)
  if case.group == 'resident':
    idx = F.resident_subset(case.M)
    whole = F.reference(case, idx)
    pick = np.sort(rng.choice(len(idx), size=len(idx) // 4, replace=False))
    sub = F.reference(case, idx[pick])
  else:
    whole = F.reference(case)
    pick = np.sort(rng.choice(case.M, size=max(1, case.M // 3), replace=False))
    sub = F.reference(case, pick)
  scale = np.max(np.abs(whole.kqq))
  assert np.max(np.abs(sub.cov - whole.cov[np.ix_(pick, pick)])) <= 1e-12 * scale
  assert np.max(np.abs(sub.kqq - whole.kqq[np.ix_(pick, pick)])) <= 1e-12 * scale
  assert np.max(np.abs(sub.mu - whole.mu[pick])) <= 1e-12 * max(np.max(np.abs(whole.mu)), 1.0)


def test_case_list_covers_what_the_gpu_tier_needs():
  sizes = {(c.n, c.M) for c in F.EDGE_CASES}
  assert sizes == set(F.EDGE_SIZES) and len(F.EDGE_CASES) == len(F.FAMILIES) * len(F.EDGE_SIZES) * 2
  assert {c.kname for c in F.EDGE_CASES} == {'squared_exponential', 'matern32', 'matern52', 'dot_product'}
  assert any(c.kumar for c in F.EDGE_CASES) and any(c.mlp for c in F.EDGE_CASES)
  assert F.resident_sizes(256) == (4224, 4096)
  for cus in (256, 304, 64, 8):   # just above / at (M / 128) * 32 = 4 * CUs
    hi, lo = F.resident_sizes(cus)
    assert (hi // 128) * 32 > 4 * cus >= (lo // 128) * 32 and hi - lo == 128
  idx = F.resident_subset(4224)
  assert len(idx) == 33 * F.RESIDENT_PER_TILE and len(set(idx.tolist())) == len(idx) and idx.max() == 4223
  assert all(np.sum(idx // 128 == t) == F.RESIDENT_PER_TILE for t in range(33))
  assert F.FP32_COV_TOL is not None and F.FP32_COV_TOL_WIDE_MFMA is not None
