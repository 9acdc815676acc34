"""The fp32 products on the 16-bit matrix cores (hyperbo_amd/csrc/post3.hip: bf16x3 and f16x2) on operands whose every product and
partial sum is exact in fp32 (tests/split_oracle.py; proved on the host by tests/test_split_products_host.py): the result is known to
the last bit, and each retained cross product is 100 % of some result instead of 2^-16 of it.

Posterior product: hbo_probe_post_product (include/hbo_tune.h) runs hbo_predict's three launches on the designs.
Factorisation, inverse and K^-1: hbo_spd_solve in fp32 on A = L L^T with an integer L and an integer inverse, on bf16x3, on f16x2
(hbo_tune spd_diag_bound) and on the fp32-MFMA form.  Measured results: profiles/split_products_exact.md.
"""
import ctypes as C

import numpy as np
import pytest

from hyperbo_amd import _native as nat

import split_oracle as so

pytestmark = pytest.mark.gpu

FORM_CODE = {'bf16x3': 0, 'f16x2': 1}
_designs = {}


def designs(n, M):
  if (n, M) not in _designs:
    ds = so.all_designs(n, M)
    _designs[(n, M)] = {(d.name, d.form): (d, so.exact_colsq(d)) for d in ds}
  return _designs[(n, M)]


DESIGN_KEYS = sorted((d.name, d.form) for d in so.all_designs(20, 4))


def probe(ctx, d, use_counter):
  nblk = so.npad_of(d.n) // so.TILE
  out = np.full((nblk, d.M), np.nan, np.float32)
  W = np.ascontiguousarray(d.W, np.float32); K = np.ascontiguousarray(d.K, np.float32)
  ctx.check(nat.lib().hbo_probe_post_product(ctx.handle, FORM_CODE[d.form], nat.ptr(W), d.n, nat.ptr(K), d.M, float(d.k_bound),
                                             int(use_counter), nat.ptr(out)), allow_not_pd=False)
  return out


def _report(tag, got, want):
  diff = np.abs(got.astype(np.float64) - want)
  print('%s: max |diff| %.3e (max expected %.3e), unequal %d of %d' % (tag, np.nanmax(diff) if diff.size else 0.0, want.max(),
                                                                     int((got.astype(np.float64) != want).sum()), want.size))


# ---- the posterior product -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(100, 70), (300, 1000)], ids=lambda s: 'n%d_M%d' % s)   # one ragged block; three blocks, plain grid
@pytest.mark.parametrize('key', DESIGN_KEYS, ids=lambda k: '%s-%s' % k)
def test_posterior_product_is_bit_exact(gpu_ctx, key, shape):
  d, want = designs(*shape)[key]
  for use_counter in (0, 1):   # (at these sizes launch_post3 drops the counter: a plain grid either way)
    got = probe(gpu_ctx, d, use_counter)
    _report('%s %s n=%d M=%d counter=%d' % (d.name, d.form, d.n, d.M, use_counter), got, want)
    assert np.array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize('form', ['bf16x3', 'f16x2'])
def test_posterior_product_resident_grid_is_bit_exact(gpu_ctx, form):
  """three full blocks and so many candidates that the column tiles times 3 exceed 4 x the CUs: with a counter the resident grid
  draws its tiles from it"""
  cus, mem = C.c_int32(0), C.c_int64(0)
  assert nat.lib().hbo_device_info(gpu_ctx.device, None, 0, C.byref(cus), C.byref(mem)) == 0 and cus.value > 0
  col_tiles = 4 * cus.value // 3 + 2
  assert col_tiles * 3 > 4 * cus.value
  d = so.design_dense(384, col_tiles * so.TILE - 57, form)
  want = so.exact_colsq(d)
  assert so.is_fp32(want) and want.max() < 2.0 ** 24 and (want > 0).all()
  got = probe(gpu_ctx, d, 1)
  _report('dense %s resident n=%d M=%d' % (form, d.n, d.M), got, want)
  assert np.array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize('use_counter', [0, 1])
def test_posterior_product_f16x2_range(gpu_ctx, use_counter):
  """One entry of W 2^13 times the typical one, in another block than most of them: not exact.  The bound follows from post3.hip's
  header -- an entry below 2^-14 of the scaled maximum carries an absolute error <= 2^-25 of the scaled operand, here RANGE_LOST per
  typical entry -- and from the design: |dV[r, j]| <= RANGE_LOST sum_k |Kxq[k, j]| over the typical entries of row r (every other
  product and partial sum is exact), so |d colsq| <= sum_r (2 |V| dV + dV^2), plus the fp32 rounding of the kernel's own sum of 128
  squares: each square and each of at most 34 additions along any path (32 per lane, one shuffle, one across the waves) rounds by at
  most 2^-24 of a partial sum <= colsq -- 36 * 2^-24 colsq."""
  d = so.design_range(300, 1000)
  V = so.exact_V(d)
  dV = so.range_bounds(d)
  want = so.colsq_of(V, d.n)
  bound = so.colsq_of(np.sqrt(2 * np.abs(V) * dV + dV ** 2), d.n) + 36 * 2.0 ** -24 * want
  got = probe(gpu_ctx, d, use_counter).astype(np.float64)
  print('range: max |diff| / bound %.3f, max rel diff %.3e, max rel bound %.3e' % ((np.abs(got - want) / bound).max(),
                                                                                 (np.abs(got - want) / want).max(), (bound / want).max()))
  assert np.isfinite(got).all() and np.all(np.abs(got - want) <= bound)


def test_probe_rejects_bad_arguments(gpu_ctx):
  d = so.design_dense(20, 4)
  out = np.zeros((1, 4), np.float32)
  lib, h = nat.lib(), gpu_ctx.handle
  good = (nat.ptr(d.W), 20, nat.ptr(d.K), 4, 2.0, 0, nat.ptr(out))
  assert lib.hbo_probe_post_product(h, 0, *good) == nat.HBO_OK
  assert lib.hbo_probe_post_product(h, 2, *good) == nat.HBO_ERR_ARG
  assert lib.hbo_probe_post_product(None, 0, *good) == nat.HBO_ERR_ARG
  assert lib.hbo_probe_post_product(h, 0, None, 20, nat.ptr(d.K), 4, 2.0, 0, nat.ptr(out)) == nat.HBO_ERR_ARG
  assert lib.hbo_probe_post_product(h, 0, nat.ptr(d.W), 0, nat.ptr(d.K), 4, 2.0, 0, nat.ptr(out)) == nat.HBO_ERR_ARG
  assert lib.hbo_probe_post_product(h, 0, nat.ptr(d.W), 20, nat.ptr(d.K), 0, 2.0, 0, nat.ptr(out)) == nat.HBO_ERR_ARG
  assert lib.hbo_probe_post_product(h, 1, nat.ptr(d.W), 20, nat.ptr(d.K), 4, 0.0, 0, nat.ptr(out)) == nat.HBO_ERR_ARG
  assert lib.hbo_probe_post_product(h, 0, nat.ptr(d.W), 20, nat.ptr(d.K), 4, 2.0, 2, nat.ptr(out)) == nat.HBO_ERR_ARG
  assert lib.hbo_probe_post_product(h, 0, nat.ptr(d.W), 20, nat.ptr(d.K), 4, 2.0, 0, None) == nat.HBO_ERR_ARG


# ---- factorisation, inverse and K^-1 ----------------------------------------------------------------------------------------------------
_cases = {}


def spd_case(n, m, big):
  if (n, m, big) not in _cases:
    _cases[(n, m, big)] = so.spd_case(n, m, big)
  return _cases[(n, m, big)]


def spd_solve(ctx, case):
  A = case['A'].astype(np.float32); b = np.ascontiguousarray(case['b'], np.float32)
  n, m = b.shape
  chol = np.full((n, n), np.nan, np.float32); inv = np.full((n, n), np.nan, np.float32); x = np.full((n, m), np.nan, np.float32)
  rc = ctx.check(nat.lib().hbo_spd_solve(ctx.handle, nat.F32, nat.ptr(A), n, nat.ptr(b), m, nat.ptr(chol), nat.ptr(inv), nat.ptr(x), None))
  assert rc == nat.HBO_OK
  return chol, inv, x


# form -> (bf16x3 option, spd_diag_bound, chol_form, inv_forms)
FORMS = {'bf16x3': (1, 0, 1, 1 | 4), 'f16x2': (1, 1, 2, 2 | 8), 'mfma': (0, 0, 0, 0)}


@pytest.mark.parametrize('nblk', [2, 3, 5, 6, 7])   # one and two levels of the inverse, a cut last group, an odd row-tile count in mode 3
@pytest.mark.parametrize('form', ['bf16x3', 'f16x2', 'mfma'])
def test_spd_solve_is_exact_on_integer_factors(gpu_ctx, form, nblk):
  """chol_out == L, inv_out == W^T W and x_out == A^-1 b to the last bit, with the inverse's modes 1 - 3 forced onto the matrix cores
  (small_nblk = 0, trtri3_min_s = 1), over look-ahead, group size, two-level groups and right-hand sides (1 column, 5 columns, 5
  columns near 2^10: the augmented tile-row's per-chunk scales then differ from the factor's).  The forms are told apart by the
  read-only options chol_form / inv_forms: on exact inputs their results are equal, and the profile's stage names are the same."""
  ctx = gpu_ctx
  n = so.TILE * nblk - 37
  bf, diag, want_chol_form, want_inv_forms = FORMS[form]
  saved = {k: ctx.get_option(k) for k in ('small_nblk', 'lookahead', 'potrf_group', 'bf16x3')}
  scheds = [(la, q, -1) for la in (1, 2) for q in (1, 3)]
  if nblk == 7:
    scheds.append((2, 4, 2))   # two-level groups: the inner update reads the split panels at kb_off != 0
  try:
    ctx.set_option('small_nblk', 0); ctx.set_option('trtri3_min_s', 1)
    ctx.set_option('bf16x3', bf); ctx.set_option('spd_diag_bound', diag); ctx.set_option('chol_f16x2', 1)
    ctx.profile_enable(2)
    for la, q, qi in scheds:
      ctx.set_option('lookahead', la); ctx.set_option('potrf_group', q); ctx.set_option('group_inner', qi)
      for m, big in ((1, False), (5, False), (5, True)):
        case = spd_case(n, m, big)
        chol, inv, x = spd_solve(ctx, case)
        tag = '%s n=%d la=%d q=%d qi=%d m=%d big=%d' % (form, n, la, q, qi, m, big)
        for name, got, want in (('chol', chol, case['L']), ('inv', inv, case['Kinv']), ('x', x, case['x'])):
          bad = int((got.astype(np.float64) != want).sum())
          if bad:
            print('%s %s: unequal %d, max |diff| %.3e' % (tag, name, bad, np.nanmax(np.abs(got.astype(np.float64) - want))))
        assert np.array_equal(chol.astype(np.float64), case['L'].astype(np.float64)), tag
        assert np.array_equal(inv.astype(np.float64), case['Kinv'].astype(np.float64)), tag
        assert np.array_equal(x.astype(np.float64), case['x'].astype(np.float64)), tag
        # the form really ran
        assert ctx.get_option('chol_form') == want_chol_form and ctx.get_option('inv_forms') == want_inv_forms, tag
        stages = ctx.profile_get()
        # (the panels are split for a trailing update only: a group that ends before the last panel)
        assert 'trtri_gemm' in stages and 'lauum' in stages and ('split3' in stages) == (form != 'mfma' and q < nblk), (tag, sorted(stages))
  finally:
    ctx.profile_enable(0)
    ctx.set_option('spd_diag_bound', 0); ctx.set_option('trtri3_min_s', 8); ctx.set_option('group_inner', -1)
    for k, v in saved.items():
      ctx.set_option(k, v)


def test_spd_solve_default_stays_on_bf16x3(gpu_ctx):
  """without the hook hbo_spd_solve knows no diagonal bound: bf16x3, whatever chol_f16x2 says"""
  case = spd_case(so.TILE * 2 - 37, 1, False)
  chol, inv, x = spd_solve(gpu_ctx, case)
  assert gpu_ctx.get_option('chol_form') == 1
  assert np.array_equal(chol.astype(np.float64), case['L'].astype(np.float64)) and np.array_equal(inv.astype(np.float64), case['Kinv'].astype(np.float64))
