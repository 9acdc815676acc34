"""hbo_predict(..., full_cov=1) beyond one tile of queries: the V output of GEMM_POST (plain and resident grid), GEMM_VTV over a grid of
tiles and more than two K blocks, the multi-tile M x M Gram with the candidates' padded leading dimension, the pitched copy out, fp32
full covariance, the prior branch, the refusal and NaN paths, workspace reuse and the Python layer -- against tests/full_cov_oracle.py
(the fp64 oracle on the same, for fp32 cases fp32-rounded, inputs), whose own standing tests/test_full_cov_host.py establishes on the
CPU.  Every failure message names the worst 128-tile.  Run with `-m gpu`.

Bounds: full_cov_oracle.FP64_COV_TOL and friends are the suite's existing ones; the two fp32 covariance bounds are 10 x the worst
device error measured on the MI355X over the case list (profiles/full_cov_errors.md).  diag(cov) against the
non-full variance: rtol 1e-8 / atol 1e-12 in fp64 (tests/test_gpu_parity.py); in fp32, whose unit roundoff is 6e-8 and whose
non-full call runs another product form, the sum of the two bounds that each side is held to against the oracle.

With HBO_FULL_COV_LOG=<file> every check appends its figures (device error, the reference's two-route gap, the NumPy-fp32
yardstick, the worst tile) before it asserts."""
import copy
import ctypes as C
import os
import types

import numpy as np
import pytest

import full_cov_oracle as F
import helpers
from oracle import hyperbo_oracle as o

pytestmark = pytest.mark.gpu
WFO = o.DEFAULT_WARP_FUNC
FP32_VAR_TOL = 5e-4      # the suite's bound for the fp32 non-full variance, relative to max |var|
PARITY_CASES = [f for f in F.FAMILIES if not f[3]]   # tests/test_gpu_parity.py CASES


def _native():
  from hyperbo_amd import _model, _native as nat
  from hyperbo_amd.basics import definitions as defs, linalg
  from hyperbo_amd.gp_utils import gp, kernel, mean, utils
  return nat, _model, defs, linalg, gp, kernel, mean, utils


def _funcs(case):
  _, _, _, _, _, kernel, mean, _ = _native()
  return getattr(mean, case.mname), getattr(kernel, case.kernel_name)


def _params(model):
  defs = _native()[2]
  return defs.GPParams(model=copy.deepcopy(model), config={'mlp_features': helpers.MLP_FEATURES})


def _log(line):
  path = os.environ.get('HBO_FULL_COV_LOG')
  if path:
    with open(path, 'a') as f:
      f.write(line + '\n')


@pytest.fixture(scope='module')
def direct_ctx(gpu_ctx):
  """A second context whose fp32 Gram matrices always take the direct form (as tests/test_gpu_conditioning.py: direct_ctx)."""
  nat = _native()[0]
  ctx = nat.Context(gpu_ctx.device)
  ctx.set_option('poison', 1)
  ctx.set_option('gram_mfma', 0)
  yield ctx
  ctx.close()


def _cus(ctx):
  nat = _native()[0]
  cus, mem = C.c_int32(0), C.c_int64(0)
  assert nat.lib().hbo_device_info(ctx.device, None, 0, C.byref(cus), C.byref(mem)) == 0 and cus.value > 0
  return cus.value


def _c_predict(ctx, mn, kn, pn, handle, xq, full_cov, mu=None, cov=None):
  """The C entry point itself on `ctx`: (status, mu, cov)."""
  nat, _model, _, _, _, _, _, utils = _native()
  m, d = xq.shape
  bm = _model.BuiltModel(mn, kn, pn, utils.DEFAULT_WARP_FUNC, xq.dtype, d)
  mu = np.empty((m, 1), xq.dtype) if mu is None else mu
  cov = np.empty((m, m) if full_cov else (m, 1), xq.dtype) if cov is None else cov
  rc = nat.lib().hbo_predict(ctx.handle, bm.ref(), handle.handle if handle is not None else None, nat.ptr(xq), m, int(full_cov),
                             nat.ptr(mu), nat.ptr(cov))
  return rc, mu, cov


def _check_cov(case, cov, ref, label, gram_form='default', idx=None):
  """cov (whole, or its rows / columns idx) against ref.cov within the case's bound, the figures logged first."""
  tol, scale_name = F.cov_bound(case, gram_form)
  scale = float(np.max(np.abs(ref.cov if scale_name == 'cov' else ref.kqq)))
  assert cov.dtype == case.np_dtype
  got = cov if idx is None else cov[np.ix_(idx, idx)]
  assert got.shape == ref.cov.shape, (got.shape, ref.cov.shape)
  if idx is None:
    err, tile = F.worst_tile(got, ref.cov)
  else:   # every tile of the whole grid holds RESIDENT_PER_TILE of the subset's queries
    diff = np.abs(got.astype(np.float64) - ref.cov)
    diff = np.where(np.isfinite(diff), diff, np.inf)
    i, j = np.unravel_index(int(np.argmax(diff)), diff.shape)
    err, tile = float(diff[i, j]), (int(idx[i]) // F.TILE, int(idx[j]) // F.TILE)
  kq = float(np.max(np.abs(ref.kqq)))
  sym = float(np.max(np.abs(cov.astype(np.float64) - cov.T.astype(np.float64))))
  ok = bool(np.isfinite(err) and err <= tol * scale)
  msg = ''
  if not ok or os.environ.get('HBO_FULL_COV_LOG'):   # (the two figures beside the device's cost a second at n = 4096)
    gap = float(np.max(np.abs(F.second_route(case, idx) - ref.cov)) / np.max(np.abs(ref.cov)))
    yard = float(np.max(np.abs(F.fp32_yardstick(case, idx) - ref.cov)) / kq)
    _log(f'cov | {case.id} | {gram_form} | {label} | dev/kqq {err / kq:.3e} | dev/cov {err / np.max(np.abs(ref.cov)):.3e} | gap {gap:.1e} | '
         f'yard/kqq {yard:.3e} | tile {tile} | sym/scale {sym / scale:.3e}')
    msg = (f'{case.id} {label}: max |cov - ref| {err:.3e} = {err / scale:.3e} of max |{scale_name}| {scale:.3e} (bound {tol:g}), worst '
           f'128-tile {tile}; NumPy-fp32 yardstick {yard:.3e} of max |Kqq|, two-route gap {gap:.1e}')
  assert ok, msg
  _, stile = F.worst_tile(cov, cov.T)
  assert sym <= tol * scale, f'{case.id} {label}: |cov - cov^T| {sym:.3e} > {tol:g} * {scale:.3e}, worst 128-tile {stile}'
  return err / scale


def _check_mu(case, mu, ref_mu, label):
  mu = np.asarray(mu, dtype=np.float64)
  assert mu.shape == ref_mu.shape
  if case.dtype == 'fp64':
    assert helpers.rel_err(mu, ref_mu) < F.FP64_MU_TOL, (case.id, label, helpers.rel_err(mu, ref_mu))
  else:
    err = float(np.max(np.abs(mu - ref_mu)))
    assert err <= F.FP32_MU_TOL * max(float(np.max(np.abs(ref_mu))), 1.0), (case.id, label, err)


def _check_diag(case, cov, var, ref, label, gram_form='default'):
  """diag(cov) against the non-full variance of the same cache."""
  d, v = np.diag(cov).astype(np.float64), var[:, 0].astype(np.float64)
  gap = float(np.max(np.abs(d - v)))
  _log(f'diag | {case.id} | {gram_form} | {label} | max |diag - var| {gap:.3e} | of kqq {gap / np.max(np.abs(ref.kqq)):.3e}')
  if case.dtype == 'fp64':
    np.testing.assert_allclose(d, v, rtol=1e-8, atol=1e-12, err_msg=f'{case.id} {label}')
  else:
    bound = F.cov_bound(case, gram_form)[0] * float(np.max(np.abs(ref.kqq))) + FP32_VAR_TOL * float(np.max(np.abs(np.diag(ref.cov))))
    assert gap <= bound, f'{case.id} {label}: max |diag(cov) - var| {gap:.3e} > {bound:.3e}, query {int(np.argmax(np.abs(d - v)))}'


def _full_and_checks(case, ctx, label, gram_form='default'):
  """Factor on ctx, gp.predict(full_cov=True) twice and the non-full call on the same cache; all of (a)'s assertions."""
  _, _, _, linalg, gp, _, _, utils = _native()
  wf = utils.DEFAULT_WARP_FUNC
  model, x, y, xq = F.inputs(case)
  mn, kn = _funcs(case)
  pn = _params(model)
  ref = F.reference(case)
  h = linalg.factor(mn, kn, pn, x, y, wf, ctx=ctx)
  try:
    cache = types.SimpleNamespace(handle=h)
    mu, cov = gp.predict(mn, kn, pn, x, y, xq, wf, full_cov=True, cache=cache)
    mu2, cov2 = gp.predict(mn, kn, pn, x, y, xq, wf, full_cov=True, cache=cache)
    _, var = gp.predict(mn, kn, pn, x, y, xq, wf, cache=cache)
  finally:
    h.close()
  assert mu.shape == (case.M, 1) and cov.shape == (case.M, case.M) and var.shape == (case.M, 1)
  rel = _check_cov(case, cov, ref, label, gram_form)
  _check_mu(case, mu, ref.mu, label)
  _check_diag(case, cov, var, ref, label, gram_form)
  assert np.array_equal(cov, cov2) and np.array_equal(mu, mu2), f'{case.id} {label}: two identical calls differ'
  return rel


# ---- a. tile and block edges, with a cache ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', F.EDGE_CASES, ids=lambda c: c.id)
def test_tile_and_block_edges(gpu_ctx, case):
  """(n, M) on both sides of the 128-tile and 128-block edges, five model families, both dtypes, through gp.predict(full_cov=True)."""
  _full_and_checks(case, gpu_ctx, 'edges')


# ---- b. prior branch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', F.DTYPES)
@pytest.mark.parametrize('M', [1, 128, 129, 300])
@pytest.mark.parametrize('kname,mlp,mname,_kumar', PARITY_CASES)
def test_prior_branch(gpu_ctx, kname, mlp, mname, _kumar, M, dtype):
  """No observations: the answer is the M x M Gram of the queries, dense (ldo = M), and the prior mean."""
  _, _, _, _, gp, kernel, mean, utils = _native()
  dt = np.float64 if dtype == 'fp64' else np.float32
  rng = np.random.default_rng([F.FAMILIES.index((kname, mlp, mname, False)), M, 3])
  model = F.cast(helpers.make_model(rng, mname, mlp, 3), dt)
  xq = rng.uniform(size=(M, 3)).astype(dt)
  po = o.GPParams(model=F.cast(model, np.float64), config={'mlp_features': helpers.MLP_FEATURES})
  suffix = '_mlp' if mlp else ''
  mu_o, k_o = o.predict(getattr(o, mname), getattr(o, kname + suffix), po, None, None, xq.astype(np.float64), WFO, full_cov=True)
  mu, cov = gp.predict(getattr(mean, mname), getattr(kernel, kname + suffix), _params(model), None, None, xq, utils.DEFAULT_WARP_FUNC,
                       full_cov=True)
  assert cov.shape == (M, M) and cov.dtype == dt and mu.shape == (M, 1)
  err, tile = F.worst_tile(cov, k_o)
  tol = 1e-13 if dtype == 'fp64' else 2e-5   # test_gram_vs_oracle, test_fp32_gram_on_the_matrix_cores_vs_oracle
  scale = float(np.max(np.abs(k_o)))
  _log(f'prior | {kname}{suffix}+{mname} M={M} {dtype} | err/max|K| {err / scale:.3e} | tile {tile}')
  assert err <= tol * scale, f'prior Gram: {err:.3e} = {err / scale:.3e} of max |K| (bound {tol:g}), worst 128-tile {tile}'
  assert np.array_equal(cov, cov.T)
  if dtype == 'fp64':
    assert helpers.rel_err(mu, mu_o) < 1e-12 or np.max(np.abs(mu_o)) == 0.0
  else:
    assert np.max(np.abs(mu - mu_o)) <= F.FP32_MU_TOL * max(float(np.max(np.abs(mu_o))), 1.0)


def test_prior_branch_fp32_wide_on_both_gram_forms(gpu_ctx, direct_ctx):
  """d = 64, M = 300, fp32: the prior's Gram with x1 = x2 on the matrix cores (default context) and in the direct form."""
  _, _, _, _, _, kernel, mean, _ = _native()
  case = F.WIDE_CASES[0]
  model, _, _, xq = F.inputs(case)
  k_o = F.reference(case).kqq
  scale = float(np.max(np.abs(k_o)))
  for form, ctx in (('mfma', gpu_ctx), ('direct', direct_ctx)):
    rc, mu, cov = _c_predict(ctx, mean.constant, getattr(kernel, case.kernel_name), _params(model), None, xq, True)
    assert rc == 0
    err, tile = F.worst_tile(cov, k_o)
    _log(f'prior | wide {case.kernel_name} M={case.M} fp32 {form} | err/max|K| {err / scale:.3e} | tile {tile}')
    assert err <= 2e-5 * scale, f'prior Gram ({form}): {err / scale:.3e} of max |K| (bound 2e-5), worst 128-tile {tile}'
    assert np.array_equal(cov, cov.T), form
    assert np.max(np.abs(mu - F.oracle_funcs(case)[0](F.oracle_params(case), xq.astype(np.float64), warp_func=WFO))) <= F.FP32_MU_TOL


# ---- c. fp32 with >= 32 features and a cache -------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['mfma', 'direct'])
@pytest.mark.parametrize('case', F.WIDE_CASES, ids=lambda c: c.id)
def test_fp32_wide_features_with_a_cache(gpu_ctx, direct_ctx, case, form):
  """n = M = 300, d = 64: the cache's Gram, the cross Gram and Kqq on the matrix cores (their absolute error amplified through K^-1:
  a bound of its own) and in the direct form (the bound of the edge cases)."""
  _full_and_checks(case, gpu_ctx if form == 'mfma' else direct_ctx, 'wide', 'default' if form == 'mfma' else 'direct')


# ---- d. the resident-grid product writing V --------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', F.DTYPES)
def test_resident_grid_product_writing_v(gpu_ctx, dtype):
  """32 row blocks; M just above (M / 128) * 32 = 4 * CUs, where GEMM_POST runs as a resident grid drawing its tiles from a counter and
  writes V from it, and M at the threshold (plain grid) on the same cache.  Four queries of every 128-tile against the oracle (the
  reference of a subset of the queries is the sub-matrix of the whole one: test_full_cov_host.py), so that each of the (M / 128)^2
  tiles contributes 16 entries; symmetry, diag against the non-full variance and repeat-call identity on the whole output."""
  _, _, _, linalg, gp, _, _, utils = _native()
  wf = utils.DEFAULT_WARP_FUNC
  m_res, m_plain = F.resident_sizes(_cus(gpu_ctx))
  case = F.resident_case(dtype, _cus(gpu_ctx))
  assert case.M == m_res
  model, x, y, xq = F.inputs(case)
  mn, kn = _funcs(case)
  pn = _params(model)
  idx = F.resident_subset(m_res)
  ref = F.reference(case, idx)
  h = linalg.factor(mn, kn, pn, x, y, wf)
  try:
    cache = types.SimpleNamespace(handle=h)
    mu, cov = gp.predict(mn, kn, pn, x, y, xq, wf, full_cov=True, cache=cache)
    grid1 = gpu_ctx.get_option('post_resident')
    mu2, cov2 = gp.predict(mn, kn, pn, x, y, xq, wf, full_cov=True, cache=cache)
    same = np.array_equal(cov, cov2) and np.array_equal(mu, mu2)
    del cov2
    _, var = gp.predict(mn, kn, pn, x, y, xq, wf, cache=cache)
    mu0, cov0 = gp.predict(mn, kn, pn, x, y, xq[:m_plain], wf, full_cov=True, cache=cache)
    grid0 = gpu_ctx.get_option('post_resident')
  finally:
    h.close()
  _log(f'grid | {case.id} | M={m_res}: post_resident {grid1} | M={m_plain}: post_resident {grid0}')
  assert grid1 == 1 and grid0 == 0, (grid1, grid0)
  _check_cov(case, cov, ref, 'resident', idx=idx)
  _check_mu(case, mu[idx], ref.mu, 'resident')
  tol, scale_name = F.cov_bound(case)
  scale = float(np.max(np.abs(ref.cov if scale_name == 'cov' else ref.kqq)))
  d, v = np.diag(cov).astype(np.float64), var[:, 0].astype(np.float64)
  gap = float(np.max(np.abs(d - v)))
  _log(f'diag | {case.id} | default | resident | max |diag - var| {gap:.3e} | of kqq {gap / np.max(np.abs(ref.kqq)):.3e}')
  if dtype == 'fp64':
    np.testing.assert_allclose(d, v, rtol=1e-8, atol=1e-12)
  else:
    assert gap <= tol * scale + FP32_VAR_TOL * float(np.max(np.abs(np.diag(ref.cov)))), gap
  assert same, 'two identical calls differ'
  # the plain grid at the threshold, on the queries both calls share
  i0 = idx[idx < m_plain]
  sub1, sub0 = cov[np.ix_(i0, i0)].astype(np.float64), cov0[np.ix_(i0, i0)].astype(np.float64)
  diff = np.abs(sub1 - sub0)
  i, j = np.unravel_index(int(np.argmax(diff)), diff.shape)
  tile = (int(i0[i]) // F.TILE, int(i0[j]) // F.TILE)
  cmax = float(np.max(np.abs(ref.cov)))
  _log(f'grids | {case.id} | max |resident - plain| {diff[i, j]:.3e} | of max|cov| {diff[i, j] / cmax:.3e} | of kqq {diff[i, j] / np.max(np.abs(ref.kqq)):.3e} | tile {tile}')
  bound = 1e-12 * cmax if dtype == 'fp64' else tol * scale
  assert diff[i, j] <= bound, f'resident against plain grid: {diff[i, j]:.3e} > {bound:.3e}, worst 128-tile {tile}'
  _check_mu(case, mu0[i0], ref.mu[idx < m_plain], 'plain')


# ---- e. workspace reuse ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', F.DTYPES)
def test_pooled_workspaces_across_calls_of_different_m(gpu_ctx, dtype):
  """WS_V / WS_KQQ / WS_COV are pooled per context and sized by the largest call so far: M = 300, 70, 129, 300 on one cache, a non-full
  predict and an acquisition between them, each bit for bit what the same call gives as the first one on a fresh cache (made on a
  context of its own, whose workspaces nothing has used, in ascending M so that every call gets new buffers)."""
  nat, _model, _, linalg, gp, kernel, mean, utils = _native()
  wf = utils.DEFAULT_WARP_FUNC
  case = F.Case('edge', 'matern52', True, 'linear_mlp', False, 300, 300, 3, dtype)
  model, x, y, xq = F.inputs(case)
  mn, kn = _funcs(case)
  pn = _params(model)
  fresh = {}
  ctx2 = nat.Context(gpu_ctx.device)
  try:
    ctx2.set_option('poison', 1)
    for m in (70, 129, 300):
      h = linalg.factor(mn, kn, pn, x, y, wf, ctx=ctx2)
      try:
        rc, mu, cov = _c_predict(ctx2, mn, kn, pn, h, xq[:m], True)
        assert rc == 0
        fresh[m] = (mu, cov)
      finally:
        h.close()
  finally:
    ctx2.close()
  h = linalg.factor(mn, kn, pn, x, y, wf)
  try:
    cache = types.SimpleNamespace(handle=h)
    bm = _model.BuiltModel(mn, kn, pn, wf, xq.dtype, case.d)
    for step, m in enumerate((300, 70, 129, 300)):
      mu, cov = gp.predict(mn, kn, pn, x, y, xq[:m], wf, full_cov=True, cache=cache)
      assert np.array_equal(mu, fresh[m][0]) and np.array_equal(cov, fresh[m][1]), (
          f'call {step} (M = {m}) differs from the first call on a fresh cache: worst 128-tile {F.worst_tile(cov, fresh[m][1])}')
      gp.predict(mn, kn, pn, x, y, xq[:200], wf, cache=cache)
      out = np.empty((150, 1), xq.dtype)
      assert nat.lib().hbo_acq(gpu_ctx.handle, bm.ref(), h.handle, nat.ptr(xq[:150]), 150, 0, float(np.max(y)), 0.1, 1.0, nat.ptr(out)) == 0
  finally:
    h.close()


# ---- f. after a row append -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kname,mlp,mname,_kumar', PARITY_CASES)
def test_full_cov_after_a_row_append(gpu_ctx, kname, mlp, mname, _kumar):
  """120 observations + 4 appended in place (one block): full_cov at M = 129 against the oracle on the 124 points, at the bound of
  test_incremental_cache_append_matches_refactorisation."""
  _, _, defs, _, gp, kernel, mean, utils = _native()
  case = F.Case('edge', kname, mlp, mname, False, 124, 129, 3, 'fp64')
  model, x, y, xq = F.inputs(case)
  mn, kn = _funcs(case)
  m = gp.GP({0: defs.SubDataset(x[:120], y[:120])}, mn, kn, _params(model), utils.DEFAULT_WARP_FUNC)
  m.predict(xq, 0)
  h0 = m.params.cache[0].handle
  m.update_sub_dataset((x[120:], y[120:]), 0, is_append=True)
  mu, cov = m.predict(xq, 0, full_cov=True, with_noise=False, unbiased=False)
  assert m.params.cache[0].handle is h0 and h0.n == 124   # appended in place
  ref = F.reference(case)
  err, tile = F.worst_tile(cov, ref.cov)
  scale = float(np.max(np.abs(ref.cov)))
  _log(f'append | {case.id} | err/max|cov| {err / scale:.3e} | tile {tile}')
  assert err <= 1e-8 * scale, f'{err / scale:.3e} of max |cov| (bound 1e-8), worst 128-tile {tile}'
  assert helpers.rel_err(mu, ref.mu) < 1e-8


# ---- g. status paths -------------------------------------------------------------------------------------------------------------
def test_more_than_65536_queries_are_refused_before_anything_is_written(gpu_ctx):
  nat, _, _, linalg, _, kernel, mean, utils = _native()
  case = F.Case('edge', 'squared_exponential', False, 'constant', False, 5, 129, 3, 'fp64')
  model, x, y, _ = F.inputs(case)
  pn = _params(model)
  m = 65537
  xq = np.random.default_rng(0).uniform(size=(m, 3))
  mu = np.full((m, 1), -7.25)
  sentinel = np.full((1, 1), -7.25)
  h = linalg.factor(mean.constant, kernel.squared_exponential, pn, x, y, utils.DEFAULT_WARP_FUNC)
  try:
    rc, _, _ = _c_predict(gpu_ctx, mean.constant, kernel.squared_exponential, pn, h, xq, True, mu=mu, cov=sentinel)
    assert rc == nat.HBO_ERR_UNSUPPORTED
    assert sentinel[0, 0] == -7.25 and np.all(mu == -7.25)
    assert gpu_ctx.get_option('post_resident') == 0
    rc, _, _ = _c_predict(gpu_ctx, mean.constant, kernel.squared_exponential, pn, None, xq, True, mu=mu, cov=sentinel)   # prior branch
    assert rc == nat.HBO_ERR_UNSUPPORTED and sentinel[0, 0] == -7.25 and np.all(mu == -7.25)
    rc, mu_ok, cov_ok = _c_predict(gpu_ctx, mean.constant, kernel.squared_exponential, pn, h, xq[:3], True)   # the context still works
    assert rc == 0 and np.isfinite(cov_ok).all()
  finally:
    h.close()


def test_cache_that_is_not_positive_definite_gives_nan_covariance(gpu_ctx):
  """A NaN input row: the suite's deterministic HBO_NOT_PD.  The C entry point reports it and fills mu and all M x M entries with NaN;
  gp.predict returns the NaN arrays and raises nothing."""
  nat, _, _, linalg, gp, kernel, mean, utils = _native()
  wf = utils.DEFAULT_WARP_FUNC
  case = F.Case('edge', 'squared_exponential', False, 'constant', False, 129, 129, 3, 'fp64')
  for dt in (np.float64, np.float32):
    model, x, y, xq = (F.cast(t, dt) if isinstance(t, dict) else t.astype(dt) for t in F.inputs(case))
    x = x.copy(); x[77, 1] = np.nan
    pn = _params(model)
    h = linalg.factor(mean.constant, kernel.squared_exponential, pn, x, y, wf)
    try:
      assert h.status == nat.HBO_NOT_PD
      mu = np.zeros((129, 1), dt); cov = np.zeros((129, 129), dt)
      rc, _, _ = _c_predict(gpu_ctx, mean.constant, kernel.squared_exponential, pn, h, xq, True, mu=mu, cov=cov)
      assert rc == nat.HBO_NOT_PD
      assert np.isnan(mu).all() and np.isnan(cov).all(), (int(np.isnan(cov).sum()), cov.size)
    finally:
      h.close()
    mu, cov = gp.predict(mean.constant, kernel.squared_exponential, pn, x, y, xq, wf, full_cov=True)
    assert mu.shape == (129, 1) and cov.shape == (129, 129) and np.isnan(mu).all() and np.isnan(cov).all()


# ---- h. Python layer -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('unbiased', [False, True])
@pytest.mark.parametrize('with_noise', [False, True])
def test_gp_predict_full_cov_noise_and_scale(gpu_ctx, with_noise, unbiased):
  """GP.predict(full_cov=True): the noise goes on the diagonal only, T / (T - 1) (three sub-datasets) on the whole matrix."""
  _, _, defs, _, gp, _, _, utils = _native()
  case = F.Case('edge', 'matern32', False, 'linear', False, 257, 129, 3, 'fp64')
  model, x, y, xq = F.inputs(case)
  mn, kn = _funcs(case)
  ds = {0: defs.SubDataset(x, y), 1: defs.SubDataset(x[:50], y[:50]), 'c': defs.SubDataset(x[50:90], y[50:90])}
  m = gp.GP(ds, mn, kn, _params(model), utils.DEFAULT_WARP_FUNC)
  mu, cov = m.predict(xq, 0, full_cov=True, with_noise=with_noise, unbiased=unbiased)
  ref = F.reference(case)
  dso = {k: o.SubDataset(v.x, v.y) for k, v in ds.items()}
  mu_o, cov_o = o.gp_predict_postprocess(F.oracle_params(case), dso, ref.mu, ref.cov, WFO, True, with_noise, unbiased)
  assert cov.shape == (129, 129)
  err, tile = F.worst_tile(cov, cov_o)
  assert err <= 1e-9 * np.max(np.abs(cov_o)), f'{err:.3e}, worst 128-tile {tile}'
  assert helpers.rel_err(mu, mu_o) < 1e-9
  off = ~np.eye(129, dtype=bool)
  scale = 1.5 if unbiased else 1.0
  np.testing.assert_allclose(cov[off], scale * ref.cov[off], rtol=0, atol=1e-9 * np.max(np.abs(cov_o)))   # no noise off the diagonal


def test_hgp_predict_full_cov_returns_one_result_per_sample(gpu_ctx):
  _, _, defs, _, gp, _, _, utils = _native()
  base = F.Case('edge', 'matern52', True, 'linear_mlp', False, 129, 257, 3, 'fp64')
  model, x, y, xq = F.inputs(base)
  mn, kn = _funcs(base)
  mo, ko = F.oracle_funcs(base)
  rng = np.random.default_rng(5)
  samples = []
  for s in range(3):
    ms = copy.deepcopy(model)
    ms['lengthscale'] = model['lengthscale'] * (1.0 + 0.2 * s)
    ms['signal_variance'] = model['signal_variance'] + 0.3 * s
    ms['noise_variance'] = model['noise_variance'] + 0.2 * rng.normal()
    samples.append(ms)
  pn = _params(model)
  pn.samples = copy.deepcopy(samples)
  ds = {0: defs.SubDataset(x, y), 1: defs.SubDataset(x[:60], y[:60]), 2: defs.SubDataset(x[60:], y[60:])}
  dso = {k: o.SubDataset(v.x, v.y) for k, v in ds.items()}
  out = gp.HGP(ds, mn, kn, pn, utils.DEFAULT_WARP_FUNC).predict(xq, 0, full_cov=True)
  assert isinstance(out, list) and len(out) == 3
  for s, (mu, cov) in enumerate(out):
    po = o.GPParams(model=samples[s], config={'mlp_features': helpers.MLP_FEATURES})
    mu_o, cov_o = o.predict(mo, ko, po, x, y, xq, WFO, full_cov=True)
    mu_o, cov_o = o.gp_predict_postprocess(po, dso, mu_o, cov_o, WFO, True, True, True)
    assert cov.shape == (257, 257)
    err, tile = F.worst_tile(cov, cov_o)
    assert err <= 1e-9 * np.max(np.abs(cov_o)), f'sample {s}: {err:.3e}, worst 128-tile {tile}'
    assert helpers.rel_err(mu, mu_o) < 1e-9
