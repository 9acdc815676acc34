"""GPU tier: the fp64 Jacobi eigensolver (hbo_sym_eig), the spectral NLL (hbo_nll_spectral) and the 'spectral' routing of the
reference's SVD call sites.  Every bound is the a-priori one; the measured worst cases are in profiles/spectral.md."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla

import helpers

EPS = np.finfo(np.float64).eps
pytestmark = pytest.mark.gpu


def _native():
  from hyperbo_amd import _native as nat
  from hyperbo_amd.basics import definitions as defs, linalg
  from hyperbo_amd.gp_utils import gp, kernel, mean, objectives, utils
  return nat, defs, linalg, gp, kernel, mean, objectives, utils


@contextlib.contextmanager
def _spectral(ctx, value=1):
  prev = ctx.get_option('spectral')
  ctx.set_option('spectral', value)
  try:
    yield
  finally:
    ctx.set_option('spectral', prev)


def _sym_eig(ctx, a, vectors=True):
  nat = _native()[0]
  a = np.ascontiguousarray(a)
  count, n = a.shape[0], a.shape[-1]
  w = np.empty((count, n))
  v = np.empty((count, n, n)) if vectors else None
  rc = nat.lib().hbo_sym_eig(ctx.handle, nat.dtype_code(a.dtype), nat.ptr(a), n, count, nat.ptr(w), nat.ptr(v))
  return rc, w, v


def _gram(kind, x, ls=0.3, noise=1e-8):
  d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
  r = np.sqrt(d2) / ls
  if kind == 'se':
    k = np.exp(-0.5 * r ** 2)
  elif kind == 'm32':
    k = (1 + np.sqrt(3) * r) * np.exp(-np.sqrt(3) * r)
  else:
    k = (1 + np.sqrt(5) * r + 5 / 3 * r ** 2) * np.exp(-np.sqrt(5) * r)
  return k + noise * np.eye(len(x))


def _family(name, n, rng):
  if name == 'gauss':
    g = rng.normal(size=(n, n))
    return (g + g.T) / 2
  if name in ('se', 'm32', 'm52'):
    return _gram(name, rng.uniform(size=(n, 3)))
  if name == 'repeated':
    x = rng.uniform(size=(max(1, n // 4), 3))
    return _gram('se', np.repeat(x, 4, axis=0)[:n], noise=0.0) if n >= 4 else _gram('se', rng.uniform(size=(n, 3)))
  if name == 'lowrank':
    x = rng.normal(size=(n, 3))
    return x @ x.T
  if name == 'diag':
    return np.diag(rng.normal(size=n))
  if name == 'zero':
    return np.zeros((n, n))
  if name in ('big', 'tiny'):
    g = rng.normal(size=(n, n))
    return (g + g.T) * (1e150 if name == 'big' else 1e-150)
  raise ValueError(name)


def _check_eig(a, w, v, tag=''):
  n = a.shape[0]
  na = np.linalg.norm(a)
  assert np.all(np.diff(w) >= 0), tag
  assert np.linalg.norm(a @ v - v * w[None, :]) <= 4 * n * EPS * na, tag
  assert np.linalg.norm(v.T @ v - np.eye(n)) <= 4 * n * EPS, tag
  ref = sla.eigh(a, eigvals_only=True)
  assert np.max(np.abs(w - ref)) <= 4 * n * EPS * np.linalg.norm(a, 2), tag


SIZES = [1, 2, 3, 17, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 513, 1000, 2048]
FAMILIES = ['gauss', 'se', 'm32', 'm52', 'repeated', 'lowrank', 'diag', 'zero', 'big', 'tiny']


def _eig_cases():
  for family in FAMILIES:
    for n in SIZES:
      if family in ('big', 'tiny') and n > 200:
        continue
      yield family, n


@pytest.mark.parametrize('family,n', list(_eig_cases()))
def test_sym_eig(gpu_ctx, family, n):
  rng = np.random.default_rng(1000 * n + FAMILIES.index(family))
  count = 3 if n <= 513 else 1
  a = np.stack([_family(family, n, rng) for _ in range(count)])
  a_lower_only = np.tril(a) + np.triu(np.full_like(a, np.nan), 1)   # only the lower triangle may be read
  rc, w, v = _sym_eig(gpu_ctx, a_lower_only)
  assert rc == 0, rc
  for t in range(count):
    _check_eig(a[t], w[t], v[t], f'{family} n={n} t={t}')
  rc2, w2, _ = _sym_eig(gpu_ctx, a_lower_only, vectors=False)
  assert rc2 == 0 and np.array_equal(w, w2)                        # w does not depend on v_out
  rc3, w3, v3 = _sym_eig(gpu_ctx, a_lower_only)
  assert rc3 == 0 and np.array_equal(w, w3) and np.array_equal(v, v3)   # identical calls, identical bits


def test_sym_eig_fp32_input_is_promoted(gpu_ctx):
  rng = np.random.default_rng(5)
  a = _family('se', 150, rng).astype(np.float32)[None]
  rc, w, v = _sym_eig(gpu_ctx, a)
  assert rc == 0
  _check_eig(a[0].astype(np.float64), w[0], v[0])


def test_sym_eig_cfg2_size(gpu_ctx):
  """n = 8192 SE Gram (cfg 2's shape): residual and orthogonality; the eigenvalues against LAPACK at n = 4096."""
  rng = np.random.default_rng(8192)
  x = rng.uniform(size=(8192, 4))
  a = _gram('se', x, ls=0.5, noise=1e-3)
  rc, w, v = _sym_eig(gpu_ctx, a[None])
  assert rc == 0
  n, na = 8192, np.linalg.norm(a)
  assert np.all(np.diff(w[0]) >= 0)
  assert np.linalg.norm(a @ v[0] - v[0] * w[0][None, :]) <= 4 * n * EPS * na
  assert np.linalg.norm(v[0].T @ v[0] - np.eye(n)) <= 4 * n * EPS
  del v
  b = a[:4096, :4096]
  rc, wb, _ = _sym_eig(gpu_ctx, b[None], vectors=False)
  assert rc == 0
  assert np.max(np.abs(wb[0] - sla.eigh(b, eigvals_only=True))) <= 4 * 4096 * EPS * np.linalg.norm(b, 2)


# ---- the spectral NLL against the host SVD path --------------------------------------------------------------------------
def _host_terms(linalg, mean_func, cov_func, params, wf, x, y):
  vy, cov = linalg.compute_delta_y_and_cov(mean_func, cov_func, params, x, y, warp_func=wf)
  return np.asarray(vy, dtype=np.float64), np.asarray(cov, dtype=np.float64)


def _nll_bound(cov, vy, m):
  """|dNLL| <= 2 * 4 n eps |K|_2 * m^2 * (sum 1/|lambda| + |K^-1 y~|^2) (two backward-stable decompositions, first order)."""
  n = cov.shape[0]
  lam = np.linalg.eigvalsh(cov)
  yt = vy.sum(axis=1)
  kinv_y = np.linalg.solve(cov, yt)
  return 2 * 4 * n * EPS * np.max(np.abs(lam)) * m * m * (np.sum(1 / np.abs(lam)) + kinv_y @ kinv_y)


COVS = ['squared_exponential', 'matern32', 'matern52', 'dot_product']


def _spectral_case(gpu_ctx, rng, cov_name, mean_name, mlp, dtype, m, sizes, kumar=False):
  nat, defs, linalg, gp, kernel, mean, objectives, utils = _native()
  d = 3
  model = helpers.make_model(rng, mean_name, mlp, d)
  if kumar:
    model['kumar_params'] = {'a': rng.uniform(-1, 1, size=d), 'b': rng.uniform(-1, 1, size=d)}
    cov_name = cov_name + '_kumar'
  params = defs.GPParams(model=model, config={'mlp_features': helpers.MLP_FEATURES})
  mean_func = getattr(mean, mean_name)
  cov_func = getattr(kernel, cov_name + ('_mlp' if mlp else ''))
  wf = utils.DEFAULT_WARP_FUNC
  ds = {}
  for i, n in enumerate(sizes):
    x, y = helpers.synthetic_task(rng, n, d, m=m, dtype=dtype)
    ds[f't{i}'] = defs.SubDataset(x, y)
  v0, k0 = objectives.neg_log_marginal_likelihood(mean_func, cov_func, params, ds, wf, return_key2nll=True, use_cholesky=False)
  with _spectral(gpu_ctx):
    v1, k1 = objectives.neg_log_marginal_likelihood(mean_func, cov_func, params, ds, wf, return_key2nll=True, use_cholesky=False)
  worst = 0.0
  for key, s in ds.items():
    vy, cov = _host_terms(linalg, mean_func, cov_func, params, wf, s.x, s.y)
    bound = _nll_bound(cov, vy, m)
    if dtype == np.float32 and m > 1:
      # the device carries y~ = sum_a y_a - m mu from the dataset's fp32 column sums; the host sums fp32 (y_a - mu): that input
      # difference enters exactly (it is not a decomposition error)
      mu = np.asarray(mean_func(params, s.x, warp_func=wf), dtype=np.float64).reshape(-1)
      yt_dev = np.float32(np.asarray(s.y, dtype=np.float64).sum(axis=1)).astype(np.float64) - m * mu
      yt_host = vy.sum(axis=1)
      bound += 0.5 * abs(yt_dev @ np.linalg.solve(cov, yt_dev) - yt_host @ np.linalg.solve(cov, yt_host))
    err = abs(k1[key] - k0[key])
    assert np.isfinite(k1[key]) and err <= bound, (key, k1[key], k0[key], err, bound)
    worst = max(worst, err / bound)
  return worst


@pytest.mark.parametrize('cov_name', COVS)
@pytest.mark.parametrize('mean_name', ['constant', 'linear'])
@pytest.mark.parametrize('mlp', [False, True])
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('m', [1, 3])
def test_nll_spectral_vs_host_svd(gpu_ctx, cov_name, mean_name, mlp, dtype, m):
  rng = np.random.default_rng(hash((cov_name, mean_name, mlp, m, np.dtype(dtype).name)) % 2 ** 32)
  _spectral_case(gpu_ctx, rng, cov_name, mean_name, mlp, dtype, m, [1, 64, 65, 100])


@pytest.mark.parametrize('cov_name', ['squared_exponential', 'matern32', 'matern52', 'dot_product'])
def test_nll_spectral_kumar(gpu_ctx, cov_name):
  rng = np.random.default_rng(77)
  _spectral_case(gpu_ctx, rng, cov_name, 'constant', False, np.float64, 1, [1, 64, 65, 100], kumar=True)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_nll_spectral_batch_24x100_and_one_large_task(gpu_ctx, dtype):
  rng = np.random.default_rng(24)
  _spectral_case(gpu_ctx, rng, 'matern52', 'constant', False, dtype, 1, [100] * 24)
  _spectral_case(gpu_ctx, rng, 'squared_exponential', 'linear', False, dtype, 1, [2048])


def _exact_nll_mp(cov, vy):
  import mpmath
  mpmath.mp.dps = 40
  n = cov.shape[0]
  kk = mpmath.matrix(cov.tolist())
  yt = mpmath.matrix(vy.sum(axis=1).tolist())
  ll = mpmath.cholesky(kk)
  z = mpmath.lu_solve(ll, yt)
  logdet = 2 * mpmath.fsum(mpmath.log(ll[i, i]) for i in range(n))
  m = vy.shape[1]
  val = 0.5 * (mpmath.fsum(z[i] ** 2 for i in range(n)) + m * m * (logdet + n * mpmath.log(2 * mpmath.pi)))
  return float(val)


def test_nll_spectral_ill_conditioned_vs_exact(gpu_ctx):
  nat, defs, linalg, gp, kernel, mean, objectives, utils = _native()
  rng = np.random.default_rng(64)
  x = rng.uniform(size=(64, 2))
  y = np.sin(3 * x[:, :1]) + 0.01 * rng.normal(size=(64, 1))
  model = {'lengthscale': np.array([2.0, 2.0]), 'signal_variance': np.array(1.0), 'noise_variance': np.array(1e-6),
           'constant': np.array(0.0)}
  params = defs.GPParams(model=model)
  ds = {0: defs.SubDataset(x, y)}
  vy, cov = _host_terms(linalg, mean.constant, kernel.squared_exponential, params, None, x, y)
  lam = np.linalg.eigvalsh(cov)
  assert lam.min() < 1e-4 and lam.max() / lam.min() > 1e5
  exact = _exact_nll_mp(cov, vy)
  host = objectives.neg_log_marginal_likelihood(mean.constant, kernel.squared_exponential, params, ds, None, use_cholesky=False)
  with _spectral(gpu_ctx):
    dev = objectives.neg_log_marginal_likelihood(mean.constant, kernel.squared_exponential, params, ds, None, use_cholesky=False)
  assert abs(dev - exact) <= 10 * abs(host - exact) + 1e-12 * abs(exact), (dev, host, exact)


def test_nll_spectral_where_fp32_cholesky_fails(gpu_ctx):
  nat, defs, linalg, gp, kernel, mean, objectives, utils = _native()
  rng = np.random.default_rng(5)
  x = rng.uniform(size=(120, 2)).astype(np.float32)
  y = np.sin(3 * x[:, :1]).astype(np.float32)
  model = {'lengthscale': np.array([3.0, 3.0]), 'signal_variance': np.array(1.0), 'noise_variance': np.array(1e-12),
           'constant': np.array(0.0)}
  params = defs.GPParams(model=model)
  ds = {0: defs.SubDataset(x, y)}
  chol = objectives.neg_log_marginal_likelihood(mean.constant, kernel.squared_exponential, params, ds, None)
  assert np.isnan(chol)
  host = objectives.neg_log_marginal_likelihood(mean.constant, kernel.squared_exponential, params, ds, None, use_cholesky=False)
  with _spectral(gpu_ctx):
    dev = objectives.neg_log_marginal_likelihood(mean.constant, kernel.squared_exponential, params, ds, None, use_cholesky=False)
  vy, cov = _host_terms(linalg, mean.constant, kernel.squared_exponential, params, None, x, y)
  assert np.isfinite(dev) and abs(dev - host) <= _nll_bound(cov, vy, 1), (dev, host)


# ---- Python routing ------------------------------------------------------------------------------------------------------
def test_routing_gp_stats_hgp_stats_and_bit_identity_when_off(gpu_ctx):
  nat, defs, linalg, gp, kernel, mean, objectives, utils = _native()
  rng = np.random.default_rng(6)
  d = 3
  model = helpers.make_model(rng, 'linear', False, d)
  params = defs.GPParams(model=model)
  xa = rng.uniform(size=(20, d))
  ya = np.sin(xa @ rng.normal(size=(d, 30)))   # aligned: more columns than rows, the sample covariance has full rank
  ds = {'a': defs.SubDataset(*helpers.synthetic_task(rng, 70, d)), 'b': defs.SubDataset(*helpers.synthetic_task(rng, 33, d, m=3)),
        'al': defs.SubDataset(xa, ya, aligned=1)}
  wf = utils.DEFAULT_WARP_FUNC
  m0 = gp.GP(ds, mean.linear, kernel.matern32, params, wf)
  nll0, k0 = m0.neg_log_marginal_likelihood()
  st0 = m0.stats(verbose=False)
  with _spectral(gpu_ctx):
    nll1, k1 = m0.neg_log_marginal_likelihood()
    st1 = m0.stats(verbose=False)
  for key, s in ds.items():
    if key in k0:
      vy, cov = _host_terms(linalg, mean.linear, kernel.matern32, params, wf, s.x, s.y)
      assert abs(k1[key] - k0[key]) <= _nll_bound(cov, vy, s.y.shape[1])
  assert abs(nll1 - nll0) <= 1e-9 * abs(nll0)
  assert abs(st1[0] - st0[0]) <= 1e-9 * abs(st0[0])
  for a, b in zip(st1[1:4], st0[1:4]):
    assert abs(a - b) <= 1e-8 * abs(b), (a, b)
  assert set(st1[4]) == set(st0[4])
  # option back at 0: bit-identical to the run before it was touched
  st2 = m0.stats(verbose=False)
  assert st2[:4] == st0[:4] and st2[4] == st0[4]
  # HGP.stats: one value per parameter sample
  samples = [helpers.make_model(np.random.default_rng(100 + i), 'linear', False, d) for i in range(2)]
  h = gp.HGP(ds, mean.linear, kernel.matern32, defs.GPParams(model=samples[0], samples=samples), wf)
  hs0 = h.stats(verbose=False)
  with _spectral(gpu_ctx):
    hs1 = h.stats(verbose=False)
  for a, b in zip(np.ravel(np.asarray(hs1[0], dtype=float)), np.ravel(np.asarray(hs0[0], dtype=float))):
    assert abs(a - b) <= 1e-9 * abs(b)


@pytest.mark.parametrize('n', [5, 64, 100])
def test_routing_svd_matrix_sqrt(gpu_ctx, n):
  nat, defs, linalg, gp, kernel, mean, objectives, utils = _native()
  rng = np.random.default_rng(n)
  g = rng.normal(size=(n, n + 7))
  cov = g @ g.T / (n + 7)
  f0 = linalg.svd_matrix_sqrt(cov)
  with _spectral(gpu_ctx):
    f1 = linalg.svd_matrix_sqrt(cov)
  assert f1.shape == f0.shape
  assert np.linalg.norm(f1 @ f1.T - cov) <= 4 * n * EPS * np.linalg.norm(cov)
  # low rank: the same rank as the host
  g = rng.normal(size=(n, 3))
  low = g @ g.T
  with _spectral(gpu_ctx):
    f2 = linalg.svd_matrix_sqrt(low)
  assert f2.shape == linalg.svd_matrix_sqrt(low).shape


@pytest.mark.parametrize('method', ['svd', 'eigh'])
def test_routing_sample_from_gp(gpu_ctx, method):
  nat, defs, linalg, gp, kernel, mean, objectives, utils = _native()
  rng = np.random.default_rng(9)
  d = 2
  model = helpers.make_model(rng, 'constant', False, d)
  params = defs.GPParams(model=model)
  x = rng.uniform(size=(90, d))
  wf = utils.DEFAULT_WARP_FUNC
  s0 = gp.sample_from_gp(3, mean.constant, kernel.squared_exponential, params, x, wf, num_samples=4, method=method)
  with _spectral(gpu_ctx):
    s1 = gp.sample_from_gp(3, mean.constant, kernel.squared_exponential, params, x, wf, num_samples=4, method=method)
    w, v = linalg.eigh(linalg.compute_delta_y_and_cov(mean.constant, kernel.squared_exponential, params, x, np.zeros((90, 1)), wf)[1])
  mu = np.asarray(mean.constant(params, x, warp_func=wf), dtype=np.float64).reshape(-1)
  z = np.random.default_rng(3).standard_normal((90, 4))
  with np.errstate(invalid='ignore'):
    f = v * np.sqrt(np.abs(w) if method == 'svd' else w)[None, :]
  np.testing.assert_array_equal(s1, mu[:, None] + f @ z)
  s2 = gp.sample_from_gp(3, mean.constant, kernel.squared_exponential, params, x, wf, num_samples=4, method=method)
  np.testing.assert_array_equal(s2, s0)   # option back at 0: the host path, bit for bit


# ---- arguments and status codes ------------------------------------------------------------------------------------------
def test_arguments_and_status_codes(gpu_ctx):
  nat = _native()[0]
  lib, h = nat.lib(), gpu_ctx.handle
  a = np.eye(4)
  w = np.empty(4)
  pw = nat.ptr(w)
  assert lib.hbo_sym_eig(h, nat.F64, nat.ptr(a), 0, 1, pw, None) == nat.HBO_ERR_ARG
  assert lib.hbo_sym_eig(h, nat.F64, nat.ptr(a), -3, 1, pw, None) == nat.HBO_ERR_ARG
  assert lib.hbo_sym_eig(h, nat.F64, nat.ptr(a), 4, 0, pw, None) == nat.HBO_ERR_ARG
  assert lib.hbo_sym_eig(h, nat.F64, None, 4, 1, pw, None) == nat.HBO_ERR_ARG
  assert lib.hbo_sym_eig(h, nat.F64, nat.ptr(a), 4, 1, None, None) == nat.HBO_ERR_ARG
  for n in (10, 100):
    b = np.stack([np.eye(n), np.eye(n) * 2])
    b[1, n // 2, 1] = np.nan
    rc, wv, vv = _sym_eig(gpu_ctx, b)
    assert rc == nat.HBO_NOT_CONVERGED
    assert np.array_equal(wv[0], np.ones(n)) and np.all(np.isnan(wv[1])) and np.all(np.isnan(vv[1]))
  assert lib.hbo_sym_eig(h, nat.F64, nat.ptr(a), 4, 1, pw, None) == nat.HBO_OK   # the context is still usable
  with pytest.raises(nat.HboError):
    gpu_ctx.get_option('no_such_option')
  prev = gpu_ctx.get_option('spectral')
  with pytest.raises(nat.HboError):
    gpu_ctx.set_option('spectral', 2)
  assert gpu_ctx.get_option('spectral') == prev
