"""Pins for the CPU oracle (oracle/hyperbo_oracle.py).

The JAX reference cannot be imported here and its own tests hold no golden values (SURVEY.md
F0.2/F0.3), so the oracle is pinned by: 50-digit mpmath recomputation, central finite differences,
an independent torch.autograd re-expression, the identities the reference's tests assert, and the
NumPy-seeded inputs of hyperbo/basics/linalg_test.py.  All CPU, `-m "not gpu"`.
"""
import os

import mpmath as mp
import numpy as np
import pytest
import scipy.linalg as spla

import helpers
from oracle import hyperbo_oracle as o

WF = o.DEFAULT_WARP_FUNC
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _params(model):
  return o.GPParams(model=model, config={'mlp_features': helpers.MLP_FEATURES})


# --- (1) mpmath 50-digit recomputation ------------------------------------------------------
def _mp_kernel(kname, a, b, ls, sv, sigma, bias):
  if kname == 'dot_product':
    return sum(x * y for x, y in zip(a, b)) / sigma**2 + bias**2
  u = sum(((x - y) / l)**2 for x, y, l in zip(a, b, ls))
  if kname == 'squared_exponential':
    return sv * mp.e**(-u / 2)
  c = 3 if kname == 'matern32' else 5
  r = mp.sqrt(c * u)
  if kname == 'matern32':
    return sv * (1 + r) * mp.e**(-r)
  return sv * (1 + r + r**2 / 3) * mp.e**(-r)


def _mp_softplus(v):
  return mp.log(1 + mp.e**mp.mpf(float(v))) + mp.mpf('1e-10')


@pytest.mark.parametrize('kname', helpers.KERNELS)
@pytest.mark.parametrize('n', [4, 16, 48])
def test_mpmath_nll_alpha_posterior_ei(kname, n):
  mp.mp.dps = 50
  rng = np.random.default_rng(100 + n)
  d = 3
  model = helpers.make_model(rng, 'constant', False, d)
  x, y = helpers.synthetic_task(rng, n, d)
  xq = rng.uniform(size=(3, d))
  params = _params(model)
  kern = getattr(o, kname)
  ls = [_mp_softplus(v) for v in model['lengthscale']]
  sv = _mp_softplus(model['signal_variance']); noise = _mp_softplus(model['noise_variance'])
  sigma = _mp_softplus(model['dot_prod_sigma']); bias = mp.mpf(float(model['dot_prod_bias']))
  const = mp.mpf(float(model['constant']))
  X = [[mp.mpf(float(v)) for v in row] for row in x]
  K = mp.matrix(n, n)
  for i in range(n):
    for j in range(n):
      K[i, j] = _mp_kernel(kname, X[i], X[j], ls, sv, sigma, bias)
    K[i, i] += noise + mp.mpf('1e-6')
  r = mp.matrix([mp.mpf(float(v)) - const for v in y[:, 0]])
  L = mp.cholesky(K)
  alpha = mp.lu_solve(K, r)
  nll = (r.T * alpha)[0] / 2 + sum(mp.log(L[i, i]) for i in range(n)) + mp.mpf(n) / 2 * mp.log(2 * mp.pi)
  # oracle
  nll_o = o.neg_log_marginal_likelihood(o.constant, kern, params, {0: o.SubDataset(x, y)}, WF)
  chol_o, kinvy_o, _ = o.solve_gp_linear_system(o.constant, kern, params, x, y, WF)
  cond = float(np.linalg.cond(np.array(K.tolist(), dtype=np.float64)))
  assert abs(nll_o - float(nll)) <= 1e-13 * max(cond, 1.0) * abs(float(nll)) + 1e-12
  np.testing.assert_allclose(kinvy_o[:, 0], [float(a) for a in alpha], rtol=1e-13 * cond, atol=1e-13 * cond)
  np.testing.assert_allclose(np.diag(chol_o), [float(L[i, i]) for i in range(n)], rtol=1e-12)
  # posterior at xq + EI
  mu_o, var_o = o.predict(o.constant, kern, params, x, y, xq, WF)
  for q in range(xq.shape[0]):
    xqv = [mp.mpf(float(v)) for v in xq[q]]
    kq = mp.matrix([_mp_kernel(kname, X[i], xqv, ls, sv, sigma, bias) for i in range(n)])
    mu = (kq.T * alpha)[0] + const
    var = _mp_kernel(kname, xqv, xqv, ls, sv, sigma, bias) - (kq.T * mp.lu_solve(K, kq))[0]
    assert abs(mu_o[q, 0] - float(mu)) <= 1e-12 * cond * (1 + abs(float(mu)))
    assert abs(var_o[q, 0] - float(var)) <= 1e-12 * cond * (1 + abs(float(var)))
    sd = mp.sqrt(var + noise)
    target = mp.mpf(float(np.max(y)))
    g = (target - mu) / sd
    ei = (mp.npdf(g) - g * (1 - mp.ncdf(g))) * sd
    ei_o = o.expected_improvement_sub(mu_o[q, 0], np.sqrt(var_o[q, 0] + float(noise)), float(target))
    assert abs(ei_o - float(ei)) <= 1e-10 * cond * (abs(float(ei)) + 1e-6)


# --- (2) finite differences for every leaf, every kernel x mean x MLP -----------------------
def _fd_check(kname, mlp, mname, exclude_aligned, rng):
  d = 3
  model = helpers.make_model(rng, mname, mlp, d)
  params = _params(model)
  kern = getattr(o, kname + ('_mlp' if mlp else ''))
  mean = getattr(o, mname)
  ds = {0: o.SubDataset(*helpers.synthetic_task(rng, 12, d)), 1: o.SubDataset(*helpers.synthetic_task(rng, 7, d)),
        2: o.SubDataset(*helpers.synthetic_task(rng, 5, d, m=3), aligned=1),
        3: o.SubDataset(np.zeros((0, d)), np.zeros((0, 1)))}
  _, g = o.nll_value_and_grad(mean, kern, params, ds, WF, exclude_aligned=exclude_aligned)
  x0 = helpers.flatten(model)
  gf = helpers.flatten(g)
  num = np.zeros_like(x0)
  h = 1e-6
  for i in range(x0.size):
    vals = []
    for sgn in (+1, -1):
      xp = x0.copy(); xp[i] += sgn * h
      vals.append(o.neg_log_marginal_likelihood(mean, kern, _params(helpers.unflatten_like(model, xp)), ds, WF,
                                                exclude_aligned=exclude_aligned))
    num[i] = (vals[0] - vals[1]) / (2 * h)
  np.testing.assert_allclose(gf, num, rtol=1e-6 * 200, atol=1e-6)


@pytest.mark.parametrize('kname', helpers.KERNELS)
@pytest.mark.parametrize('mlp', [False, True])
@pytest.mark.parametrize('mname', helpers.MEANS)
def test_finite_difference_gradient(kname, mlp, mname):
  rng = np.random.default_rng(abs(hash((kname, mlp, mname))) % 2**32)
  _fd_check(kname, mlp, mname, True, rng)


def test_finite_difference_gradient_multicolumn_quirk():
  # y with m>1 columns is only reachable with exclude_aligned=False (objectives_test.py:160)
  _fd_check('matern52', False, 'constant', False, np.random.default_rng(5))


# --- (3) independent torch.autograd re-expression -------------------------------------------
def _torch_mu_k(kname, mlp, mname, model_t, x, torch):
  """(mean vector [n,1], kernel matrix without noise, warp) of one sub-dataset, differentiable."""
  def warp(v):
    return torch.nn.functional.softplus(v) + 1e-10
  if True:
    feat = x
    if mlp or mname == 'linear_mlp':
      h = x
      for l in range(len(model_t['mlp_params'])):
        lay = model_t['mlp_params'][f'Dense_{l}']
        h = torch.tanh(h @ lay['kernel'] + lay['bias'])
      if mlp:
        feat = h
    if mname == 'zero':
      mu = torch.zeros((x.shape[0], 1), dtype=x.dtype)
    elif mname == 'constant':
      mu = model_t['constant'] * torch.ones((x.shape[0], 1), dtype=x.dtype)
    else:
      inp = x if mname == 'linear' else h
      mu = inp @ model_t['linear_mean']['kernel'] + model_t['linear_mean']['bias']
    if kname == 'dot_product':
      k = feat @ feat.T / warp(model_t['dot_prod_sigma'])**2 + model_t['dot_prod_bias']**2
    else:
      ls = warp(model_t['lengthscale'])
      diff = (feat[:, None, :] - feat[None, :, :]) / ls
      u = (diff**2).sum(-1)
      sv = warp(model_t['signal_variance'])
      if kname == 'squared_exponential':
        k = sv * torch.exp(-u / 2)
      else:
        c = 3.0 if kname == 'matern32' else 5.0
        # safe sqrt: gradient contribution 0 where u == 0 (hyperbo/basics/linalg.py:173-197)
        r = torch.sqrt(c * torch.where(u > 0, u, torch.ones_like(u))) * (u > 0)
        k = sv * (1 + r) * torch.exp(-r) if kname == 'matern32' else sv * (1 + r + r**2 / 3) * torch.exp(-r)
  return mu, k, warp


def _torch_nll(kname, mlp, mname, model_t, xs, ys, torch):
  total = 0.
  for x, y in zip(xs, ys):
    mu, k, warp = _torch_mu_k(kname, mlp, mname, model_t, x, torch)
    n = x.shape[0]
    cov = k + torch.eye(n, dtype=x.dtype) * (warp(model_t['noise_variance']) + 1e-6)
    chol = torch.linalg.cholesky(cov)
    r_ = y - mu
    alpha = torch.cholesky_solve(r_, chol)
    total = total + (0.5 * (r_.T @ alpha) + torch.log(torch.diagonal(chol)).sum()
                     + 0.5 * n * np.log(2 * np.pi)).sum()
  return total / len(xs)


@pytest.mark.parametrize('kname', helpers.KERNELS)
@pytest.mark.parametrize('mlp,mname', [(False, 'constant'), (True, 'linear_mlp'), (False, 'linear'), (True, 'zero')])
def test_torch_autograd_matches_oracle_gradient(kname, mlp, mname):
  helpers.in_torch_process(_torch_autograd_case, kname, mlp, mname)


def _torch_autograd_case(kname, mlp, mname):
  import torch
  rng = np.random.default_rng(31)
  d = 3
  model = helpers.make_model(rng, mname, mlp, d)
  tasks = [helpers.synthetic_task(rng, 15, d), helpers.synthetic_task(rng, 9, d)]
  ds = {i: o.SubDataset(x, y) for i, (x, y) in enumerate(tasks)}

  def to_t(t):
    if isinstance(t, dict):
      return {k: to_t(v) for k, v in t.items()}
    return torch.tensor(np.asarray(t, dtype=np.float64), requires_grad=True)
  model_t = to_t(model)
  xs = [torch.tensor(x) for x, _ in tasks]
  ys = [torch.tensor(y) for _, y in tasks]
  loss = _torch_nll(kname, mlp, mname, model_t, xs, ys, torch)
  loss.backward()
  kern = getattr(o, kname + ('_mlp' if mlp else ''))
  val, g = o.nll_value_and_grad(getattr(o, mname), kern, _params(model), ds, WF)
  assert abs(val - loss.item()) <= 1e-10 * abs(val)

  def grad_tree(t):
    if isinstance(t, dict):
      return {k: grad_tree(v) for k, v in t.items()}
    return np.zeros(t.shape) if t.grad is None else t.grad.numpy()
  gt = grad_tree(model_t)
  np.testing.assert_allclose(helpers.flatten(g), helpers.flatten(gt), rtol=1e-8, atol=1e-10)


# --- (3b) divergence objectives (objectives.py:29-106, utils.py:84-173): FD, torch.autograd, identities -------
def _aligned_dataset(rng, d):
  return {'a': o.SubDataset(*helpers.synthetic_task(rng, 11, d, m=4), aligned=1),
          'b': o.SubDataset(*helpers.synthetic_task(rng, 6, d, m=7), aligned='x'),
          'iid': o.SubDataset(*helpers.synthetic_task(rng, 9, d)),                 # not aligned -> skipped
          'one': o.SubDataset(*helpers.synthetic_task(rng, 5, d, m=1), aligned=2),  # m = 1 -> cov_data = 0
          'empty': o.SubDataset(np.zeros((0, d)), np.zeros((0, 2)), aligned=3)}


@pytest.mark.parametrize('kind', ['ekl', 'euc'])
@pytest.mark.parametrize('kname', helpers.KERNELS)
@pytest.mark.parametrize('mlp,mname', [(False, 'constant'), (True, 'linear_mlp'), (False, 'linear'), (True, 'zero'),
                                       (False, 'linear_mlp')])
def test_divergence_gradient_finite_difference_and_value(kind, kname, mlp, mname):
  rng = np.random.default_rng(77)
  d = 3
  model = helpers.make_model(rng, mname, mlp, d)
  kern = getattr(o, kname + ('_mlp' if mlp else '')); mean = getattr(o, mname)
  ds = _aligned_dataset(rng, d)
  dist = o.kl_multivariate_normal if kind == 'ekl' else o.euclidean_multivariate_normal
  v, g = o.divergence_value_and_grad(kind, mean, kern, _params(model), ds, WF)
  v_direct = o.multivariate_normal_divergence(mean, kern, _params(model), ds, WF, distance=dist)
  assert abs(v - v_direct) <= 1e-12 * abs(v_direct)
  x0 = helpers.flatten(model); gf = helpers.flatten(g)
  num = np.zeros_like(x0); h = 1e-6
  for i in range(x0.size):
    vals = []
    for sgn in (+1, -1):
      xp = x0.copy(); xp[i] += sgn * h
      vals.append(o.multivariate_normal_divergence(mean, kern, _params(helpers.unflatten_like(model, xp)), ds, WF,
                                                   distance=dist))
    num[i] = (vals[0] - vals[1]) / (2 * h)
  np.testing.assert_allclose(gf, num, rtol=2e-4, atol=2e-6)


@pytest.mark.parametrize('kind', ['ekl', 'euc'])
@pytest.mark.parametrize('kname,mlp,mname', [('squared_exponential', False, 'constant'), ('matern32', True, 'linear_mlp'),
                                             ('dot_product', True, 'linear'), ('matern52', False, 'zero')])
def test_divergence_torch_autograd(kind, kname, mlp, mname):
  helpers.in_torch_process(_divergence_torch_case, kind, kname, mlp, mname)


def _divergence_torch_case(kind, kname, mlp, mname):
  import torch
  rng = np.random.default_rng(5)
  d = 2
  model = helpers.make_model(rng, mname, mlp, d)
  ds = {k: v for k, v in _aligned_dataset(rng, d).items() if k in ('a', 'b', 'one')}

  def to_t(t):
    if isinstance(t, dict):
      return {k: to_t(v) for k, v in t.items()}
    return torch.tensor(np.asarray(t, dtype=np.float64), requires_grad=True)
  model_t = to_t(model)
  total = 0.
  for s in ds.values():
    x = torch.tensor(s.x); y = torch.tensor(s.y)
    mu, k, warp = _torch_mu_k(kname, mlp, mname, model_t, x, torch)
    n, m = y.shape
    mu0 = y.mean(dim=1); yc = y - mu0[:, None]; c0 = yc @ yc.T / m
    k1 = k + torch.eye(n, dtype=x.dtype) * warp(model_t['noise_variance'])
    dvec = mu[:, 0] - mu0
    if kind == 'ekl':
      total = total + torch.trace(torch.linalg.solve(k1, c0)) + dvec @ torch.linalg.solve(k1, dvec) + torch.logdet(k1)
    else:
      total = total + torch.sqrt((dvec**2).sum()) + torch.sqrt(((c0 - k1)**2).sum())
  loss = total / len(ds)
  loss.backward()
  kern = getattr(o, kname + ('_mlp' if mlp else ''))
  v, g = o.divergence_value_and_grad(kind, getattr(o, mname), kern, _params(model), ds, WF)
  assert abs(v - loss.item()) <= 1e-10 * abs(v)

  def grad_tree(t):
    if isinstance(t, dict):
      return {k: grad_tree(v) for k, v in t.items()}
    return np.zeros(t.shape) if t.grad is None else t.grad.numpy()
  np.testing.assert_allclose(helpers.flatten(g), helpers.flatten(grad_tree(model_t)), rtol=1e-8, atol=1e-9)


def test_kl_multivariate_normal_reference_test_inputs():
  # hyperbo/gp_utils/utils_test.py:26-55 (NumPy-seeded inputs, same assertions)
  np.random.seed(1)
  mu0 = np.random.uniform(-5, 5, (10,)); mu1 = np.random.uniform(-5, 5, (10,))
  cov0 = np.random.uniform(-5, 5, (10, 100)); cov0 = cov0 @ cov0.T
  cov1 = np.random.uniform(-5, 5, (10, 100)); cov1 = cov1 @ cov1.T
  assert o.kl_multivariate_normal(mu0, cov0, mu1, cov1, partial=False) > 0
  assert abs(o.kl_multivariate_normal(mu0, cov0, mu0, cov0, partial=False)) <= 1e-5
  # closed form KL between two Gaussians
  n = 10
  kl_exact = 0.5 * (np.trace(np.linalg.solve(cov1, cov0)) + (mu1 - mu0) @ np.linalg.solve(cov1, mu1 - mu0) - n
                    + np.linalg.slogdet(cov1)[1] - np.linalg.slogdet(cov0)[1])
  assert abs(o.kl_multivariate_normal(mu0, cov0, mu1, cov1, partial=False) - kl_exact) <= 1e-8 * abs(kl_exact)
  np.random.seed(1)
  mu0 = np.random.uniform(-5, 5, (100,)); mu1 = np.random.uniform(-5, 5, (100,))
  feat0 = np.random.uniform(-5, 5, (100, 5)); cov0 = feat0 @ feat0.T
  cov1 = np.random.uniform(-5, 5, (100, 1000)); cov1 = cov1 @ cov1.T
  kl = o.kl_multivariate_normal(mu0, cov0, mu1, cov1, partial=False)
  assert 0 < kl < np.inf


# --- (3c) d acquisition / d x_query (what bayesopt.py:116-125 differentiates) vs central differences ---------
@pytest.mark.parametrize('acq', ['ei', 'pi', 'ucb'])
@pytest.mark.parametrize('kname', helpers.KERNELS)
@pytest.mark.parametrize('mlp,mname', [(False, 'constant'), (True, 'linear_mlp'), (False, 'linear'), (True, 'zero'),
                                       (False, 'linear_mlp')])
@pytest.mark.parametrize('n_obs', [0, 17])
def test_acquisition_gradient_finite_difference(acq, kname, mlp, mname, n_obs):
  rng = np.random.default_rng(9)
  d = 3
  model = helpers.make_model(rng, mname, mlp, d)
  params = _params(model)
  kern = getattr(o, kname + ('_mlp' if mlp else '')); mean = getattr(o, mname)
  xo, yo = helpers.synthetic_task(rng, max(n_obs, 1), d)
  xo, yo = xo[:n_obs], yo[:n_obs]
  xq = rng.uniform(size=(5, d))
  if n_obs:
    xq[0] = xo[3]            # a query on top of a training point (Matern safe-sqrt branch)
  param = {'ei': 0.3, 'pi': 0.4, 'ucb': 3.0}[acq]
  sub = {'ei': o.expected_improvement_sub, 'pi': o.probability_of_improvement_sub, 'ucb': o.ucb_sub}[acq]
  add_noise = float(np.squeeze(o.retrieve_params(params, ['noise_variance'], WF)[0])); scale = 1.25

  def value(xqq):
    mu, var = o.predict(mean, kern, params, xo if n_obs else None, yo if n_obs else None, xqq, warp_func=WF)
    var = (var + add_noise) * scale
    return sub(mu, np.sqrt(var), param)
  val, grad = o.acquisition_value_and_grad(acq, mean, kern, params, xo, yo, xq, param, WF, add_noise, scale)
  np.testing.assert_allclose(val, value(xq), rtol=1e-10, atol=1e-12)
  h = 1e-6
  for q in range(xq.shape[0]):
    if q == 0 and n_obs and kname.startswith('matern'):
      continue   # kink of the Matern kernel at zero distance: one-sided derivatives differ
    for j in range(d):
      xp = xq.copy(); xp[q, j] += h; xm = xq.copy(); xm[q, j] -= h
      num = (value(xp)[q, 0] - value(xm)[q, 0]) / (2 * h)
      assert abs(num - grad[q, j]) <= 2e-5 * max(1.0, abs(num)), (q, j, num, grad[q, j])


# --- (4) identities the reference's tests assert ---------------------------------------------
@pytest.mark.parametrize('kname', helpers.KERNELS)
def test_svd_nll_equals_cholesky_nll(kname):  # objectives_test.py:168,185
  rng = np.random.default_rng(7)
  model = helpers.make_model(rng, 'constant', False, 2)
  ds = {i: o.SubDataset(*helpers.synthetic_task(rng, 20, 2)) for i in range(3)}
  a = o.neg_log_marginal_likelihood(o.constant, getattr(o, kname), _params(model), ds, WF)
  b = o.neg_log_marginal_likelihood(o.constant, getattr(o, kname), _params(model), ds, WF, use_cholesky=False)
  assert abs(a / b - 1) < 1e-9


@pytest.mark.parametrize('kname', helpers.KERNELS)
@pytest.mark.parametrize('mlp', [False, True])
def test_gram_shape_symmetry_psd(kname, mlp):  # kernel_test.py:77-152
  rng = np.random.default_rng(3)
  model = helpers.make_model(rng, 'zero', mlp, 4)
  kern = getattr(o, kname + ('_mlp' if mlp else ''))
  x1, x2 = rng.uniform(size=(5, 4)), rng.uniform(size=(7, 4))
  assert kern(_params(model), x1, x2, warp_func=WF).shape == (5, 7)
  k = kern(_params(model), x1, warp_func=WF)
  np.testing.assert_allclose(k, k.T, atol=1e-12)
  assert np.linalg.eigvalsh(k).min() > -1e-10
  np.testing.assert_allclose(kern(_params(model), x1, warp_func=WF, diag=True), np.diag(k), rtol=1e-12)


def test_predict_self_consistency():  # gp_test.py:151-207
  rng = np.random.default_rng(4)
  model = helpers.make_model(rng, 'constant', False, 2)
  x, y = helpers.synthetic_task(rng, 30, 2)
  xq = rng.uniform(size=(9, 2))
  p = _params(model)
  mu, var = o.predict(o.constant, o.matern52, p, x, y, xq, WF)
  mu2, cov = o.predict(o.constant, o.matern52, p, x, y, xq, WF, full_cov=True)
  assert mu.shape == (9, 1) and var.shape == (9, 1) and cov.shape == (9, 9)
  np.testing.assert_allclose(np.diag(cov), var[:, 0], rtol=1e-9, atol=1e-12)
  ds = {0: o.SubDataset(x, y)}
  _, var_n = o.gp_predict_postprocess(p, ds, mu, var, WF, False, True, True)
  noise = float(o.default_softplus(model['noise_variance']))
  np.testing.assert_allclose(var_n, var + noise)
  # unbiased scaling counts every non-aligned sub-dataset (gp.py:615-619)
  ds3 = {0: o.SubDataset(x, y), 1: o.SubDataset(x, y), 2: o.SubDataset(x, y, aligned=1)}
  _, var_s = o.gp_predict_postprocess(p, ds3, mu, var, WF, False, False, True)
  np.testing.assert_allclose(var_s, var * 2.0)
  # prior branch (gp.py:275-282) and near-noiseless interpolation
  mu_p, var_p = o.predict(o.constant, o.matern52, p, None, None, xq, WF)
  np.testing.assert_allclose(mu_p, np.full((9, 1), 0.4))
  np.testing.assert_allclose(var_p, np.full((9, 1), float(o.default_softplus(model['signal_variance']))))
  model2 = dict(model); model2['noise_variance'] = np.array(-40.0)
  ys = np.sin(x.sum(axis=1, keepdims=True))  # smooth target: the jitter-only GP interpolates it
  mu_i, var_i = o.predict(o.constant, o.matern32, _params(model2), x, ys, x[:5], WF)
  np.testing.assert_allclose(mu_i, ys[:5], atol=1e-4)
  assert (np.abs(var_i) < 1e-4).all()


def test_acquisition_properties():
  mu = np.array([[0.1], [0.5], [-0.3]]); sd = np.array([[0.2], [1e-9], [0.7]])
  ei = o.expected_improvement_sub(mu, sd, 0.2)
  assert (ei >= 0).all()
  # acfun.py:108-110 is (phi(g) - g (1 - Phi(g))) sd with g = (target - mu)/sd : as sd -> 0 it
  # tends to max(mu - target, 0)... for the *minimising* sign convention of gamma:
  assert abs(ei[1, 0] - 0.0) < 1e-6 or abs(ei[1, 0] - 0.3) < 1e-6
  np.testing.assert_allclose(o.ucb_sub(mu, sd, 2.0) + o.ucb_sub(mu, sd, 4.0), 2 * o.ucb_sub(mu, sd, 3.0))
  np.testing.assert_allclose(o.probability_of_improvement_sub(mu, sd, 0.2), -(0.2 - mu) / sd)
  assert o.ei_callback_default({}, 0) == 0.0  # acfun.py:146-147


def test_retrieve_params_and_selection_rules():
  p = o.GPParams(model={'lengthscale': np.array([0.0]), 'constant': np.array(2.0)})
  with pytest.raises(ValueError):
    o.retrieve_params(p, ['signal_variance'])
  ls, c = o.retrieve_params(p, ['lengthscale', 'constant'], WF)
  np.testing.assert_allclose(ls, np.log(2.0) + 1e-10)
  assert c == 2.0
  assert o.retrieve_params(p, ['lengthscale'], None)[0] == 0.0
  ds = {0: o.SubDataset(np.zeros((0, 2)), np.zeros((0, 1))), 1: o.SubDataset(np.ones((3, 2)), np.ones((3, 1)), aligned=1)}
  assert o.neg_log_marginal_likelihood(o.zero, o.squared_exponential,
                                       o.GPParams(model=helpers.make_model(np.random.default_rng(0), 'zero', False, 2)), ds, WF) == 0.


# --- (5) hyperbo/basics/linalg_test.py:57-110 -- NumPy-seeded SPD systems ---------------------
def test_reference_linalg_test_inputs():
  np.random.seed(1)
  dim, noise = 10, 1e-3
  for _ in range(10):
    matrix = np.random.randn(dim, dim)
    spd = matrix.T.dot(matrix) + noise * np.eye(dim)
    x = np.random.randn(dim)
    chol, kinvx = o.solve_linear_system(spd, x[:, None])
    np.testing.assert_allclose(chol @ chol.T, spd, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(spd @ kinvx[:, 0], x, rtol=1e-6, atol=1e-8)
    # the custom VJP of x^T K^-1 x (linalg.py:157-167): dK = -outer(K^-1 x, K^-1 x) vs central FD
    vec = np.random.randn(dim, dim); vec = 0.5 * (vec + vec.T); vec /= np.linalg.norm(vec)
    eps = 1e-5
    f = lambda m: float(x @ np.linalg.solve(m, x))
    num = (f(spd + eps / 2 * vec) - f(spd - eps / 2 * vec)) / eps
    exact = float(np.vdot(-np.outer(kinvx, kinvx), vec))
    assert abs(num - exact) <= 1e-4 * abs(exact) + 1e-6
  # non-PD -> NaN, never an exception (JAX cholesky semantics)
  chol, sol = o.solve_linear_system(-np.eye(3), np.ones((3, 1)))
  assert np.isnan(chol).all() and np.isnan(sol).all()


# --- golden fixtures stay reproducible ---------------------------------------------------------
def test_golden_fixtures_reproduce():
  import importlib.util
  spec = importlib.util.spec_from_file_location('make_golden', os.path.join(GOLDEN, 'make_golden.py'))
  mg = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mg)
  for case in mg.CASES:
    name, out = mg.build(case)
    ref = np.load(os.path.join(GOLDEN, name + '.npz'))
    for k in out:
      np.testing.assert_allclose(out[k], ref[k], rtol=1e-9, atol=1e-11, err_msg=f'{name}:{k}')


def test_config_fixtures_reproduce():
  """cfg 1 fixture (SURVEY.md 8(d) seed-1 inputs) is regenerated bit-for-bit-ish by the oracle; the cfg 4 fixture's
  sizes / parameters match bench.cfg4_inputs() and one of its 64 per-task values is recomputed live."""
  import importlib.util
  spec = importlib.util.spec_from_file_location('make_golden_configs', os.path.join(GOLDEN, 'make_golden_configs.py'))
  mc = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mc)
  fx = np.load(os.path.join(GOLDEN, 'cfg1_se_n256_d4.npz'))
  x, y, raw = mc.cfg1_inputs()
  np.testing.assert_array_equal(x, fx['x']); np.testing.assert_array_equal(y, fx['y'])
  p = o.GPParams(model=raw)
  v, g = o.nll_value_and_grad(o.constant, o.squared_exponential, p, {0: o.SubDataset(x, y)}, WF)
  assert abs(v - float(fx['nll'])) <= 1e-12 * abs(v) and abs(v - float(fx['nll_lapack'])) <= 1e-11 * abs(v)
  np.testing.assert_allclose(helpers.flatten(g), fx['grad_flat'], rtol=1e-9, atol=1e-11)
  vs = o.neg_log_marginal_likelihood(o.constant, o.squared_exponential, p, {0: o.SubDataset(x, y)}, WF, use_cholesky=False)
  assert abs(vs - float(fx['nll_svd'])) <= 1e-10 * abs(vs)
  import bench
  f4 = np.load(os.path.join(GOLDEN, 'cfg4_t64_oracle.npz'))
  data, raw4 = bench.cfg4_inputs()
  assert np.array_equal(f4['sizes'], [len(data[k][0]) for k in sorted(data)])
  np.testing.assert_array_equal(f4['model_flat'], helpers.flatten(raw4))
  assert abs(float(f4['nll_mean']) - float(np.mean(f4['nll_per_task']))) <= 1e-12 * abs(float(f4['nll_mean']))
  k = int(np.argmin(f4['sizes']))
  vk, _ = o.nll_sub_dataset_value_and_grad(o.constant, o.squared_exponential, o.GPParams(model=raw4), data[k][0], data[k][1], WF)
  assert abs(vk - f4['nll_per_task'][k]) <= 1e-11 * abs(vk)


def _load_ref_script():
  import importlib.util
  spec = importlib.util.spec_from_file_location('make_golden_from_reference', os.path.join(GOLDEN, 'make_golden_from_reference.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def _oracle_train_record(kname, mname, method, steps, lr, batch_size, model, data):
  """What make_golden_from_reference.py records of gp.infer_parameters, from the ORACLE's driver on the same inputs."""
  from oracle import train_oracle as to
  cfg = {'method': method, 'batch_size': batch_size, 'max_training_step': steps, 'learning_rate': lr, 'mlp_features': helpers.MLP_FEATURES}
  ds = {i: o.SubDataset(xx, yy) for i, (xx, yy) in enumerate(data)}
  log = []
  def cb(*a, **k):
    step = k.get('step', a[0] if a else None)
    prm = k.get('params', k.get('model_params', a[1] if len(a) > 1 else None))
    loss = k.get('loss', a[2] if len(a) > 2 else None)
    log.append((int(step), helpers.flatten(prm), float(loss)))
  whole = iter(lambda: ds, None)          # batch_size above every size: the sub-sampling leaves the sub-datasets whole
  out = to.infer_parameters(getattr(o, mname), getattr(o, kname), o.GPParams(model=to.tree_copy(model), config=cfg), ds, WF,
                            dataset_iter=whole, callback=cb)
  return dict(cb_steps=np.asarray([r[0] for r in log]), cb_params=np.asarray([r[1] for r in log]),
              cb_losses=np.asarray([r[2] for r in log]), final_flat=helpers.flatten(out.model))


def _oracle_hgp_record(samples, x, y, x2, y2, xq):
  """acfun.py:72-82 on an HGP, from the oracle: mean over the parameter samples of the acquisition on the noisy, unbiased posterior."""
  dso = {'test': o.SubDataset(x, y), 'other': o.SubDataset(x2, y2), 'third': o.SubDataset(x2[:5], y2[:5])}
  out = {'ei': [], 'pi': [], 'ucb': []}
  for smp in samples:
    po = o.GPParams(model=smp, config={})
    mu, var = o.predict(o.constant, o.matern52, po, x, y, xq, WF)
    mu, var = o.gp_predict_postprocess(po, dso, mu, var, WF, False, True, True)
    std = np.sqrt(var)
    out['ei'].append(o.expected_improvement_sub(mu, std, o.ei_callback_default(dso, 'test')))
    out['pi'].append(o.probability_of_improvement_sub(mu, std, o.pi_callback_default(dso, 'test')))
    out['ucb'].append(o.ucb_sub(mu, std, 3.0))
  return {k: np.mean(v, axis=0) for k, v in out.items()}


def _check_ref_file(path):
  """One `<case>_ref.npz` (outputs of the JAX reference, tests/golden/make_golden_from_reference.py) against the oracle: the oracle's
  committed fixture `<case>.npz` for the per-function cases, the oracle's training driver / HGP mean re-run on the inputs stored in
  the file for the `train_*` / `hgp_*` cases.  ASSERTS -- a reference file that disagrees is a failure, never a skip."""
  base = os.path.basename(path)
  ref = np.load(path)
  if base.startswith('train_'):
    n_sub = len([k for k in ref.files if k[0] == 'x' and k[1:].isdigit()])
    data = [(ref[f'x{i}'], ref[f'y{i}']) for i in range(n_sub)]
    kname, mname, method = str(ref['kname']), str(ref['mname']), str(ref['method'])
    lr = float(ref['learning_rate'])
    template = helpers.make_model(np.random.default_rng(0), mname, kname.endswith('_mlp'), data[0][0].shape[1])
    model = helpers.unflatten_like(template, ref['model_flat'])
    mine = _oracle_train_record(kname, mname, method, int(ref['steps']), None if np.isnan(lr) else lr, int(ref['batch_size']), model, data)
    assert np.array_equal(mine['cb_steps'], ref['cb_steps']), base
    for k, t in (('cb_losses', 1e-8), ('cb_params', 1e-7), ('final_flat', 1e-7)):
      scale = max(float(np.max(np.abs(ref[k]))), 1.0)
      assert mine[k].shape == ref[k].shape and np.max(np.abs(mine[k] - ref[k])) <= t * scale, f'{base}:{k}'
    return
  if base.startswith('hgp_'):
    template = helpers.make_model(np.random.default_rng(0), 'constant', False, ref['x'].shape[1])
    samples = [helpers.unflatten_like(template, f) for f in ref['samples_flat']]
    mine = _oracle_hgp_record(samples, ref['x'], ref['y'], ref['x2'], ref['y2'], ref['xq'])
    for k in ('ei', 'pi', 'ucb'):
      scale = max(float(np.max(np.abs(ref[k]))), 1e-300)
      assert np.max(np.abs(mine[k].reshape(ref[k].shape) - ref[k])) <= 1e-8 * scale, f'{base}:{k}'
    return
  tol = {'grad_flat': 1e-7, 'ekl_grad_flat': 1e-6, 'euc_grad_flat': 1e-6, 'kinvy': 1e-7, 'cov': 1e-7, 'var': 1e-7}
  mine = np.load(path.replace('_ref.npz', '.npz'))
  for k in ref.files:
    if k not in mine.files:
      continue
    t = tol.get(k, 1e-9)
    scale = max(float(np.max(np.abs(ref[k]))), 1e-300)
    assert np.max(np.abs(np.asarray(mine[k], dtype=np.float64).reshape(ref[k].shape) - ref[k])) <= t * scale, f'{base}:{k}'


def test_golden_fixtures_match_reference():
  """Closes the parity chain when tests/golden/make_golden_from_reference.py has run once where jax is importable:
  every `<case>_ref.npz` (outputs of the JAX reference itself: per-function outputs, the training trajectories of row f1, the HGP
  mean over samples) must agree with the oracle -- a file that is there and disagrees FAILS.  Only the absence of every such file
  skips: then there is nothing to compare and the oracle stays 'parity unpinned' (DESIGN.md section 0)."""
  import glob
  refs = sorted(glob.glob(os.path.join(GOLDEN, '*_ref.npz')))
  if not refs:
    pytest.skip('no *_ref.npz: the JAX reference has not been run (jax is not installable here)')
  for path in refs:
    _check_ref_file(path)


def test_reference_pin_consumer_on_oracle_made_stand_ins(tmp_path):
  """The consumer above has never seen a real `*_ref.npz` (no jax here), so its code paths for the training trajectories and the HGP
  mean are exercised on STAND-INS: files of the reference script's exact layout, filled from the oracle itself (so they must agree),
  then with one number moved (so they must fail).  This pins the plumbing -- file layout, input reconstruction, tolerances -- not
  the oracle: nothing written here is a fixture, and the label 'parity unpinned' does not move."""
  ref = _load_ref_script()
  kname, mname = ref.TRAIN_CASES[2]
  for method, steps, lr in ref.TRAIN_METHODS:
    model, data = ref.train_inputs(kname, mname)
    rec = _oracle_train_record(kname, mname, method, steps, lr, ref.TRAIN_BATCH, model, data)
    arrays = {f'x{i}': xx for i, (xx, yy) in enumerate(data)}
    arrays.update({f'y{i}': yy for i, (xx, yy) in enumerate(data)})
    path = str(tmp_path / f'train_{kname}_{mname}_{method}_ref.npz')
    np.savez_compressed(path, kname=kname, mname=mname, method=method, steps=steps, learning_rate=np.nan if lr is None else lr,
                        batch_size=ref.TRAIN_BATCH, model_flat=helpers.flatten(model), **rec, **arrays)
    assert len(rec['cb_losses']) >= steps
    _check_ref_file(path)
    rec['cb_losses'] = rec['cb_losses'] * (1 + 1e-6)
    np.savez_compressed(path, kname=kname, mname=mname, method=method, steps=steps, learning_rate=np.nan if lr is None else lr,
                        batch_size=ref.TRAIN_BATCH, model_flat=helpers.flatten(model), **rec, **arrays)
    with pytest.raises(AssertionError):
      _check_ref_file(path)
  samples, x, y, x2, y2, xq = ref.hgp_inputs()
  rec = _oracle_hgp_record(samples, x, y, x2, y2, xq)
  path = str(tmp_path / 'hgp_matern52_constant_ref.npz')
  np.savez_compressed(path, x=x, y=y, x2=x2, y2=y2, xq=xq, samples_flat=np.asarray([helpers.flatten(smp) for smp in samples]), **rec)
  _check_ref_file(path)
  rec['ucb'] = rec['ucb'] + 1e-5
  np.savez_compressed(path, x=x, y=y, x2=x2, y2=y2, xq=xq, samples_flat=np.asarray([helpers.flatten(smp) for smp in samples]), **rec)
  with pytest.raises(AssertionError):
    _check_ref_file(path)


def test_cpu_baseline_port_matches_oracle():
  from oracle import cpu_baseline
  rng = np.random.default_rng(9)
  d = 5
  x, y = helpers.synthetic_task(rng, 300, d)
  raw = {'lengthscale': helpers.inv_softplus(np.full(d, 0.6)), 'signal_variance': helpers.inv_softplus(1.0),
         'noise_variance': helpers.inv_softplus(1e-2), 'constant': np.array(0.2)}
  v, g = cpu_baseline.nll_and_grad_se_ard_constant(x, y, raw)
  vo, go = o.nll_value_and_grad(o.constant, o.squared_exponential, o.GPParams(model=raw), {0: o.SubDataset(x, y)}, WF)
  assert abs(v - vo) <= 1e-10 * abs(vo)
  for k in go:
    np.testing.assert_allclose(g[k], go[k], rtol=1e-6, atol=1e-8)
  # C/OpenMP + LAPACK port (what bench.py times); needs oracle/libcpu_port.so from build()
  v2, g2 = cpu_baseline.nll_and_grad_se_ard_constant_omp(x, y, raw)
  assert abs(v2 - vo) <= 1e-10 * abs(vo)
  for k in go:
    np.testing.assert_allclose(g2[k], go[k], rtol=1e-8, atol=1e-10)
  # the all-core form (tile algorithms for potrf / trtri / lauum over OpenMP, one single-threaded BLAS call per tile): tile sizes
  # that divide n, that do not, and one tile for the whole matrix
  for nb in (64, 128, 100, 512):
    v3, g3 = cpu_baseline.nll_and_grad_se_ard_constant_tiled(x, y, raw, nb=nb)
    assert abs(v3 - vo) <= 1e-10 * abs(vo), nb
    for k in go:
      np.testing.assert_allclose(g3[k], go[k], rtol=1e-8, atol=1e-10, err_msg=str(nb))


# ---- an independent third-party implementation of the same Gaussian-process formulas ------------------------------------------
@pytest.mark.parametrize('kname', ['squared_exponential', 'matern32', 'matern52'])
def test_oracle_against_scikit_learn_gaussian_process(kname):
  """The oracle (and through it the HIP path) against scikit-learn's GaussianProcessRegressor -- NOT the reference, but an
  independent, widely used implementation of the formulas the reference's path evaluates (Rasmussen & Williams alg. 2.1):
  ARD kernel values, log marginal likelihood, its gradient with respect to the (log) hyper-parameters, posterior mean and
  standard deviation.  Mapping: hyperbo's K = sv k(r / ls) + (noise + 1e-6) I  <->  ConstantKernel(sv) * RBF / Matern(ls) +
  WhiteKernel(noise + 1e-6); sklearn's theta is the log of (sv, ls_1..D, noise), so d/dtheta = value * d/dvalue."""
  from sklearn.gaussian_process import GaussianProcessRegressor
  from sklearn.gaussian_process.kernels import ConstantKernel, Matern, RBF, WhiteKernel
  rng = np.random.default_rng(8)
  n, d, nq = 60, 3, 17
  x, y = helpers.synthetic_task(rng, n, d)
  xq = rng.uniform(size=(nq, d))
  ls = np.array([0.4, 0.9, 1.7]); sv, noise = 1.3, 0.07
  wf = {k: o.identity_warp for k in ('lengthscale', 'signal_variance', 'noise_variance')}      # identity warps: raw == warped values
  model = {'lengthscale': ls.copy(), 'signal_variance': np.array(sv), 'noise_variance': np.array(noise)}
  p = o.GPParams(model=model)
  base = {'squared_exponential': RBF(length_scale=ls), 'matern32': Matern(length_scale=ls, nu=1.5), 'matern52': Matern(length_scale=ls, nu=2.5)}[kname]
  kern = ConstantKernel(sv) * base + WhiteKernel(noise + 1e-6)
  gpr = GaussianProcessRegressor(kernel=kern, optimizer=None, alpha=0.0, normalize_y=False).fit(x, y[:, 0])
  kfun = getattr(o, kname)
  # Gram (without the white noise)
  np.testing.assert_allclose(kfun(p, x, warp_func=wf), (ConstantKernel(sv) * base)(x), rtol=1e-12, atol=1e-14)
  # log marginal likelihood and its gradient
  lml, dlml = gpr.log_marginal_likelihood(gpr.kernel_.theta, eval_gradient=True)
  v, g = o.nll_value_and_grad(o.zero, kfun, p, {0: o.SubDataset(x, y)}, wf)
  assert abs(v + lml) <= 1e-10 * abs(lml), (v, lml)
  theta_grad = np.concatenate([[g['signal_variance'] * sv], np.asarray(g['lengthscale']) * ls, [g['noise_variance'] * (noise + 1e-6)]])
  np.testing.assert_allclose(-theta_grad, dlml, rtol=1e-7, atol=1e-9)
  # posterior (sklearn's WhiteKernel also sits on the diagonal of the PRIOR at the queries: its variance = latent variance + noise,
  # which is GP.predict(with_noise=True) of the reference up to the 1e-6 jitter)
  mu_s, sd_s = gpr.predict(xq, return_std=True)
  mu_o, var_o = o.predict(o.zero, kfun, p, x, y, xq, wf)
  np.testing.assert_allclose(mu_o[:, 0], mu_s, rtol=1e-9, atol=1e-11)
  np.testing.assert_allclose(np.sqrt(var_o[:, 0] + noise + 1e-6), sd_s, rtol=1e-7, atol=1e-9)
