"""CPU side of the tests of batch expected improvement (csrc/qei.hip: hbo_qei_grad_samples, hbo_qei_maximize;
acfun.BatchExpectedImprovement).  Shared by tests/test_qei_cases_host.py (this file judged on its own, no device) and
tests/test_gpu_qei.py (the device against it).  The formulas are those of include/hbo.h.

  reference(sm, xb, z, target, add_noise, scale, ft)   value, gradient [q, D] and the diagnostics of one (sample, batch) pair in the float
                        type `ft` (np.float64 or np.longdouble): the oracle's kernels and means evaluated in `ft`, the factor of
                        K + (noise + eps) I and of Sigma' by a Cholesky of our own in `ft` (SciPy's has no long double); in float64 it
                        agrees with the oracle's own factor and full-covariance posterior (test_qei_cases_host.py).  Knows the MUTANTS.
  restated(...)         the same in float64 in the kernel's order of operations: W = L^-1 explicit, l = W k, beta = W^T l, the
                        right-looking factorisation of Sigma', sums over the base samples in rising b, the reverse pass as two
                        triangular solves, the gradient as sum_i w_ji (x_j - X_i)
  term scales           value: mean_b(|mu_j*| + sum_l |C_j*l z_bl| + |t|); Sigma: k(x_j, x_l) + |l_j| |l_l|; a gradient row: the sum of the
                        absolute values of its terms
  C_VALUE, C_SIGMA, C_GRAD   the restatement's worst error against the long-double reference over CASES, in units of
                        eps64 x term scale x cond(C)^2 (the reverse pass divides by the factor twice); measured by
                        test_qei_cases_host.py::test_restatement_against_longdouble, which asserts measured <= C <= 2 measured.  The
                        device gets mes_cases.DEVICE_FACTOR = 8 times them.
  fp32 caches           the project's existing fp32 figures: for the gradient mes_cases.grad_tol at gamma = 0, 2e-2 of the batch's
                        largest component; for the value mes_cases.posterior_tolerances' figure for a posterior mean, 5e-4 of
                        max(term scale, 1) -- the value is a mean of mu_j* + (C z)_j* - t, whose every part comes from the float32 W and
                        alpha exactly as a posterior mean and standard deviation do, through fp64 sums that add nothing to it
  admitted(...)         the smooth-region condition of a gradient comparison: in the long-double reference EVERY base sample's gap
                        between its two largest f_bj and its |imp_b| exceed 1000 x the value bound of the dtype.  fp64: the bound above.
                        fp32: a factor of the cache rounded to float32 stands in for the device's; the condition asks that it picks the
                        same (j*_b, imp_b > 0) for every b as the long-double reference and that the margins exceed 1000 x eps32 x the
                        value's term scale (B <= 32 keeps that true).  The condition is part of the case: no base sample is left out.
  CASES, problem        the shapes of the GPU tier
"""
import functools
import types
from typing import NamedTuple

import numpy as np

import helpers
import mes_cases as mc
from oracle import hyperbo_oracle as o

WFO = o.DEFAULT_WARP_FUNC
EPS64, EPS32 = mc.EPS64, mc.EPS32
SCALE = mc.SCALE
DEVICE_FACTOR = mc.DEVICE_FACTOR
LD = np.longdouble
# measured by test_restatement_against_longdouble (measured <= C <= 2 measured): 46.6 (SE, n = 127, add_noise = 0), 4.46 (dot product,
# q = 16) and 172 (SE, D = 128).  The units carry cond(C) but not the conditioning of the n x n factor behind alpha, l and beta, which the
# constants therefore absorb: the plain float64 reference, which solves with L instead of multiplying by W, measures 147 in the same place.
C_VALUE, C_SIGMA, C_GRAD = 60.0, 6.0, 200.0
FP32_TOL = mc.grad_tol([0.0], np.float32)   # 2e-2
FP32_VALUE_TOL = 5e-4                       # mes_cases.posterior_tolerances: d_mu of an fp32 posterior
MUTANTS = ('diag_not_halved', 'not_symmetrised', 'coupling_dropped', 'scale_dropped', 'noise_after_scale', 'highest_index',
           'dot_diag_dropped')


# ---- linear algebra in any float type ---------------------------------------------------------------------------------------------
def chol(a):
  """Lower Cholesky factor of `a` in its own dtype, column by column; None when a pivot is not > 0."""
  n = a.shape[0]
  l = np.zeros_like(a)
  for c in range(n):
    p = a[c, c] - np.dot(l[c, :c], l[c, :c])
    if not p > 0:
      return None
    l[c, c] = np.sqrt(p)
    if c + 1 < n:
      l[c + 1:, c] = (a[c + 1:, c] - l[c + 1:, :c] @ l[c, :c]) / l[c, c]
  return l


def solve_lower(l, b):
  """L^-1 b for lower-triangular L, b [n, m], in the dtype of the operands."""
  x = np.array(b, copy=True)
  for i in range(l.shape[0]):
    x[i] = (x[i] - l[i, :i] @ x[:i]) / l[i, i]
  return x


def solve_upper_t(l, b):
  """L^-T b for lower-triangular L."""
  x = np.array(b, copy=True)
  for i in range(l.shape[0] - 1, -1, -1):
    x[i] = (x[i] - l[i + 1:, i] @ x[i + 1:]) / l[i, i]
  return x


def _cond(c):
  return float(np.linalg.cond(np.asarray(c, dtype=np.float64))) if c.shape[0] > 1 else 1.0


# ---- the model's pieces in `ft` ----------------------------------------------------------------------------------------------------
def _params(sm, ft):
  """The warped parameters of a sample as `ft` numbers."""
  g = lambda k: np.asarray(sm.pw.model[k], dtype=np.float64).astype(ft)
  r = types.SimpleNamespace(noise=g('noise_variance').reshape(()), dot=sm.kname == 'dot_product')
  if r.dot:
    r.sigma, r.bias = g('dot_prod_sigma').reshape(()), g('dot_prod_bias').reshape(())
  else:
    r.ls, r.sv = g('lengthscale').reshape(-1), g('signal_variance').reshape(())
  r.lin_w = np.asarray(sm.pw.model['linear_mean']['kernel'], dtype=np.float64).astype(ft).reshape(-1) if sm.mname == 'linear' else None
  return r


def _dk_du(kname, u, k, sv):
  """d k / d u (u: the scaled squared distance); 0 at u == 0 for the Matern pair (linalg.py:183-188)."""
  ft = u.dtype.type
  if kname == 'squared_exponential':
    return -k / ft(2)
  if kname == 'matern32':
    r = np.sqrt(ft(3) * u)
    return np.where(u == 0, ft(0), -sv * ft(3) / ft(2) * np.exp(-r))
  r = np.sqrt(ft(5) * u)
  return np.where(u == 0, ft(0), -sv * ft(5) / ft(6) * np.exp(-r) * (ft(1) + r))


def _dk_dx(sm, pr, xb, x2, kmat):
  """d k(xb_j, x2_i) / d xb_j [q, n, D] in `ft` from the kernel matrix [q, n] of the oracle."""
  if pr.dot:
    return np.broadcast_to((x2 / np.square(pr.sigma))[None, :, :], (xb.shape[0],) + x2.shape)
  diff = (xb[:, None, :] - x2[None, :, :]) / np.square(pr.ls)
  u = np.sum(np.square((xb[:, None, :] - x2[None, :, :]) / pr.ls), axis=-1)
  return (_dk_du(sm.kname, u, kmat, pr.sv) * u.dtype.type(2))[:, :, None] * diff


def _posterior(sm, xb, ft):
  """(pr, L, alpha [n], kq [n, q], kbb [q, q], mean at xb [q]) in `ft`: the oracle's kernels and means, our factor."""
  pr = _params(sm, ft)
  x, y, xb = sm.x.astype(ft), sm.y.astype(ft), np.asarray(xb).astype(ft)
  kxx = sm.ko(sm.po_ft(ft), x, warp_func=None) + np.eye(x.shape[0], dtype=ft) * (pr.noise + ft(1e-6))
  l = chol(np.asarray(kxx, dtype=ft))
  resid = (y - sm.mo(sm.po_ft(ft), x, warp_func=None)).reshape(-1, 1)
  alpha = solve_upper_t(l, solve_lower(l, resid))[:, 0]
  kq = np.asarray(sm.ko(sm.po_ft(ft), x, xb, warp_func=None), dtype=ft)
  kbb = np.asarray(sm.ko(sm.po_ft(ft), xb, xb, warp_func=None), dtype=ft)
  mb = np.asarray(sm.mo(sm.po_ft(ft), xb, warp_func=None), dtype=ft).reshape(-1)
  return pr, l, alpha, kq, kbb, mb, x, xb


def _select(f, target, mutant):
  """(j* [B], imp [B]): the lowest index of the largest f_bj (mutant: the highest)."""
  q = f.shape[1]
  js = q - 1 - np.argmax(f[:, ::-1], axis=1) if mutant == 'highest_index' else np.argmax(f, axis=1)
  return js, f[np.arange(f.shape[0]), js] - target


def _finish(sm, pr, xb, x, z, ft, mutant, scale, target, mu, c, alpha, beta, kq, kbb, js, imp, restate):
  """Value, gradient and diagnostics from mu, C, beta and the selection; restate: the kernel's order of the sums."""
  bn, q = z.shape
  d = xb.shape[1]
  pos = imp > 0
  if restate:
    value = ft(0)
    for b in range(bn):
      if pos[b]:
        value = value + imp[b]
    value = value / ft(bn)
  else:
    value = np.sum(np.where(pos, imp, ft(0))) / ft(bn)
  mubar, cbar = np.zeros(q, dtype=ft), np.zeros((q, q), dtype=ft)
  for b in range(bn):   # rising b
    if pos[b]:
      j = js[b]
      mubar[j] += ft(1)
      cbar[j, :j + 1] += z[b, :j + 1]
  mubar, cbar = mubar / ft(bn), cbar / ft(bn)
  p = np.tril(c.T @ cbar)
  if mutant != 'diag_not_halved':
    p[np.diag_indices(q)] *= ft(1) / ft(2)
  # Sbar = C^-T P C^-1:  Y = P C^-1 (rows), then C^T Sbar = Y (columns)
  yv = solve_upper_t(c, p.T).T
  sbar = solve_upper_t(c, yv)
  g = sbar if mutant == 'not_symmetrised' else (sbar + sbar.T) / ft(2)
  if mutant != 'scale_dropped':
    g = ft(scale) * g
  coef = mubar[:, None] * alpha[None, :] - ft(2) * (g @ beta.T)          # [q, n]
  dkx = _dk_dx(sm, pr, xb, x, kq.T)                                        # [q, n, D]
  dkb = _dk_dx(sm, pr, xb, xb, kbb)                                        # [q, q, D]
  grad, gscale = np.zeros((q, d), dtype=ft), np.zeros((q, d), dtype=ft)
  for j in range(q):
    terms = [coef[j][:, None] * dkx[j]]
    if mutant != 'coupling_dropped':
      off = np.array([l != j for l in range(q)])
      terms.append(ft(2) * g[j][off, None] * dkb[j][off])
    if pr.dot and mutant != 'dot_diag_dropped':
      terms.append((g[j, j] * ft(2) * xb[j] / np.square(pr.sigma))[None, :])
    if pr.lin_w is not None:
      terms.append((mubar[j] * pr.lin_w)[None, :])
    allt = np.concatenate(terms, axis=0)
    grad[j] = np.sum(allt, axis=0)
    gscale[j] = np.sum(np.abs(allt), axis=0)
  fsel = np.abs(mu)[js] + np.sum(np.abs(c[js] * z), axis=1) + abs(ft(target))
  return types.SimpleNamespace(value=value, grad=grad, grad_scale=gscale, value_scale=np.mean(fsel), mubar=mubar, g=g, c=c,
                               cond=_cond(c), js=js, pos=pos, imp=imp)


def reference(sm, xb, z, target, add_noise, scale, ft=np.float64, mutant=None):
  """One (sample, batch) pair in `ft`; .value is NaN (and .grad None) when Sigma' has a pivot that is not > 0."""
  assert mutant is None or mutant in MUTANTS
  pr, l, alpha, kq, kbb, mb, x, xb = _posterior(sm, xb, ft)
  z = np.asarray(z).astype(ft)
  v = solve_lower(l, kq)                        # [n, q]: l_j in the columns
  beta = solve_upper_t(l, v)                    # [n, q]
  mu = kq.T @ alpha + mb
  sig = kbb - v.T @ v
  q = sig.shape[0]
  if mutant == 'noise_after_scale':
    sigp = sig * ft(scale) + np.eye(q, dtype=ft) * ft(add_noise)
  else:
    sigp = (sig + np.eye(q, dtype=ft) * ft(add_noise)) * ft(scale)
  c = chol(sigp)
  sig_scale = np.abs(kbb) + np.outer(np.sqrt(np.sum(v * v, axis=0)), np.sqrt(np.sum(v * v, axis=0)))
  if c is None:
    return types.SimpleNamespace(value=ft(np.nan), grad=None, sigma=sigp, sigma_scale=sig_scale)
  f = mu[None, :] + z @ c.T
  js, imp = _select(f, ft(target), mutant)
  r = _finish(sm, pr, xb, x, z, ft, mutant, scale, target, mu, c, alpha, beta, kq, kbb, js, imp, False)
  srt = np.sort(f, axis=1)
  r.gap = srt[:, -1] - srt[:, -2] if q > 1 else np.full(f.shape[0], np.inf)
  r.sigma, r.sigma_scale, r.mu, r.f = sigp, sig_scale * ft(scale), mu, f
  return r


def restated(sm, xb, z, target, add_noise, scale, w=None, alpha=None):
  """The float64 restatement in the kernel's order.  w, alpha: a cache (W = L^-1 lower [n, n], alpha [n]) to use in the place of the
  float64 one -- the float32-rounded stand-in of the fp32 cases."""
  ft = np.float64
  pr, l, alpha64, kq, kbb, mb, x, xb = _posterior(sm, xb, ft)
  z = np.asarray(z, dtype=ft)
  n, q = kq.shape
  if w is None:
    w = solve_lower(l, np.eye(n))
  alpha = alpha64 if alpha is None else np.asarray(alpha, dtype=ft)
  w = np.tril(np.asarray(w, dtype=ft))
  v = w @ kq                                    # l_j = W k_j
  beta = w.T @ v
  mu = mb + kq.T @ alpha
  sigp = np.zeros((q, q))
  for j in range(q):
    for m in range(j + 1):
      dot = 0.0
      for i in range(n):
        dot = dot + v[i, j] * v[i, m]
      s = kbb[j, m] - dot
      if j == m:
        s = s + add_noise
      sigp[j, m] = s * scale
  c = np.array(sigp)
  for col in range(q):                          # right-looking
    p = c[col, col]
    if not p > 0:
      return types.SimpleNamespace(value=np.nan, grad=None, sigma=sigp)
    dg = np.sqrt(p)
    c[col, col] = dg
    c[col + 1:, col] = c[col + 1:, col] / dg
    for j in range(col + 1, q):
      c[j, col + 1:j + 1] = c[j, col + 1:j + 1] - c[j, col] * c[col + 1:j + 1, col]
  c = np.tril(c)
  f = np.zeros((z.shape[0], q))
  for j in range(q):
    acc = np.full(z.shape[0], mu[j])
    for m in range(j + 1):
      acc = acc + c[j, m] * z[:, m]
    f[:, j] = acc
  js, imp = _select(f, target, None)
  r = _finish(sm, pr, xb, x, z, ft, None, scale, target, mu, c, alpha, beta, kq, kbb, js, imp, True)
  r.sigma, r.f = sigp + np.tril(sigp, -1).T, f
  return r


def cache_f32(sm):
  """(W, alpha) of the sample's cache from a factorisation rounded to float32 at every stored result: the stand-in of an fp32 device
  cache in the admission condition of the fp32 cases."""
  f32 = np.float32
  pr, l, alpha, *_ = _posterior(sm, sm.x[:1], np.float64)
  l32 = l.astype(f32).astype(np.float64)
  w = solve_lower(l32, np.eye(l.shape[0])).astype(f32).astype(np.float64)
  resid = (sm.y.astype(np.float64) - sm.mo(sm.pw, sm.x.astype(np.float64), warp_func=None)).reshape(-1)
  return w, (w.T @ (w @ resid)).astype(f32).astype(np.float64)


# ---- bounds ---------------------------------------------------------------------------------------------------------------------
def value_bound(ref, dtype):
  """Absolute bound of the device's value against the long-double reference `ref`."""
  if np.dtype(dtype) == np.float32:
    return FP32_VALUE_TOL * max(float(ref.value_scale), 1.0)
  return DEVICE_FACTOR * C_VALUE * EPS64 * float(ref.value_scale) * ref.cond**2


def grad_bound(ref, dtype):
  """[q, D] absolute bounds of the device's gradient rows."""
  if np.dtype(dtype) == np.float32:
    return np.full(ref.grad.shape, FP32_TOL * float(np.max(np.abs(ref.grad))))
  return DEVICE_FACTOR * C_GRAD * EPS64 * np.asarray(ref.grad_scale, dtype=np.float64) * ref.cond**2


def ratio(err, bound):
  """err / bound elementwise; where the bound is 0 (a row whose every term is 0) the result must be exact: 0, else inf.  NaN -> inf."""
  err, bound = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(bound, dtype=np.float64)
  r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
  return np.where(np.isnan(r), np.inf, r)


def device_ratios(value, grad, ref, dtype):
  """(value ratio, worst gradient ratio) of a device result against its long-double reference and bounds."""
  rv = float(ratio(float(LD(value) - LD(ref.value)), value_bound(ref, dtype)))
  rg = float(np.max(ratio((np.asarray(grad).astype(LD) - np.asarray(ref.grad).astype(LD)).astype(np.float64), grad_bound(ref, dtype))))
  return rv, rg


def margin_needed(ref, dtype):
  """What every base sample's gap and |imp| must exceed for the gradient comparison."""
  if np.dtype(dtype) == np.float32:
    return 1000.0 * EPS32 * float(ref.value_scale)
  return 1000.0 * value_bound(ref, dtype)


def admitted(sm, xb, z, target, add_noise, scale, dtype, ref=None):
  """(ok, smallest margin, needed) of one (sample, batch) pair; `ref`: its long-double reference, computed when missing."""
  ref = reference(sm, xb, z, target, add_noise, scale, LD) if ref is None else ref
  if ref.grad is None:
    return False, 0.0, np.inf
  margin = float(min(np.min(ref.gap), np.min(np.abs(ref.imp))))
  need = margin_needed(ref, dtype)
  ok = margin > need
  if ok and np.dtype(dtype) == np.float32:
    w, alpha = cache_f32(sm)
    r32 = restated(sm, xb, z, target, add_noise, scale, w=w, alpha=alpha)
    ok = r32.grad is not None and np.array_equal(r32.js, ref.js) and np.array_equal(r32.pos, ref.pos)
  return ok, margin, need


# ---- the cases of the GPU tier ----------------------------------------------------------------------------------------------------
class Case(NamedTuple):
  kname: str
  mname: str
  ns: tuple       # observations per sample (S = len(ns))
  d: int
  q: int
  B: int
  M: int
  dtype: str
  noisy: bool     # add_noise: the model's noise variance (True) or 0

  @property
  def id(self):
    return f'{self.kname}-{self.mname}-n{"_".join(map(str, self.ns))}-d{self.d}-q{self.q}-B{self.B}-M{self.M}-{self.dtype}-{"noise" if self.noisy else "latent"}'

  @property
  def S(self):
    return len(self.ns)


CASES = [
    Case('squared_exponential', 'constant', (1,), 1, 1, 1, 2, 'fp64', True),
    Case('matern32', 'zero', (2,), 3, 2, 255, 2, 'fp64', True),
    Case('matern52', 'linear', (63, 64, 65), 17, 3, 256, 2, 'fp64', True),        # one call mixing three sizes
    Case('dot_product', 'constant', (127,), 3, 16, 257, 2, 'fp64', True),
    Case('squared_exponential', 'linear', (128,), 128, 2, 1024, 2, 'fp64', True),
    Case('matern52', 'zero', (128, 5, 127), 3, 16, 256, 3, 'fp64', True),
    Case('dot_product', 'linear', (65,), 256, 1, 255, 2, 'fp64', True),
    Case('matern32', 'constant', (64,), 17, 3, 1024, 2, 'fp64', False),          # add_noise == 0
    Case('squared_exponential', 'zero', (127,), 3, 3, 257, 5, 'fp64', False),
    Case('matern32', 'linear', (100,), 16, 16, 1024, 2, 'fp64', True),          # 66 KB of LDS: beyond the 64 KB a launch gets by default
    Case('squared_exponential', 'constant', (127,), 3, 3, 32, 2, 'fp32', True),
    Case('dot_product', 'zero', (64, 128), 3, 2, 32, 2, 'fp32', True),
    Case('matern52', 'linear', (65,), 17, 2, 1, 2, 'fp32', True),
]


def np_dtype(case):
  return np.float64 if case.dtype == 'fp64' else np.float32


def _cast(t, dtype):
  return {k: _cast(v, dtype) for k, v in t.items()} if isinstance(t, dict) else np.asarray(t, dtype=dtype)


class _Sample(types.SimpleNamespace):
  def po_ft(self, ft):
    """The sample's WARPED parameters (pw: warped once in float64, what the device is handed) with every leaf in `ft`; the oracle's
    kernels and means are called on them without a warp and compute in the dtype of their inputs."""
    return self.pw if ft == np.float64 else o.GPParams(model=_cast(self.pw.model, ft), config={})


@functools.lru_cache(maxsize=None)
def problem(case, seed=23):
  """The S (model, observations) pairs of a case, the batches xb [M, q, D], the base samples z [B, q] and per-sample targets at the
  0.4 quantile of batch 0's max_j f_bj (so that part of the base samples improve), all on dtype-rounded numbers.  No device.  Computed
  once per case and shared: do not write to it."""
  dt = np_dtype(case)
  rng = np.random.default_rng([seed, len(case.id), case.d, case.q, case.B])
  xb = np.ascontiguousarray(rng.uniform(size=(case.M, case.q, case.d)).astype(dt))
  z = np.ascontiguousarray(rng.standard_normal((case.B, case.q)))
  smp = []
  for n in case.ns:
    model_t = helpers.make_model(rng, case.mname, False, case.d)
    model_t['lengthscale'] = helpers.lengthscale(rng, case.d, 'ard')
    model_t = _cast(model_t, dt)
    po = o.GPParams(model=_cast(model_t, np.float64), config={})
    x, y = helpers.synthetic_task(rng, n, case.d, dtype=dt)
    pw = o.GPParams(model={k: (np.asarray(WFO[k](v), dtype=np.float64) if k in WFO else v) for k, v in po.model.items()}, config={})
    sm = _Sample(model_t=model_t, po=po, pw=pw, x=x, y=y, kname=case.kname, mname=case.mname, ko=getattr(o, case.kname), mo=getattr(o, case.mname),
                 noise=float(np.squeeze(o.retrieve_params(po, ['noise_variance'], WFO)[0])))
    sm.add_noise = sm.noise if case.noisy else 0.0
    r0 = reference(sm, xb[0], z, 0.0, sm.add_noise, SCALE)
    best = np.max(r0.f, axis=1)
    sm.target = float(np.quantile(best, 0.4) - 0.01 * (1.0 + abs(np.quantile(best, 0.4))))
    smp.append(sm)
  return types.SimpleNamespace(case=case, xb=xb, z=z, smp=smp, dtype=np.dtype(dt), targets=np.array([sm.target for sm in smp]),
                               noises=np.array([sm.add_noise for sm in smp]))


@functools.lru_cache(maxsize=None)
def references(case):
  """[S][M] long-double references of a case's pairs, computed once and shared: do not write to them."""
  p = problem(case)
  return [[reference(sm, p.xb[m], p.z, sm.target, sm.add_noise, SCALE, LD) for m in range(case.M)] for sm in p.smp]


def tie_problem():
  """The lowest-index rule: two identical batch points (add_noise > 0) and a base sample of zeros, so f_b0 == f_b1 == mu exactly in any
  arithmetic; the target sits below mu, so the tied sample improves and its weight goes to point 0.  The other base samples are drawn."""
  case = Case('matern52', 'constant', (5,), 3, 2, 4, 1, 'fp64', True)
  base = problem(case)
  xb = base.xb.copy()
  xb[0, 1] = xb[0, 0]
  z = base.z.copy()
  z[0] = 0.0
  sm = base.smp[0]
  mu = float(reference(sm, xb[0], z, 0.0, sm.add_noise, SCALE).mu[0])
  return types.SimpleNamespace(case=case, xb=xb, z=z, smp=[sm], dtype=base.dtype, targets=np.array([mu - 0.3]), noises=base.noises)
