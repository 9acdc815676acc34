"""NumPy restatement of the Kumaraswamy input warp (hyperbo/gp_utils/basis_functions.py:48-61 KumarWarp, kernel.py:186-222
with_kumar_bases), composed with the oracle's public kernels.  Shared by tests/test_kumar_host.py and tests/test_gpu_kumar.py."""
import numpy as np


def squareplus(t):
  t = np.asarray(t, dtype=np.float64)
  return 0.5 * (t + np.sqrt(t * t + 4.0))


def squareplus_grad(t):
  t = np.asarray(t, dtype=np.float64)
  return 0.5 * (1.0 + t / np.sqrt(t * t + 4.0))


def warp(x, a_raw, b_raw):
  """w(x) = 1 - (1 - x^a)^b per column, a = squareplus(a_raw), b = squareplus(b_raw)."""
  a, b = squareplus(a_raw), squareplus(b_raw)
  return 1.0 - (1.0 - np.asarray(x, dtype=np.float64) ** a) ** b


def dw_dab(x, a, b):
  """(dw/da, dw/db) at warped a, b; both defined as their limit 0 at x = 0 and x = 1."""
  x = np.asarray(x, dtype=np.float64)
  inner = (x > 0) & (x < 1)
  xs = np.where(inner, x, 0.5)
  u = xs ** a
  v = 1.0 - u
  da = b * v ** (b - 1.0) * u * np.log(xs)
  db = -(v ** b) * np.log(v)
  return np.where(inner, da, 0.0), np.where(inner, db, 0.0)


def dw_dx(x, a, b):
  x = np.asarray(x, dtype=np.float64)
  return a * b * x ** (a - 1.0) * (1.0 - x ** a) ** (b - 1.0)


def kumar_kernel(base):
  """The oracle kernel `base` on warped inputs; the raw kumar_params live in params.model['kumar_params']."""
  def matrix_map(params, vx1, vx2=None, warp_func=None, diag=False):
    kp = params.model['kumar_params']
    w = lambda v: warp(v, kp['a'], kp['b'])
    return base(params, w(vx1), None if vx2 is None else w(vx2), warp_func=warp_func, diag=diag)
  matrix_map.__name__ = base.__name__
  return matrix_map


def se_nll_ab_grad(model, ds):
  """Analytic d mean-NLL / d (raw a, b) of the SE kernel on warped inputs with a constant / zero mean (the oracle's
  dnll/dK = 1/2 (m^2 K^-1 - s s^T), chained through dK/dw and dw/da, dw/db).  fp64 NumPy."""
  from oracle import hyperbo_oracle as o
  kp = model['kumar_params']
  a, b = squareplus(kp['a']), squareplus(kp['b'])
  ls = o.default_softplus(model['lengthscale']); sv = o.default_softplus(model['signal_variance'])
  noise = o.default_softplus(model['noise_variance']); c = float(model.get('constant', 0.0))
  ga, gb = np.zeros_like(a), np.zeros_like(b)
  for s in ds.values():
    w = warp(s.x, kp['a'], kp['b'])
    ws = w / ls
    sq = np.sum(ws * ws, 1)
    K = sv * np.exp(-0.5 * np.maximum(sq[:, None] + sq[None, :] - 2 * ws @ ws.T, 0))
    A = K + (noise + 1e-6) * np.eye(len(w))
    Ainv = np.linalg.inv(A)
    m = s.y.shape[1]
    r = np.sum(s.y - c, axis=1)
    sv_ = Ainv @ r
    G = 0.5 * (m * m * Ainv - np.outer(sv_, sv_))
    M = G * K
    M = 0.5 * (M + M.T)
    dw = -2.0 * (M.sum(1)[:, None] * w - M @ w) / (ls * ls)      # d nll / d w
    da, db = dw_dab(s.x, a, b)
    ga += np.sum(dw * da, 0); gb += np.sum(dw * db, 0)
  n = len(ds)
  return ga / n * squareplus_grad(kp['a']), gb / n * squareplus_grad(kp['b'])
