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
