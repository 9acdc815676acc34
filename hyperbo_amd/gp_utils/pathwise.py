"""Posterior sample paths by Matheron's rule (hbo_sample_paths, include/hbo.h; csrc/paths.hip).

A posterior path is a prior path plus k(x, X) v with v = Ktilde^-1 (y - m(X) - prior path at X - noise draw).  The prior path comes from
random Fourier features for the stationary kernels and from the exact finite basis of the dot-product kernel; the update term is the
posterior-mean machinery with another right-hand side.  S paths of one call share one basis of F features, so every cosine and every
cross-Gram entry is computed once; there is no M x M object.

The draws are made HERE, on the host, from one NumPy Generator, in fp64 and in a fixed order that is part of the contract (the tests'
restatement repeats it); they are then cast to the model dtype.  The device never sees the lengthscale for the prior term.
"""
import numpy as np

from hyperbo_amd import _model
from hyperbo_amd import _native as nat
from hyperbo_amd.basics.params_utils import retrieve_params

MAX_SAMPLES = 1024     # hbo_sample_paths: 1 <= S <= 1024
MAX_FEATURES = 65536   # 1 <= F <= 65536
_MATERN_NU = {nat.KERNEL_MATERN32: 1.5, nat.KERNEL_MATERN52: 2.5}


def as_generator(key):
  """A Generator as it is; an int seeds a new one."""
  if isinstance(key, np.random.Generator):
    return key
  if key is None or isinstance(key, bool) or not isinstance(key, (int, np.integer)):
    raise ValueError(f'key must be a numpy Generator or an int seed, got {key!r}')
  return np.random.default_rng(int(key))


def warped_lengthscale(params, warp_func=None):
  """The lengthscale omega is divided by: the warp applied in fp64 to the raw values as they stand in params.model."""
  from hyperbo_amd.basics import definitions as defs
  raw = defs.GPParams(model={'lengthscale': np.asarray(params.model['lengthscale'], dtype=np.float64)})
  return np.asarray(retrieve_params(raw, ['lengthscale'], warp_func)[0], dtype=np.float64)


def draw(rng, kernel_id, fdim, lengthscale, num_features, num_samples, n_obs):
  """(omega [F, fdim], phase [F], w [F, S], eps [n_obs, S] or None) in fp64, drawn in this order:
    1. z = rng.standard_normal((F, fdim))
    2. Matern, nu = 1.5 / 2.5: g = rng.chisquare(2 nu, F); z *= sqrt(2 nu / g)[:, None]   (multivariate t with 2 nu degrees of freedom:
       the spectral density of the Matern kernel)
    3. omega = z / lengthscale   (warped; one entry is broadcast)
    4. phase = rng.uniform(0, 2 pi, F)
    5. w = rng.standard_normal((F, S))
    6. eps = rng.standard_normal((n_obs, S)), with observations only
  The dot-product kernel has an exact basis of F = fdim + 1 functions: steps 1-4 are skipped (omega and phase come back as zeros) and
  `num_features` is ignored."""
  s = int(num_samples)
  if kernel_id == nat.KERNEL_DOT:
    f = fdim + 1
    omega, phase = np.zeros((f, fdim)), np.zeros(f)
  else:
    f = int(num_features)
    z = rng.standard_normal((f, fdim))
    nu = _MATERN_NU.get(kernel_id)
    if nu is not None:
      g = rng.chisquare(2 * nu, f)
      z *= np.sqrt(2 * nu / g)[:, None]
    ls = np.broadcast_to(np.reshape(np.asarray(lengthscale, dtype=np.float64), (-1,)), (fdim,))
    omega = z / ls
    phase = rng.uniform(0, 2 * np.pi, f)
  w = rng.standard_normal((f, s))
  eps = rng.standard_normal((int(n_obs), s)) if n_obs else None
  return omega, phase, w, eps


def sample_paths(mean_func, cov_func, params, x_query, warp_func=None, handle=None, input_dim=None, num_samples=1, num_features=1024,
                 key=None, mean_column=False):
  """[M, S] values of S posterior paths at x_query in the model dtype, over the observations behind `handle` (a linalg.CacheHandle)
  or from the prior (handle None); f is the latent, noise-free function.  mean_column: one more column, with zero draws, is evaluated
  in the same call and returned last -- the posterior mean of hbo_predict."""
  rng = as_generator(key)
  xq = np.asarray(x_query)
  dtype = handle.dtype if handle is not None else _model.infer_dtype(xq)
  xq = np.ascontiguousarray(xq, dtype=dtype)
  if xq.ndim != 2:
    raise ValueError(f'x_query must be [M, D], got {xq.shape}')
  s, f = int(num_samples), int(num_features)
  s_all = s + int(bool(mean_column))
  if s < 1 or s_all > MAX_SAMPLES:
    raise ValueError(f'num_samples must lie in 1..{MAX_SAMPLES - int(bool(mean_column))}, got {num_samples}')
  if f < 1 or f > MAX_FEATURES:
    raise ValueError(f'num_features must lie in 1..{MAX_FEATURES}, got {num_features}')
  bm = _model.BuiltModel(mean_func, cov_func, params, warp_func, dtype, xq.shape[1] if input_dim is None else input_dim)
  ls = None
  if bm.kernel_id != nat.KERNEL_DOT:
    ls = warped_lengthscale(params, warp_func)
  n_obs = handle.n if handle is not None else 0
  omega, phase, w, eps = draw(rng, bm.kernel_id, bm.feat_dim, ls, f, s, n_obs)
  if mean_column:
    w = np.hstack([w, np.zeros((w.shape[0], 1))])
    eps = None if eps is None else np.hstack([eps, np.zeros((eps.shape[0], 1))])
  cast = lambda a: None if a is None else np.ascontiguousarray(a, dtype=dtype)
  omega, phase, w, eps = cast(omega), cast(phase), cast(w), cast(eps)
  out = np.empty((xq.shape[0], s_all), dtype=dtype)
  if xq.shape[0] == 0:
    return out
  ctx = handle.ctx if handle is not None else nat.default_context()
  ctx.check(nat.lib().hbo_sample_paths(ctx.handle, bm.ref(), handle.handle if handle is not None else None, nat.ptr(xq), xq.shape[0], s_all,
                                       w.shape[0], nat.ptr(omega), nat.ptr(phase), nat.ptr(w), nat.ptr(eps), nat.ptr(out)))
  return out
