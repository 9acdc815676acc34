"""Acquisition functions -- hyperbo/bo_utils/acfun.py:36-185.

For a plain GP the posterior and the EI/PI/UCB epilogue run fused on the GPU (hbo_acq).  For an HGP
(acfun.py:72-82: the mean over the model-parameter samples) all samples are factorised as ONE batch and
their posteriors + epilogues queue up on the device (hbo_acq_samples) -- the counterpart of a `jax.vmap`
over the draws; the `*_sub` functions are the host restatement of the maths, used for callables outside
the registry.
"""
import collections
import contextlib
import functools
from typing import Any, Callable, Union

import numpy as np

from hyperbo_amd import _model
from hyperbo_amd import _native as nat
from hyperbo_amd.basics import definitions as defs
from hyperbo_amd.basics.params_utils import retrieve_params
from hyperbo_amd.gp_utils import gp

partial = functools.partial


def random_search(model, x_queries, **unused_kwargs):
  """Uniformly sampled random array (acfun.py:29-34) from model.rng (numpy Generator)."""
  assert model.rng is not None, 'Random search requires random key.'
  return model.rng.uniform(size=(x_queries.shape[0], 1))


def _paths_over_pool(model, sub_dataset_key, x_queries, num_samples, key, num_features):
  if isinstance(model, gp.HGP):
    raise ValueError('Thompson sampling is defined for a GP with one set of hyper-parameters, not for an HGP')
  return model.sample_paths(np.asarray(x_queries), sub_dataset_key=sub_dataset_key, num_samples=num_samples, num_features=num_features,
                            key=key)


def thompson_sampling(model, sub_dataset_key, x_queries, key=None, num_features=1024, **unused_kwargs):
  """[M, 1]: ONE posterior sample path over the candidates (GP.sample_paths); its argmax is a Thompson-sampling suggestion.  key: a
  numpy Generator or an int seed, None takes model.rng.  Usable as `ac_func` of the host loops of bayesopt.py; it has neither
  value_and_grad nor maximize, so bayesopt.bayesopt keeps the best candidate unrefined."""
  return _paths_over_pool(model, sub_dataset_key, x_queries, 1, key, num_features)


def thompson_batch(model, sub_dataset_key, x_queries, batch_size, key=None, num_features=1024):
  """`batch_size` candidate indices, the argmax of one posterior path each (the lowest index among equals): q parallel suggestions
  from a single device call."""
  return np.argmax(_paths_over_pool(model, sub_dataset_key, x_queries, int(batch_size), key, num_features), axis=0)


def thompson_maximize(model, sub_dataset_key, x_candidates, batch_size=1, key=None, num_features=1024, starts=4, bounds=None, opts=None):
  """[batch_size, D] float64: continuous Thompson sampling -- the maximisers over the box of `batch_size` posterior sample paths,
  q suggestions from q paths x `starts` starts in one device call.  One draw of `batch_size` paths (GP.draw_paths) is scored at the
  candidates; per path the `starts` best candidates (stable order, the lower index first among equals) start a projected L-BFGS on
  the path itself (PathDraws.maximize: hbo_paths_maximize); per path the refined point with the largest value is returned, the lower
  start index among equals (a path without a finite value keeps its best candidate).  key: a numpy Generator or an int seed, None
  takes model.rng; bounds: None ([0, 1]^D) or D (lo, hi) pairs; opts: as PathDraws.maximize."""
  if isinstance(model, gp.HGP):
    raise ValueError('Thompson sampling is defined for a GP with one set of hyper-parameters, not for an HGP')
  xc = np.asarray(x_candidates)
  if xc.ndim != 2 or xc.shape[0] < 1:
    raise ValueError(f'x_candidates must be [M, D] with M >= 1, got {xc.shape}')
  q, r = int(batch_size), min(int(starts), xc.shape[0])
  if q < 1 or r < 1:
    raise ValueError('batch_size and starts must be at least 1')
  draws = model.draw_paths(sub_dataset_key, num_samples=q, num_features=num_features, key=key)
  scores = np.asarray(draws.values(xc), dtype=np.float64)                      # [M, q]
  order = np.argsort(-scores, axis=0, kind='stable')[:r]                       # [r, q]
  x0 = np.asarray(xc, dtype=np.float64)[order.T]                               # [q, r, D]
  x, val, _ = draws.maximize(x0, bounds=bounds, opts=opts)
  out = x0[:, 0, :].copy()
  for s in range(q):
    finite = np.isfinite(val[s])
    if finite.any():
      out[s] = x[s, int(np.argmax(np.where(finite, val[s], -np.inf)))]
  return out


class ThompsonContinuous:
  """Thompson sampling for the continuous loop bayesopt.bayesopt: called, it scores candidates with a fresh posterior path (as
  thompson_sampling does); `suggest` refines the best candidates on that path's own gradient (thompson_maximize) -- the loop takes
  its next point from there, the prior branch included."""
  __name__ = 'thompson_continuous'

  def __init__(self, num_features=1024, starts=4, opts=None):
    self.num_features, self.starts, self.opts = num_features, starts, opts

  def __call__(self, model, sub_dataset_key, x_queries, key=None, **unused_kwargs):
    return thompson_sampling(model, sub_dataset_key, x_queries, key=key, num_features=self.num_features)

  def suggest(self, *, model, sub_dataset_key, x_candidates, key=None, batch_size=1, bounds=None):
    """[batch_size, D]: thompson_maximize from the candidates."""
    return thompson_maximize(model, sub_dataset_key, x_candidates, batch_size=batch_size, key=key, num_features=self.num_features,
                             starts=self.starts, bounds=bounds, opts=self.opts)


thompson_continuous = ThompsonContinuous()


def _norm_pdf(x):
  return np.exp(-0.5 * x * x) / np.sqrt(2 * np.pi)


def _norm_cdf(x):
  from math import erfc
  return 0.5 * np.vectorize(erfc)(-np.asarray(x, dtype=np.float64) / np.sqrt(2.0))


def expected_improvement_sub(mu, std, target):
  gamma = (target - mu) / std  # acfun.py:108-110
  # 1 - cdf(gamma) is written cdf(-gamma) = erfc(gamma / sqrt 2) / 2: the literal form cancels (relative error 2e-3 at gamma = 7,
  # negative values at 8); the device epilogue (csrc/kernfun.h: ei_over_sd) evaluates the same expression
  # (the floor: where pdf is a denormal, gamma > 37.6, the two rounded terms can differ by a few quanta of either sign; NaN stays NaN)
  return np.maximum(_norm_pdf(gamma) - gamma * _norm_cdf(-gamma), 0.0) * std


def probability_of_improvement_sub(mu, std, target):
  gamma = (target - mu) / std
  return -gamma


def ucb_sub(mu, std, beta=3.):
  return mu + beta * std


_NATIVE_ID = {expected_improvement_sub: nat.ACQ_EI, probability_of_improvement_sub: nat.ACQ_PI,
              ucb_sub: nat.ACQ_UCB}
# acquisition function object -> (acq_id, param_mode, param) of hbo_bo_simulated: the epilogue and the default callback's parameter
# rule, which the device loop (bayesopt.py: bo_on_device) evaluates from the observed y itself.  Filled below, where the objects exist.
_BO_DEVICE = {}


def _leaves(t):
  if isinstance(t, dict):
    for k in sorted(t):
      yield from _leaves(t[k])
  else:
    yield t


def _samples_fingerprint(model, samples, dtype):
  """Content fingerprint of an HGP's parameter samples: the bytes of every leaf (an in-place edit that keeps a sum, or a replaced
  array on a recycled id, both change it), the config entries a BuiltModel reads, input_dim, warp / mean / covariance identities."""
  import hashlib
  h = hashlib.blake2b(digest_size=16)
  for smp in samples:
    for v in _leaves(smp):
      a = np.ascontiguousarray(v)
      h.update(a.dtype.str.encode()); h.update(repr(a.shape).encode()); h.update(a.tobytes())
    h.update(b'|')
  cfg = model.params.config
  return (np.dtype(dtype).str, id(model.warp_func), model.mean_func, model.cov_func, model.input_dim,
          repr(cfg.get('mlp_features')), len(samples), h.digest())


def _sample_models(model, samples, dtype):
  """One hbo_model per parameter sample, rebuilt only when the fingerprint moved (0.05-0.1 ms of Python each)."""
  finger = _samples_fingerprint(model, samples, dtype)
  cached = getattr(model, '_hbo_sample_models', None)
  if cached is None or cached[0] != finger:
    built, noises = [], []
    for smp in samples:
      ps = defs.GPParams(config=model.params.config, model=smp)
      built.append(_model.BuiltModel(model.mean_func, model.cov_func, ps, model.warp_func, dtype, model.input_dim))
      nv, = retrieve_params(ps, ['noise_variance'], warp_func=model.warp_func)
      noises.append(float(np.squeeze(nv)))
    cached = (finger, built, noises)
    model._hbo_sample_models = cached
  return cached[1], cached[2]


def _per_sample(value, s):
  """[s] doubles for ctypes, every sample with the same value."""
  return (nat.C.c_double * s)(*([float(value)] * s))


def _sample_args(built, handles, noises):
  """The per-sample ctypes arrays of the batched calls: (models, caches or None without handles, noises)."""
  s = len(built)
  structs = (nat.Model * s)(*[b.struct for b in built])
  caches = None if handles is None else (nat.C.c_void_p * s)(*[h.handle for h in handles])
  nse = (nat.C.c_double * s)(*[float(v) for v in noises])
  return structs, caches, nse


def _ctx_and_cache(handle):
  """(context, cache pointer) of a call over one factor handle; without one (the prior branch): the default context and None."""
  return (handle.ctx, handle.handle) if handle is not None else (nat.default_context(), None)


def _single_model(model, sub_dataset_key, x_queries=None):
  """The set-up of the single-model calls: (factor handle or None without observations, x_queries in the model dtype, BuiltModel,
  noise, scale); the last three are None for an empty set of queries.  Fused device path: posterior (gp.py:562-620 incl. +noise
  and T/(T-1)) + acquisition epilogue."""
  handle = None
  if model.has_observations(sub_dataset_key):
    model.setup_predictor(sub_dataset_key)
    handle = model.params.cache[sub_dataset_key].handle
  dtype = handle.dtype if handle is not None else _model.infer_dtype(x_queries)
  xq = None if x_queries is None else np.ascontiguousarray(x_queries, dtype=dtype)
  if xq is not None and xq.shape[0] == 0:
    return handle, xq, None, None, None
  add_noise, scale = model.predict_noise_and_scale(True, True)
  bm = _model.BuiltModel(model.mean_func, model.cov_func, model.params, model.warp_func, dtype, model.input_dim)
  return handle, xq, bm, add_noise, scale


def _samples_per_call(n, dtype, n_samples):
  """How many samples hbo_acq_samples may factorise at once: every sample holds a complete cache (Gram -> L, L^-1 and the
  K^-1 scratch, 3 matrices of npad x ld) -- at most HALF of the device's memory, and the entry point's own limit of 4096."""
  npad = -(-n // 128) * 128
  es = np.dtype(dtype).itemsize
  per = 3 * (npad + 128) * (npad + 128 // es) * es + (1 << 20)
  mem = nat.C.c_int64(0); cus = nat.C.c_int32(0)
  ctx = nat.default_context()
  nat.lib().hbo_device_info(ctx.device, None, 0, nat.C.byref(cus), nat.C.byref(mem))
  budget = (mem.value or (64 << 30)) // 2
  return int(max(1, min(n_samples, 4096, budget // per)))


def hgp_sample_values(model, sub_dataset_key, x_queries, acq_id, acfun_param):
  """(S, M, 1) acquisition values of every model-parameter sample of an HGP from batched device calls: the S Gram matrices of
  the sub-dataset are built, factorised and inverted together (one ModelDev per task), the S posterior + acquisition passes
  follow one another on the stream (hbo_acq_samples).  gp.py:666-682 / acfun.py:72-82 as a batch.  The samples go in chunks
  that fit the device (`_samples_per_call`); a chunk that still fails to allocate is halved down to one sample per call."""
  samples = model.get_model_params_samples()
  sub = model.dataset[sub_dataset_key]
  x = np.asarray(sub.x)
  y = np.asarray(sub.y)
  dtype = _model.infer_dtype(x, y)
  x = np.ascontiguousarray(x, dtype=dtype)
  y = np.ascontiguousarray(y.reshape(x.shape[0], -1), dtype=dtype)
  xq = np.ascontiguousarray(x_queries, dtype=dtype)
  _, scale = model.predict_noise_and_scale(True, True)
  built, noises = _sample_models(model, samples, dtype)
  s_count = len(samples)
  out = np.empty((s_count, xq.shape[0], 1), dtype=dtype)
  ctx = nat.default_context()
  chunk = _samples_per_call(x.shape[0], dtype, s_count)
  s0 = 0
  while s0 < s_count:
    sc = min(chunk, s_count - s0)
    structs, _, nse = _sample_args(built[s0:s0 + sc], None, noises[s0:s0 + sc])
    part = out[s0:s0 + sc]
    rc = nat.lib().hbo_acq_samples(ctx.handle, structs, sc, nat.ptr(x), x.shape[0], nat.ptr(y), y.shape[1], nat.ptr(xq), xq.shape[0],
                                   int(acq_id), _per_sample(acfun_param, sc), nse, float(scale), part.ctypes.data_as(nat.C.c_void_p))
    if rc == nat.HBO_ERR_HIP and sc > 1:      # out of device memory after all: smaller chunks, same result
      chunk = max(1, sc // 2)
      continue
    ctx.check(rc)
    s0 += sc
  return out


def _array_digest(*arrays):
  import hashlib
  h = hashlib.blake2b(digest_size=16)
  for a in arrays:
    a = np.ascontiguousarray(a)
    h.update(a.dtype.str.encode()); h.update(repr(a.shape).encode()); h.update(a.tobytes())
  return h.digest()


def drop_sample_caches(model):
  """Close the per-sample factorisations an HGP acquisition gradient left on the model (called when its dataset changes)."""
  cached = getattr(model, '_hbo_sample_caches', None)
  if cached is not None:
    for h in cached[1]:
      h.close()
    model._hbo_sample_caches = None


def _factor_sample(model, sub, smp):
  """The factorisation of the sub-dataset `sub` under the parameter sample `smp`: a handle the caller keeps or closes."""
  from hyperbo_amd.basics import linalg
  return linalg.factor(model.mean_func, model.cov_func, defs.GPParams(config=model.params.config, model=smp), sub.x, sub.y, model.warp_func)


def _hgp_sample_caches(model, sub_dataset_key, samples, dtype):
  """Factorisations of one sub-dataset under the parameter samples, kept on the model until the samples or the observations
  change (CONTENT fingerprint of x / y: an in-place edit of the observations must not be served a stale factor): bayesopt()'s inner
  L-BFGS-B (bayesopt.py:116-125) differentiates the acquisition dozens of times with the model fixed, and the reference would
  re-factorise all S samples every time (gp.py:676-678 drops the cache per sample).  Only as many samples as fit HALF of the
  device memory are kept (`_samples_per_call`, the budget of hgp_sample_values); the caller factorises the rest per call."""
  sd = model.dataset[sub_dataset_key]
  finger = (_samples_fingerprint(model, samples, dtype), sub_dataset_key, _array_digest(sd.x, sd.y))
  cached = getattr(model, '_hbo_sample_caches', None)
  if cached is not None and cached[0] == finger:
    return cached[1]
  drop_sample_caches(model)
  keep = _samples_per_call(np.shape(sd.x)[0], dtype, len(samples))
  handles = []
  try:
    for smp in samples[:keep]:
      handles.append(_factor_sample(model, sd, smp))
  except nat.HboError:
    # out of device memory after all: keep the factors that were built, the rest go one at a time
    if not handles:
      raise
  model._hbo_sample_caches = (finger, handles)
  return handles


def _each_sample(model, sub_dataset_key, samples, built, noises, handles):
  """(i, BuiltModel, noise, factor handle) per parameter sample of an HGP, for the calls that take one sample at a time: the kept factors
  first (`_hgp_sample_caches`); a sample beyond the budget is factorised, yielded and closed on the spot; the prior branch: None.
  Close the generator (contextlib.closing): a caller's exception then closes the factor in flight at once."""
  sub = model.dataset[sub_dataset_key] if model.has_observations(sub_dataset_key) else None
  for i, (bm, noise) in enumerate(zip(built, noises)):
    transient = sub is not None and i >= len(handles)
    h = _factor_sample(model, sub, samples[i]) if transient else (handles[i] if sub is not None else None)
    try:
      yield i, bm, noise, h
    finally:
      if transient:
        h.close()


ACQ_FUSED_MAX_N = 128   # hbo_acq_grad_samples: one 128-block per cache


def _acq_blocked(model):
  """True when model.params.config['acq_blocked'] asks for the entry points without the 128-observation limit
  (hbo_acq_grad_samples_blocked, hbo_acq_maximize_blocked).  A model without params or config has not asked."""
  cfg = getattr(getattr(model, 'params', None), 'config', None)
  return bool(cfg.get('acq_blocked')) if isinstance(cfg, dict) else False


def _blocked_max_n(model):
  """The `max_n` of `_acq_fused_unmet` / `_acq_opt_unmet` for this model: None (no limit) with config['acq_blocked']."""
  return None if _acq_blocked(model) else ACQ_FUSED_MAX_N


def _acq_mlp(model):
  """True when model.params.config['acq_mlp'] asks for the entry points that serve MLP-basis kernels and the linear_mlp mean
  (hbo_acq_grad_samples_mlp, hbo_acq_maximize_mlp).  They have no 128-observation limit: the key implies 'acq_blocked'.  A model
  without params or config has not asked."""
  cfg = getattr(getattr(model, 'params', None), 'config', None)
  return bool(cfg.get('acq_mlp')) if isinstance(cfg, dict) else False


def _acq_fused_unmet(model, sub_dataset_key, n_samples=1, n_kept=None, enabled=None, max_n=ACQ_FUSED_MAX_N, allow_mlp=False):
  """The first condition that keeps a value_and_grad call from the one-launch path (hbo_acq_grad_samples, context option
  'acq_fused'), as a message, or None.  Host-side checks only.  n_kept: factor handles at hand for the n_samples parameter samples
  (None: not known yet); enabled: the option's value (None: read from the default context); max_n: the largest sub-dataset (None:
  no limit -- the caller goes to the _blocked entry points); allow_mlp: the MLP-basis and linear_mlp conditions are skipped (the
  caller goes to the _mlp entry points)."""
  if not (nat.acq_fused_enabled() if enabled is None else enabled):
    return "the context option 'acq_fused' is off"
  if not model.has_observations(sub_dataset_key):
    return 'the sub-dataset has no observations (the prior branch)'
  n = np.shape(model.dataset[sub_dataset_key].x)[0]
  if max_n is not None and n > max_n:
    return f'the sub-dataset has {n} > {max_n} observations'
  if not allow_mlp and getattr(model.cov_func, 'uses_mlp', False):
    return 'the kernel runs on an MLP basis'
  if not allow_mlp and getattr(model.mean_func, 'mean_id', None) == nat.MEAN_LINEAR_MLP:
    return 'the mean is linear_mlp'
  if getattr(model.cov_func, 'uses_kumar', False):
    return 'the kernel is input-warped (Kumaraswamy)'
  if n_kept is not None and n_kept < n_samples:
    return f'only {n_kept} of the {n_samples} per-sample factors fit the device budget'
  return None


ACQ_OPT_DEFAULTS = dict(memory=10, ls_steps=20, max_iters=200, c1=1e-4, tau=0.5, pgtol=1e-5, ftol=2.2e-9)
ACQ_OPT_SEGMENT = 48       # evaluations per hbo_acq_maximize call (profiles/acq_opt.md: how it was chosen)
ACQ_OPT_MAX_EVALS = 4096   # evaluations a maximisation may spend in all


def _acq_opt_unmet(model, sub_dataset_key, acfun_sub, n_samples=1, n_kept=None, max_n=ACQ_FUSED_MAX_N, allow_mlp=False):
  """The first condition that keeps a maximisation off the device loop (hbo_acq_maximize), as a message, or None: an acquisition
  function outside the native registry, then `_acq_fused_unmet`'s conditions without the option check.  Host-side checks only."""
  if acfun_sub not in _NATIVE_ID:
    return f'the acquisition function {getattr(acfun_sub, "__name__", acfun_sub)!r} is not one of the native ones (EI, PI, UCB)'
  return _acq_fused_unmet(model, sub_dataset_key, n_samples, n_kept, enabled=True, max_n=max_n, allow_mlp=allow_mlp)


# The routes of the registry's entry points over finished factors: the names of the gradient and the maximiser, and what
# `_acq_fused_unmet` / `_acq_opt_unmet` are asked on that route (max_n: the largest sub-dataset, None: no limit; allow_mlp)
_Route = collections.namedtuple('_Route', 'grad maximize max_n allow_mlp')
_ROUTES = {
    'small': _Route('hbo_acq_grad_samples', 'hbo_acq_maximize', ACQ_FUSED_MAX_N, False),
    'blocked': _Route('hbo_acq_grad_samples_blocked', 'hbo_acq_maximize_blocked', None, False),
    'mlp': _Route('hbo_acq_grad_samples_mlp', 'hbo_acq_maximize_mlp', None, True),
}


def _route_of(model):
  """The route model.params.config asks for: 'acq_mlp' wins (it implies no size limit), then 'acq_blocked', else the one-block one."""
  return _ROUTES['mlp' if _acq_mlp(model) else ('blocked' if _acq_blocked(model) else 'small')]


# What a call over finished factors evaluates: the names of its gradient entry point and its maximiser, and args(s_count), the ctypes
# arguments they take where the registry's take (acq_id, params[S])
_Request = collections.namedtuple('_Request', 'grad maximize args')


def _registry_request(route, acq_id, param):
  """EI / PI / UCB by acq_id on a route of _ROUTES, every sample with the parameter `param`."""
  return _Request(route.grad, route.maximize, lambda s: (int(acq_id), _per_sample(param, s)))


def _mes_request(maxima):
  """Max-value entropy search under the maxima [S, K] float64: (ystar, K)."""
  def args(s_count):
    if maxima.dtype != np.float64 or maxima.ndim != 2 or maxima.shape[0] != s_count or not maxima.flags.c_contiguous:
      raise ValueError(f'maxima must be a contiguous float64 array [{s_count}, K], got {maxima.dtype} {maxima.shape}')
    return maxima.ctypes.data_as(nat.C.POINTER(nat.C.c_double)), maxima.shape[1]
  return _Request('hbo_mes_grad_samples', 'hbo_mes_maximize', args)


def _logei_request(target):
  """Log expected improvement, every sample against `target`: (targets[S])."""
  return _Request('hbo_logei_grad_samples', 'hbo_logei_maximize', lambda s: (_per_sample(target, s),))


def _as_request(via, acq_id, acfun_param):
  """The selector of `_fused_value_and_grad` / `_device_maximize`: a _Request, or a route (None: 'small') for the registry's pair."""
  return via if isinstance(via, _Request) else _registry_request(via or _ROUTES['small'], acq_id, acfun_param)


def _device_maximize(built, handles, noises, x0, lo, hi, acq_id, acfun_param, scale, opts, want_log, via=None):
  """The maximiser of the request `via` (`_as_request`; a _Request reads neither acq_id nor acfun_param) in segments of opts['segment']
  evaluations until no start is RUNNING or opts['max_evals'] are spent.  x0 [R, D] in the model dtype; lo / hi [D] float64 or None.
  Returns (x [R, D], values [R], status [R], evaluations [R], log or None)."""
  req = _as_request(via, acq_id, acfun_param)
  entry = getattr(nat.lib(), req.maximize)
  s_count, (r_count, d) = len(built), x0.shape
  ctx = handles[0].ctx
  structs, caches, nse = _sample_args(built, handles, noises)
  what = req.args(s_count)
  o = nat.AcqOptOpts(*[opts[k] for k in ('memory', 'ls_steps', 'max_iters', 'c1', 'tau', 'pgtol', 'ftol')])
  ns = nat.lib().hbo_acq_opt_state_doubles(d, o.memory)
  state = np.zeros((r_count, max(ns, 1)), dtype=np.float64)
  x = np.zeros((r_count, d), dtype=np.float64)
  val = np.full(r_count, np.nan)
  status = np.zeros(r_count, dtype=np.int32)
  logs, spent = [], 0
  while spent < opts['max_evals']:
    evals = int(min(opts['segment'], opts['max_evals'] - spent))
    log = np.zeros((evals, r_count), dtype=nat.ACQ_OPT_EVAL_DTYPE) if want_log else None
    ctx.check(entry(ctx.handle, structs, s_count, caches, nat.ptr(x0), r_count, nat.ptr(lo), nat.ptr(hi), *what,
                    nse, float(scale), nat.C.byref(o), nat.ptr(state), evals, nat.ptr(x), nat.ptr(val),
                    nat.ptr(status), nat.ptr(log)))
    spent += evals
    if want_log:
      logs.append(log)
    if not np.any(status == nat.ACQ_OPT_RUNNING):
      break
  n_evals = state[:, nat.ACQ_OPT_S_EVALS].astype(np.int64)
  return x, val, status, n_evals, (np.concatenate(logs) if want_log else None)


def _box_of(bounds, d):
  """(lo, hi) [d] float64 of a box given as d (lo, hi) pairs; (None, None) for None, the unit box of the entry points."""
  if bounds is None:
    return None, None
  b = np.asarray(bounds, dtype=np.float64).reshape(d, 2)
  return np.ascontiguousarray(b[:, 0]), np.ascontiguousarray(b[:, 1])


def _maximize_over_box(built, handles, noises, dtype, input_dim, x_init, bounds, scale, via, *opts):
  """What the `maximize` methods share around `_device_maximize` under the request `via`: the options (ACQ_OPT_DEFAULTS, 'segment',
  'max_evals', 'log', then the dicts `opts` in order, None skipped), the starts x_init [D] or [R, D], the box, the per-start `info` and
  the winner (x_best [D] float64, value_best, info): the largest finite value, the lowest index among equals; without any, x_init[0], NaN."""
  o = dict(ACQ_OPT_DEFAULTS, segment=ACQ_OPT_SEGMENT, max_evals=ACQ_OPT_MAX_EVALS, log=False)
  for layer in opts:
    o.update(layer or {})
  x_init = np.atleast_2d(np.asarray(x_init, dtype=np.float64))
  lo, hi = _box_of(bounds, input_dim)
  x, val, status, n_evals, log = _device_maximize(built, handles, noises, np.ascontiguousarray(x_init, dtype=dtype), lo, hi, None, None,
                                                  scale, o, bool(o['log']), via)
  info = {'x': x, 'value': val, 'status': status, 'evals': n_evals}
  if o['log']:
    info['log'] = log
  finite = np.isfinite(val)
  if not finite.any():
    return x_init[0].copy(), float('nan'), info
  best = int(np.argmax(np.where(finite, val, -np.inf)))
  return x[best].copy(), float(val[best]), info


def _fused_value_and_grad(built, handles, noises, xq, acq_id, acfun_param, scale, via=None):
  """((S, M, 1) values in the model dtype, (S, M, D) gradients in float64) of S models over their finished factors: one call of the gradient
  entry point of the request `via` (`_as_request`; by default hbo_acq_grad_samples) -- one upload, the launches, one copy back."""
  req = _as_request(via, acq_id, acfun_param)
  s_count, (nq, d) = len(built), xq.shape
  ctx = handles[0].ctx
  structs, caches, nse = _sample_args(built, handles, noises)
  out = np.empty((s_count, nq, 1), dtype=xq.dtype)
  g = np.empty((s_count, nq, d), dtype=np.float64)
  ctx.check(getattr(nat.lib(), req.grad)(ctx.handle, structs, s_count, caches, nat.ptr(xq), nq, *req.args(s_count), nse, float(scale),
                                         nat.ptr(out), g.ctypes.data_as(nat.C.POINTER(nat.C.c_double))))
  return out, g


def _hgp_value_and_grad(model, sub_dataset_key, x_queries, acq_id, acfun_param):
  """Mean over the parameter samples of (acquisition, d acquisition / d x): what jax differentiates when bayesopt() runs on an
  HGP (acfun.py:72-82 under bayesopt.py:116-125).  One hbo_acq_grad per sample against that sample's cached factor (samples
  beyond the cache budget: factorised, used and released on the spot) -- or, with the context option 'acq_fused' on and a model
  `_acq_fused_unmet` has nothing against, one hbo_acq_grad_samples call over all of them."""
  if getattr(model.cov_func, 'uses_kumar', False):   # (as hbo_acq_samples: HGP over Kumaraswamy kernels is out of scope)
    raise nat.HboError(nat.HBO_ERR_UNSUPPORTED, 'HGP acquisition over a Kumaraswamy kernel is not supported')
  samples = model.get_model_params_samples()
  has_obs = model.has_observations(sub_dataset_key)
  dtype = _model.infer_dtype(model.dataset[sub_dataset_key].x, model.dataset[sub_dataset_key].y) if has_obs \
      else _model.infer_dtype(x_queries)
  xq = np.ascontiguousarray(x_queries, dtype=dtype)
  nq = xq.shape[0]
  val = np.zeros((nq, 1), dtype=np.float64)
  grad = np.zeros((nq, model.input_dim), dtype=np.float64)
  if nq == 0:
    return val.astype(dtype), grad
  built, noises = _sample_models(model, samples, dtype)
  handles = _hgp_sample_caches(model, sub_dataset_key, samples, dtype) if has_obs else []
  _, scale = model.predict_noise_and_scale(True, True)
  route = _route_of(model)
  if _acq_fused_unmet(model, sub_dataset_key, len(samples), len(handles), max_n=route.max_n, allow_mlp=route.allow_mlp) is None:
    # option 'acq_fused': every sample's pass in ONE call over the kept factors; the mean as the loop below takes it
    outs, gs = _fused_value_and_grad(built, handles, noises, xq, acq_id, acfun_param, scale, route)
    for out, g in zip(outs, gs):
      val += out
      grad += g
    model.update_model_params(samples[-1])
    return (val / len(samples)).astype(dtype), grad / len(samples)
  out = np.empty((nq, 1), dtype=dtype)
  g = np.zeros((nq, model.input_dim), dtype=np.float64)
  with contextlib.closing(_each_sample(model, sub_dataset_key, samples, built, noises, handles)) as each:
    for _, bm, noise, h in each:
      c, cache = _ctx_and_cache(h)
      c.check(nat.lib().hbo_acq_grad(c.handle, bm.ref(), cache, nat.ptr(xq), nq, int(acq_id), float(acfun_param), float(noise), float(scale),
                                     nat.ptr(out), g.ctypes.data_as(nat.C.POINTER(nat.C.c_double))))
      val += out
      grad += g
  model.update_model_params(samples[-1])     # the side effect of the reference's loop over samples (gp.py:674-678)
  return (val / len(samples)).astype(dtype), grad / len(samples)


def acfun_wrapper(acfun_sub, acfun_callback_default):
  """acfun.py:36-93."""

  def acquisition_function(*, model, sub_dataset_key, x_queries, acfun_callback=acfun_callback_default):
    x_queries = np.asarray(x_queries)
    if isinstance(model, gp.HGP):
      acfun_param = acfun_callback(model, sub_dataset_key)
      if acfun_sub in _NATIVE_ID and model.has_observations(sub_dataset_key) and x_queries.shape[0] > 0:
        vals = hgp_sample_values(model, sub_dataset_key, x_queries, _NATIVE_ID[acfun_sub], acfun_param)
        # the reference's loop (gp.py:674-678) leaves the LAST sample in params.model and the cache dropped: same here
        model.update_model_params(model.get_model_params_samples()[-1])
        return np.mean(vals, axis=0)
      predicts = model.predict(x_queries, sub_dataset_key=sub_dataset_key, full_cov=False, with_noise=True)
      ac_vals = [acfun_sub(mu, np.sqrt(var), acfun_param) for mu, var in predicts]
      return np.mean(ac_vals, axis=0)
    acfun_param = acfun_callback(model, sub_dataset_key)
    handle, xq, bm, add_noise, scale = _single_model(model, sub_dataset_key, x_queries)
    out = np.empty((xq.shape[0], 1), dtype=xq.dtype)
    if bm is None:
      return out
    ctx, cache = _ctx_and_cache(handle)
    ctx.check(nat.lib().hbo_acq(ctx.handle, bm.ref(), cache, nat.ptr(xq), xq.shape[0], _NATIVE_ID[acfun_sub], float(acfun_param),
                                float(add_noise), float(scale), nat.ptr(out)))
    return out

  def value_and_grad(*, model, sub_dataset_key, x_queries, acfun_callback=acfun_callback_default):
    """(values (M,1), d value_q / d x_queries[q] (M,D) in float64) -- the pair jax.value_and_grad of
    `lambda x: ac_func(model=..., x_queries=x[None])` yields inside bayesopt() (bayesopt.py:116-125)."""
    x_queries = np.asarray(x_queries)
    acfun_param = acfun_callback(model, sub_dataset_key)
    if isinstance(model, gp.HGP):
      return _hgp_value_and_grad(model, sub_dataset_key, x_queries, _NATIVE_ID[acfun_sub], acfun_param)
    handle, xq, bm, add_noise, scale = _single_model(model, sub_dataset_key, x_queries)
    out = np.empty((xq.shape[0], 1), dtype=xq.dtype)
    grad = np.zeros((xq.shape[0], model.input_dim), dtype=np.float64)
    if bm is None:
      return out, grad
    route = _route_of(model)
    if _acq_fused_unmet(model, sub_dataset_key, max_n=route.max_n, allow_mlp=route.allow_mlp) is None:   # option 'acq_fused': the one-launch path with S = 1
      outs, gs = _fused_value_and_grad([bm], [handle], [add_noise], xq, _NATIVE_ID[acfun_sub], acfun_param, scale, route)
      return outs[0], gs[0]
    ctx, cache = _ctx_and_cache(handle)
    ctx.check(nat.lib().hbo_acq_grad(ctx.handle, bm.ref(), cache, nat.ptr(xq), xq.shape[0], _NATIVE_ID[acfun_sub], float(acfun_param),
                                     float(add_noise), float(scale), nat.ptr(out), grad.ctypes.data_as(nat.C.POINTER(nat.C.c_double))))
    return out, grad

  def maximize(*, model, sub_dataset_key, x_init, bounds=None, acfun_callback=acfun_callback_default, opts=None):
    """Maximises the acquisition function over a box on the device (hbo_acq_maximize: projected L-BFGS, every start in one call, no
    host round trip per evaluation).  x_init [D] or [R, D]: the starts; bounds: None ([0, 1]^D) or D (lo, hi) pairs; opts: overrides
    of ACQ_OPT_DEFAULTS, plus 'segment' (evaluations per call), 'max_evals' and 'log' (keep the per-evaluation log).
    Returns (x_best [D] float64, value_best, info): the start with the largest finite value wins, the lowest index among equals;
    without any, x_init[0] and NaN.  info: per-start 'x', 'value', 'status', 'evals', and 'log' ([evaluations, R] records) on
    request.  Works on the cached factors value_and_grad uses; a model the device loop does not cover raises
    HboError(HBO_ERR_UNSUPPORTED) -- there is no fall-back.  More than 128 observations are such a model unless
    model.params.config['acq_blocked'] is set: the calls then go to hbo_acq_maximize_blocked.  An MLP-basis kernel or a linear_mlp
    mean is such a model unless model.params.config['acq_mlp'] is set: the calls then go to hbo_acq_maximize_mlp (any number of
    observations)."""
    hgp = isinstance(model, gp.HGP)
    samples = model.get_model_params_samples() if hgp else None
    n_samples = len(samples) if hgp else 1
    route = _route_of(model)
    unmet = _acq_opt_unmet(model, sub_dataset_key, acfun_sub, n_samples, max_n=route.max_n, allow_mlp=route.allow_mlp)
    if unmet is not None:
      raise nat.HboError(nat.HBO_ERR_UNSUPPORTED, 'ac_func.maximize: ' + unmet)
    acfun_param = acfun_callback(model, sub_dataset_key)
    if hgp:
      sd = model.dataset[sub_dataset_key]
      dtype = _model.infer_dtype(sd.x, sd.y)
      built, noises = _sample_models(model, samples, dtype)
      handles = _hgp_sample_caches(model, sub_dataset_key, samples, dtype)
      unmet = _acq_opt_unmet(model, sub_dataset_key, acfun_sub, n_samples, len(handles), max_n=route.max_n, allow_mlp=route.allow_mlp)
      if unmet is not None:
        raise nat.HboError(nat.HBO_ERR_UNSUPPORTED, 'ac_func.maximize: ' + unmet)
      _, scale = model.predict_noise_and_scale(True, True)
    else:
      handle, _, bm, add_noise, scale = _single_model(model, sub_dataset_key)   # (_acq_opt_unmet: it has observations)
      dtype = handle.dtype
      built, handles, noises = [bm], [handle], [add_noise]
    best = _maximize_over_box(built, handles, noises, dtype, model.input_dim, x_init, bounds, scale,
                              _registry_request(route, _NATIVE_ID[acfun_sub], acfun_param), opts)
    if hgp:
      model.update_model_params(samples[-1])   # as every HGP path here leaves it (gp.py:674-678)
    return best

  acquisition_function.value_and_grad = value_and_grad
  acquisition_function.maximize = maximize
  return acquisition_function


def ei_callback_default(model, key, **unused_kwargs):
  if key not in model.dataset or model.dataset[key].y.shape[0] == 0:
    return 0.0
  return np.max(model.dataset[key].y)


expected_improvement = acfun_wrapper(acfun_sub=expected_improvement_sub,
                                     acfun_callback_default=ei_callback_default)
ei = expected_improvement


def pi_callback_default(model, key, zeta=0.1, use_std=False, **unused_kwargs):
  if key not in model.dataset or model.dataset[key].y.shape[0] == 0:
    return 0.0
  if use_std:
    return np.max(model.dataset[key].y) + zeta * np.std(model.dataset[key].y)
  return np.max(model.dataset[key].y) + zeta


probability_of_improvement = acfun_wrapper(acfun_sub=probability_of_improvement_sub,
                                           acfun_callback_default=pi_callback_default)
pi = probability_of_improvement
pi2 = acfun_wrapper(acfun_sub=probability_of_improvement_sub,
                    acfun_callback_default=partial(pi_callback_default, use_std=True))
pi3 = acfun_wrapper(acfun_sub=probability_of_improvement_sub,
                    acfun_callback_default=partial(pi_callback_default, zeta=0.05))

ucb4 = acfun_wrapper(acfun_sub=ucb_sub, acfun_callback_default=lambda a, b: 4.)
ucb3 = acfun_wrapper(acfun_sub=ucb_sub, acfun_callback_default=lambda a, b: 3.)
ucb2 = acfun_wrapper(acfun_sub=ucb_sub, acfun_callback_default=lambda a, b: 2.)
ucb = ucb3
rand = random_search

_BO_DEVICE.update({
    expected_improvement: (nat.ACQ_EI, nat.BO_PARAM_MAX_PLUS, 0.0),        # ei_callback_default: max y
    probability_of_improvement: (nat.ACQ_PI, nat.BO_PARAM_MAX_PLUS, 0.1),  # pi_callback_default: max y + zeta
    pi2: (nat.ACQ_PI, nat.BO_PARAM_MAX_PLUS_STD, 0.1),                     # ... + zeta * np.std(y)
    pi3: (nat.ACQ_PI, nat.BO_PARAM_MAX_PLUS, 0.05),
    ucb2: (nat.ACQ_UCB, nat.BO_PARAM_CONST, 2.0),
    ucb3: (nat.ACQ_UCB, nat.BO_PARAM_CONST, 3.0),
    ucb4: (nat.ACQ_UCB, nat.BO_PARAM_CONST, 4.0),
})


# ---- max-value entropy search (Wang & Jegelka 2017; include/hbo.h has the formulas, csrc/mes.hip the entry points) ------------------
def _plain_gp_only(model, what):
  if isinstance(model, gp.HGP):
    raise ValueError(f'{what} is defined for a GP with one set of hyper-parameters, not for an HGP')


def max_value_samples(model, sub_dataset_key, x_candidates, num_maxima=16, key=None, num_features=1024, starts=4, bounds=None, opts=None,
                      refine=True):
  """[num_maxima] float64: sampled maxima y*_k of the latent function over the box, one per posterior sample path.  One draw of
  `num_maxima` paths (GP.draw_paths) is scored at the candidates; with `refine` the `starts` best candidates of every path (stable
  order) start PathDraws.maximize and the larger of the pool maximum and the refined maximum is kept.  With observations every maximum
  is then raised to the incumbent max_i y_i: a sampled maximum below it is an artefact of the finite basis and would put gamma < 0 at
  the incumbent.  key: a numpy Generator or an int seed, None takes model.rng; bounds, opts: as PathDraws.maximize."""
  _plain_gp_only(model, 'max-value entropy search')
  xc = np.asarray(x_candidates)
  if xc.ndim != 2 or xc.shape[0] < 1:
    raise ValueError(f'x_candidates must be [M, D] with M >= 1, got {xc.shape}')
  k, r = int(num_maxima), min(int(starts), xc.shape[0])
  if k < 1 or k > nat.MES_MAX_K:
    raise ValueError(f'num_maxima must lie in 1..{nat.MES_MAX_K}, got {num_maxima}')
  if refine and r < 1:
    raise ValueError('starts must be at least 1')
  draws = model.draw_paths(sub_dataset_key, num_samples=k, num_features=num_features, key=key)
  scores = np.asarray(draws.values(xc), dtype=np.float64)                      # [M, K]
  ystar = np.max(scores, axis=0)
  if refine:
    order = np.argsort(-scores, axis=0, kind='stable')[:r]                     # [r, K]
    _, val, _ = draws.maximize(np.asarray(xc, dtype=np.float64)[order.T], bounds=bounds, opts=opts)
    val = np.asarray(val, dtype=np.float64)
    ystar = np.maximum(ystar, np.max(np.where(np.isfinite(val), val, -np.inf), axis=1))
  if model.has_observations(sub_dataset_key):
    ystar = np.maximum(ystar, float(np.max(model.dataset[sub_dataset_key].y)))
  return np.ascontiguousarray(ystar, dtype=np.float64)


class MaxValueEntropySearch:
  """Max-value entropy search: the expected reduction of the entropy of the objective's maximum, value = mean_k h(gamma_k) over K
  sampled maxima (max_value_samples).  Called, it scores a pool (hbo_acq_mes); value_and_grad and maximize go through
  hbo_mes_grad_samples and hbo_mes_maximize over the cached factor (any number of observations; without observations -- the prior
  branch -- they raise HboError(HBO_ERR_UNSUPPORTED) here, before any device call; MLP bases and input-warped kernels are refused
  by the entry points with the same error; no fall-back); `suggest` is what bayesopt.bayesopt calls.
  The variance is the latent one -- add_noise = 0 and the unbiased scale, as GP.draw_paths scales its paths -- unless with_noise."""
  __name__ = 'mes'

  def __init__(self, num_maxima=16, num_features=1024, starts=4, opts=None, with_noise=False):
    self.num_maxima, self.num_features, self.starts, self.opts, self.with_noise = num_maxima, num_features, starts, opts, bool(with_noise)

  def _setup(self, model, sub_dataset_key, x_queries=None, what=None):
    """`what`: the method that needs a cached factor -- without observations it raises, as the entry point itself would."""
    _plain_gp_only(model, 'max-value entropy search')
    if what is not None and not model.has_observations(sub_dataset_key):
      raise nat.HboError(nat.HBO_ERR_UNSUPPORTED, f'mes.{what}: the sub-dataset has no observations (the prior branch)')
    handle, xq, bm, _, _ = _single_model(model, sub_dataset_key, x_queries)
    add_noise, scale = model.predict_noise_and_scale(self.with_noise, True)
    return handle, xq, bm, add_noise, scale

  @staticmethod
  def _given(maxima):
    ystar = np.ascontiguousarray(np.asarray(maxima, dtype=np.float64).reshape(-1))
    if ystar.size < 1 or ystar.size > nat.MES_MAX_K or not np.all(np.isfinite(ystar)):
      raise ValueError(f'maxima must be 1..{nat.MES_MAX_K} finite numbers')
    return ystar

  def __call__(self, model, sub_dataset_key, x_queries, key=None, maxima=None, **unused_kwargs):
    """[M, 1] MES values in the model dtype.  maxima: [K] sampled maxima; None draws them over x_queries, unrefined, from `key`."""
    handle, xq, bm, add_noise, scale = self._setup(model, sub_dataset_key, np.asarray(x_queries))
    out = np.empty((xq.shape[0], 1), dtype=xq.dtype)
    if bm is None:
      return out
    ystar = self._given(maxima) if maxima is not None else max_value_samples(
        model, sub_dataset_key, xq, self.num_maxima, key, self.num_features, refine=False)
    ctx, cache = _ctx_and_cache(handle)
    ctx.check(nat.lib().hbo_acq_mes(ctx.handle, bm.ref(), cache, nat.ptr(xq), xq.shape[0],
                                    ystar.ctypes.data_as(nat.C.POINTER(nat.C.c_double)), ystar.size, float(add_noise), float(scale),
                                    nat.ptr(out)))
    return out

  def value_and_grad(self, *, model, sub_dataset_key, x_queries, maxima):
    """(values [M, 1] in the model dtype, d value_q / d x_queries[q] [M, D] float64) under the given maxima (hbo_mes_grad_samples)."""
    handle, xq, bm, add_noise, scale = self._setup(model, sub_dataset_key, np.asarray(x_queries), what='value_and_grad')
    if bm is None:
      return np.empty((xq.shape[0], 1), dtype=xq.dtype), np.zeros((xq.shape[0], model.input_dim))
    outs, gs = _fused_value_and_grad([bm], [handle], [add_noise], xq, None, None, scale, _mes_request(self._given(maxima)[None]))
    return outs[0], gs[0]

  def maximize(self, *, model, sub_dataset_key, x_init, maxima, bounds=None, opts=None):
    """Maximises the MES value over a box on the device (hbo_mes_maximize) from the starts x_init [D] or [R, D], under the given
    maxima.  bounds, opts and the return value (x_best [D] float64, value_best, info) are those of the `maximize` of the EI / PI / UCB
    objects: segments of ACQ_OPT_SEGMENT evaluations, the start with the largest finite value wins."""
    handle, _, bm, add_noise, scale = self._setup(model, sub_dataset_key, what='maximize')
    return _maximize_over_box([bm], [handle], [add_noise], handle.dtype, model.input_dim, x_init, bounds, scale,
                              _mes_request(self._given(maxima)[None]), self.opts, opts)

  def suggest(self, *, model, sub_dataset_key, x_candidates, key=None, batch_size=1, bounds=None):
    """[1, D] float64, the next point of bayesopt.bayesopt: refined maxima over the candidates (max_value_samples), the candidates'
    MES values, then hbo_mes_maximize from the `starts` best of them (stable order).  Without observations the best candidate is
    returned unrefined (the gradient entry points refuse the prior branch).  batch_size other than 1 raises ValueError."""
    if int(batch_size) != 1:
      raise ValueError('max-value entropy search suggests one point at a time (batch MES is not implemented)')
    _plain_gp_only(model, 'max-value entropy search')
    xc = np.asarray(x_candidates, dtype=np.float64)
    ystar = max_value_samples(model, sub_dataset_key, xc, self.num_maxima, key, self.num_features, self.starts, bounds, self.opts)
    vals = np.asarray(self(model, sub_dataset_key, xc, maxima=ystar), dtype=np.float64).reshape(-1)
    order = np.argsort(-vals, kind='stable')[:max(1, min(int(self.starts), xc.shape[0]))]
    if not model.has_observations(sub_dataset_key):
      return xc[order[:1]].copy()
    x, val, _ = self.maximize(model=model, sub_dataset_key=sub_dataset_key, x_init=xc[order], maxima=ystar, bounds=bounds)
    return (x if np.isfinite(val) else xc[order[0]])[None, :].copy()


max_value_entropy_search = mes = MaxValueEntropySearch()


# ---- log expected improvement (Ament et al. 2023; include/hbo.h has the formulas, csrc/logei.hip the entry points) ------------------
LOGEI_SERIES_U = 256.0   # csrc/kernfun.h: beyond it the asymptotic series replaces 1 + u m


def logei_terms_host(u):
  """(log h, cdf / h, pdf / h) at u, h = pdf + u cdf: the float64 restatement of csrc/kernfun.h: logei_terms (literal for u > -1,
  erfcx down to -LOGEI_SERIES_U, the asymptotic series beyond)."""
  from scipy.special import erfc, erfcx
  u = np.asarray(u, dtype=np.float64)
  logh, cdf_h, pdf_h = (np.full(u.shape, np.nan) for _ in range(3))
  with np.errstate(all='ignore'):
    hi, far = u > -1.0, u < -LOGEI_SERIES_U
    mid = ~hi & ~far & ~np.isnan(u)
    x = u[hi]
    p, c = np.exp(-0.5 * x * x) * 0.3989422804014327, 0.5 * erfc(-x * 0.7071067811865476)
    h = p + x * c
    logh[hi], cdf_h[hi], pdf_h[hi] = np.log(h), c / h, p / h
    x = u[mid]
    m = 1.2533141373155003 * erfcx(-x * 0.7071067811865476)
    w = 1.0 + x * m
    logh[mid], cdf_h[mid], pdf_h[mid] = -0.5 * x * x - 0.9189385332046727 + np.log(w), m / w, 1.0 / w
    x = u[far]
    i2 = 1.0 / (x * x)
    ws = 1.0 + i2 * (-3.0 + i2 * (15.0 - 105.0 * i2))
    ms = 1.0 + i2 * (-1.0 + i2 * (3.0 - 15.0 * i2))
    logh[far], cdf_h[far], pdf_h[far] = -0.5 * x * x - 0.9189385332046727 + (np.log(ws) - 2.0 * np.log(-x)), -x * (ms / ws), x * x / ws
  return logh, cdf_h, pdf_h


def log_expected_improvement_sub(mu, std, target):
  """log EI in the stable form, float64, for the host route: log std + log h((mu - target) / std); std <= 0: log(mu - target) above
  the target and -inf at or below it; a NaN std stays NaN."""
  mu, std = np.broadcast_arrays(np.asarray(mu, dtype=np.float64), np.asarray(std, dtype=np.float64))
  d = mu - float(target)
  with np.errstate(all='ignore'):
    flat = std <= 0.0
    safe = np.where(flat, 1.0, std)
    val = np.log(safe) + logei_terms_host(d / safe)[0]
    return np.where(flat, np.where(d > 0.0, np.log(np.where(d > 0.0, d, 1.0)), np.where(d <= 0.0, -np.inf, np.nan)), val)


def logei_combine(vals, grads=None):
  """The acquisition over S parameter samples from per-sample LogEI values [S, ...] (and gradients [S, ..., D]): the log of the MEAN
  of the samples' EI, m + log(sum_s exp(v_s - m) / S) with m = max_s v_s, and the gradient sum_s w_s g_s / sum_s w_s; float64 sums in
  sample order.  m = -inf: -inf and gradient 0; any NaN row: NaN.  S = 1: the input to the bit.  Returns value or (value, grad)."""
  v = np.asarray(vals, dtype=np.float64)
  s_count = v.shape[0]
  with np.errstate(all='ignore'):
    nan = np.isnan(v).any(axis=0)
    m = np.max(np.where(np.isnan(v), -np.inf, v), axis=0)
    dead = np.isneginf(m)
    ms = np.where(dead, 0.0, m)
    sw = np.zeros(v.shape[1:])
    for s in range(s_count):
      sw = sw + np.exp(v[s] - ms)
    val = np.where(nan, np.nan, np.where(dead, -np.inf, m + np.log(sw / s_count)))
    if grads is None:
      return val
    g = np.asarray(grads, dtype=np.float64)
    sg = np.zeros(g.shape[1:])
    for s in range(s_count):
      sg = sg + np.exp(v[s] - ms)[..., None] * g[s]
    grad = np.where(nan[..., None], np.nan, np.where(dead[..., None], 0.0, sg / np.where(dead, 1.0, sw)[..., None]))
  return val, grad


class LogExpectedImprovement:
  """Log expected improvement: log EI with EI's maximiser, finite and with a usable gradient where EI underflows.  Called, it
  scores a pool (hbo_acq_logei; an HGP: one call per sample cache, combined by logei_combine); value_and_grad and maximize go through
  hbo_logei_grad_samples and hbo_logei_maximize over the cached factors -- any number of observations, MLP bases included, no opt-in
  key.  Without observations (the prior branch) the pool values still come (GP: the device's prior branch; HGP: the host route,
  log_expected_improvement_sub), and value_and_grad and maximize raise HboError(HBO_ERR_UNSUPPORTED), as they do for input-warped
  (Kumaraswamy) kernels; no fall-back.  The target is EI's: acfun_callback, by default the largest observed y."""
  __name__ = 'log_ei'

  def _hgp_setup(self, model, sub_dataset_key, what, all_kept=True):
    """(samples, dtype, built, noises, handles, scale) of an HGP with observations; all_kept: its S factors must all fit the device
    budget (the gradient and the maximiser take them in one call)."""
    if getattr(model.cov_func, 'uses_kumar', False):
      raise nat.HboError(nat.HBO_ERR_UNSUPPORTED, f'log_ei.{what}: HGP acquisition over a Kumaraswamy kernel is not supported')
    if not model.has_observations(sub_dataset_key):
      raise nat.HboError(nat.HBO_ERR_UNSUPPORTED, f'log_ei.{what}: the sub-dataset has no observations (the prior branch)')
    samples = model.get_model_params_samples()
    sd = model.dataset[sub_dataset_key]
    dtype = _model.infer_dtype(sd.x, sd.y)
    built, noises = _sample_models(model, samples, dtype)
    handles = _hgp_sample_caches(model, sub_dataset_key, samples, dtype)
    if all_kept and len(handles) < len(samples):
      raise nat.HboError(nat.HBO_ERR_UNSUPPORTED,
                         f'log_ei.{what}: only {len(handles)} of the {len(samples)} per-sample factors fit the device budget')
    _, scale = model.predict_noise_and_scale(True, True)
    return samples, dtype, built, noises, handles, scale

  def __call__(self, *, model, sub_dataset_key, x_queries, acfun_callback=None):
    """[M, 1] LogEI values in the model dtype."""
    x_queries = np.asarray(x_queries)
    target = float((acfun_callback or ei_callback_default)(model, sub_dataset_key))
    if isinstance(model, gp.HGP):
      device = model.has_observations(sub_dataset_key) and x_queries.shape[0] > 0 and not getattr(model.cov_func, 'uses_kumar', False)
      if not device:   # the host route, as for ei: predict per sample, the stable form in NumPy, the combination
        predicts = model.predict(x_queries, sub_dataset_key=sub_dataset_key, full_cov=False, with_noise=True)
        vals = [log_expected_improvement_sub(mu, np.sqrt(var), target) for mu, var in predicts]
        return logei_combine(vals).astype(np.asarray(predicts[0][0]).dtype)
      samples, dtype, built, noises, handles, scale = self._hgp_setup(model, sub_dataset_key, '__call__', all_kept=False)
      xq = np.ascontiguousarray(x_queries, dtype=dtype)
      outs = np.empty((len(samples), xq.shape[0], 1), dtype=dtype)
      # (samples beyond the cache budget: factorised, used and released on the spot, as for ei's gradient)
      with contextlib.closing(_each_sample(model, sub_dataset_key, samples, built, noises, handles)) as each:
        for i, bm, noise, h in each:
          h.ctx.check(nat.lib().hbo_acq_logei(h.ctx.handle, bm.ref(), h.handle, nat.ptr(xq), xq.shape[0], target, float(noise), float(scale),
                                              nat.ptr(outs[i])))
      model.update_model_params(samples[-1])   # as every HGP path here leaves it (gp.py:674-678)
      return logei_combine(outs).astype(dtype)
    handle, xq, bm, add_noise, scale = _single_model(model, sub_dataset_key, x_queries)
    out = np.empty((xq.shape[0], 1), dtype=xq.dtype)
    if bm is None:
      return out
    ctx, cache = _ctx_and_cache(handle)
    ctx.check(nat.lib().hbo_acq_logei(ctx.handle, bm.ref(), cache, nat.ptr(xq), xq.shape[0], target, float(add_noise), float(scale), nat.ptr(out)))
    return out

  def _setup(self, model, sub_dataset_key, what, x_queries=None):
    """(dtype, built, noises, handles, scale, x_queries in the model dtype, samples or None) for the gradient entry points."""
    if isinstance(model, gp.HGP):
      samples, dtype, built, noises, handles, scale = self._hgp_setup(model, sub_dataset_key, what)
      xq = None if x_queries is None else np.ascontiguousarray(x_queries, dtype=dtype)
      return dtype, built, noises, handles, scale, xq, samples
    if not model.has_observations(sub_dataset_key):
      raise nat.HboError(nat.HBO_ERR_UNSUPPORTED, f'log_ei.{what}: the sub-dataset has no observations (the prior branch)')
    handle, xq, bm, add_noise, scale = _single_model(model, sub_dataset_key, x_queries)
    return handle.dtype, [bm], [add_noise], [handle], scale, xq, None

  def value_and_grad(self, *, model, sub_dataset_key, x_queries, acfun_callback=None):
    """(values [M, 1] in the model dtype, d value_q / d x_queries[q] [M, D] float64): hbo_logei_grad_samples, an HGP's per-sample rows
    combined by logei_combine."""
    target = float((acfun_callback or ei_callback_default)(model, sub_dataset_key))
    dtype, built, noises, handles, scale, xq, samples = self._setup(model, sub_dataset_key, 'value_and_grad', np.asarray(x_queries))
    if xq.shape[0] == 0:
      return np.empty((0, 1), dtype=dtype), np.zeros((0, model.input_dim))
    outs, gs = _fused_value_and_grad(built, handles, noises, xq, None, None, scale, _logei_request(target))
    if samples is None:
      return outs[0], gs[0]
    model.update_model_params(samples[-1])
    val, grad = logei_combine(outs[:, :, 0], gs)
    return val[:, None].astype(dtype), grad

  def maximize(self, *, model, sub_dataset_key, x_init, bounds=None, acfun_callback=None, opts=None):
    """Maximises LogEI over a box on the device (hbo_logei_maximize) from the starts x_init [D] or [R, D].  bounds, opts and the return
    value (x_best [D] float64, value_best, info) are those of the `maximize` of the EI / PI / UCB objects."""
    target = float((acfun_callback or ei_callback_default)(model, sub_dataset_key))
    dtype, built, noises, handles, scale, _, samples = self._setup(model, sub_dataset_key, 'maximize')
    best = _maximize_over_box(built, handles, noises, dtype, model.input_dim, x_init, bounds, scale, _logei_request(target), opts)
    if samples is not None:
      model.update_model_params(samples[-1])
    return best


log_expected_improvement = log_ei = LogExpectedImprovement()


# ---- batch (q-point) expected improvement (Ginsbourger et al. 2010; Wilson et al. 2018; include/hbo.h has the formulas, csrc/qei.hip
#      the kernel and the entry points) -----------------------------------------------------------------------------------------------
def _generator(model, key):
  """A numpy Generator from `key`: a Generator itself, an int seed, or None -- model.rng, or seed 0 without one."""
  if isinstance(key, np.random.Generator):
    return key
  if key is None:
    return model.rng if getattr(model, 'rng', None) is not None else np.random.default_rng(0)
  return np.random.default_rng(key)


def _qei_checked(ctx, rc):
  """ctx.check, with a refusal of the entry point (HBO_ERR_UNSUPPORTED, HBO_ERR_ARG) as ValueError under the entry point's message."""
  try:
    return ctx.check(rc)
  except nat.HboError as e:
    if e.code in (nat.HBO_ERR_UNSUPPORTED, nat.HBO_ERR_ARG):
      raise ValueError(str(e)) from e
    raise


class BatchExpectedImprovement:
  """Joint expected improvement of q points evaluated together, qEI(x_1..x_q) = E[max(0, max_j f(x_j) - t)], as the average over
  `num_base` fixed base samples of the reparameterised posterior draw (include/hbo.h).  Called, it scores batches [M, q, D]
  (hbo_qei_grad_samples; an HGP: the mean over its parameter samples); value_and_grad adds the exact gradient of that average with
  respect to every coordinate of every point; maximize refines starting batches over a box on the device (hbo_qei_maximize); `suggest`
  proposes `batch_size` points from a pool of candidates and is what bayesopt.bayesopt_batch calls.  The device route serves caches of
  up to 128 observations without MLP bases or Kumaraswamy warps; a model it refuses raises ValueError with the entry point's message --
  there is no fall-back.  The target is EI's: acfun_callback, by default the largest observed y."""
  __name__ = 'q_expected_improvement'

  def __init__(self, num_base=256, starts=8, opts=None):
    if not 1 <= int(num_base) <= nat.QEI_MAX_BASE:
      raise ValueError(f'num_base must lie in 1..{nat.QEI_MAX_BASE}, got {num_base}')
    self.num_base, self.starts, self.opts = int(num_base), int(starts), opts

  def base_samples(self, q, key=None):
    """[num_base, q] float64 standard normals from a numpy Generator (`key`: a Generator or an int seed; None: seed 0)."""
    rng = key if isinstance(key, np.random.Generator) else np.random.default_rng(0 if key is None else key)
    return np.ascontiguousarray(rng.standard_normal((self.num_base, int(q))), dtype=np.float64)

  @staticmethod
  def _base(base_samples, q):
    z = np.ascontiguousarray(base_samples, dtype=np.float64)
    if z.ndim != 2 or z.shape[1] != q or not 1 <= z.shape[0] <= nat.QEI_MAX_BASE:
      raise ValueError(f'base_samples must be [B, {q}] with 1 <= B <= {nat.QEI_MAX_BASE}, got {z.shape}')
    return z

  def _setup(self, model, sub_dataset_key, what):
    """(dtype, built, noises, handles, scale, samples or None): the per-sample models and finished factors of the call."""
    if not model.has_observations(sub_dataset_key):
      raise ValueError(f'q_expected_improvement.{what}: the sub-dataset has no observations (the prior branch)')
    if isinstance(model, gp.HGP):
      samples = model.get_model_params_samples()
      sd = model.dataset[sub_dataset_key]
      dtype = _model.infer_dtype(sd.x, sd.y)
      built, noises = _sample_models(model, samples, dtype)
      handles = _hgp_sample_caches(model, sub_dataset_key, samples, dtype)
      if len(handles) < len(samples):
        raise ValueError(f'q_expected_improvement.{what}: only {len(handles)} of the {len(samples)} per-sample factors fit the device budget')
      _, scale = model.predict_noise_and_scale(True, True)
      return dtype, built, noises, handles, scale, samples
    handle, _, bm, add_noise, scale = _single_model(model, sub_dataset_key)
    return handle.dtype, [bm], [add_noise], [handle], scale, None

  def _batches(self, x_batches, dtype, input_dim):
    xb = np.asarray(x_batches)
    if xb.ndim != 3 or xb.shape[2] != input_dim or not 1 <= xb.shape[1] <= nat.QEI_MAX_Q:
      raise ValueError(f'batches must be [M, q, {input_dim}] with 1 <= q <= {nat.QEI_MAX_Q}, got {xb.shape}')
    return np.ascontiguousarray(xb, dtype=dtype)

  def value_and_grad(self, *, model, sub_dataset_key, x_batches, base_samples, acfun_callback=None):
    """(values [M, 1] float64, d value_m / d x_batches[m] [M, q, D] float64): the mean over the parameter samples of
    hbo_qei_grad_samples' rows."""
    target = float((acfun_callback or ei_callback_default)(model, sub_dataset_key))
    dtype, built, noises, handles, scale, samples = self._setup(model, sub_dataset_key, 'value_and_grad')
    xb = self._batches(x_batches, dtype, model.input_dim)
    m_count, q, d = xb.shape
    z = self._base(base_samples, q)
    s_count = len(built)
    ctx = handles[0].ctx
    structs, caches, nse = _sample_args(built, handles, noises)
    vals = np.empty((s_count, m_count), dtype=np.float64)
    grads = np.empty((s_count, m_count, q, d), dtype=np.float64)
    dp = nat.C.POINTER(nat.C.c_double)
    _qei_checked(ctx, nat.lib().hbo_qei_grad_samples(ctx.handle, structs, s_count, caches, nat.ptr(xb), m_count, q, z.ctypes.data_as(dp),
                                                     z.shape[0], _per_sample(target, s_count), nse, float(scale), vals.ctypes.data_as(dp),
                                                     grads.ctypes.data_as(dp)))
    if samples is not None:
      model.update_model_params(samples[-1])   # as every HGP path here leaves it (gp.py:674-678)
    val, grad = np.zeros(m_count), np.zeros((m_count, q, d))
    for s in range(s_count):   # sample order, as the control kernel sums
      val = val + vals[s]
      grad = grad + grads[s]
    return (val / s_count)[:, None], grad / s_count

  def __call__(self, *, model, sub_dataset_key, x_batches, base_samples, acfun_callback=None):
    """[M, 1] float64: qEI of every batch, the mean over an HGP's parameter samples."""
    return self.value_and_grad(model=model, sub_dataset_key=sub_dataset_key, x_batches=x_batches, base_samples=base_samples,
                               acfun_callback=acfun_callback)[0]

  def maximize(self, *, model, sub_dataset_key, x_init, base_samples, bounds=None, opts=None, acfun_callback=None):
    """Maximises qEI over the box on the device (hbo_qei_maximize) from the starting batches x_init [q, D] or [R, q, D], all in one
    call per segment of opts['segment'] evaluations until no start is RUNNING or opts['max_evals'] are spent.  bounds: None ([0, 1]^D)
    or D (lo, hi) pairs; opts: as the `maximize` of the EI / PI / UCB objects.  Returns (x_best [q, D] float64, value_best, info): the
    start with the largest finite value, the lowest index among equals; without any, x_init[0] and NaN."""
    target = float((acfun_callback or ei_callback_default)(model, sub_dataset_key))
    dtype, built, noises, handles, scale, samples = self._setup(model, sub_dataset_key, 'maximize')
    o = dict(ACQ_OPT_DEFAULTS, segment=ACQ_OPT_SEGMENT, max_evals=ACQ_OPT_MAX_EVALS, log=False)
    for layer in (self.opts, opts):
      o.update(layer or {})
    x_init = np.asarray(x_init, dtype=np.float64)
    x0 = self._batches(x_init[None] if x_init.ndim == 2 else x_init, dtype, model.input_dim)
    r_count, q, d = x0.shape
    z = self._base(base_samples, q)
    lo, hi = _box_of(bounds, d)
    s_count = len(built)
    ctx = handles[0].ctx
    structs, caches, nse = _sample_args(built, handles, noises)
    oo = nat.AcqOptOpts(*[o[k] for k in ('memory', 'ls_steps', 'max_iters', 'c1', 'tau', 'pgtol', 'ftol')])
    ns = nat.lib().hbo_acq_opt_state_doubles(q * d, oo.memory)
    state = np.zeros((r_count, max(ns, 1)), dtype=np.float64)
    x = np.zeros((r_count, q, d), dtype=np.float64)
    val = np.full(r_count, np.nan)
    status = np.zeros(r_count, dtype=np.int32)
    dp = nat.C.POINTER(nat.C.c_double)
    targets = _per_sample(target, s_count)
    logs, spent = [], 0
    while spent < o['max_evals']:
      evals = int(min(o['segment'], o['max_evals'] - spent))
      log = np.zeros((evals, r_count), dtype=nat.ACQ_OPT_EVAL_DTYPE) if o['log'] else None
      _qei_checked(ctx, nat.lib().hbo_qei_maximize(ctx.handle, structs, s_count, caches, nat.ptr(x0), r_count, q, nat.ptr(lo), nat.ptr(hi),
                                                   z.ctypes.data_as(dp), z.shape[0], targets, nse, float(scale), nat.C.byref(oo),
                                                   nat.ptr(state), evals, nat.ptr(x), nat.ptr(val), nat.ptr(status), nat.ptr(log)))
      spent += evals
      if o['log']:
        logs.append(log)
      if not np.any(status == nat.ACQ_OPT_RUNNING):
        break
    if samples is not None:
      model.update_model_params(samples[-1])
    info = {'x': x, 'value': val, 'status': status, 'evals': state[:, nat.ACQ_OPT_S_EVALS].astype(np.int64)}
    if o['log']:
      info['log'] = np.concatenate(logs)
    finite = np.isfinite(val)
    if not finite.any():
      return np.asarray(x0[0], dtype=np.float64).copy(), float('nan'), info
    best = int(np.argmax(np.where(finite, val, -np.inf)))
    return x[best].copy(), float(val[best]), info

  def suggest(self, *, model, sub_dataset_key, x_candidates, key=None, batch_size=1, bounds=None):
    """[batch_size, D] float64: the candidates are scored with EI over the pool; start 0 is the `batch_size` best of them (stable
    order), every further start `batch_size` distinct candidates drawn by the Generator from the best 4 * batch_size * starts; all
    starts are refined in one hbo_qei_maximize call under base samples drawn from the same Generator, and the best final batch is
    returned.  Without observations (the prior branch): `batch_size` distinct candidates drawn by the Generator.  Deterministic given
    `key` (a numpy Generator or an int seed; None takes model.rng, or seed 0 without one)."""
    xc = np.asarray(x_candidates, dtype=np.float64)
    q = int(batch_size)
    if xc.ndim != 2 or not 1 <= q <= min(nat.QEI_MAX_Q, xc.shape[0]):
      raise ValueError(f'x_candidates must be [M, D] and 1 <= batch_size <= min({nat.QEI_MAX_Q}, M), got {xc.shape} and {batch_size}')
    rng = _generator(model, key)
    if not model.has_observations(sub_dataset_key):
      return xc[rng.choice(xc.shape[0], size=q, replace=False)].copy()
    scores = np.asarray(expected_improvement(model=model, sub_dataset_key=sub_dataset_key, x_queries=xc), dtype=np.float64).reshape(-1)
    order = np.argsort(-np.where(np.isnan(scores), -np.inf, scores), kind='stable')
    pool = order[:min(xc.shape[0], 4 * q * max(1, self.starts))]
    starts = [xc[order[:q]]] + [xc[rng.choice(pool, size=q, replace=False)] for _ in range(max(1, self.starts) - 1)]
    z = self.base_samples(q, rng)
    x, val, _ = self.maximize(model=model, sub_dataset_key=sub_dataset_key, x_init=np.stack(starts), base_samples=z, bounds=bounds)
    return (x if np.isfinite(val) else starts[0]).copy()


q_expected_improvement = BatchExpectedImprovement()
