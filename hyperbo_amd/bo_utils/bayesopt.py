"""BO loops over the native posterior -- hyperbo/bo_utils/bayesopt.py:32-190.

Host control flow only: the per-iteration work -- cache append / re-factorisation,
acquisition over the candidate set, and d acquisition / d x for the continuous variant -- runs on the GPU.
`key` arguments are NumPy Generators or seeds (no JAX PRNG here).
"""
import logging
import time

import numpy as np
import scipy.optimize

from hyperbo_amd.basics import definitions as defs
from hyperbo_amd.gp_utils import objectives as obj

SubDataset = defs.SubDataset


def _rng(key):
  return key if isinstance(key, np.random.Generator) else np.random.default_rng(0 if key is None else key)


def get_best_datapoint(sub_dataset):
  """bayesopt.py:32-39."""
  if sub_dataset.y.shape[0] == 0:
    return None
  best_idx = int(np.argmax(sub_dataset.y))
  return sub_dataset.x[best_idx], sub_dataset.y[best_idx]


def retrain_model(model, sub_dataset_key, random_key=None, get_params_path=None, callback=None):
  """bayesopt.py:42-72: optional re-training once the test sub-dataset has observations."""
  cfg = model.params.config
  retrain_condition = ('retrain' in cfg and cfg['retrain'] > 0 and sub_dataset_key in model.dataset
                       and model.dataset[sub_dataset_key].x.shape[0] > 0)
  if not retrain_condition:
    return
  if cfg['objective'] in [obj.regkl, obj.regeuc]:
    raise ValueError('Objective must include NLL to retrain.')
  cfg['max_training_step'] = cfg['retrain']
  model.train(random_key, get_params_path=get_params_path, callback=callback)


def bayesopt(key, model, sub_dataset_key, query_oracle, ac_func, iters, input_sampler):
  """bayesopt.py:75-133: continuous BO on [0,1]^D -- pick the best of `input_sampler`'s candidates, then
  L-BFGS-B on -ac_func from there (SciPy's, the one jaxopt.ScipyBoundedMinimize wraps) with the native
  `ac_func.value_and_grad`, query the oracle, append.

  With config['acq_opt_on_device'] set, the SciPy call is replaced by `ac_func.maximize` (hbo_acq_maximize: the optimiser itself on
  the device) from the config['acq_opt_starts'] (default 1) best candidates -- ordered by acquisition value, the lower index first
  among equals -- once the sub-dataset has observations; an iteration without any (the prior branch) takes the SciPy path.  There is
  no fall-back: the iteration at which the sub-dataset has grown past 128 observations raises HboError(HBO_ERR_UNSUPPORTED).
  With config['acq_blocked'] set as well, `ac_func.maximize` calls hbo_acq_maximize_blocked and the loop continues on the device
  past 128 observations (below them the two are the same launches and the same bits).  A model on the MLP basis (`*_mlp` kernels,
  the linear_mlp mean) raises as well unless config['acq_mlp'] is set: `ac_func.maximize` then calls hbo_acq_maximize_mlp, at any
  number of observations.

  An `ac_func` with a `suggest` attribute (acfun.thompson_continuous) proposes the point itself: x_opt is
  `ac_func.suggest(model=, sub_dataset_key=, x_candidates=, key=)[0]` over the iteration's candidates and this loop's Generator."""
  rng = _rng(key)
  input_dim = model.input_dim
  cfg = model.params.config or {}
  on_device = bool(cfg.get('acq_opt_on_device'))
  bounds = [(0.0, 1.0)] * input_dim
  for i in range(iters):
    start_time = time.time()
    retrain_model(model, sub_dataset_key=sub_dataset_key, random_key=rng)
    x_samples = np.asarray(input_sampler(rng, input_dim))
    suggest = getattr(ac_func, 'suggest', None)
    if suggest is not None:
      select_idx = 0   # (the strategy scores the candidates itself)
    elif ac_func.__name__ in ('rand', 'random_search'):
      select_idx = int(rng.integers(x_samples.shape[0]))
    else:
      evals = ac_func(model=model, sub_dataset_key=sub_dataset_key, x_queries=x_samples)
      select_idx = int(np.argmax(evals))
    x_init = np.asarray(x_samples[select_idx], dtype=np.float64)
    if suggest is not None:
      # a strategy that proposes points itself (acfun.thompson_continuous: the maximiser of a posterior sample path, refined on the
      # device from the best candidates), with or without observations
      x_opt = np.asarray(suggest(model=model, sub_dataset_key=sub_dataset_key, x_candidates=x_samples, key=rng)[0], dtype=np.float64)
    elif ac_func.__name__ in ('rand', 'random_search') or not (hasattr(ac_func, 'value_and_grad') or hasattr(ac_func, 'maximize')):
      x_opt = x_init   # (neither a gradient nor a maximiser to refine with, e.g. thompson_sampling: the best candidate stays as it is)
    elif on_device and model.has_observations(sub_dataset_key):
      starts = np.argsort(-np.asarray(evals, dtype=np.float64).reshape(-1), kind='stable')[:max(1, int(cfg.get('acq_opt_starts', 1)))]
      x_opt, _, _ = ac_func.maximize(model=model, sub_dataset_key=sub_dataset_key, x_init=x_samples[starts])
    else:
      def neg_acq(x):
        val, grad = ac_func.value_and_grad(model=model, sub_dataset_key=sub_dataset_key, x_queries=x[None, :])
        return -float(val[0, 0]), -grad[0]
      res = scipy.optimize.minimize(neg_acq, x_init, jac=True, method='L-BFGS-B', bounds=bounds)
      x_opt = np.asarray(res.x, dtype=np.float64)
    eval_datapoint = x_opt, np.asarray(query_oracle(x_opt[None, :])).reshape(-1)
    logging.info('%d-th iter, x_init=%s, eval_datapoint=%s, elapsed_time=%s', i, x_init, eval_datapoint,
                 time.time() - start_time)
    model.update_sub_dataset(eval_datapoint, sub_dataset_key=sub_dataset_key, is_append=True)
  return model.dataset.get(sub_dataset_key, SubDataset(np.empty(0), np.empty(0)))


def bayesopt_batch(model, sub_dataset_key, queried_sub_dataset, ac_func, iters, batch_size, input_sampler, key=None):
  """Continuous BO on [0,1]^D with `batch_size` points per iteration, for evaluation on parallel workers: every iteration takes
  `ac_func.suggest(model=, sub_dataset_key=, x_candidates=, key=, batch_size=)` [batch_size, D] over `input_sampler`'s candidates and
  this loop's Generator, queries the oracle `queried_sub_dataset` (a callable on [batch_size, D]) once for the whole batch and appends
  the batch_size observations.  `ac_func` needs a `suggest` that takes batch_size: acfun.q_expected_improvement (the joint criterion,
  refined on the device) or acfun.thompson_continuous (independent posterior paths).  Returns the sub-dataset after iters * batch_size
  appended observations."""
  suggest = getattr(ac_func, 'suggest', None)
  if suggest is None:
    raise ValueError('bayesopt_batch needs an ac_func with a `suggest` method (acfun.q_expected_improvement, acfun.thompson_continuous)')
  q = int(batch_size)
  if q < 1:
    raise ValueError('batch_size must be at least 1')
  rng = _rng(key)
  input_dim = model.input_dim
  for i in range(iters):
    start_time = time.time()
    retrain_model(model, sub_dataset_key=sub_dataset_key, random_key=rng)
    x_samples = np.asarray(input_sampler(rng, input_dim))
    x_batch = np.asarray(suggest(model=model, sub_dataset_key=sub_dataset_key, x_candidates=x_samples, key=rng, batch_size=q),
                         dtype=np.float64).reshape(q, input_dim)
    y_batch = np.asarray(queried_sub_dataset(x_batch)).reshape(q, -1)
    logging.info('%d-th iter, batch=%s, values=%s, elapsed_time=%s', i, x_batch, y_batch, time.time() - start_time)
    model.update_sub_dataset((x_batch, y_batch), sub_dataset_key=sub_dataset_key, is_append=True)
  return model.dataset.get(sub_dataset_key, SubDataset(np.empty(0), np.empty(0)))


def _bo_on_device_unmet(model, sub_dataset_key, queried_sub_dataset, ac_func):
  """The first condition that keeps a simulated BO loop off the device loop (hbo_bo_simulated, config['bo_on_device']), as a
  message, or None.  Host-side checks only."""
  from hyperbo_amd.bo_utils import acfun
  from hyperbo_amd.gp_utils import gp
  if isinstance(model, gp.HGP):
    return 'the model is an HGP (the acquisition is a mean over parameter samples)'
  if (model.params.config or {}).get('retrain', 0) > 0:
    return "config['retrain'] > 0 re-trains the model between iterations"
  if getattr(ac_func, '__name__', '') in ('rand', 'random_search'):
    return 'random search draws its selections on the host'
  if ac_func is acfun.log_ei:
    return "log_ei is outside the device loop's registry (hbo_bo_simulated scores with EI, PI or UCB)"
  if ac_func not in acfun._BO_DEVICE:
    return f'ac_func {ac_func!r} is not one of the native acquisition functions of bo_utils/acfun.py'
  if getattr(model.cov_func, 'uses_kumar', False):
    return 'the kernel is input-warped (Kumaraswamy)'
  ys = [np.asarray(queried_sub_dataset.y)]
  if sub_dataset_key in model.dataset:
    ys.append(np.asarray(model.dataset[sub_dataset_key].y))
  if any(y.ndim > 1 and y.shape[1] > 1 for y in ys):
    return 'y has more than one column'
  if np.shape(queried_sub_dataset.x)[0] == 0:
    return 'the candidate pool is empty'
  return None


def _bo_scales(model, sub_dataset_key):
  """(add_noise, scale of iteration 0, scale of the later ones) -- gp.py:607-619.  The first append creates a sub-dataset whose
  key is not in model.dataset yet, and the unbiased T / (T - 1) then counts one more."""
  add_noise, scale0 = model.predict_noise_and_scale(True, True)
  if sub_dataset_key in model.dataset:
    return add_noise, scale0, scale0
  count = len([k for k, v in model.dataset.items() if v.aligned is None]) + 1
  return add_noise, scale0, (count / (count - 1.) if count > 1 else 1.0)


def simulated_bayesopt_batch(runs, iters):
  """simulated_bayesopt for a sequence of (model, sub_dataset_key, queried_sub_dataset, ac_func) as ONE hbo_bo_simulated call: every
  iteration of every run on the device (csrc/bo_loop.hip), one synchronisation.  The models must share a family
  (dtype, covariance, mean, input_dim, MLP architecture).  Afterwards every selection is appended to its model's sub-dataset
  (update_sub_dataset, as the host loop does); returns the list of resulting SubDatasets."""
  from hyperbo_amd import _model
  from hyperbo_amd import _native as nat
  from hyperbo_amd.bo_utils import acfun
  runs = list(runs)
  empty = SubDataset(np.empty(0), np.empty(0))
  if iters <= 0 or not runs:
    return [model.dataset.get(key, empty) for model, key, _, _ in runs]
  built, structs, keep, family = [], [], [], None
  for model, key, pool, ac_func in runs:
    unmet = _bo_on_device_unmet(model, key, pool, ac_func)
    if unmet is not None:
      raise ValueError('bo_on_device: ' + unmet)
    has_obs = model.has_observations(key)
    sd = model.dataset[key] if has_obs else None
    dtype = _model.infer_dtype(pool.x, pool.y, *((sd.x, sd.y) if has_obs else ()))
    bm = _model.BuiltModel(model.mean_func, model.cov_func, model.params, model.warp_func, dtype, model.input_dim)
    fam = (bm.code, bm.kernel_id, bm.mean_id, model.input_dim, bm.uses_mlp_kernel, bm.struct.n_lengthscale, tuple(bm.mlp_shapes))
    if family is None:
      family = fam
    elif fam != family:
      raise ValueError('bo_on_device: the runs of one batch must share dtype, covariance, mean, input_dim and MLP architecture')
    d = model.input_dim
    xc = np.ascontiguousarray(np.asarray(pool.x).reshape(-1, d), dtype=dtype)
    yc = np.ascontiguousarray(np.asarray(pool.y).reshape(-1), dtype=dtype)
    x0 = np.ascontiguousarray(np.asarray(sd.x).reshape(-1, d), dtype=dtype) if has_obs else None
    y0 = np.ascontiguousarray(np.asarray(sd.y).reshape(-1), dtype=dtype) if has_obs else None
    acq_id, mode, param = acfun._BO_DEVICE[ac_func]
    add_noise, scale0, scale = _bo_scales(model, key)
    structs.append(nat.BoRun(nat.ptr(xc), nat.ptr(yc), xc.shape[0], nat.ptr(x0), nat.ptr(y0), 0 if x0 is None else x0.shape[0],
                             acq_id, mode, param, add_noise, scale0, scale))
    built.append(bm)
    keep.append((xc, yc, x0, y0))
  count = len(runs)
  sel = np.zeros((count, iters), dtype=np.int32)
  acq = np.zeros((count, iters), dtype=np.float64)
  status = np.zeros(count, dtype=np.int32)
  ctx = nat.default_context()
  # (a run whose appended rows made the matrix numerically indefinite, status HBO_NOT_PD: its later selections are index 0 -- what
  #  the host loop's np.argmax returns over the NaN values of a cache that failed to factorise; the rows are appended all the same)
  ctx.check(nat.lib().hbo_bo_simulated(ctx.handle, (nat.Model * count)(*[b.struct for b in built]), (nat.BoRun * count)(*structs), count,
                                       int(iters), sel.ctypes.data_as(nat.C.POINTER(nat.C.c_int32)),
                                       acq.ctypes.data_as(nat.C.POINTER(nat.C.c_double)), None, None,
                                       status.ctypes.data_as(nat.C.POINTER(nat.C.c_int32))))
  out = []
  for (model, key, pool, _), row in zip(runs, sel):
    for idx in row:
      model.update_sub_dataset((pool.x[idx], pool.y[idx]), sub_dataset_key=key, is_append=True)
    out.append(model.dataset.get(key, empty))
  return out


def simulated_bayesopt(model, sub_dataset_key, queried_sub_dataset, ac_func, iters, random_key=None,
                       get_params_path=None, callback=None):
  """bayesopt.py:136-190: BO restricted to a set of pre-evaluated candidates.  With config['bo_on_device'] set the whole loop runs
  on the device (simulated_bayesopt_batch with one run); a model or acquisition function it does not cover raises ValueError."""
  if (model.params.config or {}).get('bo_on_device'):
    return simulated_bayesopt_batch([(model, sub_dataset_key, queried_sub_dataset, ac_func)], iters)[0]
  rng = None if random_key is None else _rng(random_key)
  for _ in range(iters):
    retrain_model(model, sub_dataset_key=sub_dataset_key, random_key=rng, get_params_path=get_params_path,
                  callback=callback)
    if ac_func.__name__ in ('rand', 'random_search'):
      if rng is None:
        raise ValueError('Must specify a random key for random search.')
      select_idx = int(rng.integers(queried_sub_dataset.x.shape[0]))
    else:
      evals = ac_func(model=model, sub_dataset_key=sub_dataset_key, x_queries=queried_sub_dataset.x)
      select_idx = int(np.argmax(evals))
    eval_datapoint = queried_sub_dataset.x[select_idx], queried_sub_dataset.y[select_idx]
    model.update_sub_dataset(eval_datapoint, sub_dataset_key=sub_dataset_key, is_append=True)
  return model.dataset.get(sub_dataset_key, SubDataset(np.empty(0), np.empty(0)))


def run_bayesopt(dataset, sub_dataset_key, queried_sub_dataset, mean_func, cov_func, init_params, ac_func, iters,
                 warp_func=None, init_random_key=None, method='hyperbo', init_model=False, data_loader_name='',
                 get_params_path=None, callback=None, save_retrain_model=False):
  """bayesopt.py:193-302: build the model, optionally initialise + pre-train it, then run the simulated loop on a
  candidate SubDataset or the continuous loop on a query oracle.  Returns ((x, y) of the test sub-dataset after BO,
  the best candidate (x, y) or None, the model's params)."""
  from hyperbo_amd.bo_utils import const
  from hyperbo_amd.gp_utils import gp
  if method in const.USE_HGP:
    raise NotImplementedError('hierarchical GP (slice sampling over hyper-parameters) is outside the native path')
  model = gp.GP(dataset=dataset, mean_func=mean_func, cov_func=cov_func, params=init_params, warp_func=warp_func)
  rng = _rng(init_random_key)
  if init_model:
    assert init_random_key is not None, 'Cannot initialize with init_random_key == None.'
    model.initialize_params(rng)
    model.train(rng, get_params_path, callback=callback)
  else:
    model.rng = rng
  if isinstance(queried_sub_dataset, SubDataset):
    best_query = get_best_datapoint(queried_sub_dataset)
    sub = simulated_bayesopt(model=model, sub_dataset_key=sub_dataset_key, queried_sub_dataset=queried_sub_dataset,
                             ac_func=ac_func, iters=iters, random_key=rng,
                             get_params_path=get_params_path if save_retrain_model else None,
                             callback=callback if save_retrain_model else None)
    return (sub.x, sub.y), best_query, model.params
  if data_loader_name not in const.INPUT_SAMPLERS:
    raise NotImplementedError(f'Input sampler for {data_loader_name} not found.')
  sub = bayesopt(key=rng, model=model, sub_dataset_key=sub_dataset_key, query_oracle=queried_sub_dataset,
                 ac_func=ac_func, iters=iters, input_sampler=const.INPUT_SAMPLERS[data_loader_name])
  return (sub.x, sub.y), None, model.params
