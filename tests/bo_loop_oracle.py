"""Oracle side of the device BO loop's tests.

oracle_loop: the reference's simulated loop (hyperbo/bo_utils/bayesopt.py:136-190) on the oracle -- every iteration calls o.predict
from scratch, gp_predict_postprocess, the oracle's *_sub epilogue and default callback, np.argmax, and appends.  Optionally driven
along given selections (the replay check).
recurrence_loop: a NumPy restatement of what csrc/bo_loop.hip computes -- V = L^-1 K(X_obs, C) carried row by row -- with the
oracle's kernel and mean functions; test_bo_device_host.py holds it to oracle_loop."""
import collections

import numpy as np

import bo_device_cases as cases
from oracle import hyperbo_oracle as o

KEY, WFO = cases.KEY, cases.WFO
Loop = collections.namedtuple('Loop', 'sel acq vals mu var')   # selections, their values, all values per iteration, final mu / var at the pool


def oracle_loop(w, selections=None):
  case = w.case
  mean_func, cov_func = cases.oracle_funcs(case)
  sub, callback, _ = cases.ACQS[case.acq]
  params = cases.oracle_params(w)
  dataset = cases.oracle_dataset(w)
  pool_x, pool_y = np.asarray(w.pool_x, dtype=np.float64), np.asarray(w.pool_y, dtype=np.float64)

  def observed():
    if KEY in dataset and dataset[KEY].x.shape[0] > 0:
      return dataset[KEY].x, dataset[KEY].y
    return None, None

  sel, acq, vals_all = [], [], []
  for i in range(case.iters):
    x_obs, y_obs = observed()
    with np.errstate(all='ignore'):
      mu, var = o.predict(mean_func, cov_func, params, x_obs, y_obs, pool_x, WFO)
      mu, var = o.gp_predict_postprocess(params, dataset, mu, var, WFO, False, True, True)
      vals = np.asarray(sub(mu, np.sqrt(var), callback(dataset, KEY))).reshape(-1)
    idx = int(np.argmax(vals)) if selections is None else int(selections[i])
    sel.append(idx); acq.append(vals[idx]); vals_all.append(vals)
    if KEY not in dataset:
      dataset[KEY] = o.SubDataset(np.empty((0, case.D)), np.empty((0, 1)))
    dataset[KEY] = o.SubDataset(np.vstack((dataset[KEY].x, pool_x[idx])), np.vstack((dataset[KEY].y, pool_y[idx])))
  x_obs, y_obs = observed()
  with np.errstate(all='ignore'):
    mu, var = o.predict(mean_func, cov_func, params, x_obs, y_obs, pool_x, WFO)
  return Loop(np.asarray(sel), np.asarray(acq), np.asarray(vals_all), mu.reshape(-1), var.reshape(-1))


def case_world(case, dtype=np.float64):
  """cases.world; for the NaN case the value of the candidate that the NaN-free loop selects at iteration `nan_at` set to NaN; for the
  duplicate case the candidate the loop selects most often after iteration 0 copied into the OTHER workgroup of 256 columns (over
  row dup[0] of workgroup 0 if it sits in a later one, else over row dup[1]): the lower twin must win every tie across workgroups."""
  w = cases.world(case, dtype)
  if case.dup is not None:
    later = oracle_loop(w).sel[1:].tolist()
    src = max(set(later), key=later.count)
    w = cases.with_twin(w, src, case.dup[0] if src >= 256 else case.dup[1])
  if case.nan_at is not None:
    w = cases.with_nan(w, int(oracle_loop(w).sel[case.nan_at]))
  return w


def recurrence_loop(w):
  """The row recurrence: columns = pool then initial observations; the first n0 rows are forced pivots on the extra columns."""
  case = w.case
  mean_func, cov_func = cases.oracle_funcs(case)
  sub, _, _ = cases.ACQS[case.acq]
  params = cases.oracle_params(w)
  dataset = cases.oracle_dataset(w)
  f8 = lambda a: np.asarray(a, dtype=np.float64)
  cols = np.vstack((f8(w.pool_x), f8(w.x0).reshape(-1, case.D)))
  ycol = np.concatenate((f8(w.pool_y).reshape(-1), f8(w.y0).reshape(-1)))
  M, n0, steps = case.M, case.n0, case.n0 + case.iters
  noise, = o.retrieve_params(params, ['noise_variance'], WFO)
  noise = float(np.squeeze(noise))
  mu = mean_func(params, cols, warp_func=WFO).reshape(-1).astype(np.float64)
  kd = cov_func(params, cols, warp_func=WFO, diag=True).reshape(-1)
  V = np.zeros((steps, cols.shape[0]))
  ss = np.zeros(cols.shape[0])
  count = len([k for k, v in dataset.items() if v.aligned is None])
  scale_of = lambda c: c / (c - 1.) if c > 1 else 1.0
  scale0, scale = scale_of(count), scale_of(count + (KEY not in dataset))
  yobs, sel, acq = [], [], []
  for step in range(steps):
    if step < n0:
      p = M + step
    else:
      if not yobs:
        param = 3.0 if case.acq == 'ucb3' else 0.0
      elif case.acq == 'ucb3':
        param = 3.0
      else:
        param = np.max(yobs) + {'ei': 0.0, 'pi': 0.1, 'pi2': 0.1 * np.std(yobs)}[case.acq]
      with np.errstate(all='ignore'):
        v2 = (kd[:M] - ss[:M] + noise) * (scale0 if step == n0 else scale)
        vals = np.asarray(sub(mu[:M], np.sqrt(v2), param))
      p = int(np.argmax(vals))
      sel.append(p); acq.append(vals[p])
    with np.errstate(all='ignore'):
      kp = cov_func(params, cols[p:p + 1], cols, warp_func=WFO).reshape(-1)
      l2 = kd[p] + noise + 1e-6 - ss[p]
      l = np.sqrt(l2) if l2 > 0 else np.nan
      V[step] = (kp - V[:step, p] @ V[:step]) / l
      z = (ycol[p] - mu[p]) / l
      ss = ss + V[step]**2
      mu = mu + V[step] * z
    yobs.append(ycol[p])
  return Loop(np.asarray(sel), np.asarray(acq), None, mu[:M], (kd - ss)[:M])


def min_gap(loop):
  """Smallest relative gap between the best and the second-best value over the iterations, exact ties excepted (inf: none)."""
  worst = np.inf
  for vals in loop.vals:
    if vals.size < 2 or np.any(np.isnan(vals)):
      continue
    top = np.sort(vals)[-2:]
    if top[1] == top[0]:
      continue
    worst = min(worst, (top[1] - top[0]) / max(abs(top[1]), 1e-300))
  return worst
