"""ms per Adam step of GP.train() on bench.py's small_tasks workloads, host driver vs config['adam_on_device'] (hbo_train_adam), side
by side: se_constant and matern52_mlp_linear_mlp (24 tasks x 100 points, D = 4, batch_size > n: resident) and
se_constant_resampled_400_to_100 (24 x 400 points, batch_size 100: a fresh batch per step).  A host clock around complete train()
calls (each ends in a synchronisation); one warm-up call per setting, then `reps` interleaved rounds, median.

  python tools/train_device_time.py [steps=200] [reps=5] [only=<workload>] [device_only] [method=adam|lbfgs] [segment=]

`device_only` with `only=` runs one device-loop train() and nothing else: the run to put under rocprofv3 --kernel-trace --stats.

`method=lbfgs` (steps defaults to 30): the same three workloads under L-BFGS, host driver vs config['lbfgs_on_device']
(hbo_train_lbfgs); ms per train() call and ms per evaluation, the evaluations counted from the device loop's log and, for the host
driver, around DeviceDataset.evaluate.  The resampled workload draws its one sub-sample per call.  `segment=` overrides gp.LBFGS_SEGMENT."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hyperbo_amd.basics import definitions as defs  # noqa: E402
from hyperbo_amd.gp_utils import gp, kernel, mean, objectives, utils  # noqa: E402


def workloads():
  rng = np.random.default_rng(0)
  d, tasks, feats = 4, 24, (8, 8)

  def data_of(n):
    out = {}
    for k in range(tasks):
      x = rng.uniform(size=(n, d)); w = rng.normal(size=d)
      out[k] = defs.SubDataset(x, np.sin(2 * np.pi * x @ w)[:, None] + 0.1 * rng.normal(size=(n, 1)))
    return out
  model = lambda: {'lengthscale': np.zeros(d), 'signal_variance': np.array(0.0), 'noise_variance': np.array(-2.0), 'constant': np.array(0.0)}
  mrng = np.random.default_rng(1)
  mlp0 = {}
  fin = d
  for l, f in enumerate(feats):
    mlp0[f'Dense_{l}'] = {'kernel': mrng.normal(size=(fin, f)) / np.sqrt(fin), 'bias': np.zeros(f)}; fin = f
  lin0 = {'kernel': mrng.normal(size=(feats[-1], 1)) / np.sqrt(feats[-1]), 'bias': np.zeros(1)}

  def mlp_model():
    mm = model(); mm['lengthscale'] = np.zeros(feats[-1])
    mm['mlp_params'] = {k: dict(v) for k, v in mlp0.items()}
    mm['linear_mean'] = dict(lin0)
    return mm
  d100, d400 = data_of(100), data_of(400)
  return {'se_constant': (d100, model, kernel.squared_exponential, mean.constant, 101, feats),
          'matern52_mlp_linear_mlp': (d100, mlp_model, kernel.matern52_mlp, mean.linear_mlp, 101, feats),
          'se_constant_resampled_400_to_100': (d400, model, kernel.squared_exponential, mean.constant, 100, feats)}


def run(w, steps, on_device, key):
  data, mk, cov, mu, bs, feats = w
  config = {'method': 'adam', 'batch_size': bs, 'max_training_step': steps, 'learning_rate': 1e-3, 'objective': objectives.nll,
            'mlp_features': feats}
  if on_device:
    config['adam_on_device'] = True
  g = gp.GP(data, mu, cov, defs.GPParams(model=mk(), config=config), utils.DEFAULT_WARP_FUNC)
  t0 = time.perf_counter()
  g.train(key=key)
  return (time.perf_counter() - t0) / steps * 1e3


def run_lbfgs(w, steps, on_device, key):
  """(ms per train() call, evaluations made)."""
  data, mk, cov, mu, bs, feats = w
  config = {'method': 'lbfgs', 'batch_size': bs, 'max_training_step': steps, 'objective': objectives.nll, 'mlp_features': feats}
  if on_device:
    config['lbfgs_on_device'] = True
    config['lbfgs_eval_log'] = {}
  g = gp.GP(data, mu, cov, defs.GPParams(model=mk(), config=config), utils.DEFAULT_WARP_FUNC)
  calls = [0]
  orig = objectives.DeviceDataset.evaluate

  def counting(self, *a, **k):
    calls[0] += 1
    return orig(self, *a, **k)
  objectives.DeviceDataset.evaluate = counting
  try:
    t0 = time.perf_counter()
    g.train(key=key)
    ms = (time.perf_counter() - t0) * 1e3
  finally:
    objectives.DeviceDataset.evaluate = orig
  return ms, (len(config['lbfgs_eval_log']['evals']) if on_device else calls[0])


def main_lbfgs(args):
  steps, reps = int(args.get('steps', 30)), int(args.get('reps', 5))
  if 'segment' in args:   # evaluations per hbo_train_lbfgs call, to compare against the default
    gp.LBFGS_SEGMENT = int(args['segment'])
  ws = workloads()
  names = [args['only']] if 'only' in args else list(ws)
  if 'device_only' in args:
    ms, n = run_lbfgs(ws[names[0]], steps, True, 0)
    print(json.dumps({names[0]: {'ms_per_call': ms, 'evaluations': n}}))
    return
  out = {}
  for name in names:
    for dev in (False, True):
      run_lbfgs(ws[name], steps, dev, 0)   # warm-up
    t = {False: [], True: []}
    for r in range(reps):
      for dev in (False, True):
        t[dev].append(run_lbfgs(ws[name], steps, dev, r + 1))
    res = {}
    for dev, label in ((False, 'host'), (True, 'device')):
      ms = [v for v, _ in t[dev]]
      per = [v / n for v, n in t[dev]]
      res[label + '_ms_per_call'] = round(float(np.median(ms)), 4)
      res[label + '_ms_per_eval'] = round(float(np.median(per)), 4)
      res[label + '_all_ms'] = [round(v, 4) for v in ms]
      res[label + '_evals'] = [n for _, n in t[dev]]
    res['device_faster'] = bool(max(res['device_all_ms']) < min(res['host_all_ms']))   # all five rounds below all five host rounds
    out[name] = res
    print(name, json.dumps(res), flush=True)
  print(json.dumps({'method': 'lbfgs', 'steps': steps, 'reps': reps, 'segment': gp.LBFGS_SEGMENT, 'results': out}))


def main():
  args = dict(a.split('=', 1) if '=' in a else (a, '1') for a in sys.argv[1:])
  if args.get('method', 'adam') == 'lbfgs':
    return main_lbfgs(args)
  steps, reps = int(args.get('steps', 200)), int(args.get('reps', 5))
  ws = workloads()
  names = [args['only']] if 'only' in args else list(ws)
  if 'device_only' in args:
    print(json.dumps({names[0]: run(ws[names[0]], steps, True, 0)}))
    return
  out = {}
  for name in names:
    for dev in (False, True):
      run(ws[name], steps, dev, 0)   # warm-up: pools, staging buffers, code objects
    t = {False: [], True: []}
    for r in range(reps):
      for dev in (False, True):
        t[dev].append(run(ws[name], steps, dev, r + 1))
    out[name] = {'host_ms_per_step': round(float(np.median(t[False])), 4), 'device_ms_per_step': round(float(np.median(t[True])), 4),
                 'host_all': [round(v, 4) for v in t[False]], 'device_all': [round(v, 4) for v in t[True]]}
    print(name, json.dumps(out[name]), flush=True)
  print(json.dumps({'steps': steps, 'reps': reps, 'results': out}))


if __name__ == '__main__':
  main()
