"""ms per maximisation of posterior sample paths over [0, 1]^D: PathDraws.maximize (hbo_paths_maximize: the optimiser on the device,
all paths and starts in one call) beside SciPy's L-BFGS-B over PathDraws.value_and_grad (hbo_sample_paths_grad per evaluation), one
(path, start) pair at a time.  Same process, same seeded model (Matern-5/2, constant mean, fp64), same draws, same starts:

  python tools/path_opt_bench.py            8 paths x 4 starts, D = 6, n = 100, F = 1024, 64 evaluations per pair on the device
  options: --S --R --D --n --F --evals --warmup 3 --repeats 7

Both sides are warmed up first (factor cached, workspaces grown, draws made); the repeats alternate between the sides so that clock
drift hits them alike.  Reported per side: median, min and spread (max - min) / median over the repeats; beside the time the
evaluations spent (device: the longest pair / those queued; SciPy: calls of value_and_grad, all pairs) and the mean over the pairs of
the path value reached.  One JSON line at the end."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.optimize

from hyperbo_amd.basics import definitions as defs
from hyperbo_amd.gp_utils import gp, kernel, mean, utils


def make(n, D, seed=0):
  rng = np.random.default_rng(seed)
  x = rng.uniform(size=(n, D))
  y = np.sin(2 * np.pi * x @ rng.normal(size=(D, 1))) + 0.1 * rng.normal(size=(n, 1))
  inv_softplus = lambda v: np.log(np.expm1(np.asarray(v, dtype=np.float64)))
  model = {'constant': np.array(0.1), 'lengthscale': inv_softplus(np.full(D, 0.5 * np.sqrt(D))), 'signal_variance': inv_softplus(1.0),
           'noise_variance': inv_softplus(0.01)}
  return gp.GP({0: defs.SubDataset(x, y)}, mean.constant, kernel.matern52, defs.GPParams(model=model, config={}), utils.DEFAULT_WARP_FUNC)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--S', type=int, default=8); ap.add_argument('--R', type=int, default=4); ap.add_argument('--D', type=int, default=6)
  ap.add_argument('--n', type=int, default=100); ap.add_argument('--F', type=int, default=1024); ap.add_argument('--evals', type=int, default=64)
  ap.add_argument('--warmup', type=int, default=3); ap.add_argument('--repeats', type=int, default=7)
  a = ap.parse_args()
  model = make(a.n, a.D)
  draws = model.draw_paths(0, num_samples=a.S, num_features=a.F, key=1)
  x0 = np.random.default_rng(2).uniform(size=(a.S, a.R, a.D))
  bounds = [(0.0, 1.0)] * a.D

  def by_device():
    x, val, info = draws.maximize(x0, evals=a.evals, opts={'segment': a.evals})
    return int(np.max(info['evals'])), float(np.mean(val))

  def by_scipy():
    count, total = [0], 0.0
    for s in range(a.S):
      def neg(x, s=s):
        count[0] += 1
        v, g = draws.value_and_grad(x[None, :])
        return -float(v[0, s]), -g[0, s]
      for r in range(a.R):
        res = scipy.optimize.minimize(neg, x0[s, r], jac=True, method='L-BFGS-B', bounds=bounds, options={'maxfun': a.evals})
        total += -float(res.fun)
    return count[0], total / (a.S * a.R)

  for _ in range(a.warmup):
    ed, vd = by_device(); es, vs = by_scipy()
  times = {'device': [], 'scipy': []}
  for _ in range(a.repeats):
    for name, call in (('device', by_device), ('scipy', by_scipy)):
      t0 = time.perf_counter()
      call()
      times[name].append(1e3 * (time.perf_counter() - t0))
  stat = lambda ts: dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), spread=float((max(ts) - min(ts)) / np.median(ts)))
  out = dict(S=a.S, R=a.R, D=a.D, n=a.n, F=a.F, evals=a.evals, warmup=a.warmup, repeats=a.repeats,
             device=dict(stat(times['device']), evals_longest=ed, evals_queued=a.evals, mean_value=vd),
             scipy=dict(stat(times['scipy']), evals_all_pairs=es, mean_value=vs))
  out['scipy_over_device'] = out['scipy']['median_ms'] / out['device']['median_ms']
  print(f"| side | ms (median) | ms (min) | spread | evaluations | mean path value reached |")
  print('|---|---|---|---|---|---|')
  print(f"| PathDraws.maximize, {a.S} x {a.R} pairs in one call | {out['device']['median_ms']:.3f} | {out['device']['min_ms']:.3f} | "
        f"{100 * out['device']['spread']:.1f} % | {ed} longest / {a.evals} queued per pair | {vd:.9g} |")
  print(f"| SciPy L-BFGS-B over value_and_grad, pair by pair | {out['scipy']['median_ms']:.3f} | {out['scipy']['min_ms']:.3f} | "
        f"{100 * out['scipy']['spread']:.1f} % | {es} over all pairs | {vs:.9g} |")
  print(json.dumps(out))


if __name__ == '__main__':
  main()
