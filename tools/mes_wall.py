"""Wall-clock figures of max-value entropy search (profiles/mes.md), every pair measured in the same process and run:

  1. hbo_mes_grad_samples against hbo_acq_grad_samples_blocked with EI: n in {100, 1000}, M = 256, K in {16, 64, 256}
  2. one acfun.mes.suggest split into its parts: draw + path maximisation, pool scoring, maximisation
  3. hbo_acq_mes against hbo_acq with EI: M = 65536 against the n = 1000 cache

The yardstick is the existing EI entry point on the same shapes, never MES against itself.  Each figure is the median of `--reps` calls
after `--warmup` calls, host wall clock around the whole call (upload, launches, copy back, one synchronisation).

  python tools/mes_wall.py [--reps 20] [--warmup 3] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hyperbo_amd import _model as hmodel            # noqa: E402
from hyperbo_amd import _native as nat              # noqa: E402
from hyperbo_amd.basics import definitions as defs, linalg   # noqa: E402
from hyperbo_amd.bo_utils import acfun              # noqa: E402
from hyperbo_amd.gp_utils import gp, kernel, mean, utils     # noqa: E402

PD = C.POINTER(C.c_double)
D = 6


def median_ms(fn, reps, warmup):
  for _ in range(warmup):
    fn()
  t = []
  for _ in range(reps):
    t0 = time.perf_counter()
    fn()
    t.append((time.perf_counter() - t0) * 1e3)
  return float(np.median(t))


def problem(n, seed=0):
  rng = np.random.default_rng(seed)
  x = rng.uniform(size=(n, D))
  y = np.sin(3.0 * x[:, :1]) + np.cos(2.0 * x[:, 1:2]) + 0.05 * rng.normal(size=(n, 1))
  model_t = {'lengthscale': np.full(D, 0.5), 'signal_variance': np.array(0.5), 'noise_variance': np.array(-3.0), 'constant': np.array(0.1)}
  ds = {'t': defs.SubDataset(x, y), 'a': defs.SubDataset(x[:8], y[:8])}
  return gp.GP(ds, mean.constant, kernel.matern52, defs.GPParams(model=model_t, config={}), utils.DEFAULT_WARP_FUNC), rng


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  lib = nat.lib()
  res = {'grad': [], 'pool': [], 'suggest': {}}
  for n in (100, 1000):
    model, rng = problem(n)
    handle, _, bm, noise, scale = acfun._single_model(model, 't')
    ctx = handle.ctx
    ymax = float(np.max(model.dataset['t'].y))
    xq = np.ascontiguousarray(rng.uniform(size=(256, D)))
    structs, caches = (nat.Model * 1)(bm.struct), (C.c_void_p * 1)(handle.handle)
    prm, nse = (C.c_double * 1)(ymax), (C.c_double * 1)(noise)
    out, grad = np.empty((1, 256)), np.empty((1, 256, D))
    ei = lambda: ctx.check(lib.hbo_acq_grad_samples_blocked(ctx.handle, structs, 1, caches, nat.ptr(xq), 256, nat.ACQ_EI, prm, nse, scale, nat.ptr(out),
                                                            grad.ctypes.data_as(PD)))
    t_ei = median_ms(ei, a.reps, a.warmup)
    for k in (16, 64, 256):
      ys = np.ascontiguousarray(ymax + np.abs(rng.normal(size=(1, k))) * 0.3)
      mes = lambda: ctx.check(lib.hbo_mes_grad_samples(ctx.handle, structs, 1, caches, nat.ptr(xq), 256, ys.ctypes.data_as(PD), k, nse, scale, nat.ptr(out),
                                                       grad.ctypes.data_as(PD)))
      res['grad'].append({'n': n, 'M': 256, 'K': k, 'ei_ms': t_ei, 'mes_ms': median_ms(mes, a.reps, a.warmup)})
    if n == 1000:
      m = 65536
      pool = np.ascontiguousarray(rng.uniform(size=(m, D)))
      vals = np.empty((m, 1))
      ei = lambda: ctx.check(lib.hbo_acq(ctx.handle, bm.ref(), handle.handle, nat.ptr(pool), m, nat.ACQ_EI, ymax, noise, scale, nat.ptr(vals)))
      t_ei = median_ms(ei, a.reps, a.warmup)
      for k in (16, 64, 256):
        ys = np.ascontiguousarray(ymax + np.abs(rng.normal(size=k)) * 0.3)
        mes = lambda: ctx.check(lib.hbo_acq_mes(ctx.handle, bm.ref(), handle.handle, nat.ptr(pool), m, ys.ctypes.data_as(PD), k, 0.0, scale, nat.ptr(vals)))
        res['pool'].append({'n': n, 'M': m, 'K': k, 'ei_ms': t_ei, 'mes_ms': median_ms(mes, a.reps, a.warmup)})
      # one suggest, part by part (what MaxValueEntropySearch.suggest does, with a clock between the parts)
      xc = np.ascontiguousarray(rng.uniform(size=(1024, D)))
      ac = acfun.MaxValueEntropySearch()
      parts = {'draw_and_path_maximisation': [], 'pool_scoring': [], 'maximisation': []}
      for rep in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        ys = acfun.max_value_samples(model, 't', xc, ac.num_maxima, 100 + rep, ac.num_features, ac.starts)
        t1 = time.perf_counter()
        v = np.asarray(ac(model, 't', xc, maxima=ys), dtype=np.float64).reshape(-1)
        t2 = time.perf_counter()
        order = np.argsort(-v, kind='stable')[:ac.starts]
        ac.maximize(model=model, sub_dataset_key='t', x_init=xc[order], maxima=ys)
        t3 = time.perf_counter()
        if rep >= a.warmup:
          for key, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2)):
            parts[key].append(dt * 1e3)
      res['suggest'] = {'n': n, 'candidates': 1024, 'K': ac.num_maxima, 'starts': ac.starts, **{k: float(np.median(v)) for k, v in parts.items()}}
  line = json.dumps(res)
  print(line)
  if a.out:
    with open(a.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
