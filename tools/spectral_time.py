"""Device eigensolver vs host LAPACK: hbo_sym_eig with and without vectors, hbo_nll_spectral, and GP.stats() with the option
'spectral' off (host SVD) and on, on SE Gram matrices.  Prints one table (wall ms, best of --reps) with the outer sweep counts.

  python tools/spectral_time.py [--sizes 512,1024,2048,4096,8192] [--reps 2] [--stats-n 8192]
The host side runs numpy.linalg.svd / eigh on the same fp64 Gram (the thread count is the BLAS library's, e.g. OMP_NUM_THREADS)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hyperbo_amd import _native as nat  # noqa: E402
from hyperbo_amd.basics import definitions as defs  # noqa: E402
from hyperbo_amd.gp_utils import gp, kernel, mean, objectives, utils  # noqa: E402


def best(fn, reps):
  out, t = None, []
  for _ in range(reps):
    t0 = time.perf_counter(); out = fn(); t.append((time.perf_counter() - t0) * 1e3)
  return min(t), out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--sizes', default='512,1024,2048,4096,8192')
  ap.add_argument('--reps', type=int, default=2)
  ap.add_argument('--stats-n', type=int, default=8192)
  ap.add_argument('--host-max', type=int, default=8192, help='largest n timed on the host')
  a = ap.parse_args()
  ctx = nat.default_context()
  lib = nat.lib()
  rng = np.random.default_rng(0)
  d = 4
  params = defs.GPParams(model={'lengthscale': np.full(d, 0.0), 'signal_variance': np.array(0.0), 'noise_variance': np.array(-6.0),
                                'constant': np.array(0.0)})
  wf = utils.DEFAULT_WARP_FUNC
  rows = []

  def eig(A, count, vecs):
    n = A.shape[-1]
    w = np.empty((count, n)); v = np.empty((count, n, n)) if vecs else None
    rc = lib.hbo_sym_eig(ctx.handle, nat.F64, nat.ptr(A), n, count, nat.ptr(w), nat.ptr(v))
    sw = ctx.get_option('eig_sweeps')
    return sw if rc == 0 else -sw   # (a negative count: not converged at the cap)

  def case(label, tasks):
    ds = {i: defs.SubDataset(x, y) for i, (x, y) in enumerate(tasks)}
    n = tasks[0][0].shape[0]
    A = np.stack([np.asarray(kernel.squared_exponential(params, x, warp_func=wf)) + np.eye(n) * (np.log1p(np.exp(-6.0)) + 1e-6)
                  for x, _ in tasks])
    t_nv, sw = best(lambda: eig(A, len(tasks), False), a.reps)
    t_v, _ = best(lambda: eig(A, len(tasks), True), a.reps)
    dev = objectives.DeviceDataset(ds)
    t_nll, _ = best(lambda: dev.evaluate_spectral(mean.constant, kernel.squared_exponential, params, wf), a.reps)
    dev.close()
    sw_nll = ctx.get_option('eig_sweeps')
    t_svd = t_eigh = float('nan')
    if n <= a.host_max:
      t_svd, _ = best(lambda: [np.linalg.svd(A[i]) for i in range(len(tasks))], 1)
      t_eigh, _ = best(lambda: [np.linalg.eigh(A[i]) for i in range(len(tasks))], 1)
    rows.append((label, t_nv, t_v, t_nll, t_svd, t_eigh, sw, sw_nll))

  case('24 x 100', [(rng.uniform(size=(100, d)), rng.normal(size=(100, 1))) for _ in range(24)])
  for n in [int(s) for s in a.sizes.split(',') if s]:
    case(f'1 x {n}', [(rng.uniform(size=(n, d)), rng.normal(size=(n, 1)))])
  print('| tasks x n | sym_eig w (ms) | sym_eig w+V (ms) | nll_spectral (ms) | host svd (ms) | host eigh (ms) | sweeps (eig) | sweeps (nll) |')
  print('|---|---|---|---|---|---|---|---|')
  for r in rows:
    print('| %s | %.1f | %.1f | %.1f | %.1f | %.1f | %d | %d |' % r)
  if a.stats_n:
    n = a.stats_n
    x = rng.uniform(size=(n, d)); y = np.sin(3 * x.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(n, 1))
    xa = rng.uniform(size=(40, d)); ya = np.sin(xa @ rng.normal(size=(d, 60)))
    m = gp.GP({0: defs.SubDataset(x, y), 'al': defs.SubDataset(xa, ya, aligned=1)}, mean.constant, kernel.squared_exponential,
              params, wf)
    t_host, st_h = best(lambda: m.stats(verbose=False), 1)
    prev = ctx.get_option('spectral')
    ctx.set_option('spectral', 1)
    try:
      t_dev, st_d = best(lambda: m.stats(verbose=False), a.reps)
    finally:
      ctx.set_option('spectral', prev)
    print(f'GP.stats() on a {n}-point task + an aligned 40 x 60 task: host {t_host:.0f} ms, device {t_dev:.0f} ms; '
          f'nll host {st_h[0]!r} device {st_d[0]!r}')


if __name__ == '__main__':
  main()
