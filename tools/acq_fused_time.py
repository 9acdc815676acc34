"""ms per acquisition value_and_grad call with the context option 'acq_fused' off and on, same process, same seeded model:

  python tools/acq_fused_time.py                 every shape of profiles/acq_fused.md, windows of >= 0.5 s, 5 repeats per side
  python tools/acq_fused_time.py --trace off|on  one shape (S n M below), `--calls` calls of one path after a warm-up: the process to
                                                 put under `rocprofv3 --kernel-trace --stats` (kernels per call = launches / calls)
  options: --S 50 --n 100 --M 1 --D 6 --calls 200 --window 0.5 --repeats 5

Each call ends in a stream synchronisation inside the library, so the host clock brackets whole calls.  Both paths are warmed up
first (factors cached on the model, workspaces grown); the windows alternate off / on so that clock drift hits both alike; the spread
reported is (max - min) / median over the repeats of a side."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from hyperbo_amd import _native as nat
from hyperbo_amd.basics import definitions as defs
from hyperbo_amd.bo_utils import acfun
from hyperbo_amd.gp_utils import gp, kernel, mean, utils


def inv_softplus(v):
  return np.log(np.expm1(np.asarray(v, dtype=np.float64)))


def make(S, n, M, D, seed=7):
  """An HGP of S parameter samples (S = 0: a plain GP) over n observations in D dimensions, and M queries."""
  rng = np.random.default_rng(seed)
  x = rng.uniform(size=(n, D)); w = rng.normal(size=D)
  y = np.sin(2 * np.pi * x @ w)[:, None] + 0.1 * rng.normal(size=(n, 1))
  xq = rng.uniform(size=(M, D))
  smp = lambda: {'lengthscale': inv_softplus(np.full(D, 0.5)) + 0.2 * rng.normal(size=D), 'signal_variance': inv_softplus(1.0) + 0.1 * rng.normal(),
                 'noise_variance': inv_softplus(1e-2) + 0.1 * rng.normal(), 'constant': np.array(0.1 * rng.normal())}
  samples = [smp() for _ in range(max(S, 1))]
  data = {0: defs.SubDataset(x, y), 1: defs.SubDataset(x[:5], y[:5])}
  if S == 0:
    model = gp.GP(data, mean.constant, kernel.matern52, defs.GPParams(model=samples[0]), utils.DEFAULT_WARP_FUNC)
  else:
    model = gp.HGP(data, mean.constant, kernel.matern52, defs.GPParams(model=samples[0], samples=samples), utils.DEFAULT_WARP_FUNC)
  return model, xq


def window(call, seconds):
  """ms per call over a window of at least `seconds`."""
  n, t0 = 0, time.perf_counter()
  while True:
    call(); n += 1
    t = time.perf_counter() - t0
    if t >= seconds:
      return 1e3 * t / n


def measure(S, n, M, D, seconds, repeats):
  ctx = nat.default_context()
  model, xq = make(S, n, M, D)
  call = lambda: acfun.expected_improvement.value_and_grad(model=model, sub_dataset_key=0, x_queries=xq)
  res = {0: [], 1: []}
  try:
    for v in (0, 1):
      ctx.set_option('acq_fused', v)
      for _ in range(5):
        call()
    for _ in range(repeats):
      for v in (0, 1):
        ctx.set_option('acq_fused', v)
        res[v].append(window(call, seconds))
  finally:
    ctx.set_option('acq_fused', 0)
    if S:
      acfun.drop_sample_caches(model)
  stat = lambda ts: (float(np.median(ts)), float((max(ts) - min(ts)) / np.median(ts)))
  (off, s_off), (on, s_on) = stat(res[0]), stat(res[1])
  print(f'| {S if S else "1 (GP)"} | {n} | {D} | {M} | {off:.3f} | {100 * s_off:.1f} % | {on:.3f} | {100 * s_on:.1f} % | {off / on:.2f} |', flush=True)


def trace(side, S, n, M, D, calls):
  ctx = nat.default_context()
  model, xq = make(S, n, M, D)
  ctx.set_option('acq_fused', 1 if side == 'on' else 0)
  call = lambda: acfun.expected_improvement.value_and_grad(model=model, sub_dataset_key=0, x_queries=xq)
  try:
    call()   # factorises the samples (S factorisations: subtract them from the trace by the kernel names)
    t0 = time.perf_counter()
    for _ in range(calls):
      call()
    print(f'trace {side}: S={S} n={n} M={M} D={D}: {calls} calls after 1 warm-up, {1e3 * (time.perf_counter() - t0) / calls:.3f} ms per call')
  finally:
    ctx.set_option('acq_fused', 0)
    if S:
      acfun.drop_sample_caches(model)


if __name__ == '__main__':
  ap = argparse.ArgumentParser()
  ap.add_argument('--trace', choices=['off', 'on'])
  ap.add_argument('--S', type=int, default=50); ap.add_argument('--n', type=int, default=100); ap.add_argument('--M', type=int, default=1)
  ap.add_argument('--D', type=int, default=6); ap.add_argument('--calls', type=int, default=200)
  ap.add_argument('--window', type=float, default=0.5); ap.add_argument('--repeats', type=int, default=5)
  a = ap.parse_args()
  if a.trace:
    trace(a.trace, a.S, a.n, a.M, a.D, a.calls)
  else:
    print('| S | n | D | M | off ms/call | off spread | on ms/call | on spread | off / on |')
    print('|---|---|---|---|---|---|---|---|---|')
    for S, n, M in ((50, 100, 1), (100, 100, 1), (50, 100, 16), (50, 10, 1), (50, 128, 1), (0, 100, 1), (0, 100, 16)):
      measure(S, n, M, a.D, a.window, a.repeats)
