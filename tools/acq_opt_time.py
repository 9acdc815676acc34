"""ms per inner maximisation of the acquisition function, SciPy's L-BFGS-B over value_and_grad (context option 'acq_fused' on: the
fastest host-driven path) against ac_func.maximize (hbo_acq_maximize: the optimiser on the device), same process, same seeded model
(tools/acq_fused_time.py: make -- Matern-5/2, constant mean, EI, D = 6), same start:

  python tools/acq_opt_time.py                      S in {1 (GP), 50} x n in {10, 100}; new side with R = 1 and R = 16 starts
  python tools/acq_opt_time.py --trace scipy|device one shape (--S --n --R), `--calls` maximisations of one side after a warm-up: the
                                                    process to put under `rocprofv3 --kernel-trace --stats`
  options: --window 0.5 --repeats 5 --segment N (evaluations per hbo_acq_maximize call; default acfun.ACQ_OPT_SEGMENT)

Both sides are warmed up first (factors cached on the model, workspaces grown); the windows alternate between the sides so that clock
drift hits them alike; the spread reported is (max - min) / median over the repeats of a side.  Beside the time: the evaluations a
maximisation spent (SciPy: calls of value_and_grad; device: evaluations consumed by the start that took longest, and the evaluations
queued, a multiple of the segment) and the acquisition value reached (device, R = 16: the best start's)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.optimize

from hyperbo_amd import _native as nat
from hyperbo_amd.bo_utils import acfun
from tools.acq_fused_time import make, window

AC = acfun.expected_improvement


def sides(S, n, D, R, segment):
  """(scipy side, device side, close): callables that run one maximisation and return (evaluations, value reached, evaluations queued)."""
  model, cand = make(S, n, 64, D)
  vals = AC(model=model, sub_dataset_key=0, x_queries=cand).reshape(-1)
  order = np.argsort(-vals, kind='stable')
  x_init, starts = np.asarray(cand[order[0]], dtype=np.float64), cand[order[:R]]
  bounds = [(0.0, 1.0)] * D

  def by_scipy():
    count = [0]

    def neg(x):
      count[0] += 1
      v, g = AC.value_and_grad(model=model, sub_dataset_key=0, x_queries=x[None, :])
      return -float(v[0, 0]), -g[0]
    res = scipy.optimize.minimize(neg, x_init, jac=True, method='L-BFGS-B', bounds=bounds)
    return count[0], -float(res.fun), count[0]

  def by_device():
    _, v, info = AC.maximize(model=model, sub_dataset_key=0, x_init=starts, opts={'segment': segment})
    longest = int(np.max(info['evals']))
    return longest, v, -(-longest // segment) * segment
  return by_scipy, by_device, (lambda: acfun.drop_sample_caches(model) if S else None)


def measure(S, n, D, R, seconds, repeats, segment):
  ctx = nat.default_context()
  ctx.set_option('acq_fused', 1)
  by_scipy, by_device, close = sides(S, n, D, R, segment)
  try:
    for _ in range(3):
      es, vs, _ = by_scipy(); ed, vd, qd = by_device()
    res = {0: [], 1: []}
    for _ in range(repeats):
      res[0].append(window(by_scipy, seconds)); res[1].append(window(by_device, seconds))
  finally:
    ctx.set_option('acq_fused', 0)
    close()
  stat = lambda ts: (float(np.median(ts)), float((max(ts) - min(ts)) / np.median(ts)))
  (a, sa), (b, sb) = stat(res[0]), stat(res[1])
  print(f'| {S if S else "1 (GP)"} | {n} | {R} | {a:.3f} | {100 * sa:.1f} % | {es} | {vs:.9g} | {b:.3f} | {100 * sb:.1f} % | {ed} / {qd} | {vd:.9g} | {a / b:.2f} |',
        flush=True)


def trace(side, S, n, D, R, calls, segment):
  ctx = nat.default_context()
  ctx.set_option('acq_fused', 1)
  by_scipy, by_device, close = sides(S, n, D, R, segment)
  call = by_scipy if side == 'scipy' else by_device
  try:
    call()
    t0 = time.perf_counter()
    for _ in range(calls):
      evals, value, queued = call()
    print(f'trace {side}: S={S} n={n} D={D} R={R}: {calls} maximisations after 1 warm-up, {1e3 * (time.perf_counter() - t0) / calls:.3f} ms each, '
          f'{evals} evaluations ({queued} queued), value {value:.9g}')
  finally:
    ctx.set_option('acq_fused', 0)
    close()


if __name__ == '__main__':
  ap = argparse.ArgumentParser()
  ap.add_argument('--trace', choices=['scipy', 'device'])
  ap.add_argument('--S', type=int, default=50); ap.add_argument('--n', type=int, default=100); ap.add_argument('--R', type=int, default=1)
  ap.add_argument('--D', type=int, default=6); ap.add_argument('--calls', type=int, default=20)
  ap.add_argument('--window', type=float, default=0.5); ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--segment', type=int, default=acfun.ACQ_OPT_SEGMENT)
  a = ap.parse_args()
  if a.trace:
    trace(a.trace, a.S, a.n, a.D, a.R, a.calls, a.segment)
  else:
    print(f'segment = {a.segment} evaluations per hbo_acq_maximize call')
    print('| S | n | R | SciPy ms | spread | evals | value | device ms | spread | evals longest / queued | value | SciPy / device |')
    print('|---|---|---|---|---|---|---|---|---|---|---|---|')
    for S in (0, 50):
      for n in (10, 100):
        for R in (1, 16):
          measure(S, n, a.D, R, a.window, a.repeats, a.segment)
