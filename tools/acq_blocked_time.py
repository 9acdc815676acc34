"""ms per evaluation and per inner maximisation of the acquisition function over caches of MORE than 128 observations: the fastest
route without config['acq_blocked'] against the blocked entry points (csrc/acq_blocked.hip), same process, same seeded model
(tools/acq_fused_time.py: make -- Matern-5/2, constant mean, EI, D = 6), same starts.

  evaluation     ac_func.value_and_grad at R queries.  Without the key: one hbo_acq_grad per parameter sample (the per-sample loop; a plain
                 GP: one call).  With it (and the context option 'acq_fused'): one hbo_acq_grad_samples_blocked call.
  maximisation   Without the key: SciPy's L-BFGS-B over value_and_grad, one run per start, one after the other.  With it:
                 ac_func.maximize (hbo_acq_maximize_blocked), the R starts in one call.

  python tools/acq_blocked_time.py                 n in {129, 512, 2048} x S in {1 (GP), 50} x R in {1, 16}
  options: --window 0.3 --repeats 3 --n / --S / --R (one shape) --D 6 --no-maximise

Both sides are warmed up first (factors cached on the models, workspaces grown); the windows alternate between the sides so that clock
drift hits them alike; a window holds at least one call; the spread reported is (max - min) / median over the repeats of a side.
Beside the maximisation times: the evaluations spent (SciPy: calls of value_and_grad summed over the starts; device: evaluations
consumed by the start that took longest) and the acquisition value reached (the best start's)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.optimize

from hyperbo_amd import _native as nat
from hyperbo_amd.bo_utils import acfun
from tools.acq_fused_time import make, window

AC = acfun.expected_improvement


def sides(S, n, D, R):
  """((old evaluation, new evaluation), (old maximisation, new maximisation), close)."""
  old, cand = make(S, n, 64, D)
  new, _ = make(S, n, 64, D)
  new.params.config['acq_blocked'] = True
  vals = AC(model=old, sub_dataset_key=0, x_queries=cand).reshape(-1)
  starts = np.ascontiguousarray(cand[np.argsort(-vals, kind='stable')[:R]], dtype=np.float64)
  bounds = [(0.0, 1.0)] * D
  ev = lambda model: (lambda: AC.value_and_grad(model=model, sub_dataset_key=0, x_queries=starts))

  def by_scipy():
    count, best = [0], -np.inf

    def neg(x):
      count[0] += 1
      v, g = AC.value_and_grad(model=old, sub_dataset_key=0, x_queries=x[None, :])
      return -float(v[0, 0]), -g[0]
    for x0 in starts:
      best = max(best, -float(scipy.optimize.minimize(neg, x0, jac=True, method='L-BFGS-B', bounds=bounds).fun))
    return count[0], best

  def by_device():
    _, v, info = AC.maximize(model=new, sub_dataset_key=0, x_init=starts)
    return int(np.max(info['evals'])), v

  def close():
    if S:
      acfun.drop_sample_caches(old); acfun.drop_sample_caches(new)
  return (ev(old), ev(new)), (by_scipy, by_device), close


def _stat(ts):
  return float(np.median(ts)), float((max(ts) - min(ts)) / np.median(ts))


def _pair(a, b, seconds, repeats):
  res = ([], [])
  for _ in range(repeats):
    res[0].append(window(a, seconds)); res[1].append(window(b, seconds))
  return _stat(res[0]), _stat(res[1])


def measure(S, n, D, R, seconds, repeats, maximise):
  ctx = nat.default_context()
  ctx.set_option('acq_fused', 1)
  evs, mxs, close = sides(S, n, D, R)
  try:
    for f in evs:
      f(); f()
    vo, go = evs[0](); vn, gn = evs[1]()
    dv = float(np.max(np.abs(vo - vn) / np.maximum(np.abs(vo), 1e-300))); dg = float(np.max(np.abs(go - gn)) / max(np.max(np.abs(go)), 1e-3))
    (a, sa), (b, sb) = _pair(evs[0], evs[1], seconds, repeats)
    row = f'| {S if S else "1 (GP)"} | {n} | {R} | {a:.3f} | {100 * sa:.1f} % | {b:.3f} | {100 * sb:.1f} % | {a / b:.2f} | {dv:.1e} / {dg:.1e} |'
    if maximise:
      (es, vs), (ed, vd) = mxs[0](), mxs[1]()
      (c, sc), (d, sd) = _pair(mxs[0], mxs[1], seconds, repeats)
      row += f' {c:.2f} | {100 * sc:.1f} % | {es} | {vs:.9g} | {d:.2f} | {100 * sd:.1f} % | {ed} | {vd:.9g} | {c / d:.2f} |'
    print(row, flush=True)
  finally:
    ctx.set_option('acq_fused', 0)
    close()


if __name__ == '__main__':
  ap = argparse.ArgumentParser()
  ap.add_argument('--S', type=int); ap.add_argument('--n', type=int); ap.add_argument('--R', type=int)
  ap.add_argument('--D', type=int, default=6)
  ap.add_argument('--window', type=float, default=0.3); ap.add_argument('--repeats', type=int, default=3)
  ap.add_argument('--no-maximise', action='store_true')
  a = ap.parse_args()
  head = '| S | n | R | loop ms / evaluation | spread | blocked ms / evaluation | spread | loop / blocked | value / gradient difference |'
  if not a.no_maximise:
    head += ' SciPy ms / maximisation | spread | evals | value | device ms / maximisation | spread | evals longest | value | SciPy / device |'
  print(head)
  print('|' + '---|' * (head.count('|') - 1))
  for n in ([a.n] if a.n else (129, 512, 2048)):
    for S in ([a.S] if a.S is not None else (0, 50)):
      for R in ([a.R] if a.R else (1, 16)):
        measure(S, n, a.D, R, a.window, a.repeats, not a.no_maximise)
