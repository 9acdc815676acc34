"""What the Kumaraswamy input warp adds (hbo_profile stage times, level 1): cfg-2 NLL + gradient (N = 8192, D = 16, fp64, SE), one
24 x 100 Adam-step evaluation (NLL + gradient, fp64, SE) and a cfg-3-shaped EI (N = 16384 observations, 65536 candidates, D = 16,
fp32, Matern-5/2), each plain vs *_kumar.  Median of `reps` runs per leg; prints one line per leg with the stage sums and the
warp's own stages.  Usage: python tools/kumar_cost.py [reps]"""
import copy
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hyperbo_amd import _model, _native as nat   # noqa: E402
from hyperbo_amd.basics import definitions as defs, linalg   # noqa: E402
from hyperbo_amd.gp_utils import kernel, mean, objectives, utils   # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
WF = utils.DEFAULT_WARP_FUNC
KUMAR_STAGES = ('kumar_forward', 'kumar_backward')


def _params(rng, d):
  return {'lengthscale': np.zeros(d), 'signal_variance': np.array(0.0), 'noise_variance': np.array(-2.0), 'constant': np.array(0.1),
          'kumar_params': {'a': rng.uniform(-1, 1, d), 'b': rng.uniform(-1, 1, d)}}


def _run(ctx, fn):
  runs = []
  for _ in range(REPS + 1):
    ctx.profile_enable(1)
    fn()
    runs.append(ctx.profile_get())
    ctx.profile_enable(0)
  runs = runs[1:]   # (first run: allocations)
  total = np.median([sum(ms for name, (ms, _) in r.items() if name != 'host_enqueue') for r in runs])
  warp = np.median([sum(r.get(s, (0.0, 0))[0] for s in KUMAR_STAGES) for r in runs])
  return total, warp


def main():
  ctx = nat.default_context()
  rng = np.random.default_rng(0)
  d = 16

  def nll_leg(tasks, kname):
    ds = defs.SubDataset
    data = {i: ds(rng.uniform(size=(n, d)), rng.normal(size=(n, 1))) for i, n in enumerate(tasks)}
    dev = objectives._as_device(data, True)[0]
    p = _params(rng, d)
    for kn in (getattr(kernel, kname), getattr(kernel, kname + '_kumar')):
      pp = copy.deepcopy(p)
      if not kn.uses_kumar:
        pp.pop('kumar_params')
      tot, warp = _run(ctx, lambda: dev.evaluate(mean.constant, kn, defs.GPParams(model=pp), WF, want_grad=True))
      yield kn.uses_kumar, tot, warp
    dev.close()

  for label, tasks in (('cfg2 nll+grad N=8192 D=16 fp64 SE', [8192]), ('24x100 nll+grad fp64 SE', [100] * 24)):
    res = list(nll_leg(tasks, 'squared_exponential'))
    (_, t0, _), (_, t1, w1) = res
    print(f'{label}: plain {t0:.3f} ms, kumar {t1:.3f} ms (+{t1 - t0:.3f} ms; warp stages {w1:.3f} ms)')

  n, m = 16384, 65536
  x = rng.uniform(size=(n, d)).astype(np.float32)
  y = rng.normal(size=(n, 1)).astype(np.float32)
  xq = rng.uniform(size=(m, d)).astype(np.float32)
  p = _params(rng, d)
  out = np.empty((m, 1), dtype=np.float32)
  res = []
  for kn in (kernel.matern52, kernel.matern52_kumar):
    pp = copy.deepcopy(p)
    if not kn.uses_kumar:
      pp.pop('kumar_params')
    gp_p = defs.GPParams(model=pp)
    h = linalg.factor(mean.constant, kn, gp_p, x, y, WF)
    bm = _model.BuiltModel(mean.constant, kn, gp_p, WF, np.float32, d)
    res.append(_run(ctx, lambda: ctx.check(nat.lib().hbo_acq(ctx.handle, bm.ref(), h.handle, nat.ptr(xq), m, nat.ACQ_EI, float(np.max(y)),
                                                              0.1, 1.0, nat.ptr(out)))))
    h.close()
  (t0, _), (t1, w1) = res
  print(f'cfg3 EI N=16384 M=65536 D=16 fp32 M52: plain {t0:.3f} ms, kumar {t1:.3f} ms (+{t1 - t0:.3f} ms; warp stages {w1:.3f} ms)')


if __name__ == '__main__':
  main()
