"""Wall-clock and device-time figures of batch expected improvement (profiles/qei.md), every pair measured in the same process and run:
S = 8 samples over caches of n = 128 observations in D = 8, B = 256 base samples, q in {1, 4, 16}, M = R = 64:

  1. one hbo_qei_grad_samples call over M batches of q points
  2. hbo_acq_grad_samples with EI over the same M * q points: the cost of scoring the points without coupling them, the only
     existing yardstick
  3. one round of hbo_qei_maximize (evals = 1 against evals = 9, the difference / 8), and its two launches from hbo_profile_enable(2)

Each wall figure is the median of `--reps` calls after `--warmup` calls, host clock around the whole call (upload, launches, copy back,
one synchronisation); the device figures are event times of the launches alone.

The driver runs every q as a step of its own: a child process under `--step-timeout` seconds with the thread pools capped at 16, and
stops at the first step that fails.

  python tools/qei_bench.py [--reps 20] [--warmup 3] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PD = C.POINTER(C.c_double)
S, N, D, B, M = 8, 128, 8, 256, 64


def median_ms(fn, reps, warmup):
  for _ in range(warmup):
    fn()
  t = []
  for _ in range(reps):
    t0 = time.perf_counter()
    fn()
    t.append((time.perf_counter() - t0) * 1e3)
  return float(np.median(t))


def step(q, reps, warmup):
  from hyperbo_amd import _model as hmodel
  from hyperbo_amd import _native as nat
  from hyperbo_amd.basics import definitions as defs, linalg
  from hyperbo_amd.bo_utils import acfun
  from hyperbo_amd.gp_utils import kernel, mean, utils
  lib = nat.lib()
  ctx = nat.default_context()
  rng = np.random.default_rng(q)
  x = rng.uniform(size=(N, D))
  y = np.sin(3.0 * x[:, :1]) + np.cos(2.0 * x[:, 1:2]) + 0.05 * rng.normal(size=(N, 1))
  wf = utils.DEFAULT_WARP_FUNC
  built, handles = [], []
  for s in range(S):
    model_t = {'lengthscale': np.full(D, 0.4 + 0.05 * s), 'signal_variance': np.array(0.5), 'noise_variance': np.array(-3.0), 'constant': np.array(0.1)}
    pn = defs.GPParams(model=model_t, config={})
    handles.append(linalg.factor(mean.constant, kernel.matern52, pn, x, y, wf, ctx=ctx))
    built.append(hmodel.BuiltModel(mean.constant, kernel.matern52, pn, wf, np.float64, D))
  structs = (nat.Model * S)(*[b.struct for b in built])
  caches = (C.c_void_p * S)(*[h.handle for h in handles])
  ymax = float(np.max(y))
  tg, nse = (C.c_double * S)(*[ymax] * S), (C.c_double * S)(*[0.05] * S)
  xb = np.ascontiguousarray(rng.uniform(size=(M, q, D)))
  z = np.ascontiguousarray(rng.standard_normal((B, q)))
  val, grad = np.empty((S, M)), np.empty((S, M, q, D))
  qei = lambda: ctx.check(lib.hbo_qei_grad_samples(ctx.handle, structs, S, caches, nat.ptr(xb), M, q, z.ctypes.data_as(PD), B, tg, nse, 1.5,
                                                   val.ctypes.data_as(PD), grad.ctypes.data_as(PD)))
  pts = np.ascontiguousarray(xb.reshape(M * q, D))
  out, g1 = np.empty((S, M * q)), np.empty((S, M * q, D))
  ei = lambda: ctx.check(lib.hbo_acq_grad_samples(ctx.handle, structs, S, caches, nat.ptr(pts), M * q, nat.ACQ_EI, tg, nse, 1.5, nat.ptr(out),
                                                  g1.ctypes.data_as(PD)))
  res = {'q': q, 'S': S, 'n': N, 'D': D, 'B': B, 'M': M, 'qei_grad_ms': median_ms(qei, reps, warmup), 'ei_grad_points_ms': median_ms(ei, reps, warmup)}
  opts = nat.AcqOptOpts(**acfun.ACQ_OPT_DEFAULTS)
  ns = lib.hbo_acq_opt_state_doubles(q * D, opts.memory)
  xo, vo, st = np.empty((M, q, D)), np.empty(M), np.empty(M, dtype=np.int32)

  def rounds(evals):
    state = np.zeros((M, ns))

    def call():
      state[:] = 0.0                                            # a fresh run every time
      ctx.check(lib.hbo_qei_maximize(ctx.handle, structs, S, caches, nat.ptr(xb), M, q, None, None, z.ctypes.data_as(PD), B, tg, nse, 1.5,
                                     C.byref(opts), nat.ptr(state), evals, nat.ptr(xo), nat.ptr(vo), nat.ptr(st), None))
    return call
  t1, t9 = median_ms(rounds(1), reps, warmup), median_ms(rounds(9), reps, warmup)
  res.update(maximize_1_ms=t1, maximize_9_ms=t9, round_ms=(t9 - t1) / 8.0)
  ctx.profile_enable(2)
  rounds(9)()
  prof = ctx.profile_get()
  qei()
  prof_grad = ctx.profile_get()
  ctx.profile_enable(0)
  res['device_ms'] = {k: v[0] / max(v[1], 1) for k, v in prof.items()}
  res['device_ms']['qei_eval_grad_call'] = prof_grad.get('qei_eval', (0.0, 1))[0]
  for h in handles:
    h.close()
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--out', default=None)
  ap.add_argument('--step', type=int, default=None, help='internal: run the step of this q in this process')
  ap.add_argument('--step-timeout', type=int, default=120)
  a = ap.parse_args()
  if a.step is not None:
    print(json.dumps(step(a.step, a.reps, a.warmup)))
    return 0
  env = dict(os.environ)
  for k in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):
    env[k] = str(min(16, int(env.get(k, '16') or 16)))
  res = []
  for q in (1, 4, 16):
    try:
      r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', str(q), '--reps', str(a.reps), '--warmup', str(a.warmup)],
                         capture_output=True, text=True, timeout=a.step_timeout, env=env)
    except subprocess.TimeoutExpired:
      print(f'qei_bench: the step q = {q} ran past {a.step_timeout} s; stopping', file=sys.stderr)
      return 124
    if r.returncode != 0:
      print(f'qei_bench: the step q = {q} ended with {r.returncode}; stopping\n{r.stderr[-2000:]}', file=sys.stderr)
      return r.returncode if r.returncode > 0 else 1
    res.append(json.loads(r.stdout.strip().splitlines()[-1]))
  line = json.dumps(res)
  print(line)
  if a.out:
    with open(a.out, 'w') as f:
      f.write(line + '\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())
