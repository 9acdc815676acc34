"""Wall time of the simulated BO loop with config['bo_on_device'] off (the host loop: one acquisition call, one np.argmax and one
append per iteration) and on (hbo_bo_simulated: every iteration on the device), same process, same seeded problem:

  python tools/bo_loop_wall.py                       the table of profiles/bo_device.md: 100 iterations from an empty sub-dataset, D = 16,
                                                     squared exponential + constant mean, fp64 and fp32, M = 1000 and 16384; one run
                                                     (R = 1), and R = 115 runs through simulated_bayesopt_batch against 115 host loops
  python tools/bo_loop_wall.py --rocprof DIR         one `rocprofv3 --kernel-trace --stats` run of its own (a child process running
                                                     --trace below) and the two kernels' rows of its statistics
  python tools/bo_loop_wall.py --trace               `--calls` device loops of one shape (--M --R --dtype) after a warm-up, nothing else
  options: --iters 100 --D 16 --repeats 5 --batch 115 --sizes 1000,16384 --json FILE

Every timed call ends in a stream synchronisation inside the library (the host loop's last acquisition call copies its values back;
the device loop copies its results back), so the host clock brackets whole loops.  Each side is warmed up once per shape; the repeats
alternate off / on so that drift hits both alike; the spread reported is (max - min) / median over the repeats of a side.  The two
sides' selections are compared as well (fp32 may differ where two candidates are closer than its rounding)."""
import argparse
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def inv_softplus(v):
  return np.log(np.expm1(np.asarray(v, dtype=np.float64)))


def problem(M, D, dtype, seed):
  """(pool, model factory): a pool of M pre-evaluated candidates, and fresh models (squared exponential + constant mean) whose test
  sub-dataset does not exist yet -- what run_bayesopt starts a test task from."""
  from hyperbo_amd.basics import definitions as defs
  from hyperbo_amd.gp_utils import gp, kernel, mean, utils
  rng = np.random.default_rng(seed)
  x = rng.uniform(size=(M + 50, D)); w = rng.normal(size=D) / np.sqrt(D)
  y = np.sin(2 * np.pi * x @ w)[:, None] + 0.1 * rng.normal(size=(M + 50, 1))
  x, y = x.astype(dtype), y.astype(dtype)
  pool = defs.SubDataset(x[:M], y[:M])
  params = {'lengthscale': inv_softplus(np.full(D, 0.6)) + 0.1 * rng.normal(size=D), 'signal_variance': np.array(inv_softplus(1.0)),
            'noise_variance': np.array(inv_softplus(1e-2)), 'constant': np.array(0.1)}
  params = {k: np.asarray(v, dtype=dtype) for k, v in params.items()}

  def model(on_device):
    return gp.GP({0: defs.SubDataset(x[M:], y[M:])}, mean.constant, kernel.squared_exponential,
                 defs.GPParams(model=dict(params), config={'bo_on_device': bool(on_device)}), utils.DEFAULT_WARP_FUNC)
  return pool, model


def stat(ts):
  return float(np.median(ts)), float((max(ts) - min(ts)) / np.median(ts))


def measure(M, R, D, dtype, iters, repeats):
  from hyperbo_amd.bo_utils import acfun, bayesopt
  probs = [problem(M, D, dtype, 100 + r) for r in range(R)]
  fn = acfun.expected_improvement

  def host():
    return [bayesopt.simulated_bayesopt(mk(False), 'test', pool, fn, iters) for pool, mk in probs]

  def device():
    if R == 1:
      return [bayesopt.simulated_bayesopt(probs[0][1](True), 'test', probs[0][0], fn, iters)]
    return bayesopt.simulated_bayesopt_batch([(mk(False), 'test', pool, fn) for pool, mk in probs], iters)

  sides = {'off': host, 'on': device}
  res, last = {'off': [], 'on': []}, {}
  for name, call in sides.items():
    call()   # warm-up: workspaces, code objects
  for _ in range(repeats):
    for name, call in sides.items():
      t0 = time.perf_counter()
      last[name] = call()
      res[name].append(1e3 * (time.perf_counter() - t0))
  same = sum(int(np.array_equal(a.x, b.x)) for a, b in zip(last['off'], last['on']))
  (off, s_off), (on, s_on) = stat(res['off']), stat(res['on'])
  row = dict(dtype=np.dtype(dtype).name, M=M, R=R, iters=iters, D=D, off_ms=off, off_spread=s_off, on_ms=on, on_spread=s_on, ratio=off / on,
             same_selections=same, repeats=repeats)
  print(f'| {row["dtype"]} | {M} | {R} | {off:.2f} | {100 * s_off:.1f} % | {on:.2f} | {100 * s_on:.1f} % | {off / on:.2f} | {same} / {R} |', flush=True)
  return row


def trace(M, R, D, dtype, iters, calls):
  from hyperbo_amd.bo_utils import acfun, bayesopt
  probs = [problem(M, D, dtype, 100 + r) for r in range(R)]
  call = lambda: bayesopt.simulated_bayesopt_batch([(mk(False), 'test', pool, acfun.expected_improvement) for pool, mk in probs], iters)
  call()
  t0 = time.perf_counter()
  for _ in range(calls):
    call()
  print(f'trace: {np.dtype(dtype).name} M={M} R={R} iters={iters}: {calls} calls after 1 warm-up, '
        f'{1e3 * (time.perf_counter() - t0) / calls:.2f} ms per call; launches per call: {iters + 1} bo_row_kernel, {iters} bo_select_kernel')


def rocprof(out_dir, a):
  """The kernel statistics of `--trace` from a rocprofv3 run of its own: a fresh child process, nothing else on the GPU from here."""
  os.makedirs(out_dir, exist_ok=True)
  cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '--', sys.executable, os.path.abspath(__file__),
         '--trace', '--M', str(a.M), '--R', str(a.R), '--dtype', a.dtype, '--iters', str(a.iters), '--D', str(a.D), '--calls', str(a.calls)]
  out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
  print(out.stdout.strip().splitlines()[-1] if out.stdout.strip() else out.stderr[-2000:])
  if out.returncode != 0:
    raise SystemExit(f'rocprofv3 exited with {out.returncode}: {out.stderr[-2000:]}')
  files = sorted(glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True))
  if not files:
    raise SystemExit('no *kernel_stats.csv under ' + out_dir)
  lines = open(files[-1]).read().splitlines()
  print(lines[0])
  for line in lines[1:]:
    if 'bo_row_kernel' in line or 'bo_select_kernel' in line:
      print(line)


if __name__ == '__main__':
  ap = argparse.ArgumentParser()
  ap.add_argument('--trace', action='store_true'); ap.add_argument('--rocprof')
  ap.add_argument('--M', type=int, default=1000); ap.add_argument('--R', type=int, default=1); ap.add_argument('--dtype', default='float64')
  ap.add_argument('--calls', type=int, default=20)
  ap.add_argument('--iters', type=int, default=100); ap.add_argument('--D', type=int, default=16); ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--batch', type=int, default=115); ap.add_argument('--sizes', default='1000,16384'); ap.add_argument('--json')
  a = ap.parse_args()
  if a.rocprof:
    rocprof(a.rocprof, a)
  elif a.trace:
    trace(a.M, a.R, a.D, np.dtype(a.dtype), a.iters, a.calls)
  else:
    print('| dtype | M | R | off ms | off spread | on ms | on spread | off / on | same selections |')
    print('|---|---|---|---|---|---|---|---|---|')
    rows = []
    for dtype in (np.float64, np.float32):
      for M in [int(s) for s in a.sizes.split(',')]:
        for R in (1, a.batch):
          rows.append(measure(M, R, a.D, dtype, a.iters, a.repeats))
    if a.json:
      with open(a.json, 'w') as f:
        json.dump(rows, f, indent=1)
