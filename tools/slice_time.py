"""Slice sampling of hyper-parameters: the cost of one lockstep round and of a whole run.  Per shape and S in {1, 2, 8, 32}:
  - device ms (hbo_profile, stage sums) of ONE hbo_nll_samples call over S samples, against S sequential value-only hbo_nll calls;
  - wall ms of one round as the sampler pays it (objectives.nll_log_densities: models built, one call, priors) and its host share
    (wall - device);
and per shape the wall time of a whole infer_parameters(method='slice_sample') run (burnin = nsamples = 50, 2 chains) with its round
count.  Shapes: 24 tasks x 100 points (fused path) and 2 x 1000 (blocked path), fp64, squared exponential + constant mean.

  python tools/slice_time.py [--reps 5] [--skip-run]"""
import argparse
import ctypes as C
import logging
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hyperbo_amd import _model, _native as nat  # noqa: E402
from hyperbo_amd.basics import definitions as defs  # noqa: E402
from hyperbo_amd.gp_utils import gp, kernel, mean, objectives, priors, utils  # noqa: E402


def device_ms(ctx):
  return sum(ms for name, (ms, _) in ctx.profile_get().items() if name != 'host_enqueue')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--skip-run', action='store_true', help='no whole slice_sample run')
  a = ap.parse_args()
  logging.getLogger().setLevel(logging.ERROR)   # (DEFAULT_PRIORS has no lengthscale prior: one warning per sample and evaluation)
  ctx = nat.default_context()
  lib = nat.lib()
  wf = utils.DEFAULT_WARP_FUNC
  cfg = {'priors': priors.DEFAULT_PRIORS}
  d = 4
  print('| shape | S | hbo_nll_samples device ms | S x hbo_nll device ms | ratio to one hbo_nll | round wall ms | round host ms |')
  print('|---|---|---|---|---|---|---|')
  runs = []
  for label, sizes in (('24 x 100', [100] * 24), ('2 x 1000', [1000] * 2)):
    rng = np.random.default_rng(0)
    ds = {}
    for i, n in enumerate(sizes):
      x = rng.uniform(size=(n, d))
      ds[i] = defs.SubDataset(x, np.sin(3 * x @ rng.normal(size=(d, 1))) + 0.1 * rng.normal(size=(n, 1)))
    dev = objectives.DeviceDataset(ds)
    for S in (1, 2, 8, 32):
      models = [{'constant': np.array(0.1 * s), 'lengthscale': np.full(d, 0.1 * s - 0.5), 'signal_variance': np.array(0.05 * s),
                 'noise_variance': np.array(-3.0 + 0.01 * s)} for s in range(S)]
      built = [_model.BuiltModel(mean.constant, kernel.squared_exponential, defs.GPParams(model=m, config=cfg), wf, np.float64, d)
               for m in models]
      structs = (nat.Model * S)(*[b.struct for b in built])
      tot = np.zeros(S)
      one = C.c_double(0.0)
      ctx.profile_enable(1)
      t_batch, t_seq, t_one = [], [], []
      for _ in range(a.reps):
        ctx.check(lib.hbo_nll_samples(ctx.handle, structs, S, dev._h, tot.ctypes.data_as(C.POINTER(C.c_double)), None))
        t_batch.append(device_ms(ctx))
        seq = 0.0
        for b in built:
          ctx.check(lib.hbo_nll(ctx.handle, b.ref(), dev._h, C.byref(one), None, None))
          seq += device_ms(ctx)
          if b is built[0]:
            t_one.append(device_ms(ctx))
        t_seq.append(seq)
      ctx.profile_enable(0)
      wall = []
      for _ in range(a.reps):
        t0 = time.perf_counter()
        objectives.nll_log_densities(mean.constant, kernel.squared_exponential, cfg, models, dev, wf)
        wall.append((time.perf_counter() - t0) * 1e3)
      tb, ts, t1, tw = np.median(t_batch), np.median(t_seq), np.median(t_one), np.median(wall)
      print(f'| {label} | {S} | {tb:.3f} | {ts:.3f} | {tb / t1:.2f} | {tw:.3f} | {tw - tb:.3f} |')
    dev.close()
    if not a.skip_run:
      rounds = []
      params = defs.GPParams(model={'constant': np.array(0.0), 'lengthscale': np.zeros(d), 'signal_variance': np.array(0.0),
                                    'noise_variance': np.array(-3.0)},
                             config={'method': 'slice_sample', 'burnin': 50, 'nsamples': 50, 'priors': priors.DEFAULT_PRIORS})
      t0 = time.perf_counter()
      gp.infer_parameters(mean.constant, kernel.squared_exponential, params, ds, warp_func=wf, key=0,
                          callback=lambda r, m, loss: rounds.append(r))
      runs.append((label, (time.perf_counter() - t0), len(rounds)))
  for label, sec, nr in runs:
    print(f'slice_sample run {label}: burnin 50, nsamples 50, 2 chains: {sec:.2f} s wall, {nr} rounds, {1e3 * sec / max(nr, 1):.3f} ms per round')


if __name__ == '__main__':
  main()
