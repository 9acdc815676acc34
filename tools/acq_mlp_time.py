"""ms per evaluation of the acquisition function and its gradient for a GP on an MLP basis (matern52_mlp + linear_mlp, EI, D = 6): the
per-sample route without config['acq_mlp'] -- one hbo_acq_grad per parameter sample, code this feature does not touch -- against one
hbo_acq_grad_samples_mlp call (csrc/acq_mlp.h), same process, same seeded model and queries; and the rounds per second of
ac_func.maximize (hbo_acq_maximize_mlp).

  python tools/acq_mlp_time.py             stacks (12, 33) and (256, 256) x S in {1 (GP), 8, 32}, n = 100, M = 16; then n = 300
  options: --window 0.3 --repeats 3 --n --M --D

`entry point alone`: hbo_acq_grad_samples_mlp over models and factors that are already built (acfun._fused_value_and_grad), without
the per-call host work of value_and_grad -- for an HGP the content fingerprint of the S parameter samples, which hashes every weight.

Both sides are warmed up first; the windows alternate between the sides; a window holds at least one call; the spread reported is
(max - min) / median over the repeats of a side.  Both sides end in the entry point's own device synchronise."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from hyperbo_amd import _native as nat
from hyperbo_amd.basics import definitions as defs
from hyperbo_amd.bo_utils import acfun
from hyperbo_amd.gp_utils import gp, kernel, mean, utils
from tools.acq_fused_time import inv_softplus, window

AC = acfun.expected_improvement


def make(S, n, M, D, feats, config, seed=7):
  """An HGP of S parameter samples (S = 1: a plain GP) with weights of their own over n observations, and M queries."""
  rng = np.random.default_rng(seed)
  x = rng.uniform(size=(n, D)); w = rng.normal(size=D)
  y = np.sin(2 * np.pi * x @ w)[:, None] + 0.1 * rng.normal(size=(n, 1))
  xq = rng.uniform(size=(M, D))

  def smp():
    m = {'lengthscale': inv_softplus(0.5 * np.sqrt(feats[-1]) * np.exp(rng.uniform(-0.4, 0.4, size=feats[-1]))), 'signal_variance': inv_softplus(0.8),
         'noise_variance': inv_softplus(0.1), 'linear_mean': {'kernel': rng.normal(size=(feats[-1], 1)) / np.sqrt(feats[-1]), 'bias': rng.normal(size=1)},
         'mlp_params': {}}
    fin = D
    for l, f in enumerate(feats):
      m['mlp_params'][f'Dense_{l}'] = {'kernel': rng.normal(size=(fin, f)) * (2.0 / np.sqrt(fin)), 'bias': rng.normal(size=f) * 0.1}
      fin = f
    return m
  samples = [smp() for _ in range(S)]
  data = {0: defs.SubDataset(x, y), 1: defs.SubDataset(x[:5], y[:5])}
  cfg = dict(config, mlp_features=tuple(feats))
  if S == 1:
    return gp.GP(data, mean.linear_mlp, kernel.matern52_mlp, defs.GPParams(model=samples[0], config=cfg), utils.DEFAULT_WARP_FUNC), xq
  return gp.HGP(data, mean.linear_mlp, kernel.matern52_mlp, defs.GPParams(model=samples[0], samples=samples, config=cfg), utils.DEFAULT_WARP_FUNC), xq


def _stat(ts):
  return float(np.median(ts)), float((max(ts) - min(ts)) / np.median(ts))


def measure(S, n, M, D, feats, seconds, repeats):
  ctx = nat.default_context()
  ctx.set_option('acq_fused', 1)
  old, xq = make(S, n, M, D, feats, {})
  new, _ = make(S, n, M, D, feats, {'acq_mlp': True})
  ev = lambda model: (lambda: AC.value_and_grad(model=model, sub_dataset_key=0, x_queries=xq))
  a, b = ev(old), ev(new)
  try:
    for f in (a, b):
      f(); f()
    (vo, go), (vn, gn) = a(), b()
    dv = float(np.max(np.abs(vo - vn) / np.maximum(np.abs(vo), 1e-300))); dg = float(np.max(np.abs(go - gn)) / max(np.max(np.abs(go)), 1e-3))
    res = ([], [])
    for _ in range(repeats):
      res[0].append(window(a, seconds)); res[1].append(window(b, seconds))
    (ta, sa), (tb, sb) = _stat(res[0]), _stat(res[1])
    # the entry point alone, over what value_and_grad builds per call
    if S == 1:
      handle, _, bm, noise, scale = acfun._single_model(new, 0, xq)
      built, handles, noises = [bm], [handle], [noise]
    else:
      samples = new.get_model_params_samples()
      built, noises = acfun._sample_models(new, samples, np.float64)
      handles = acfun._hgp_sample_caches(new, 0, samples, np.float64)
      _, scale = new.predict_noise_and_scale(True, True)
    raw = lambda: acfun._fused_value_and_grad(built, handles, noises, xq, nat.ACQ_EI, 0.5, scale, acfun._ROUTES['mlp'])
    raw(); raw()
    tr, sr = _stat([window(raw, seconds) for _ in range(repeats)])
    # the maximiser: R = 16 starts, rounds (evaluations of every start) per second over whole maximisations
    starts = np.ascontiguousarray(xq[:16])
    rounds = [0]

    def mx():
      _, _, info = AC.maximize(model=new, sub_dataset_key=0, x_init=starts)
      rounds[0] = int(np.max(info['evals']))
    mx(); mx()
    tm = [window(mx, seconds) for _ in range(repeats)]
    tmed, sm = _stat(tm)
    # a maximisation runs whole segments of acfun.ACQ_OPT_SEGMENT rounds until every start has stopped
    seg = acfun.ACQ_OPT_SEGMENT
    ran = -(-rounds[0] // seg) * seg
    print(f'| {"x".join(map(str, feats))} | {n} | {S} | {M} | {ta:.3f} | {100 * sa:.1f} % | {tb:.3f} | {100 * sb:.1f} % | {ta / tb:.2f} | {tr:.3f} | {100 * sr:.1f} % | {dv:.1e} / {dg:.1e} | '
          f'{tmed:.2f} | {100 * sm:.1f} % | {ran} | {1e3 * ran / tmed:.0f} |', flush=True)
  finally:
    ctx.set_option('acq_fused', 0)
    if S > 1:
      acfun.drop_sample_caches(old); acfun.drop_sample_caches(new)


if __name__ == '__main__':
  ap = argparse.ArgumentParser()
  ap.add_argument('--n', type=int); ap.add_argument('--M', type=int, default=16); ap.add_argument('--D', type=int, default=6)
  ap.add_argument('--window', type=float, default=0.3); ap.add_argument('--repeats', type=int, default=3)
  a = ap.parse_args()
  print('| stack | n | S | M | loop ms / evaluation | spread | mlp ms / evaluation | spread | loop / mlp | entry point alone ms | spread | value / gradient difference | '
        'ms / maximisation (R = 16) | spread | rounds run | rounds / s |')
  print('|' + '---|' * 16)
  for n in ([a.n] if a.n else (100, 300)):
    for feats in ((12, 33), (256, 256)):
      for S in (1, 8, 32):
        measure(S, n, a.M, a.D, feats, a.window, a.repeats)
