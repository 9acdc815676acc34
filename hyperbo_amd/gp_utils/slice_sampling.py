"""Slice sampling of GP hyper-parameters: what config['method'] = 'slice_sample' asks infer_parameters for
(hyperbo/bo_utils/bayesopt.py:247-255, hyperbo/gp_utils/slice_sampling_test.py:56-153).  The reference snapshot names the method
but has no sampler behind it; this is Neal (2003), "Slice sampling", Ann. Statist. 31(3): stepping out (fig. 3) and shrinkage
(fig. 5) along a random direction of the flattened raw parameters.

One transition of one chain, in this order of draws from the chain's Generator:
  1. log y = f(x0) - E,  E ~ Exp(1)
  2. d = z / |z|,  z ~ N(0, I_P)
  3. L = -w u,  R = L + w,  u ~ U(0, 1)
  4. j = floor(m v),  k = m - 1 - j,  v ~ U(0, 1):  L -= w while j > 0 and f(x0 + L d) > log y (j -= 1 each time), likewise
     R += w while k > 0 and f(x0 + R d) > log y
  5. t = L + U (R - L), U ~ U(0, 1): accept x0 + t d if f > log y, else L = t (t < 0) or R = t -- at most SHRINK_MAX times;
     past that the chain stays at x0 (logged).
A NaN density counts as -inf (outside every slice).

The chains run in lockstep: every round collects the pending evaluations of all unfinished chains -- the two sides of the
stepping out go together, they are independent -- and hands them to ONE call of the batched log density.  Nothing else in a
transition depends on the round structure, so a chain's trajectory is the one it would have alone.
"""
import logging

import numpy as np

STEP_OUT_MAX = 8     # m: the interval grows to at most m w
SHRINK_MAX = 100     # shrinkage steps per transition before the chain keeps its point


def chain_seeds(rng, n_chains):
  """Per-chain SeedSequences: children of one SeedSequence seeded from `rng`.  Child c does not depend on n_chains."""
  ss = np.random.SeedSequence(int(rng.integers(np.iinfo(np.int64).max)))
  return ss.spawn(n_chains)


def _transition(x0, f0, rng, w):
  """Generator of one transition: yields lists of points, receives their log densities, returns (x, f, shrink_cap_hit)."""
  log_y = f0 - rng.standard_exponential()
  z = rng.standard_normal(x0.shape[0])
  d = z / np.linalg.norm(z)
  left = -w * rng.random()
  right = left + w
  j = int(np.floor(STEP_OUT_MAX * rng.random()))
  k = STEP_OUT_MAX - 1 - j
  open_l, open_r = j > 0, k > 0
  while open_l or open_r:
    pts = ([x0 + left * d] if open_l else []) + ([x0 + right * d] if open_r else [])
    vals = yield pts
    i = 0
    if open_l:
      if vals[0] > log_y:
        left -= w
        j -= 1
        open_l = j > 0
      else:
        open_l = False
      i = 1
    if open_r:
      if vals[i] > log_y:
        right += w
        k -= 1
        open_r = k > 0
      else:
        open_r = False
  for _ in range(SHRINK_MAX):
    t = left + rng.random() * (right - left)
    x1 = x0 + t * d
    f1, = yield [x1]
    if f1 > log_y:
      return x1, f1, False
    if t < 0:
      left = t
    else:
      right = t
  return x0, f0, True


def _chain(x0, f0, rng, n_steps, w, trace):
  x, f = x0, f0
  for it in range(n_steps):
    x, f, capped = yield from _transition(x, f, rng, w)
    if capped:
      logging.warning('slice sampling: no point of the slice found in %d shrinkage steps; the chain keeps its state (transition %d)',
                      SHRINK_MAX, it)
    trace.append((x, f))


def _as_log_density(values, count):
  v = np.asarray(values, dtype=np.float64).reshape(count)
  return np.where(np.isnan(v), -np.inf, v)


def slice_sample(log_density, x0, rng, n_chains, burnin, nsamples, step_size=1.0, callback=None):
  """Runs `n_chains` slice-sampling chains from x0 in lockstep.

  log_density: callable mapping a (K, P) array of points to their (K,) log densities -- all pending evaluations of a round in
    one call.  rng: numpy Generator; chain c draws from default_rng(chain_seeds(rng, n_chains)[c]).
  Discards `burnin` transitions per chain, keeps the next `nsamples`.  callback(round, x, f), if given, is called once per round
  with chain 0's current point and log density.
  Returns (samples (n_chains * nsamples, P), log densities (n_chains * nsamples,)), chain-major.
  Raises ValueError when the log density at x0 is not finite.
  """
  x0 = np.asarray(x0, dtype=np.float64).ravel().copy()
  f0 = float(_as_log_density(log_density(x0[None, :]), 1)[0])
  if not np.isfinite(f0):
    raise ValueError(f'slice sampling: the log density at the initial parameters is {f0}; it must be finite.')
  n_steps = burnin + nsamples
  rngs = [np.random.default_rng(s) for s in chain_seeds(rng, n_chains)]
  traces = [[] for _ in range(n_chains)]
  chains = [_chain(x0, f0, rngs[c], n_steps, float(step_size), traces[c]) for c in range(n_chains)]
  pending = []
  for c, g in enumerate(chains):
    try:
      pending.append(next(g))
    except StopIteration:
      pending.append(None)
  rnd = 0
  while any(p is not None for p in pending):
    active = [c for c in range(n_chains) if pending[c] is not None]
    pts = np.stack([p for c in active for p in pending[c]])
    vals = _as_log_density(log_density(pts), pts.shape[0])
    pos = 0
    for c in active:
      n = len(pending[c])
      try:
        pending[c] = chains[c].send(list(vals[pos:pos + n]))
      except StopIteration:
        pending[c] = None
      pos += n
    if callback is not None:
      x, f = traces[0][-1] if traces[0] else (x0, f0)
      callback(rnd, x, f)
    rnd += 1
  kept = [tr[burnin:] for tr in traces]
  xs = np.array([x for tr in kept for x, _ in tr]).reshape(n_chains * nsamples, x0.shape[0])
  fs = np.array([f for tr in kept for _, f in tr], dtype=np.float64)
  return xs, fs
