"""Test-side restatement of the slice sampler of hyperbo_amd/gp_utils/slice_sampling.py: Neal (2003) stepping out and shrinkage
along a random direction, one chain after the other and one evaluation at a time -- the textbook sequential form, against which
the library's lockstep rounds (both stepping-out sides per round, all chains in one batched call) must give the same trajectories.
Same draws in the same order: Exp(1), N(0, I_P), U(0, 1) for the interval, U(0, 1) for the step-out split, U(0, 1) per shrinkage."""
import numpy as np


def chain_rngs(rng, n_chains):
  ss = np.random.SeedSequence(int(rng.integers(np.iinfo(np.int64).max)))
  return [np.random.default_rng(child) for child in ss.spawn(n_chains)]


def slice_sample(log_density, x0, rng, n_chains, burnin, nsamples, w=1.0, m=8, max_shrink=100):
  """log_density: ONE point (P,) -> float.  Returns the kept points (n_chains * nsamples, P), chain-major."""
  def f(x):
    v = float(log_density(x))
    return -np.inf if np.isnan(v) else v
  x0 = np.asarray(x0, dtype=np.float64).ravel()
  f0 = f(x0)
  kept = []
  for rng_c in chain_rngs(rng, n_chains):
    x, fx = x0.copy(), f0
    for it in range(burnin + nsamples):
      log_y = fx - rng_c.standard_exponential()
      z = rng_c.standard_normal(x.shape[0])
      d = z / np.linalg.norm(z)
      lo = -w * rng_c.random()
      hi = lo + w
      j = int(np.floor(m * rng_c.random()))
      k = m - 1 - j
      while j > 0 and f(x + lo * d) > log_y:
        lo -= w
        j -= 1
      while k > 0 and f(x + hi * d) > log_y:
        hi += w
        k -= 1
      for _ in range(max_shrink):
        t = lo + rng_c.random() * (hi - lo)
        x1 = x + t * d
        f1 = f(x1)
        if f1 > log_y:
          x, fx = x1, f1
          break
        if t < 0:
          lo = t
        else:
          hi = t
      if it >= burnin:
        kept.append(x.copy())
  return np.array(kept).reshape(n_chains * nsamples, x0.shape[0])
