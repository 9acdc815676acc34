"""CPU side of the tests of the acquisition gradient and the device maximiser beyond one 128-row block (csrc/acq_blocked.hip:
acq_blk_k_kernel, acq_blk_fwd_kernel, acq_blk_trans_kernel, acq_blk_finish_kernel; hbo_acq_grad_samples_blocked,
hbo_acq_maximize_blocked).  Shared by tests/test_acq_blocked_host.py (this file judged on its own) and tests/test_gpu_acq_blocked.py
(the device against it).  Nothing here is new machinery: the cases are acq_grad_cases.Case (one cache: inputs, reference, ratios,
conditions, route) and acq_opt_oracle.Case (S samples and the maximiser: inputs, oracle_value_and_grad, oracle_run).

  GRAD_CASES      40 cases: n across the edges of the blocked kernels, M across the groups of eight, D across the G = 256, 32, 4, 1 row
                  groups of the finish kernel, S, all four covariances x three means, fp64 and fp32, rotated with co-prime periods.
                  Every case is judged for UCB(3), EI and PI (acq_grad_cases.reference).
  companions(gc)  the other S - 1 caches of a call with S = 3: the same family and shapes from other draws (group letters 'Y', 'Z')
  blocked_route   the device's route restated in NumPy, block by block: l = W k by 128-row tiles, beta = W^T l by 64 columns over
                  256-row chunks, then acq_grad_cases.route on them
  MUTANTS         that route with one failure this structure could have, each
  OPT_CASES       the maximiser at n = 129, 257, 385
"""
import functools
from typing import NamedTuple

import numpy as np

import acq_grad_cases as G
import acq_opt_oracle as ao

NS = [129, 192, 193, 255, 256, 257, 384, 385, 513]   # one row in the second block; the 64-column workgroup edge of the transposed
                                                     # product; its 256-row chunk edge and the half last chunk; three to five blocks
MS = [1, 7, 8, 9, 17]                                # the groups of eight
DS = [1, 5, 33, 256]                                 # G = 256, 32, 4, 1
SS = [1, 3]
MEANS = ['zero', 'constant', 'linear']
N_CASES = 40
DEFAULT_GROUP = 'G'

# case index -> another group letter (part of acq_grad_cases' seed) for a case that breaks one of acq_grad_cases.conditions with 'G';
# test_acq_blocked_host.py::test_every_case_meets_the_conditions names what is broken.  No case of the 40 needed another draw.
RESEED = {}


class GradCase(NamedTuple):
  index: int
  case: G.Case
  S: int

  @property
  def id(self):
    return f'{self.index:02d}-S{self.S}-{self.case.id}'


def _grad_cases():
  out = []
  for i in range(N_CASES):
    kname, mname = G.KERNELS[i % 4], MEANS[i % 3]
    n, m, d, s = NS[i % 9], MS[i % 5], DS[(i + i // 4) % 4], SS[(i // 3) % 2]
    dtype = 'fp32' if i % 7 in (1, 3, 5) else 'fp64'
    ls = 'none' if kname == 'dot_product' else 'ard'
    out.append(GradCase(i, G.Case(RESEED.get(i, DEFAULT_GROUP), kname, False, mname, False, n, m, d, (), ls, dtype), s))
  return out


GRAD_CASES = _grad_cases()


def companions(gc):
  """The cases of the other samples of the call (S - 1 of them): same family, same shapes, other draws."""
  return [gc.case._replace(group=letter) for letter in 'YZ'[:gc.S - 1]]


# ---- the blocked route, restated -------------------------------------------------------------------------------------------------
def blocked_l(W, k, drop_off_diagonal=False):
  """l = W k tile by tile of 128 rows x 128 columns, the tiles of a row block added in rising column order."""
  n = W.shape[0]
  l = np.zeros_like(k)
  for r0 in range(0, n, 128):
    r1 = min(r0 + 128, n)
    for c0 in range(0, r1, 128):
      if drop_off_diagonal and c0 != r0:
        continue
      c1 = min(c0 + 128, n)
      l[r0:r1] += np.tril(W)[r0:r1, c0:c1] @ k[c0:c1]
  return l


def blocked_beta(W, l, row_limit=None):
  """beta = W^T l, 64 columns at a time over 256-row chunks from the chunk of the diagonal on (rows < row_limit only)."""
  n = W.shape[0]
  lim = n if row_limit is None else min(n, row_limit)
  beta = np.zeros_like(l)
  Wl = np.tril(W)
  for j0 in range(0, n, 64):
    j1 = min(j0 + 64, n)
    for rc in range(j0 // 256 * 256, lim, 256):
      r1 = min(rc + 256, lim)
      beta[j0:j1] += Wl[rc:r1, j0:j1].T @ l[rc:r1]
  return beta


def _lb(case):
  p = G.parts(case)
  l = blocked_l(p.W, p.kxq)
  return p, l, blocked_beta(p.W, l)


def blocked_route(case, acq, param):
  """Value (M,) and gradient (M, d) by acq_grad_cases.route with l and beta formed block by block."""
  _, l, beta = _lb(case)
  return G.route(case, acq, param, l=l, beta=beta)


def mutant_l_diagonal_tiles(case, acq, param):
  """l = W k without the off-diagonal tiles of W (a forward product that stops at its own row block)."""
  p = G.parts(case)
  l = blocked_l(p.W, p.kxq, drop_off_diagonal=True)
  return G.route(case, acq, param, l=l, beta=blocked_beta(p.W, l))


def mutant_beta_last_block(case, acq, param):
  """beta = W^T l misses the rows of the last 128-row block."""
  p, l, _ = _lb(case)
  return G.route(case, acq, param, l=l, beta=blocked_beta(p.W, l, row_limit=case.npad - 128))


def mutant_beta_half_chunk(case, acq, param):
  """beta = W^T l misses the rows of the half last 256-row chunk (npad an odd multiple of 128)."""
  p, l, _ = _lb(case)
  return G.route(case, acq, param, l=l, beta=blocked_beta(p.W, l, row_limit=case.npad // 256 * 256))


def mutant_ll_first_chunk(case, acq, param):
  """|l|^2 is summed over the first 256-row chunk only (beta from the whole l)."""
  _, l, beta = _lb(case)
  cut = l.copy()
  cut[256:] = 0.0
  return G.route(case, acq, param, l=cut, beta=beta)


def mutant_grad_first_chunk(case, acq, param):
  """The feature gradient drops the observation rows from 256 on (an accumulator that is not kept across chunks)."""
  _, l, beta = _lb(case)
  return G.route(case, acq, param, l=l, beta=beta, rowmask=(np.arange(case.n) < 256).astype(np.float64))


def mutant_neighbour_k(case, acq, param):
  """The second query of a group of eight reads its neighbour's k: its l and beta are the first query's."""
  _, l, beta = _lb(case)
  l, beta = l.copy(), beta.copy()
  l[:, 1], beta[:, 1] = l[:, 0], beta[:, 0]
  return G.route(case, acq, param, l=l, beta=beta)


MUTANTS = {'l_diagonal_tiles': mutant_l_diagonal_tiles, 'beta_last_block': mutant_beta_last_block, 'beta_half_chunk': mutant_beta_half_chunk,
           'll_first_chunk': mutant_ll_first_chunk, 'grad_first_chunk': mutant_grad_first_chunk, 'neighbour_k': mutant_neighbour_k}


def applicable(name, case):
  """Whether the mutant's failure can exist at the case's shape."""
  if name == 'beta_half_chunk':
    return (case.npad // 128) % 2 == 1
  if name in ('ll_first_chunk', 'grad_first_chunk'):
    return case.n > 256
  if name == 'neighbour_k':
    return case.M >= 2
  return True


# ---- the maximiser -----------------------------------------------------------------------------------------------------------------
# n = 129 (one row in the second block), 257 (one row in the second 256-row chunk), 385 (four blocks, the half chunk); S, R, D and the
# acquisition vary with them.  seed: another draw where the first one puts a decision of some start within a relative 1e-6 of its
# threshold (test_acq_blocked_host.py::test_maximiser_cases_clear_their_thresholds); none needed one.
OPT_CASES = [
    ao.Case('blocked-matern52-constant-ei-n129-D3-S3-R9', 'matern52', 'constant', 'ei', 129, 3, 3, 9),
    ao.Case('blocked-matern32-zero-ucb-n257-D5-S1-R9', 'matern32', 'zero', 'ucb', 257, 5, 1, 9),
    ao.Case('blocked-matern52-linear-pi-n385-D3-S3-R1', 'matern52', 'linear', 'pi', 385, 3, 3, 1),
]
OPT_BY_NAME = {c.name: c for c in OPT_CASES}


@functools.lru_cache(maxsize=None)
def opt_run(case, r):
  """acq_opt_oracle.oracle_run (shared, not to be written to)."""
  return ao.oracle_run(case, r)
