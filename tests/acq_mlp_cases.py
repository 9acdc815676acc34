"""CPU side of the tests of hbo_acq_grad_samples_mlp and hbo_acq_maximize_mlp (csrc/acq_mlp.h inside csrc/acq_small.hip and
csrc/acq_blocked.hip): the acquisition gradient and the device maximiser for kernels on an MLP basis and the linear_mlp mean.  Shared by
tests/test_acq_mlp_cases_host.py (this file judged on its own) and tests/test_gpu_acq_mlp.py (the device against it).

Cases are acq_grad_cases.Case, unchanged: inputs, oracle_setup, reference, ratios, conditions and the project's bounds apply as they
are.  d = 5, matern52, ard, both dtypes and the three pairings of acq_grad_cases.B_PAIRINGS unless noted:

  S  stacks               n = 100, M = 9: every layer width on both sides of the 64-lane wave and the 256-thread workgroup, depth 8
  T  kernels              n = 100, M = 9, stack (12, 33), MLP kernel + linear_mlp: every kernel with each of its length-scale forms
  U  n and M              stack (12, 33), MLP kernel + linear_mlp: n across the waves of the one-launch kernel, M = 1 and 9
  V  input width          n = 100, M = 9, stack (12, 33): d = 1, 17, 64, 256
  L  n beyond one block   M = 20: n = 129, 257, 385 (the blocked route), two stacks, and the dot product

The group letter is part of a case's seed.  route() is the device's route restated in NumPy for ANY of a case's parameter samples
(sample 0 is the case's own model), with the handles the MUTANTS turn; it is first held against the oracle."""
import functools
from typing import NamedTuple

import numpy as np
import scipy.linalg as spla

import acq_grad_cases as G
import acq_opt_oracle as ao
from oracle import hyperbo_oracle as o

Case = G.Case
WFO, SCALE = G.WFO, G.SCALE
S_STACKS = [(12, 17), (12, 33), (12, 64), (12, 256), (40, 17), (7, 40, 9, 33), (256, 256), (9,) * 8]
U_SIZES = [1, 2, 63, 64, 65, 127, 128]
V_WIDTHS = [1, 17, 64, 256]
L_SIZES = [129, 257, 385]
L_STACKS = [(12, 33), (7, 40, 9, 33)]
PAIRINGS = G.B_PAIRINGS
FULL = (True, 'linear_mlp')

CASES_S = [Case('S', 'matern52', mk, mn, False, 100, 9, 5, st, 'ard', dt) for st in S_STACKS for (mk, mn) in PAIRINGS for dt in G.DTYPES]
CASES_T = [Case('T', k, True, 'linear_mlp', False, 100, 9, 5, (12, 33), ls, dt) for k in G.KERNELS for ls in G._ls_forms(k) for dt in G.DTYPES]
CASES_U = [Case('U', 'matern52', True, 'linear_mlp', False, n, M, 5, (12, 33), 'ard', dt) for n in U_SIZES for M in (1, 9) for dt in G.DTYPES]
CASES_V = [Case('V', 'matern52', mk, mn, False, 100, 9, d, (12, 33), 'ard', dt) for d in V_WIDTHS for (mk, mn) in PAIRINGS for dt in G.DTYPES]
CASES_L = ([Case('L', 'matern52', mk, mn, False, n, 20, 5, st, 'ard', dt) for n in L_SIZES for st in L_STACKS for (mk, mn) in PAIRINGS for dt in G.DTYPES] +
           [Case('L', 'dot_product', True, 'linear_mlp', False, n, 20, 5, (12, 33), 'none', dt) for n in L_SIZES for dt in G.DTYPES])
CASES = CASES_S + CASES_T + CASES_U + CASES_V + CASES_L
assert len(CASES) == 156 and len(set(CASES)) == 156
SMALL = [c for c in CASES if c.n <= 128]      # the one-launch route
LARGE = [c for c in CASES if c.n > 128]       # the blocked route

# ---- S = 3 parameter samples: one case per stack of S, U at n = 128 and L at n = 129 (MLP kernel + linear_mlp, both dtypes) ---------
N_SAMPLES = 3
MULTI = ([c for c in CASES_S if (c.mlp_k, c.mname) == FULL] + [c for c in CASES_U if c.n == 128 and c.M == 9] +
         [c for c in CASES_L if c.n == 129 and c.kname == 'matern52' and c.feats == (12, 33) and (c.mlp_k, c.mname) == FULL])


@functools.lru_cache(maxsize=None)
def sample_models(case):
  """N_SAMPLES models of the case's family in its dtype: the case's own, then draws from seeds of their own (distinct MLP weights,
  length-scales and mean weights).  Observations and queries are the case's."""
  out = [G.inputs(case)[0]]
  for i in range(1, N_SAMPLES):
    out.append(G.cast(G._model(np.random.default_rng(G._seed(case) + [7000 + i]), case), case.np_dtype))
  return out


class Sample(NamedTuple):
  po: object
  noise: float


@functools.lru_cache(maxsize=None)
def sample_setup(case, i=0):
  po = o.GPParams(model=G.cast(sample_models(case)[i], np.float64), config=G.config(case))
  return Sample(po, float(np.squeeze(o.retrieve_params(po, ['noise_variance'], WFO)[0])))


def _fns(case):
  return getattr(o, case.mname), getattr(o, case.kname + ('_mlp' if case.mlp_k else ''))


@functools.lru_cache(maxsize=None)
def sample_reference(case, i, acq, param):
  """acq_grad_cases.Ref of one acquisition for sample i of the case at the case's queries (sample 0 at the case's own parameter is
  acq_grad_cases.reference)."""
  st, sm = G.oracle_setup(case), sample_setup(case, i)
  mo, ko = _fns(case)
  v, g = o.acquisition_value_and_grad(acq, mo, ko, sm.po, st.x, st.y, st.xq, param, WFO, add_noise=sm.noise, scale=SCALE)
  mu, var = o.predict(mo, ko, sm.po, st.x, st.y, st.xq, WFO)
  mu, var = np.asarray(mu, dtype=np.float64).ravel(), np.asarray(var, dtype=np.float64).ravel()
  sd = np.sqrt((var + sm.noise) * SCALE)
  return G.Ref(float(param), mu, sd, {acq: v[:, 0]}, {acq: g}, {acq: np.zeros_like(mu) if acq == 'ucb' else (param - mu) / sd})


# ---- the device's route, restated --------------------------------------------------------------------------------------------------
def _forward(mlp, x, transpose=None, trunc=False):
  """Activations [input, layer 0, ...].  transpose: that layer's (square) weights read as [out][in]; trunc: sums stop at input index
  64 and outputs from 64 on are never written (zeros)."""
  acts = [x]
  for l in range(len(mlp)):
    w, b = np.asarray(mlp[f'Dense_{l}']['kernel'], dtype=np.float64), np.asarray(mlp[f'Dense_{l}']['bias'], dtype=np.float64)
    w = w.T if l == transpose else w
    h = acts[-1]
    z = (h[:, :64] @ w[:64] if trunc else h @ w) + b
    a = np.tanh(z)
    if trunc:
      a[:, 64:] = 0.0
    acts.append(a)
  return acts


def route(case, acq, param, sample=0, weights_of=None, skip_tanh=None, drop_mlp_mean=False, drop_raw_mean=False, transpose=None, trunc=False):
  """Value (M,) and gradient (M, d) of sample `sample` by the device's route: forward pass of the query, k, l = W k, beta = W^T l in the
  kernel's own space, the mean in the mean's own space, the backward pass on the sum of the feature-space pieces, plus the raw-space
  pieces.  The keyword arguments are the mutants' handles: the query's passes with another sample's weights, a layer whose tanh' is
  skipped, the mean's gradient terms dropped, a layer read transposed, a truncated forward."""
  st, sm = G.oracle_setup(case), sample_setup(case, sample)
  model = sm.po.model
  mlp_q = sample_setup(case, sample if weights_of is None else weights_of).po.model['mlp_params']
  kbase = getattr(o, case.kname)
  acts = _forward(mlp_q, st.xq, transpose, trunc)
  fq = acts[-1] if case.mlp_k else st.xq
  fo = o.mlp_apply(model['mlp_params'], st.x) if case.mlp_k else st.x
  mo, ko = _fns(case)
  chol, kinvy, _ = o.solve_gp_linear_system(mo, ko, sm.po, st.x, st.y, WFO)
  W = spla.solve_triangular(chol, np.eye(case.n), lower=True, check_finite=False)
  alpha = kinvy[:, 0]
  kxq = np.asarray(kbase(sm.po, fo, fq, warp_func=WFO), dtype=np.float64)
  kdiag = np.asarray(kbase(sm.po, fq, warp_func=WFO, diag=True), dtype=np.float64)
  wlin = np.asarray(model['linear_mean']['kernel'], dtype=np.float64)[:, 0]
  blin = float(np.squeeze(model['linear_mean']['bias']))
  mu0 = (acts[-1] if case.mname == 'linear_mlp' else st.xq) @ wlin + blin
  l = W @ kxq
  beta = W.T @ l
  mu, var = kxq.T @ alpha + mu0, kdiag - np.sum(l * l, axis=0)
  with np.errstate(invalid='ignore'):
    sd = np.sqrt((var + sm.noise) * SCALE)
  if acq == 'ei':
    u = (mu - param) / sd
    val, a_mu, a_sd = sd * (o._norm_pdf(u) + u * o._norm_cdf(u)), o._norm_cdf(u), o._norm_pdf(u)
  elif acq == 'pi':
    val, a_mu, a_sd = (mu - param) / sd, 1.0 / sd, -(mu - param) / sd**2
  else:
    val, a_mu, a_sd = mu + param * sd, np.ones_like(mu), np.full_like(mu, param)
  a_var = a_sd / (2 * sd) * SCALE
  coef = (a_mu[None, :] * alpha[:, None] - 2.0 * a_var[None, :] * beta).T      # (M, n)
  if case.kname == 'dot_product':
    s2 = float(np.squeeze(o.retrieve_params(sm.po, ['dot_prod_sigma'], WFO)[0]))**2
    gfeat = (a_var * 2.0 / s2)[:, None] * fq + coef @ fo / s2
  else:
    ls, sv = o.retrieve_params(sm.po, ['lengthscale', 'signal_variance'], WFO)
    ls = np.broadcast_to(np.asarray(ls, dtype=np.float64).reshape(-1), (fq.shape[1],)); sv = float(np.squeeze(sv))
    diff = fq[:, None, :] - fo[None, :, :]
    u2 = np.sum((diff / ls)**2, axis=-1)
    if case.kname == 'squared_exponential':
      dk = -0.5 * sv * np.exp(-u2 / 2)
    elif case.kname == 'matern32':
      dk = np.where(u2 == 0, 0.0, -sv * 1.5 * np.exp(-np.sqrt(3.0 * u2)))
    else:
      rr = np.sqrt(5.0 * u2); dk = np.where(u2 == 0, 0.0, -sv * 5.0 * np.exp(-rr) * (1 + rr) / 6)
    gfeat = 2.0 * np.einsum('qi,qid->qd', coef * dk, diff) / ls**2
  grad = np.zeros((case.M, case.d))
  gmlp = np.zeros_like(acts[-1])
  if case.mlp_k:
    gmlp += gfeat
  else:
    grad += gfeat
  if case.mname == 'linear' and not drop_raw_mean:
    grad += a_mu[:, None] * wlin[None, :]
  elif case.mname == 'linear_mlp' and not drop_mlp_mean:
    gmlp += a_mu[:, None] * wlin[None, :]
  g = gmlp
  for layer in range(len(case.feats) - 1, -1, -1):
    w = np.asarray(mlp_q[f'Dense_{layer}']['kernel'], dtype=np.float64)
    w = w.T if layer == transpose else w
    dz = g if layer == skip_tanh else g * (1.0 - acts[layer + 1]**2)
    g = dz @ w.T
  return val, grad + g


# ---- mutants: name -> (the cases it applies to, route keyword arguments) -------------------------------------------------------------
def _last_tanh(case): return dict(skip_tanh=len(case.feats) - 1)
def _hidden_tanh(case): return dict(skip_tanh=int(np.argmax(case.feats[:-1])))     # acq_grad_cases: mutant h
def _transpose(case): return dict(transpose=1)


MUTANTS = {
    'last_tanh': (lambda c: True, _last_tanh),
    'h': (lambda c: len(c.feats) >= 2, _hidden_tanh),
    'mlp_mean_dropped': (lambda c: c.mname == 'linear_mlp', lambda c: dict(drop_mlp_mean=True)),
    'raw_mean_dropped': (lambda c: c.mlp_k and c.mname == 'linear', lambda c: dict(drop_raw_mean=True)),
    'transposed': (lambda c: c.feats in ((256, 256), (9,) * 8), _transpose),
    'truncated': (lambda c: c.feats in ((12, 256), (256, 256)) or c.d == 256, lambda c: dict(trunc=True)),
}


def mutant_cases(name):
  return [c for c in CASES if MUTANTS[name][0](c)]


def mutant(name, case, acq, param):
  return route(case, acq, param, **MUTANTS[name][1](case))


def mutant_wrong_sample(case, s, acq, param):
  """Sample s > 0 of a MULTI case with the query's passes under sample 0's weights."""
  return route(case, acq, param, sample=s, weights_of=0)


def distance(case, acq, ref, val, grad):
  """The larger of the worst value and gradient ratios to the bounds of the GPU tier."""
  (rv, _), (rg, _, _) = G.worst(case, acq, ref, val, grad)
  return max(rv, rg)


# ---- the maximiser ---------------------------------------------------------------------------------------------------------------
class OptCase(NamedTuple):
  case: Case         # an fp64 case; the fp32 run rounds its inputs
  acq: str
  S: int
  R: int = 3

  @property
  def name(self):
    return f'{self.case.id}-{self.acq}-S{self.S}-R{self.R}'


_OPT_BASE = [next(c for c in CASES_S if c.feats == (12, 33) and (c.mlp_k, c.mname) == p and c.dtype == 'fp64') for p in PAIRINGS] + \
            [next(c for c in CASES_L if c.n == 129 and c.feats == (12, 33) and (c.mlp_k, c.mname) == FULL and c.kname == 'matern52' and c.dtype == 'fp64')]
OPT_CASES = [OptCase(c, acq, 1) for c in _OPT_BASE for acq in G.ACQS] + [OptCase(_OPT_BASE[0], acq, N_SAMPLES) for acq in G.ACQS]


def opt_param(oc):
  return G.acq_param(oc.acq, G.reference(oc.case))


def opt_x0(oc):
  return np.ascontiguousarray(G.inputs(oc.case)[3][:oc.R].astype(np.float64))


def oracle_value_and_grad(oc):
  """x [D] -> (vals [S], grads [S, D]) from the oracle, one acquisition_value_and_grad per parameter sample."""
  st = G.oracle_setup(oc.case)
  mo, ko = _fns(oc.case)
  sms, param = [sample_setup(oc.case, i) for i in range(oc.S)], opt_param(oc)

  def vg(x):
    vals, grads = [], []
    for sm in sms:
      v, g = o.acquisition_value_and_grad(oc.acq, mo, ko, sm.po, st.x, st.y, np.asarray(x, dtype=np.float64)[None, :], param, WFO,
                                          add_noise=sm.noise, scale=SCALE)
      vals.append(float(v[0, 0])); grads.append(np.asarray(g[0], dtype=np.float64))
    return np.array(vals), np.array(grads)
  return vg


@functools.lru_cache(maxsize=None)
def opt_run(oc, r, mutant=None):
  """The oracle-driven restatement of start r (shared, not to be written to)."""
  return ao.minimise(oracle_value_and_grad(oc), opt_x0(oc)[r], mutant=mutant)
