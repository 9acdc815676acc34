"""CPU side of the MLP-basis tier: tanh(Dense) layers up to the ABI's 256 columns (HBO_MAX_FEATURE_DIM) and eight layers, under the `*_mlp`
kernels and the linear_mlp mean.  No device code here.  Shared by tests/test_mlp_cases_host.py (this file judged on its own, on the
CPU) and tests/test_gpu_mlp.py (the four device implementations against it, PER LEAF: every Dense_l/kernel and Dense_l/bias is a leaf).

  CASES               input width d, layer widths, kernel, length-scale form.  Last layers on both sides of every thread count of the
                      weight-gradient kernels (64 / 128 / 192 / 256 threads from fout, csrc/mlp.hip: launch_dense_bwd_batch, csrc/grad.hip:
                      launch_dense_bwd), hidden layers on the same edges, depths 1, 2, 3 and 8, single-column layers, d = 1 and 256
  SIZES               two ragged task lists: 'blocked' (three 256-row chunks of the weight gradient; tasks that end inside the first and
                      the second) and 'small' (every task in one workgroup, csrc/small.hip)
  inputs(...)         model (helpers.mlp_model) and tasks in the dtype, seeded by the case's id; fp32 is the fp64 draw rounded once
  reference(...)      oracle/hyperbo_oracle.py: nll_value_and_grad in fp64 on those inputs, with each task's activations, the d f / d
                      features the oracle hands to its MLP backward, and the un-cancelled term scale T_leaf of every MLP leaf
  forward / backward  the MLP and its backward pass (dW, db, din) for a given upstream dF restated in `wide` = np.longdouble (the
                      reference's own error), float32 (the yardstick of the fp32 bounds) or float64 (what the MUTANTS are wrong variants of)
  leaf_ratios(...)    the per-leaf bound of helpers.assert_grad_close(..., leaf_scales=...), as ratios to it

The bound of an MLP leaf: tol * max(|leaf|_inf, min(1e-3 max|g|, T_leaf)).  helpers.assert_grad_close floors a leaf's scale at 1e-3 of
the largest leaf, which is right for a leaf that is small by cancellation -- its error scales with the un-cancelled terms -- and wrong
for one that is small because its terms are: at the fp32 tolerance a wholly wrong leaf of 2e-6 max|g| would pass under that floor.
T_leaf = max_{k,o} sum_i |in[i,k]| |dz[i,o]| (kernel), max_o sum_i |dz[i,o]| (bias), summed over the tasks like the leaf itself, is the
scale of those terms; the floor never exceeds it.  (On this table the one-column bottlenecks put MLP leaves down to 7.5e-5 of the
largest leaf, all of them by cancellation: the least T_leaf is 2.3e-2 max|g|, so the rule coincides with the default floor here; it
is what keeps that true of a later case.)
"""
import functools
from typing import NamedTuple, Tuple

import numpy as np
import scipy.linalg as spla

import helpers
from oracle import hyperbo_oracle as o

WFO = o.DEFAULT_WARP_FUNC
LD = np.longdouble
STATIONARY = ['squared_exponential', 'matern32', 'matern52']
ROWS_PER_CHUNK = 256        # rows_per_block of the weight-gradient kernels
SMALL_LIMIT = 128           # the single-workgroup evaluation takes batches whose tasks all have n <= 128

# ---- bounds (the project's own: tests/test_gpu_small_path.py, tests/test_gpu_parity.py) --------------------------------------------
FP64_VALUE_TOL = 1e-10      # relative
FP64_GRAD_TOL = 1e-10       # per leaf
FP32_VALUE_TOL = 2e-4
FP32_GRAD_TOL = 2.5e-3
REFERENCE_SHARE = 0.01      # the oracle agrees with the longdouble restatement to this much of every fp64 bound
YARDSTICK_SHARE = 0.25      # the float32 restatement stays under this much of every fp32 bound
SATURATION = 0.99
SATURATION_SHARE = 0.10
DTYPES = ('fp64', 'fp32')


def np_dtype(dtype):
  return np.float64 if dtype == 'fp64' else np.float32


def tols(dtype):
  return (FP64_VALUE_TOL, FP64_GRAD_TOL) if dtype == 'fp64' else (FP32_VALUE_TOL, FP32_GRAD_TOL)


class Case(NamedTuple):
  d: int
  feats: Tuple[int, ...]
  kname: str = 'matern52'
  ls: str = 'ard'            # 'ard' | 'scalar' | 'none' (dot product)

  @property
  def id(self):
    return f'd{self.d}-f' + 'x'.join(str(f) for f in self.feats) + f'-{self.kname}-{self.ls}'

  @property
  def fins(self):
    return (self.d,) + tuple(self.feats[:-1])


LAST_WIDTHS = (1, 63, 64, 65, 128, 129, 192, 193, 256)
HIDDEN_WIDTHS = (65, 129, 193, 256)
DEPTH8 = (256, 1, 256, 1, 256, 1, 256, 192)
CASES_LAST = [Case(5, (12, f), STATIONARY[i % 3], ('ard', 'scalar')[i % 2]) for i, f in enumerate(LAST_WIDTHS)]
CASES_HIDDEN = [Case(5, (h, 33), STATIONARY[(i + 1) % 3], ('scalar', 'ard')[i % 2]) for i, h in enumerate(HIDDEN_WIDTHS)] + [Case(5, (256, 256), 'squared_exponential', 'ard')]
CASES_DEPTH = [Case(5, (256,), 'matern32', 'ard'), Case(5, (65,), 'squared_exponential', 'scalar'), Case(5, (129, 65, 193), 'matern52', 'scalar'),
               Case(5, DEPTH8, 'matern52', 'ard')]
CASES_INPUT = [Case(1, (1, 256), 'squared_exponential', 'ard'), Case(256, (193, 1), 'matern32', 'scalar')]
CASES_DOT = [Case(5, (128, 193), 'dot_product', 'none')]
CASES = CASES_LAST + CASES_HIDDEN + CASES_DEPTH + CASES_INPUT + CASES_DOT
SIZES = {'blocked': (129, 255, 256, 257, 513), 'small': (128, 90, 33, 2)}
BY_FEATS = {c.feats: c for c in CASES}


def threads(fout):
  """The block size launch_dense_bwd_batch / launch_dense_bwd choose for a layer of fout columns."""
  return 64 if fout < 64 else (256 if fout > 256 else -(-fout // 64) * 64)


def chunks(n):
  return -(-n // ROWS_PER_CHUNK)


def last_chunk(n):
  """The row chunk in which a task of n rows ends."""
  return (n - 1) // ROWS_PER_CHUNK


def config(case):
  return {'mlp_features': tuple(case.feats)}


def cast(tree, dtype):
  return {k: cast(v, dtype) for k, v in tree.items()} if isinstance(tree, dict) else np.asarray(tree, dtype=dtype)


def mlp_leaf_paths(case):
  return [f'mlp_params/Dense_{l}/{part}' for l in range(len(case.feats)) for part in ('kernel', 'bias')]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
class Inputs(NamedTuple):
  model: dict                # raw params.model in the dtype
  tasks: tuple               # ((x [n, d], y [n, 1]), ...) in the dtype, in SIZES' order


@functools.lru_cache(maxsize=None)
def _inputs64(case, sizes):
  rng = np.random.default_rng([ord(ch) for ch in case.id])
  model = helpers.mlp_model(rng, case.d, case.feats, case.kname, case.ls)
  return model, tuple(helpers.synthetic_task(rng, n, case.d) for n in SIZES[sizes])


@functools.lru_cache(maxsize=None)
def inputs(case, sizes, dtype):
  """Shared and not to be written to.  The model does not depend on `sizes`."""
  model, tasks = _inputs64(case, sizes)
  dt = np_dtype(dtype)
  return Inputs(cast(model, dt), tuple((np.ascontiguousarray(x, dtype=dt), np.ascontiguousarray(y, dtype=dt)) for x, y in tasks))


def oracle_funcs(case):
  return o.linear_mlp, getattr(o, case.kname + '_mlp')


def oracle_params(case, model):
  return o.GPParams(model=cast(model, np.float64), config=config(case))


def weights(model, wide=np.float64):
  """[(W, b)] per layer, in `wide`."""
  mp = model['mlp_params']
  return [(np.asarray(mp[f'Dense_{l}']['kernel']).astype(wide), np.asarray(mp[f'Dense_{l}']['bias']).astype(wide)) for l in range(len(mp))]


# ---- the restatement: forward, backward, and the wrong variants ------------------------------------------------------------------------
MUTANTS = {
    'cols_ge_64': 'output columns >= 64 of the weight gradient (its bias row included) dropped',
    'cols_ge_128': 'the same from column 128',
    'cols_ge_192': 'the same from column 192',
    'no_bias_row': 'the bias row of the weight gradient skipped',
    'rows_ge_256': 'rows >= 256 of a task skipped by the weight gradient',
    'chunk_twice': 'the second row chunk of the shortest multi-chunk task counted twice',
    'neighbour_act': '1 - out^2 taken from the neighbouring layer\'s activations (read as the flat buffer they are)',
    'pingpong_odd': 'one layer of an odd-depth model reads the other ping-pong buffer (the dz the layer above left there)',
    'pingpong_even': 'the same at one layer of an even-depth model',
    'din_transposed': 'din with w read transposed (w[o * fin + k])',
    'sample0_weights': 'sample 0\'s weights used for every sample',
    'last_col_zero': 'the last column of the last layer\'s features zero in the forward pass',
}
VALUE_MUTANTS = ('sample0_weights', 'last_col_zero')      # judged by the value bound (per task, per sample), not per leaf
PINGPONG_LAYER = 0          # the layer that reads the wrong buffer: the lowest one (the whole chain above it is lost)


def applicable(case, sizes, mutant):
  """By the shapes alone: whether the mutant can differ from the restatement on this case."""
  L, feats, ns = len(case.feats), case.feats, SIZES[sizes]
  if mutant.startswith('cols_ge_'):
    return max(feats) > int(mutant[8:])
  if mutant in ('rows_ge_256', 'chunk_twice'):
    return max(ns) > ROWS_PER_CHUNK
  if mutant == 'neighbour_act':
    return L >= 2
  if mutant in ('pingpong_odd', 'pingpong_even'):
    return L >= 2 and L % 2 == (1 if mutant == 'pingpong_odd' else 0)
  if mutant == 'din_transposed':       # din of layer l >= 1 feeds layer l - 1; a one-column or one-row w is its own transpose in memory
    return any(case.fins[l] > 1 and feats[l] > 1 for l in range(1, L))
  return mutant in ('no_bias_row', 'last_col_zero')      # (sample0_weights: the per-sample cases, SAMPLE_CASES)


def forward(wts, x, wide, mutant=None):
  """acts[0] = x, acts[l + 1] = tanh(acts[l] W_l + b_l), every array in `wide`."""
  acts = [np.asarray(x).astype(wide)]
  for W, b in wts:
    assert W.dtype == wide and b.dtype == wide
    acts.append(np.tanh(acts[-1] @ W + b))
  if mutant == 'last_col_zero':
    acts[-1] = acts[-1].copy()
    acts[-1][:, -1] = 0
  assert all(a.dtype == wide for a in acts)
  return acts


def backward(wts, acts, dF, wide, mutant=None, row_weight=None):
  """The backward pass for an upstream dF (d f / d last-layer features): ([(dW_l, db_l)], din of layer 0, [dz_l]).  `mutant` names the one
  line that is changed; row_weight (n,): how often the weight gradient counts each row (the row-chunk mutants)."""
  L = len(wts)
  g = np.asarray(dF).astype(wide)
  grads, dzs, dz_above = [None] * L, [None] * L, None
  for l in reversed(range(L)):
    W = wts[l][0]
    fin, fout = W.shape
    out = acts[l + 1]
    if mutant == 'neighbour_act':
      out = np.resize(acts[l] if l >= 1 else acts[2], out.shape)
    if mutant in ('pingpong_odd', 'pingpong_even') and l == PINGPONG_LAYER:
      g = np.resize(dz_above, g.shape)
    dz = g * (1 - out * out)
    dzw = dz if row_weight is None else dz * np.asarray(row_weight).astype(wide)[:, None]
    dW, db = acts[l].T @ dzw, dzw.sum(axis=0)
    if mutant is not None and mutant.startswith('cols_ge_'):
      dW[:, int(mutant[8:]):] = 0
      db[int(mutant[8:]):] = 0
    if mutant == 'no_bias_row':
      db = np.zeros_like(db)
    g = dz @ (W.ravel().reshape(fout, fin) if mutant == 'din_transposed' else W.T)
    grads[l], dzs[l], dz_above = (dW, db), dz, dz
    assert dW.dtype == wide and db.dtype == wide and g.dtype == wide
  return grads, g, dzs


def row_weight(n, mutant, twice_n):
  if mutant == 'rows_ge_256':
    return (np.arange(n) < ROWS_PER_CHUNK).astype(np.float64)
  if mutant == 'chunk_twice' and n == twice_n:
    r = np.arange(n)
    return 1.0 + ((r >= ROWS_PER_CHUNK) & (r < 2 * ROWS_PER_CHUNK))
  return None


def mlp_tree(per_task_grads, ntasks):
  """The mlp_params sub-tree of the batch gradient (the mean over the tasks) from each task's [(dW, db)]."""
  L = len(per_task_grads[0])
  return {f'Dense_{l}': {'kernel': np.asarray(sum(g[l][0] for g in per_task_grads) / ntasks, dtype=np.float64),
                         'bias': np.asarray(sum(g[l][1] for g in per_task_grads) / ntasks, dtype=np.float64)} for l in range(L)}


# ---- the NLL of a task from its features (the value mutants; the float32 yardstick of the value) -------------------------------------
def nll_from_features(case, model, feat, y):
  """One task's Cholesky NLL (linalg.py:36-69 with the 1e-6 jitter) under the kernel on `feat` and the linear mean on `feat`, in fp64."""
  po = oracle_params(case, model)
  feat, y = np.asarray(feat, dtype=np.float64), np.asarray(y, dtype=np.float64)
  n = feat.shape[0]
  lm = po.model['linear_mean']
  r = y - (feat @ lm['kernel'] + lm['bias'])
  noise = float(np.squeeze(o.retrieve_params(po, ['noise_variance'], WFO)[0]))
  kmat = getattr(o, case.kname)(po, feat, warp_func=WFO) if n <= 130 else _gram(case, po, feat)
  chol = spla.cholesky(kmat + np.eye(n) * (noise + 1e-6), lower=True)
  alpha = spla.cho_solve((chol, True), r)
  return float(0.5 * np.sum(r * alpha) + np.sum(np.log(np.diag(chol))) + 0.5 * n * np.log(2 * np.pi))


def _gram(case, po, feat):
  """The Gram matrix without the oracle's n x n x F array of differences (|a|^2 + |b|^2 - 2 a.b in fp64: enough for a value)."""
  if case.kname == 'dot_product':
    return o.dot_product(po, feat, warp_func=WFO)
  ls, sv = o.retrieve_params(po, ['lengthscale', 'signal_variance'], WFO)
  a = feat / np.asarray(ls, dtype=np.float64)
  sq = np.sum(a * a, axis=1)
  u = np.maximum(sq[:, None] + sq[None, :] - 2 * a @ a.T, 0.0)
  np.fill_diagonal(u, 0.0)
  sv = float(np.squeeze(sv))
  if case.kname == 'squared_exponential':
    return sv * np.exp(-u / 2)
  r = np.sqrt((3.0 if case.kname == 'matern32' else 5.0) * u)
  return sv * (1 + r) * np.exp(-r) if case.kname == 'matern32' else sv * (1 + r + r * r / 3) * np.exp(-r)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
class Ref(NamedTuple):
  value: float               # the mean over the tasks: what nll_value_and_grad returns
  per_task: tuple            # every task's value
  grad: dict                 # d value / d raw params.model
  acts: tuple                # per task: the oracle's activations (acts[0] = x)
  dF: tuple                  # per task: the d f / d features the oracle hands to its MLP backward
  task_mlp: tuple            # per task: the oracle's mlp_params gradient of that task
  din: tuple                 # per task: d f / d x through the MLP (float64 restatement)
  scales: dict               # MLP leaf path -> T_leaf


def oracle_task(case, model64, x, y):
  """(value, gradient tree, acts, dF) of one task; the activations and dF are taken where the oracle calls its MLP backward."""
  seen = []
  inner = o._mlp_backward

  def recording(mlp_params, acts, dfeat):
    seen.append((acts, dfeat))
    return inner(mlp_params, acts, dfeat)
  o._mlp_backward = recording
  try:
    mo, ko = oracle_funcs(case)
    v, g = o.nll_sub_dataset_value_and_grad(mo, ko, oracle_params(case, model64), np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), WFO)
  finally:
    o._mlp_backward = inner
  assert len(seen) == 1
  return v, g, seen[0][0], seen[0][1]


@functools.lru_cache(maxsize=None)
def reference(case, sizes, dtype):
  """Shared and not to be written to.  fp32: the oracle in float64 on the fp32-rounded inputs."""
  model, tasks = inputs(case, sizes, dtype)
  m64 = cast(model, np.float64)
  out = [oracle_task(case, m64, x, y) for x, y in tasks]
  T = len(tasks)
  grad = o._tree_scale(functools.reduce(o._tree_add, [g for _, g, _, _ in out]), 1.0 / T)
  wts = weights(m64)
  scales, dins = {}, []
  tk = [np.zeros(w.shape) for w, _ in wts]
  tb = [np.zeros(b.shape) for _, b in wts]
  for _, _, acts, dF in out:
    _, din, dzs = backward(wts, acts, dF, np.float64)
    dins.append(din)
    for l, dz in enumerate(dzs):
      tk[l] += np.abs(acts[l]).T @ np.abs(dz)
      tb[l] += np.abs(dz).sum(axis=0)
  for l in range(len(wts)):
    scales[f'mlp_params/Dense_{l}/kernel'] = float(np.max(tk[l])) / T
    scales[f'mlp_params/Dense_{l}/bias'] = float(np.max(tb[l])) / T
  return Ref(float(sum(v for v, _, _, _ in out) / T), tuple(v for v, _, _, _ in out), grad, tuple(a for _, _, a, _ in out),
             tuple(f for _, _, _, f in out), tuple(g['mlp_params'] for _, g, _, _ in out), tuple(dins), scales)


def with_mlp(grad, mlp):
  """The gradient tree with its mlp_params leaves replaced."""
  out = dict(grad)
  out['mlp_params'] = mlp
  return out


def restated_tree(case, sizes, dtype, wide=np.float64, mutant=None):
  """The reference's gradient tree with the MLP leaves from the restatement in `wide` on the oracle's dF (forward pass included)."""
  ref, (model, tasks) = reference(case, sizes, dtype), inputs(case, sizes, dtype)
  wts = weights(model, wide)
  multi = [n for n in SIZES[sizes] if n > ROWS_PER_CHUNK]
  per = []
  for (x, _), dF in zip(tasks, ref.dF):
    acts = forward(wts, x, wide)
    per.append(backward(wts, acts, dF, wide, mutant, row_weight(x.shape[0], mutant, min(multi) if multi else None))[0])
  return with_mlp(ref.grad, mlp_tree(per, len(tasks)))


# ---- the per-leaf bound -------------------------------------------------------------------------------------------------------------
def leaf_ratios(got, ref, tol, leaf_scales=None, floor_rel=1e-3):
  """path -> max |got - ref| over the leaf's bound, by the rule of helpers.assert_grad_close(..., leaf_scales=leaf_scales); anything not
  finite: inf."""
  errs = helpers.grad_leaf_errors(got, ref)
  gmax = max((nrm for _, _, nrm in errs), default=0.0)
  out = {}
  for path, err, nrm in errs:
    floor = floor_rel * gmax
    if leaf_scales is not None and path in leaf_scales:
      floor = min(floor, leaf_scales[path])
    out[path] = err / (tol * max(nrm, floor, 1e-300)) if np.isfinite(err) else np.inf
  return out


def worst_leaf(ratios):
  path = max(ratios, key=ratios.get)
  return ratios[path], path


def value_ratio(got, ref, tol):
  """The value rule of tests/test_gpu_small_path.py: |got - ref| <= tol max(|ref|, 1)."""
  return abs(got - ref) / (tol * max(abs(ref), 1.0)) if np.isfinite(got) else np.inf


def mutant_ratios(case, sizes, dtype, mutant):
  """How far the mutant lies from the reference, in bounds of the GPU tier: per MLP leaf (a value mutant: {'value': the worst task})."""
  ref, (model, tasks) = reference(case, sizes, dtype), inputs(case, sizes, dtype)
  vtol, gtol = tols(dtype)
  if mutant in VALUE_MUTANTS:
    assert mutant == 'last_col_zero'
    wts = weights(cast(model, np.float64))
    return {'value': max(value_ratio(nll_from_features(case, model, forward(wts, x, np.float64, mutant)[-1], y), v, vtol)
                         for (x, y), v in zip(tasks, ref.per_task))}
  ratios = leaf_ratios(restated_tree(case, sizes, dtype, np.float64, mutant), ref.grad, gtol, ref.scales)
  return {p: ratios[p] for p in mlp_leaf_paths(case)}


def saturation(acts):
  """Per layer: the share of activations beyond SATURATION."""
  return [float(np.mean(np.abs(a) > SATURATION)) for a in acts[1:]]


# ---- per-sample weight sets (hbo_nll_samples) ------------------------------------------------------------------------------------------
# (65, 129): arrays of 2600, 520, 67080 and 1032 bytes in fp64; (5,) on d = 5: 25 weights and 5 biases, 200 / 40 bytes in fp64 and 100 / 20
# in fp32 -- models_pack puts every array on a 256-byte boundary, so neither a sample's stride nor an array's offset is its size
SAMPLE_CASES = [Case(5, (65, 129), 'matern52', 'ard'), Case(5, (5,), 'squared_exponential', 'ard')]
SAMPLE_COUNT = 3
SAMPLE_SIZES = {'fused': (100, 128), 'blocked': (129, 257)}
SAMPLE_TOL = {'fp64': (1e-12, 1e-10), 'fp32': (1e-5, 1e-5)}     # (against hbo_nll alone, against the oracle): tests/test_gpu_slice.py


@functools.lru_cache(maxsize=None)
def sample_inputs(case, shape, dtype):
  """(models: SAMPLE_COUNT params.model of one family with different values, tasks) in the dtype."""
  dt = np_dtype(dtype)
  models = []
  for s in range(SAMPLE_COUNT):
    rng = np.random.default_rng([ord(ch) for ch in case.id] + [31 * s])
    models.append(cast(helpers.mlp_model(rng, case.d, case.feats, case.kname, case.ls), dt))
  rng = np.random.default_rng([ord(ch) for ch in case.id] + [7])
  tasks = tuple(helpers.synthetic_task(rng, n, case.d, dtype=dt) for n in SAMPLE_SIZES[shape])
  return tuple(models), tasks


def sample_values(case, shape, dtype, mutant=None):
  """[sample][task] -> NLL by nll_from_features on the float64 forward pass (sample0_weights: with sample 0's MLP)."""
  models, tasks = sample_inputs(case, shape, dtype)
  out = []
  for m in models:
    wts = weights(cast((models[0] if mutant == 'sample0_weights' else m), np.float64))
    out.append([nll_from_features(case, m, forward(wts, x, np.float64)[-1], y) for x, y in tasks])
  return np.array(out)


# ---- the divergence objective on one wide case ---------------------------------------------------------------------------------------------
EKL_CASE = Case(5, (12, 129), 'matern52', 'ard')
EKL_TASK = (130, 4)         # one aligned task: 130 points (two 128-row blocks), 4 columns of y
# the bounds of tests/test_gpu_divergence.py (tests/divergence_cases.py): fp64 value 1e-10 S, S the sum of |term|; fp32 value 4 x the
# float32 restatement's own error + 8 eps32 S; gradient per leaf at the tolerances above
EKL_FP64_VALUE, EKL_REL_FACTOR, EKL_FLOOR_C = 1e-10, 4.0, 8.0


@functools.lru_cache(maxsize=None)
def ekl_inputs(dtype):
  case, (n, m) = EKL_CASE, EKL_TASK
  rng = np.random.default_rng([ord(ch) for ch in case.id] + [n, m])
  model = helpers.mlp_model(rng, case.d, case.feats, case.kname, case.ls)
  x = rng.uniform(size=(n, case.d))
  y = np.sin(3 * x.sum(axis=1, keepdims=True) + rng.normal(size=(1, m))) + 0.3 * rng.normal(size=(n, m))      # tests/divergence_cases.py
  dt = np_dtype(dtype)
  return cast(model, dt), np.ascontiguousarray(x, dtype=dt), np.ascontiguousarray(y, dtype=dt)


def ekl_terms(dtype, wide):
  """The terms of the partial KL (utils.py:84-106 on the sample statistics of objectives.py:57-58) with every array in `wide`."""
  import pathwise_cases as pc
  case = EKL_CASE
  model, x, y = ekl_inputs(dtype)
  po = o.GPParams(model=cast(model, np.float32 if wide == np.float32 else np.float64), config=config(case))
  x, y = x.astype(wide), y.astype(wide)
  n, m = y.shape
  mu1 = np.asarray(o.linear_mlp(po, x, warp_func=WFO), dtype=wide)[:, 0]
  noise = np.asarray(o.retrieve_params(po, ['noise_variance'], WFO)[0], dtype=wide)
  k1 = getattr(o, case.kname + '_mlp')(po, x, warp_func=WFO) + np.eye(n, dtype=wide) * noise
  mu0 = np.sum(y, axis=1) / wide(m)
  rows = (y - mu0[:, None]) / np.sqrt(wide(m))
  assert k1.dtype == wide and rows.dtype == wide
  c = pc.chol(k1)
  z = pc.solve_lower(c, np.concatenate([rows, (mu1 - mu0)[:, None]], axis=1))
  return {'tr': np.sum(z[:, :-1] ** 2), 'mahalanobis': np.sum(z[:, -1] ** 2), 'logdet': wide(2) * np.sum(np.log(np.diag(c)))}


@functools.lru_cache(maxsize=None)
def ekl_reference(dtype):
  """(value, gradient tree, S, the value bound) of the task from the oracle in fp64 on the dtype's inputs."""
  model, x, y = ekl_inputs(dtype)
  v, g, terms = o._divergence_sub_dataset_value_and_grad('ekl', o.linear_mlp, getattr(o, EKL_CASE.kname + '_mlp'), oracle_params(EKL_CASE, model),
                                                          x.astype(np.float64), y.astype(np.float64), WFO, return_terms=True)
  s = float(sum(abs(t) for t in terms.values()))
  if dtype == 'fp64':
    return v, g, s, EKL_FP64_VALUE * s
  level = float(abs(LD(sum(ekl_terms(dtype, np.float32).values())) - sum(ekl_terms(dtype, LD).values())))
  return v, g, s, EKL_REL_FACTOR * level + EKL_FLOOR_C * float(np.finfo(np.float32).eps) * s
