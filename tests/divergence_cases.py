"""CPU side of the divergence tier (hbo_objective with HBO_OBJ_EKL / HBO_OBJ_EUC, csrc/objective.hip: the augmented tile row of a task with
m + 1 <= 128 aligned columns, and from m = 128 on the m + 1 outer-product vectors of fill_desc's nvec path -- expand_rows_kernel, two
tri_matvec passes and add_sumsq_kernel for EKL, the nvec loops of grad.hip and kumar.hip).  Shared by tests/test_divergence_cases_host.py
(this file judged on its own, on the CPU) and tests/test_gpu_divergence.py (the device against it, PER TASK):

  CASES               one record per task list.  A: the column edge m + 1 = 128 (m in 1, 2, 126..129, 257); B: the row edge n = 128
                      (n in 1, 2, 127..129, 257) on both column paths; C: every kernel family, plain, on the MLP basis and Kumaraswamy-
                      warped, at (129, 127) and (129, 128); D: one batch mixing naug = 3, naug = 128 and nvec tasks of 1-3 blocks; E: fp32;
                      F: |d| = 0, C0 = 0 on the nvec path, m = 1; S: a nine-block task beside both column paths (the one-sweep inverse)
  inputs(case)        model and [(x, y)] in the case's dtype, seeded by the case's id (without its kind and dtype: 'ekl' / 'euc' and
                      fp64 / fp32 see the same numbers, the fp32 ones rounded once, here)
  reference(case)     per task: value, terms, term scale S_k, gradient tree -- oracle._divergence_sub_dataset_value_and_grad in fp64
                      (a Kumaraswamy kernel: on the warped inputs; its a / b leaves analytic from the kernel adjoint, ab_analytic)
  restate_task(...)   the value terms by the formulas of utils.py:84-173 in `wide` = float32, float64 or np.longdouble (Cholesky and
                      substitutions by hand: pathwise_cases.chol / solve_lower), and the value MUTANTS; grad_mutant: the gradient ones
                      (wrong adjoints through the oracle's backward pass); mutant_ratio: how many bounds away a mutant lies
  value_bounds(case)  per task.  fp64: FP64_VALUE * S_k; fp32: REL_FACTOR x the float32 restatement's own error + FLOOR_C eps32 S_k

The term scale S_k = sum of |term| over the task's terms (EKL: tr(K1^-1 C0), the Mahalanobis term, logdet K1; EUC: |d|, |C0 - K1|_F):
the terms of the partial KL have opposite signs, so a bound relative to the value itself would tighten with the cancellation, and a
bound relative to the batch total lets a task that is wrong by 1e-7 of its own terms pass beside a larger one.
"""
import functools
from typing import NamedTuple, Tuple

import numpy as np

import helpers
import kumar_cases
import kumar_oracle
import pathwise_cases as pc
from oracle import hyperbo_oracle as o

WFO = o.DEFAULT_WARP_FUNC
LD = np.longdouble
TILE = 128
NLL_EPS = 1e-6              # the jitter of the NLL (linalg.py:36-69), which the divergences do NOT add (objectives.py:63-65)

# ---- bounds ------------------------------------------------------------------------------------------------------------------------
FP64_VALUE = 1e-10          # of S_k, per task: the suite's fp64 level (tests/test_gpu_parity.py), without the x50 of the batch-mean tests
COND_BOUND = 1e-11          # |fp64 reference - longdouble restatement| <= COND_BOUND * S_k on every fp64 case: a tenth of the bound
FP64_GRAD_TOL = 1e-10       # per leaf, helpers.assert_grad_close (tests/test_gpu_parity.py)
FP32_GRAD_TOL = 2.5e-3      # per leaf, helpers.assert_grad_close (tests/test_gpu_parity.py)
# fp32 value: err_k <= REL_FACTOR * (error of the float32 restatement of task k against longdouble) + FLOOR_C * eps32 * S_k -- the rule
# of pathwise_cases.bound, for the same reason: the device rounds its operands (the Gram matrix, the factor, the augmented rows) to
# fp32 as the float32 restatement does and sums in fp64, so its error is of the restatement's order; the floor covers a restatement
# that happens to land within an ulp.
REL_FACTOR = 4.0
FLOOR_C = 8.0
AB_FD_STEP = 1e-5           # a / b leaves: central differences of the oracle value (tests/test_gpu_kumar.py: _fd_ab) ...
AB_FD_TOL = 1e-6            # ... to which the analytic reference is held on the CPU, rtol = atol / max|leaf| = 1e-6 (test_divergence_value_and_grad there)
AB_TOL = 1e-10              # the device against the analytic reference (ab_analytic), same form: the suite's fp64 level per leaf


class Case(NamedTuple):
  group: str                 # 'A' .. 'F'
  kind: str                  # 'ekl' | 'euc'
  kname: str                 # the base kernel
  mlp: bool                  # the kernel works on the MLP basis (helpers.MLP_FEATURES)
  mname: str
  kumar: bool
  dtype: str                 # 'fp64' | 'fp32'
  tasks: Tuple[Tuple[int, int], ...]     # (n, m) of every task, in the dataset's order
  special: str = ''          # group F: 'zero_mean' | 'identical'
  d: int = 3

  @property
  def kernel_name(self):
    return self.kname + ('_mlp' if self.mlp else '') + ('_kumar' if self.kumar else '')

  @property
  def data_id(self):
    return (f'{self.group}-{self.kernel_name}+{self.mname}-' + '_'.join(f'{n}x{m}' for n, m in self.tasks) +
            (f'-{self.special}' if self.special else ''))

  @property
  def id(self):
    return f'{self.data_id}-{self.kind}-{self.dtype}'

  @property
  def np_dtype(self):
    return np.float64 if self.dtype == 'fp64' else np.float32

  @property
  def obj_id(self):
    return 1 if self.kind == 'ekl' else 2        # include/hbo.h: HBO_OBJ_EKL, HBO_OBJ_EUC


KINDS = ('ekl', 'euc')
A_N, A_M = (70, 150), (1, 2, 126, 127, 128, 129, 257)
B_M, B_N = (3, 130), (1, 2, 127, 128, 129, 257)
C_SHAPES = ((129, 127), (129, 128))
C_FAMILIES = ([(k, False, 'zero', False) for k in helpers.KERNELS] + [(k, True, 'linear_mlp', False) for k in helpers.KERNELS] +
              [('squared_exponential', False, 'constant', True), ('matern52', False, 'linear', True), ('dot_product', False, 'zero', True)])
D_TASKS = ((300, 2), (150, 127), (140, 128), (70, 257), (1, 130), (40, 1))
D_FAMILIES = [('matern52', False, 'constant', False), ('dot_product', True, 'linear_mlp', False)]
D_FP32_FAMILIES = [('squared_exponential', False, 'zero', False), ('matern52', True, 'linear_mlp', False)]
A_FAMILY = ('matern52', False, 'linear', False)
B_FAMILY = ('squared_exponential', False, 'constant', False)


def _both(group, family, dtype, tasks, special=''):
  return [Case(group, kind, *family, dtype, tuple(tasks), special) for kind in KINDS]


GROUP_A = [c for n in A_N for m in A_M for c in _both('A', A_FAMILY, 'fp64', [(n, m)])]
GROUP_B = [c for m in B_M for n in B_N for c in _both('B', B_FAMILY, 'fp64', [(n, m)])]
GROUP_C = [c for fam in C_FAMILIES for shape in C_SHAPES for c in _both('C', fam, 'fp64', [shape])]
GROUP_D = [c for fam in D_FAMILIES for c in _both('D', fam, 'fp64', D_TASKS)]
GROUP_E = ([c for m in (127, 128, 257) for c in _both('E', A_FAMILY, 'fp32', [(150, m)])] +
           [c for m in B_M for n in (128, 129) for c in _both('E', B_FAMILY, 'fp32', [(n, m)])] +
           [c for fam in D_FP32_FAMILIES for c in _both('E', fam, 'fp32', D_TASKS)])
# F.  zero_mean: every row of y sums to exactly zero over the columns (dyadic entries in +- pairs, so in any order of summation) and
# the model mean is zero -- the zero function, or a constant mean whose constant IS 0 / a linear_mlp mean whose weights and bias ARE 0,
# which have gradient leaves (and, through d f / d features, the MLP's) for a NaN of d / |d| to land in -- so
# d = mu1 - mu0 = 0 exactly, on the tile path and on the nvec path; identical: m = 130 equal columns, C0 = 0 exactly; and m = 1
GROUP_F = ([c for fam, tasks in ((('squared_exponential', False, 'zero', False), [(70, 4)]), (('squared_exponential', False, 'constant', False), [(70, 4)]),
                                 (('matern52', False, 'constant', False), [(70, 130)]), (('matern52', True, 'linear_mlp', False), [(70, 130)]))
            for c in _both('F', fam, 'fp64', tasks, 'zero_mean')] +
           _both('F', B_FAMILY, 'fp64', [(70, 130)], 'identical') + _both('F', B_FAMILY, 'fp64', [(129, 1)]))
# S.  sched.hip:use_sweep is false below eight blocks whatever the options say, so no batch of n <= 300 reaches the one-sweep inverse: one
# nine-block task beside a full tile row and an nvec task (the extra rows read the W the sweep completes), for the two EKL back ends
S_TASKS = ((1030, 2), (150, 127), (140, 128))
GROUP_S = _both('S', D_FAMILIES[0], 'fp64', S_TASKS)
FP64_CASES = GROUP_A + GROUP_B + GROUP_C + GROUP_D + GROUP_F + GROUP_S
CASES = FP64_CASES + GROUP_E
GROUPS = {'A': GROUP_A, 'B': GROUP_B, 'C': GROUP_C, 'D': GROUP_D, 'E': GROUP_E, 'F': GROUP_F, 'S': GROUP_S}
D_SUBSAMPLE = {1: 100, 2: 90, 0: 200}      # group D's device sub-sample: task index -> rows kept, of (150, 127), (140, 128) and (300, 2)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def cast(tree, dtype):
  return {k: cast(v, dtype) for k, v in tree.items()} if isinstance(tree, dict) else np.asarray(tree, dtype=dtype)


def config():
  return {'mlp_features': helpers.MLP_FEATURES}


class Inputs(NamedTuple):
  model: dict                # raw params.model in the case's dtype
  tasks: tuple               # ((x [n, d], y [n, m]), ...) in the case's dtype


@functools.lru_cache(maxsize=None)
def _inputs64(data_id, case):
  rng = np.random.default_rng([ord(ch) for ch in data_id])
  model = helpers.make_model(rng, case.mname, case.mlp, case.d)
  if case.kumar:
    model['kumar_params'] = {'a': rng.uniform(-1.0, 1.0, size=case.d), 'b': rng.uniform(-1.0, 1.0, size=case.d)}
  if case.special == 'zero_mean':
    if case.mname == 'constant':
      model['constant'] = np.array(0.0)
    if case.mname == 'linear_mlp':
      model['linear_mean'] = {'kernel': np.zeros_like(model['linear_mean']['kernel']), 'bias': np.zeros_like(model['linear_mean']['bias'])}
  tasks = []
  for n, m in case.tasks:
    # the data of test_divergence_with_more_than_127_aligned_columns
    x = rng.uniform(size=(n, case.d))
    y = np.sin(3 * x.sum(axis=1, keepdims=True) + rng.normal(size=(1, m))) + 0.3 * rng.normal(size=(n, m))
    if case.special == 'zero_mean':
      assert m % 2 == 0
      y = np.round(8 * y) / 8
      y[:, 1::2] = -y[:, 0::2]
    if case.special == 'identical':
      y = np.repeat(np.round(8 * y[:, :1]) / 8, m, axis=1)
    tasks.append((x, y))
  return model, tuple(tasks)


def inputs(case):
  """The case's model and tasks in its dtype.  Shared and not to be written to."""
  return _inputs_typed(case._replace(kind='ekl'))


@functools.lru_cache(maxsize=None)
def _inputs_typed(case):
  model, tasks = _inputs64(case.data_id, case._replace(dtype='fp64'))
  dt = case.np_dtype
  return Inputs(cast(model, dt), tuple((np.ascontiguousarray(x, dtype=dt), np.ascontiguousarray(y, dtype=dt)) for x, y in tasks))


def subsample_rows(case):
  """Group D: task index -> the sorted rows of its device sub-sample (None: the whole task)."""
  rng = np.random.default_rng([ord(ch) for ch in case.data_id] + [17])
  return {k: (np.sort(rng.permutation(case.tasks[k][0])[:D_SUBSAMPLE[k]]).astype(np.int32) if k in D_SUBSAMPLE else None)
          for k in range(len(case.tasks))}


# ---- the fp64 reference ------------------------------------------------------------------------------------------------------------
def scale(terms):
  """S_k: the sum of the absolute values of a task's terms."""
  return float(sum(abs(v) for v in terms.values()))


def _oracle_funcs(case):
  return getattr(o, case.mname), getattr(o, case.kname + ('_mlp' if case.mlp else ''))


def _without_kumar(model):
  return {k: v for k, v in model.items() if k != 'kumar_params'}


def oracle_task(case, model64, x, y, adjoint=None):
  """(value, gradient tree without the a / b leaves, terms) of one task: the oracle on fp64 images of the inputs; a Kumaraswamy kernel
  as the base kernel on warped inputs (kumar_oracle.warp), the mean on the inputs as they are."""
  mo, ko = _oracle_funcs(case)
  po = o.GPParams(model=_without_kumar(model64), config=config())
  x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
  if case.kumar:
    kp = model64['kumar_params']
    return o._divergence_sub_dataset_value_and_grad(case.kind, mo, ko, po, kumar_oracle.warp(x, kp['a'], kp['b']), y, WFO, return_terms=True,
                                                    adjoint=adjoint, mean_vx=x)
  return o._divergence_sub_dataset_value_and_grad(case.kind, mo, ko, po, x, y, WFO, return_terms=True, adjoint=adjoint)


def tree_sum(trees):
  out = trees[0]
  for t in trees[1:]:
    out = o._tree_add(out, t)
  return out


class Ref(NamedTuple):
  values: tuple              # per task
  terms: tuple               # per task: name -> term
  scales: tuple              # per task: S_k
  grads: tuple               # per task: gradient tree (no a / b leaves)
  grad_sum: dict             # the sum over the tasks: what hbo_objective returns


def _reference_of(case, tasks, adjoint=None):
  model64 = cast(inputs(case).model, np.float64)
  out = [oracle_task(case, model64, x, y, adjoint) for x, y in tasks]
  return Ref(tuple(v for v, _, _ in out), tuple(t for _, _, t in out), tuple(scale(t) for _, _, t in out), tuple(g for _, g, _ in out),
             tree_sum([g for _, g, _ in out]))


@functools.lru_cache(maxsize=None)
def reference(case):
  """Shared and not to be written to."""
  return _reference_of(case, inputs(case).tasks)


@functools.lru_cache(maxsize=None)
def reference_subsampled(case):
  """reference() on the rows of subsample_rows(case)."""
  rows = subsample_rows(case)
  return _reference_of(case, [(x, y) if rows[k] is None else (x[rows[k]], y[rows[k]]) for k, (x, y) in enumerate(inputs(case).tasks)])


def _value_sum_with_ab(case, a_raw, b_raw):
  model64 = cast(inputs(case).model, np.float64)
  model64['kumar_params'] = {'a': a_raw, 'b': b_raw}
  return sum(oracle_task(case, model64, x, y)[0] for x, y in inputs(case).tasks)


def ab_central_differences(case, h=AB_FD_STEP):
  """d (sum of the tasks' values) / d (raw a, b) by central differences of the oracle value."""
  kp = cast(inputs(case).model['kumar_params'], np.float64)
  out = {}
  for key in ('a', 'b'):
    g = np.zeros(case.d)
    for i in range(case.d):
      hi, lo = {k: v.copy() for k, v in kp.items()}, {k: v.copy() for k, v in kp.items()}
      hi[key][i] += h; lo[key][i] -= h
      g[i] = (_value_sum_with_ab(case, hi['a'], hi['b']) - _value_sum_with_ab(case, lo['a'], lo['b'])) / (2 * h)
    out[key] = g
  return out


@functools.lru_cache(maxsize=None)
def ab_reference(case):
  return ab_central_differences(case)


def _capturing_adjoint(store):
  """The oracle's own adjoint (the formulas of _adjoint without a mutant), which also keeps d f / d K1 of the task in store['dk1']."""
  def adjoint(kind, k1, c0, d, kinv):
    dk1, dmu = _adjoint(None)(kind, k1, c0, d, kinv)
    store['dk1'] = dk1
    return dk1, dmu
  return adjoint


@functools.lru_cache(maxsize=None)
def ab_analytic(case):
  """d (sum of the tasks' values) / d (raw a, b), analytic: the kernel adjoint d f / d K1 of the oracle's backward pass (its adjoint=
  hook hands K1, C0, d and K1^-1 over), through d K / d w of the base kernel and dw/da, dw/db (kumar_cases.ab_from_adjoint).  What the
  device is held to, at AB_TOL; ab_reference, the central differences, is its yardstick on the CPU."""
  model64 = cast(inputs(case).model, np.float64)
  out = {'a': np.zeros(case.d), 'b': np.zeros(case.d)}
  for x, y in inputs(case).tasks:
    store = {}
    oracle_task(case, model64, x, y, _capturing_adjoint(store))
    ab = kumar_cases.ab_from_adjoint(case.kname, model64, x, store['dk1'])
    out = {k: out[k] + ab[k] for k in out}
  return out


def ab_errors(got, ref, tol=AB_FD_TOL):
  """Per leaf: max |got - ref| over (tol |ref| + tol max |ref leaf|), the allclose of test_gpu_kumar.py."""
  out = {}
  for key in ('a', 'b'):
    g, r = np.asarray(got[key], dtype=np.float64).ravel(), np.asarray(ref[key], dtype=np.float64).ravel()
    e = np.abs(g - r) / (tol * np.abs(r) + tol * np.max(np.abs(r)))
    out[key] = float(np.max(e)) if np.isfinite(e).all() else np.inf
  return out


def grad_ratio(got, ref, tol, floor_rel=1e-3):
  """The worst leaf's error over its bound, by the rule of helpers.assert_grad_close (anything not finite: inf), and that leaf."""
  errs = helpers.grad_leaf_errors(got, ref)
  gmax = max((nrm for _, _, nrm in errs), default=0.0)
  worst, leaf = 0.0, ''
  for path, err, nrm in errs:
    r = err / (tol * max(nrm, floor_rel * gmax, 1e-300)) if np.isfinite(err) else np.inf
    if r > worst:
      worst, leaf = r, path
  return worst, leaf


# ---- the value terms, restated -----------------------------------------------------------------------------------------------------
MUTANTS = {
    'c0_m1': 'C0 divided by m - 1 (the unbiased sample covariance)',
    'row_127': 'row 127 of the m + 1 augmented rows [yc_0 .. yc_m-1, d] dropped: the last row of a full tile row (m = 127: d itself; m >= 128: the data row of column 127)',
    'cols_ge_128': 'the data rows of the columns from 128 on dropped',
    'd_col0': 'd taken against column 0 of y instead of the column mean',
    'logdet_half': 'logdet K1 without its factor 2',
    'jitter': "the NLL's jitter left inside K1",
    'task_count': 'the per-task value divided by the task count',
    'dk1_no_c0_nvec': 'the C0 part left out of d f / d K1 for the tasks of the nvec path (m >= 128)',
    'no_guard': 'EUC: d / |d| without the guard at |d| = 0',
}
GRAD_MUTANTS = ('dk1_no_c0_nvec', 'no_guard')


def applicable(case, mutant):
  """By the shapes alone: whether the mutant can differ from the formulas on this case."""
  ms = [m for _, m in case.tasks]
  return {'c0_m1': any(m > 1 for m in ms) and case.special != 'identical', 'row_127': any(m >= 127 for m in ms) and case.special != 'identical',
          'cols_ge_128': any(m > 128 for m in ms) and case.special != 'identical', 'd_col0': any(m > 1 for m in ms) and case.special != 'identical',
          'logdet_half': case.kind == 'ekl', 'jitter': True, 'task_count': len(case.tasks) > 1,
          'dk1_no_c0_nvec': any(m >= 128 for m in ms) and case.special != 'identical',
          'no_guard': case.kind == 'euc' and case.special == 'zero_mean' and case.mname != 'zero'}[mutant]     # (the zero function has no leaf for d f / d mu to reach)


def _params(case, wide):
  """The oracle's parameter container: float32 parameters for the float32 restatement (everything in float32), else fp64 (exact images
  of the case-dtype values; the oracle's kernels and means then compute in the dtype of their inputs)."""
  return o.GPParams(model=cast(inputs(case).model, np.float32 if wide == np.float32 else np.float64), config=config())


def _features(case, po, x):
  if case.mlp:
    return o.mlp_apply(o.retrieve_params(po, ['mlp_params'], WFO)[0], x)
  if case.kumar:
    kp = po.model['kumar_params']
    a, b = kumar_oracle.squareplus(kp['a']).astype(x.dtype), kumar_oracle.squareplus(kp['b']).astype(x.dtype)
    return 1 - (1 - x ** a) ** b
  return x


def restate_task(case, k, wide, mutant=None):
  """The terms of task k (name -> term, in `wide`) by utils.py:84-106 (partial KL) / utils.py:151-173 (Euclid) on the sample statistics of
  objectives.py:57-58, every array in `wide`; `mutant` names the one line that is changed."""
  assert mutant is None or (mutant in MUTANTS and mutant not in GRAD_MUTANTS)
  x, y = inputs(case).tasks[k]
  x, y = x.astype(wide), y.astype(wide)
  n, m = y.shape
  po = _params(case, wide)
  mu1 = np.asarray(getattr(o, case.mname)(po, x, warp_func=WFO), dtype=wide)[:, 0]
  noise = np.asarray(o.retrieve_params(po, ['noise_variance'], WFO)[0], dtype=wide)
  k1 = getattr(o, case.kname)(po, _features(case, po, x), warp_func=WFO) + np.eye(n, dtype=wide) * (noise + (wide(NLL_EPS) if mutant == 'jitter' else wide(0)))
  mu0 = np.sum(y, axis=1) / wide(m)
  rows = (y - mu0[:, None]) / np.sqrt(wide(m - 1 if mutant == 'c0_m1' and m > 1 else m))       # C0 = rows rows^T
  d = mu1 - (y[:, 0] if mutant == 'd_col0' else mu0)
  if mutant == 'row_127' and m >= 128:
    rows = np.delete(rows, 127, axis=1)
  if mutant == 'row_127' and m == 127:
    d = np.zeros_like(d)
  if mutant == 'cols_ge_128':
    rows = rows[:, :128]
  assert k1.dtype == wide and rows.dtype == wide and d.dtype == wide, (k1.dtype, rows.dtype, d.dtype)
  if case.kind == 'ekl':
    c = pc.chol(k1)
    z = pc.solve_lower(c, np.concatenate([rows, d[:, None]], axis=1))
    return {'tr': np.sum(z[:, :-1] ** 2), 'mahalanobis': np.sum(z[:, -1] ** 2), 'logdet': wide(1 if mutant == 'logdet_half' else 2) * np.sum(np.log(np.diag(c)))}
  return {'dnorm': np.sqrt(np.sum(d * d)), 'fnorm': np.sqrt(np.sum((rows @ rows.T - k1) ** 2))}


def restate_value(case, k, wide, mutant=None):
  terms = restate_task(case, k, wide, None if mutant == 'task_count' else mutant)
  v = sum(terms.values())
  return v / wide(len(case.tasks)) if mutant == 'task_count' else v


@functools.lru_cache(maxsize=None)
def reference_ld(case):
  """Per task: the terms in np.longdouble -- the yardstick of the reference's own error, and of the float32 restatement's."""
  return tuple(restate_task(case, k, LD) for k in range(len(case.tasks)))


@functools.lru_cache(maxsize=None)
def f32_levels(case):
  """Per task: |value of the float32 restatement - value of the longdouble one|."""
  return tuple(float(abs(LD(restate_value(case, k, np.float32)) - sum(reference_ld(case)[k].values()))) for k in range(len(case.tasks)))


def value_bounds(case, ref=None):
  """Per task, in the dataset's order.  ref: the reference whose scales to use (reference_subsampled; the fp32 rule needs the whole tasks)."""
  ref = ref or reference(case)
  if case.dtype == 'fp64':
    return tuple(FP64_VALUE * s for s in ref.scales)
  assert ref is reference(case)
  eps32 = float(np.finfo(np.float32).eps)
  return tuple(REL_FACTOR * lvl + FLOOR_C * eps32 * s for lvl, s in zip(f32_levels(case), ref.scales))


def grad_tol(case):
  return FP64_GRAD_TOL if case.dtype == 'fp64' else FP32_GRAD_TOL


# ---- the gradient mutants: wrong adjoints through the oracle's backward pass ------------------------------------------------------------
def _adjoint(mutant):
  def adjoint(kind, k1, c0, d, kinv):
    n, nd = k1.shape[0], np.sqrt(np.sum(d * d))
    fn = np.sqrt(np.sum((c0 - k1) ** 2))
    if mutant == 'dk1_no_c0_nvec':
      c0 = np.zeros_like(c0)       # (only called for the tasks of the nvec path, grad_mutant)
    if kind == 'ekl':
      return kinv - kinv @ (c0 + np.outer(d, d)) @ kinv, 2 * kinv @ d
    with np.errstate(invalid='ignore', divide='ignore'):
      dmu = d / nd if (nd > 0 or mutant == 'no_guard') else np.zeros(n)
    return (k1 - c0) / fn, dmu
  return adjoint


def grad_mutant(case, mutant):
  """The gradient sum over the tasks with the mutant's adjoint."""
  assert mutant in GRAD_MUTANTS
  model64 = cast(inputs(case).model, np.float64)
  trees = []
  for x, y in inputs(case).tasks:
    hit = mutant != 'dk1_no_c0_nvec' or y.shape[1] >= TILE
    trees.append(oracle_task(case, model64, x, y, _adjoint(mutant) if hit else None)[1])
  return tree_sum(trees)


def mutant_ratio(case, mutant):
  """How far the mutant lies from the reference, in bounds of the GPU tier: the worst task's |value - reference| / bound, or (the gradient
  mutants) the worst leaf's error over its bound."""
  if mutant in GRAD_MUTANTS:
    return grad_ratio(grad_mutant(case, mutant), reference(case).grad_sum, grad_tol(case))[0]
  ref, bounds = reference(case), value_bounds(case)
  return max(abs(float(restate_value(case, k, np.float64, mutant)) - ref.values[k]) / bounds[k] for k in range(len(case.tasks)))
