"""CPU side of the Gram tier (csrc/gram.hip: gram_kernel, gram_mfma_kernel, kdiag_kernel; csrc/pair_tile.h; csrc/kernfun.h: stage_x, kfun).
Shared by tests/test_gram_cases_host.py (this file judged on its own, on the CPU) and tests/test_gpu_gram.py (the device against it, PER
ENTRY).  No device, no library call.

  CASES            A: widths (cross Gram 70 x 130, 1..65 features, across the 16-feature LDS chunk); B: shapes across the 64-row and
                   128-column tile edges, cross and symmetric; C: graded distances u = 0 ... 1400 on inputs offset by 0 / 10 / 1000;
                   D: the posterior's padded cross Gram (hbo_probe_gram form 1); E: the batched symmetric task form (form 2), one model
                   and one model per task; F: diag = 1 (kdiag_kernel)
  inputs(case)     x1 / x2 (or the task list) and the model parameters in the case's dtype, seeded by the case's data key: fp64 and fp32
                   see the same numbers, the fp32 ones rounded once, here
  reference        the four covariances in np.longdouble from the ROUNDED inputs and parameters, 1 / lengthscale as the fp64 quotient
                   the device receives (hbo_internal.h: model_dev_fill)
  bound            per entry, from the kernel's own arithmetic (below); never from a device result
  restate          the kernel's arithmetic in NumPy float32 / float64 (feature by feature, in the kernel's order), and the MUTANTS
  judge(case, got) every assertion of a case on what the device (or fake(case, mutant)) returned; the largest error / bound

The bound.  gram_kernel computes u = sum_d (a_d s_d - b_d s_d)^2 in the model dtype T, s_d = (T)(1 / lengthscale_d).  The two products
round relative to |a_d| s_d and |b_d| s_d, the difference, the square, the rounding of s_d and the fdim - 1 additions relative to the
terms of u themselves.  To first order, with eps the unit roundoff of T:
    |du| <= eps U,   U = sum_d 2 |a_d - b_d| s_d^2 (|a_d| + |b_d|) + (fdim + 4) u
    |dk| <= 2 (eps (|dk/du| U + (8 + 2 r) k) + tiny)
r the argument of the exponential (u / 2, sqrt(3u), sqrt(5u): an argument off by eps r moves e^-r by eps r e^-r; the polynomial in
front, the product with the signal variance and the exponential itself are the 8), tiny the smallest normal of T (fp32 tails underflow), the
outer 2 the margin for the second-order terms and the device's exp / sqrt (<= 1.5 ulp: test_device_exp_against_numpy).  Dot product:
    |dk| <= 2 eps ((fdim + 2) sum_d |a_d b_d| / sigma^2 + 2 |k|)
On the diagonal of the task form the kernel adds (T)(noise + eps_jitter) in T: one more rounding, eps |k + noise + eps_jitter|.  Where an
fp32 case runs on the matrix cores the bound is this one plus the kernel's documented budget of 1e-6 sv (gram.hip, "Accuracy").
"""
import functools
from typing import NamedTuple, Tuple

import numpy as np

LD = np.longdouble
DC, GTR, TILE = 16, 64, 128        # kernfun.h: DC, GTR; hbo_internal.h: HBO_TILE
MFMA_MIN_F = 32                    # ctx.h: opt_gram_mfma
MFMA_BUDGET = 1e-6                 # gram.hip, "Accuracy": of the signal variance
SENTINEL = -7.25                   # exact in both dtypes; no covariance of the table takes it
STATIONARY = ('squared_exponential', 'matern32', 'matern52')
KERNELS = STATIONARY + ('dot_product',)
KERNEL_ID = {k: i for i, k in enumerate(KERNELS)}      # include/hbo.h: hbo_kernel_id
SV, NOISE, JITTER, DOT_BIAS = 0.8, 0.01, 1e-6, 0.2
RESTATE_SHARE = 0.5                # the restatement stays at or below this share of the bound (the reference's own yardstick)


class Case(NamedTuple):
  group: str                 # 'A' .. 'F'
  kname: str
  dtype: str                 # 'fp64' | 'fp32'
  fdim: int
  n1: int = 0
  n2: int = 0                # 0: x2 = None (symmetric call, or diag)
  engine: str = 'valu'       # 'valu': gram_kernel (fp64; fp32 below MFMA_MIN_F, with gram_mfma = 0 or direct_form); 'mfma': gram_mfma_kernel
  ctx: str = 'default'       # 'default' | 'direct' (a context with gram_mfma = 0)
  offset: float = 0.0
  direct_form: int = 0       # group D
  tasks: Tuple[int, ...] = ()    # group E: n of every task, in the caller's order
  per_task: bool = False     # group E: one model per task (model_stride 1)

  @property
  def np_dtype(self):
    return np.float64 if self.dtype == 'fp64' else np.float32

  @property
  def shape_id(self):
    if self.tasks:
      return 'T' + '_'.join(str(n) for n in self.tasks) + ('-permodel' if self.per_task else '-onemodel')
    return f'{self.n1}x{self.n2}' if self.n2 else f'{self.n1}{"diag" if self.group == "F" else "sym"}'

  @property
  def id(self):
    return (f'{self.group}-{self.kname}-{self.dtype}-f{self.fdim}-{self.shape_id}-{self.engine}' + (f'-off{self.offset:g}' if self.offset else '') +
            ('-direct' if self.direct_form else '') + ('-ctxdirect' if self.ctx == 'direct' else ''))

  @property
  def data_key(self):
    """What the inputs depend on: neither kernel nor dtype nor engine."""
    return (self.group, self.fdim, self.n1, self.n2, self.offset, self.tasks, self.per_task)


DTYPES = ('fp64', 'fp32')
A_WIDTHS = (1, 2, 15, 16, 17, 31, 32, 33, 48, 65)
A_SHAPE = (70, 130)
B_FDIMS = (3, 17)
B_CROSS = ((1, 1), (1, 129), (63, 127), (64, 128), (65, 129), (129, 1), (128, 256), (200, 300))
B_SYM = (1, 63, 64, 65, 127, 128, 129, 193, 300)
C_FDIMS = (2, 17)
C_OFFSETS = (0.0, 10.0, 1000.0)
C_BASE = 8
C_TARGETS = (0.0, 1e-16, 1e-12, 1e-8, 1e-4, 1e-2, 1.0, 10.0, 100.0, 170.0, 1400.0)   # u of the graded pairs; 170: fp32's exp(-85), 1400: SE's exp(-700)
D_SHAPES = ((130, 1), (130, 129), (200, 300))
D_FDIMS = (3, 17)
D_MFMA_FDIM = 33
E_TASKS = (1, 64, 65, 128, 129, 257, 300)
E_FDIMS = (3, 17)
E_MFMA_FDIMS = (33, 40)
E_SINGLE = (600,)
F_N = (1, 255, 256, 257)
F_FDIM = 17


def _engine(dtype, kname, fdim, ctx='default', direct_form=0):
  mfma = dtype == 'fp32' and kname != 'dot_product' and fdim >= MFMA_MIN_F and ctx == 'default' and not direct_form
  return 'mfma' if mfma else 'valu'


def _case(group, kname, dtype, fdim, ctx='default', **kw):
  return Case(group, kname, dtype, fdim, engine=_engine(dtype, kname, fdim, ctx, kw.get('direct_form', 0)), ctx=ctx, **kw)


# A.  fp64 on the default context; fp32 on the gram_mfma = 0 context (VALU at every width) and again on the default one from 32 features on
GROUP_A = ([_case('A', k, 'fp64', f, n1=A_SHAPE[0], n2=A_SHAPE[1]) for f in A_WIDTHS for k in KERNELS] +
           [_case('A', k, 'fp32', f, ctx='direct', n1=A_SHAPE[0], n2=A_SHAPE[1]) for f in A_WIDTHS for k in KERNELS] +
           [_case('A', k, 'fp32', f, n1=A_SHAPE[0], n2=A_SHAPE[1]) for f in A_WIDTHS if f >= MFMA_MIN_F for k in STATIONARY])
GROUP_B = [_case('B', k, dt, f, n1=n1, n2=n2) for dt in DTYPES for f in B_FDIMS for n1, n2 in B_CROSS + tuple((n, 0) for n in B_SYM)
           for k in KERNELS]
GROUP_C = [_case('C', k, dt, f, n1=C_BASE, n2=C_BASE * len(C_TARGETS), offset=off) for dt in DTYPES for f in C_FDIMS for off in C_OFFSETS for k in STATIONARY]
GROUP_D = ([_case('D', k, dt, f, n1=n1, n2=n2, direct_form=df) for dt in DTYPES for f in D_FDIMS for n1, n2 in D_SHAPES for df in (0, 1) for k in KERNELS] +
           [_case('D', k, 'fp32', D_MFMA_FDIM, n1=n1, n2=n2, direct_form=df) for n1, n2 in D_SHAPES for df in (0, 1) for k in STATIONARY])
GROUP_E = ([_case('E', k, dt, f, tasks=E_TASKS, per_task=pt) for dt in DTYPES for f in E_FDIMS for pt in (False, True) for k in KERNELS] +
           [_case('E', k, 'fp32', f, tasks=E_TASKS, per_task=pt) for f in E_MFMA_FDIMS for pt in (False, True) for k in STATIONARY] +
           [_case('E', k, dt, 3, tasks=E_SINGLE) for dt in DTYPES for k in KERNELS] +
           [_case('E', 'squared_exponential', 'fp32', 33, tasks=E_SINGLE)])
GROUP_F = [_case('F', k, dt, F_FDIM, n1=n) for dt in DTYPES for n in F_N for k in ('dot_product', 'matern32')]
CASES = GROUP_A + GROUP_B + GROUP_C + GROUP_D + GROUP_E + GROUP_F
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def round_up(n, q):
  return (n + q - 1) // q * q


def padded_ld(extent, np_dtype):
  """runtime.h: padded_ld -- the extent plus 128 bytes."""
  return extent + 128 // np.dtype(np_dtype).itemsize


def lengthscales(rng, fdim):
  """Every one distinct, a factor 5 between the smallest and the largest, in an order of their own; around 0.5 sqrt(fdim), so that the
  Gram of inputs in [0, 1]^fdim neither decays to the diagonal nor fills with the signal variance."""
  return 0.5 * np.sqrt(fdim) * rng.permutation(np.geomspace(0.5, 2.5, fdim)) if fdim > 1 else np.array([0.6])


def _model(ls, T, z=0):
  """The parameters as the device sees them: length-scales in T; the scalars are doubles of hbo_model that the kernels cast to T, chosen
  representable in T so that the cast is exact.  z: the task of a per-task model (other length-scales, signal variance and noise)."""
  fdim = ls.size
  sigma = float(T(0.5 * np.sqrt(fdim) * (1 + 0.25 * z)))
  return {'ls': (ls * (1 + 0.3 * z)).astype(T), 'sv': float(T(SV * (1 + 0.25 * z))), 'noise': float(T(NOISE * (1 + z))), 'jitter': JITTER,
          'sigma': sigma, 'bias': float(T(DOT_BIAS))}


@functools.lru_cache(maxsize=None)
def _raw_inputs(data_key):
  group, fdim, n1, n2, offset, tasks, per_task = data_key
  rng = np.random.default_rng([ord(group), fdim, n1, n2, int(offset), len(tasks), int(per_task)])
  ls = lengthscales(rng, fdim)
  if group == 'C':
    x1 = rng.uniform(size=(C_BASE, fdim)) + offset
    sign = rng.choice([-1.0, 1.0], size=(n2, fdim))
    x2 = np.empty((n2, fdim))
    for j in range(n2):
      x2[j] = x1[j % C_BASE] + sign[j] * np.sqrt(C_TARGETS[j // C_BASE] / fdim) * ls
    return ls, [x1, x2]
  if tasks:
    return ls, [rng.uniform(size=(n, fdim)) for n in tasks]
  x1 = rng.uniform(size=(n1, fdim)) + offset
  x2 = rng.uniform(size=(n2, fdim)) + offset if n2 else None
  if n2 and min(n1, n2) >= 3:
    x2[-1] = x1[0]                                # an exact duplicate across the sets
  elif not n2 and n1 >= 3:
    x1[-1] = x1[1]                                # ... and inside a symmetric one
  return ls, [x1, x2]


def inputs(case):
  """(xs, models): xs = [x1, x2 or None] (groups A-D, F) or the tasks' inputs (group E), in the case's dtype; models: one dict, or one
  per task."""
  T = case.np_dtype
  ls, xs = _raw_inputs(case.data_key)
  xs = [None if x is None else np.ascontiguousarray(x.astype(T)) for x in xs]
  models = [_model(ls, T, z) for z in range(len(case.tasks))] if case.per_task else [_model(ls, T)]
  return xs, models


# ---- reference and bound -----------------------------------------------------------------------------------------------------------
def inv_ls64(p):
  return 1.0 / p['ls'].astype(np.float64)          # model_dev_fill: the fp64 quotient of the length-scale as stored


def dot_coefs(p, T):
  """pair_tile.h: pair_coef -- (T)(1 / sigma^2) and (T)(bias^2), both formed in fp64."""
  return T(1.0 / (p['sigma'] * p['sigma'])), T(p['bias'] * p['bias'])


def diag_add(p, T):
  return T(p['noise'] + p['jitter'])               # gram_kernel: (T)(md->noise + md->eps)


def pair_terms(x1, x2, inv):
  """Over all pairs: u = sum ((a - b) inv)^2 and sum a b in longdouble; U1 = sum 2 |a - b| inv^2 (|a| + |b|) and sum |a b| in fp64."""
  n1, n2 = x1.shape[0], x2.shape[0]
  u, ab = np.zeros((n1, n2), LD), np.zeros((n1, n2), LD)
  U1, abs_ab = np.zeros((n1, n2)), np.zeros((n1, n2))
  a_, b_ = x1.astype(LD), x2.astype(LD)
  for d in range(x1.shape[1]):
    a, b, s = a_[:, d][:, None], b_[:, d][None, :], LD(inv[d])
    diff = a - b
    t = diff * s
    u += t * t
    prod = a * b
    ab += prod
    ap = np.abs(prod).astype(np.float64)
    abs_ab += ap
    U1 += 2.0 * np.abs(diff).astype(np.float64) * float(s) ** 2 * (np.abs(a) + np.abs(b)).astype(np.float64)
  return u, ab, U1, abs_ab


def cov_ld(kname, u, sv):
  """k(u) of a stationary covariance in longdouble (kernel.py:63-123), and r, |dk/du|."""
  u, sv = np.asarray(u, LD), LD(sv)
  if kname == 'squared_exponential':
    k = sv * np.exp(-u / 2)
    return k, u / 2, k / 2
  if kname == 'matern32':
    r = np.sqrt(3 * u)
    e = sv * np.exp(-r)
    return e * (1 + r), r, LD(1.5) * e
  r = np.sqrt(5 * u)
  e = sv * np.exp(-r)
  return e * (1 + r + r * r / 3), r, (LD(5) / 6) * e * (1 + r)


def gram_ref(kname, x1, x2, p, T, terms=None):
  """(reference in longdouble, per-entry bound in fp64) of K(x1, x2) for VALU arithmetic in T; x2 = None: K(x1, x1).  terms: what
  pair_terms gave for these inputs and length-scales."""
  T = np.dtype(T).type
  x2 = x1 if x2 is None else x2
  fdim = x1.shape[1]
  eps, tiny = float(np.finfo(T).eps) / 2, float(np.finfo(T).tiny)
  u, ab, U1, abs_ab = terms if terms is not None else pair_terms(x1, x2, inv_ls64(p))
  if kname == 'dot_product':
    is2, b2 = dot_coefs(p, T)
    ref = ab * LD(is2) + LD(b2)
    return ref, 2.0 * eps * ((fdim + 2) * abs_ab * float(is2) + 2.0 * np.abs(ref).astype(np.float64))
  k, r, dkdu = cov_ld(kname, u, T(p['sv']))
  U = U1 + (fdim + 4) * u.astype(np.float64)
  bound = 2.0 * (eps * (dkdu.astype(np.float64) * U + (8.0 + 2.0 * r.astype(np.float64)) * k.astype(np.float64)) + tiny)
  return k, bound


def _operands(case, z, model_z):
  xs, models = inputs(case)
  return (xs[z], xs[z], models[model_z]) if case.tasks else (xs[0], xs[0] if xs[1] is None else xs[1], models[model_z])


@functools.lru_cache(maxsize=32)
def _terms_cached(data_key, dtype, z, model_z):
  """pair_terms of a case's operands: the same for every covariance (cases that share their data follow each other in CASES)"""
  case = Case(data_key[0], '', dtype, data_key[1], data_key[2], data_key[3], offset=data_key[4], tasks=data_key[5], per_task=data_key[6])
  x1, x2, p = _operands(case, z, model_z)
  return pair_terms(x1, x2, inv_ls64(p))


@functools.lru_cache(maxsize=32)
def _expected_cached(data_key, kname, dtype, z, model_z):
  case = Case(data_key[0], kname, dtype, data_key[1], data_key[2], data_key[3], offset=data_key[4], tasks=data_key[5], per_task=data_key[6])
  x1, x2, p = _operands(case, z, model_z)
  return gram_ref(kname, x1, x2, p, case.np_dtype, _terms_cached(data_key, dtype, z, model_z))


def expected(case, z=0, model_z=None):
  """(ref, bound) of the data region of `case` (task z of group E, under model model_z: its own, or the one model), the matrix-core
  budget added where the case runs there.  The diagonal term of the task form is NOT in it (judge_tasks adds it)."""
  if model_z is None:
    model_z = z if case.per_task else 0
  ref, bound = _expected_cached(case.data_key, case.kname, case.dtype, z, model_z)
  if case.engine == 'mfma':
    bound = bound + MFMA_BUDGET * inputs(case)[1][model_z]['sv']
  return ref, bound


# ---- the kernel's arithmetic restated ----------------------------------------------------------------------------------------------
def restate(kname, x1, x2, p, T, ls_shift=False, drop_partial=False, matern_u0=None):
  """gram_kernel in NumPy arithmetic of dtype T: features in order, (a s - b s)^2 summed in T, the covariance in T.  The mutants:
  ls_shift: feature d >= DC takes the length-scale of feature d - DC; drop_partial: the partial last feature chunk is left out;
  matern_u0: the factor a Matern covariance returns at u = 0 in place of 1."""
  T = np.dtype(T).type
  x2 = x1 if x2 is None else x2
  fdim = x1.shape[1]
  dot = kname == 'dot_product'
  inv = inv_ls64(p)
  nfeat = fdim - fdim % DC if drop_partial else fdim
  acc = np.zeros((x1.shape[0], x2.shape[0]), T)
  for d in range(nfeat):
    s = T(1) if dot else T(inv[d - DC] if ls_shift and d >= DC else inv[d])
    a, b = (x1[:, d] * s)[:, None], (x2[:, d] * s)[None, :]
    if dot:
      acc += a * b
    else:
      df = a - b
      acc += df * df
  assert acc.dtype == T
  if dot:
    is2, b2 = dot_coefs(p, T)
    return acc * is2 + b2
  sv = T(p['sv'])
  if kname == 'squared_exponential':
    return sv * np.exp(T(-0.5) * acc)
  r = np.sqrt(T(3 if kname == 'matern32' else 5) * acc)
  poly = (T(1) + r) if kname == 'matern32' else (T(1) + r + r * r / T(3))
  out = sv * poly * np.exp(-r)
  if matern_u0 is not None:
    out = np.where(acc == 0, T(p['sv'] * matern_u0), out)
  return out.astype(T)


def restate_diag(kname, x, p, T):
  """kdiag_kernel: the signal variance, or sum v^2 in T over sigma^2 plus bias^2."""
  T = np.dtype(T).type
  if kname != 'dot_product':
    return np.full(x.shape[0], T(p['sv']), T)
  is2, b2 = dot_coefs(p, T)
  s = np.zeros(x.shape[0], T)
  for d in range(x.shape[1]):
    s += x[:, d] * x[:, d]
  return s * is2 + b2


# ---- layouts -----------------------------------------------------------------------------------------------------------------------
def pt_col(vec, tx, q):
  """pair_tile.h: pt_col -- column, from the tile's first, of element q of thread tx's eight, VEC = vec."""
  return 16 * vec * (q // vec) + vec * tx + q % vec


def padded_layout(case):
  """(rows, n2pad, ld) of the posterior's cross-Gram workspace (api_internal.h: PostChunk)."""
  n2pad = round_up(case.n2, TILE)
  return round_up(case.n1, TILE), n2pad, padded_ld(n2pad, case.np_dtype)


def task_layout(n, np_dtype):
  """(npad, ld) of a task's A (dataset.hip: hbo_dataset_create, through api_internal.h's task_shape)."""
  npad = round_up(n, TILE)
  return npad, padded_ld(npad, np_dtype)


def interior_tiles(case):
  """(r0, c0) of gram_kernel's tiles of the padded cross form that take the straight epilogue: all 64 x 128 elements are data."""
  return [(r0, c0) for r0 in range(0, case.n1 - GTR + 1, GTR) for c0 in range(0, case.n2 - TILE + 1, TILE)]


# ---- what a correct device returns, and the mutants --------------------------------------------------------------------------------
MUTANTS = {   # name -> the groups in which it must be rejected
    'ls_shift': 'A', 'drop_partial_chunk': 'A', 'swap_row_halves': 'BD', 'pt_col_vec2': 'AB', 'one_entry_8x': 'B', 'flush_tails': 'C',
    'matern_u0': 'C', 'missing_pad_zeros': 'D', 'interior_shift': 'D', 'no_diag_term': 'E', 'diag_term_in_cross': 'D', 'pad_diag_zero': 'E',
    'model0_for_all': 'E', 'upper_tile_written': 'E', 'dot_diag_no_bias': 'F',
}


def _values(case, mutant, z=0):
  """The restated data region of `case` (task z), with the mutants that act on the values."""
  T = case.np_dtype
  xs, models = inputs(case)
  p = models[z if case.per_task and mutant != 'model0_for_all' else 0]
  x1, x2 = (xs[z], None) if case.tasks else (xs[0], xs[1])
  v = restate(case.kname, x1, x2, p, T, ls_shift=mutant == 'ls_shift', drop_partial=mutant == 'drop_partial_chunk',
              matern_u0=(1 - 1e-7) if mutant == 'matern_u0' else None)
  n1, n2 = v.shape
  if mutant == 'swap_row_halves':
    assert n1 >= TILE
    v = v.copy()
    v[:GTR], v[GTR:TILE] = v[GTR:TILE].copy(), v[:GTR].copy()
  if mutant == 'pt_col_vec2':
    assert T == np.float32
    w = v.copy()
    for c0 in range(0, n2, TILE):
      for tx in range(16):
        for q in range(8):
          src, dst = c0 + pt_col(2, tx, q), c0 + pt_col(4, tx, q)
          if src < n2 and dst < n2:
            w[:, dst] = v[:, src]
    v = w
  if mutant == 'one_entry_8x':
    v = v.copy()
    v[-1, -1] = T(np.float64(v[-1, -1]) + 8.0 * expected(case, z)[1][-1, -1])
  if mutant == 'flush_tails':
    v = np.where(np.abs(v) < 1e-30 * p['sv'], T(0), v)
  if mutant == 'diag_term_in_cross':
    v = v.copy()
    m = min(n1, n2)
    v[np.arange(m), np.arange(m)] += diag_add(p, T)
  return v


def fake(case, mutant=None):
  """What a device that computes as restate() does would hand to judge(): the dense result (A-C), the diagonal (F), (buffer, rows, ld)
  of form 1 (D) or [(buffer, rows, ld)] per task of form 2 (E) -- or, with `mutant`, what a device with that fault would."""
  T = case.np_dtype
  xs, models = inputs(case)
  if case.group == 'F':
    p = models[0]
    out = restate_diag(case.kname, xs[0], p, T)
    if mutant == 'dot_diag_no_bias':
      out = out - dot_coefs(p, T)[1]
    return out
  if case.group in 'ABC':
    return _values(case, mutant)
  if case.group == 'D':
    rows, n2pad, ld = padded_layout(case)
    buf = np.full((rows, ld), T(SENTINEL), T)
    buf[:, :n2pad] = 0
    v = _values(case, mutant)
    buf[:case.n1, :case.n2] = v
    if mutant == 'missing_pad_zeros':
      buf[:, n2pad - 1] = T(SENTINEL)
    if mutant == 'interior_shift':
      vec = 16 // np.dtype(T).itemsize
      tiles = interior_tiles(case)
      assert tiles
      for r0, c0 in tiles:
        buf[r0:r0 + GTR, c0:c0 + vec] = T(SENTINEL)
      for r0, c0 in tiles:
        buf[r0:r0 + GTR, c0 + vec:c0 + TILE + vec] = v[r0:r0 + GTR, c0:c0 + TILE]
    return buf, rows, ld
  out = []
  for z, n in enumerate(case.tasks):
    p = models[z if case.per_task else 0]
    npad, ld = task_layout(n, T)
    buf = np.full((npad, ld), T(SENTINEL), T)
    full = np.zeros((npad, npad), T)
    full[:n, :n] = _values(case, mutant, z)
    idx = np.arange(npad)
    full[idx[:n], idx[:n]] += T(0) if mutant == 'no_diag_term' else diag_add(p, T)
    full[idx[n:], idx[n:]] = T(0) if mutant == 'pad_diag_zero' else T(1)
    for ti in range(npad // TILE):
      for tj in range(ti + 1):
        buf[ti * TILE:(ti + 1) * TILE, tj * TILE:(tj + 1) * TILE] = full[ti * TILE:(ti + 1) * TILE, tj * TILE:(tj + 1) * TILE]
    if mutant == 'upper_tile_written' and npad >= 2 * TILE:
      buf[:TILE, TILE:2 * TILE] = full[:TILE, TILE:2 * TILE]
    out.append((buf, npad, ld))
  return out


# ---- the assertions ----------------------------------------------------------------------------------------------------------------
def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _is_sentinel(a):
  return _bits(a) == _bits(np.array([SENTINEL], a.dtype))[0]


def _per_entry(label, got, ref, bound):
  """every entry within its bound; the largest error / bound"""
  assert got.shape == ref.shape, (label, got.shape, ref.shape)
  err = np.abs(got.astype(LD) - ref).astype(np.float64)
  ok = err <= bound                                  # (a NaN fails)
  if not np.all(ok):
    i = np.unravel_index(np.argmax(np.where(ok, 0.0, np.where(np.isnan(err), np.inf, err / bound))), err.shape)
    raise AssertionError(f'{label}: entry {tuple(int(k) for k in i)}: device {got[i]!r}, reference {float(ref[i])!r}, |error| {err[i]:.3e} = '
                         f'{err[i] / bound[i]:.2f} x its bound {bound[i]:.3e}; {int(np.sum(~ok))} of {ok.size} entries out of bounds')
  return float(np.max(err / bound)) if err.size else 0.0


def _duplicates_exact(case, got, x1, x2, p):
  """pairs of identical rows: exactly (T)sv from the VALU kernel (u = 0 exactly, exp(0) = 1, the polynomial 1)"""
  if case.kname == 'dot_product' or case.engine != 'valu':
    return
  dup = np.all(x1[:, None, :] == x2[None, :, :], axis=2)
  want = case.np_dtype(p['sv'])
  bad = dup & (_bits(got) != _bits(np.array([want]))[0])
  assert not np.any(bad), f'{case.id}: duplicate pair {tuple(int(k[0]) for k in np.nonzero(bad))} gives {got[bad][0]!r}, not exactly {want!r}'


def judge_dense(case, got):
  xs, models = inputs(case)
  x1, x2 = xs[0], xs[0] if xs[1] is None else xs[1]
  assert got.dtype == case.np_dtype and got.shape == (x1.shape[0], x2.shape[0]), (case.id, got.dtype, got.shape)
  ref, bound = expected(case)
  ratio = _per_entry(case.id, got, ref, bound)
  _duplicates_exact(case, got, x1, x2, models[0])
  if xs[1] is None and case.engine == 'valu':
    assert np.array_equal(_bits(got), _bits(got.T)), f'{case.id}: the symmetric Gram differs from its transpose'
  return ratio


def judge_diag(case, got):
  xs, models = inputs(case)
  p, T = models[0], case.np_dtype
  assert got.dtype == T and got.shape == (case.n1,), (case.id, got.dtype, got.shape)
  if case.kname != 'dot_product':
    assert np.all(_bits(got) == _bits(np.array([T(p['sv'])]))[0]), f'{case.id}: k(x, x) is not exactly the signal variance'
    return 0.0
  ref, bound = expected(case)
  return _per_entry(case.id, got, np.diagonal(ref), np.diagonal(bound))


def judge_padded(case, got):
  buf, rows, ld = got
  want_rows, n2pad, want_ld = padded_layout(case)
  assert (rows, ld) == (want_rows, want_ld) and buf.shape == (rows, ld) and buf.dtype == case.np_dtype, (case.id, rows, ld, buf.shape)
  n1, n2 = case.n1, case.n2
  ref, bound = expected(case)
  ratio = _per_entry(case.id, buf[:n1, :n2], ref, bound)
  xs, models = inputs(case)
  _duplicates_exact(case, buf[:n1, :n2], xs[0], xs[1], models[0])
  for name, block in (('rows beyond n1', buf[n1:rows, :n2pad]), ('columns beyond n2', buf[:rows, n2:n2pad])):
    bad = _bits(block) != 0
    assert not np.any(bad), f'{case.id}: {name}: {int(np.sum(bad))} elements of the padding are not +0, first at {tuple(int(k[0]) for k in np.nonzero(bad))}'
  out = ~_is_sentinel(buf[:, n2pad:])
  assert not np.any(out), f'{case.id}: {int(np.sum(out))} elements beyond the padded extent were written'
  return ratio


def judge_tasks(case, got):
  xs, models = inputs(case)
  T = case.np_dtype
  assert len(got) == len(case.tasks)
  worst = 0.0
  eps = float(np.finfo(T).eps) / 2
  for z, (n, (buf, rows, ld)) in enumerate(zip(case.tasks, got)):
    label = f'{case.id} task {z} (n = {n})'
    p = models[z if case.per_task else 0]
    npad, want_ld = task_layout(n, T)
    assert (rows, ld) == (npad, want_ld) and buf.shape == (rows, ld) and buf.dtype == T, (label, rows, ld, buf.shape)
    ref, bound = expected(case, z)
    dg = diag_add(p, T)
    idx = np.arange(n)
    ref, bound = ref.copy(), bound.copy()
    ref[idx, idx] += LD(dg)
    bound[idx, idx] += eps * np.abs(ref[idx, idx]).astype(np.float64)
    low = np.tril(np.ones((n, n), bool))
    sq = buf[:npad, :npad]
    worst = max(worst, _per_entry(label + ', lower triangle', np.where(low, sq[:n, :n], T(0)), np.where(low, ref, LD(0)), bound))
    # the padding of the lower tiles: identity
    r, c = np.meshgrid(np.arange(npad), np.arange(npad), indexing='ij')
    pad_low = (c <= r) & ((r >= n) | (c >= n))
    want = np.where(r == c, T(1), T(0)).astype(T)
    bad = pad_low & (_bits(sq) != _bits(want))
    assert not np.any(bad), f'{label}: padding is not the identity at {tuple(int(k[0]) for k in np.nonzero(bad))}: {sq[bad][0]!r}'
    # above the diagonal: tiles strictly above the tile diagonal untouched; inside a diagonal tile the sentinel or the exact mirror
    upper_tile = (c // TILE) > (r // TILE)
    bad = upper_tile & ~_is_sentinel(sq)
    assert not np.any(bad), f'{label}: a tile above the diagonal was written, first at {tuple(int(k[0]) for k in np.nonzero(bad))}'
    in_diag_tile = (c > r) & ~upper_tile
    bad = in_diag_tile & ~_is_sentinel(sq) & (_bits(sq) != _bits(sq.T))
    assert not np.any(bad), f'{label}: above the diagonal at {tuple(int(k[0]) for k in np.nonzero(bad))}: {sq[bad][0]!r} is neither the sentinel nor the mirror {sq.T[bad][0]!r}'
    out = ~_is_sentinel(buf[:, npad:])
    assert not np.any(out), f'{label}: {int(np.sum(out))} elements beyond the padded extent were written'
  return worst


def judge(case, got):
  """Every assertion of `case` on `got`; returns the largest error / bound over its entries."""
  if case.group == 'F':
    return judge_diag(case, got)
  if case.group == 'D':
    return judge_padded(case, got)
  if case.group == 'E':
    return judge_tasks(case, got)
  return judge_dense(case, got)
