"""CPU side of the gradient-contraction tier (csrc/grad.hip: grad_contract_kernel, grad_prereduce_kernel, grad_finalize_kernel,
grad_feat_kernel; csrc/pair_tile.h: pt_g_dkdu).  Shared by tests/test_grad_contract_cases_host.py (this file judged on its own, on the CPU)
and tests/test_gpu_grad_contract.py (the device, through the test hook hbo_probe_grad_contract of include/hbo_tune.h, PER TASK AND LEAF).
No device, no library call.

  CASES            A row edges of the half-tile grid; B feature chunks and column strips; C the four covariances; D a ragged batch, both
                   orders; E EKL / EUC with 1..9 outer-product vectors, the Frobenius slot, EUC's rescaled dF; F the mean leaves across the
                   x4 unrolled loops; G the two-step column sum (32 blocks); H dF per row and feature; N the anchor (G of a real NLL)
  inputs(case)     features, s (where K^-1 stands), vectors, coefficients, d f / d mu and the model: every number representable in fp32, so
                   that fp64 and fp32 see the same operands and ONE longdouble reference serves both
  reference(case)  every half-tile slot, every leaf of every task and dF in np.longdouble from the formulas at the head of grad.hip (k from
                   oracle/hyperbo_oracle.py: _pair_kernel_matrix), with the un-cancelled scale S of each: sum |G_ij| |dK_ij / dtheta|
  restate          the kernels' arithmetic in NumPy float32 / float64 in the kernels' order (u accumulated feature by feature in T; k, G, gw
                   in T; the thread's 4 x 8 products summed in T; everything else in fp64; half-tile slots; weight 2 off the tile
                   diagonal; column sums; chain-rule factors), and the MUTANTS
  judge            a device (or restated) result against the bound, per task and leaf; the largest error / bound

The bound of a slot total is  C1 |restatement - reference| + C2 eps_T S_slot  and a leaf takes it through its chain-rule factor (EUC:
through 1 / sqrt(Frobenius slot) as well, to first order).  The first term is what rounding the operands to T and forming u, k, G and the
products in T costs -- the device does the same, so it may be off by as much again (C1 = 2); the second covers what the device does in
another order or with another rounding (fused multiply-adds, its exp, the order of the fp64 sums).  C2 is measured by the host test as the
smallest round number with the restatement at <= RESTATE_SHARE of the bound on every case; the mean leaves are fp64 sums of fp64 products
whatever T is and take eps of fp64.  dF adds the reorder term of its fp64 atomics, REORDER_ADDS eps64 S per block row of the task.
"""
import functools
import math
from typing import NamedTuple, Tuple

import numpy as np

from oracle import hyperbo_oracle as o

LD = np.longdouble
DC, GTR, TILE, QW, PRE_ROWS = 16, 64, 128, 32, 32       # kernfun.h: DC, GTR; HBO_TILE; grad_finalize_kernel: QW; HBO_GRAD_PRE_ROWS
KERNELS = ('squared_exponential', 'matern32', 'matern52', 'dot_product')
KERNEL_ID = {k: i for i, k in enumerate(KERNELS)}
MEANS = ('zero', 'constant', 'linear', 'linear_mlp')
MEAN_ID = {k: i for i, k in enumerate(MEANS)}
OBJS = ('nll', 'ekl', 'euc')
OBJ_ID = {k: i for i, k in enumerate(OBJS)}
SV, NOISE, DOT_BIAS = 0.8, 0.01, 0.2
C1, C2 = 2.0, 20.0              # see the module docstring and profiles/grad_contract_errors.md
RESTATE_SHARE = 0.25
REORDER_ADDS = 16
ROUND = (1.0, 2.0, 5.0, 10.0, 20.0, 50.0, 100.0)     # what "a round number" means for C2
MUTANT_FACTOR = 10.0
SHARE_MIN = 0.01                # every half tile carries this much of S of every slot it reaches ...
SHARE_MAX_TILES = 100           # ... on grids of at most this many half tiles (the shares sum to 1); beyond: SHARE_FAIR of an equal share
SHARE_FAIR = 0.05
ANCHOR_TOL = 1e-12
DTYPES = ('fp64', 'fp32')
MUTANTS = ('drop_half_tile', 'weight1', 'diag_upper_skipped', 'mask_off_by_one', 'last_chunk_cut', 'second_strip_dropped',
           'prereduce_row_skipped', 'neighbour_slot', 'fro_g0g0', 'a_g_omitted')


class Case(NamedTuple):
  group: str
  kname: str
  dtype: str
  ns: Tuple[int, ...]
  fdim: int = 3
  obj: str = 'nll'
  nvec: int = 1
  mean: str = 'zero'
  scalar_ls: bool = False
  mlp: bool = False          # an MLP kernel: x is F, dF comes back

  @property
  def np_dtype(self):
    return np.float64 if self.dtype == 'fp64' else np.float32

  @property
  def id(self):
    return (f'{self.group}-{self.kname}-{self.dtype}-{self.obj}-n{"_".join(map(str, self.ns))}-f{self.fdim}-v{self.nvec}-{self.mean}' +
            ('-scalar' if self.scalar_ls else '') + ('-mlp' if self.mlp else ''))

  @property
  def data_key(self):
    return self._replace(dtype='')

  @property
  def nacc(self):
    return 4 if self.kname == 'dot_product' else self.fdim + 3

  @property
  def fmean(self):
    return self.fdim if self.mean in ('linear', 'linear_mlp') else 0

  @property
  def n_ls(self):
    return 0 if self.kname == 'dot_product' else (1 if self.scalar_ls else self.fdim)

  @property
  def out_stride(self):
    return self.n_ls + 6 + self.fmean

  @property
  def prereduced(self):
    nb = max(nblk(n) for n in self.ns)
    return nb * (nb + 1) >= 1024


def nblk(n):
  return (n + TILE - 1) // TILE


A_NS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 300)
B_FDIMS = (1, 15, 16, 17, 29, 30, 33, 64, 256)
D_NS = (300, 1, 129, 128, 513, 64)
E_NVEC, E_NS = (1, 2, 3, 9), (100, 129, 300)
F_NS = (255, 256, 257, 1023, 1025, 1300)
G_N = 3969
SE, M32, M52, DOT = KERNELS


def _both(**kw):
  return [Case(dtype=dt, **kw) for dt in DTYPES]


GROUP_A = [c for n in A_NS for c in _both(group='A', kname=SE, ns=(n,))]
GROUP_B = [c for f in B_FDIMS for sc in (False, True) for c in _both(group='B', kname=M52 if sc else SE, ns=(130,), fdim=f, scalar_ls=sc)]
GROUP_C = [c for k in KERNELS for c in _both(group='C', kname=k, ns=(200,), fdim=5)]
GROUP_D = [c for ns in (D_NS, D_NS[::-1]) for c in _both(group='D', kname=SE, ns=ns)]
GROUP_E = ([c for ob in ('ekl', 'euc') for v in E_NVEC for n in E_NS for c in _both(group='E', kname=SE, ns=(n,), obj=ob, nvec=v)] +
           [c for n, v in ((129, 2), (300, 3)) for c in _both(group='E', kname=M52, ns=(n,), fdim=4, obj='euc', nvec=v, mlp=True)])
GROUP_F = [c for mn, mlp in (('constant', False), ('linear', False), ('linear_mlp', True)) for n in F_NS
           for c in _both(group='F', kname=SE, ns=(n,), mean=mn, mlp=mlp)]
# (at 30 features the second column strip holds the Frobenius slot alone, which only EUC reads: the batch runs under EUC as well, and
#  group B has its two widths at the strip edge under EUC)
GROUP_B += [c for f in (29, 30) for c in _both(group='B', kname=SE, ns=(130,), fdim=f, obj='euc')]
GROUP_G = ([c for ns, f in (((G_N,), 3), ((G_N, 200), 30)) for c in _both(group='G', kname=SE, ns=ns, fdim=f)] +
           [c for c in _both(group='G', kname=SE, ns=(G_N, 200), fdim=30, obj='euc')])
GROUP_H = ([c for n in (1, 65, 129, 257) for c in _both(group='H', kname=SE, ns=(n,), mlp=True)] +
           [c for f in (16, 17, 64) for c in _both(group='H', kname=M32, ns=(130,), fdim=f, mlp=True)] +
           [c for c in _both(group='H', kname=M52, ns=D_NS, mlp=True)] +
           [c for c in _both(group='H', kname=DOT, ns=(200,), fdim=5, mlp=True)])
GROUP_N = [Case(group='N', kname=k, dtype='fp64', ns=(150,)) for k in (SE, M52, DOT)]
CASES = GROUP_A + GROUP_B + GROUP_C + GROUP_D + GROUP_E + GROUP_F + GROUP_G + GROUP_H + GROUP_N
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
SHARE_GROUPS = ('A', 'D', 'E', 'G')


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _f32(a):
  return np.asarray(a, dtype=np.float32).astype(np.float64)


def _unit_counts(n):
  return np.array([min(GTR, n - GTR * u) for u in range((n + GTR - 1) // GTR)], dtype=np.float64)


class Inputs(NamedTuple):
  model: dict            # ls [fdim or 1] (None: dot product), sv, noise, sigma, bias, lin_w [fmean], all fp32-representable doubles
  x: list                # per task [n, fdim] float64 holding fp32-representable numbers
  s: list                # per task [n, n] or None (EUC)
  vecs: list             # per task [nvec, n]
  lh: np.ndarray         # [T]
  c: np.ndarray          # [T]
  dmu: list              # per task [n] float64 (any double), or None


def _anchor_inputs(case):
  """G of a real NLL: K^-1 and alpha = K^-1 (sum_a y_a - m mu) in fp64 on the host, coef_lh = m^2 / 2 and coef_c = 1 / 2 as fill_desc sets
  them.  Zero mean; m = 2 target columns."""
  n, m = case.ns[0], 2
  rng = np.random.default_rng([78, n, KERNEL_ID[case.kname]])
  x = rng.uniform(size=(n, case.fdim))
  y = rng.normal(size=(n, m))
  model = {'ls': None if case.kname == DOT else np.array([0.4, 0.7, 1.1]), 'sv': 0.9, 'noise': 0.2, 'sigma': 1.3, 'bias': 0.3, 'lin_w': np.zeros(0)}
  kmat = np.asarray(_oracle_k(case.kname, model, x.astype(LD), x.astype(LD)), dtype=np.float64) + np.eye(n) * (model['noise'] + 1e-6)
  kinv = np.linalg.inv(kmat)
  kinv = 0.5 * (kinv + kinv.T)
  alpha = kinv @ y.sum(axis=1)
  return Inputs(model, [x], [kinv], [alpha[None, :]], np.array([0.5 * m * m]), np.array([0.5]), None), y


@functools.lru_cache(maxsize=None)
def _inputs(key):
  case = key
  if case.group == 'N':
    return _anchor_inputs(case)[0]
  rng = np.random.default_rng([ord(case.group), case.fdim, case.nvec, OBJ_ID[case.obj], KERNEL_ID[case.kname], int(case.scalar_ls), len(case.ns), max(case.ns)])
  f = case.fdim
  if case.kname == DOT:
    ls = None
  elif case.scalar_ls:
    ls = _f32([0.5 * math.sqrt(f)])
  else:
    ls = _f32(0.5 * math.sqrt(f) * rng.permutation(np.geomspace(0.5, 2.5, f)) if f > 1 else [0.6])
  model = {'ls': ls, 'sv': float(_f32(SV)), 'noise': float(_f32(NOISE)), 'sigma': float(_f32(0.5 * math.sqrt(f))), 'bias': float(_f32(DOT_BIAS)),
           'lin_w': _f32(rng.normal(size=case.fmean))}
  xs, ss, vs, dm = [], [], [], []
  # every task's data depends on its size alone, so that a batch in another order holds the same tasks
  for n in case.ns:
    r = np.random.default_rng([ord(case.group), f, case.nvec, n])
    x = _f32(r.uniform(size=(n, f)))
    if case.group == 'C' and n > 150:
      x[128], x[150] = x[127], x[5]                     # exact duplicates across the 128-row edge: u = 0 off the diagonal
    cnt = _unit_counts(n)
    w = (GTR / cnt)[np.arange(n) // GTR]                # 64-row units with few rows weigh more: every half tile carries its share
    a = r.uniform(-0.5, 1.5, size=(n, n))
    a = np.tril(a) + np.tril(a, -1).T
    ww = np.outer(w, w)
    a[np.arange(n), np.arange(n)] = r.uniform(0.75, 1.5, size=n)   # (a one-point tile is its diagonal entry: never near 0)
    s = None if case.obj == 'euc' else _f32(a * ww)
    # EUC has no s: the vectors alone give the small tiles their share of G = K1 - sum_b v_b v_b^T, whose Frobenius slot is quadratic in them
    v = _f32(0.3 / math.sqrt(case.nvec) * r.uniform(0.75, 1.25, size=(case.nvec, n)) * r.choice([-1.0, 1.0], size=(case.nvec, n)) *
             w[None, :] ** ((0.9 if n <= 1024 else 1.0) if case.obj == 'euc' else 0.5))
    xs.append(x); ss.append(s); vs.append(v)
    dm.append(r.normal(size=n) if case.mean != 'zero' else None)
  T = len(case.ns)
  if case.obj == 'nll':
    lh = np.array([(0.5, 2.0, 4.5)[n % 3] for n in case.ns]); c = np.full(T, 0.5)
  elif case.obj == 'ekl':
    lh = np.ones(T); c = np.ones(T)
  else:
    lh = np.zeros(T); c = np.zeros(T)
  return Inputs(model, xs, ss, vs, lh, c, dm if dm[0] is not None else None)


def inputs(case):
  return _inputs(case.data_key)


# ---- the covariances -----------------------------------------------------------------------------------------------------------------
def inv_ls64(case, model):
  """model_dev_fill: the fp64 quotient 1 / lengthscale, broadcast; ones for the dot product."""
  if model['ls'] is None:
    return np.ones(case.fdim)
  return np.broadcast_to(1.0 / np.asarray(model['ls'], dtype=np.float64), (case.fdim,)).copy()


def _oracle_k(kname, model, a, b):
  """k(a, b) through the oracle's kernel function, in the dtype of a."""
  dt = a.dtype.type
  if kname == DOT:
    p = o.GPParams(model={'dot_prod_sigma': dt(model['sigma']), 'dot_prod_bias': dt(model['bias'])})
  else:
    p = o.GPParams(model={'lengthscale': np.asarray(model['ls'], dtype=dt), 'signal_variance': dt(model['sv'])})
  return o._pair_kernel_matrix(kname, p, a, b, None)   # pylint: disable=protected-access


def _dk_du(kname, u, k, sv):
  """d k / d u of the stationary covariances, 0 at u = 0 for the Matern ones (kernfun.h: dk_du), in the dtype of u."""
  dt = u.dtype.type
  if kname == SE:
    return dt(-0.5) * k
  if kname == M32:
    r = np.sqrt(dt(3) * u)
    return np.where(u == 0, dt(0), -dt(sv) * dt(1.5) * np.exp(-r))
  r = np.sqrt(dt(5) * u)
  return np.where(u == 0, dt(0), -dt(sv) * (dt(5) / dt(6)) * np.exp(-r) * (dt(1) + r))


def _kfun(kname, u, model, dt):
  """kernfun.h: kfun in T."""
  sv = dt(model['sv'])
  if kname == SE:
    return sv * np.exp(dt(-0.5) * u)
  if kname == M32:
    r = np.sqrt(dt(3) * u)
    return sv * (dt(1) + r) * np.exp(-r)
  if kname == M52:
    r = np.sqrt(dt(5) * u)
    return sv * (dt(1) + r + r * r / dt(3)) * np.exp(-r)
  return u * dt(1.0 / (model['sigma'] * model['sigma'])) + dt(model['bias'] * model['bias'])


def half_tiles(n):
  """(slot, ti, h, tj, rows, cols) of the non-empty half tiles of a task, in slot order."""
  out = []
  for ti in range(nblk(n)):
    for tj in range(ti + 1):
      for h in (0, 1):
        r0 = TILE * ti + GTR * h
        if r0 < n:
          out.append(((ti * (ti + 1) // 2 + tj) * 2 + h, ti, h, tj, (r0, min(r0 + GTR, n)), (TILE * tj, min(TILE * tj + TILE, n))))
  return out


def _thread_sum(prod, dt):
  """[64, 128, F] products in T -> [F] : each thread's 4 x 8 (rows ty + 16 a, columns pt_col(tx, q)) summed in T in the kernel's order,
  the 256 threads in fp64."""
  vec = 16 // np.dtype(dt).itemsize
  fdim = prod.shape[2]
  p = prod.reshape(4, 16, 8 // vec, 16, vec, fdim).transpose(1, 3, 0, 2, 4, 5).reshape(256, 32, fdim)
  return np.cumsum(p, axis=1, dtype=dt)[:, -1, :].astype(np.float64).sum(axis=0)


# ---- one task: slots, dF -------------------------------------------------------------------------------------------------------------
def _task_pass(case, model, x, s, vecs, lh, c, dt, mutant=None, want_abs=False, want_df=False):
  """The half-tile slots [nblk (nblk + 1), nacc] of one task (empty half tiles: zeros) and, for an MLP kernel, the un-rescaled dF [n, fdim].
  dt = LD: the reference -- everything in longdouble, k from the oracle, with the slots' and dF's un-cancelled scales; dt = float32 /
  float64: the kernels' arithmetic in their order."""
  exact = dt is LD
  acc_t = LD if exact else np.float64
  n, f, kname, nacc = x.shape[0], case.fdim, case.kname, case.nacc
  dot, euc, multi = kname == DOT, case.obj == 'euc', case.obj != 'nll'
  inv = inv_ls64(case, model)
  sc = inv.astype(LD) if exact else inv.astype(dt)          # stage_x: (T) inv_ls[d]
  fs = x.astype(dt) if dot else x.astype(dt) * sc[None, :]    # (the dot product stages its features unscaled)
  fuse = f if mutant != 'last_chunk_cut' else DC * ((f - 1) // DC)
  n_eff = n - 1 if mutant == 'mask_off_by_one' else n
  nslots = nblk(n) * (nblk(n) + 1)
  part = np.zeros((nslots, nacc), dtype=acc_t)
  pabs = np.zeros((nslots, nacc), dtype=acc_t) if want_abs else None
  dF = np.zeros((n, f), dtype=acc_t) if want_df else None
  dFabs = np.zeros((n, f), dtype=acc_t) if want_df and want_abs else None
  V = vecs.astype(dt)
  S = None if euc else s.astype(dt)
  lh_t, c_t, noise_t, sv = dt(lh), dt(c), dt(model['noise']), model['sv']
  cd = (2.0 / (model['sigma'] * model['sigma']) * np.ones(f) if dot else 4.0 * inv).astype(acc_t)   # grad_feat_kernel: cd in fp64
  ls_model = dict(model, ls=(LD(1) / inv.astype(LD)) if exact and not dot else model['ls'])
  for slot, ti, h, tj, (r0, r1), (c0, c1) in half_tiles(n):
    a, b = fs[r0:r1, :fuse], fs[c0:c1, :fuse]
    if dot:
      u = np.cumsum(a[:, None, :] * b[None, :, :], axis=2, dtype=dt)[:, :, -1] if fuse else np.zeros((r1 - r0, c1 - c0), dtype=dt)
      df = None
    else:
      df = a[:, None, :] - b[None, :, :]
      u = np.cumsum(df * df, axis=2, dtype=dt)[:, :, -1] if fuse else np.zeros((r1 - r0, c1 - c0), dtype=dt)
    if exact and fuse == f:
      k = _oracle_k(kname, ls_model, x[r0:r1].astype(LD), x[c0:c1].astype(LD))
    else:
      k = _kfun(kname, u, model, dt)
    outer = np.zeros_like(u)
    for vb in V:
      outer = outer + vb[r0:r1, None] * vb[None, c0:c1]
    rows, cols = np.arange(r0, r1)[:, None], np.arange(c0, c1)[None, :]
    eye = rows == cols
    g0 = (k + np.where(eye, noise_t, dt(0)) - outer) if euc else (lh_t * S[r0:r1, c0:c1] - c_t * outer)
    mask = (rows < n_eff) & (cols < n_eff)
    if mutant == 'diag_upper_skipped' and ti == tj:
      mask = mask & (cols <= rows)
    g0 = np.where(mask, g0, dt(0))
    wt = dt(1) if (ti == tj or mutant == 'weight1') else dt(2)
    g = g0 * wt
    gk = g * (u if dot else k)
    terms = [gk, np.where(eye, g, dt(0))]
    if dot:
      terms.append(np.zeros_like(g) if mutant == 'a_g_omitted' else g)
    fro = (g0 * (g0 if mutant == 'fro_g0g0' else g)) if multi else np.zeros_like(g)
    for q, t in enumerate(terms):
      part[slot, q] = t.astype(acc_t).sum()
      if want_abs:
        pabs[slot, q] = np.abs(t).astype(acc_t).sum()
    part[slot, nacc - 1] = fro.astype(acc_t).sum()
    if want_abs:
      pabs[slot, nacc - 1] = np.abs(fro).astype(acc_t).sum()
    if not dot:
      gw = g * _dk_du(kname, u, k, sv)
      prod = (gw[:, :, None] * df) * df
      if exact:
        part[slot, 2:2 + fuse] = prod.sum(axis=(0, 1))
      else:
        full = np.zeros((GTR, TILE, fuse), dtype=dt)
        full[:r1 - r0, :c1 - c0] = prod
        part[slot, 2:2 + fuse] = _thread_sum(full, dt)
      if want_abs:
        pabs[slot, 2:2 + fuse] = np.abs(prod).sum(axis=(0, 1))
    if want_df:
      # grad_feat_kernel: g = G0 dk/du without the weight; rows of every tile, columns of the tiles off the diagonal
      if dot:
        wr = g0[:, :, None] * b[None, :, :]
        wc = g0[:, :, None] * a[:, None, :]
      else:
        wr = (g0 * _dk_du(kname, u, k, sv))[:, :, None] * df
        wc = -wr
      dF[r0:r1, :fuse] += cd[:fuse] * wr.astype(acc_t).sum(axis=1)
      if ti != tj:
        dF[c0:c1, :fuse] += cd[:fuse] * wc.astype(acc_t).sum(axis=0)
      if want_abs:
        dFabs[r0:r1, :fuse] += np.abs(cd[:fuse]) * np.abs(wr).astype(acc_t).sum(axis=1)
        if ti != tj:
          dFabs[c0:c1, :fuse] += np.abs(cd[:fuse]) * np.abs(wc).astype(acc_t).sum(axis=0)
  return part, pabs, dF, dFabs


# ---- column sums and chain rule (grad_prereduce_kernel, grad_finalize_kernel) ---------------------------------------------------------
def _column_sums(case, parts, k, mutant):
  """s_tot [nacc] of task k from the batch's slot arrays, in fp64 (or longdouble) as the two kernels sum them."""
  part = parts[k]
  ntile = part.shape[0]
  if mutant == 'neighbour_slot':
    nb = parts[(k + 1) % len(parts)]
    part = np.zeros_like(part)
    m = min(ntile, nb.shape[0])
    part[:m] = nb[:m]
  if mutant == 'drop_half_tile' and k == 0:
    part = part.copy()
    part[half_tiles(case.ns[0])[-1][0]] = 0
  if case.prereduced:
    pre = np.zeros((PRE_ROWS, part.shape[1]), dtype=part.dtype)
    for r in range(PRE_ROWS):
      pre[r] = part[r::PRE_ROWS].sum(axis=0)
    if mutant == 'prereduce_row_skipped':
      pre[5] = 0
    part = pre
  tot = part.sum(axis=0)
  if mutant == 'second_strip_dropped':
    tot[QW:2 * QW] = 0
  return tot


def _leaves(case, model, tot, x, dmu, dt_acc):
  """grad_finalize_kernel: the task's gradient block [out_stride] from the column sums, and |C0 - K1|_F (EUC, else 0)."""
  out = np.zeros(case.out_stride, dtype=dt_acc)
  nacc, n_ls, f = case.nacc, case.n_ls, case.fdim
  inv = inv_ls64(case, model).astype(dt_acc)
  fro = np.sqrt(tot[nacc - 1]) if case.obj == 'euc' else dt_acc(0)
  scale = (dt_acc(1) / fro if fro > 0 else dt_acc(0)) if case.obj == 'euc' else dt_acc(1)
  st = tot * scale
  if case.kname != DOT:
    out[n_ls] = st[0] / dt_acc(model['sv'])
    out[n_ls + 1] = st[1]
    gd = st[2:2 + f] * (dt_acc(-2) * inv)
    if n_ls == 1:
      out[0] = gd.sum()
    else:
      out[:f] = gd
  else:
    sg = dt_acc(model['sigma'])
    out[n_ls + 3] = st[0] * (dt_acc(-2) / (sg * sg * sg))
    out[n_ls + 1] = st[1]
    out[n_ls + 4] = st[2] * dt_acc(2) * dt_acc(model['bias'])
  d = np.zeros(x.shape[0], dtype=dt_acc) if dmu is None else dmu.astype(dt_acc)
  if case.mean == 'constant':
    out[n_ls + 2] = d.sum()
  if case.fmean:
    out[n_ls + 5:n_ls + 5 + f] = d @ x.astype(dt_acc)
    out[n_ls + 5 + f] = d.sum()
  return out, fro


class Result(NamedTuple):
  grad: np.ndarray        # [T, out_stride]
  tots: list              # per task [nacc] column sums
  parts: list             # per task [nslots, nacc]
  fro: np.ndarray         # [T]
  dF: list                # per task [n, fdim] or None (rescaled for EUC)
  tots_abs: list = None   # reference only: the un-cancelled scales
  parts_abs: list = None
  dF_abs: list = None
  mean_abs: np.ndarray = None   # [T, out_stride]: sum |dmu_i fm_id| of the mean leaves


def _run(case, dt, mutant=None):
  inp = inputs(case)
  exact = dt is LD
  acc_t = LD if exact else np.float64
  T = len(case.ns)
  res = [_task_pass(case, inp.model, inp.x[k], None if inp.s[k] is None else inp.s[k], inp.vecs[k], inp.lh[k], inp.c[k], dt, mutant, exact, case.mlp)
         for k in range(T)]
  parts = [r[0] for r in res]
  tots = [_column_sums(case, parts, k, mutant) for k in range(T)]
  grad = np.zeros((T, case.out_stride), dtype=acc_t)
  fro = np.zeros(T, dtype=acc_t)
  dFs = []
  for k in range(T):
    grad[k], fro[k] = _leaves(case, inp.model, tots[k], inp.x[k], None if inp.dmu is None else inp.dmu[k], acc_t)
    d = res[k][2]
    if d is not None and case.obj == 'euc':
      d = d * (acc_t(1) / fro[k] if fro[k] > 0 else acc_t(0))
    dFs.append(d)
  if not exact:
    return Result(grad, tots, parts, fro, dFs)
  mabs = np.zeros((T, case.out_stride), dtype=LD)
  for k in range(T):
    if inp.dmu is not None:
      d = np.abs(inp.dmu[k]).astype(LD)
      if case.mean == 'constant':
        mabs[k, case.n_ls + 2] = d.sum()
      if case.fmean:
        mabs[k, case.n_ls + 5:case.n_ls + 5 + case.fdim] = d @ np.abs(inp.x[k]).astype(LD)
        mabs[k, case.n_ls + 5 + case.fdim] = d.sum()
  return Result(grad, tots, parts, fro, dFs, [r[1].sum(axis=0) for r in res], [r[1] for r in res], [r[3] for r in res], mabs)


@functools.lru_cache(maxsize=None)
def _reference(key):
  return _run(key, LD)


def reference(case):
  return _reference(case.data_key._replace(dtype='fp64'))


@functools.lru_cache(maxsize=None)
def _restate(key):
  return _run(key, key.np_dtype)


def restate(case, mutant=None):
  return _restate(case) if mutant is None else _run(case, case.np_dtype, mutant)


def applies(mutant, case):
  nb = max(nblk(n) for n in case.ns)
  if mutant in ('drop_half_tile',):
    return True
  if mutant == 'weight1':
    return nblk(case.ns[0]) >= 2
  if mutant == 'diag_upper_skipped':
    return case.ns[0] >= 2
  if mutant == 'mask_off_by_one':
    return True
  if mutant == 'last_chunk_cut':
    return case.fdim > DC and case.kname != DOT
  if mutant == 'second_strip_dropped':              # (a slot that is read lies in the second strip)
    return case.nacc > QW + 1 or (case.nacc > QW and case.obj == 'euc')
  if mutant == 'prereduce_row_skipped':
    return nb * (nb + 1) >= 1024
  if mutant == 'neighbour_slot':
    return len(case.ns) > 1
  if mutant == 'fro_g0g0':
    return case.obj == 'euc' and nb >= 2
  if mutant == 'a_g_omitted':
    return case.kname == DOT
  raise ValueError(mutant)


# a mutant that cannot reach MUTANT_FACTOR bounds on an fp32 case: (mutant, case id) -> why.  At most 10 % of the (mutant, case) pairs,
# none from groups A or G (tests/test_grad_contract_cases_host.py).
WEAK = {}


# ---- bound and judge -------------------------------------------------------------------------------------------------------------------
def eps_of(case):
  return float(np.finfo(case.np_dtype).eps) / 2


EPS64 = float(np.finfo(np.float64).eps) / 2


def slot_bounds(case, c1=C1, c2=C2):
  """per task [nacc]: C1 |restatement - reference| + C2 eps_T S_slot."""
  ref, rs = reference(case), restate(case)
  return [c1 * np.abs(rs.tots[k].astype(LD) - ref.tots[k]) + c2 * eps_of(case) * ref.tots_abs[k] for k in range(len(case.ns))]


def leaf_bounds(case, c1=C1, c2=C2):
  """[T, out_stride] bounds of the leaves and [T] of |C0 - K1|_F, from the slot bounds through the chain-rule factors."""
  ref, inp = reference(case), inputs(case)
  sb = slot_bounds(case, c1, c2)
  T, nacc, n_ls, f = len(case.ns), case.nacc, case.n_ls, case.fdim
  out = np.zeros((T, case.out_stride), dtype=LD)
  fb = np.zeros(T, dtype=LD)
  inv = inv_ls64(case, inp.model).astype(LD)
  rs = restate(case)
  for k in range(T):
    b, tot = sb[k].copy(), ref.tots[k]
    if case.obj == 'euc':
      fr = ref.fro[k]
      fb[k] = b[nacc - 1] / (2 * fr)
      b = b / fr + np.abs(tot) * fb[k] / (fr * fr)
    if case.kname != DOT:
      out[k, n_ls] = b[0] / LD(inp.model['sv'])
      out[k, n_ls + 1] = b[1]
      gd = b[2:2 + f] * 2 * inv
      if n_ls == 1:
        out[k, 0] = gd.sum()
      else:
        out[k, :f] = gd
    else:
      out[k, n_ls + 3] = b[0] * 2 / LD(inp.model['sigma']) ** 3
      out[k, n_ls + 1] = b[1]
      out[k, n_ls + 4] = b[2] * 2 * LD(inp.model['bias'])
    mean = ref.mean_abs[k] > 0
    out[k, mean] = c1 * np.abs(rs.grad[k, mean].astype(LD) - ref.grad[k, mean]) + c2 * EPS64 * ref.mean_abs[k, mean]
  return out, fb


def df_bounds(case, c1=C1, c2=C2):
  ref, rs = reference(case), restate(case)
  out = []
  for k, n in enumerate(case.ns):
    sabs = ref.dF_abs[k] * ((1 / ref.fro[k]) if case.obj == 'euc' else 1)
    b = c1 * np.abs(rs.dF[k].astype(LD) - ref.dF[k]) + (c2 * eps_of(case) + REORDER_ADDS * nblk(n) * EPS64) * sabs
    if case.obj == 'euc':
      b = b + np.abs(ref.dF[k]) * leaf_bounds(case, c1, c2)[1][k] / ref.fro[k]
    out.append(b)
  return out


def _ratio(got, want, bound):
  got, want, bound = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD), np.asarray(bound, dtype=LD)
  err = np.abs(got - want)
  err = np.where(np.isfinite(err), err, np.inf)
  with np.errstate(divide='ignore', invalid='ignore'):
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0, np.inf))
  return np.asarray(r, dtype=np.float64)


def leaf_ratios(case, grad, fro=None, c1=C1, c2=C2):
  """[T, out_stride] error / bound of a gradient block (a leaf with bound 0 is a structural zero: it must be 0 exactly); with fro, [T] too."""
  ref = reference(case)
  lb, fb = leaf_bounds(case, c1, c2)
  r = _ratio(grad, ref.grad, lb)
  return (r, _ratio(fro, ref.fro, fb)) if fro is not None else r


def worst_half_tile(case, k, parts_k):
  """(ratio, (ti, h, tj), slot column) of the half-tile slot of task k that lies farthest from the reference, for a failure message."""
  ref, rs = reference(case), restate(case)
  b = C1 * np.abs(rs.parts[k].astype(LD) - ref.parts[k]) + C2 * eps_of(case) * ref.parts_abs[k]
  r = _ratio(parts_k, ref.parts[k], b)
  tiles = {t[0]: t[1:4] for t in half_tiles(case.ns[k])}
  r = np.where(np.isin(np.arange(r.shape[0]), list(tiles))[:, None], r, 0)     # (the slots of empty half tiles are never written nor read)
  i, q = np.unravel_index(np.argmax(r), r.shape)
  return float(r[i, q]), tiles.get(int(i)), int(q)


def judge(case, grad, parts=None, fro=None, dF=None):
  """Every assertion on what the device (or a restatement) returned for a case; the largest error / bound."""
  r = leaf_ratios(case, grad, fro if case.obj == 'euc' else None)
  worst = float(np.max(r[0])) if isinstance(r, tuple) else float(np.max(r))
  if isinstance(r, tuple):
    worst = max(worst, float(np.max(r[1])))
    r = r[0]
  assert np.all(np.isfinite(np.asarray(grad, dtype=np.float64))), f'{case.id}: a non-finite leaf (the sentinel?)'
  if case.mlp and dF is not None:
    ref = reference(case)
    for k, b in enumerate(df_bounds(case)):
      assert np.all(np.isfinite(dF[k])), f'{case.id}: non-finite dF in task {k}'
      worst = max(worst, float(np.max(_ratio(dF[k], ref.dF[k], b))))
  if worst > 1.0 and parts is not None:
    k = int(np.argmax(np.max(r, axis=1)))
    raise AssertionError(f'{case.id}: error / bound = {worst:.3g}; task {k} leaf {int(np.argmax(r[k]))}; worst half tile (ti, h, tj), slot: {worst_half_tile(case, k, parts[k])}')
  return worst


# ---- the anchor ------------------------------------------------------------------------------------------------------------------------
def anchor_oracle_leaves(case):
  """The kernel leaves of oracle.nll_sub_dataset_value_and_grad on the anchor's data, in the layout of the gradient block."""
  inp, y = _anchor_inputs(case)
  m = inp.model
  model = {'noise_variance': np.array(m['noise']), 'signal_variance': np.array(m['sv']), 'dot_prod_sigma': np.array(m['sigma']),
           'dot_prod_bias': np.array(m['bias'])}
  if m['ls'] is not None:
    model['lengthscale'] = np.asarray(m['ls'])
  names = {SE: 'squared_exponential', M32: 'matern32', M52: 'matern52', DOT: 'dot_product'}
  _, g = o.nll_sub_dataset_value_and_grad(o.zero, getattr(o, names[case.kname]), o.GPParams(model=model), inp.x[0], y, None)
  out = np.zeros(case.out_stride)
  n_ls = case.n_ls
  out[n_ls + 1] = g['noise_variance']
  if case.kname == DOT:
    out[n_ls + 3], out[n_ls + 4] = g['dot_prod_sigma'], g['dot_prod_bias']
  else:
    out[:n_ls] = g['lengthscale']
    out[n_ls] = g['signal_variance']
  return out


def leaf_scales(case):
  """[T, out_stride]: the un-cancelled scale S of every kernel leaf (the bound with C1 = 0, C2 eps = 1)."""
  ref, inp = reference(case), inputs(case)
  T, n_ls, f = len(case.ns), case.n_ls, case.fdim
  out = np.zeros((T, case.out_stride), dtype=LD)
  inv = inv_ls64(case, inp.model).astype(LD)
  for k in range(T):
    b = ref.tots_abs[k]
    if case.kname != DOT:
      out[k, n_ls], out[k, n_ls + 1] = b[0] / LD(inp.model['sv']), b[1]
      gd = b[2:2 + f] * 2 * inv
      out[k, :n_ls] = gd.sum() if n_ls == 1 else gd
    else:
      out[k, n_ls + 3], out[k, n_ls + 1], out[k, n_ls + 4] = b[0] * 2 / LD(inp.model['sigma']) ** 3, b[1], b[2] * 2 * LD(inp.model['bias'])
  return out
