"""The blocked gradient contraction on the device, PER TASK AND LEAF, against tests/grad_contract_cases.py (reference in longdouble, bound
from the kernels' own arithmetic, the table and what it reaches: see there), through the test hook hbo_probe_grad_contract
(include/hbo_tune.h): G is the caller's, so the bound is the contraction's and not cond(K)'s.  Every padding element the hook writes is NaN.
Run with `-m gpu`.  With HBO_GRAD_LOG=<file> every case appends its largest error / bound, and the module the largest per group, dtype and
kernel."""
import ctypes as C
import os

import numpy as np
import pytest

import grad_contract_cases as gc

pytestmark = pytest.mark.gpu
_WORST = {}
_D = C.POINTER(C.c_double)


def _nat():
  from hyperbo_amd import _native as nat
  return nat


@pytest.fixture(scope='module', autouse=True)
def _summary():
  _WORST.clear()
  yield
  log = os.environ.get('HBO_GRAD_LOG')
  if log:
    with open(log, 'a') as f:
      for (group, dtype, kname), (ratio, cid) in sorted(_WORST.items()):
        f.write(f'{ratio:.3e} tol=grad-contract-per-leaf group={group} {dtype} {kname} worst case {cid}\n')


def _record(case, ratio):
  key = (case.group, case.dtype, case.kname)
  if ratio >= _WORST.get(key, (-1.0, ''))[0]:
    _WORST[key] = (ratio, case.id)
  log = os.environ.get('HBO_GRAD_LOG')
  if log:
    with open(log, 'a') as f:
      f.write(f'{ratio:.3e} tol=grad-contract-per-leaf {case.id} {os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]}\n')
  assert ratio <= 1.0, (case.id, ratio)


def _model(case):
  """hbo_model of the case and the arrays it points into.  An MLP kernel: one layer of fdim outputs over 2 inputs, weights never read."""
  nat = _nat()
  T, p = case.np_dtype, gc.inputs(case).model
  m, keep = nat.Model(), []
  m.kernel_id, m.mean_id, m.dtype = gc.KERNEL_ID[case.kname], gc.MEAN_ID[case.mean], nat.dtype_code(T)
  m.input_dim, m.eps, m.noise_variance, m.signal_variance = case.fdim, 1e-6, p['noise'], p['sv']
  m.dot_prod_sigma, m.dot_prod_bias = p['sigma'], p['bias']
  if case.mlp:
    w, b = np.zeros((2, case.fdim), dtype=T), np.zeros(case.fdim, dtype=T)
    keep += [w, b]
    m.input_dim, m.kernel_uses_mlp, m.n_layers = 2, 1, 1
    m.features[0], m.mlp_kernel[0], m.mlp_bias[0] = case.fdim, nat.ptr(w).value, nat.ptr(b).value
  if p['ls'] is not None:
    ls = np.ascontiguousarray(p['ls'], dtype=T)
    keep.append(ls)
    m.lengthscale, m.n_lengthscale = nat.ptr(ls).value, ls.size
  if case.fmean:
    lw = np.ascontiguousarray(p['lin_w'], dtype=T)
    keep.append(lw)
    m.linear_kernel = nat.ptr(lw).value
  return m, keep


class _Out:
  pass


def _probe(ctx, case, want=('grad', 'parts', 'fro', 'dF', 'pre')):
  nat = _nat()
  inp, T = gc.inputs(case), case.np_dtype
  model, keep = _model(case)
  nt = len(case.ns)
  x = np.ascontiguousarray(np.concatenate(inp.x), dtype=T)
  s = None if case.obj == 'euc' else np.ascontiguousarray(np.concatenate([a.ravel() for a in inp.s]), dtype=T)
  v = np.ascontiguousarray(np.concatenate([a.ravel() for a in inp.vecs]), dtype=T)
  lh, cc = np.ascontiguousarray(inp.lh, dtype=np.float64), np.ascontiguousarray(inp.c, dtype=np.float64)
  dmu = None if inp.dmu is None else np.ascontiguousarray(np.concatenate(inp.dmu), dtype=np.float64)
  slots = [gc.nblk(n) * (gc.nblk(n) + 1) for n in case.ns]
  o = _Out()
  o.grad = np.full((nt, case.out_stride), 7.0) if 'grad' in want else None
  o.parts = np.full(sum(slots) * case.nacc, 7.0) if 'parts' in want else None
  o.fro = np.full(nt, 7.0) if 'fro' in want and case.obj == 'euc' else None
  o.dF = np.full((sum(case.ns), case.fdim), 7.0) if 'dF' in want and case.mlp else None
  pre = C.c_int32(-1)
  dp = lambda a: None if a is None else a.ctypes.data_as(_D)
  rc = nat.lib().hbo_probe_grad_contract(ctx.handle, C.byref(model), gc.OBJ_ID[case.obj], nt, (C.c_int64 * nt)(*case.ns), nat.ptr(x), nat.ptr(s),
                                         nat.ptr(v), case.nvec, dp(lh), dp(cc), dp(dmu), float('nan'), dp(o.grad), dp(o.parts), dp(o.fro), dp(o.dF),
                                         C.byref(pre) if 'pre' in want else None)
  ctx.check(rc, allow_not_pd=False)
  del keep
  o.pre = pre.value
  if o.parts is not None:
    off, per = np.cumsum([0] + slots) * case.nacc, []
    for k in range(nt):
      per.append(o.parts[off[k]:off[k + 1]].reshape(slots[k], case.nacc))
    o.parts_k = per
  if o.dF is not None:
    off = np.cumsum((0,) + case.ns)
    o.dF_k = [o.dF[off[k]:off[k + 1]] for k in range(nt)]
  return o


def _written(case, parts_k):
  """the slots of the non-empty half tiles of every task: what the kernels write and read"""
  return np.concatenate([parts_k[k][[t[0] for t in gc.half_tiles(n)]].ravel() for k, n in enumerate(case.ns)])


def _check(ctx, case):
  a = _probe(ctx, case)
  assert a.pre == int(case.prereduced)
  # the sentinel (NaN) never appears in an output
  assert np.all(np.isfinite(a.grad)) and np.all(np.isfinite(_written(case, a.parts_k)))
  assert a.fro is None or np.all(np.isfinite(a.fro))
  assert a.dF is None or np.all(np.isfinite(a.dF))
  ratio = gc.judge(case, a.grad, a.parts_k, a.fro, a.dF_k if case.mlp else None)
  # no atomics in the contraction and its column sums: a second call gives the same bits (dF: fp64 atomics, need not)
  b = _probe(ctx, case, want=('grad', 'parts', 'fro'))
  assert np.array_equal(a.grad, b.grad) and np.array_equal(_written(case, a.parts_k), _written(case, b.parts_k))
  assert a.fro is None or np.array_equal(a.fro, b.fro)
  _record(case, ratio)
  return a


def _ids(group):
  return [c.id for c in gc.CASES if c.group == group]


@pytest.mark.parametrize('cid', _ids('A'))
def test_row_edges_of_the_half_tile_grid(gpu_ctx, cid):
  _check(gpu_ctx, gc.BY_ID[cid])


@pytest.mark.parametrize('cid', _ids('B'))
def test_feature_chunks_and_column_strips(gpu_ctx, cid):
  _check(gpu_ctx, gc.BY_ID[cid])


@pytest.mark.parametrize('cid', _ids('C'))
def test_four_covariances_with_duplicate_rows(gpu_ctx, cid):
  _check(gpu_ctx, gc.BY_ID[cid])


@pytest.mark.parametrize('dtype', gc.DTYPES)
def test_ragged_batch_per_task_in_both_orders(gpu_ctx, dtype):
  fwd, rev = [c for c in gc.CASES if c.group == 'D' and c.dtype == dtype]
  assert fwd.ns == rev.ns[::-1]
  a, b = _check(gpu_ctx, fwd), _check(gpu_ctx, rev)
  nt = len(fwd.ns)
  for k in range(nt):                      # the same task in another place of another batch: the same bits
    used = [t[0] for t in gc.half_tiles(fwd.ns[k])]
    assert np.array_equal(a.grad[k], b.grad[nt - 1 - k]), (k, fwd.ns[k])
    assert np.array_equal(a.parts_k[k][used], b.parts_k[nt - 1 - k][used]), (k, fwd.ns[k])


@pytest.mark.parametrize('cid', _ids('E'))
def test_divergences_with_outer_product_vectors(gpu_ctx, cid):
  _check(gpu_ctx, gc.BY_ID[cid])


@pytest.mark.parametrize('cid', _ids('F'))
def test_mean_leaves_across_the_unrolled_loops(gpu_ctx, cid):
  _check(gpu_ctx, gc.BY_ID[cid])


@pytest.mark.parametrize('cid', _ids('G'))
def test_two_step_column_sum(gpu_ctx, cid):
  a = _check(gpu_ctx, gc.BY_ID[cid])
  assert a.pre == 1


@pytest.mark.parametrize('cid', _ids('H'))
def test_feature_gradient_per_row_and_feature(gpu_ctx, cid):
  _check(gpu_ctx, gc.BY_ID[cid])


@pytest.mark.parametrize('cid', _ids('N'))
def test_anchor_of_a_real_nll(gpu_ctx, cid):
  _check(gpu_ctx, gc.BY_ID[cid])


# ---- the hook's argument validation -----------------------------------------------------------------------------------------------
def test_probe_rejects_bad_arguments_and_leaves_outputs_alone(gpu_ctx):
  nat = _nat()
  lib = nat.lib()
  case = next(c for c in gc.CASES if c.group == 'E' and c.obj == 'ekl' and c.ns == (129,) and c.nvec == 2 and c.dtype == 'fp64')
  inp = gc.inputs(case)
  x, s, v = (np.ascontiguousarray(a, dtype=np.float64) for a in (inp.x[0], inp.s[0], inp.vecs[0]))
  one = np.ones(1)
  outs = {k: np.full(n, 7.0) for k, n in (('grad', case.out_stride), ('parts', 6 * case.nacc), ('fro', 1), ('dF', 129 * case.fdim))}
  pre = C.c_int32(-1)
  dp = lambda a: None if a is None else a.ctypes.data_as(_D)

  def model_with(**kw):
    m, keep = _model(case)
    for k, val in kw.items():
      setattr(m, k, val)
    return m, keep

  def call(m=None, obj=1, nt=1, ns=(129,), xx=x, ss=s, vv=v, nvec=2, lh=one, cc=one, fro=None, dF=None):
    m = m or model_with()
    return lib.hbo_probe_grad_contract(gpu_ctx.handle, C.byref(m[0]), obj, nt, None if ns is None else (C.c_int64 * len(ns))(*ns), nat.ptr(xx), nat.ptr(ss),
                                       nat.ptr(vv), nvec, dp(lh), dp(cc), None, float('nan'), dp(outs['grad']), dp(outs['parts']), dp(fro), dp(dF), C.byref(pre))

  assert call() == nat.HBO_OK and pre.value == 0 and np.all(np.isfinite(outs['grad']))
  for a in outs.values():
    a[:] = 7.0
  pre.value = -1
  lin = model_with(mean_id=nat.MEAN_LINEAR_MLP)
  bad = [dict(obj=-1), dict(obj=3), dict(nt=0), dict(nt=65), dict(ns=None), dict(ns=(0,)), dict(ns=(4097,)), dict(xx=None), dict(ss=None), dict(vv=None),
         dict(nvec=0), dict(nvec=10), dict(obj=0), dict(lh=None), dict(cc=None), dict(fro=outs['fro']), dict(dF=outs['dF']),
         dict(m=model_with(input_warp=nat.WARP_KUMAR)), dict(m=model_with(kernel_id=7)), dict(m=model_with(n_lengthscale=2)), dict(m=lin)]
  for kw in bad:
    rc = call(**kw)
    assert rc == nat.HBO_ERR_ARG, (kw.keys(), rc)
    assert b'hbo_probe_grad_contract' in lib.hbo_last_error(gpu_ctx.handle) or 'm' in kw, kw.keys()
    assert all(np.all(a == 7.0) for a in outs.values()) and pre.value == -1, kw.keys()
  assert call() == nat.HBO_OK and pre.value == 0            # and the context still works
  assert gc.judge(case, outs['grad'][None, :]) <= 1.0
