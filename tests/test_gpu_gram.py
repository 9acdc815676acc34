"""The Gram on the device, PER ENTRY, against tests/gram_cases.py (reference in longdouble, bound from the kernel's own arithmetic, the
table and what it reaches: see there).  Groups A-C and F go through hbo_gram, the padded cross form (D) and the batched task form (E)
through the test hook hbo_probe_gram (include/hbo_tune.h), which returns the whole padded buffers preset to a sentinel.  fp32 on the VALU
kernel beyond 31 features runs on a context of its own (gram_mfma = 0); the default context is never changed.  Run with `-m gpu`.
With HBO_GRAD_LOG=<file> every case appends its largest error / bound, and the module the largest per group, dtype, kernel and engine.
"""
import ctypes as C
import os

import numpy as np
import pytest

import gram_cases as gc

pytestmark = pytest.mark.gpu
_WORST = {}


def _nat():
  from hyperbo_amd import _native as nat
  return nat


@pytest.fixture(scope='module')
def direct_ctx(gpu_ctx):
  """A second context whose fp32 Gram matrices always take the VALU kernel."""
  ctx = _nat().Context(gpu_ctx.device)
  ctx.set_option('poison', 1)
  ctx.set_option('gram_mfma', 0)
  yield ctx
  ctx.close()


@pytest.fixture(scope='module', autouse=True)
def _summary():
  _WORST.clear()
  yield
  log = os.environ.get('HBO_GRAD_LOG')
  if log:
    with open(log, 'a') as f:
      for (group, dtype, kname, engine), (ratio, cid) in sorted(_WORST.items()):
        f.write(f'{ratio:.3e} tol=gram-per-entry group={group} {dtype} {kname} {engine} worst case {cid}\n')


def _record(case, ratio):
  key = (case.group, case.dtype, case.kname, case.engine)
  if ratio >= _WORST.get(key, (-1.0, ''))[0]:
    _WORST[key] = (ratio, case.id)
  log = os.environ.get('HBO_GRAD_LOG')
  if log:
    with open(log, 'a') as f:
      f.write(f'{ratio:.3e} tol=gram-per-entry {case.id} {os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]}\n')
  assert ratio <= 1.0


def _models(case):
  """hbo_model[] of the case's parameters as they stand (no warp), and the arrays they point into."""
  nat = _nat()
  ms = gc.inputs(case)[1]
  arr = (nat.Model * len(ms))()
  keep = []
  for m, p in zip(arr, ms):
    m.kernel_id, m.mean_id, m.dtype, m.input_dim = gc.KERNEL_ID[case.kname], nat.MEAN_ZERO, nat.dtype_code(case.np_dtype), case.fdim
    m.eps, m.noise_variance = p['jitter'], p['noise']
    if case.kname == 'dot_product':
      m.dot_prod_sigma, m.dot_prod_bias = p['sigma'], p['bias']
    else:
      ls = np.ascontiguousarray(p['ls'], dtype=case.np_dtype)
      keep.append(ls)
      m.lengthscale, m.n_lengthscale, m.signal_variance = nat.ptr(ls).value, ls.size, p['sv']
  return arr, keep


def _gram(ctx, case):
  nat = _nat()
  (x1, x2), _ = gc.inputs(case)
  models, keep = _models(case)
  diag = case.group == 'F'
  n1 = x1.shape[0]
  n2 = n1 if x2 is None else x2.shape[0]
  out = np.full((n1,) if diag else (n1, n2), np.nan, dtype=case.np_dtype)
  ctx.check(nat.lib().hbo_gram(ctx.handle, C.byref(models[0]), nat.ptr(x1), n1, nat.ptr(x2), n2, int(diag), nat.ptr(out)), allow_not_pd=False)
  del keep
  return out


def _probe(ctx, case):
  """hbo_probe_gram for a case of group D (form 1) or E (form 2): what gram_cases.judge takes."""
  nat = _nat()
  xs, _ = gc.inputs(case)
  models, keep = _models(case)
  T = case.np_dtype
  if case.group == 'D':
    form, x, ns, x2, n2 = 1, xs[0], [case.n1], xs[1], case.n2
    cap = (case.n1 + 2 * gc.TILE) * (case.n2 + 3 * gc.TILE)
  else:
    form, x, ns, x2, n2 = 2, np.ascontiguousarray(np.concatenate(xs)), list(case.tasks), None, 0
    cap = sum((n + 2 * gc.TILE) ** 2 for n in ns)
  nt = len(ns)
  ns_c = (C.c_int64 * nt)(*ns)
  rows, ld = (C.c_int64 * nt)(), (C.c_int64 * nt)()
  out = np.full(cap, np.nan, dtype=T)
  rc = nat.lib().hbo_probe_gram(ctx.handle, form, C.cast(models, C.c_void_p), len(models), nat.ptr(x), ns_c, nt, nat.ptr(x2), n2, case.direct_form,
                                gc.SENTINEL, nat.ptr(out), cap, rows, ld)
  ctx.check(rc, allow_not_pd=False)
  del keep
  bufs, off = [], 0
  for k in range(nt):
    cnt = rows[k] * ld[k]
    bufs.append((out[off:off + cnt].reshape(rows[k], ld[k]), int(rows[k]), int(ld[k])))
    off += cnt
  return bufs[0] if form == 1 else bufs


def _ctx_of(case, gpu_ctx, direct_ctx):
  return direct_ctx if case.ctx == 'direct' else gpu_ctx


def _ids(group):
  return [c.id for c in gc.CASES if c.group == group]


@pytest.mark.parametrize('cid', _ids('A'))
def test_widths_across_the_feature_chunk(gpu_ctx, direct_ctx, cid):
  case = gc.BY_ID[cid]
  _record(case, gc.judge(case, _gram(_ctx_of(case, gpu_ctx, direct_ctx), case)))


@pytest.mark.parametrize('cid', _ids('B'))
def test_shapes_across_the_tile_edges(gpu_ctx, cid):
  case = gc.BY_ID[cid]
  _record(case, gc.judge(case, _gram(gpu_ctx, case)))


@pytest.mark.parametrize('cid', _ids('C'))
def test_tails_near_pairs_and_offsets(gpu_ctx, cid):
  case = gc.BY_ID[cid]
  _record(case, gc.judge(case, _gram(gpu_ctx, case)))


@pytest.mark.parametrize('cid', _ids('D'))
def test_padded_cross_form(gpu_ctx, cid):
  case = gc.BY_ID[cid]
  _record(case, gc.judge(case, _probe(gpu_ctx, case)))


@pytest.mark.parametrize('cid', _ids('E'))
def test_batched_task_form(gpu_ctx, cid):
  case = gc.BY_ID[cid]
  _record(case, gc.judge(case, _probe(gpu_ctx, case)))


@pytest.mark.parametrize('cid', _ids('F'))
def test_diagonal(gpu_ctx, cid):
  case = gc.BY_ID[cid]
  _record(case, gc.judge(case, _gram(gpu_ctx, case)))


def test_default_context_still_takes_the_matrix_cores(gpu_ctx, direct_ctx):
  """the two contexts take different kernels at 33 features (this module ran last: the default one was not changed by it)"""
  on =next(c for c in gc.CASES if c.group == 'A' and c.engine == 'mfma' and c.fdim == 33 and c.kname == 'matern52')
  off = next(c for c in gc.CASES if c.group == 'A' and c.ctx == 'direct' and c.dtype == 'fp32' and c.fdim == 33 and c.kname == 'matern52')
  assert not np.array_equal(_gram(gpu_ctx, on), _gram(direct_ctx, off))


# ---- the hook's argument validation -----------------------------------------------------------------------------------------------
def test_probe_gram_rejects_bad_arguments(gpu_ctx):
  nat = _nat()
  lib = nat.lib()
  case = next(c for c in gc.CASES if c.group == 'D' and (c.n1, c.n2) == (130, 129) and c.dtype == 'fp64' and c.fdim == 3 and c.kname == 'matern52')
  xs, _ = gc.inputs(case)
  models, keep = _models(case)
  ecase = next(c for c in gc.CASES if c.group == 'E' and c.per_task and c.dtype == 'fp64' and c.fdim == 3 and c.kname == 'matern52')
  emodels, ekeep = _models(ecase)
  cap = 256 * 512
  out = np.zeros(cap)
  rows, ld = (C.c_int64 * 8)(), (C.c_int64 * 8)()
  one = (C.c_int64 * 8)(130, 5, 5, 5, 5, 5, 5, 5)
  mp_, x1, x2 = C.cast(models, C.c_void_p), nat.ptr(xs[0]), nat.ptr(xs[1])

  def call(form=1, m=mp_, nm=1, x=x1, ns=one, nt=1, xq=x2, n2=129, direct=0, o=nat.ptr(out), oc=cap, r=rows, l=ld):
    return lib.hbo_probe_gram(gpu_ctx.handle, form, m, nm, x, ns, nt, xq, n2, direct, gc.SENTINEL, o, oc, r, l)

  def model_with(**kw):
    arr, _ = _models(case)
    for k, v in kw.items():
      setattr(arr[0], k, v)
    return arr

  assert call() == nat.HBO_OK and (rows[0], ld[0]) == (256, 256 + 16)
  mlp, warp, lmlp = model_with(kernel_uses_mlp=1), model_with(input_warp=nat.WARP_KUMAR), model_with(mean_id=nat.MEAN_LINEAR_MLP)
  bad = [dict(form=0), dict(form=3), dict(m=None), dict(x=None), dict(ns=None), dict(o=None), dict(r=None), dict(l=None), dict(xq=None), dict(n2=0),
         dict(nt=0), dict(nt=65), dict(nt=2), dict(nm=2), dict(direct=2), dict(direct=-1), dict(oc=0), dict(oc=256 * 272 - 1),
         dict(ns=(C.c_int64 * 1)(0)), dict(ns=(C.c_int64 * 1)(4097)), dict(n2=1 << 20),
         dict(m=C.cast(mlp, C.c_void_p)), dict(m=C.cast(warp, C.c_void_p)), dict(m=C.cast(lmlp, C.c_void_p)),
         dict(form=2), dict(form=2, xq=None, n2=0, direct=1), dict(form=2, xq=None, n2=0, nt=3, nm=2, m=C.cast(emodels, C.c_void_p)),
         dict(form=2, xq=None, n2=0, oc=128 * 144 - 1)]
  for kw in bad:
    rc = call(**kw)
    assert rc == nat.HBO_ERR_ARG, (kw, rc)
    assert b'hbo_probe_gram' in lib.hbo_last_error(gpu_ctx.handle), kw
  # the models of a batch must be one family
  mixed = (nat.Model * 2)()
  C.memmove(mixed, emodels, 2 * C.sizeof(nat.Model))
  mixed[1].kernel_id = gc.KERNEL_ID['matern32']
  assert call(form=2, xq=None, n2=0, nt=2, nm=2, m=C.cast(mixed, C.c_void_p)) == nat.HBO_ERR_ARG
  assert call() == nat.HBO_OK            # and the context still works
  del keep, ekeep
