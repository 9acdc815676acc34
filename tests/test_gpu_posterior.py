"""The streamed posterior (hbo_predict / hbo_acq without full_cov; csrc/cache.hip: posterior) per query on every route.  Run with `-m gpu`.

Exact tier: hbo_probe_posterior (include/hbo_tune.h) runs posterior() itself over the integer designs of tests/posterior_cases.py, on
which every route has one right answer to the last bit: mu, var (= r_q in {0, 1, 2, 3}) and, on single-chunk calls, the per-block
partials colsq and mupart are compared with np.array_equal.  The sizes follow from the device's CU count, and every run first asserts
the route it is there for from hbo_probe_post_plan: one block; split along K with kchunk 1, 2, 3; the plain GEMM_POST grid, streamed
through two workspaces; the resident grid and the plain side of its edge -- in fp64 and, where the product is not split along K, in the
three fp32 forms (and bf16x3 by k_bound = 0 although f16x2 is on).  tests/test_posterior_cases_host.py proves on the CPU that the
designs are exact and live and that the faults named there change an asserted output.

Real-kernel tier: hbo_factor + hbo_predict against the fp64 oracle, per query and relative to the query's own terms; see
test_posterior_per_query_against_the_oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import posterior_cases as P

pytestmark = pytest.mark.gpu
TUNE_DEFAULTS = {'post_bf16x3': 1, 'post_f16x2': 1, 'lauum_persist': 1}


def _nat():
  from hyperbo_amd import _native as nat
  return nat


def _cus(ctx):
  nat = _nat()
  cus, mem = C.c_int32(0), C.c_int64(0)
  assert nat.lib().hbo_device_info(ctx.device, None, 0, C.byref(cus), C.byref(mem)) == 0 and cus.value > 0
  return cus.value


class _Options:
  """Sets the posterior's options for one run and puts back what they were."""

  def __init__(self, ctx, **values):
    self.ctx, self.values = ctx, values

  def __enter__(self):
    # (post_chunk can be read back; the three hbo_tune knobs cannot: they return to their defaults, csrc/ctx.h)
    self.old = {'post_chunk': self.ctx.get_option('post_chunk'), **TUNE_DEFAULTS}
    for k, v in self.values.items():
      assert k in self.old
      self.ctx.set_option(k, v)

  def __exit__(self, *exc):
    for k, v in self.old.items():
      self.ctx.set_option(k, v)


def _form_options(form):
  return {'post_bf16x3': int(form != 'mfma'), 'post_f16x2': int(form == 'f16x2')}


def _probe(ctx, d, dtype, k_bound, want_parts):
  """hbo_probe_posterior on design d: (mu, var, colsq, mupart, plan)."""
  nat = _nat()
  dt = np.float64 if dtype == 'fp64' else np.float32
  arrs = [np.ascontiguousarray(a, dtype=dt) for a in (d.W, d.alpha, d.Kxq, d.kdiag, d.mu0)]
  W, alpha, Kxq, kdiag, mu0 = arrs
  mu, var = np.full(d.M, np.nan, dt), np.full(d.M, np.nan, dt)
  colsq = np.full((d.nblk, d.M), np.nan, dt) if want_parts else None
  mupart = np.full((d.nblk, d.M), np.nan, dt) if want_parts else None
  plan = nat.ProbePostPlan()
  ctx.check(nat.lib().hbo_probe_posterior(ctx.handle, nat.dtype_code(dt), nat.ptr(W), d.n, nat.ptr(alpha), nat.ptr(Kxq), nat.ptr(kdiag),
                                          nat.ptr(mu0), d.M, float(k_bound), nat.ptr(mu), nat.ptr(var), nat.ptr(colsq), nat.ptr(mupart),
                                          C.addressof(plan)), allow_not_pd=False)
  return mu, var, colsq, mupart, plan.as_dict()


def _first_diff(got, ref):
  bad = np.argwhere(got.astype(np.float64) != ref)
  i = tuple(int(v) for v in bad[0])
  return f'{len(bad)} of {ref.size} differ, first at {i}: got {got[i]!r}, expected {ref[i]!r}'


def _exact_cases():
  # (collected without a device: the ids come from the MI355X's CU count, the sizes of a run from the device it runs on)
  return [(c.name, run) for c in P.route_cases(256) for run in P.runs_of(c)]


@pytest.mark.parametrize('name,run', _exact_cases(), ids=lambda v: v if isinstance(v, str) else f'{v[0]}-{v[1]}-kb{v[2]:g}')
def test_exact_posterior_on_every_route(gpu_ctx, name, run):
  dtype, form, k_bound = run
  cus = _cus(gpu_ctx)
  case = {c.name: c for c in P.route_cases(cus)}[name]
  d, ref = P.design(case.n, case.M), P.direct(case.n, case.M)
  want = P.plan(case.n, case.M, case.post_chunk, cus, dtype, form, k_bound)
  with _Options(gpu_ctx, post_chunk=case.post_chunk, lauum_persist=1, **_form_options(form)):
    mu, var, colsq, mupart, plan = _probe(gpu_ctx, d, dtype, k_bound, case.single_chunk)
  # the route first: a run that took another one proves nothing about this one
  assert plan == want, f'{case.id} {run}: ran {plan}, the case is there for {want}'
  if case.route == 'splitk':
    assert plan['kchunk'] == P.EXPECT_KCHUNK[case.name] and plan['form'] == 0
  else:
    assert plan['kchunk'] == 0 and plan['resident_chunks'] == (1 if case.route == 'resident' else 0)
  if case.name in ('one_3chunks', 'k1_3chunks'):
    assert (plan['nchunks'], plan['nbuf']) == (3, 2)
  if case.name == 'plain_streamed':
    assert plan['nchunks'] >= 2 and plan['nbuf'] == 2 and (cus != 256 or plan['nchunks'] == 4)
  label = f'{case.id} {dtype} {form} k_bound {k_bound:g} {plan}'
  print(f'exact | {cus} CUs | {label}')
  if case.single_chunk:
    assert np.array_equal(colsq, ref.colsq), f'{label}: colsq [block, query]: {_first_diff(colsq, ref.colsq)}'
    assert np.array_equal(mupart, ref.mupart), f'{label}: mupart [block, query]: {_first_diff(mupart, ref.mupart)}'
  assert np.array_equal(mu, ref.mu), f'{label}: mu [query]: {_first_diff(mu, ref.mu)}'
  assert np.array_equal(var, ref.var), f'{label}: var [query]: {_first_diff(var, ref.var)}'
  assert np.array_equal(var, d.r)


def test_plain_grid_without_the_resident_option(gpu_ctx):
  """lauum_persist = 0: the shape of the resident case on the plain grid, same bits."""
  cus = _cus(gpu_ctx)
  case = {c.name: c for c in P.route_cases(cus)}['resident']
  d, ref = P.design(case.n, case.M), P.direct(case.n, case.M)
  with _Options(gpu_ctx, post_chunk=case.post_chunk, lauum_persist=0):
    mu, var, colsq, mupart, plan = _probe(gpu_ctx, d, 'fp64', P.K_BOUND, True)
  assert plan == P.plan(case.n, case.M, case.post_chunk, cus, lauum_persist=0) and plan['resident_chunks'] == 0
  for got, want, what in ((colsq, ref.colsq, 'colsq'), (mupart, ref.mupart, 'mupart'), (mu, ref.mu, 'mu'), (var, ref.var, 'var')):
    assert np.array_equal(got, want), f'{case.id} plain: {what}: {_first_diff(got, want)}'


def test_probe_posterior_refuses_bad_arguments(gpu_ctx):
  nat = _nat()
  lib, h = nat.lib(), gpu_ctx.handle
  d = P.design(100, 300)
  W, al, K, kd, m0 = (np.ascontiguousarray(a, dtype=np.float64) for a in (d.W, d.alpha, d.Kxq, d.kdiag, d.mu0))
  mu, var = np.full(300, 7.0), np.full(300, 7.0)
  parts = np.full((1, 300), 7.0)
  plan = nat.ProbePostPlan()

  def call(ctx=h, dtype=nat.F64, w=W, n=100, alpha=al, kxq=K, kdiag=kd, mu0=m0, M=300, kb=2.0, mu_o=mu, var_o=var, cs=None, mp=None):
    return lib.hbo_probe_posterior(ctx, dtype, nat.ptr(w), n, nat.ptr(alpha), nat.ptr(kxq), nat.ptr(kdiag), nat.ptr(mu0), M, kb,
                                   nat.ptr(mu_o), nat.ptr(var_o), nat.ptr(cs), nat.ptr(mp), C.addressof(plan))
  with _Options(gpu_ctx, post_chunk=128):
    assert call(cs=parts) == nat.HBO_ERR_ARG and call(mp=parts) == nat.HBO_ERR_ARG   # three chunks
    assert b'single-chunk' in lib.hbo_last_error(h)
    assert call() == nat.HBO_OK
  assert call(cs=parts, mp=parts) == nat.HBO_OK
  mu[:], var[:] = 7.0, 7.0
  upper = W.copy(); upper[3, 50] = 1.0
  for bad in (dict(ctx=None), dict(dtype=2), dict(w=None), dict(alpha=None), dict(kxq=None), dict(kdiag=None), dict(mu0=None),
              dict(mu_o=None), dict(var_o=None), dict(n=0), dict(n=4097), dict(M=0), dict(M=(1 << 17) + 1), dict(kb=-1.0),
              dict(kb=float('nan')), dict(kb=float('inf')), dict(w=upper)):
    assert call(**bad) == nat.HBO_ERR_ARG, bad
  assert np.all(mu == 7.0) and np.all(var == 7.0)


# ---- real-kernel tier: hbo_factor + hbo_predict per query against the fp64 oracle ------------------------------------------------
def _real_ids():
  # (collected without a device, as above)
  shapes = P.real_shapes(256)
  return [(c.kname, c.mname, shapes.index((c.n, c.M, c.post_chunk)), c.dtype, form) for c in P.real_cases(256) for form in P.real_forms(c, 256)]


def _log(line):
  print(line)
  path = os.environ.get('HBO_POSTERIOR_LOG')
  if path:
    with open(path, 'a') as f:
      f.write(line + '\n')


def _predict(ctx, case, post_chunk, form):
  """Factor and predict through the Python layer on ctx: (mu [M], var [M]) in the case's dtype."""
  import copy
  import types
  from hyperbo_amd.basics import definitions as defs, linalg
  from hyperbo_amd.gp_utils import gp, kernel, mean, utils
  model, x, y, xq = P.real_inputs(case)
  mn, kn, wf = getattr(mean, case.mname), getattr(kernel, case.kname), utils.DEFAULT_WARP_FUNC
  pn = defs.GPParams(model=copy.deepcopy(model))
  with _Options(ctx, post_chunk=post_chunk, lauum_persist=1, **_form_options(form)):
    h = linalg.factor(mn, kn, pn, x, y, wf, ctx=ctx)
    try:
      mu, var = gp.predict(mn, kn, pn, x, y, xq, wf, cache=types.SimpleNamespace(handle=h))
    finally:
      h.close()
  assert mu.shape == var.shape == (case.M, 1) and mu.dtype == var.dtype == case.np_dtype
  return mu[:, 0], var[:, 0]


@pytest.mark.parametrize('kname,mname,shape,dtype,form', _real_ids())
def test_posterior_per_query_against_the_oracle(gpu_ctx, kname, mname, shape, dtype, form):
  """Mean and variance of every query within C * the query's own terms (posterior_cases.REAL_BOUNDS), the queries' scales orders of
  magnitude apart: a max-norm bound says nothing about a query whose own terms are small.  And the claim of include/hbo.h: post_chunk
  = 128 and 8192 give the same bits."""
  cus = _cus(gpu_ctx)
  n, M, chunk = P.real_shapes(cus)[shape]
  case = P.RealCase(kname, mname, n, M, chunk, dtype)
  assert form in P.real_forms(case, cus), f'{case.id}: {form} is not reachable with {cus} CUs'
  ref = P.real_reference(case)
  mu, var = _predict(gpu_ctx, case, chunk, form)
  other = 8192 if chunk == 128 else 128
  mu2, var2 = _predict(gpu_ctx, case, other, form)
  e_mu = np.abs(mu.astype(np.float64) - ref.mu) / ref.mu_scale
  e_var = np.abs(var.astype(np.float64) - ref.var) / ref.var_scale
  e_mu, e_var = (np.where(np.isfinite(e), e, np.inf) for e in (e_mu, e_var))
  qm, qv = int(np.argmax(e_mu)), int(np.argmax(e_var))
  _log(f'real | {case.id} | {form} | mu {e_mu[qm]:.3e} (query {qm}, kind {qm % 3}) | var {e_var[qv]:.3e} (query {qv}, kind {qv % 3}) | '
       f'gap mu {np.max(ref.gap_mu / ref.mu_scale):.1e} var {np.max(ref.gap_var / ref.var_scale):.1e} | '
       f'max-norm mu {np.max(np.abs(mu - ref.mu)) / np.max(np.abs(ref.mu)):.3e} var {np.max(np.abs(var - ref.var)) / np.max(np.abs(ref.var)):.3e}')
  c_mu, c_var = P.real_bounds(case, form)
  assert e_mu[qm] <= c_mu, f'{case.id} {form}: mean of query {qm}: {e_mu[qm]:.3e} of its own terms {ref.mu_scale[qm]:.3e} (bound {c_mu:g})'
  assert e_var[qv] <= c_var, f'{case.id} {form}: variance of query {qv}: {e_var[qv]:.3e} of its own terms {ref.var_scale[qv]:.3e} (bound {c_var:g})'
  assert np.array_equal(mu, mu2) and np.array_equal(var, var2), f'{case.id} {form}: post_chunk {chunk} and {other} differ in bits'
