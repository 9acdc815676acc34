"""The one-launch acquisition gradient over parameter samples (run with `-m gpu` on an MI355X): hbo_acq_grad_samples
(csrc/acq_small.hip, caches of n <= 128) and the context option 'acq_fused' that routes bo_utils/acfun.py's value_and_grad to it.

Against the oracle (o.acquisition_value_and_grad, the mean over samples) with the bounds of
test_gpu_parity.py::test_hgp_acquisition_value_and_grad_is_the_mean_over_samples (values rtol 1e-8 / atol 1e-10, gradient
1e-7 * max(max |g|, 1e-3)); against the per-sample path (hbo_acq_grad on the same caches) with the batch-vs-loop bound of
test_gpu_parity.py (values rtol 1e-9 / atol 1e-11) and, for the gradient, LOOP_GRAD_TOL below; independence of a row from what
shares its launch, bit for bit.

LOOP_GRAD_TOL.  Both paths form the gradient from the same cache in fp64; they differ in the order of the sums (k, l = W k,
beta = W^T l, the feature reduction).  The largest difference measured over the cases of test_fused_vs_the_per_sample_path on an
MI355X is 3.212e-14 relative to max(max |g|, 1e-3) (dot_product / zero / UCB, n = 128, D = 33, S = 5, M = 1; profiles/acq_fused.md has
every case and the command); the bound is 10 x that, far inside the oracle bound 1e-7.  The routing tests hold the mean over samples
to the same bound."""
import types

import numpy as np
import pytest

import acq_oracle as ao
import helpers
import test_gpu_acq_tails as tails
from oracle import hyperbo_oracle as o

pytestmark = pytest.mark.gpu
WFO = o.DEFAULT_WARP_FUNC
SCALE = 1.5
ACQ = {'ei': 0, 'pi': 1, 'ucb': 2}
MEANS = ['zero', 'constant', 'linear']
NS, DS, SS, MS = [1, 7, 65, 127, 128], [1, 3, 33], [1, 5], [1, 9]
LOOP_GRAD_TOL = 10 * 3.212e-14


def _oracle_cases():
  """36 of the 5 x 3 x 12 x 3 x 2 x 2 product: every covariance x mean with each acquisition once; n, D, S, M cycle with co-prime
  periods, so that every n meets every D, S and M."""
  cases, i = [], 0
  for kname in helpers.KERNELS:
    for mname in MEANS:
      for acq in ('ei', 'pi', 'ucb'):
        cases.append((kname, mname, acq, NS[i % 5], DS[i % 3], SS[i % 2], MS[(i // 2) % 2]))
        i += 1
  return cases


CASES = _oracle_cases()
assert {c[3] for c in CASES} == set(NS) and {c[4] for c in CASES} == set(DS) and len({c[:2] for c in CASES}) == 12


def _nv():
  from hyperbo_amd import _model as hmodel
  from hyperbo_amd import _native as nat
  from hyperbo_amd.basics import definitions as defs, linalg, params_utils
  from hyperbo_amd.bo_utils import acfun, bayesopt
  from hyperbo_amd.gp_utils import gp, kernel, mean, utils
  return types.SimpleNamespace(hmodel=hmodel, nat=nat, defs=defs, linalg=linalg, params_utils=params_utils, acfun=acfun, bayesopt=bayesopt,
                               gp=gp, kernel=kernel, mean=mean, utils=utils)


def _cast(t, dtype):
  return {k: _cast(v, dtype) for k, v in t.items()} if isinstance(t, dict) else np.asarray(t, dtype=dtype)


class Case:
  """S parameter samples of one family, their factors of one sub-dataset, M queries.  Close it."""

  def __init__(self, kname, mname, n, d, S, M, dtype=np.float64, seed=71, samples=None, xq=None, warp=True):
    nv = self.nv = _nv()
    rng = np.random.default_rng(seed)
    self.kname, self.mname, self.d, self.dtype = kname, mname, d, np.dtype(dtype)
    self.samples = samples if samples is not None else [_cast(helpers.make_model(np.random.default_rng(seed * 100 + i), mname, False, d), dtype)
                                                        for i in range(S)]
    self.x, self.y = helpers.synthetic_task(rng, n, d, dtype=dtype)
    self.xq = np.ascontiguousarray(rng.uniform(size=(M, d)).astype(dtype)) if xq is None else xq
    self.wf, self.wfo = (nv.utils.DEFAULT_WARP_FUNC, WFO) if warp else (None, None)
    self.kn, self.mn, self.ko, self.mo = getattr(nv.kernel, kname), getattr(nv.mean, mname), getattr(o, kname), getattr(o, mname)
    self.handles, self.built, self.noises = [], [], []
    for smp in self.samples:
      pn = nv.defs.GPParams(model=smp, config={})
      self.handles.append(nv.linalg.factor(self.mn, self.kn, pn, self.x, self.y, self.wf))
      self.built.append(nv.hmodel.BuiltModel(self.mn, self.kn, pn, self.wf, dtype, d))
      self.noises.append(float(np.squeeze(o.retrieve_params(o.GPParams(model=_cast(smp, np.float64)), ['noise_variance'], self.wfo)[0])))

  def close(self):
    for h in self.handles:
      h.close()

  def fused(self, acq_id, param, sel=None, xq=None):
    sel = range(len(self.samples)) if sel is None else sel
    xq = self.xq if xq is None else xq
    return self.nv.acfun._fused_value_and_grad([self.built[s] for s in sel], [self.handles[s] for s in sel], [self.noises[s] for s in sel],
                                               xq, acq_id, param, SCALE)

  def loop(self, acq_id, param):
    nat = self.nv.nat
    M = self.xq.shape[0]
    vals, grads = [], []
    for bm, h, noise in zip(self.built, self.handles, self.noises):
      out, g = np.empty((M, 1), dtype=self.dtype), np.zeros((M, self.d))
      h.ctx.check(nat.lib().hbo_acq_grad(h.ctx.handle, bm.ref(), h.handle, nat.ptr(self.xq), M, acq_id, float(param), float(noise), SCALE,
                                         nat.ptr(out), g.ctypes.data_as(nat.C.POINTER(nat.C.c_double))))
      vals.append(out); grads.append(g)
    return np.asarray(vals), np.asarray(grads)

  def oracle(self, acq, param):
    x, y = self.x, self.y
    vals, grads = [], []
    for smp, noise in zip(self.samples, self.noises):
      v, g = o.acquisition_value_and_grad(acq, self.mo, self.ko, o.GPParams(model=_cast(smp, np.float64), config={}), x.astype(np.float64),
                                          y.astype(np.float64), self.xq.astype(np.float64), param, self.wfo, add_noise=noise, scale=SCALE)
      vals.append(v); grads.append(g)
    return np.asarray(vals), np.asarray(grads)


def _param(acq, y):
  return {'ei': float(np.max(y)), 'pi': float(np.max(y)) + 0.1, 'ucb': 3.0}[acq]


def _grad_err(g, ref):
  return float(np.max(np.abs(g - ref)) / max(np.max(np.abs(ref)), 1e-3))


@pytest.fixture
def fused_option(gpu_ctx):
  """Sets the context option for the test and restores it."""
  before = gpu_ctx.get_option('acq_fused')

  def set_to(v):
    gpu_ctx.set_option('acq_fused', v)
  try:
    yield set_to
  finally:
    gpu_ctx.set_option('acq_fused', before)


@pytest.mark.parametrize('kname,mname,acq,n,d,S,M', CASES, ids=['-'.join(map(str, c)) for c in CASES])
def test_fused_vs_the_oracle_and_the_per_sample_path(gpu_ctx, kname, mname, acq, n, d, S, M):
  c = Case(kname, mname, n, d, S, M)
  try:
    param = _param(acq, c.y)
    val, grad = c.fused(ACQ[acq], param)
    assert val.shape == (S, M, 1) and val.dtype == np.float64 and grad.shape == (S, M, d) and grad.dtype == np.float64
    vo, go = c.oracle(acq, param)
    vl, gl = c.loop(ACQ[acq], param)
    e_loop = _grad_err(grad, gl)
    print(f'\nacq fused: {kname} {mname} {acq} n={n} D={d} S={S} M={M}: gradient vs oracle (mean) {_grad_err(grad.mean(0), go.mean(0)):.3e}, '
          f'vs hbo_acq_grad {e_loop:.3e}; value vs hbo_acq_grad {helpers.rel_err(val, vl):.3e}')
    # the mean over samples, as acfun forms it, against the oracle's
    np.testing.assert_allclose(val.mean(0), vo.mean(0), rtol=1e-8, atol=1e-10)
    assert np.max(np.abs(grad.mean(0) - go.mean(0))) <= 1e-7 * max(np.max(np.abs(go.mean(0))), 1e-3)
    # the per-sample path on the same caches
    np.testing.assert_allclose(val, vl, rtol=1e-9, atol=1e-11)
    assert e_loop <= LOOP_GRAD_TOL, e_loop
  finally:
    c.close()


def test_fp32_against_the_fp64_oracle(gpu_ctx):
  c = Case('matern52', 'constant', 100, 4, 3, 9, dtype=np.float32, seed=72)
  try:
    for acq in ('ucb', 'ei'):
      param = _param(acq, c.y)
      val, grad = c.fused(ACQ[acq], param)
      vo, go = c.oracle(acq, param)
      assert val.dtype == np.float32 and grad.dtype == np.float64
      ev, eg = np.max(np.abs(val - vo)) / np.max(np.abs(vo)), np.max(np.abs(grad - go)) / np.max(np.abs(go))
      print(f'\nacq fused: fp32 {acq}: value {ev:.3e}, gradient {eg:.3e}')
      assert ev <= 5e-3 and eg <= 2e-2
  finally:
    c.close()


@pytest.mark.parametrize('kname,mname,dtype', [('squared_exponential', 'linear', np.float64), ('dot_product', 'constant', np.float64),
                                                ('matern32', 'linear', np.float32)])
def test_a_row_does_not_depend_on_what_shares_the_launch(gpu_ctx, kname, mname, dtype):
  c = Case(kname, mname, 77, 3, 5, 9, dtype=dtype, seed=73)
  try:
    param = _param('ei', c.y)
    val, grad = c.fused(0, param)
    val2, grad2 = c.fused(0, param)
    assert np.array_equal(val, val2) and np.array_equal(grad, grad2) and np.isfinite(val).all() and np.isfinite(grad).all()
    for s in range(5):
      v1, g1 = c.fused(0, param, sel=[s])
      assert np.array_equal(v1[0], val[s]) and np.array_equal(g1[0], grad[s]), s
    for q in (0, 4, 8):
      vq, gq = c.fused(0, param, xq=np.ascontiguousarray(c.xq[q:q + 1]))
      assert np.array_equal(vq[:, 0], val[:, q]) and np.array_equal(gq[:, 0], grad[:, q]), q
  finally:
    c.close()


def test_cache_after_a_row_append(gpu_ctx):
  nv = _nv()
  rng = np.random.default_rng(74)
  d = 3
  model = helpers.make_model(rng, 'constant', False, d)
  x, y = helpers.synthetic_task(rng, 101, d)
  ds = {0: nv.defs.SubDataset(x[:100], y[:100]), 1: nv.defs.SubDataset(x[:9], y[:9]), 2: nv.defs.SubDataset(x[:5], y[:5])}
  m = nv.gp.GP(ds, nv.mean.constant, nv.kernel.matern52, nv.defs.GPParams(model=model, config={}), nv.utils.DEFAULT_WARP_FUNC)
  m.setup_predictor(0)
  h = m.params.cache[0].handle
  m.update_sub_dataset((x[100:], y[100:]), 0, is_append=True)
  m.setup_predictor(0)
  assert m.params.cache[0].handle is h and h.n == 101      # the O(N^2) append, not a new factor
  bm = nv.hmodel.BuiltModel(nv.mean.constant, nv.kernel.matern52, m.params, nv.utils.DEFAULT_WARP_FUNC, np.float64, d)
  xq = rng.uniform(size=(9, d))
  po = o.GPParams(model=model, config={})
  noise = float(np.squeeze(o.retrieve_params(po, ['noise_variance'], WFO)[0]))
  val, grad = nv.acfun._fused_value_and_grad([bm], [h], [noise], xq, 2, 3.0, SCALE)
  vo, go = o.acquisition_value_and_grad('ucb', o.constant, o.matern52, po, x, y, xq, 3.0, WFO, add_noise=noise, scale=SCALE)
  np.testing.assert_allclose(val[0], vo, rtol=1e-8, atol=1e-10)
  assert np.max(np.abs(grad[0] - go)) <= 1e-7 * max(np.max(np.abs(go)), 1e-3)


@pytest.mark.parametrize('kname', ['matern32', 'matern52'])
def test_matern_query_on_a_training_point(gpu_ctx, kname):
  rng = np.random.default_rng(75)
  x, _ = helpers.synthetic_task(rng, 40, 3)
  xq = np.ascontiguousarray(np.vstack([x[7], rng.uniform(size=3), x[39]]))
  c = Case(kname, 'linear', 40, 3, 2, 3, seed=75, xq=xq)
  try:
    assert np.array_equal(c.x[7], xq[0]) and np.array_equal(c.x[39], xq[2])
    for acq in ('ei', 'ucb'):
      param = _param(acq, c.y)
      val, grad = c.fused(ACQ[acq], param)
      vo, go = c.oracle(acq, param)
      assert np.isfinite(grad).all() and np.isfinite(val).all()
      np.testing.assert_allclose(val, vo, rtol=1e-8, atol=1e-10)
      for s in range(2):
        assert np.max(np.abs(grad[s] - go[s])) <= 1e-7 * max(np.max(np.abs(go[s])), 1e-3)
  finally:
    c.close()


def test_ei_in_the_tail_against_mpmath(gpu_ctx):
  """EI at gamma = 10 and 25 (u = -10, -25) per query against acq_oracle.exact_ei of the device's own posterior (hbo_predict), with the
  relative bound test_gpu_acq_tails.py holds hbo_acq_grad's value to: the posterior term of two device routes to mu, var plus the
  epilogue bound."""
  c = tails._case(gpu_ctx, 'squared_exponential', False, 'constant', 100, 7, np.float64, seed=76)
  try:
    mu, var = tails._predict(c)
    sd = tails._device_sd(c, var)
    nv = _nv()
    reached = set()
    for k, g in enumerate((10.0, 25.0)):
      qk = (k * 5) % 7
      target = tails._target(c, qk, g)
      val, _ = nv.acfun._fused_value_and_grad([c.bm], [c.h], [c.noise], c.xq, 0, target, tails.SCALE)
      for q in range(7):
        gq = ao.exact_gamma(mu[q], sd[q], target)
        if not -10.25 <= gq <= 37.25:
          continue
        if q == qk and abs(gq - g) <= 0.25:
          reached.add(g)
        bound = tails._posterior_term(c, gq, float(sd[q]), True) + tails._epilogue_bound(gq, np.float64)
        r = ao.rel_to(val[0, q, 0], ao.exact_ei(mu[q], sd[q], target)) / bound
        print(f'\nacq fused: EI tail gamma {gq:.3f}: ratio to the bound {r:.3e}')
        assert val[0, q, 0] > 0 and r <= 1.0, (g, q, gq, float(val[0, q, 0]), r)
    assert reached == {10.0, 25.0}
  finally:
    tails._close(c)


def test_a_sample_that_is_not_positive_definite(gpu_ctx):
  nv = _nv()
  bad = [{'dot_prod_sigma': np.array(1.0), 'dot_prod_bias': np.array(0.1), 'noise_variance': np.array(nvar)} for nvar in (0.1, -1.0, 0.2)]
  c = Case('dot_product', 'zero', 90, 2, 3, 4, seed=77, samples=bad, warp=False)
  try:
    assert [h.status for h in c.handles] == [nv.nat.HBO_OK, nv.nat.HBO_NOT_PD, nv.nat.HBO_OK]
    nat = nv.nat
    structs = (nat.Model * 3)(*[b.struct for b in c.built])
    caches = (nat.C.c_void_p * 3)(*[h.handle for h in c.handles])
    prm = (nat.C.c_double * 3)(3.0, 3.0, 3.0)
    nse = (nat.C.c_double * 3)(*c.noises)
    val, grad = np.zeros((3, 4, 1)), np.zeros((3, 4, 2))
    ctx = c.handles[0].ctx
    rc = nat.lib().hbo_acq_grad_samples(ctx.handle, structs, 3, caches, nat.ptr(c.xq), 4, 2, prm, nse, SCALE, nat.ptr(val),
                                        grad.ctypes.data_as(nat.C.POINTER(nat.C.c_double)))
    assert rc == nat.HBO_NOT_PD
    assert np.isnan(val[1]).all() and np.isnan(grad[1]).all()
    for s in (0, 2):
      v1, g1 = c.fused(2, 3.0, sel=[s])
      assert np.isfinite(v1).all() and np.array_equal(v1[0], val[s]) and np.array_equal(g1[0], grad[s])
  finally:
    c.close()


def test_refusals_touch_no_output(gpu_ctx):
  nv = _nv()
  nat = nv.nat
  rng = np.random.default_rng(78)
  d = 3
  wf = nv.utils.DEFAULT_WARP_FUNC
  cfg = {'mlp_features': helpers.MLP_FEATURES}
  xq = rng.uniform(size=(2, d))
  err = lambda ctx: (nat.lib().hbo_last_error(ctx.handle) or b'').decode()

  def call(built, handles):
    S = len(built)
    structs = (nat.Model * S)(*[b.struct for b in built])
    caches = (nat.C.c_void_p * S)(*[h.handle if h is not None else None for h in handles])
    prm, nse = (nat.C.c_double * S)(*([3.0] * S)), (nat.C.c_double * S)(*([0.1] * S))
    val, grad = np.full((S, 2, 1), 7.0), np.full((S, 2, d), 7.0)
    rc = nat.lib().hbo_acq_grad_samples(gpu_ctx.handle, structs, S, caches, nat.ptr(xq), 2, 2, prm, nse, SCALE, nat.ptr(val),
                                        grad.ctypes.data_as(nat.C.POINTER(nat.C.c_double)))
    assert np.all(val == 7.0) and np.all(grad == 7.0)
    return rc, err(gpu_ctx)

  def one(kn, mn, model, n):
    x, y = helpers.synthetic_task(rng, n, d)
    pn = nv.defs.GPParams(model=model, config=dict(cfg))
    return nv.hmodel.BuiltModel(mn, kn, pn, wf, np.float64, d), nv.linalg.factor(mn, kn, pn, x, y, wf)

  handles = []
  try:
    plain = helpers.make_model(rng, 'constant', False, d)
    b_ok, h_ok = one(nv.kernel.matern52, nv.mean.constant, plain, 30); handles.append(h_ok)
    b, h = one(nv.kernel.matern52, nv.mean.constant, plain, 129); handles.append(h)
    rc, msg = call([b], [h]); assert rc == nat.HBO_ERR_UNSUPPORTED and 'n > 128' in msg, (rc, msg)
    rc, msg = call([b_ok], [None]); assert rc == nat.HBO_ERR_UNSUPPORTED and 'prior branch' in msg, (rc, msg)
    b, h = one(nv.kernel.matern52_mlp, nv.mean.constant, helpers.make_model(rng, 'constant', True, d), 30); handles.append(h)
    rc, msg = call([b], [h]); assert rc == nat.HBO_ERR_UNSUPPORTED and 'MLP basis' in msg, (rc, msg)
    b, h = one(nv.kernel.matern52, nv.mean.linear_mlp, helpers.make_model(rng, 'linear_mlp', False, d), 30); handles.append(h)
    rc, msg = call([b], [h]); assert rc == nat.HBO_ERR_UNSUPPORTED and 'linear_mlp' in msg, (rc, msg)
    km = dict(plain); km['kumar_params'] = {'a': np.full(d, 0.3), 'b': np.full(d, -0.2)}
    b, h = one(nv.kernel.matern52_kumar, nv.mean.constant, km, 30); handles.append(h)
    rc, msg = call([b], [h]); assert rc == nat.HBO_ERR_UNSUPPORTED and 'Kumaraswamy' in msg, (rc, msg)
    # mixed families: another covariance, another mean, another dtype's cache
    b2, h2 = one(nv.kernel.matern32, nv.mean.constant, plain, 30); handles.append(h2)
    rc, msg = call([b_ok, b2], [h_ok, h2]); assert rc == nat.HBO_ERR_ARG and 'must share' in msg, (rc, msg)
    b3, h3 = one(nv.kernel.matern52, nv.mean.zero, plain, 30); handles.append(h3)
    rc, msg = call([b_ok, b3], [h_ok, h3]); assert rc == nat.HBO_ERR_ARG and 'must share' in msg, (rc, msg)
    x32, y32 = helpers.synthetic_task(rng, 30, d, dtype=np.float32)
    h32 = nv.linalg.factor(nv.mean.constant, nv.kernel.matern52, nv.defs.GPParams(model=_cast(plain, np.float32), config={}), x32, y32, wf)
    handles.append(h32)
    rc, msg = call([b_ok], [h32]); assert rc == nat.HBO_ERR_ARG and 'mismatch' in msg, (rc, msg)
  finally:
    for h in handles:
      h.close()


def _count_calls(monkeypatch, nat):
  """Wraps the two entry points on the loaded library; returns the counters."""
  counts = {'samples': 0, 'single': 0}
  lib = nat.lib()
  real_s, real_1 = lib.hbo_acq_grad_samples, lib.hbo_acq_grad

  def wrap_s(*a):
    counts['samples'] += 1
    return real_s(*a)

  def wrap_1(*a):
    counts['single'] += 1
    return real_1(*a)
  monkeypatch.setattr(lib, 'hbo_acq_grad_samples', wrap_s)
  monkeypatch.setattr(lib, 'hbo_acq_grad', wrap_1)
  return counts


def _hgp(nv, n, S, d=3, seed=79, kname='matern52', mname='linear'):
  rng = np.random.default_rng(seed)
  samples = [helpers.make_model(np.random.default_rng(seed * 100 + i), mname, False, d) for i in range(S)]
  x, y = helpers.synthetic_task(rng, n, d)
  x2, y2 = helpers.synthetic_task(rng, 20, d)
  ds = {'test': nv.defs.SubDataset(x, y), 'other': nv.defs.SubDataset(x2, y2), 'third': nv.defs.SubDataset(x2[:5], y2[:5])}
  hgp = nv.gp.HGP(ds, getattr(nv.mean, mname), getattr(nv.kernel, kname), nv.defs.GPParams(model=samples[0], samples=samples, config={}),
                  nv.utils.DEFAULT_WARP_FUNC)
  return hgp, samples, rng.uniform(size=(5, d))


def _loop_by_hand(nv, hgp, samples, xq, acq_id, param):
  """The parent's HGP loop restated: one hbo_acq_grad per sample on factors of its own, summed in sample order, divided."""
  nat = nv.nat
  sd = hgp.dataset['test']
  _, scale = hgp.predict_noise_and_scale(True, True)
  val, grad = np.zeros((xq.shape[0], 1)), np.zeros((xq.shape[0], hgp.input_dim))
  for smp in samples:
    pn = nv.defs.GPParams(model=smp, config={})
    h = nv.linalg.factor(hgp.mean_func, hgp.cov_func, pn, sd.x, sd.y, hgp.warp_func)
    try:
      bm = nv.hmodel.BuiltModel(hgp.mean_func, hgp.cov_func, pn, hgp.warp_func, np.float64, hgp.input_dim)
      noise = float(np.squeeze(nv.params_utils.retrieve_params(pn, ['noise_variance'], warp_func=hgp.warp_func)[0]))
      out, g = np.empty((xq.shape[0], 1)), np.zeros((xq.shape[0], hgp.input_dim))
      h.ctx.check(nat.lib().hbo_acq_grad(h.ctx.handle, bm.ref(), h.handle, nat.ptr(xq), xq.shape[0], acq_id, float(param), noise, float(scale),
                                         nat.ptr(out), g.ctypes.data_as(nat.C.POINTER(nat.C.c_double))))
    finally:
      h.close()
    val += out; grad += g
  return val / len(samples), grad / len(samples)


def test_routing_off_is_the_per_sample_loop_bit_for_bit(gpu_ctx, fused_option, monkeypatch):
  nv = _nv()
  fused_option(0)
  hgp, samples, xq = _hgp(nv, 30, 4)
  try:
    want_v, want_g = _loop_by_hand(nv, hgp, samples, xq, 2, 3.0)
    counts = _count_calls(monkeypatch, nv.nat)
    val, grad = nv.acfun.ucb.value_and_grad(model=hgp, sub_dataset_key='test', x_queries=xq)
    assert counts == {'samples': 0, 'single': 4}
    assert np.array_equal(val, want_v) and np.array_equal(grad, want_g)
    # a plain GP: one hbo_acq_grad, the numbers of the direct call
    m = nv.gp.GP(hgp.dataset, hgp.mean_func, hgp.cov_func, nv.defs.GPParams(model=samples[1], config={}), hgp.warp_func)
    v1, g1 = nv.acfun.ucb.value_and_grad(model=m, sub_dataset_key='test', x_queries=xq)
    assert counts == {'samples': 0, 'single': 5}
    w1, wg1 = _loop_by_hand(nv, hgp, samples[1:2], xq, 2, 3.0)
    assert np.array_equal(v1, w1) and np.array_equal(g1, wg1)
  finally:
    nv.acfun.drop_sample_caches(hgp)


def test_routing_on_is_one_library_call(gpu_ctx, fused_option, monkeypatch):
  nv = _nv()
  hgp, samples, xq = _hgp(nv, 30, 4)
  try:
    fused_option(0)
    off_v, off_g = nv.acfun.expected_improvement.value_and_grad(model=hgp, sub_dataset_key='test', x_queries=xq)
    fused_option(1)
    assert nv.nat.acq_fused_enabled()
    counts = _count_calls(monkeypatch, nv.nat)
    for rep in range(2):   # the second call finds the factors cached: still exactly one call
      val, grad = nv.acfun.expected_improvement.value_and_grad(model=hgp, sub_dataset_key='test', x_queries=xq)
      assert counts == {'samples': rep + 1, 'single': 0}
      assert val.shape == (5, 1) and val.dtype == np.float64 and grad.shape == (5, 3) and grad.dtype == np.float64
      assert hgp.params.model is samples[-1] and hgp.params.cache == {}
      np.testing.assert_allclose(val, off_v, rtol=1e-9, atol=1e-11)
      assert _grad_err(grad, off_g) <= LOOP_GRAD_TOL
    # a plain GP with the option on: S = 1 through the same entry point
    m = nv.gp.GP(hgp.dataset, hgp.mean_func, hgp.cov_func, nv.defs.GPParams(model=samples[2], config={}), hgp.warp_func)
    v1, g1 = nv.acfun.expected_improvement.value_and_grad(model=m, sub_dataset_key='test', x_queries=xq)
    assert counts == {'samples': 3, 'single': 0} and v1.shape == (5, 1) and g1.shape == (5, 3)
    fused_option(0)
    v0, g0 = nv.acfun.expected_improvement.value_and_grad(model=m, sub_dataset_key='test', x_queries=xq)
    assert counts == {'samples': 3, 'single': 1}
    np.testing.assert_allclose(v1, v0, rtol=1e-9, atol=1e-11)
    assert _grad_err(g1, g0) <= LOOP_GRAD_TOL
  finally:
    nv.acfun.drop_sample_caches(hgp)


def test_routing_on_with_an_ineligible_model_uses_the_loop(gpu_ctx, fused_option, monkeypatch):
  nv = _nv()
  hgp, samples, xq = _hgp(nv, 131, 3, seed=80)
  try:
    fused_option(0)
    off_v, off_g = nv.acfun.ucb.value_and_grad(model=hgp, sub_dataset_key='test', x_queries=xq)
    fused_option(1)
    assert '131 > 128' in nv.acfun._acq_fused_unmet(hgp, 'test', 3, 3)
    counts = _count_calls(monkeypatch, nv.nat)
    val, grad = nv.acfun.ucb.value_and_grad(model=hgp, sub_dataset_key='test', x_queries=xq)
    assert counts == {'samples': 0, 'single': 3}
    assert np.array_equal(val, off_v) and np.array_equal(grad, off_g)
  finally:
    nv.acfun.drop_sample_caches(hgp)


def test_bayesopt_loop_on_an_hgp_with_the_option_on(gpu_ctx, fused_option, monkeypatch):
  nv = _nv()
  fused_option(1)
  hgp, samples, _ = _hgp(nv, 6, 3, d=2, seed=81, mname='constant')
  f = lambda xx: -np.sum((np.atleast_2d(xx) - 0.3)**2, axis=1, keepdims=True)
  hgp.update_sub_dataset((hgp.dataset['test'].x, f(hgp.dataset['test'].x)), 'test')
  counts = _count_calls(monkeypatch, nv.nat)
  dropped = []
  real_drop = nv.acfun.drop_sample_caches
  monkeypatch.setattr(nv.acfun, 'drop_sample_caches', lambda m: (dropped.append(getattr(m, '_hbo_sample_caches', None) is not None), real_drop(m))[1])
  try:
    out = nv.bayesopt.bayesopt(7, hgp, 'test', f, nv.acfun.ucb, iters=2, input_sampler=lambda key, dim: key.uniform(size=(16, dim)))
    assert out.x.shape == (8, 2) and out.y.shape == (8, 1) and np.isfinite(out.x).all() and np.isfinite(out.y).all()
    assert np.all(out.x >= 0) and np.all(out.x <= 1)
    assert counts['samples'] >= 2 and counts['single'] == 0       # every L-BFGS-B evaluation was one fused call
    assert sum(dropped) >= 2 and hgp._hbo_sample_caches is None     # the factors were dropped at each append
  finally:
    real_drop(hgp)
