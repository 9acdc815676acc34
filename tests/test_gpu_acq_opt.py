"""hbo_acq_maximize, ac_func.maximize and config['acq_opt_on_device'] on the device (run with `-m gpu` on an MI355X).

The device loop against the same run driven from the host -- a Python loop over the fused acquisition kernel (through the hook
hbo_probe_acq_grad_samples64, which is hbo_acq_grad_samples plus the fp64 values the control kernel reads) that feeds
hbo_probe_acq_opt_ctl -- to the bit, fp64 and fp32; against the oracle-driven NumPy restatement (tests/acq_opt_oracle.py): the same
sequence of decisions, final point and value within measured bounds; independence of a start from what shares its call, from how the
run is cut into calls and from `hbo_tune poison`; corners and caller bounds; refusals; ac_func.maximize and bayesopt().

DEV_X_TOL, DEV_VALUE_TOL, FP32_VALUE_TOL: 10 x the largest deviation measured on an MI355X over all cases and starts
(profiles/acq_opt.md has the run): final point |x - x_oracle|_inf, final value |v - v_oracle| / max(1, |v_oracle|), and the same for
the fp32 run's value against the fp64 oracle run."""
import ctypes as C
import types

import numpy as np
import pytest

import acq_opt_oracle as ao

pytestmark = pytest.mark.gpu
EVALS = ao.MAX_EVALS
# box-matern32-ei; dot_product-linear-ucb-n128-D33-S5-R9 (both values)
DEV_X_MEASURED, DEV_VALUE_MEASURED, FP32_VALUE_MEASURED = 5.045e-12, 2.952e-14, 1.213e-5
DEV_X_TOL, DEV_VALUE_TOL, FP32_VALUE_TOL = 10 * DEV_X_MEASURED, 10 * DEV_VALUE_MEASURED, 10 * FP32_VALUE_MEASURED
IDS = [c.name for c in ao.CASES]


def _nv():
  from hyperbo_amd import _model as hmodel
  from hyperbo_amd import _native as nat
  from hyperbo_amd.basics import definitions as defs, linalg
  from hyperbo_amd.bo_utils import acfun, bayesopt
  from hyperbo_amd.gp_utils import gp, kernel, mean, utils
  return types.SimpleNamespace(hmodel=hmodel, nat=nat, defs=defs, linalg=linalg, acfun=acfun, bayesopt=bayesopt, gp=gp, kernel=kernel, mean=mean,
                               utils=utils)


class Dev:
  """The S samples of a case factorised on the device, and the calls the tests make on them.  Close it."""

  def __init__(self, case, dtype=np.float64):
    nv = self.nv = _nv()
    self.case, self.dtype, inp = case, np.dtype(dtype), ao.inputs(case)
    self.inp = inp
    kn, mn, wf = getattr(nv.kernel, case.kname), getattr(nv.mean, case.mname), nv.utils.DEFAULT_WARP_FUNC
    x, y = inp.x.astype(dtype), inp.y.astype(dtype)
    self.handles, self.built, self.noises = [], [], []
    for smp in inp.samples:
      pn = nv.defs.GPParams(model=ao._cast(smp, dtype), config={})
      self.handles.append(nv.linalg.factor(mn, kn, pn, x, y, wf))
      self.built.append(nv.hmodel.BuiltModel(mn, kn, pn, wf, dtype, case.d))
      self.noises.append(ao.noise_of(ao._cast(smp, dtype)))
    self.ctx = self.handles[0].ctx
    s = len(self.built)
    nat = nv.nat
    self.structs = (nat.Model * s)(*[b.struct for b in self.built])
    self.caches = (nat.C.c_void_p * s)(*[h.handle for h in self.handles])
    self.prm = (nat.C.c_double * s)(*([float(self.dtype.type(inp.param))] * s))
    self.nse = (nat.C.c_double * s)(*self.noises)
    self.opts = nat.AcqOptOpts(**ao.DEFAULTS)
    self.ns = nat.lib().hbo_acq_opt_state_doubles(case.d, self.opts.memory)
    self.x0 = np.ascontiguousarray(inp.x0, dtype=dtype)
    unit = (case.lo, case.hi) == (0.0, 1.0)
    self.lo, self.hi = (None, None) if unit else (inp.lo, inp.hi)

  def close(self):
    for h in self.handles:
      h.close()

  def maximize(self, x0=None, evals=EVALS, state=None, want_log=True, rc_only=False, r=None):
    """One hbo_acq_maximize call: (log [evals, R], x_out, val_out, status, state).  r: the R handed over, if not x0's rows."""
    nat = self.nv.nat
    x0 = self.x0 if x0 is None else x0
    rows = x0.shape[0]
    r = rows if r is None else r
    state = np.zeros((rows, self.ns)) if state is None else state
    x, val, status = np.full((rows, self.case.d), 7.0), np.full(rows, 7.0), np.full(rows, 7, dtype=np.int32)
    log = np.zeros((max(evals, 1), rows), dtype=nat.ACQ_OPT_EVAL_DTYPE) if want_log else None
    rc = nat.lib().hbo_acq_maximize(self.ctx.handle, self.structs, len(self.built), self.caches, nat.ptr(x0), r, nat.ptr(self.lo), nat.ptr(self.hi),
                                    ao.ACQ_IDS[self.case.acq], self.prm, self.nse, ao.SCALE, C.byref(self.opts), nat.ptr(state), evals,
                                    nat.ptr(x), nat.ptr(val), nat.ptr(status), nat.ptr(log))
    if rc_only:
      return rc, x, val, status
    self.ctx.check(rc, allow_not_pd=False)
    return log, x, val, status, state

  def samples64(self, xq):
    """(values in the model dtype [S, M], gradients [S, M, D], fp64 values [S, M]) of the fused kernel at xq [M, D]."""
    nat = self.nv.nat
    s, (m, d) = len(self.built), xq.shape
    out, g, v64 = np.empty((s, m), dtype=self.dtype), np.empty((s, m, d)), np.empty((s, m))
    pd = nat.C.POINTER(nat.C.c_double)
    self.ctx.check(nat.lib().hbo_probe_acq_grad_samples64(self.ctx.handle, self.structs, s, self.caches, nat.ptr(xq), m, ao.ACQ_IDS[self.case.acq],
                                                          self.prm, self.nse, ao.SCALE, nat.ptr(out), g.ctypes.data_as(pd), v64.ctypes.data_as(pd)),
                   allow_not_pd=False)
    return out, g, v64

  def host_driven(self, evals=EVALS):
    """The same run as a Python loop: the fused kernel on the pending points, the hook once per start.  The outputs of maximize()."""
    nat = self.nv.nat
    r, d = self.x0.shape
    state = np.zeros((r, self.ns))
    log = np.zeros((evals, r), dtype=nat.ACQ_OPT_EVAL_DTYPE)
    pending = self.x0.copy()
    x, status = np.zeros((r, d)), np.zeros(r, dtype=np.int32)
    ev, st, x_next, x_iter = nat.AcqOptEval(), C.c_int32(0), np.zeros(d), np.zeros(d)
    for e in range(evals):
      _, grads, v64 = self.samples64(pending)
      for k in range(r):
        start = np.ascontiguousarray(pending[k], dtype=np.float64)
        rc = nat.lib().hbo_probe_acq_opt_ctl(nat.ptr(state[k]), d, nat.dtype_code(self.dtype), C.byref(self.opts), nat.ptr(self.lo), nat.ptr(self.hi),
                                             nat.ptr(start), nat.ptr(np.ascontiguousarray(v64[:, k])), nat.ptr(np.ascontiguousarray(grads[:, k])),
                                             len(self.built), nat.ptr(x_next), nat.ptr(x_iter), C.byref(ev), C.byref(st))
        assert rc == nat.HBO_OK, (nat.lib().hbo_last_error(None) or b'').decode()
        log[e, k] = (ev.kind, ev.iter, ev.alpha, ev.value)
        if ev.kind != nat.ACQ_OPT_IDLE:
          pending[k] = x_next
        x[k], status[k] = x_iter, st.value
    return log, x, -state[:, 5], status, state


def same_bits(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_outputs(got, want):
  for g, w, what in zip(got, want, ('log', 'x_out', 'val_out', 'status', 'state')):
    assert same_bits(g, w), what


@pytest.fixture(scope='module')
def runs(gpu_ctx):
  """One device run per case and dtype, shared by the tests below and not to be written to."""
  cache = {}

  def get(case, dtype=np.float64):
    key = (case.name, np.dtype(dtype).name)
    if key not in cache:
      dev = Dev(case, dtype)
      try:
        cache[key] = dev.maximize()
      finally:
        dev.close()
    return cache[key]
  return get


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['fp64', 'fp32'])
@pytest.mark.parametrize('case', ao.CASES, ids=IDS)
def test_device_loop_is_the_host_driven_hook_to_the_bit(gpu_ctx, runs, case, dtype):
  got = runs(case, dtype)
  dev = Dev(case, dtype)
  try:
    want = dev.host_driven()
    same_outputs(got, want)
    log, x, val, status, _ = got
    assert np.all(log['kind'][0] == ao.START)
    # the first logged value is -mean of the per-sample values at x0, summed in sample order
    out, grads, v64 = dev.samples64(dev.x0)
    if dtype == np.float64:
      nat = dev.nv.nat
      o2, g2 = np.empty_like(out), np.empty_like(grads)
      dev.ctx.check(nat.lib().hbo_acq_grad_samples(dev.ctx.handle, dev.structs, len(dev.built), dev.caches, nat.ptr(dev.x0), dev.x0.shape[0],
                                                   ao.ACQ_IDS[case.acq], dev.prm, dev.nse, ao.SCALE, nat.ptr(o2),
                                                   g2.ctypes.data_as(nat.C.POINTER(nat.C.c_double))))
      assert same_bits(o2, out) and same_bits(g2, grads) and same_bits(v64, out)
    else:
      assert same_bits(v64.astype(np.float32), out)
    for k in range(case.R):
      assert log['value'][0, k] == ao.reduce_samples(v64[:, k], grads[:, k])[0]
    assert np.array_equal(x, x.astype(dtype).astype(np.float64))     # representable in the model dtype
    assert np.all(x >= dev.inp.lo) and np.all(x <= dev.inp.hi)
  finally:
    dev.close()


def _kinds(log, k):
  kinds = [int(v) for v in log['kind'][:, k]]
  return kinds[:kinds.index(ao.IDLE)] if ao.IDLE in kinds else kinds


@pytest.mark.parametrize('case', ao.CASES, ids=IDS)
def test_device_loop_against_the_oracle_driven_restatement(gpu_ctx, runs, case):
  log, x, val, status, _ = runs(case)
  log32, _, val32, _, _ = runs(case, np.float32)
  worst = [0.0, 0.0, 0.0]
  for k in range(case.R):
    ref = ao.oracle_run(case, k)
    assert _kinds(log, k) == [e[0] for e in ref.log], (k, _kinds(log, k), [e[0] for e in ref.log])
    n = len(ref.log)
    assert [int(v) for v in log['iter'][:n, k]] == [e[1] for e in ref.log] and status[k] == ref.status
    worst[0] = max(worst[0], float(np.max(np.abs(x[k] - ref.x))))
    worst[1] = max(worst[1], abs(val[k] + ref.f) / max(1.0, abs(ref.f)))
    worst[2] = max(worst[2], abs(val32[k] + ref.f) / max(1.0, abs(ref.f)))
  print(f'\nacq opt device vs oracle: {case.name}: |dx|_inf {worst[0]:.3e}, value {worst[1]:.3e}, fp32 value {worst[2]:.3e}')
  assert worst[0] <= DEV_X_TOL and worst[1] <= DEV_VALUE_TOL and worst[2] <= FP32_VALUE_TOL, worst


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['fp64', 'fp32'])
@pytest.mark.parametrize('name', ['matern32-zero-ucb-n128-D33-S5-R9', 'box-matern32-ei', 'corner-dot-ucb'])
def test_a_start_does_not_depend_on_its_call(gpu_ctx, runs, name, dtype):
  case = ao.BY_NAME[name]
  whole = runs(case, dtype)
  dev = Dev(case, dtype)
  try:
    same_outputs(dev.maximize(), whole)                                   # a repeated call
    for k in (0, 4, 8):                                                   # the same start alone
      log, x, val, status, state = dev.maximize(x0=np.ascontiguousarray(dev.x0[k:k + 1]))
      assert same_bits(log[:, 0], np.ascontiguousarray(whole[0][:, k])) and same_bits(x[0], whole[1][k]) and val[0] == whole[2][k]
      assert status[0] == whole[3][k] and same_bits(state[0], whole[4][k])
    # segments of 5 evaluations against one of 128 (the last segment takes the remaining 3)
    state, logs = np.zeros((case.R, dev.ns)), []
    for e0 in range(0, EVALS, 5):
      log, x, val, status, state = dev.maximize(evals=min(5, EVALS - e0), state=state)
      logs.append(log)
    same_outputs((np.concatenate(logs), x, val, status, state), whole)
    # and without the poisoned scratch
    dev.ctx.set_option('poison', 0)
    try:
      same_outputs(dev.maximize(), whole)
    finally:
      dev.ctx.set_option('poison', 1)
    assert np.array_equal(dev.maximize(want_log=False)[1], whole[1])      # the log is optional
  finally:
    dev.close()


def test_corners_and_caller_bounds(gpu_ctx, runs):
  for case in ao.CASES:
    if case.kind == 'corner':
      for dtype in (np.float64, np.float32):
        x = runs(case, dtype)[1]
        assert np.all((x == 0.0) | (x == 1.0)), (case.name, x)
  # caller bounds, and a start on a bound: every component the oracle-driven run leaves on a face is on that face exactly, every other
  # component strictly inside (fp64: the same decisions; fp32 may take others, and is held to the box)
  for name in ('box-matern32-ei', 'bound-matern52-ucb'):
    case = ao.BY_NAME[name]
    lo, hi = ao.inputs(case).lo, ao.inputs(case).hi
    x = runs(case)[1]
    on_face = 0
    for k in range(case.R):
      ref = ao.oracle_run(case, k).x
      assert np.array_equal(x[k] == lo, ref == lo) and np.array_equal(x[k] == hi, ref == hi), (name, k, x[k], ref)
      assert np.all(x[k] >= lo) and np.all(x[k] <= hi)
      on_face += int(np.sum((ref == lo) | (ref == hi)))
    assert on_face > 0, name                                               # the case has active bounds to hit
    x32, val32 = runs(case, np.float32)[1:3]
    assert np.all(x32 >= lo) and np.all(x32 <= hi) and np.all(np.isfinite(val32))


def test_refusals_come_before_any_device_work(gpu_ctx):
  nv = _nv()
  nat = nv.nat
  import helpers
  err = lambda: (nat.lib().hbo_last_error(gpu_ctx.handle) or b'').decode()
  base = ao.BY_NAME['squared_exponential-zero-pi-n7-D3-S5-R1']
  dev = Dev(base)
  extra = []
  try:
    def refused(code, text, **kw):
      kw.setdefault('state', np.zeros((1, dev.ns)))
      before = kw['state'].copy()
      rc, x, val, status = dev.maximize(rc_only=True, **kw)
      assert rc == code and text in err(), (rc, err())
      assert np.all(x == 7.0) and np.all(val == 7.0) and np.all(status == 7)
      assert np.array_equal(kw['state'], before)                          # a fresh state is not started by a call that fails
    refused(nat.HBO_ERR_ARG, '1 <= R', r=0)
    refused(nat.HBO_ERR_ARG, 'outside the box', x0=np.array([[0.5, 1.5, 0.5]]))
    refused(nat.HBO_ERR_ARG, 'outside the box', x0=np.array([[0.5, np.nan, 0.5]]))
    refused(nat.HBO_ERR_ARG, '1 <= evals', evals=0)
    dev.opts.tau = 1.0
    refused(nat.HBO_ERR_ARG, 'opts.tau')
    dev.opts.tau = 0.5
    refused(nat.HBO_ERR_ARG, 'state is neither', state=np.full((1, dev.ns), 2.0))
    dev.lo, dev.hi = np.array([0.0, 0.6, 0.0]), np.array([1.0, 0.4, 1.0])
    refused(nat.HBO_ERR_ARG, 'lo <= hi')
    dev.lo = dev.hi = None
    rng = np.random.default_rng(5)
    wf = nv.utils.DEFAULT_WARP_FUNC

    def swap(kn, mn, model, n, config=None):
      x, y = helpers.synthetic_task(rng, n, 3)
      pn = nv.defs.GPParams(model=model, config=config or {})
      h = nv.linalg.factor(mn, kn, pn, x, y, wf)
      extra.append(h)
      bm = nv.hmodel.BuiltModel(mn, kn, pn, wf, np.float64, 3)
      extra.append(bm)
      dev.structs = (nat.Model * 1)(bm.struct)
      dev.caches = (nat.C.c_void_p * 1)(h.handle)
      dev.built = [bm]
    plain = helpers.make_model(rng, 'constant', False, 3)
    swap(nv.kernel.matern52, nv.mean.constant, plain, 129)
    refused(nat.HBO_ERR_UNSUPPORTED, 'n > 128')
    swap(nv.kernel.matern52_mlp, nv.mean.constant, helpers.make_model(rng, 'constant', True, 3), 30, {'mlp_features': helpers.MLP_FEATURES})
    refused(nat.HBO_ERR_UNSUPPORTED, 'MLP basis')
    km = dict(plain); km['kumar_params'] = {'a': np.full(3, 0.3), 'b': np.full(3, -0.2)}
    swap(nv.kernel.matern52_kumar, nv.mean.constant, km, 30)
    refused(nat.HBO_ERR_UNSUPPORTED, 'Kumaraswamy')
  finally:
    dev.close()
    for h in extra:
      if hasattr(h, 'close'):
        h.close()


def _bo_model(nv, hgp, seed=83):
  import helpers
  rng = np.random.default_rng(seed)
  d = 2
  f = lambda xx: -np.sum((np.atleast_2d(xx) - 0.3)**2, axis=1, keepdims=True)
  x = rng.uniform(size=(6, d))
  x2, y2 = helpers.synthetic_task(rng, 20, d)
  ds = {'test': nv.defs.SubDataset(x, f(x)), 'other': nv.defs.SubDataset(x2, y2), 'third': nv.defs.SubDataset(x2[:5], y2[:5])}
  samples = [helpers.make_model(np.random.default_rng(seed * 100 + i), 'constant', False, d) for i in range(5)]
  wf = nv.utils.DEFAULT_WARP_FUNC
  if hgp:
    return nv.gp.HGP(ds, nv.mean.constant, nv.kernel.matern52, nv.defs.GPParams(model=samples[0], samples=samples, config={}), wf), f
  return nv.gp.GP(ds, nv.mean.constant, nv.kernel.matern52, nv.defs.GPParams(model=samples[0], config={}), wf), f


@pytest.mark.parametrize('hgp', [True, False], ids=['hgp-S5', 'gp'])
def test_maximize_and_bayesopt_on_the_device(gpu_ctx, monkeypatch, hgp):
  import scipy.optimize
  nv = _nv()
  ac = nv.acfun.ucb
  spied = []
  real = scipy.optimize.minimize
  monkeypatch.setattr(scipy.optimize, 'minimize', lambda *a, **k: (spied.append(1), real(*a, **k))[1])
  winners = {}
  for starts in (1, 4):
    model, f = _bo_model(nv, hgp)
    model.params.config.update(acq_opt_on_device=True, acq_opt_starts=starts)
    seen = {}

    def sampler(key, dim):
      seen['cand'] = key.uniform(size=(16, dim))
      return seen['cand']

    def oracle(x):
      # the model is still the one the point was chosen on: the chosen point against the best candidate, both through ac_func
      vals = ac(model=model, sub_dataset_key='test', x_queries=np.vstack([x, seen['cand']]))
      assert np.all(x >= 0.0) and np.all(x <= 1.0)
      assert vals[0, 0] >= np.max(vals[1:, 0]), (vals[0, 0], np.max(vals[1:, 0]))
      winners.setdefault(starts, []).append(float(vals[0, 0]))
      return f(x)
    try:
      out = nv.bayesopt.bayesopt(7, model, 'test', oracle, ac, iters=3, input_sampler=sampler)
      assert out.x.shape == (9, 2) and np.all(out.x >= 0.0) and np.all(out.x <= 1.0)
      # one more maximisation, looked at closely
      cand = np.random.default_rng(9).uniform(size=(4, 2))
      xb, vb, info = ac.maximize(model=model, sub_dataset_key='test', x_init=cand, opts={'log': True, 'segment': 16})
      assert xb.shape == (2,) and xb.dtype == np.float64 and info['x'].shape == (4, 2) and info['log'].shape[1] == 4
      assert not np.any(info['status'] == nv.nat.ACQ_OPT_RUNNING) and info['log'].shape[0] % 16 == 0
      best = int(np.argmax(info['value']))
      assert np.array_equal(xb, info['x'][best]) and vb == info['value'][best]
      again = ac(model=model, sub_dataset_key='test', x_queries=info['x'])[:, 0]
      np.testing.assert_allclose(info['value'], again, rtol=1e-9, atol=1e-11)
      if hgp:
        assert model.params.model is model.get_model_params_samples()[-1]
    finally:
      if hgp:
        nv.acfun.drop_sample_caches(model)
  assert spied == []                                      # the sub-dataset had observations from the first iteration on
  # the same seed gives both runs the same first iteration: four starts cannot end below one
  assert winners[4][0] >= winners[1][0]
