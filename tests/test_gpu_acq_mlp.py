"""hbo_acq_grad_samples_mlp, hbo_acq_maximize_mlp and config['acq_mlp'] on the device (run with `-m gpu` on an MI355X): the acquisition
gradient over parameter samples and the device maximiser for kernels on an MLP basis and the linear_mlp mean (csrc/acq_mlp.h inside
csrc/acq_small.hip and csrc/acq_blocked.hip).  Cases, references, bounds and mutants: tests/acq_mlp_cases.py, judged on its own by
tests/test_acq_mlp_cases_host.py.  The session runs under `hbo_tune poison` (conftest.py).

  1  every case and acquisition per query against the oracle with the bounds of acq_grad_cases (groups S - V: one launch; L: blocked)
  2  force_blocked on U and chunk_queries 1 and 7 on L: the same bounds, the same bits across the chunkings, val64 rounds to acq_out
  3  S = 3: row s of the joint call is the S = 1 call of sample s to the bit; samples permuted, queries reversed, a repeated call,
     and the same without poison
  4  models without any MLP: the _mlp entry points are the _blocked ones byte for byte
  5  refusals before any device work; an MLP model now returns HBO_OK (the symbol does not exist before this feature)
  6  the maximiser: the device loop is the host-driven loop (hbo_probe_acq_grad_samples_mlp64 feeding hbo_probe_acq_opt_ctl) to the
     bit, the decisions of the oracle-driven restatement, a run cut into calls of 5 evaluations, a start alone
  7  acfun.value_and_grad / maximize and bayesopt() with config['acq_mlp']

DEV_X_TOL, DEV_VALUE_TOL, FP32_VALUE_TOL: 10 x the largest deviation of the device maximiser from the oracle-driven restatement measured
on an MI355X over OPT_CASES and their starts (|dx|_inf 1.093e-12, value 3.897e-14, fp32 value 1.068e-5; `python -m pytest
tests/test_gpu_acq_mlp.py -m gpu -s` prints every case's figures; profiles/acq_mlp.md has them), the convention of
tests/test_gpu_acq_opt.py.  The figures of the models without an MLP are 5.0e-12, 3.0e-14 and 1.2e-5: none of these is above its
counterpart by more than a factor of 1.3."""
import ctypes as C
import types

import numpy as np
import pytest

import acq_grad_cases as G
import acq_mlp_cases as A
import acq_opt_oracle as ao
import helpers

pytestmark = pytest.mark.gpu
# S-matern52_mlp+linear_mlp-...-f12x33-fp64-ei-S1-R3; S-matern52_mlp+linear-...-f12x33-fp64-pi-S1-R3; L-matern52_mlp+linear_mlp-...-n129-...-pi-S1-R3
DEV_X_MEASURED, DEV_VALUE_MEASURED, FP32_VALUE_MEASURED = 1.093e-12, 3.897e-14, 1.068e-5
DEV_X_TOL, DEV_VALUE_TOL, FP32_VALUE_TOL = 10 * DEV_X_MEASURED, 10 * DEV_VALUE_MEASURED, 10 * FP32_VALUE_MEASURED
SCALE = G.SCALE
PD = C.POINTER(C.c_double)
EVALS = ao.MAX_EVALS


def _nv():
  from hyperbo_amd import _model as hmodel
  from hyperbo_amd import _native as nat
  from hyperbo_amd.basics import definitions as defs, linalg
  from hyperbo_amd.bo_utils import acfun, bayesopt
  from hyperbo_amd.gp_utils import gp, kernel, mean, utils
  return types.SimpleNamespace(hmodel=hmodel, nat=nat, defs=defs, linalg=linalg, acfun=acfun, bayesopt=bayesopt, gp=gp, kernel=kernel, mean=mean,
                               utils=utils)


def same_bits(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Samples:
  """The first `count` parameter samples of a case (acq_mlp_cases.sample_models) factorised on the device, and the calls the tests make
  on them.  Close it."""

  def __init__(self, ctx, case, count=1, dtype=None):
    nv = self.nv = _nv()
    self.ctx, self.case, self.d = ctx, case, case.d
    self.dtype = np.dtype(case.np_dtype if dtype is None else dtype)
    kn, mn, wf = getattr(nv.kernel, case.kernel_name), getattr(nv.mean, case.mname), nv.utils.DEFAULT_WARP_FUNC
    _, x, y, _ = G.inputs(case)
    x, y = x.astype(self.dtype), y.astype(self.dtype)
    self.handles, self.built, self.noises = [], [], []
    for i in range(count):
      pn = nv.defs.GPParams(model=G.cast(A.sample_models(case)[i], self.dtype), config=G.config(case))
      self.handles.append(nv.linalg.factor(mn, kn, pn, x, y, wf, ctx=ctx))
      self.built.append(nv.hmodel.BuiltModel(mn, kn, pn, wf, self.dtype, case.d))
      self.noises.append(A.sample_setup(case, i).noise if self.dtype == case.np_dtype else ao.noise_of(G.cast(A.sample_models(case)[i], self.dtype)))

  def close(self):
    for h in self.handles:
      h.close()

  def args(self, sel, params):
    nat = self.nv.nat
    s = len(sel)
    return ((nat.Model * s)(*[self.built[i].struct for i in sel]), (C.c_void_p * s)(*[self.handles[i].handle for i in sel]),
            (C.c_double * s)(*[float(params[i]) for i in sel]), (C.c_double * s)(*[float(self.noises[i]) for i in sel]))

  def call(self, acq_id, params, xq, sel=None, entry='hbo_acq_grad_samples_mlp', rc_only=False, fill=np.nan):
    """A public entry point: (values [S, M] in the model dtype, gradients [S, M, D])."""
    nat = self.nv.nat
    sel = list(range(len(self.built))) if sel is None else list(sel)
    structs, caches, prm, nse = self.args(sel, params)
    m = xq.shape[0]
    val, grad = np.full((len(sel), m), fill, dtype=self.dtype), np.full((len(sel), m, self.d), fill)
    rc = getattr(nat.lib(), entry)(self.ctx.handle, structs, len(sel), caches, nat.ptr(xq), m, acq_id, prm, nse, SCALE, nat.ptr(val),
                                   grad.ctypes.data_as(PD))
    if rc_only:
      return rc, val, grad
    self.ctx.check(rc, allow_not_pd=False)
    return val, grad

  def probe(self, acq_id, params, xq, sel=None, force=0, chunk=0):
    """hbo_probe_acq_grad_samples_mlp64: (values, gradients, fp64 values [S, M])."""
    nat = self.nv.nat
    sel = list(range(len(self.built))) if sel is None else list(sel)
    structs, caches, prm, nse = self.args(sel, params)
    m = xq.shape[0]
    val, grad, v64 = np.full((len(sel), m), np.nan, dtype=self.dtype), np.full((len(sel), m, self.d), np.nan), np.full((len(sel), m), np.nan)
    self.ctx.check(nat.lib().hbo_probe_acq_grad_samples_mlp64(self.ctx.handle, structs, len(sel), caches, nat.ptr(xq), m, acq_id, prm, nse, SCALE,
                                                              nat.ptr(val), grad.ctypes.data_as(PD), force, chunk, v64.ctypes.data_as(PD)),
                   allow_not_pd=False)
    return val, grad, v64


def _judge(case, acq, ref, val, grad, what):
  rv, rg = G.ratios(case, acq, ref, val, grad)
  print(f'\nacq mlp: {case.id} {what} {acq}: worst ratio to the oracle bounds: value {np.max(rv):.3e}, '
        f'gradient {np.max(np.where(np.isnan(rg), -1.0, rg)):.3e}')
  assert np.all(rv <= 1.0) and not np.any(rg > 1.0), (what, acq, rv, rg)


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', A.CASES, ids=lambda c: c.id)
def test_against_the_oracle_per_query(gpu_ctx, case):
  """Worst ratios per group: profiles/acq_mlp_errors.md."""
  ref, xq = G.reference(case), G.inputs(case)[3]
  dev = Samples(gpu_ctx, case)
  try:
    for acq in G.ACQS:
      val, grad = dev.call(G.ACQ_IDS[acq], [G.acq_param(acq, ref)], xq)
      assert val.dtype == case.np_dtype and grad.dtype == np.float64 and val.shape == (1, case.M) and grad.shape == (1, case.M, case.d)
      _judge(case, acq, ref, val[0], grad[0], 'entry')
  finally:
    dev.close()


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', A.CASES_U + A.CASES_L, ids=lambda c: c.id)
def test_forced_blocking_and_chunking(gpu_ctx, case):
  ref, xq = G.reference(case), G.inputs(case)[3]
  dev = Samples(gpu_ctx, case)
  try:
    for acq in G.ACQS:
      prm = [G.acq_param(acq, ref)]
      base = dev.probe(G.ACQ_IDS[acq], prm, xq, force=1)
      _judge(case, acq, ref, base[0][0], base[1][0], 'force_blocked')
      assert same_bits(base[2].astype(case.np_dtype), base[0])
      if case.n > 128:
        pub = dev.call(G.ACQ_IDS[acq], prm, xq)
        assert same_bits(pub[0], base[0]) and same_bits(pub[1], base[1])      # the public entry point is the hook's launches
      for chunk in (1, 7):
        got = dev.probe(G.ACQ_IDS[acq], prm, xq, force=1, chunk=chunk)
        assert all(same_bits(a, b) for a, b in zip(got, base)), (acq, chunk)
  finally:
    dev.close()


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', A.MULTI, ids=lambda c: c.id)
def test_a_row_does_not_depend_on_what_shares_the_call(gpu_ctx, case):
  ref0, xq = G.reference(case), G.inputs(case)[3]
  dev = Samples(gpu_ctx, case, A.N_SAMPLES)
  try:
    for acq in G.ACQS:
      p = G.acq_param(acq, ref0)
      prm, aid = [p] * A.N_SAMPLES, G.ACQ_IDS[acq]

      def check():
        val, grad, v64 = dev.probe(aid, prm, xq)
        assert np.isfinite(val).all() and np.isfinite(grad).all() and same_bits(v64.astype(case.np_dtype), val)
        again = dev.probe(aid, prm, xq)
        assert all(same_bits(a, b) for a, b in zip(again, (val, grad, v64)))                   # identical calls, identical bits
        for s in range(A.N_SAMPLES):                                                           # a sample alone
          v1, g1, w1 = dev.probe(aid, prm, xq, sel=[s])
          assert same_bits(v1[0], val[s]) and same_bits(g1[0], grad[s]) and same_bits(w1[0], v64[s]), s
        v2, g2, _ = dev.probe(aid, prm, xq, sel=[2, 0, 1])                                     # permuted
        assert same_bits(v2[0], val[2]) and same_bits(g2[0], grad[2]) and same_bits(v2[1], val[0]) and same_bits(g2[1], grad[0])
        assert same_bits(v2[2], val[1]) and same_bits(g2[2], grad[1])
        vr, gr, _ = dev.probe(aid, prm, np.ascontiguousarray(xq[::-1]))                        # the queries reversed
        assert same_bits(vr[:, ::-1], val) and same_bits(gr[:, ::-1], grad)
        return val, grad, v64
      val, grad, v64 = check()
      for s in range(A.N_SAMPLES):                                                             # every sample against its own reference
        _judge(case, acq, A.sample_reference(case, s, acq, p), val[s], grad[s], f'sample {s}')
      gpu_ctx.set_option('poison', 0)
      try:
        plain = check()
        assert all(same_bits(a, b) for a, b in zip(plain, (val, grad, v64)))
      finally:
        gpu_ctx.set_option('poison', 1)
  finally:
    dev.close()


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------
PLAIN = [next(c for c in G.CASES_D if c.n == 65 and c.M == 9 and c.kname == 'matern52' and c.dtype == 'fp64'),
         next(c for c in G.CASES_A if c.d == 5 and c.kname == 'matern52' and c.ls == 'ard' and c.dtype == 'fp32'),
         next(c for c in G.CASES_A if c.d == 5 and c.kname == 'dot_product' and c.dtype == 'fp64')]


class PlainSamples(Samples):
  """One sample of an acq_grad_cases case without any MLP."""

  def __init__(self, ctx, case):
    nv = self.nv = _nv()
    self.ctx, self.case, self.d, self.dtype = ctx, case, case.d, np.dtype(case.np_dtype)
    kn, mn, wf = getattr(nv.kernel, case.kernel_name), getattr(nv.mean, case.mname), nv.utils.DEFAULT_WARP_FUNC
    model, x, y, _ = G.inputs(case)
    pn = nv.defs.GPParams(model=model, config={})
    self.handles = [nv.linalg.factor(mn, kn, pn, x, y, wf, ctx=ctx)]
    self.built = [nv.hmodel.BuiltModel(mn, kn, pn, wf, self.dtype, case.d)]
    self.noises = [G.oracle_setup(case).noise]


def _maximize(dev, entry, acq_id, params, x0, evals=EVALS, state=None, sel=None, opts=None):
  """One call of a maximiser entry point: (log [evals, R], x_out, val_out, status, state)."""
  nat = dev.nv.nat
  sel = list(range(len(dev.built))) if sel is None else list(sel)
  structs, caches, prm, nse = dev.args(sel, params)
  opts = nat.AcqOptOpts(**ao.DEFAULTS) if opts is None else opts
  ns = nat.lib().hbo_acq_opt_state_doubles(dev.d, opts.memory)
  rows = x0.shape[0]
  state = np.zeros((rows, ns)) if state is None else state
  x, val, status = np.full((rows, dev.d), 7.0), np.full(rows, 7.0), np.full(rows, 7, dtype=np.int32)
  log = np.zeros((evals, rows), dtype=nat.ACQ_OPT_EVAL_DTYPE)
  dev.ctx.check(getattr(nat.lib(), entry)(dev.ctx.handle, structs, len(sel), caches, nat.ptr(x0), rows, None, None, acq_id, prm, nse, SCALE,
                                          C.byref(opts), nat.ptr(state), evals, nat.ptr(x), nat.ptr(val), nat.ptr(status), nat.ptr(log)),
                allow_not_pd=False)
  return log, x, val, status, state


def same_outputs(got, want):
  for g, w, what in zip(got, want, ('log', 'x_out', 'val_out', 'status', 'state')):
    assert same_bits(g, w), what


@pytest.mark.parametrize('case', PLAIN, ids=lambda c: c.id)
def test_models_without_an_mlp_take_the_blocked_entry_points(gpu_ctx, case):
  ref, xq = G.reference(case), G.inputs(case)[3]
  dev = PlainSamples(gpu_ctx, case)
  try:
    for acq in G.ACQS:
      prm = [G.acq_param(acq, ref)]
      new, old = dev.call(G.ACQ_IDS[acq], prm, xq), dev.call(G.ACQ_IDS[acq], prm, xq, entry='hbo_acq_grad_samples_blocked')
      assert same_bits(new[0], old[0]) and same_bits(new[1], old[1]) and np.isfinite(new[1]).all()
      x0 = np.ascontiguousarray(xq[:3])
      same_outputs(_maximize(dev, 'hbo_acq_maximize_mlp', G.ACQ_IDS[acq], prm, x0, evals=24),
                   _maximize(dev, 'hbo_acq_maximize_blocked', G.ACQ_IDS[acq], prm, x0, evals=24))
  finally:
    dev.close()


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_no_output_and_an_mlp_model_is_served(gpu_ctx):
  nv = _nv()
  nat = nv.nat
  rng = np.random.default_rng(193)
  d = 3
  wf = nv.utils.DEFAULT_WARP_FUNC
  xq = rng.uniform(size=(2, d))
  err = lambda: (nat.lib().hbo_last_error(gpu_ctx.handle) or b'').decode()

  def call(built, handles, entry='hbo_acq_grad_samples_mlp'):
    S = len(built)
    structs = (nat.Model * S)(*[b.struct for b in built])
    caches = (C.c_void_p * S)(*[h.handle if h is not None else None for h in handles])
    prm, nse = (C.c_double * S)(*([3.0] * S)), (C.c_double * S)(*([0.1] * S))
    val, grad = np.full((S, 2, 1), 7.0), np.full((S, 2, d), 7.0)
    rc = getattr(nat.lib(), entry)(gpu_ctx.handle, structs, S, caches, nat.ptr(xq), 2, 2, prm, nse, SCALE, nat.ptr(val), grad.ctypes.data_as(PD))
    if rc != nat.HBO_OK:
      assert np.all(val == 7.0) and np.all(grad == 7.0)
    else:
      assert np.isfinite(val).all() and np.isfinite(grad).all()
    return rc, err()

  def one(kn, mn, model, n, feats=helpers.MLP_FEATURES):
    x, y = helpers.synthetic_task(rng, n, d)
    pn = nv.defs.GPParams(model=model, config={'mlp_features': feats})
    return nv.hmodel.BuiltModel(mn, kn, pn, wf, np.float64, d), nv.linalg.factor(mn, kn, pn, x, y, wf)

  handles = []
  try:
    b_mlp, h_mlp = one(nv.kernel.matern52_mlp, nv.mean.linear_mlp, helpers.make_model(rng, 'linear_mlp', True, d), 130); handles.append(h_mlp)
    rc, msg = call([b_mlp], [h_mlp]); assert rc == nat.HBO_OK, (rc, msg)                                  # served here ...
    rc, msg = call([b_mlp], [h_mlp], 'hbo_acq_grad_samples_blocked'); assert rc == nat.HBO_ERR_UNSUPPORTED and 'MLP basis' in msg, (rc, msg)
    b40, h40 = one(nv.kernel.matern52_mlp, nv.mean.linear_mlp, helpers.make_model(rng, 'linear_mlp', True, d), 40); handles.append(h40)
    rc, msg = call([b40], [h40]); assert rc == nat.HBO_OK, (rc, msg)
    rc, msg = call([b40], [h40], 'hbo_acq_grad_samples'); assert rc == nat.HBO_ERR_UNSUPPORTED and 'MLP basis' in msg, (rc, msg)   # ... and only here
    rc, msg = call([b_mlp], [None]); assert rc == nat.HBO_ERR_UNSUPPORTED and 'prior branch' in msg and 'hbo_acq_grad' in msg, (rc, msg)
    plain = helpers.make_model(rng, 'constant', False, d)
    km = dict(plain); km['kumar_params'] = {'a': np.full(d, 0.3), 'b': np.full(d, -0.2)}
    b, h = one(nv.kernel.matern52_kumar, nv.mean.constant, km, 130); handles.append(h)
    rc, msg = call([b], [h]); assert rc == nat.HBO_ERR_UNSUPPORTED and 'Kumaraswamy' in msg and 'evaluate the samples with hbo_acq_grad' in msg, (rc, msg)
    # another architecture across the samples
    m2 = helpers.make_model(rng, 'linear_mlp', True, d)
    fin = d
    for l, f in enumerate((6, helpers.MLP_FEATURES[-1])):
      m2['mlp_params'][f'Dense_{l}'] = {'kernel': rng.normal(size=(fin, f)) * 0.7, 'bias': rng.normal(size=f) * 0.1}
      fin = f
    b2, h2 = one(nv.kernel.matern52_mlp, nv.mean.linear_mlp, m2, 130, feats=(6, helpers.MLP_FEATURES[-1])); handles.append(h2)
    rc, msg = call([b_mlp, b2], [h_mlp, h2]); assert rc == nat.HBO_ERR_ARG and 'must share' in msg, (rc, msg)
    # the maximiser: the same refusals, the same service
    opts = nat.AcqOptOpts(**ao.DEFAULTS)
    ns = nat.lib().hbo_acq_opt_state_doubles(d, opts.memory)

    def mx(built, handle, entry):
      structs = (nat.Model * 1)(built.struct)
      caches = (C.c_void_p * 1)(handle.handle if handle is not None else None)
      prm, nse = (C.c_double * 1)(3.0), (C.c_double * 1)(0.1)
      state, x, val, status = np.zeros((1, ns)), np.full((1, d), 7.0), np.full(1, 7.0), np.full(1, 7, dtype=np.int32)
      x0 = np.full((1, d), 0.5)
      rc = getattr(nat.lib(), entry)(gpu_ctx.handle, structs, 1, caches, nat.ptr(x0), 1, None, None, 2, prm, nse, SCALE, C.byref(opts), nat.ptr(state), 3,
                                     nat.ptr(x), nat.ptr(val), nat.ptr(status), None)
      if rc != nat.HBO_OK:
        assert np.all(x == 7.0) and np.all(val == 7.0) and np.all(status == 7) and not state.any()
      return rc, err()
    rc, msg = mx(b_mlp, h_mlp, 'hbo_acq_maximize_mlp'); assert rc == nat.HBO_OK, (rc, msg)
    rc, msg = mx(b_mlp, h_mlp, 'hbo_acq_maximize_blocked'); assert rc == nat.HBO_ERR_UNSUPPORTED and 'MLP basis' in msg, (rc, msg)
    rc, msg = mx(b_mlp, None, 'hbo_acq_maximize_mlp'); assert rc == nat.HBO_ERR_UNSUPPORTED and 'prior branch' in msg, (rc, msg)
    rc, msg = mx(b, h, 'hbo_acq_maximize_mlp'); assert rc == nat.HBO_ERR_UNSUPPORTED and 'Kumaraswamy' in msg, (rc, msg)
  finally:
    for h in handles:
      h.close()


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------
class OptDev:
  """The samples of an OptCase in a dtype, and its runs."""

  def __init__(self, ctx, oc, dtype):
    self.oc, self.dtype = oc, np.dtype(dtype)
    self.dev = Samples(ctx, oc.case, oc.S, dtype)
    self.nat = self.dev.nv.nat
    self.prm = [float(self.dtype.type(A.opt_param(oc)))] * oc.S
    self.x0 = np.ascontiguousarray(A.opt_x0(oc), dtype=dtype)
    self.acq_id = G.ACQ_IDS[oc.acq]

  def close(self):
    self.dev.close()

  def maximize(self, x0=None, evals=EVALS, state=None):
    return _maximize(self.dev, 'hbo_acq_maximize_mlp', self.acq_id, self.prm, self.x0 if x0 is None else x0, evals, state)

  def host_driven(self, evals=EVALS):
    """The same run as a Python loop: the gradient hook on the pending points, the control hook once per start."""
    nat = self.nat
    r, d = self.x0.shape
    opts = nat.AcqOptOpts(**ao.DEFAULTS)
    state = np.zeros((r, nat.lib().hbo_acq_opt_state_doubles(d, opts.memory)))
    log = np.zeros((evals, r), dtype=nat.ACQ_OPT_EVAL_DTYPE)
    pending = self.x0.copy()
    x, status = np.zeros((r, d)), np.zeros(r, dtype=np.int32)
    ev, st, x_next, x_iter = nat.AcqOptEval(), C.c_int32(0), np.zeros(d), np.zeros(d)
    for e in range(evals):
      _, grads, v64 = self.dev.probe(self.acq_id, self.prm, pending)
      for k in range(r):
        start = np.ascontiguousarray(pending[k], dtype=np.float64)
        rc = nat.lib().hbo_probe_acq_opt_ctl(nat.ptr(state[k]), d, nat.dtype_code(self.dtype), C.byref(opts), None, None,
                                             nat.ptr(start), nat.ptr(np.ascontiguousarray(v64[:, k])), nat.ptr(np.ascontiguousarray(grads[:, k])),
                                             self.oc.S, nat.ptr(x_next), nat.ptr(x_iter), C.byref(ev), C.byref(st))
        assert rc == nat.HBO_OK, (nat.lib().hbo_last_error(None) or b'').decode()
        log[e, k] = (ev.kind, ev.iter, ev.alpha, ev.value)
        if ev.kind != nat.ACQ_OPT_IDLE:
          pending[k] = x_next
        x[k], status[k] = x_iter, st.value
    return log, x, -state[:, 5], status, state


@pytest.fixture(scope='module')
def runs(gpu_ctx):
  """One device run per case and dtype, shared by the tests below and not to be written to."""
  cache = {}

  def get(oc, dtype=np.float64):
    key = (oc.name, np.dtype(dtype).name)
    if key not in cache:
      dev = OptDev(gpu_ctx, oc, dtype)
      try:
        cache[key] = dev.maximize()
      finally:
        dev.close()
    return cache[key]
  return get


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['fp64', 'fp32'])
@pytest.mark.parametrize('oc', A.OPT_CASES, ids=[c.name for c in A.OPT_CASES])
def test_device_loop_is_the_host_driven_hook_to_the_bit(gpu_ctx, runs, oc, dtype):
  got = runs(oc, dtype)
  dev = OptDev(gpu_ctx, oc, dtype)
  try:
    same_outputs(got, dev.host_driven())
    log, x, val, status, _ = got
    assert np.all(log['kind'][0] == ao.START)
    assert np.array_equal(x, x.astype(dtype).astype(np.float64)) and np.all(x >= 0.0) and np.all(x <= 1.0)
    # one run cut into calls of 5 evaluations; a start alone
    state, logs = None, []
    for _ in range(0, EVALS - 3, 5):
      part = dev.maximize(evals=5, state=state)
      state = part[4]; logs.append(part[0])
    part = dev.maximize(evals=3, state=state); logs.append(part[0])
    same_outputs((np.concatenate(logs),) + part[1:], got)
    alone = dev.maximize(x0=np.ascontiguousarray(dev.x0[1:2]))
    for a, g in zip(alone, (log[:, 1:2], x[1:2], val[1:2], status[1:2], got[4][1:2])):
      assert same_bits(np.ascontiguousarray(a), np.ascontiguousarray(g))
  finally:
    dev.close()


def _kinds(log, k):
  kinds = [int(v) for v in log['kind'][:, k]]
  return kinds[:kinds.index(ao.IDLE)] if ao.IDLE in kinds else kinds


@pytest.mark.parametrize('oc', A.OPT_CASES, ids=[c.name for c in A.OPT_CASES])
def test_device_loop_against_the_oracle_driven_restatement(gpu_ctx, runs, oc):
  """Measured on an MI355X (`python -m pytest tests/test_gpu_acq_mlp.py -m gpu -s`): |x - x_oracle|_inf 1.093e-12 (EI, MLP kernel +
  linear_mlp, n = 100), value 3.897e-14 (PI, MLP kernel + linear, n = 100) and fp32 value 1.068e-5 (PI, n = 129) -> DEV_X_MEASURED,
  DEV_VALUE_MEASURED, FP32_VALUE_MEASURED; the bounds are 10 x these."""
  log, x, val, status, _ = runs(oc)
  _, _, val32, _, _ = runs(oc, np.float32)
  worst = [0.0, 0.0, 0.0]
  for k in range(oc.R):
    ref = A.opt_run(oc, k)
    assert _kinds(log, k) == [e[0] for e in ref.log], (k, _kinds(log, k), [e[0] for e in ref.log])
    n = len(ref.log)
    assert [int(v) for v in log['iter'][:n, k]] == [e[1] for e in ref.log] and status[k] == ref.status
    worst[0] = max(worst[0], float(np.max(np.abs(x[k] - ref.x))))
    worst[1] = max(worst[1], abs(val[k] + ref.f) / max(1.0, abs(ref.f)))
    worst[2] = max(worst[2], abs(val32[k] + ref.f) / max(1.0, abs(ref.f)))
  print(f'\nacq mlp device vs oracle: {oc.name}: |dx|_inf {worst[0]:.3e}, value {worst[1]:.3e}, fp32 value {worst[2]:.3e}')
  assert worst[0] <= DEV_X_TOL and worst[1] <= DEV_VALUE_TOL and worst[2] <= FP32_VALUE_TOL, worst


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------
def _py_case():
  return next(c for c in A.CASES_S if c.feats == (12, 33) and (c.mlp_k, c.mname) == A.FULL and c.dtype == 'fp64')


def _py_model(nv, case, hgp, config):
  model, x, y, _ = G.inputs(case)
  rng = np.random.default_rng(195)
  x2, y2 = helpers.synthetic_task(rng, 20, case.d)
  ds = {'test': nv.defs.SubDataset(x, y), 'other': nv.defs.SubDataset(x2, y2), 'third': nv.defs.SubDataset(x2[:5], y2[:5])}
  cfg = dict(G.config(case)); cfg.update(config)
  kn, mn, wf = getattr(nv.kernel, case.kernel_name), getattr(nv.mean, case.mname), nv.utils.DEFAULT_WARP_FUNC
  if hgp:
    samples = A.sample_models(case)
    return nv.gp.HGP(ds, mn, kn, nv.defs.GPParams(model=samples[0], samples=list(samples), config=cfg), wf)
  return nv.gp.GP(ds, mn, kn, nv.defs.GPParams(model=model, config=cfg), wf)


def test_value_and_grad_and_maximize_with_the_config_key(gpu_ctx, monkeypatch):
  nv = _nv()
  nat = nv.nat
  case = _py_case()
  ref, xq = G.reference(case), G.inputs(case)[3]
  target = ref.target
  cb = lambda model, key, **kw: target
  counts = {'mlp': 0, 'single': 0}
  lib = nat.lib()
  for key, name in (('mlp', 'hbo_acq_grad_samples_mlp'), ('single', 'hbo_acq_grad')):
    real = getattr(lib, name)
    monkeypatch.setattr(lib, name, (lambda real, key: lambda *a: (counts.__setitem__(key, counts[key] + 1), real(*a))[1])(real, key))
  before = gpu_ctx.get_option('acq_fused')
  models = []
  try:
    gpu_ctx.set_option('acq_fused', 1)
    gp_on = _py_model(nv, case, False, {'acq_mlp': True}); models.append(gp_on)
    val, grad = nv.acfun.expected_improvement.value_and_grad(model=gp_on, sub_dataset_key='test', x_queries=xq, acfun_callback=cb)
    assert counts == {'mlp': 1, 'single': 0} and val.shape == (case.M, 1) and grad.shape == (case.M, case.d)
    _judge(case, 'ei', ref, val[:, 0], grad, 'GP value_and_grad')
    hgp_on = _py_model(nv, case, True, {'acq_mlp': True}); models.append(hgp_on)
    val, grad = nv.acfun.expected_improvement.value_and_grad(model=hgp_on, sub_dataset_key='test', x_queries=xq, acfun_callback=cb)
    assert counts == {'mlp': 2, 'single': 0}
    refs = [A.sample_reference(case, s, 'ei', target) for s in range(A.N_SAMPLES)]
    mean_ref = G.Ref(target, ref.mu, ref.sd, {'ei': np.mean([r.val['ei'] for r in refs], axis=0)}, {'ei': np.mean([r.grad['ei'] for r in refs], axis=0)},
                     {'ei': np.zeros(case.M)})      # (gamma 0: the tightest gradient bound)
    _judge(case, 'ei', mean_ref, val[:, 0], grad, 'HGP value_and_grad')
    # maximize: the best of the starts, no refusal
    x0 = np.ascontiguousarray(xq[:3])
    xb, vb, info = nv.acfun.expected_improvement.maximize(model=gp_on, sub_dataset_key='test', x_init=x0, acfun_callback=cb)
    assert np.isfinite(vb) and vb == np.max(info['value']) and np.array_equal(xb, info['x'][int(np.argmax(info['value']))])
    assert np.all(xb >= 0.0) and np.all(xb <= 1.0) and counts['single'] == 0
    v_at, _ = nv.acfun.expected_improvement.value_and_grad(model=gp_on, sub_dataset_key='test', x_queries=xb[None, :], acfun_callback=cb)
    assert abs(float(v_at[0, 0]) - vb) <= 1e-9 * max(1.0, abs(vb)) and vb >= float(np.max(ref.val['ei'][:3])) * (1.0 - 1e-7)
    # without the key: today's refusal and today's per-cache path
    gp_off = _py_model(nv, case, False, {}); models.append(gp_off)
    with pytest.raises(nat.HboError) as e:
      nv.acfun.expected_improvement.maximize(model=gp_off, sub_dataset_key='test', x_init=x0, acfun_callback=cb)
    assert e.value.code == nat.HBO_ERR_UNSUPPORTED and 'MLP basis' in str(e.value)
    nv.acfun.expected_improvement.value_and_grad(model=gp_off, sub_dataset_key='test', x_queries=xq, acfun_callback=cb)
    assert counts == {'mlp': counts['mlp'], 'single': 1}
  finally:
    gpu_ctx.set_option('acq_fused', before)
    for m in models:
      nv.acfun.drop_sample_caches(m)


def test_bayesopt_on_the_device_with_an_mlp_model(gpu_ctx, monkeypatch):
  import scipy.optimize
  nv = _nv()
  case = _py_case()
  spied = []
  real = scipy.optimize.minimize
  monkeypatch.setattr(scipy.optimize, 'minimize', lambda *a, **k: (spied.append(1), real(*a, **k))[1])
  f = lambda xx: -np.sum((np.atleast_2d(xx) - 0.3)**2, axis=1, keepdims=True)
  model = _py_model(nv, case, False, {'acq_mlp': True, 'acq_opt_on_device': True, 'acq_opt_starts': 2})
  sampler = lambda key, dim: key.uniform(size=(16, dim))
  out = nv.bayesopt.bayesopt(7, model, 'test', f, nv.acfun.ucb, iters=3, input_sampler=sampler)
  assert out.x.shape == (case.n + 3, case.d) and np.isfinite(out.y).all()
  assert np.all(out.x[case.n:] >= 0.0) and np.all(out.x[case.n:] <= 1.0) and spied == []
