"""Batch expected improvement on the device (run with `-m gpu` on an MI355X): hbo_qei_grad_samples, hbo_qei_maximize,
acfun.q_expected_improvement and bayesopt.bayesopt_batch.  Cases, references, bounds and mutants: tests/qei_cases.py, judged on its own
by tests/test_qei_cases_host.py.  Every comparison is per (sample, batch) pair and per gradient row, never max-norm over a call.  Each
test prints its worst ratio to its bound (-s); profiles/qei_errors.md keeps them.

Bounds (qei_cases.py): fp64 -- DEVICE_FACTOR = 8 times the constants the float64 restatement needs against the long-double reference,
in units of eps64 x the un-cancelled term scale x cond(C)^2; fp32 caches -- the project's fp32 figure, 2e-2 of the batch's largest
gradient component and of the value's term scale.  Every compared pair satisfies the smooth-region condition (qei_cases.admitted)."""
import ctypes as C
import types

import numpy as np
import pytest

import acq_opt_oracle as ao
import helpers
import logei_cases as lc
import qei_cases as qc

pytestmark = pytest.mark.gpu
PD = C.POINTER(C.c_double)
SCALE = qc.SCALE
LD = qc.LD


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


def _dp(a):
  return None if a is None else a.ctypes.data_as(PD)


class Dev:
  """The S (model, factorised cache) pairs of a qei_cases.problem on the device and the calls the tests make on them.  Close it."""

  def __init__(self, ctx, p):
    nv = self.nv = _nv()
    case = p.case
    self.ctx, self.p, self.d, self.dtype = ctx, p, case.d, p.dtype
    kn = getattr(nv.kernel, case.kname + ('_mlp' if getattr(case, 'mlp_k', False) else ''))
    mn, wf = getattr(nv.mean, case.mname), nv.utils.DEFAULT_WARP_FUNC
    feats = getattr(case, 'feats', ())
    self.handles, self.built = [], []
    for sm in p.smp:
      pn = nv.defs.GPParams(model=sm.model_t, config={'mlp_features': tuple(feats)} if feats else {})
      self.handles.append(nv.linalg.factor(mn, kn, pn, sm.x, sm.y, wf, ctx=ctx))
      self.built.append(nv.hmodel.BuiltModel(mn, kn, pn, wf, self.dtype, self.d))

  def close(self):
    for h in self.handles:
      h.close()

  def _args(self, sel, noises, targets):
    nat = self.nv.nat
    s = len(sel)
    return ((nat.Model * s)(*[self.built[i].struct for i in sel]), (C.c_void_p * s)(*[self.handles[i].handle for i in sel]),
            (C.c_double * s)(*[float(noises[i]) for i in sel]), (C.c_double * s)(*[float(targets[i]) for i in sel]))

  def grad(self, xb, z, targets=None, noises=None, sel=None, scale=SCALE, rc_only=False):
    """hbo_qei_grad_samples over the samples `sel`: (values [S, M], gradients [S, M, q, D]); rc_only: (rc, values, gradients)."""
    nat = self.nv.nat
    sel = list(range(len(self.built))) if sel is None else list(sel)
    structs, caches, nse, tg = self._args(sel, self.p.noises if noises is None else noises, self.p.targets if targets is None else targets)
    xb = np.ascontiguousarray(xb, dtype=self.dtype)
    z = np.ascontiguousarray(z, dtype=np.float64)
    m, q, _ = xb.shape
    val, grad = np.full((len(sel), m), 7.0), np.full((len(sel), m, q, self.d), 7.0)
    rc = nat.lib().hbo_qei_grad_samples(self.ctx.handle, structs, len(sel), caches, nat.ptr(xb), m, q, _dp(z), z.shape[0], tg, nse, float(scale),
                                        _dp(val), _dp(grad))
    if rc_only:
      return rc, val, grad
    self.ctx.check(rc, allow_not_pd=False)
    return val, grad

  def maximize(self, x0, z, lo, hi, evals, state=None, opts=None, sel=None, targets=None, noises=None, rc_only=False):
    """One hbo_qei_maximize call: (log [evals, R], x_out [R, q, D], val_out, status, state)."""
    nat = self.nv.nat
    o = nat.AcqOptOpts(**(opts or ao.DEFAULTS))
    sel = list(range(len(self.built))) if sel is None else list(sel)
    structs, caches, nse, tg = self._args(sel, self.p.noises if noises is None else noises, self.p.targets if targets is None else targets)
    x0 = np.ascontiguousarray(x0, dtype=self.dtype)
    z = np.ascontiguousarray(z, dtype=np.float64)
    r, q, _ = x0.shape
    ns = nat.lib().hbo_acq_opt_state_doubles(q * self.d, o.memory)
    state = np.zeros((r, ns)) if state is None else state
    x, val, status = np.full((r, q, self.d), 7.0), np.full(r, 7.0), np.full(r, 7, dtype=np.int32)
    log = np.zeros((evals, r), dtype=nat.ACQ_OPT_EVAL_DTYPE)
    rc = nat.lib().hbo_qei_maximize(self.ctx.handle, structs, len(sel), caches, nat.ptr(x0), r, q, nat.ptr(lo), nat.ptr(hi), _dp(z), z.shape[0], tg, nse,
                                    SCALE, C.byref(o), nat.ptr(state), evals, nat.ptr(x), nat.ptr(val), nat.ptr(status), nat.ptr(log))
    if rc_only:
      return rc, x, val, status, state
    self.ctx.check(rc, allow_not_pd=False)
    return log, x, val, status, state


# ---- value and gradient against the case module ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', qc.CASES, ids=[c.id for c in qc.CASES])
def test_value_and_gradient_per_pair_and_row(gpu_ctx, case):
  """One call over the S samples and M batches of the case; every (sample, batch) pair against its long-double reference: the value to
  its bound and every gradient row (point, coordinate) to its own.  A second identical call gives the same bits."""
  p = qc.problem(case)
  refs = qc.references(case)
  dev = Dev(gpu_ctx, p)
  try:
    val, grad = dev.grad(p.xb, p.z)
    again = dev.grad(p.xb, p.z)
    assert same_bits(val, again[0]) and same_bits(grad, again[1])
    worst = (0.0, 0.0)
    for s in range(case.S):
      for m in range(case.M):
        ref = refs[s][m]
        rv, rg = qc.device_ratios(val[s, m], grad[s, m], ref, p.dtype)
        worst = (max(worst[0], rv), max(worst[1], rg))
        print(f'\nqei: {case.id} s={s} m={m}: value {val[s, m]:.6e} (ratio {rv:.3e}), gradient ratio {rg:.3e}, cond(C) {ref.cond:.3g}')
        assert rv <= 1.0 and rg <= 1.0, (case.id, s, m, rv, rg, float(val[s, m]), float(ref.value))
    print(f'\nqei: {case.id}: worst ratio to the bound: value {worst[0]:.3e}, gradient {worst[1]:.3e}')
  finally:
    dev.close()


def test_a_pair_does_not_depend_on_what_shares_the_call(gpu_ctx):
  """M = 1 against M = 5 and S = 1 against S = 3, bit for bit; the pending smaller call after a larger one (the workspaces are re-used)."""
  c5 = next(c for c in qc.CASES if c.M == 5)
  p = qc.problem(c5)
  dev = Dev(gpu_ctx, p)
  try:
    val, grad = dev.grad(p.xb, p.z)
    for m in (0, 3, 4):
      v1, g1 = dev.grad(p.xb[m:m + 1], p.z)
      assert same_bits(v1[:, 0], val[:, m]) and same_bits(g1[:, 0], grad[:, m]), m
  finally:
    dev.close()
  c3 = next(c for c in qc.CASES if c.S == 3 and len(set(c.ns)) == 3 and c.q == 16)
  p3 = qc.problem(c3)
  dev3 = Dev(gpu_ctx, p3)
  try:
    small = lambda: dev3.grad(p3.xb[1:2, :5], p3.z[:7, :5], sel=[2])
    v1, g1 = small()
    val, grad = dev3.grad(p3.xb, p3.z)
    v2, g2 = small()                                            # a smaller call right after the larger one: the workspaces are re-used
    assert same_bits(v1, v2) and same_bits(g1, g2) and np.all(np.isfinite(g1))
    for s in range(3):
      v1, g1 = dev3.grad(p3.xb, p3.z, sel=[s])
      assert same_bits(v1[0], val[s]) and same_bits(g1[0], grad[s]), s
  finally:
    dev3.close()


# ---- the rules -----------------------------------------------------------------------------------------------------------------------
def test_targets_out_of_reach(gpu_ctx):
  """target = 1e300: no base sample improves, the value is 0 and every gradient component exactly 0.  target = -1e300: every base sample
  improves, so the weights sum to 1: the gradient is that of any target below every f_bj (the reference at min_b max_j f_bj - 1), to its
  bound, and the value is 1e300 to eps."""
  case = qc.CASES[2]
  p = qc.problem(case)
  dev = Dev(gpu_ctx, p)
  try:
    val, grad = dev.grad(p.xb, p.z, targets=[1e300] * case.S)
    assert np.all(val == 0.0) and np.all(grad == 0.0)
    val, grad = dev.grad(p.xb, p.z, targets=[-1e300] * case.S)
    worst = 0.0
    for s, sm in enumerate(p.smp):
      for m in range(case.M):
        f = qc.reference(sm, p.xb[m], p.z, 0.0, sm.add_noise, SCALE).f
        low = float(np.min(np.max(f, axis=1))) - 1.0
        ref = qc.reference(sm, p.xb[m], p.z, low, sm.add_noise, SCALE, LD)
        assert qc.admitted(sm, p.xb[m], p.z, low, sm.add_noise, SCALE, p.dtype, ref)[0]
        assert abs(float(np.sum(ref.mubar)) - 1.0) <= 1e-15
        rg = float(np.max(qc.ratio((grad[s, m].astype(LD) - ref.grad).astype(np.float64), qc.grad_bound(ref, p.dtype))))
        worst = max(worst, rg)
        assert rg <= 1.0 and abs(val[s, m] - 1e300) <= 4 * qc.EPS64 * 1e300, (s, m, rg, val[s, m])
    print(f'\nqei: every sample improves: worst gradient ratio {worst:.3e}')
  finally:
    dev.close()


def test_identical_batch_points(gpu_ctx):
  """Two identical batch points.  add_noise > 0: finite, and to the bounds of the reference, in which a Matern pair at zero distance
  contributes 0 -- with a base sample of zeros both points tie exactly and the weight goes to the LOWER index.  add_noise == 0: the
  factorisation of Sigma' meets a pivot that is not > 0: NaN for that pair only, HBO_OK, the other batch of the call intact.  The second
  pivot of two equal Matern points is p - (p / sqrt p)^2, whose sign is a matter of rounding; the case here is exact in any
  arithmetic: a dot-product kernel without bias and both points at the origin, so k(x, X), l and Sigma' are exactly 0."""
  tie = qc.tie_problem()
  dev = Dev(gpu_ctx, tie)
  try:
    sm = tie.smp[0]
    val, grad = dev.grad(tie.xb, tie.z, targets=tie.targets)
    ref = qc.reference(sm, tie.xb[0], tie.z, float(tie.targets[0]), sm.add_noise, SCALE, LD)
    rv, rg = qc.device_ratios(val[0, 0], grad[0, 0], ref, tie.dtype)
    print(f'\nqei: tie: value ratio {rv:.3e}, gradient ratio {rg:.3e}; mubar {ref.mubar.astype(float).tolist()}')
    assert np.all(np.isfinite(grad)) and rv <= 1.0 and rg <= 1.0
    hi = qc.reference(sm, tie.xb[0], tie.z, float(tie.targets[0]), sm.add_noise, SCALE, LD, 'highest_index')
    assert max(qc.device_ratios(val[0, 0], grad[0, 0], types.SimpleNamespace(**{**vars(ref), 'grad': hi.grad, 'value': hi.value}), tie.dtype)) > 1.0
  finally:
    dev.close()
  nv = _nv()
  nat = nv.nat
  rng = np.random.default_rng(4)
  pn = nv.defs.GPParams(model={'dot_prod_sigma': np.array(1.0), 'dot_prod_bias': np.array(0.0), 'noise_variance': np.array(0.1)}, config={})
  x, y = helpers.synthetic_task(rng, 9, 3)
  h = nv.linalg.factor(nv.mean.zero, nv.kernel.dot_product, pn, x, y, None, ctx=gpu_ctx)
  try:
    b = nv.hmodel.BuiltModel(nv.mean.zero, nv.kernel.dot_product, pn, None, np.float64, 3)
    xb2 = np.concatenate([np.zeros((1, 2, 3)), rng.uniform(size=(1, 2, 3))])
    rc, v0, g0 = _raw_grad(gpu_ctx, nat, [b], [h], xb2, tie.z, [-1.0], [0.0])
    _, v1, g1 = _raw_grad(gpu_ctx, nat, [b], [h], xb2[1:], tie.z, [-1.0], [0.0])
    assert rc == nat.HBO_OK
    assert np.isnan(v0[0, 0]) and np.all(np.isnan(g0[0, 0]))
    assert same_bits(v0[0, 1:], v1[0]) and same_bits(g0[0, 1:], g1[0]) and np.all(np.isfinite(g0[0, 1])) and np.isfinite(v0[0, 1])
    rc, v2, g2 = _raw_grad(gpu_ctx, nat, [b], [h], xb2, tie.z, [-1.0], [0.1])     # with noise the same call is finite throughout
    assert rc == nat.HBO_OK and np.all(np.isfinite(v2)) and np.all(np.isfinite(g2))
  finally:
    h.close()


def test_a_sample_that_is_not_positive_definite(gpu_ctx):
  nv = _nv()
  nat = nv.nat
  rng = np.random.default_rng(92)
  bad = [{'dot_prod_sigma': np.array(1.0), 'dot_prod_bias': np.array(0.1), 'noise_variance': np.array(nvar)} for nvar in (0.1, -1.0, 0.2)]
  x, y = helpers.synthetic_task(rng, 90, 2)
  xb, z = rng.uniform(size=(2, 3, 2)), rng.standard_normal((17, 3))
  handles, built = [], []
  try:
    for model in bad:
      pn = nv.defs.GPParams(model=model, config={})
      handles.append(nv.linalg.factor(nv.mean.zero, nv.kernel.dot_product, pn, x, y, None, ctx=gpu_ctx))
      built.append(nv.hmodel.BuiltModel(nv.mean.zero, nv.kernel.dot_product, pn, None, np.float64, 2))
    assert [h.status for h in handles] == [nat.HBO_OK, nat.HBO_NOT_PD, nat.HBO_OK]
    call = lambda sel: _raw_grad(gpu_ctx, nat, [built[i] for i in sel], [handles[i] for i in sel], xb, z, [0.3] * len(sel), [0.1] * len(sel))
    rc, val, grad = call([0, 1, 2])
    assert rc == nat.HBO_NOT_PD
    assert np.all(np.isnan(val[1])) and np.all(np.isnan(grad[1]))
    rc2, v2, g2 = call([0, 2])
    assert rc2 == nat.HBO_OK and same_bits(val[[0, 2]], v2) and same_bits(grad[[0, 2]], g2) and np.all(np.isfinite(g2))
  finally:
    for h in handles:
      h.close()


def _raw_grad(ctx, nat, built, handles, xb, z, targets, noises, fill=7.0):
  s = len(built)
  structs = (nat.Model * s)(*[b.struct for b in built])
  caches = (C.c_void_p * s)(*[None if h is None else h.handle for h in handles])
  m, q, d = xb.shape
  val, grad = np.full((s, m), fill), np.full((s, m, q, d), fill)
  rc = nat.lib().hbo_qei_grad_samples(ctx.handle, structs, s, caches, nat.ptr(xb), m, q, _dp(z), z.shape[0], (C.c_double * s)(*targets),
                                      (C.c_double * s)(*noises), SCALE, _dp(val), _dp(grad))
  return rc, val, grad


def test_refusals_touch_no_output(gpu_ctx):
  """Every HBO_ERR_UNSUPPORTED of the two entry points names its reason and leaves the outputs and the state as they were: a cache of
  n > 128, the prior branch, an MLP-basis kernel, a linear_mlp mean, a Kumaraswamy warp, and (the maximiser) a state beyond 64 KB of LDS.
  HBO_ERR_ARG the same way: samples of two families; a cache of another input_dim, dtype or input warp than its model; and, for the
  maximiser, the box, start and state checks it takes over from hbo_acq_maximize, on the box tiled q times."""
  nv = _nv()
  nat = nv.nat
  rng = np.random.default_rng(197)
  d, wf = 3, nv.utils.DEFAULT_WARP_FUNC
  xb, z = rng.uniform(size=(2, 2, d)), rng.standard_normal((9, 2))
  err = lambda: (nat.lib().hbo_last_error(gpu_ctx.handle) or b'').decode()
  opts = nat.AcqOptOpts(**ao.DEFAULTS)

  def calls(built, hs, xb=xb, o_=opts, z=z, lo=None, hi=None, state0=None, only_max=False):
    """Both entry points over sentinels: (rc, message) of each and whether every output (only_max: of the maximiser) and the state
    are as they were."""
    rc1, val, grad = _raw_grad(gpu_ctx, nat, built, hs, xb, z, [0.5] * len(built), [0.1] * len(built))
    m1 = err()
    s, (r, q, dd) = len(built), xb.shape
    structs = (nat.Model * s)(*[b.struct for b in built])
    caches = (C.c_void_p * s)(*[None if h is None else h.handle for h in hs])
    ns = nat.lib().hbo_acq_opt_state_doubles(q * dd, o_.memory)
    state, x, v, status = np.zeros((r, ns)), np.full((r, q, dd), 7.0), np.full(r, 7.0), np.full(r, 7, dtype=np.int32)
    if state0 is not None:
      state[:, :state0.size] = state0
    before = state.copy()
    rc2 = nat.lib().hbo_qei_maximize(gpu_ctx.handle, structs, s, caches, nat.ptr(xb), r, q, nat.ptr(lo), nat.ptr(hi), _dp(z), z.shape[0], (C.c_double * s)(*[0.5] * s),
                                     (C.c_double * s)(*[0.1] * s), SCALE, C.byref(o_), nat.ptr(state), 4, nat.ptr(x), nat.ptr(v), nat.ptr(status), None)
    m2 = err()
    untouched = bool((only_max or (np.all(val == 7.0) and np.all(grad == 7.0))) and np.all(x == 7.0) and np.all(v == 7.0) and np.all(status == 7) and
                     same_bits(state, before))
    return rc1, m1, rc2, m2, untouched

  handles = []
  try:
    plain = helpers.make_model(rng, 'constant', False, d)
    pn = nv.defs.GPParams(model=plain, config={})
    mk = lambda n, kern=nv.kernel.matern52, mean=nv.mean.constant, par=pn: (
        nv.hmodel.BuiltModel(mean, kern, par, wf, np.float64, d),
        handles.append(nv.linalg.factor(mean, kern, par, *helpers.synthetic_task(rng, n, d), wf, ctx=gpu_ctx)) or handles[-1])
    b, h = mk(128)
    rc1, m1, rc2, m2, untouched = calls([b], [h])
    assert rc1 == rc2 == nat.HBO_OK and not untouched, (rc1, m1, rc2, m2)                                    # served ...
    b129, h129 = mk(129)
    rc1, m1, rc2, m2, untouched = calls([b129], [h129])
    assert rc1 == rc2 == nat.HBO_ERR_UNSUPPORTED and 'n > 128' in m1 and 'n > 128' in m2 and untouched, (rc1, m1, rc2, m2)
    rc1, m1, rc2, m2, untouched = calls([b], [None])
    assert rc1 == rc2 == nat.HBO_ERR_UNSUPPORTED and 'prior branch' in m1 and 'prior branch' in m2 and untouched, (rc1, m1, rc2, m2)
    for case, word in ((lc.Case('matern32', 'linear_mlp', (5,), d, 9, 'fp64', (8, 8), True), 'MLP basis'),
                       (lc.Case('squared_exponential', 'linear_mlp', (5,), d, 9, 'fp64', (4, 5), False), 'linear_mlp')):
      pm = lc.problem(case)
      dm = Dev(gpu_ctx, pm)
      try:
        rc1, m1, rc2, m2, untouched = calls(dm.built, dm.handles)
        assert rc1 == rc2 == nat.HBO_ERR_UNSUPPORTED and word in m1 and word in m2 and untouched, (rc1, m1, rc2, m2)
      finally:
        dm.close()
    km = dict(plain); km['kumar_params'] = {'a': np.full(d, 0.3), 'b': np.full(d, -0.2)}
    bk, hk = mk(20, kern=nv.kernel.matern52_kumar, par=nv.defs.GPParams(model=km, config={}))
    rc1, m1, rc2, m2, untouched = calls([bk], [hk])
    assert rc1 == rc2 == nat.HBO_ERR_UNSUPPORTED and 'Kumaraswamy' in m1 and 'Kumaraswamy' in m2 and untouched, (rc1, m1, rc2, m2)
    # two families in one call
    bse, hse = mk(20, kern=nv.kernel.squared_exponential)
    rc1, m1, rc2, m2, untouched = calls([b, bse], [h, hse])
    assert rc1 == rc2 == nat.HBO_ERR_ARG and 'must share' in m1 and 'must share' in m2 and untouched, (rc1, m1, rc2, m2)
    # the maximiser alone: q * input_dim = 48 with memory 64 fits the control kernel's LDS, 80 does not; the gradient entry serves both
    big = nat.AcqOptOpts(**dict(ao.DEFAULTS, memory=64))
    assert nat.lib().hbo_acq_opt_state_doubles(48, 64) * 8 < 65536 - 4096 and nat.lib().hbo_acq_opt_state_doubles(80, 64) * 8 > 65536
    rc1, m1, rc2, m2, _ = calls([b], [h], xb=rng.uniform(size=(2, 16, d)), o_=big, z=rng.standard_normal((9, 16)))
    assert rc1 == rc2 == nat.HBO_OK, (rc1, m1, rc2, m2)
    p5 = nv.defs.GPParams(model=helpers.make_model(rng, 'constant', False, 5), config={})
    b5 = nv.hmodel.BuiltModel(nv.mean.constant, nv.kernel.matern52, p5, wf, np.float64, 5)
    h5 = nv.linalg.factor(nv.mean.constant, nv.kernel.matern52, p5, *helpers.synthetic_task(rng, 20, 5), wf, ctx=gpu_ctx); handles.append(h5)
    rc1, m1, rc2, m2, untouched = calls([b5], [h5], xb=rng.uniform(size=(2, 16, 5)), o_=big, z=rng.standard_normal((9, 16)), only_max=True)
    assert rc1 == nat.HBO_OK and rc2 == nat.HBO_ERR_UNSUPPORTED and '64 KB of LDS' in m2 and untouched, (rc1, m1, rc2, m2)
    # a cache that does not match its model: another input_dim, another dtype, another input warp
    rc1, m1, rc2, m2, untouched = calls([b], [h5])
    assert rc1 == rc2 == nat.HBO_ERR_ARG and 'cache/model mismatch' in m1 and 'cache/model mismatch' in m2 and untouched, (rc1, m1, rc2, m2)
    b32 = nv.hmodel.BuiltModel(nv.mean.constant, nv.kernel.matern52, nv.defs.GPParams(model=qc._cast(plain, np.float32), config={}), wf, np.float32, d)
    rc1, m1, rc2, m2, untouched = calls([b32], [h], xb=xb.astype(np.float32))
    assert rc1 == rc2 == nat.HBO_ERR_ARG and 'cache/model mismatch' in m1 and 'cache/model mismatch' in m2 and untouched, (rc1, m1, rc2, m2)
    rc1, m1, rc2, m2, untouched = calls([b], [hk])
    assert rc1 == rc2 == nat.HBO_ERR_ARG and 'another input warp' in m1 and 'another input warp' in m2 and untouched, (rc1, m1, rc2, m2)
    # the maximiser's box, start and state checks, on the box tiled q times: the gradient entry has none of them
    lo, hi = np.full(d, 0.25), np.full(d, 0.75)
    inside = np.ascontiguousarray(0.25 + 0.5 * xb)
    bad_hi = hi.copy(); bad_hi[1] = 0.2
    _, _, rc2, m2, untouched = calls([b], [h], xb=inside, lo=lo, hi=bad_hi, only_max=True)
    assert rc2 == nat.HBO_ERR_ARG and 'lo <= hi' in m2 and untouched, (rc2, m2)
    _, _, rc2, m2, untouched = calls([b], [h], xb=inside, lo=lo, hi=None, only_max=True)
    assert rc2 == nat.HBO_ERR_ARG and 'both' in m2 and untouched, (rc2, m2)
    outside = inside.copy(); outside[1, 1, 2] = 0.76                           # the last coordinate of the last point of the last start
    _, _, rc2, m2, untouched = calls([b], [h], xb=outside, lo=lo, hi=hi, only_max=True)
    assert rc2 == nat.HBO_ERR_ARG and 'outside the box' in m2 and untouched, (rc2, m2)
    _, _, rc2, m2, untouched = calls([b], [h], xb=inside, lo=lo, hi=hi, state0=np.array([3.0, 1.0, 2.0]), only_max=True)
    assert rc2 == nat.HBO_ERR_ARG and 'state is neither' in m2 and untouched, (rc2, m2)
    _, _, rc2, m2, untouched = calls([b], [h], xb=inside, lo=lo, hi=hi, only_max=True)
    assert rc2 == nat.HBO_OK and not untouched, (rc2, m2)                       # ... and served inside the box
  finally:
    for hh in handles:
      hh.close()


# ---- the maximiser --------------------------------------------------------------------------------------------------------------
def _host_driven(dev, x0, z, lo, hi, evals, sel):
  """The same run as a Python loop: hbo_qei_grad_samples on the pending batches, the control code's host hook once per start."""
  nat = dev.nv.nat
  r, q, d = x0.shape
  opts = nat.AcqOptOpts(**ao.DEFAULTS)
  ns = nat.lib().hbo_acq_opt_state_doubles(q * d, opts.memory)
  state = np.zeros((r, ns))
  log = np.zeros((evals, r), dtype=nat.ACQ_OPT_EVAL_DTYPE)
  pending = np.ascontiguousarray(x0, dtype=dev.dtype).copy()
  x, status = np.zeros((r, q * d)), np.zeros(r, dtype=np.int32)
  blo, bhi = np.tile(lo, q), np.tile(hi, q)
  ev, st, x_next, x_iter = nat.AcqOptEval(), C.c_int32(0), np.zeros(q * d), np.zeros(q * d)
  for e in range(evals):
    v64, grads = dev.grad(pending, z, sel=sel)
    for k in range(r):
      start = np.ascontiguousarray(pending[k].reshape(-1), dtype=np.float64)
      rc = nat.lib().hbo_probe_acq_opt_ctl(nat.ptr(state[k]), q * d, nat.dtype_code(dev.dtype), C.byref(opts), nat.ptr(blo), nat.ptr(bhi), nat.ptr(start),
                                           nat.ptr(np.ascontiguousarray(v64[:, k])), nat.ptr(np.ascontiguousarray(grads[:, k].reshape(len(sel), -1))),
                                           len(sel), nat.ptr(x_next), nat.ptr(x_iter), C.byref(ev), C.byref(st))
      assert rc == nat.HBO_OK, (nat.lib().hbo_last_error(None) or b'').decode()
      log[e, k] = (ev.kind, ev.iter, ev.alpha, ev.value)
      if ev.kind != nat.ACQ_OPT_IDLE:
        pending[k] = x_next.reshape(q, d)
      x[k], status[k] = x_iter, st.value
  return log, x.reshape(r, q, d), -state[:, 5], status, state


@pytest.mark.parametrize('S', [1, 3])
@pytest.mark.parametrize('q', [2, 4])
def test_maximiser(gpu_ctx, q, S):
  """R = 4 starting batches of q points in D = 3 over the box [0.25, 0.75]^3, one on the boundary.  The log, x_out, val_out and status
  equal acq_opt_oracle.minimise on the flattened variable, driven by the device's own hbo_qei_grad_samples, to the bit, and the state
  the control code's host hook leaves when driven the same way; 48 evaluations in one call equal 7 + 41 in two, to the bit; every
  iterate stays inside the box; val_out is the sample-order mean of the gradient entry's values at x_out; the final value is no lower
  than the start's."""
  case = qc.Case('matern52', 'constant', (40, 64, 17)[:S], 3, q, 64, 4, 'fp64', True)
  p = qc.problem(case)
  dev = Dev(gpu_ctx, p)
  try:
    nat = dev.nv.nat
    lo, hi = np.full(3, 0.25), np.full(3, 0.75)
    x0 = np.ascontiguousarray(lo + (hi - lo) * p.xb)
    x0[0, 0] = [0.25, 0.75, 0.5]                                # a point of a start on the boundary
    sel = list(range(S))
    run = lambda e, **kw: dev.maximize(x0, p.z, lo, hi, e, **kw)
    log, x, val, status, state = run(48)
    la, xa, va, sa, sta = run(7)
    lb, xb, vb, sb, stb = run(41, state=sta.copy())
    assert same_bits(np.concatenate([la, lb]), log) and same_bits(xb, x) and same_bits(vb, val) and same_bits(sb, status) and same_bits(stb, state)
    assert np.all(np.isfinite(val)) and np.all((x >= lo) & (x <= hi))
    assert np.all(log['kind'][0] == nat.ACQ_OPT_START) and np.any(log['kind'] == nat.ACQ_OPT_MAIN)
    # the control code's own host hook, driven by the gradient entry: everything to the bit, the state included
    hl, hx, hv, hs, hst = _host_driven(dev, x0, p.z, lo, hi, 48, sel)
    assert same_bits(hl, log) and same_bits(hx, x) and same_bits(hv, val) and same_bits(hs, status) and same_bits(hst, state)
    # the NumPy restatement of the optimiser on the flattened variable
    blo, bhi = np.tile(lo, q), np.tile(hi, q)

    def vg(xf):
      v, g = dev.grad(xf.reshape(1, q, 3), p.z, sel=sel)
      assert np.all((xf >= blo) & (xf <= bhi))                 # every iterate and probe inside the box
      return v[:, 0], g[:, 0].reshape(S, -1)
    for r in range(4):
      ref = ao.minimise(vg, x0[r].reshape(-1), blo, bhi, max_evals=48)
      for e, (kind, it, alpha, _, f) in enumerate(ref.log):
        rec = log[e, r]
        assert (rec['kind'], rec['iter']) == (kind, it) and rec['alpha'] == alpha and rec['value'] == f, (r, e, rec, kind, it, alpha, f)
      assert np.all(log['kind'][len(ref.log):, r] == nat.ACQ_OPT_IDLE)
      assert same_bits(x[r].reshape(-1), ref.x) and val[r] == -ref.f and status[r] == ref.status, (r, status[r], ref.status)
    v_end, _ = dev.grad(x, p.z, sel=sel)
    v_start, _ = dev.grad(x0, p.z, sel=sel)
    mean = lambda v: np.array([-ao.reduce_samples(v[:, r], np.zeros((S, 1)))[0] for r in range(4)])
    assert same_bits(mean(v_end), val) and same_bits(-log['value'][0], mean(v_start))
    assert np.all(val >= mean(v_start))
    print(f'\nqei: maximiser q={q} S={S}: status {status.tolist()}, value {mean(v_start).tolist()} -> {val.tolist()}')
  finally:
    dev.close()


# ---- Python ---------------------------------------------------------------------------------------------------------------------------
def _models(nv, hgp, n=30, d=2, seed=3):
  rng = np.random.default_rng(seed)
  f = lambda x: np.sin(3.0 * x[:, :1]) + np.cos(2.0 * x[:, 1:2])
  x = rng.uniform(size=(n, d))
  x2 = rng.uniform(size=(10, d))
  ds = {'t': nv.defs.SubDataset(x, f(x)), 'a': nv.defs.SubDataset(x2, f(x2)), 'b': nv.defs.SubDataset(x2[:4], f(x2[:4]))}
  samples = [{'lengthscale': np.full(d, 0.1 * i), 'signal_variance': np.array(0.5 - 0.2 * i), 'noise_variance': np.array(-5.0), 'constant': np.array(0.3)}
             for i in range(3)]
  wf = nv.utils.DEFAULT_WARP_FUNC
  if hgp:
    return nv.gp.HGP(ds, nv.mean.constant, nv.kernel.squared_exponential, nv.defs.GPParams(model=samples[0], samples=samples, config={}), wf), f
  return nv.gp.GP(ds, nv.mean.constant, nv.kernel.squared_exponential, nv.defs.GPParams(model=samples[0], config={}), wf), f


def test_python_values_are_the_c_entry_and_the_hgp_mean(gpu_ctx):
  nv = _nv()
  nat = nv.nat
  qei = nv.acfun.q_expected_improvement
  model, _ = _models(nv, False)
  xb = np.random.default_rng(8).uniform(size=(5, 3, 2))
  z = qei.base_samples(3, 11)
  out = qei(model=model, sub_dataset_key='t', x_batches=xb, base_samples=z)
  v, g = qei.value_and_grad(model=model, sub_dataset_key='t', x_batches=xb, base_samples=z)
  assert out.shape == (5, 1) and g.shape == (5, 3, 2) and same_bits(out, v) and np.all(np.isfinite(g)) and np.all(v >= 0) and np.any(v > 0)
  handle, _, bm, add_noise, scale = nv.acfun._single_model(model, 't')
  target = float(np.max(model.dataset['t'].y))
  rc, val, grad = _raw_grad(handle.ctx, nat, [bm], [handle], np.ascontiguousarray(xb, dtype=handle.dtype), z, [target], [add_noise])
  assert rc == nat.HBO_OK and scale == SCALE and same_bits(val[0][:, None], v) and same_bits(grad[0], g)
  # an HGP: the mean over plain GPs under each sample's parameters (to a few ulp: the GP's own factor against the HGP's per-sample one)
  hgp, _ = _models(nv, True)
  hv, hg = qei.value_and_grad(model=hgp, sub_dataset_key='t', x_batches=xb, base_samples=z)
  rows = []
  for smp in hgp.get_model_params_samples():
    gp1 = nv.gp.GP(hgp.dataset, hgp.mean_func, hgp.cov_func, nv.defs.GPParams(model=smp, config={}), hgp.warp_func)
    rows.append(qei.value_and_grad(model=gp1, sub_dataset_key='t', x_batches=xb, base_samples=z))
  mv, mg = sum(r[0] for r in rows) / 3, sum(r[1] for r in rows) / 3
  assert np.allclose(hv, mv, rtol=1e-9, atol=1e-12) and np.allclose(hg, mg, rtol=1e-7, atol=1e-10 * np.max(np.abs(mg)))
  # a model the device route refuses: ValueError under the entry point's message, no fall-back
  big, _ = _models(nv, False, n=129)
  with pytest.raises(ValueError, match='n > 128'):
    qei(model=big, sub_dataset_key='t', x_batches=xb, base_samples=z)


@pytest.mark.parametrize('hgp', [False, True], ids=['gp', 'hgp-S3'])
def test_python_suggest(gpu_ctx, hgp):
  nv = _nv()
  qei = nv.acfun.BatchExpectedImprovement(num_base=64, starts=3)
  model, _ = _models(nv, hgp)
  xc = np.random.default_rng(5).uniform(size=(48, 2))
  a = qei.suggest(model=model, sub_dataset_key='t', x_candidates=xc, key=21, batch_size=3)
  b = qei.suggest(model=model, sub_dataset_key='t', x_candidates=xc, key=21, batch_size=3)
  assert a.shape == (3, 2) and a.dtype == np.float64 and same_bits(a, b)
  assert np.all((a >= 0.0) & (a <= 1.0)) and len({tuple(r) for r in a}) == 3
  c = qei.suggest(model=model, sub_dataset_key='t', x_candidates=xc, key=22, batch_size=3)
  assert not same_bits(a, c) or qei.starts == 1                 # another key draws other starts and base samples
  assert qei.suggest(model=model, sub_dataset_key='t', x_candidates=xc, key=22, batch_size=1).shape == (1, 2)


@pytest.mark.parametrize('name', ['q_expected_improvement', 'thompson_continuous'])
def test_python_bayesopt_batch(gpu_ctx, name):
  """Three iterations of q = 3: nine observations appended in place, inside the box."""
  nv = _nv()
  model, f = _models(nv, False)
  n0 = model.dataset['t'].x.shape[0]
  ac = nv.acfun.BatchExpectedImprovement(num_base=64, starts=3) if name == 'q_expected_improvement' else nv.acfun.thompson_continuous
  sub = nv.bayesopt.bayesopt_batch(model, 't', f, ac, iters=3, batch_size=3, input_sampler=lambda rng, d: rng.uniform(size=(48, d)), key=17)
  assert sub is model.dataset['t'] and sub.x.shape == (n0 + 9, 2) and sub.y.shape[0] == n0 + 9
  new = np.asarray(sub.x[n0:], dtype=np.float64)
  assert np.all((new >= 0.0) & (new <= 1.0)) and np.all(np.isfinite(sub.y)) and len({tuple(r) for r in new}) == 9
