"""hbo_sample_paths_grad and hbo_paths_maximize (csrc/path_opt.hip) on an MI355X (run with `-m gpu`) against tests/path_opt_cases.py:
(a) every (query, path) pair's value and gradient against the longdouble restatement, and the values against hbo_sample_paths;
(b) bit independence -- of the queries and paths that share a call, of the call, and of the maximiser's own evaluations, by replaying
    its log through hbo_probe_acq_opt_ctl fed with hbo_sample_paths_grad;
(c) the maximiser: cut runs, independent pairs, monotone values, the box, and the exact corner of a linear path;
(d) acfun.thompson_maximize and bayesopt.bayesopt with acfun.thompson_continuous;
(e) a cache that is not positive definite, and the refusals.

Bounds (path_opt_cases.py): values fp64 1e-9 per column, fp32 4 x the float32 restatement's own error + 8 eps32; gradients per pair,
max_d |g - g_ref| over the path's largest max_d |g_ref|: fp64 FP64_GRAD_BOUND, fp32 by the same rule as the values.
RATIOS_MEASURED: error over bound, the worst pair of each case, as measured on an MI355X (also in profiles/path_maximize.md).
"""
import ctypes as C

import numpy as np
import pytest

import helpers
import path_opt_cases as poc
import pathwise_cases as pc
from hyperbo_amd import _model
from hyperbo_amd import _native as nat
from hyperbo_amd.basics import definitions as defs
from hyperbo_amd.basics import linalg
from hyperbo_amd.bo_utils import acfun, bayesopt
from hyperbo_amd.gp_utils import gp, kernel, mean, pathwise, utils

pytestmark = pytest.mark.gpu
WF = utils.DEFAULT_WARP_FUNC
EVALS = 16

# largest fp64 gradient error per case (max_d |g - g_ref| over the path's gradient scale) measured on an MI355X: what
# path_opt_cases.FP64_GRAD_BOUND is ten times the maximum of, rounded up to one digit
GRAD_RATIOS_MEASURED = {
    'worst': 1.924e-13,     # dot_product + linear, n 300, D 17, S 9 (a Gram matrix of rank 18 under noise 0.13): 10 x -> 2e-12
    'others': 2.262e-14,    # the largest of the other fourteen fp64 cases (SE, n 256, D 3); they measure 1.3e-16 .. 2.3e-14
    'fp32 / bound': 0.261,  # the worst fp32 case against its own bound (dot_product + zero, n 129, D 3); the others 0.02 .. 0.25
}


class Dev:
  """A case on the device: its model, and its cache when it has observations.  Close it."""

  def __init__(self, case, ctx, prob=None):
    self.case, self.ctx = case, ctx
    self.prob = p = poc.problem(case) if prob is None else prob
    self.mean_func, self.cov_func = getattr(mean, p.mname), getattr(kernel, p.kname)
    self.params = defs.GPParams(model=p.model, config={})
    self.dtype = p.xq.dtype
    self.d = p.xq.shape[1]
    self.bm = _model.BuiltModel(self.mean_func, self.cov_func, self.params, WF, self.dtype, self.d)
    self.handle = linalg.factor(self.mean_func, self.cov_func, self.params, p.x, p.y, WF, ctx=ctx) if p.x.shape[0] else None
    self.opts = nat.AcqOptOpts(**poc.OPT_DEFAULTS)
    self.ns = nat.lib().hbo_acq_opt_state_doubles(self.d, self.opts.memory)
    self.lo = self.hi = None

  def close(self):
    if self.handle is not None:
      self.handle.close()

  def _draws(self, cols):
    p = self.prob
    cols = list(range(p.w.shape[1])) if cols is None else list(cols)
    w = np.ascontiguousarray(p.w[:, cols])
    eps = None if p.eps is None else np.ascontiguousarray(p.eps[:, cols])
    return w, eps

  def vg(self, xq=None, cols=None, dev=None, rc_only=False):
    """hbo_sample_paths_grad: ([M, S] values, [M, S, D] gradients) of the paths `cols` at xq."""
    p = self.prob
    xq = p.xq if xq is None else np.ascontiguousarray(xq, dtype=self.dtype)
    w, eps = self._draws(cols)
    out = np.full((xq.shape[0], w.shape[1]), 7.0, dtype=self.dtype)
    grad = np.full((xq.shape[0], w.shape[1], self.d), 7.0)
    rc = nat.lib().hbo_sample_paths_grad(self.ctx.handle, self.bm.ref(), self.handle.handle if self.handle else None, nat.ptr(xq), xq.shape[0],
                                         w.shape[1], w.shape[0], nat.ptr(p.omega), nat.ptr(p.phase), nat.ptr(w), nat.ptr(eps),
                                         self.case.dev if dev is None else dev, nat.ptr(out), grad.ctypes.data_as(C.POINTER(C.c_double)))
    if rc_only:
      return rc, out, grad
    self.ctx.check(rc, allow_not_pd=False)
    return out, grad

  def paths(self):
    p = self.prob
    out = np.full((p.xq.shape[0], p.w.shape[1]), np.nan, dtype=self.dtype)
    self.ctx.check(nat.lib().hbo_sample_paths(self.ctx.handle, self.bm.ref(), self.handle.handle if self.handle else None, nat.ptr(p.xq),
                                              p.xq.shape[0], p.w.shape[1], p.w.shape[0], nat.ptr(p.omega), nat.ptr(p.phase), nat.ptr(p.w),
                                              nat.ptr(p.eps) if self.handle else None, nat.ptr(out)), allow_not_pd=False)
    return out

  def starts(self, r=None):
    """[S, R, D] starts in the model dtype: the case's queries, taken round the clock."""
    p, r = self.prob, self.case.R if r is None else r
    s = p.w.shape[1]
    idx = (np.arange(s)[:, None] * 2 + np.arange(r)[None, :] + 3) % p.xq.shape[0]
    return np.ascontiguousarray(p.xq[idx], dtype=self.dtype)

  def maximize(self, x0, cols=None, evals=EVALS, state=None, want_log=True, rc_only=False):
    """One hbo_paths_maximize call over x0 [S, R, D]: (log [evals, S R], x [S, R, D], val [S, R], status [S, R], state)."""
    p = self.prob
    w, eps = self._draws(cols)
    s, r, d = x0.shape
    assert s == w.shape[1]
    state = np.zeros((s * r, self.ns)) if state is None else state
    x, val, status = np.full((s, r, d), 7.0), np.full((s, r), 7.0), np.full((s, r), 7, dtype=np.int32)
    log = np.zeros((evals, s * r), dtype=nat.ACQ_OPT_EVAL_DTYPE) if want_log else None
    rc = nat.lib().hbo_paths_maximize(self.ctx.handle, self.bm.ref(), self.handle.handle if self.handle else None, s, w.shape[0],
                                      nat.ptr(p.omega), nat.ptr(p.phase), nat.ptr(w), nat.ptr(eps), self.case.dev, nat.ptr(x0), r,
                                      nat.ptr(self.lo), nat.ptr(self.hi), C.byref(self.opts), nat.ptr(state), evals, nat.ptr(x), nat.ptr(val),
                                      nat.ptr(status), nat.ptr(log))
    if rc_only:
      return rc, x, val, status
    self.ctx.check(rc, allow_not_pd=False)
    return log, x, val, status, state

  def host_driven(self, x0, evals=EVALS):
    """The same run as a Python loop: hbo_sample_paths_grad at the pending points, the host hook once per pair."""
    s, r, d = x0.shape
    state = np.zeros((s * r, self.ns))
    log = np.zeros((evals, s * r), dtype=nat.ACQ_OPT_EVAL_DTYPE)
    pending = np.array(x0.reshape(s * r, d))
    x, status = np.zeros((s * r, d)), np.zeros(s * r, dtype=np.int32)
    ev, st, x_next, x_iter = nat.AcqOptEval(), C.c_int32(0), np.zeros(d), np.zeros(d)
    for e in range(evals):
      vals, grads = self.vg(pending)                                     # [S R, S], [S R, S, D]: pair k reads column k // r
      for k in range(s * r):
        start = np.ascontiguousarray(pending[k], dtype=np.float64)
        v = np.array([float(vals[k, k // r])])
        g = np.ascontiguousarray(grads[k, k // r])
        rc = nat.lib().hbo_probe_acq_opt_ctl(nat.ptr(state[k]), d, nat.dtype_code(self.dtype), C.byref(self.opts), nat.ptr(self.lo), nat.ptr(self.hi),
                                             nat.ptr(start), nat.ptr(v), nat.ptr(g), 1, nat.ptr(x_next), nat.ptr(x_iter), C.byref(ev), C.byref(st))
        assert rc == nat.HBO_OK, (nat.lib().hbo_last_error(None) or b'').decode()
        log[e, k] = (ev.kind, ev.iter, ev.alpha, ev.value)
        if ev.kind != nat.ACQ_OPT_IDLE:
          pending[k] = x_next
        x[k], status[k] = x_iter, st.value
    return log, x.reshape(s, r, d), (-state[:, 5]).reshape(s, r), status.reshape(s, r), state


def same_bits(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_outputs(got, want):
  for g, w, what in zip(got, want, ('log', 'x_out', 'val_out', 'status', 'state')):
    assert same_bits(g, w), what


# ---- (a) values and gradients against longdouble -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', poc.CASES, ids=lambda c: c.id)
def test_values_and_gradients_match_the_restatement_per_pair(gpu_ctx, case):
  dev = Dev(case, gpu_ctx)
  try:
    val, grad = dev.vg()
    sampled = dev.paths() if case.dev == 1.0 else None
  finally:
    dev.close()
  v_ref, g_ref = poc.reference(case)
  vb, gb = poc.value_bound(case), poc.grad_bound(case)
  ev, eg = float(np.max(pc.col_errors(val, v_ref))), float(np.max(poc.grad_errors(grad, g_ref)))
  print(f'PATHOPT {case.id}: value {ev:.3e} bound {vb:.3e} ratio {ev / vb:.3f}; gradient {eg:.3e} bound {gb:.3e} ratio {eg / gb:.3f}'
        + (f' f32 levels {poc.f32_levels(case)[0]:.3e} {poc.f32_levels(case)[1]:.3e}' if case.dtype == 'fp32' else ''))
  assert val.dtype == case.np_dtype and grad.dtype == np.float64
  assert ev <= vb, (ev, vb)
  assert eg <= gb, (np.unravel_index(np.argmax(poc.grad_errors(grad, g_ref)), grad.shape[:2]), eg, gb)
  if sampled is not None:       # dev_scale = 1: the paths of hbo_sample_paths at the same draws
    es = float(np.max(pc.col_errors(val, sampled.astype(np.float64))))
    print(f'PATHOPT {case.id}: against hbo_sample_paths {es:.3e}')
    assert es <= vb, (es, vb)


# ---- (b) bit independence ------------------------------------------------------------------------------------------------------------------
BIT_CASES = [c for c in poc.CASES if (c.n, c.d) in ((127, 3), (128, 17), (257, 1), (0, 3), (127, 256), (300, 17))]


@pytest.mark.parametrize('case', BIT_CASES, ids=lambda c: c.id)
def test_bits_do_not_depend_on_the_call_or_on_what_shares_it(gpu_ctx, case):
  dev = Dev(case, gpu_ctx)
  p = dev.prob
  try:
    a = dev.vg()
    b = dev.vg()
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all() and same_bits(a[0], b[0]) and same_bits(a[1], b[1]), 'two identical calls differ'
    for j in sorted({0, case.S // 2, case.S - 1}):
      for rows in ([0], [5, 2], [3]):
        v, g = dev.vg(p.xq[rows], cols=[j])
        assert same_bits(v[:, 0], np.ascontiguousarray(a[0][rows, j])), f'value of path {j} at queries {rows} depends on the call'
        assert same_bits(g[:, 0], np.ascontiguousarray(a[1][rows, j])), f'gradient of path {j} at queries {rows} depends on the call'
    # the maximiser's own evaluations: its log, replayed on the host from hbo_sample_paths_grad at every pending point
    x0 = dev.starts()
    got = dev.maximize(x0)
    want = dev.host_driven(x0)
    same_outputs(got, want)
    log = got[0]
    assert np.all(log['kind'][0] == nat.ACQ_OPT_START)
    v0, _ = dev.vg(x0.reshape(-1, case.d))
    for k in range(x0.shape[0] * x0.shape[1]):
      assert log['value'][0, k] == -float(v0[k, k // x0.shape[1]])
  finally:
    dev.close()


# ---- (c) the maximiser -----------------------------------------------------------------------------------------------------------------------
MAX_CASES = [c for c in poc.CASES if (c.n, c.d, c.R) in ((127, 3, 5), (129, 33, 5), (256, 3, 5), (0, 3, 5), (129, 3, 5))]


@pytest.mark.parametrize('case', MAX_CASES, ids=lambda c: c.id)
def test_maximiser_cuts_pairs_values_and_box(gpu_ctx, case):
  dev = Dev(case, gpu_ctx)
  try:
    x0 = dev.starts()
    whole = dev.maximize(x0, evals=16)
    first = dev.maximize(x0, evals=8)
    second = dev.maximize(x0, evals=8, state=first[4])
    assert same_bits(np.concatenate([first[0], second[0]]), whole[0]), 'log of 8 + 8 evaluations'
    for k, what in ((1, 'x_out'), (2, 'val_out'), (3, 'status'), (4, 'state')):
      assert same_bits(second[k], whole[k]), what + ' of 8 + 8 evaluations'
    log, x, val, status, state = whole
    s, r, d = x0.shape
    # a pair alone: its path alone, its start alone
    for si, ri in sorted({(0, 0), (s - 1, r - 1), (s // 2, 1 % r)}):
      lone = dev.maximize(np.ascontiguousarray(x0[si:si + 1, ri:ri + 1]), cols=[si], evals=16)
      k = si * r + ri
      assert same_bits(lone[0][:, 0], np.ascontiguousarray(log[:, k])) and same_bits(lone[1][0, 0], x[si, ri]), (si, ri)
      assert lone[2][0, 0] == val[si, ri] and lone[3][0, 0] == status[si, ri] and same_bits(lone[4][0], state[k]), (si, ri)
    v0, _ = dev.vg(x0.reshape(-1, d))
    v0 = np.array([float(v0[k, k // r]) for k in range(s * r)]).reshape(s, r)
    assert np.all(val >= v0), 'a run ended below its start'
    assert np.all(x >= 0.0) and np.all(x <= 1.0) and np.array_equal(x, x.astype(dev.dtype).astype(np.float64))
    # val_out is the path's value at x_out, as hbo_sample_paths_grad returns it
    v1, _ = dev.vg(x.reshape(-1, d))
    v1 = np.array([float(v1[k, k // r]) for k in range(s * r)]).reshape(s, r)
    assert np.array_equal(val, v1)
    # caller's bounds: fp32 numbers, hit exactly
    dev.lo, dev.hi = np.full(d, 0.25), np.full(d, 0.75)
    xb0 = np.ascontiguousarray(np.clip(x0, 0.25, 0.75), dtype=dev.dtype)
    _, xb, _, _, _ = dev.maximize(xb0, evals=16)
    assert np.all(xb >= 0.25) and np.all(xb <= 0.75)
  finally:
    dev.close()


@pytest.mark.parametrize('case', poc.LINEAR_CASES, ids=lambda c: c.id)
def test_linear_paths_end_in_their_corner(gpu_ctx, case):
  corner, _, chosen = poc.linear_corner(case)
  cols = [int(j) for j in np.flatnonzero(chosen)]
  assert cols
  dev = Dev(case, gpu_ctx)
  try:
    dev.opts.max_iters = poc.CORNER_EVALS
    x0 = dev.starts()[cols]
    log, x, val, status, _ = dev.maximize(x0, cols=cols, evals=poc.CORNER_EVALS, want_log=False)
    assert np.all(status == nat.ACQ_OPT_CONVERGED), status
    for a, j in enumerate(cols):
      assert np.array_equal(x[a], np.broadcast_to(corner[j], x[a].shape)), (j, x[a], corner[j])
  finally:
    dev.close()


# ---- (d) the Python surface ------------------------------------------------------------------------------------------------------------------
def _gp_model(case, n=None):
  p = poc.problem(case)
  n = case.n if n is None else n
  ds = {0: defs.SubDataset(p.x[:n].copy(), p.y[:n].copy())}     # (n = 0: an empty sub-dataset, the prior branch)
  return gp.GP(ds, getattr(mean, p.mname), getattr(kernel, p.kname), defs.GPParams(model=p.model, config={}), WF)


def test_thompson_maximize_beats_the_best_candidate_of_every_path(gpu_ctx):
  case = next(c for c in poc.CASES if c.n == 127 and c.d == 3 and c.dtype == 'fp64')
  model = _gp_model(case)
  xc = np.random.default_rng(31).uniform(size=(40, case.d))
  got = acfun.thompson_maximize(model, 0, xc, batch_size=4, key=9, num_features=64, starts=3)
  assert got.shape == (4, case.d) and np.all(got >= 0) and np.all(got <= 1)
  draws = model.draw_paths(0, num_samples=4, num_features=64, key=9)          # the same key: the same paths
  assert isinstance(draws, pathwise.PathDraws) and draws.n == case.n
  best = draws.values(xc).max(axis=0)
  mine = draws.values(got)
  for s in range(4):
    assert mine[s, s] >= best[s], (s, mine[s, s], best[s])
  # the paths are sample_paths' own
  f = model.sample_paths(xc, num_samples=4, num_features=64, key=9)
  assert np.max(pc.col_errors(draws.values(xc), f)) <= pc.FP64_BOUND
  # draws over a cache that has grown since are refused
  model.update_sub_dataset((xc[:1], np.zeros((1, 1))), 0, is_append=True)
  model.setup_predictor(0)
  with pytest.raises(ValueError, match='draw again'):
    draws.values(xc)


def test_bayesopt_with_thompson_continuous_from_an_empty_sub_dataset(gpu_ctx):
  case = next(c for c in poc.CASES if c.n == 127 and c.d == 3 and c.dtype == 'fp64')
  model = _gp_model(case, n=0)
  f = lambda x: -np.sum((x - 0.3) ** 2, axis=1, keepdims=True)
  sub = bayesopt.bayesopt(np.random.default_rng(4), model, 0, f, acfun.ThompsonContinuous(num_features=64, starts=2), 3,
                          lambda r, d: r.uniform(size=(20, d)))
  assert sub.x.shape == (3, case.d) and np.all(sub.x >= 0.0) and np.all(sub.x <= 1.0) and sub.y.shape[0] == 3


# ---- (e) failure paths ---------------------------------------------------------------------------------------------------------------------
def test_a_cache_that_is_not_positive_definite(gpu_ctx):
  good_case = next(c for c in poc.CASES if c.kname == 'dot_product' and c.n == 129 and c.dtype == 'fp64')
  good = Dev(good_case, gpu_ctx)
  bad_model = {'dot_prod_sigma': np.array(1.0), 'dot_prod_bias': np.array(0.1), 'noise_variance': np.array(-1.0)}
  p = good.prob
  bad = None
  try:
    before = good.vg()
    x0 = good.starts()
    run_before = good.maximize(x0)
    # the model of test_gpu_acq_fused.py's indefinite sample: unwarped parameters with a negative noise variance
    params = defs.GPParams(model=bad_model, config={})
    h = linalg.factor(mean.zero, kernel.dot_product, params, p.x, p.y, None, ctx=gpu_ctx)
    assert h.status == nat.HBO_NOT_PD
    bad = Dev(good_case, gpu_ctx, prob=p._replace(model=bad_model, x=p.x[:0], y=p.y[:0]))
    bad.bm = _model.BuiltModel(mean.zero, kernel.dot_product, params, None, np.float64, good_case.d)
    bad.handle = h
    rc, val, grad = bad.vg(rc_only=True)
    assert rc == nat.HBO_NOT_PD and np.isnan(val).all() and np.isnan(grad).all()
    rc, x, v, status = bad.maximize(x0, rc_only=True)
    assert rc == nat.HBO_NOT_PD and np.isnan(v).all() and np.all(status == nat.ACQ_OPT_NONFINITE_AT_START)
    assert np.array_equal(x, x0.astype(np.float64))                    # the iterate of a run that never started: its start
    # a later good call on the same context is what it was
    after = good.vg()
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
    same_outputs(good.maximize(x0), run_before)
  finally:
    good.close()
    if bad is not None:
      bad.close()


def test_refusals_leave_the_outputs_alone(gpu_ctx):
  err = lambda: (nat.lib().hbo_last_error(gpu_ctx.handle) or b'').decode()
  base = next(c for c in poc.CASES if c.n == 127 and c.d == 3 and c.dtype == 'fp64')
  dev = Dev(base, gpu_ctx)
  extra = []
  try:
    x0 = dev.starts()

    def refused(code, text):
      rc, val, grad = dev.vg(rc_only=True)
      assert rc == code and text in err(), (rc, err())
      assert np.all(val == 7.0) and np.all(grad == 7.0)
      state = np.zeros((x0.shape[0] * x0.shape[1], dev.ns))
      rc, x, v, status = dev.maximize(x0, state=state, rc_only=True)
      assert rc == code and text in err(), (rc, err())
      assert np.all(x == 7.0) and np.all(v == 7.0) and np.all(status == 7) and np.all(state == 0.0)

    rng = np.random.default_rng(5)
    p = dev.prob

    def swap(kn, mn, model, config=None):
      pn = defs.GPParams(model=model, config=config or {})
      h = linalg.factor(mn, kn, pn, p.x, p.y, WF, ctx=gpu_ctx)
      extra.append(h)
      old = dev.handle
      dev.handle, dev.bm = h, _model.BuiltModel(mn, kn, pn, WF, np.float64, base.d)
      if old is not None and old not in extra:
        extra.append(old)

    cfg = {'mlp_features': helpers.MLP_FEATURES}
    swap(kernel.matern32_mlp, mean.constant, helpers.make_model(rng, 'constant', True, base.d), cfg)
    # (omega of an MLP-basis model has the width of the last layer; the refusal comes before it is read)
    refused(nat.HBO_ERR_UNSUPPORTED, 'MLP basis')
    swap(kernel.matern32, mean.linear_mlp, helpers.make_model(rng, 'linear_mlp', False, base.d), cfg)
    refused(nat.HBO_ERR_UNSUPPORTED, 'linear_mlp mean')
    km = dict(helpers.make_model(rng, 'constant', False, base.d)); km['kumar_params'] = {'a': np.full(base.d, 0.3), 'b': np.full(base.d, -0.2)}
    swap(kernel.matern32_kumar, mean.constant, km)
    refused(nat.HBO_ERR_UNSUPPORTED, 'Kumaraswamy')
    # an argument error on the device box, too: nothing is written
    swap(kernel.matern32, mean.constant, helpers.make_model(rng, 'constant', False, base.d))
    dev.case = base._replace(dev=0.0)
    refused(nat.HBO_ERR_ARG, 'dev_scale')
    dev.case = base
    # a state beyond the control kernel's LDS (D = 256, memory 64): the maximiser alone
    wide = next(c for c in poc.CASES if c.d == 256 and c.n == 1 and c.dtype == 'fp64')
    dw = Dev(wide, gpu_ctx)
    try:
      dw.opts.memory = 64
      dw.ns = nat.lib().hbo_acq_opt_state_doubles(wide.d, 64)
      xw = dw.starts()
      state = np.zeros((xw.shape[0] * xw.shape[1], dw.ns))
      rc, x, v, status = dw.maximize(xw, state=state, rc_only=True)
      assert rc == nat.HBO_ERR_UNSUPPORTED and 'LDS' in err()
      assert np.all(x == 7.0) and np.all(v == 7.0) and np.all(status == 7) and np.all(state == 0.0)
    finally:
      dw.close()
  finally:
    dev.close()
    for h in extra:
      h.close()
