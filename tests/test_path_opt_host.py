"""CPU tier of the path gradient and the path maximiser (hbo_sample_paths_grad, hbo_paths_maximize; pathwise.PathDraws,
acfun.thompson_maximize / thompson_continuous, the `suggest` branch of bayesopt.bayesopt): the exports and their bindings, every
argument error before any device call, the header text, tests/path_opt_cases.py judged on its own (the case list, the longdouble
gradient against central differences of pathwise_cases.restate, the float64 restatement against the bounds, the distance of every
mutant), and the Python surface with the two device calls replaced by the restatement."""
import ctypes as C
import os

import numpy as np
import pytest

import acq_opt_oracle as ao
import helpers
import path_opt_cases as poc
import pathwise_cases as pc
from hyperbo_amd import _native as nat
from hyperbo_amd.basics import definitions as defs
from hyperbo_amd.bo_utils import acfun, bayesopt
from hyperbo_amd.gp_utils import gp, kernel, mean, pathwise, utils

LD = pc.LD


# ---- exports and argument errors -------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_and_bound():
  for name, count in (('hbo_sample_paths_grad', 14), ('hbo_paths_maximize', 21)):
    assert name in nat.SIGNATURES
    f = getattr(nat.lib(), name)
    res, args = nat.SIGNATURES[name]
    assert f.restype is res and list(f.argtypes) == args and len(args) == count


def _model(kernel_id=nat.KERNEL_SE, d=2, dtype=nat.F64):
  m = nat.Model()
  m.kernel_id, m.mean_id, m.dtype, m.input_dim = kernel_id, nat.MEAN_ZERO, dtype, d
  ls = np.ones(d, dtype=np.float64 if dtype == nat.F64 else np.float32)
  m.lengthscale, m.n_lengthscale, m.signal_variance, m.noise_variance, m.eps = nat.ptr(ls).value, d, 1.0, 0.1, 1e-6
  m.dot_prod_sigma, m.dot_prod_bias = 1.0, 0.1
  return m, ls


class Args:
  """Valid arguments of both entry points over a prior-branch model (no cache); outputs and state preset to 7 / 0."""

  def __init__(self, S=2, F=4, M=3, R=2, d=2, kernel_id=nat.KERNEL_SE, dtype=nat.F64, memory=10):
    self.m, self.ls = _model(kernel_id, d, dtype)
    npd = np.float64 if dtype == nat.F64 else np.float32
    s1, f1 = max(S, 1), max(F, 1)
    self.S, self.F, self.M, self.R, self.d = S, F, M, R, d
    self.model, self.cache, self.eps = C.byref(self.m), None, None
    self.xq, self.omega, self.phase, self.w = np.full((M, d), 0.5, dtype=npd), np.zeros((f1, d), dtype=npd), np.zeros(f1, dtype=npd), np.zeros((f1, s1), dtype=npd)
    self.dev_scale = 1.0
    self.out, self.grad = np.full((M, s1), 7.0, dtype=npd), np.full((M, s1, d), 7.0)
    self.x0 = np.full((s1, max(R, 1), d), 0.5, dtype=npd)
    self.lo = self.hi = None
    self.opts = nat.AcqOptOpts(**dict(ao.DEFAULTS, memory=memory))
    self.opts_ref = C.byref(self.opts)
    ns = nat.lib().hbo_acq_opt_state_doubles(d, memory)
    self.state = np.zeros((s1 * max(R, 1), ns))
    self.evals = 4
    self.x, self.val, self.status = np.full((s1, max(R, 1), d), 7.0), np.full((s1, max(R, 1)), 7.0), np.full((s1, max(R, 1)), 7, dtype=np.int32)

  def grad_call(self, ctx=None):
    p = lambda a: a if a is None or not isinstance(a, np.ndarray) else nat.ptr(a)
    return nat.lib().hbo_sample_paths_grad(ctx, self.model, self.cache, p(self.xq), self.M, self.S, self.F, p(self.omega), p(self.phase), p(self.w),
                                           p(self.eps), self.dev_scale, p(self.out),
                                           None if self.grad is None else self.grad.ctypes.data_as(C.POINTER(C.c_double)))

  def max_call(self, ctx=None):
    p = lambda a: a if a is None or not isinstance(a, np.ndarray) else nat.ptr(a)
    return nat.lib().hbo_paths_maximize(ctx, self.model, self.cache, self.S, self.F, p(self.omega), p(self.phase), p(self.w), p(self.eps),
                                        self.dev_scale, p(self.x0), self.R, p(self.lo), p(self.hi), self.opts_ref, p(self.state), self.evals,
                                        p(self.x), p(self.val), p(self.status), None)

  def untouched(self):
    same = lambda a, v: a is None or bool(np.all(a == v))     # (an argument a test has nulled is not there to be written)
    return (same(self.out, 7.0) and same(self.grad, 7.0) and same(self.x, 7.0) and same(self.val, 7.0) and same(self.status, 7) and
            same(self.state, 0.0))


def _err():
  return (nat.lib().hbo_last_error(None) or b'').decode()


def _refused(call, code, text, **kw):
  a = Args(**{k: v for k, v in kw.items() if k in ('S', 'F', 'M', 'R', 'd', 'kernel_id', 'dtype', 'memory')})
  for k, v in kw.items():
    if k not in ('S', 'F', 'M', 'R', 'd', 'kernel_id', 'dtype', 'memory'):
      setattr(a, k, v)
  rc = getattr(a, call)()
  assert rc == code and text in _err(), (call, kw, rc, _err())
  assert a.untouched(), (call, kw)


@pytest.mark.parametrize('call', ['grad_call', 'max_call'])
def test_shared_argument_errors_come_before_any_device_call(call):
  E = nat.HBO_ERR_ARG
  for name in ('model', 'omega', 'phase', 'w'):
    _refused(call, E, 'null argument', **{name: None})
  for S in (0, -1, 1025):
    _refused(call, E, '1 <= S <= 1024', S=S)
  for F in (0, 65537):
    _refused(call, E, '1 <= F <= 65536', F=F)
  for F in (2, 4):
    _refused(call, E, 'F = feature dim + 1', F=F, kernel_id=nat.KERNEL_DOT)
  _refused(call, E, 'eps goes with a cache', eps=np.zeros((3, 2)))
  for c in (0.0, -1.0, np.nan, np.inf):
    _refused(call, E, 'dev_scale', dev_scale=c)
  # the models the kernel does not cover: HBO_ERR_UNSUPPORTED, in the words of hbo_acq_grad_samples
  a = Args()
  a.m.mean_id, a.m.n_layers = nat.MEAN_LINEAR_MLP, 1
  a.m.features[0] = 2
  wk, wb, lk = np.zeros((2, 2)), np.zeros(2), np.zeros(2)
  a.m.mlp_kernel[0], a.m.mlp_bias[0], a.m.linear_kernel = nat.ptr(wk).value, nat.ptr(wb).value, nat.ptr(lk).value
  assert getattr(a, call)() == nat.HBO_ERR_UNSUPPORTED and 'a linear_mlp mean is not supported' in _err(), _err()
  a.m.mean_id, a.m.kernel_uses_mlp = nat.MEAN_ZERO, 1
  assert getattr(a, call)() == nat.HBO_ERR_UNSUPPORTED and 'a kernel on an MLP basis is not supported' in _err(), _err()
  assert a.untouched()
  # ctx is null: reported last, behind every other check
  a = Args()
  assert getattr(a, call)() == nat.HBO_ERR_ARG and 'ctx is null' in _err() and a.untouched()
  a = Args(F=3, kernel_id=nat.KERNEL_DOT)
  assert getattr(a, call)() == nat.HBO_ERR_ARG and 'ctx is null' in _err() and a.untouched()


def test_kumaraswamy_models_are_refused():
  for call in ('grad_call', 'max_call'):
    a = Args()
    mk = nat.ModelKumar()
    ka, kb = np.ones(2), np.ones(2)
    C.memmove(C.byref(mk), C.byref(a.m), C.sizeof(nat.Model))
    mk.base.input_warp = nat.WARP_KUMAR
    mk.kumar_a, mk.kumar_b = nat.ptr(ka).value, nat.ptr(kb).value
    a.model = C.cast(C.byref(mk), C.POINTER(nat.Model))
    assert getattr(a, call)() == nat.HBO_ERR_UNSUPPORTED and 'Kumaraswamy' in _err(), _err()
    assert a.untouched()


def test_argument_errors_of_the_gradient_call():
  for name in ('xq', 'out', 'grad'):
    _refused('grad_call', nat.HBO_ERR_ARG, 'null argument', **{name: None})
  # M == 0: nothing to do, before the context is looked at?  No: HBO_OK needs a context like every call that passed its checks
  a = Args(M=0)
  assert a.grad_call() == nat.HBO_ERR_ARG and 'ctx is null' in _err()


def test_argument_errors_of_the_maximiser():
  E = nat.HBO_ERR_ARG
  for name in ('x0', 'state', 'x', 'val', 'status'):
    _refused('max_call', E, 'null argument', **{name: None})
  _refused('max_call', E, 'opts is null', opts_ref=None)
  for R in (0, -3):
    _refused('max_call', E, 'R >= 1', R=R)
  _refused('max_call', E, 'S * R <= 4096', S=64, R=65)
  for evals in (0, 4097):
    _refused('max_call', E, '1 <= evals', evals=evals)
  for field, bad in (('memory', 0), ('memory', 65), ('ls_steps', 0), ('max_iters', 0), ('c1', 1.0), ('tau', 0.0), ('pgtol', -1.0), ('ftol', np.nan)):
    a = Args()
    setattr(a.opts, field, bad)
    assert a.max_call() == E and 'opts.' in _err() and a.untouched(), (field, _err())
  _refused('max_call', E, 'lo <= hi', lo=np.array([0.0, 0.6]), hi=np.array([1.0, 0.4]))
  _refused('max_call', E, 'lo and hi must both', lo=np.zeros(2))
  _refused('max_call', E, 'fp32 numbers', dtype=nat.F32, lo=np.array([0.1, 0.0]), hi=np.ones(2))
  for bad in (1.5, np.nan):
    a = Args()
    a.x0[1, 0, 1] = bad
    assert a.max_call() == E and 'outside the box' in _err() and a.untouched()
  a = Args()
  a.state[:] = 2.0
  assert a.max_call() == E and 'state is neither' in _err()
  assert np.all(a.state == 2.0) and np.all(a.x == 7.0) and np.all(a.val == 7.0) and np.all(a.status == 7)
  # a state that does not fit the control kernel's LDS: D = 256 with memory 64
  a = Args(d=256, memory=64, S=1, R=1)
  assert a.max_call() == nat.HBO_ERR_UNSUPPORTED and 'LDS' in _err() and a.untouched()


def test_header_documents_the_entry_points():
  text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'hbo.h')).read()
  block = text[text.index('value and d/dx of those paths'):text.index('int hbo_sample_paths_grad')]
  for word in ('dev_scale', 'sin(omega_j', 'zero distance', 'dot product', 'linear mean', 'HBO_ERR_ARG', 'HBO_ERR_UNSUPPORTED', 'HBO_NOT_PD',
               'bit-identical', 'M == 0', 'csrc/path_opt.hip'):
    assert word in block, word
  block = text[text.index('the maximisation of S posterior sample paths'):text.index('int hbo_paths_maximize')]
  for word in ('hbo_acq_maximize', 'S * R', 'x0 [S, R, input_dim]', 'HBO_ERR_ARG', 'HBO_ERR_UNSUPPORTED', 'NONFINITE_AT_START', 'same bits',
               'fp32 numbers', 'one synchronisation'):
    assert word in block, word
  src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'hyperbo_amd', 'csrc', 'path_opt.hip')).read()
  assert 'PO_OT = 256' in src and str(poc.OBS_TILE) == '256' and 'FT x D <= PO_OM = 4096' in src


# ---- tests/path_opt_cases.py on its own -------------------------------------------------------------------------------------------------
FP64_CASES = [c for c in poc.CASES if c.dtype == 'fp64']


def test_case_list_covers_the_issue():
  cs = poc.CASES
  assert {c.n for c in cs} >= {0, 1, 127, 128, 129, 300, poc.OBS_TILE - 1, poc.OBS_TILE, poc.OBS_TILE + 1}
  stationary = [c for c in cs if c.kname != 'dot_product']
  assert {c.F for c in stationary} >= {1, 63, 64, 65, 200}
  offsets = {c.F - poc.feature_tile(c.d) for c in stationary}
  assert offsets >= {-1, 0, 1}
  assert {poc.feature_tile(d) for d in (1, 3, 16)} == {256} and poc.feature_tile(17) == 128 and poc.feature_tile(33) == 64 and poc.feature_tile(256) == 16
  assert {c.d for c in cs} >= {1, 3, 17, 33, 256} and {c.S for c in cs} >= {1, 3, 9} and {c.R for c in cs} >= {1, 5}
  assert {(c.kname, c.ls) for c in cs} == {(k, l) for k in helpers.KERNELS for l in ('scalar', 'ard')}
  assert {c.mname for c in cs} == {'zero', 'constant', 'linear'} and {c.dev for c in cs} == {1.0, poc.SQRT15}
  assert {c.dtype for c in cs} == {'fp64', 'fp32'} and len({c.id for c in cs}) == len(cs)
  assert all(c.F == c.d + 1 for c in cs if c.kname == 'dot_product')
  for c in cs:
    p = poc.problem(c)
    assert p.xq.shape == (poc.N_QUERIES, c.d) and p.xq.dtype == c.np_dtype
    assert (c.n == 0 or np.array_equal(p.xq[0], p.x[0])) and np.all(p.xq[1] == 0) and np.all(p.xq[2] == 1)
    assert (p.model['lengthscale'].size == 1) == (c.ls == 'scalar' and c.kname != 'dot_product') or c.d == 1
  every = set()
  for c in cs:
    every |= set(poc.MUTANTS) - poc.not_applicable(c)
  assert every == set(poc.MUTANTS)


@pytest.mark.parametrize('case', FP64_CASES, ids=lambda c: c.id)
def test_values_agree_with_the_pathwise_restatement(case):
  """dev_scale = 1: pathwise_cases.restate itself.  Otherwise mean + c (path - mean), the mean as its zero draw."""
  prob = poc.problem(case)
  v = poc.reference(case)[0]
  f1, f0 = pc.restate(prob, LD), pc.restate(prob, LD, zero=True)
  want = f0 + LD(case.dev) * (f1 - f0)
  assert np.max(pc.col_errors(v, want)) <= 1e-15, np.max(pc.col_errors(v, want))


@pytest.mark.parametrize('case', [c for c in FP64_CASES if c.d <= 33], ids=lambda c: c.id)
def test_longdouble_gradient_is_the_central_difference_of_the_pathwise_restatement(case):
  prob = poc.problem(case)
  g = poc.reference(case)[1]
  h = LD(2) ** (-6 if case.kname == 'dot_product' else -22)     # (a dot-product path is linear in x: no truncation error at any h)
  f0 = pc.restate(prob, LD, zero=True)
  num = np.zeros_like(g)
  # (queries 1..5: a Matern kernel is not twice differentiable at the coincident query 0, whose one-sided slopes differ from the
  #  rule's 0 by O(h); the corners are differentiated like any point: the formulas do not know the box)
  for dd in range(case.d):
    e = np.zeros(case.d, dtype=LD); e[dd] = h
    fp, fm = [pc.restate(prob._replace(xq=prob.xq.astype(LD) + s * e[None, :]), LD) for s in (1, -1)]
    mp, mm = [pc.restate(prob._replace(xq=prob.xq.astype(LD) + s * e[None, :]), LD, zero=True) for s in (1, -1)]
    num[:, :, dd] = ((mp + LD(case.dev) * (fp - mp)) - (mm + LD(case.dev) * (fm - mm))) / (2 * h)
  first = 1 if case.kname in pc.NU and case.n else 0
  err = poc.grad_errors(g[first:], num[first:]).max()
  assert err <= 1e-9, err          # O(h^2 f''') with h = 2^-22, far above longdouble rounding x conditioning / h


@pytest.mark.parametrize('case', poc.CASES, ids=lambda c: c.id)
def test_case_is_well_conditioned_and_sees_every_mutant(case):
  v, g = poc.reference(case)
  assert v.dtype == LD and g.dtype == LD and v.shape == (poc.N_QUERIES, case.S) and g.shape == (poc.N_QUERIES, case.S, case.d)
  assert np.isfinite(v.astype(np.float64)).all() and np.isfinite(g.astype(np.float64)).all()
  v64, g64 = poc.restate_vg(case, np.float64)
  ev, eg = float(np.max(pc.col_errors(v64, v))), float(np.max(poc.grad_errors(g64, g)))
  # the float64 restatement within a tenth of the case's bounds (fp64 cases: FP64_BOUND and FP64_GRAD_BOUND; fp32 cases: theirs)
  assert ev <= poc.value_bound(case) / 10 and eg <= poc.grad_bound(case) / 10, (ev, eg)
  if case.dtype == 'fp32':
    assert poc.value_bound(case) < 1e-2 and poc.grad_bound(case) < 1e-2, poc.f32_levels(case)   # (fp32 bounds that still mean something)
  for mutant in sorted(set(poc.MUTANTS) - poc.not_applicable(case)):
    vm, gm = poc.restate_vg(case, np.float64, mutant)
    far_v = float(np.max(pc.col_errors(vm, v))) / pc.FP64_BOUND
    far_g = float(np.max(poc.grad_errors(gm, g))) / poc.FP64_GRAD_BOUND
    assert max(far_v, far_g) >= poc.MUTANT_FACTOR, (mutant, far_v, far_g)


@pytest.mark.parametrize('case', poc.LINEAR_CASES, ids=lambda c: c.id)
def test_linear_paths_have_a_corner_decided_by_more_than_rounding(case):
  corner, margin, chosen = poc.linear_corner(case)
  assert corner.shape == (case.S, case.d) and margin.shape == (case.S,) and chosen.any()
  assert np.all(margin[chosen] >= poc.CORNER_MARGIN * poc.value_bound(case)), margin


def test_the_linear_case_left_out_has_no_path_to_choose():
  assert len(poc.LINEAR_LEFT_OUT) == 1 and len(poc.LINEAR_CASES) == 5
  assert not poc.linear_corner(poc.LINEAR_LEFT_OUT[0])[2].any()


# ---- the Python surface, the two device calls replaced by the restatement ----------------------------------------------------------------
SV, CONST = 0.8, 0.3


def _gp(cls=gp.GP, d=2, tasks=1):
  ds = {k + 1: defs.SubDataset(np.zeros((3, d)), np.zeros((3, 1))) for k in range(tasks)}   # (other sub-datasets: the unbiased scale counts them)
  model = {'constant': CONST, 'lengthscale': helpers.inv_softplus(np.full(d, 0.4)), 'signal_variance': helpers.inv_softplus(SV),
           'noise_variance': helpers.inv_softplus(0.1)}
  return cls(ds, mean.constant, kernel.squared_exponential, defs.GPParams(model=model, config={}), utils.DEFAULT_WARP_FUNC)


def _prior_vg(draws, x):
  """The prior branch of the formulas of include/hbo.h for squared_exponential + constant: ([M, S], [M, S, D])."""
  amp = draws.dev_scale * np.sqrt(2 * (SV + o_eps()) / draws.w.shape[0])
  arg = x @ draws.omega.T + draws.phase[None, :]
  return CONST + amp * np.cos(arg) @ draws.w, -amp * np.einsum('mj,js,jd->msd', np.sin(arg), draws.w, draws.omega)


def o_eps():
  from oracle import hyperbo_oracle as o
  return o.EPS        # default_softplus adds it to the warped signal variance


@pytest.fixture
def on_host(monkeypatch):
  """PathDraws with hbo_sample_paths_grad and hbo_paths_maximize replaced by the restatement (the prior branch) and acq_opt_oracle."""
  calls = []

  def vg(self, xq):
    calls.append(('vg', xq.shape))
    v, g = _prior_vg(self, np.asarray(xq, dtype=np.float64))
    return v.astype(self.dtype), g

  def mx(self, x0, lo, hi, o, state, evals, x, val, status, log):
    calls.append(('max', x0.shape, evals))
    s, r, d = x0.shape
    for si in range(s):
      one = lambda p, si=si: tuple(a[0, si:si + 1] for a in _prior_vg(self, p[None, :]))
      for ri in range(r):
        run = ao.minimise(one, np.asarray(x0[si, ri], dtype=np.float64), lo, hi, self.dtype, max_evals=evals)
        x[si, ri], val[si, ri], status[si, ri] = run.x, -run.f, run.status
        state[si * r + ri, nat.ACQ_OPT_S_EVALS] = len(run.log)

  monkeypatch.setattr(pathwise.PathDraws, '_device_value_and_grad', vg)
  monkeypatch.setattr(pathwise.PathDraws, '_device_maximize', mx)
  return calls


def test_draw_paths_makes_the_contract_draws_and_carries_the_scale(on_host):
  m = _gp(tasks=2)
  with pytest.raises(ValueError, match='random key'):
    m.draw_paths(0)
  with pytest.raises(ValueError, match='HGP'):
    _gp(gp.HGP).draw_paths(0, key=1)
  dr = m.draw_paths(0, num_samples=3, num_features=16, key=5)
  assert isinstance(dr, pathwise.PathDraws) and dr.n == 0 and dr.handle is None and dr.num_samples == 3
  assert dr.dev_scale == float(np.sqrt(2.0))            # T = 2 sub-datasets without the empty one: sqrt(T / (T - 1))
  assert m.draw_paths(0, key=5, unbiased=False).dev_scale == 1.0 and _gp(tasks=1).draw_paths(0, key=5).dev_scale == 1.0
  ls = pathwise.warped_lengthscale(m.params, m.warp_func)
  want = pathwise.draw(np.random.default_rng(5), nat.KERNEL_SE, 2, ls, 16, 3, 0)
  for got, ref in zip((dr.omega, dr.phase, dr.w), want):
    assert got.dtype == np.float64 and np.array_equal(got, ref)
  assert dr.eps is None
  x = np.random.default_rng(1).uniform(size=(5, 2))
  v, g = dr.value_and_grad(x)
  assert v.shape == (5, 3) and g.shape == (5, 3, 2) and np.array_equal(dr.values(x), v)
  with pytest.raises(ValueError, match=r'\[M, 2\]'):
    dr.values(np.zeros((4, 3)))
  for bad in (dict(num_samples=0), dict(num_samples=1025), dict(num_features=0)):
    with pytest.raises(ValueError):
      m.draw_paths(0, key=1, **bad)


def test_stale_draws_are_refused(on_host):
  class Handle:     # what PathDraws reads of a linalg.CacheHandle
    def __init__(self):
      self.n, self.dtype, self.ctx, self.handle = 4, np.dtype(np.float64), None, C.c_void_p(1234)
  h = Handle()
  m = _gp()
  dr = pathwise.PathDraws(m.mean_func, m.cov_func, m.params, m.warp_func, h, 2, np.float64, 2, 8, 3)
  assert dr.n == 4 and dr.eps.shape == (4, 2)
  dr.values(np.zeros((1, 2)))
  h.n = 5
  for call in (lambda: dr.values(np.zeros((1, 2))), lambda: dr.value_and_grad(np.zeros((1, 2))), lambda: dr.maximize(np.zeros((1, 2)))):
    with pytest.raises(ValueError, match='drawn over 4 observations'):
      call()
  h.n, h.handle = 4, C.c_void_p(99)      # re-factorised: another cache of the same size
  with pytest.raises(ValueError, match='the cache has changed'):
    dr.values(np.zeros((1, 2)))


def test_maximize_shapes_segments_and_refusals(on_host):
  dr = _gp().draw_paths(0, num_samples=2, num_features=16, key=7)
  x0 = np.random.default_rng(2).uniform(size=(2, 3, 2))
  x, val, info = dr.maximize(x0, evals=20, opts={'segment': 8})
  assert x.shape == (2, 3, 2) and val.shape == (2, 3) and info['status'].shape == (2, 3) and info['evals'].shape == (2, 3)
  assert np.all(x >= 0) and np.all(x <= 1)
  v0 = np.stack([dr.values(x0[s])[:, s] for s in range(2)])
  v1 = np.stack([dr.values(x[s])[:, s] for s in range(2)])
  assert np.all(v1 >= v0) and np.allclose(v1, val, rtol=0, atol=1e-12)
  segs = [c[2] for c in on_host if c[0] == 'max']
  assert segs and all(s == 8 for s in segs[:-1]) and sum(segs) <= 20 + 8
  xb, _, _ = dr.maximize(x0[0])                       # [R, D]: the same starts for every path
  assert xb.shape == (2, 3, 2)
  for bad in (np.zeros((3, 3, 2)), np.zeros((2, 3, 3)), np.zeros(2), np.zeros((2, 0, 2))):
    with pytest.raises(ValueError, match='x_init'):
      dr.maximize(bad)
  with pytest.raises(ValueError, match='pairs'):
    dr.maximize(np.zeros((2, 2049, 2)))
  with pytest.raises(ValueError):
    dr.maximize(x0, evals=0)


def test_thompson_maximize_takes_the_best_candidates_and_the_best_refinement(on_host, monkeypatch):
  m = _gp()
  xc = np.random.default_rng(3).uniform(size=(12, 2))
  seen = {}
  real = pathwise.PathDraws.maximize

  def spy(self, x_init, bounds=None, opts=None, evals=None):
    seen['draws'], seen['x0'] = self, np.array(x_init)
    seen['out'] = real(self, x_init, bounds=bounds, opts=opts, evals=evals)
    return seen['out']
  monkeypatch.setattr(pathwise.PathDraws, 'maximize', spy)
  got = acfun.thompson_maximize(m, 0, xc, batch_size=3, key=11, num_features=16, starts=4)
  assert got.shape == (3, 2) and got.dtype == np.float64
  dr = seen['draws']
  scores = dr.values(xc)
  for s in range(3):
    order = np.argsort(-scores[:, s], kind='stable')[:4]
    assert np.array_equal(seen['x0'][s], xc[order])                     # the four best candidates, the lower index first among equals
    x, val, _ = seen['out']
    assert np.array_equal(got[s], x[s, int(np.argmax(val[s]))])         # np.argmax: the lower start index among equals
    assert dr.values(got[s][None])[0, s] >= scores[:, s].max()
  assert len([c for c in on_host if c[0] == 'max' and c[1] == (3, 4, 2)]) >= 1 and not [c for c in on_host if c[0] == 'max' and c[1] != (3, 4, 2)]
  # fewer candidates than starts; the same key gives the same suggestion
  two = acfun.thompson_maximize(m, 0, xc[:2], batch_size=1, key=11, num_features=16, starts=4)
  assert seen['x0'].shape == (1, 2, 2) and np.array_equal(two, acfun.thompson_maximize(m, 0, xc[:2], key=11, num_features=16))
  with pytest.raises(ValueError, match='HGP'):
    acfun.thompson_maximize(_gp(gp.HGP), 0, xc, key=1)
  with pytest.raises(ValueError):
    acfun.thompson_maximize(m, 0, xc, batch_size=0, key=1)
  with pytest.raises(ValueError):
    acfun.thompson_maximize(m, 0, np.zeros((0, 2)), key=1)


def test_thompson_continuous_is_a_suggesting_strategy(on_host):
  tc = acfun.thompson_continuous
  assert tc.__name__ == 'thompson_continuous' and callable(tc) and hasattr(tc, 'suggest')
  assert not hasattr(tc, 'value_and_grad') and not hasattr(tc, 'maximize') and tc not in acfun._BO_DEVICE
  # the pool strategies stay as they are
  assert not hasattr(acfun.thompson_sampling, 'suggest') and not hasattr(acfun.thompson_sampling, 'maximize')
  m = _gp()
  xc = np.random.default_rng(4).uniform(size=(9, 2))
  got = tc.suggest(model=m, sub_dataset_key=0, x_candidates=xc, key=np.random.default_rng(6))
  want = acfun.thompson_maximize(m, 0, xc, key=np.random.default_rng(6), num_features=tc.num_features, starts=tc.starts)
  assert got.shape == (1, 2) and np.array_equal(got, want)


def test_bayesopt_asks_a_suggesting_strategy_for_its_point(on_host):
  m = _gp()
  seen, asked = [], []

  class Strategy:
    __name__ = 'corner_seeker'

    def __call__(self, **kw):
      raise AssertionError('a strategy with `suggest` scores its candidates itself')

    def suggest(self, *, model, sub_dataset_key, x_candidates, key):
      seen.append((np.array(x_candidates), key, model.has_observations(sub_dataset_key)))
      return np.vstack([x_candidates.max(axis=0), np.zeros(x_candidates.shape[1])])

  def oracle(x):
    asked.append(np.array(x[0]))
    return np.zeros((1, 1))

  rng = np.random.default_rng(2)
  bayesopt.bayesopt(rng, m, 0, oracle, Strategy(), 3, lambda r, d: r.uniform(size=(8, d)))
  assert len(seen) == 3 and len(asked) == 3 and m.dataset[0].x.shape[0] == 3
  assert [s[2] for s in seen] == [False, True, True]                     # the first iteration is the prior branch
  for (xs, key, _), xa in zip(seen, asked):
    assert key is rng and xs.shape == (8, 2) and np.array_equal(xa, xs.max(axis=0))


def test_bayesopt_with_thompson_continuous_from_an_empty_sub_dataset(on_host, monkeypatch):
  """The loop end to end on the host: every iteration is served by the (replaced) prior-branch calls, because the model is drawn
  again after each append and the replacement ignores the observations -- what is checked is the plumbing, not the posterior."""
  m = _gp()
  monkeypatch.setattr(gp.GP, 'has_observations', lambda self, key: False)
  sub = bayesopt.bayesopt(np.random.default_rng(5), m, 0, lambda x: np.sum(x, axis=1, keepdims=True),
                          acfun.ThompsonContinuous(num_features=16, starts=2), 3, lambda r, d: r.uniform(size=(6, d)))
  assert sub.x.shape == (3, 2) and np.all(sub.x >= 0) and np.all(sub.x <= 1)
  assert len([c for c in on_host if c[0] == 'max']) >= 3
