"""Log expected improvement on the device (run with `-m gpu` on an MI355X): hbo_acq_logei, hbo_logei_grad_samples, hbo_logei_maximize and
acfun.log_ei.  Cases, references, bounds and mutants: tests/logei_cases.py, judged on its own by tests/test_logei_cases_host.py.  Every
comparison is per query, never max-norm; u is placed as tests/test_gpu_acq_tails.py places it: target = mu_q - u sd_q from the device's
own hbo_predict.  Each test prints its worst ratio to its bound (-s); profiles/logei_errors.md keeps them.

Bounds (logei_cases.py): DEVICE_FACTOR = 8 times the constants the float64 restatement needs against mpmath, in units of
eps64 (1 + u^2), absolute for the value (plus eps64 |log sd|); an fp32 result adds the rounding of the output; comparisons across two
routes to mu, var (or against the oracle's posterior) add the posterior's own tolerance through the value's two slopes.  Gradients:
1e-7 (1 + u^2) of the query's largest component in fp64; fp32: 2e-2 (1 + u^2), at queries with |u| <= 3.25 only.

Two dispatch paths, as for EI and MES: a call whose caches all have n <= 128 takes acq_small_kernel, and the blocked kernels are
reachable for it through the test hook's force_blocked only; they sum in another order.  The public call and the hook without
force_blocked are held to identical bits; the forced path to the siblings' bound."""
import ctypes as C
import types

import mpmath as mp
import numpy as np
import pytest

import acq_opt_oracle as ao
import helpers
import logei_cases as lc
import mes_cases as mc

pytestmark = pytest.mark.gpu
PD = C.POINTER(C.c_double)
SCALE = lc.SCALE
FORCED_GRAD_TOL = 10 * 3.211e-13      # tests/test_gpu_acq_blocked.py: LOOP_GRAD_TOL


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
  return a.ctypes.data_as(PD)


class Dev:
  """The S (model, factorised cache) pairs of a logei_cases.problem on the device and the calls the tests make on them.  Close it."""

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
            (C.c_double * s)(*[float(noises[i]) for i in sel]), (C.c_double * s)(*[float(t) for t in targets]))

  def predict(self, xq, s=0, cache=True):
    nat = self.nv.nat
    mu, var = np.empty((xq.shape[0], 1), dtype=self.dtype), np.empty((xq.shape[0], 1), dtype=self.dtype)
    self.ctx.check(nat.lib().hbo_predict(self.ctx.handle, self.built[s].ref(), self.handles[s].handle if cache else None, nat.ptr(xq), xq.shape[0], 0,
                                         nat.ptr(mu), nat.ptr(var)), allow_not_pd=False)
    return mu[:, 0], var[:, 0]

  def acq(self, xq, target, s=0, add_noise=0.0, scale=SCALE, cache=True):
    """hbo_acq_logei: [M] in the model dtype."""
    nat = self.nv.nat
    out = np.full((xq.shape[0], 1), 7.0, dtype=self.dtype)
    self.ctx.check(nat.lib().hbo_acq_logei(self.ctx.handle, self.built[s].ref(), self.handles[s].handle if cache else None, nat.ptr(xq), xq.shape[0],
                                           float(target), float(add_noise), float(scale), nat.ptr(out)), allow_not_pd=False)
    return out[:, 0]

  def ei(self, xq, target, s=0, add_noise=0.0, scale=SCALE):
    """hbo_acq with EI: [M] in the model dtype."""
    nat = self.nv.nat
    out = np.full((xq.shape[0], 1), 7.0, dtype=self.dtype)
    self.ctx.check(nat.lib().hbo_acq(self.ctx.handle, self.built[s].ref(), self.handles[s].handle, nat.ptr(xq), xq.shape[0], nat.ACQ_EI, float(target),
                                     float(add_noise), float(scale), nat.ptr(out)), allow_not_pd=False)
    return out[:, 0]

  def grad(self, xq, targets, sel=None, noises=None, scale=SCALE, force=None, chunk=0):
    """hbo_logei_grad_samples (force None) or its hook: (values [S, M] model dtype, gradients [S, M, D], fp64 values or None)."""
    nat = self.nv.nat
    sel = list(range(len(self.built))) if sel is None else list(sel)
    structs, caches, nse, tg = self._args(sel, [0.0] * len(self.built) if noises is None else noises, np.ravel(targets))
    m = xq.shape[0]
    val, grad = np.full((len(sel), m), 7.0, dtype=self.dtype), np.full((len(sel), m, self.d), 7.0)
    if force is None:
      self.ctx.check(nat.lib().hbo_logei_grad_samples(self.ctx.handle, structs, len(sel), caches, nat.ptr(xq), m, tg, nse, float(scale), nat.ptr(val),
                                                      _dp(grad)), allow_not_pd=False)
      return val, grad, None
    v64 = np.full((len(sel), m), 7.0)
    self.ctx.check(nat.lib().hbo_probe_logei_grad_samples64(self.ctx.handle, structs, len(sel), caches, nat.ptr(xq), m, tg, nse, float(scale), nat.ptr(val),
                                                            _dp(grad), int(force), int(chunk), _dp(v64)), allow_not_pd=False)
    return val, grad, v64

  def maximize(self, x0, targets, lo, hi, evals, state=None, opts=None, sel=None, noises=None, ei=False):
    """One hbo_logei_maximize call (ei: hbo_acq_maximize with EI): (log [evals, R], x_out, val_out, status, state)."""
    nat = self.nv.nat
    o = nat.AcqOptOpts(**(opts or self.nv.acfun.ACQ_OPT_DEFAULTS))
    sel = list(range(len(self.built))) if sel is None else list(sel)
    s, r = len(sel), x0.shape[0]
    structs, caches, nse, tg = self._args(sel, [0.0] * len(self.built) if noises is None else noises, np.ravel(targets))
    ns = nat.lib().hbo_acq_opt_state_doubles(self.d, o.memory)
    state = np.zeros((r, ns)) if state is None else state
    x, val, status = np.full((r, self.d), 7.0), np.full(r, 7.0), np.full(r, 7, dtype=np.int32)
    log = np.zeros((evals, r), dtype=nat.ACQ_OPT_EVAL_DTYPE)
    tail = (nse, SCALE, C.byref(o), nat.ptr(state), evals, nat.ptr(x), nat.ptr(val), nat.ptr(status), nat.ptr(log))
    if ei:
      rc = nat.lib().hbo_acq_maximize(self.ctx.handle, structs, s, caches, nat.ptr(x0), r, nat.ptr(lo), nat.ptr(hi), nat.ACQ_EI, tg, *tail)
    else:
      rc = nat.lib().hbo_logei_maximize(self.ctx.handle, structs, s, caches, nat.ptr(x0), r, nat.ptr(lo), nat.ptr(hi), tg, *tail)
    self.ctx.check(rc, allow_not_pd=False)
    return log, x, val, status, state


def _u_of(target, mu, sd):
  return ((mu.astype(np.longdouble) - np.longdouble(target)) / sd.astype(np.longdouble)).astype(np.float64)


def _device_sd(var, dtype, add_noise=0.0):
  t = np.dtype(dtype).type
  return np.sqrt((var + t(add_noise)) * t(SCALE))


def _exact_value(u, sd):
  """log sd + log h(u) as a float, from mpmath."""
  return float(mp.log(mp.mpf(float(sd))) + mp.mpf(lc.exact_terms(float(u))[0]))


def _hit(u_row, u):
  return abs(u_row - u) <= 1e-6 * max(1.0, abs(u))


# ---- the epilogue alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['fp64', 'fp32'])
@pytest.mark.parametrize('n_obs', [0, 300], ids=['prior', 'n300'])
def test_pool_epilogue_against_mpmath_at_the_devices_own_posterior(gpu_ctx, n_obs, dtype):
  """hbo_acq_logei over M = 600 queries in chunks of post_chunk = 256 against mpmath at the device's own mu, var (hbo_predict: the same
  routine, identical bits) and sd formed in the model dtype as the kernel forms it.  One call per u of U, its target aimed at one row;
  that row and every 37th row of the call are checked at their own u (all 600 rows for u = -3).  A second run with post_chunk at its
  default gives the same bits.  n_obs = 0: the prior branch."""
  case = lc.Case('squared_exponential', 'constant', (300,), 3, 9, dtype)
  p = lc.problem(case)
  xq = np.ascontiguousarray(np.random.default_rng(11).uniform(size=(600, 3)).astype(p.dtype))
  dev = Dev(gpu_ctx, p)
  old = gpu_ctx.get_option('post_chunk')
  try:
    cache = n_obs > 0
    gpu_ctx.set_option('post_chunk', 256)
    mu, var = dev.predict(xq, cache=cache)
    assert np.all(var > 0)
    sd = _device_sd(var, p.dtype)
    worst, reached = (0.0, None), set()
    for k, u in enumerate(lc.U):
      qk = (k * 37 + 5) % 600
      target = float(mu[qk]) - u * float(sd[qk])
      out = dev.acq(xq, target, cache=cache)
      assert out.dtype == p.dtype
      ur = _u_of(target, mu, sd)
      rows = range(600) if u == -3.0 else sorted({qk} | set(range(0, 600, 37)))
      for q in rows:
        if not (-3.1e7 <= ur[q] <= 1.1e3):
          continue
        exact = _exact_value(ur[q], sd[q])
        bound = lc.value_bound(ur[q], float(sd[q]), float(var[q]), p.dtype, value=exact)
        r = abs(float(out[q]) - exact) / bound if np.isfinite(out[q]) else np.inf
        if q == qk and _hit(ur[q], u):
          reached.add(u)
        if r > worst[0]:
          worst = (r, (q, float(ur[q]), float(out[q]), exact))
        assert r <= 1.0, (q, ur[q], float(out[q]), exact, r)
      if u == -3.0:
        gpu_ctx.set_option('post_chunk', old)
        again = dev.acq(xq, target, cache=cache)
        gpu_ctx.set_option('post_chunk', 256)
        assert same_bits(again, out)
    print(f'\nlogei: epilogue {dtype} n={n_obs}: worst ratio to the bound {worst[0]:.3e} at {worst[1]}')
    assert reached == set(lc.U), sorted(set(lc.U) - reached)
  finally:
    gpu_ctx.set_option('post_chunk', old)
    dev.close()


def test_a_pool_where_ei_underflows(gpu_ctx):
  """An fp32 pool whose rows all have u < -15: hbo_acq with EI returns 0 for every row (the premise: existing behaviour), so its argmax is
  row 0 whatever the rows hold.  hbo_acq_logei's argmax is the argmax of the mpmath values at the device's own posterior, and no two rows
  whose mpmath values differ by more than their bounds are ordered wrongly."""
  p = lc.problem(lc.Case('squared_exponential', 'constant', (300,), 3, 9, 'fp32'))
  xq = np.ascontiguousarray(np.random.default_rng(12).uniform(size=(160, 3)).astype(p.dtype))
  dev = Dev(gpu_ctx, p)
  try:
    mu, var = dev.predict(xq)
    sd = _device_sd(var, p.dtype)
    target = float(np.max(mu.astype(np.float64) + 15.5 * sd.astype(np.float64)))
    u = _u_of(target, mu, sd)
    if int(np.argmax([_exact_value(u[q], sd[q]) for q in range(160)])) == 0:     # keep the best row off index 0, where an all-zero argmax lands
      xq = np.ascontiguousarray(xq[::-1])
      mu, var, sd, u = mu[::-1].copy(), var[::-1].copy(), sd[::-1].copy(), u[::-1].copy()
      assert same_bits(dev.predict(xq)[0], mu)
    assert np.all(u < -15.0)
    ei = dev.ei(xq, target)
    assert np.all(ei == 0.0) and int(np.argmax(ei)) == 0
    out = dev.acq(xq, target)
    assert np.all(np.isfinite(out)) and np.all(out < 0.0)
    exact = np.array([_exact_value(u[q], sd[q]) for q in range(160)])
    bound = np.array([lc.value_bound(u[q], float(sd[q]), float(var[q]), p.dtype, value=exact[q]) for q in range(160)])
    assert np.all(np.abs(out - exact) <= bound)
    best = int(np.argmax(exact))
    clear = exact[best] - np.delete(exact, best) > bound[best] + np.delete(bound, best)
    print(f'\nlogei: underflow pool: u in [{u.min():.2f}, {u.max():.2f}], argmax {best} (EI: 0), clear of {int(clear.sum())} / 159 rows')
    assert best != 0 and out[best] >= np.max(out[np.delete(np.arange(160), best)[clear]])
    if clear.all():
      assert int(np.argmax(out)) == best
    apart = exact[:, None] - exact[None, :] > bound[:, None] + bound[None, :]
    assert np.all(out[:, None][apart.nonzero()[0], 0] > out[apart.nonzero()[1]]) and apart.sum() > 160
  finally:
    dev.close()


# ---- the gradient entry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['fp64', 'fp32'])
@pytest.mark.parametrize('n_obs', [128, 300])
def test_gradient_entry_value_against_mpmath(gpu_ctx, n_obs, dtype):
  """The fp64 value of hbo_logei_grad_samples (through the probe) at each u of U against mpmath at hbo_predict's mu, var.  The two reach
  mu, var by different routes (model-dtype sums over the product's column squares / fp64 sums over l = W k): the bound adds the
  posterior term, with d_mu, d_v as test_gpu_parity.py holds the posterior to them."""
  case = lc.Case('matern52', 'constant', (n_obs,), 3, 9, dtype)
  p = lc.problem(case)
  dev = Dev(gpu_ctx, p)
  try:
    mu, var = dev.predict(p.xq)
    sd = _device_sd(var, p.dtype)
    d_mu, d_v = lc.posterior_tolerances(p.dtype, p.smp[0].mu, p.smp[0].var)
    worst, reached = (0.0, None), set()
    for k, u in enumerate(lc.U):
      qk = (k * 5) % case.M
      target = float(mu[qk]) - u * float(sd[qk])
      val, grad, v64 = dev.grad(p.xq, [target], force=0)
      pub = dev.grad(p.xq, [target])
      assert same_bits(pub[0], val) and same_bits(pub[1], grad) and same_bits(v64.astype(p.dtype), val)
      ur = _u_of(target, mu, sd)
      for q in range(case.M):
        if not (-3.1e7 <= ur[q] <= 1.1e3):
          continue
        if q == qk and _hit(ur[q], u):
          reached.add(u)
        exact = _exact_value(ur[q], sd[q])
        bound = lc.value_bound(ur[q], float(sd[q]), float(var[q]), np.float64, d_mu, d_v)
        r = abs(float(v64[0, q]) - exact) / bound if np.isfinite(v64[0, q]) else np.inf
        if r > worst[0]:
          worst = (r, (q, float(ur[q])))
        assert r <= 1.0 and np.all(np.isfinite(grad[0, q])), (q, ur[q], float(v64[0, q]), exact, r)
    print(f'\nlogei: gradient-entry value {dtype} n={n_obs}: worst ratio to the bound {worst[0]:.3e} at {worst[1]}')
    assert reached == set(lc.U)
  finally:
    dev.close()


@pytest.mark.parametrize('case', lc.CASES, ids=lambda c: c.id)
def test_value_and_gradient_against_the_oracle(gpu_ctx, case):
  """hbo_logei_grad_samples per query and per component against the oracle (its posterior and the posterior's derivative), every sample
  of the call against its own reference; hbo_acq_logei of every sample against the same values.  The MLP cases run the forward and
  backward pass inside the pair's workgroup."""
  p = lc.problem(case)
  dev = Dev(gpu_ctx, p)
  try:
    val, grad, _ = dev.grad(p.xq, p.targets, noises=p.noises)
    assert val.dtype == p.dtype and grad.dtype == np.float64 and val.shape == (case.S, case.M) and grad.shape == (case.S, case.M, case.d)
    wv = wg = wa = 0.0
    checked = 0
    for s, sm in enumerate(p.smp):
      rv, rg, u = lc.oracle_value_and_grad(sm, p.xq, p.targets[s])
      d_mu, d_v = lc.posterior_tolerances(p.dtype, sm.mu, sm.var)
      pool = dev.acq(p.xq, p.targets[s], s=s, add_noise=sm.noise)
      for q in range(case.M):
        bound = lc.value_bound(u[q], float(sm.sd[q]), float(sm.var[q] + sm.noise), p.dtype, d_mu, d_v, value=rv[q])
        r = abs(float(val[s, q]) - rv[q]) / bound
        ra = abs(float(pool[q]) - rv[q]) / bound
        wv, wa = max(wv, r), max(wa, ra)
        assert r <= 1.0 and ra <= 1.0, (s, q, u[q], float(val[s, q]), float(pool[q]), rv[q], r, ra)
        if case.dtype == 'fp32' and abs(u[q]) > 3.25:
          continue
        checked += 1
        rgq = float(np.max(np.abs(grad[s, q] - rg[q])) / (lc.grad_tol(u[q], p.dtype) * np.max(np.abs(rg[q]))))
        wg = max(wg, rgq)
        assert rgq <= 1.0, (s, q, u[q], grad[s, q], rg[q], rgq)
    print(f'\nlogei: {case.id}: worst ratio to the oracle bounds: value {wv:.3e}, pool value {wa:.3e}, gradient {wg:.3e} ({checked} queries)')
    assert checked >= case.S                                    # query 0 of every sample sits at u = -2 by construction
  finally:
    dev.close()


def test_the_devices_own_value_against_central_differences(gpu_ctx):
  """d value / dx of three queries against central differences of the device's own fp64 value, step 1e-5: truncation ~ step^2 |f'''| / 6
  and rounding ~ eps64 |f| / step are both ~1e-10 of a value of order one; the bound is 1e-6 of the query's largest component."""
  case = lc.Case('matern52', 'linear', (129,), 3, 3, 'fp64')
  p = lc.problem(case)
  dev = Dev(gpu_ctx, p)
  try:
    _, grad, _ = dev.grad(p.xq, p.targets, noises=p.noises, force=0)
    step = 1e-5
    pts = np.repeat(p.xq, 2 * case.d, axis=0)
    for q in range(3):
      for d in range(case.d):
        pts[(q * case.d + d) * 2, d] += step
        pts[(q * case.d + d) * 2 + 1, d] -= step
    _, _, v64 = dev.grad(np.ascontiguousarray(pts), p.targets, noises=p.noises, force=0)
    fd = ((v64[0, 0::2] - v64[0, 1::2]) / (pts[0::2] - pts[1::2])[np.arange(3 * case.d), np.tile(np.arange(case.d), 3)]).reshape(3, case.d)
    worst = max(float(np.max(np.abs(fd[q] - grad[0, q])) / (1e-6 * np.max(np.abs(grad[0, q])))) for q in range(3))
    print(f'\nlogei: central differences: worst ratio to the bound {worst:.3e}')
    assert worst <= 1.0, (fd, grad[0])
  finally:
    dev.close()


@pytest.mark.parametrize('dtype', ['fp64', 'fp32'])
def test_a_row_does_not_depend_on_what_shares_the_call(gpu_ctx, dtype):
  p = lc.problem(lc.Case('matern32', 'constant', (100, 300, 100), 3, 9, dtype))
  dev = Dev(gpu_ctx, p)
  try:
    t, ns = p.targets, p.noises
    val, grad, v64 = dev.grad(p.xq, t, noises=ns, force=0)
    assert np.isfinite(val).all() and np.isfinite(grad).all() and same_bits(v64.astype(p.dtype), val)
    again = dev.grad(p.xq, t, noises=ns, force=0)
    assert all(same_bits(a, b) for a, b in zip(again, (val, grad, v64)))                   # identical calls, identical bits
    pub = dev.grad(p.xq, t, noises=ns)
    assert same_bits(pub[0], val) and same_bits(pub[1], grad)
    # a sample alone, a query alone at another place, another chunking: the blocked kernels throughout (sample 1 has n = 300)
    one = dev.grad(np.ascontiguousarray(p.xq[4:5]), t[1:2], sel=[1], noises=ns, force=0)
    assert same_bits(one[0][0], val[1, 4:5]) and same_bits(one[1][0], grad[1, 4:5]) and same_bits(one[2][0], v64[1, 4:5])
    cut = dev.grad(p.xq, t, noises=ns, force=0, chunk=2)
    assert all(same_bits(a, b) for a, b in zip(cut, (val, grad, v64)))
    moved = dev.grad(np.ascontiguousarray(p.xq[::-1]), t, noises=ns, force=0, chunk=4)
    assert same_bits(np.ascontiguousarray(moved[0][:, ::-1]), val) and same_bits(np.ascontiguousarray(moved[1][:, ::-1]), grad)
    # samples 0 and 2 alone (n = 100): the one-launch path; forced through the blocked kernels they keep the bits they had beside n = 300
    small = dev.grad(p.xq, t[[0, 2]], sel=[0, 2], noises=ns, force=0)
    forced = dev.grad(p.xq, t[[0, 2]], sel=[0, 2], noises=ns, force=1)
    assert same_bits(forced[0], val[[0, 2]]) and same_bits(forced[1], grad[[0, 2]]) and same_bits(forced[2], v64[[0, 2]])
    pub = dev.grad(p.xq, t[[0, 2]], sel=[0, 2], noises=ns)
    assert same_bits(pub[0], small[0]) and same_bits(pub[1], small[1])                     # the public call is the one-launch path
    alone = dev.grad(np.ascontiguousarray(p.xq[2:3]), t[2:3], sel=[2], noises=ns, force=0)
    assert same_bits(alone[0][0], small[0][1, 2:3]) and same_bits(alone[1][0], small[1][1, 2:3])
    # the two paths against each other: the siblings' bound (module docstring)
    ev = float(np.max(np.abs(small[2] - forced[2]) / np.maximum(np.abs(forced[2]), 1e-300)))
    eg = max(float(np.max(np.abs(small[1][i] - forced[1][i])) / max(np.max(np.abs(forced[1][i])), 1e-3)) for i in range(2))
    print(f'\nlogei: one launch against the blocked kernels at n = 100, {dtype}: value {ev:.3e} relative, gradient {eg:.3e}')
    if dtype == 'fp64':
      assert ev <= 1e-9 and eg <= FORCED_GRAD_TOL, (ev, eg)
  finally:
    dev.close()


@pytest.mark.parametrize('dtype', ['fp64', 'fp32'])
def test_no_variance_and_nan_rules(gpu_ctx, dtype):
  """v2 = (var + add_noise) * scale <= 0 -- forced through add_noise, and through a posterior variance that is itself 0 with add_noise = 0
  (mes_cases.zero_variance_problem) --: value log(mu - target) and d value / dx = d mu / dx / (mu - target) above the target, -inf and a
  zero gradient at or below it, in every entry point and on both dispatch paths; a NaN v2 stays NaN."""
  tol = 1e-6 if dtype == 'fp64' else 2e-3            # the posterior's two routes to mu (posterior_tolerances, relative to |mu| <= ~2)
  for n in (100, 300):
    z = mc.zero_variance_problem(n, dtype)
    dev = Dev(gpu_ctx, z)
    try:
      mu, var = dev.predict(z.xq)
      assert var[0] == 0.0 and np.isfinite(mu[0]) and np.all(var[1:] > 0.0)
      below, above = float(mu[0]) - 1.0, float(mu[0]) + 0.5
      out = dev.acq(z.xq, below)
      assert abs(float(out[0]) - np.log(float(mu[0]) - below)) <= 4 * np.finfo(z.dtype).eps and np.all(np.isfinite(out))
      assert dev.acq(z.xq, above)[0] == -np.inf and dev.acq(z.xq, float(mu[0]))[0] == -np.inf
      assert dev.acq(z.xq, above, cache=False)[0] == -np.inf                                    # prior: k(0, 0) = 0, mu = the constant
      for force in (0, 1):
        val, grad, v64 = dev.grad(z.xq, [below], force=force)
        assert abs(v64[0, 0]) <= tol and np.all(np.isfinite(grad[0])) and np.all(np.isfinite(v64[0, 1:])), (n, force, v64[0, 0])
        val, grad, v64 = dev.grad(z.xq, [above], force=force)
        assert val[0, 0] == -np.inf and v64[0, 0] == -np.inf and np.all(grad[0, 0] == 0.0), (n, force, val[0, 0], grad[0, 0])
        assert np.all(np.isfinite(val[0, 1:])) and np.all(np.isfinite(grad[0, 1:])) and np.any(grad[0, 1:] != 0.0)
      # every row through add_noise: the rule row by row, against the device's own mu
      t = float(np.median(mu))
      out = dev.acq(z.xq, t, add_noise=-1e3)
      up = mu.astype(np.float64) > t
      assert np.all(out[~up] == -np.inf) and np.all(np.abs(out[up] - np.log(mu[up].astype(np.float64) - t)) <= 4 * np.finfo(z.dtype).eps * (1 + np.abs(out[up])))
      val, grad, v64 = dev.grad(z.xq, [t], noises=[-1e3], force=0)
      clear = np.abs(mu.astype(np.float64) - t) > 10 * tol
      assert np.all(v64[0][clear & ~up] == -np.inf) and np.all(grad[0][clear & ~up] == 0.0) and np.all(np.isfinite(v64[0][clear & up]))
      out = dev.acq(z.xq, t, add_noise=np.nan)
      val, grad, _ = dev.grad(z.xq, [t], noises=[np.nan])
      assert np.all(np.isnan(out)) and np.all(np.isnan(val)) and np.all(np.isnan(grad)), n
      assert np.all(np.isnan(dev.acq(z.xq, t, add_noise=np.nan, cache=False)))                   # the prior branch
    finally:
      dev.close()


def test_refusals_touch_no_output(gpu_ctx):
  """The prior branch and a Kumaraswamy-warped model: HBO_ERR_UNSUPPORTED from the gradient entry and the maximiser, outputs untouched;
  a target that is not finite: HBO_ERR_ARG."""
  nv = _nv()
  nat = nv.nat
  rng = np.random.default_rng(197)
  d, wf = 3, nv.utils.DEFAULT_WARP_FUNC
  xq = rng.uniform(size=(2, d))
  err = lambda: (nat.lib().hbo_last_error(gpu_ctx.handle) or b'').decode()
  opts = nat.AcqOptOpts(**ao.DEFAULTS)
  ns = nat.lib().hbo_acq_opt_state_doubles(d, opts.memory)

  def calls(b, h, target=0.5):
    structs, caches = (nat.Model * 1)(b.struct), (C.c_void_p * 1)(h.handle if h is not None else None)
    tg, nse = (C.c_double * 1)(target), (C.c_double * 1)(0.1)
    val, grad = np.full((1, 2, 1), 7.0), np.full((1, 2, d), 7.0)
    rc1 = nat.lib().hbo_logei_grad_samples(gpu_ctx.handle, structs, 1, caches, nat.ptr(xq), 2, tg, nse, SCALE, nat.ptr(val), _dp(grad))
    m1 = err()
    state, x, v, status = np.zeros((2, ns)), np.full((2, d), 7.0), np.full(2, 7.0), np.full(2, 7, dtype=np.int32)
    rc2 = nat.lib().hbo_logei_maximize(gpu_ctx.handle, structs, 1, caches, nat.ptr(xq), 2, None, None, tg, nse, SCALE, C.byref(opts), nat.ptr(state), 4,
                                       nat.ptr(x), nat.ptr(v), nat.ptr(status), None)
    m2 = err()
    untouched = np.all(val == 7.0) and np.all(grad == 7.0) and np.all(x == 7.0) and np.all(v == 7.0) and np.all(status == 7) and not state.any()
    return rc1, m1, rc2, m2, untouched

  handles = []
  try:
    plain = helpers.make_model(rng, 'constant', False, d)
    x, y = helpers.synthetic_task(rng, 130, d)
    pn = nv.defs.GPParams(model=plain, config={})
    b = nv.hmodel.BuiltModel(nv.mean.constant, nv.kernel.matern52, pn, wf, np.float64, d)
    h = nv.linalg.factor(nv.mean.constant, nv.kernel.matern52, pn, x, y, wf, ctx=gpu_ctx); handles.append(h)
    rc1, m1, rc2, m2, untouched = calls(b, h)
    assert rc1 == nat.HBO_OK and rc2 == nat.HBO_OK and not untouched, (rc1, m1, rc2, m2)                   # served ...
    rc1, m1, rc2, m2, untouched = calls(b, None)
    assert rc1 == rc2 == nat.HBO_ERR_UNSUPPORTED and 'prior branch' in m1 and 'prior branch' in m2 and untouched, (rc1, m1, rc2, m2)
    rc1, m1, rc2, m2, untouched = calls(b, h, target=np.inf)
    assert rc1 == rc2 == nat.HBO_ERR_ARG and 'not finite' in m1 and 'not finite' in m2 and untouched
    km = dict(plain); km['kumar_params'] = {'a': np.full(d, 0.3), 'b': np.full(d, -0.2)}
    pk = nv.defs.GPParams(model=km, config={})
    bk = nv.hmodel.BuiltModel(nv.mean.constant, nv.kernel.matern52_kumar, pk, wf, np.float64, d)
    hk = nv.linalg.factor(nv.mean.constant, nv.kernel.matern52_kumar, pk, x, y, wf, ctx=gpu_ctx); handles.append(hk)
    rc1, m1, rc2, m2, untouched = calls(bk, hk)
    assert rc1 == rc2 == nat.HBO_ERR_UNSUPPORTED and 'Kumaraswamy' in m1 and 'Kumaraswamy' in m2 and untouched, (rc1, m1, rc2, m2)
  finally:
    for h in handles:
      h.close()


# ---- the maximiser --------------------------------------------------------------------------------------------------------------
def _oracle_combined(p):
  """x [D] -> (vals [1], grads [1, D]): the oracle's LogEI combined over the samples of p, for acq_opt_oracle.minimise."""
  def vg(x):
    rows = [lc.oracle_value_and_grad(sm, np.asarray(x, dtype=np.float64)[None, :], t) for sm, t in zip(p.smp, p.targets)]
    v, g = lc.combine([r[0][0] for r in rows], [r[1][0] for r in rows])
    return np.array([v]), g[None, :]
  return vg


@pytest.mark.parametrize('S', [1, 3])
@pytest.mark.parametrize('n', [60, 300])
def test_maximiser(gpu_ctx, n, S):
  """R = 4 starts, under the rules of test_gpu_mes.py::test_maximiser: val_out is the combination (logei_cases.combine, to the bit for
  S = 1 and to the libraries' exp / log otherwise) of the gradient entry's fp64 values at x_out; 48 evaluations in one call equal
  7 + 41 in two (state, log, outputs, to the bit); every iterate stays inside the box; the value at the end is at least the value at
  the start.  Against acq_opt_oracle.minimise driven by the oracle's combined value and gradient from the same starts: the device ends
  no lower than the oracle-driven run by more than 1e-6 max(1, |f|) -- both stop once a step gains no more than ftol |f| = 2.2e-9 |f|,
  so what either leaves on the table is a few such gains."""
  p = lc.problem(lc.Case('matern52', 'constant', (n,) * S, 3, 4, 'fp64'))
  dev = Dev(gpu_ctx, p)
  try:
    lo, hi = np.full(3, 0.25), np.full(3, 0.75)
    x0 = np.ascontiguousarray(lo + (hi - lo) * np.random.default_rng(n + S).uniform(size=(4, 3)))
    x0[0] = [0.25, 0.75, 0.5]                                   # a start on the boundary
    run = lambda e, **kw: dev.maximize(x0, p.targets, lo, hi, e, noises=p.noises, **kw)
    log, x, val, status, state = run(48)
    la, xa, va, sa, sta = run(7)
    lb, xb, vb, sb, stb = run(41, state=sta.copy())
    assert same_bits(np.concatenate([la, lb]), log) and same_bits(xb, x) and same_bits(vb, val) and same_bits(sb, status) and same_bits(stb, state)
    assert np.all(np.isfinite(val)) and np.all((x >= lo) & (x <= hi))
    nat = dev.nv.nat
    assert np.all(log['kind'][0] == nat.ACQ_OPT_START) and np.any(log['kind'] == nat.ACQ_OPT_MAIN)
    _, _, v_end = dev.grad(np.ascontiguousarray(x), p.targets, noises=p.noises, force=0)
    _, _, v_start = dev.grad(x0, p.targets, noises=p.noises, force=0)
    comb = lambda v: np.array([lc.combine(v[:, r])[0] for r in range(4)])
    if S == 1:
      assert same_bits(comb(v_end), val) and same_bits(-log['value'][0], comb(v_start))
    assert np.all(np.abs(comb(v_end) - val) <= 8 * lc.EPS64 * (1.0 + np.abs(val))), (comb(v_end), val)
    assert np.all(np.abs(-log['value'][0] - comb(v_start)) <= 8 * lc.EPS64 * (1.0 + np.abs(comb(v_start))))
    assert np.all(val >= comb(v_start) - 8 * lc.EPS64 * (1.0 + np.abs(val))), (val, comb(v_start))
    vg = _oracle_combined(p)
    gap = []
    for r in range(2):                                          # (the oracle at n = 300, S = 3 costs a second per start)
      ref = ao.minimise(vg, x0[r], lo, hi)
      gap.append(float((-ref.f - val[r]) / max(1.0, abs(ref.f))))
      assert val[r] >= -ref.f - 1e-6 * max(1.0, abs(ref.f)), (r, val[r], -ref.f, x[r], ref.x, status[r], ref.status)
    print(f'\nlogei: maximiser n={n} S={S}: status {status.tolist()}, value {comb(v_start).tolist()} -> {val.tolist()}; oracle run minus device, relative: {gap}')
  finally:
    dev.close()


def test_maximiser_with_a_sample_whose_row_is_minus_infinity(gpu_ctx):
  """S = 3 with the second sample's target at 1e300 (u^2 overflows: its row is -inf with a zero gradient): the run is the run over samples
  0 and 2 alone, its value shifted by log(2 / 3)."""
  p = lc.problem(lc.Case('matern52', 'constant', (60, 60, 60), 3, 4, 'fp64'))
  dev = Dev(gpu_ctx, p)
  try:
    lo, hi = np.full(3, 0.25), np.full(3, 0.75)
    x0 = np.ascontiguousarray(lo + (hi - lo) * np.random.default_rng(31).uniform(size=(4, 3)))
    t3 = np.array([p.targets[0], 1e300, p.targets[2]])
    val3, grad3, v64 = dev.grad(x0, t3, noises=p.noises, force=0)
    assert np.all(v64[1] == -np.inf) and np.all(grad3[1] == 0.0) and np.all(np.isfinite(v64[[0, 2]]))
    _, x3, v3, s3, _ = dev.maximize(x0, t3, lo, hi, 48, noises=p.noises)
    _, x2, v2, s2, _ = dev.maximize(x0, t3[[0, 2]], lo, hi, 48, noises=p.noises, sel=[0, 2])
    print(f'\nlogei: -inf row: status {s3.tolist()} / {s2.tolist()}, |dx| {float(np.max(np.abs(x3 - x2))):.3e}, value shift {(v3 - v2).tolist()}')
    assert np.all(np.isfinite(v3)) and np.all(np.abs(x3 - x2) <= 1e-6)
    assert np.all(np.abs(v3 - (v2 + np.log(2.0 / 3.0))) <= 1e-8 * (1.0 + np.abs(v2)))
    # every sample at -inf: NONFINITE_AT_START, the start stays where it is
    _, xi, vi, si, _ = dev.maximize(x0, np.full(3, 1e300), lo, hi, 4, noises=p.noises)
    assert np.all(si == dev.nv.nat.ACQ_OPT_NONFINITE_AT_START) and same_bits(xi, x0)
  finally:
    dev.close()


def test_the_flat_tail(gpu_ctx):
  """logei_cases.flat_tail_problem: hbo_acq_maximize with EI ends at its start, CONVERGED on its first evaluation; hbo_logei_maximize
  ends where tests/test_logei_cases_host.py says -- SciPy's end point on the oracle's LogEI -- within DEVICE_FACTOR times the distance
  between the oracle-driven run and that point on the CPU."""
  p = lc.flat_tail_problem()
  run, x_scipy, dist, _ = lc.flat_tail_reference()
  dev = Dev(gpu_ctx, p)
  try:
    nat = dev.nv.nat
    x0 = np.ascontiguousarray(p.x0[None, :])
    log, x, val, status, _ = dev.maximize(x0, [p.target], p.lo, p.hi, 48, noises=p.noises, ei=True)
    n_ei = int(np.sum(log['kind'][:, 0] != nat.ACQ_OPT_IDLE))
    assert status[0] == nat.ACQ_OPT_CONVERGED and same_bits(x, x0) and n_ei == 1 and 0.0 <= val[0] < 1e-20, (status, x, val)
    s_ei = int(status[0])
    log, x, val, status, _ = dev.maximize(x0, [p.target], p.lo, p.hi, 48, noises=p.noises)
    n_le = int(np.sum(log['kind'][:, 0] != nat.ACQ_OPT_IDLE))
    err = float(np.max(np.abs(x[0] - x_scipy)))
    print(f'\nlogei: flat tail: EI {n_ei} evaluation, status {s_ei}, at the start; LogEI {n_le} evaluations, status {int(status[0])}, '
          f'value {val[0]:.6f}, |x - SciPy| {err:.3e} (bound {lc.DEVICE_FACTOR * dist:.3e}; oracle run: {len(run.log)} evaluations, status {run.status})')
    assert status[0] in (nat.ACQ_OPT_CONVERGED, nat.ACQ_OPT_FTOL) and err <= lc.DEVICE_FACTOR * dist, (x, x_scipy, err, dist)
  finally:
    dev.close()


# ---- Python ---------------------------------------------------------------------------------------------------------------------
def _models(nv, hgp, n=30, d=2, seed=3, config=None):
  rng = np.random.default_rng(seed)
  f = lambda x: np.sin(3.0 * x[:, :1]) + np.cos(2.0 * x[:, 1:2])
  x = rng.uniform(size=(n, d))
  x2 = rng.uniform(size=(10, d))
  ds = {'t': nv.defs.SubDataset(x, f(x)), 'a': nv.defs.SubDataset(x2, f(x2)), 'b': nv.defs.SubDataset(x2[:4], f(x2[:4]))}
  samples = [{'lengthscale': np.full(d, 0.1 * i), 'signal_variance': np.array(0.5 - 0.2 * i), 'noise_variance': np.array(-5.0), 'constant': np.array(0.3)}
             for i in range(3)]
  wf = nv.utils.DEFAULT_WARP_FUNC
  if hgp:
    return nv.gp.HGP(ds, nv.mean.constant, nv.kernel.squared_exponential, nv.defs.GPParams(model=samples[0], samples=samples, config=dict(config or {})), wf), f
  return nv.gp.GP(ds, nv.mean.constant, nv.kernel.squared_exponential, nv.defs.GPParams(model=samples[0], config=dict(config or {})), wf), f


def test_python_pool_values_are_hbo_acq_logei(gpu_ctx):
  nv = _nv()
  model, _ = _models(nv, False)
  xq = np.random.default_rng(8).uniform(size=(37, 2))
  out = nv.acfun.log_ei(model=model, sub_dataset_key='t', x_queries=xq)
  assert out.shape == (37, 1) and np.all(np.isfinite(out))
  handle, xq_t, bm, add_noise, scale = nv.acfun._single_model(model, 't', xq)
  target = float(np.max(model.dataset['t'].y))
  direct = np.empty((37, 1), dtype=xq_t.dtype)
  handle.ctx.check(nv.nat.lib().hbo_acq_logei(handle.ctx.handle, bm.ref(), handle.handle, nv.nat.ptr(xq_t), 37, target, float(add_noise), float(scale),
                                              nv.nat.ptr(direct)))
  assert same_bits(out, direct)
  # it is the log of ei where ei is representable
  ei = nv.acfun.ei(model=model, sub_dataset_key='t', x_queries=xq)
  ok = ei[:, 0] > 1e-200
  assert ok.sum() > 5 and np.allclose(np.log(ei[ok, 0]), out[ok, 0], rtol=1e-9, atol=1e-9)
  v, g = nv.acfun.log_ei.value_and_grad(model=model, sub_dataset_key='t', x_queries=xq)
  assert v.shape == (37, 1) and g.shape == (37, 2) and np.all(np.isfinite(g))
  np.testing.assert_allclose(v, out, rtol=1e-6, atol=1e-8)
  # the prior branch: values from the device, the gradient and the maximiser refuse
  model.dataset['e'] = nv.defs.SubDataset(np.zeros((0, 2)), np.zeros((0, 1)))
  assert np.all(np.isfinite(nv.acfun.log_ei(model=model, sub_dataset_key='e', x_queries=xq)))
  for call in (lambda: nv.acfun.log_ei.value_and_grad(model=model, sub_dataset_key='e', x_queries=xq),
               lambda: nv.acfun.log_ei.maximize(model=model, sub_dataset_key='e', x_init=xq[:2])):
    with pytest.raises(nv.nat.HboError) as e:
      call()
    assert e.value.code == nv.nat.HBO_ERR_UNSUPPORTED


def test_python_hgp_combines_by_the_host_rule(gpu_ctx):
  nv = _nv()
  hgp, _ = _models(nv, True)
  xq = np.random.default_rng(9).uniform(size=(11, 2))
  out = nv.acfun.log_ei(model=hgp, sub_dataset_key='t', x_queries=xq)
  v, g = nv.acfun.log_ei.value_and_grad(model=hgp, sub_dataset_key='t', x_queries=xq)
  assert out.shape == v.shape == (11, 1) and g.shape == (11, 2)
  # per-sample rows from plain GPs under each sample's parameters, combined by logei_cases.combine
  target = float(np.max(hgp.dataset['t'].y))
  rows_v, rows_g = [], []
  for smp in hgp.get_model_params_samples():
    gp1 = nv.gp.GP(hgp.dataset, hgp.mean_func, hgp.cov_func, nv.defs.GPParams(model=smp, config={}), hgp.warp_func)
    rows_v.append(np.asarray(nv.acfun.log_ei(model=gp1, sub_dataset_key='t', x_queries=xq), dtype=np.float64)[:, 0])
    vv, gg = nv.acfun.log_ei.value_and_grad(model=gp1, sub_dataset_key='t', x_queries=xq)
    rows_g.append((np.asarray(vv, dtype=np.float64)[:, 0], gg))
  for q in range(11):
    # (to a few ulp: NumPy's vector exp / log against the scalar ones, and the GP's own factor against the HGP's per-sample one)
    cp = lc.combine([r[q] for r in rows_v])[0]
    assert abs(out[q, 0] - cp) <= 1e-12 * (1.0 + abs(cp))
    cv, cg = lc.combine([r[0][q] for r in rows_g], [r[1][q] for r in rows_g])
    assert abs(v[q, 0] - cv) <= 1e-12 * (1.0 + abs(cv)) and np.allclose(g[q], cg, rtol=1e-10, atol=1e-12 * np.max(np.abs(cg)))
  # it is the log of the mean of EI, not the mean of the logs
  ei = nv.acfun.ei(model=hgp, sub_dataset_key='t', x_queries=xq)
  ok = ei[:, 0] > 1e-200
  assert ok.sum() > 3 and np.allclose(np.log(ei[ok, 0]), out[ok, 0], rtol=1e-8, atol=1e-8)
  x, val, info = nv.acfun.log_ei.maximize(model=hgp, sub_dataset_key='t', x_init=xq[:3])
  assert np.all((x >= 0.0) & (x <= 1.0)) and np.isfinite(val) and val >= np.max(v[:3, 0]) - 1e-9 and info['x'].shape == (3, 2)


@pytest.mark.parametrize('hgp', [False, True], ids=['gp', 'hgp-S3'])
def test_python_bayesopt_on_device(gpu_ctx, hgp):
  """Three iterations of bayesopt.bayesopt with config['acq_opt_on_device'] on a 2-D problem: acfun.log_ei scores the candidates
  (hbo_acq_logei) and log_ei.maximize refines the best (hbo_logei_maximize); the suggestions are inside the box."""
  nv = _nv()
  model, f = _models(nv, hgp, config={'acq_opt_on_device': True, 'acq_opt_starts': 2})
  n0 = model.dataset['t'].x.shape[0]
  sub = nv.bayesopt.bayesopt(key=17, model=model, sub_dataset_key='t', query_oracle=f, ac_func=nv.acfun.log_ei, iters=3,
                             input_sampler=lambda rng, d: rng.uniform(size=(64, d)))
  assert sub.x.shape == (n0 + 3, 2) and sub.y.shape[0] == n0 + 3
  new = np.asarray(sub.x[n0:], dtype=np.float64)
  assert np.all((new >= 0.0) & (new <= 1.0)) and np.all(np.isfinite(sub.y))
