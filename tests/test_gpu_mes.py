"""Max-value entropy search on the device (run with `-m gpu` on an MI355X): hbo_acq_mes, hbo_mes_grad_samples, hbo_mes_maximize and
acfun.mes.  Cases, references, bounds and mutants: tests/mes_cases.py, judged on its own by tests/test_mes_cases_host.py.  Every
comparison is per query, never max-norm; gamma is placed as tests/test_gpu_acq_tails.py places it: y*_k = mu_q + gamma_k sd_q from the
device's own hbo_predict.  Each test prints its worst ratio to its bound (-s); profiles/mes_errors.md keeps them.

Bounds (mes_cases.py): per term DEVICE_FACTOR = 8 times the constant the float64 restatement needs against mpmath, in units of
eps64 * (gamma^2 / 2 + |log cdf| + |gamma r| / 2) -- for gamma >= 0 no more than the same in units of eps64 (1 + gamma^2) h --; an fp32
result adds the rounding of the output; comparisons across two routes to mu, var (or against the oracle's posterior) add
|h'| (d_mu / sd + |gamma| d_v / (2 v2)) with the tolerances test_gpu_parity.py holds the posterior to.  Gradients: 1e-7 (1 + gamma^2) of
the query's largest component in fp64, gamma^2 the mean over the query's K maxima; fp32: 2e-2 (1 + gamma^2), at queries whose every
|gamma| <= 3.25 only.

Two dispatch paths.  A call whose caches all have n <= 128 takes acq_small_kernel; the blocked kernels are reachable for it through
the test hook's force_blocked only, and they sum l = W k and beta = W^T l in another order -- as for EI / PI / UCB, where
tests/test_gpu_acq_blocked.py measures 3.2e-13 between the two.  The public call and the hook without force_blocked are held to
identical bits; the forced path to the siblings' bound (values rtol 1e-9, gradients 10 x 3.211e-13 of max(max |g|, 1e-3))."""
import ctypes as C
import types

import numpy as np
import pytest

import mes_cases as mc

pytestmark = pytest.mark.gpu
PD = C.POINTER(C.c_double)
SCALE = mc.SCALE
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
  """The S (model, factorised cache) pairs of a mes_cases.problem on the device and the calls the tests make on them.  Close it."""

  def __init__(self, ctx, p):
    nv = self.nv = _nv()
    self.ctx, self.p, self.d, self.dtype = ctx, p, p.case.d, p.dtype
    kn, mn, wf = getattr(nv.kernel, p.case.kname), getattr(nv.mean, p.case.mname), nv.utils.DEFAULT_WARP_FUNC
    self.handles, self.built = [], []
    for sm in p.smp:
      pn = nv.defs.GPParams(model=sm.model_t, config={})
      self.handles.append(nv.linalg.factor(mn, kn, pn, sm.x, sm.y, wf, ctx=ctx))
      self.built.append(nv.hmodel.BuiltModel(mn, kn, pn, wf, self.dtype, self.d))

  def close(self):
    for h in self.handles:
      h.close()

  def _args(self, sel, noises):
    nat = self.nv.nat
    s = len(sel)
    return ((nat.Model * s)(*[self.built[i].struct for i in sel]), (C.c_void_p * s)(*[self.handles[i].handle for i in sel]),
            (C.c_double * s)(*[float(noises[i]) for i in sel]))

  def predict(self, xq, s=0, cache=True):
    nat = self.nv.nat
    mu, var = np.empty((xq.shape[0], 1), dtype=self.dtype), np.empty((xq.shape[0], 1), dtype=self.dtype)
    self.ctx.check(nat.lib().hbo_predict(self.ctx.handle, self.built[s].ref(), self.handles[s].handle if cache else None, nat.ptr(xq), xq.shape[0], 0,
                                         nat.ptr(mu), nat.ptr(var)), allow_not_pd=False)
    return mu[:, 0], var[:, 0]

  def acq(self, xq, ystar, s=0, add_noise=0.0, scale=SCALE, cache=True):
    """hbo_acq_mes: [M] in the model dtype."""
    nat = self.nv.nat
    ys = np.ascontiguousarray(ystar, dtype=np.float64).reshape(-1)
    out = np.full((xq.shape[0], 1), 7.0, dtype=self.dtype)
    self.ctx.check(nat.lib().hbo_acq_mes(self.ctx.handle, self.built[s].ref(), self.handles[s].handle if cache else None, nat.ptr(xq), xq.shape[0], _dp(ys),
                                         ys.size, float(add_noise), float(scale), nat.ptr(out)), allow_not_pd=False)
    return out[:, 0]

  def grad(self, xq, ystar, sel=None, noises=None, scale=SCALE, force=None, chunk=0):
    """hbo_mes_grad_samples (force None) or its hook: (values [S, M] model dtype, gradients [S, M, D], fp64 values or None)."""
    nat = self.nv.nat
    sel = list(range(len(self.built))) if sel is None else list(sel)
    ys = np.ascontiguousarray(ystar, dtype=np.float64).reshape(len(sel), -1)
    structs, caches, nse = self._args(sel, [0.0] * len(self.built) if noises is None else noises)
    m = xq.shape[0]
    val, grad = np.full((len(sel), m), 7.0, dtype=self.dtype), np.full((len(sel), m, self.d), 7.0)
    if force is None:
      self.ctx.check(nat.lib().hbo_mes_grad_samples(self.ctx.handle, structs, len(sel), caches, nat.ptr(xq), m, _dp(ys), ys.shape[1], nse, float(scale),
                                                    nat.ptr(val), _dp(grad)), allow_not_pd=False)
      return val, grad, None
    v64 = np.full((len(sel), m), 7.0)
    self.ctx.check(nat.lib().hbo_probe_mes_grad_samples64(self.ctx.handle, structs, len(sel), caches, nat.ptr(xq), m, _dp(ys), ys.shape[1], nse, float(scale),
                                                          nat.ptr(val), _dp(grad), int(force), int(chunk), _dp(v64)), allow_not_pd=False)
    return val, grad, v64

  def maximize(self, x0, ystar, lo, hi, evals, state=None, opts=None):
    """One hbo_mes_maximize call: (log [evals, R], x_out, val_out, status, state)."""
    nat = self.nv.nat
    o = nat.AcqOptOpts(**(opts or self.nv.acfun.ACQ_OPT_DEFAULTS))
    s, r = len(self.built), x0.shape[0]
    ys = np.ascontiguousarray(ystar, dtype=np.float64).reshape(s, -1)
    structs, caches, nse = self._args(range(s), [0.0] * s)
    ns = nat.lib().hbo_acq_opt_state_doubles(self.d, o.memory)
    state = np.zeros((r, ns)) if state is None else state
    x, val, status = np.full((r, self.d), 7.0), np.full(r, 7.0), np.full(r, 7, dtype=np.int32)
    log = np.zeros((evals, r), dtype=nat.ACQ_OPT_EVAL_DTYPE)
    self.ctx.check(nat.lib().hbo_mes_maximize(self.ctx.handle, structs, s, caches, nat.ptr(x0), r, nat.ptr(lo), nat.ptr(hi), _dp(ys), ys.shape[1], nse, SCALE,
                                              C.byref(o), nat.ptr(state), evals, nat.ptr(x), nat.ptr(val), nat.ptr(status), nat.ptr(log)), allow_not_pd=False)
    return log, x, val, status, state


def _gamma_of(ystar, mu, sd):
  return ((np.longdouble(ystar) - mu.astype(np.longdouble)) / sd.astype(np.longdouble)).astype(np.float64)


def _device_sd(var, dtype, add_noise=0.0):
  t = np.dtype(dtype).type
  return np.sqrt((var + t(add_noise)) * t(SCALE))


# ---- the epilogue alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['fp64', 'fp32'])
@pytest.mark.parametrize('n_obs', [0, 300], ids=['prior', 'n300'])
def test_epilogue_against_mpmath_at_the_devices_own_posterior(gpu_ctx, n_obs, dtype):
  """hbo_acq_mes of every query against mpmath at the device's own mu, var (hbo_predict: the same routine, identical bits) and sd formed
  in the model dtype as the kernel forms it; one call with K = 1 per gamma of GAMMAS aimed at one query (every query of the call is
  checked at its own gamma) and one call with all of them as the K maxima.  n_obs = 0: the prior branch."""
  case = mc.Case('squared_exponential', 'constant', (max(n_obs, 1),), 3, 1, 9, dtype)
  p = mc.problem(case)
  dev = Dev(gpu_ctx, p)
  try:
    cache = n_obs > 0
    mu, var = dev.predict(p.xq, cache=cache)
    mu2, var2 = dev.predict(p.xq, cache=cache)
    assert same_bits(mu, mu2) and same_bits(var, var2) and np.all(var > 0)
    sd = _device_sd(var, p.dtype)
    gammas = mc.GAMMAS if dtype == 'fp64' else mc.GAMMAS_FP32
    lo, hi = -30.5, (38.5 if dtype == 'fp64' else 8.55)
    worst, reached = (0.0, None), set()

    def check(ystar, out, aimed):
      nonlocal worst
      gam = np.stack([_gamma_of(y, mu, sd) for y in ystar], axis=1)            # [M, K]
      for q in range(case.M):
        if not np.all((gam[q] >= lo) & (gam[q] <= hi)):
          continue
        exact = float(np.mean([mc.exact_terms(float(g))[0] for g in gam[q]]))
        bound = mc.value_bound(gam[q], float(sd[q]), float(var[q]), p.dtype)
        r = abs(float(out[q]) - exact) / bound if np.isfinite(out[q]) else np.inf
        if aimed is not None and q == aimed[0] and abs(gam[q][0] - aimed[1]) <= 0.25:
          reached.add(aimed[1])
        if r > worst[0]:
          worst = (r, (q, [round(float(g), 3) for g in gam[q][:4]], float(out[q]), exact))
        assert r <= 1.0 and out[q] >= 0.0, (q, gam[q], float(out[q]), exact, r)

    for k, g in enumerate(gammas):
      qk = (k * 5) % case.M
      ystar = [float(mu[qk]) + g * float(sd[qk])]
      out = dev.acq(p.xq, ystar, cache=cache)
      assert out.dtype == p.dtype
      check(ystar, out, (qk, g))
    ystar = [float(mu[0]) + g * float(sd[0]) for g in gammas]
    check(ystar, dev.acq(p.xq, ystar, cache=cache), None)
    print(f'\nmes: epilogue {dtype} n={n_obs}: worst ratio to the bound {worst[0]:.3e} at {worst[1]}')
    assert reached == set(gammas), sorted(set(gammas) - reached)
  finally:
    dev.close()


@pytest.mark.parametrize('dtype', ['fp64', 'fp32'])
@pytest.mark.parametrize('n_obs', [100, 300])
def test_gradient_entry_value_against_mpmath(gpu_ctx, n_obs, dtype):
  """The value of hbo_mes_grad_samples at each gamma of GAMMAS against mpmath at hbo_predict's mu, var.  The two reach mu, var by
  different routes (model-dtype sums over the product's column squares / fp64 sums over l = W k): the bound adds the posterior term,
  with d_mu, d_v as test_gpu_parity.py holds the posterior to them.  fp32: the gammas at which the output is a normal float."""
  case = mc.Case('matern52', 'constant', (n_obs,), 3, 1, 9, dtype)
  p = mc.problem(case)
  dev = Dev(gpu_ctx, p)
  try:
    mu, var = dev.predict(p.xq)
    sd = _device_sd(var, p.dtype)
    gammas = mc.GAMMAS if dtype == 'fp64' else mc.GAMMAS_FP32
    lo, hi = -30.5, (38.5 if dtype == 'fp64' else 8.55)
    d_mu, d_v = mc.posterior_tolerances(p.dtype, p.smp[0].mu, p.smp[0].var)
    worst, reached = (0.0, None), set()
    for k, g in enumerate(gammas):
      qk = (k * 5) % case.M
      ystar = [float(mu[qk]) + g * float(sd[qk])]
      val, grad, v64 = dev.grad(p.xq, ystar, force=0)
      pub = dev.grad(p.xq, ystar)
      assert same_bits(pub[0], val) and same_bits(pub[1], grad) and same_bits(v64.astype(p.dtype), val)
      gam = _gamma_of(ystar[0], mu, sd)
      for q in range(case.M):
        if not lo <= gam[q] <= hi:
          continue
        if q == qk and abs(gam[q] - g) <= 0.25:
          reached.add(g)
        exact = mc.exact_terms(float(gam[q]))[0]
        bound = mc.value_bound([gam[q]], float(sd[q]), float(var[q]), p.dtype, d_mu, d_v)
        r = abs(float(val[0, q]) - exact) / bound if np.isfinite(val[0, q]) else np.inf
        if r > worst[0]:
          worst = (r, (q, round(float(gam[q]), 3)))
        assert r <= 1.0 and val[0, q] >= 0.0 and np.all(np.isfinite(grad[0, q])), (q, gam[q], float(val[0, q]), exact, r)
    print(f'\nmes: gradient-entry value {dtype} n={n_obs}: worst ratio to the bound {worst[0]:.3e} at {worst[1]}')
    assert reached == set(gammas)
  finally:
    dev.close()


@pytest.mark.parametrize('dtype', ['fp64', 'fp32'])
def test_no_variance_no_information_and_nan_stays_nan(gpu_ctx, dtype):
  """v2 = (var + add_noise) * scale <= 0 -- forced through add_noise and scale, and through a posterior variance that is itself 0 with
  add_noise = 0 -- : value 0, gradient 0, in every entry point and on both dispatch paths; a NaN v2 stays NaN."""
  for n in (100, 300):
    p = mc.problem(mc.Case('squared_exponential', 'linear', (n,), 3, 7, 9, dtype))
    dev = Dev(gpu_ctx, p)
    try:
      for add_noise, scale in ((-1e3, SCALE), (0.0, 0.0), (-1e3, 1.0)):
        out = dev.acq(p.xq, p.ystar[0], add_noise=add_noise, scale=scale)
        val, grad, v64 = dev.grad(p.xq, p.ystar[0], noises=[add_noise], scale=scale, force=0)
        assert np.all(out == 0.0) and np.all(val == 0.0) and np.all(v64 == 0.0) and np.all(grad == 0.0), (n, add_noise, scale)
      out = dev.acq(p.xq, p.ystar[0], add_noise=np.nan)
      val, grad, _ = dev.grad(p.xq, p.ystar[0], noises=[np.nan])
      assert np.all(np.isnan(out)) and np.all(np.isnan(val)) and np.all(np.isnan(grad)), n
      assert np.all(np.isnan(dev.acq(p.xq, p.ystar[0], add_noise=np.nan, cache=False)))          # the prior branch
      assert np.all(dev.acq(p.xq, p.ystar[0], add_noise=-1e3, cache=False) == 0.0)
    finally:
      dev.close()
    # the variance itself, out of the products, with add_noise = 0: exactly 0 at query 0 (mes_cases.zero_variance_problem); without the
    # rule sd = 0 there gives gamma = inf or NaN.  The other queries of the same call keep their information
    z = mc.zero_variance_problem(n, dtype)
    dev = Dev(gpu_ctx, z)
    try:
      mu, var = dev.predict(z.xq)
      assert var[0] == 0.0 and np.isfinite(mu[0]) and np.all(var[1:] > 0.0)
      out = dev.acq(z.xq, z.ystar[0])
      for force in (0, 1):
        val, grad, v64 = dev.grad(z.xq, z.ystar[0], force=force)
        assert val[0, 0] == 0.0 and v64[0, 0] == 0.0 and np.all(grad[0, 0] == 0.0), (n, force, val[0, 0], grad[0, 0])
        assert np.all(val[0, 1:] >= 0.0) and np.any(val[0, 1:] > 0.0) and np.all(np.isfinite(grad[0, 1:])) and np.any(grad[0, 1:] != 0.0)
      assert out[0] == 0.0 and np.all(out[1:] >= 0.0) and np.any(out[1:] > 0.0) and int(np.argmax(out)) != 0
      assert dev.acq(z.xq, z.ystar[0], cache=False)[0] == 0.0                                    # prior: k(0, 0) = 0
    finally:
      dev.close()


# ---- shapes: value and gradient against the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize('case', mc.CASES, ids=lambda c: c.id)
def test_value_and_gradient_against_the_oracle(gpu_ctx, case):
  """hbo_mes_grad_samples per query and per component against the oracle (its posterior and the posterior's derivative), every sample
  of the call against its own reference; hbo_acq_mes of every sample against the same values."""
  p = mc.problem(case)
  dev = Dev(gpu_ctx, p)
  try:
    val, grad, _ = dev.grad(p.xq, p.ystar)
    assert val.dtype == p.dtype and grad.dtype == np.float64 and val.shape == (case.S, case.M) and grad.shape == (case.S, case.M, case.d)
    wv = wg = wa = 0.0
    checked = 0
    for s, sm in enumerate(p.smp):
      rv, rg, gam = mc.oracle_value_and_grad(sm, p.xq, p.ystar[s])
      d_mu, d_v = mc.posterior_tolerances(p.dtype, sm.mu, sm.var)
      pool = dev.acq(p.xq, p.ystar[s], s=s)
      for q in range(case.M):
        bound = mc.value_bound(gam[q], float(sm.sd[q]), float(sm.var[q]), p.dtype, d_mu, d_v)
        r = abs(float(val[s, q]) - rv[q]) / bound
        ra = abs(float(pool[q]) - rv[q]) / bound
        wv, wa = max(wv, r), max(wa, ra)
        assert r <= 1.0 and ra <= 1.0, (s, q, gam[q], float(val[s, q]), float(pool[q]), rv[q], r, ra)
        if case.dtype == 'fp32' and np.max(np.abs(gam[q])) > 3.25:
          continue
        checked += 1
        rgq = float(np.max(np.abs(grad[s, q] - rg[q])) / (mc.grad_tol(gam[q], p.dtype) * np.max(np.abs(rg[q]))))
        wg = max(wg, rgq)
        assert rgq <= 1.0, (s, q, gam[q], grad[s, q], rg[q], rgq)
    print(f'\nmes: {case.id}: worst ratio to the oracle bounds: value {wv:.3e}, pool value {wa:.3e}, gradient {wg:.3e} ({checked} queries)')
    assert checked >= case.S                                    # query 0 of every sample sits inside the window by construction
  finally:
    dev.close()


def test_the_devices_own_value_against_central_differences(gpu_ctx):
  """d value / dx of three queries against central differences of the device's own fp64 value, step 1e-5: truncation ~ step^2 |f'''| / 6
  and rounding ~ eps64 |f| / step are both ~1e-10 of a value of order one; the bound is 1e-6 of the query's largest component."""
  case = mc.Case('matern52', 'linear', (129,), 3, 7, 3, 'fp64')
  p = mc.problem(case)
  dev = Dev(gpu_ctx, p)
  try:
    _, grad, _ = dev.grad(p.xq, p.ystar, force=0)
    step = 1e-5
    pts = np.repeat(p.xq, 2 * case.d, axis=0)
    for q in range(3):
      for d in range(case.d):
        pts[(q * case.d + d) * 2, d] += step
        pts[(q * case.d + d) * 2 + 1, d] -= step
    _, _, v64 = dev.grad(np.ascontiguousarray(pts), p.ystar, force=0)
    fd = ((v64[0, 0::2] - v64[0, 1::2]) / (pts[0::2] - pts[1::2])[np.arange(3 * case.d), np.tile(np.arange(case.d), 3)]).reshape(3, case.d)
    worst = max(float(np.max(np.abs(fd[q] - grad[0, q])) / (1e-6 * np.max(np.abs(grad[0, q])))) for q in range(3))
    print(f'\nmes: central differences: worst ratio to the bound {worst:.3e}')
    assert worst <= 1.0, (fd, grad[0])
  finally:
    dev.close()


def test_pool_values_do_not_depend_on_the_chunking(gpu_ctx):
  """hbo_acq_mes with post_chunk below M against the unchunked call, to the bit (fp64 and fp32, 300 observations, 300 queries)."""
  for dtype in ('fp64', 'fp32'):
    p = mc.problem(mc.Case('matern32', 'linear', (300,), 3, 7, 37, dtype))
    xq = np.ascontiguousarray(np.random.default_rng(5).uniform(size=(300, 3)).astype(p.dtype))
    dev = Dev(gpu_ctx, p)
    try:
      whole = dev.acq(xq, p.ystar[0])
      alone = dev.acq(np.ascontiguousarray(xq[200:201]), p.ystar[0])
      old = gpu_ctx.get_option('post_chunk')
      try:
        gpu_ctx.set_option('post_chunk', 128)
        cut = dev.acq(xq, p.ystar[0])
      finally:
        gpu_ctx.set_option('post_chunk', old)
      assert np.all(np.isfinite(whole)) and same_bits(whole, cut) and same_bits(dev.acq(xq, p.ystar[0]), whole)
      # a row does not depend on what the other rows hold (include/hbo.h): every other row replaced by another query
      other = np.ascontiguousarray(np.random.default_rng(6).uniform(size=(300, 3)).astype(p.dtype))
      other[200] = xq[200]
      assert dev.acq(other, p.ystar[0])[200].tobytes() == whole[200].tobytes()
      # ... and here not on M either: post_plan gives M = 1 and M = 300 the same product form over three row blocks (split along K,
      # one block per chunk, in both dtypes), which is as far as the header's statement about M goes
      assert alone[0].tobytes() == whole[200].tobytes()
    finally:
      dev.close()


# ---- determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['fp64', 'fp32'])
def test_a_row_does_not_depend_on_what_shares_the_call(gpu_ctx, dtype):
  p = mc.problem(mc.Case('matern32', 'constant', (100, 300, 100), 3, 65, 9, dtype))
  dev = Dev(gpu_ctx, p)
  try:
    val, grad, v64 = dev.grad(p.xq, p.ystar, force=0)
    assert np.isfinite(val).all() and np.isfinite(grad).all() and same_bits(v64.astype(p.dtype), val)
    again = dev.grad(p.xq, p.ystar, force=0)
    assert all(same_bits(a, b) for a, b in zip(again, (val, grad, v64)))                   # identical calls, identical bits
    pub = dev.grad(p.xq, p.ystar)
    assert same_bits(pub[0], val) and same_bits(pub[1], grad)
    # a sample alone, a query alone, another chunking: the blocked kernels throughout (sample 1 has n = 300)
    one = dev.grad(np.ascontiguousarray(p.xq[4:5]), p.ystar[1:2], sel=[1], force=0)
    assert same_bits(one[0][0], val[1, 4:5]) and same_bits(one[1][0], grad[1, 4:5]) and same_bits(one[2][0], v64[1, 4:5])
    cut = dev.grad(p.xq, p.ystar, force=0, chunk=2)
    assert all(same_bits(a, b) for a, b in zip(cut, (val, grad, v64)))
    # samples 0 and 2 alone (n = 100): the one-launch path; forced through the blocked kernels they keep the bits they had beside n = 300
    small = dev.grad(p.xq, p.ystar[[0, 2]], sel=[0, 2], force=0)
    forced = dev.grad(p.xq, p.ystar[[0, 2]], sel=[0, 2], force=1)
    assert same_bits(forced[0], val[[0, 2]]) and same_bits(forced[1], grad[[0, 2]]) and same_bits(forced[2], v64[[0, 2]])
    pub = dev.grad(p.xq, p.ystar[[0, 2]], sel=[0, 2])
    assert same_bits(pub[0], small[0]) and same_bits(pub[1], small[1])                     # the public call is the one-launch path
    alone = dev.grad(np.ascontiguousarray(p.xq[2:3]), p.ystar[2:3], sel=[2], force=0)
    assert same_bits(alone[0][0], small[0][1, 2:3]) and same_bits(alone[1][0], small[1][1, 2:3])
    # the two paths against each other: the siblings' bound (module docstring)
    ev = float(np.max(np.abs(small[2] - forced[2]) / np.maximum(np.abs(forced[2]), 1e-300)))
    eg = max(float(np.max(np.abs(small[1][i] - forced[1][i])) / max(np.max(np.abs(forced[1][i])), 1e-3)) for i in range(2))
    print(f'\nmes: one launch against the blocked kernels at n = 100, {dtype}: value {ev:.3e} relative, gradient {eg:.3e}')
    if dtype == 'fp64':
      assert ev <= 1e-9 and eg <= FORCED_GRAD_TOL, (ev, eg)
  finally:
    dev.close()


# ---- the maximiser --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [1, 3])
@pytest.mark.parametrize('n', [60, 300])
def test_maximiser(gpu_ctx, n, S):
  """R = 4 starts.  val_out is the mean over s of the gradient entry's fp64 values at x_out; 48 evaluations in one call equal 7 + 41 in
  two (state, log, outputs, to the bit); every iterate stays inside the box and the bounds are hit exactly; the value at the end is at
  least the value at the start."""
  p = mc.problem(mc.Case('matern52', 'constant', (n,) * S, 3, 7, 4, 'fp64'))
  dev = Dev(gpu_ctx, p)
  try:
    lo, hi = np.full(3, 0.25), np.full(3, 0.75)
    x0 = np.ascontiguousarray(lo + (hi - lo) * np.random.default_rng(n + S).uniform(size=(4, 3)))
    x0[0] = [0.25, 0.75, 0.5]                                   # a start on the boundary
    log, x, val, status, state = dev.maximize(x0, p.ystar, lo, hi, 48)
    la, xa, va, sa, sta = dev.maximize(x0, p.ystar, lo, hi, 7)
    lb, xb, vb, sb, stb = dev.maximize(x0, p.ystar, lo, hi, 41, state=sta.copy())
    assert same_bits(np.concatenate([la, lb]), log) and same_bits(xb, x) and same_bits(vb, val) and same_bits(sb, status) and same_bits(stb, state)
    assert np.all(np.isfinite(val)) and np.all((x >= lo) & (x <= hi))
    nat = dev.nv.nat
    assert np.all(log['kind'][0] == nat.ACQ_OPT_START) and np.any(log['kind'] == nat.ACQ_OPT_MAIN)
    _, _, v_end = dev.grad(np.ascontiguousarray(x), p.ystar, force=0)
    _, _, v_start = dev.grad(x0, p.ystar, force=0)
    mean = lambda v: np.array([sum([0.0] + [v[s, r] for s in range(S)]) / S for r in range(4)])    # in sample order, as the control kernel sums
    assert same_bits(mean(v_end), val), (mean(v_end), val)
    assert np.all(val >= mean(v_start)), (val, mean(v_start))
    assert same_bits(-log['value'][0], mean(v_start))
    # a box so small that the value is monotone across it: every start ends in a corner, on the bounds to the bit
    lo2, hi2 = np.full(3, 0.5), np.full(3, 0.5 + 2.0**-10)
    x2 = np.ascontiguousarray(np.tile(0.5 * (lo2 + hi2), (4, 1)))
    _, xc, vc, _, _ = dev.maximize(x2, p.ystar, lo2, hi2, 48)
    assert np.all((xc >= lo2) & (xc <= hi2)) and np.all(np.isfinite(vc))
    assert np.any((xc == lo2) | (xc == hi2)), xc
    print(f'\nmes: maximiser n={n} S={S}: status {status.tolist()}, value {mean(v_start).tolist()} -> {val.tolist()}')
  finally:
    dev.close()


# ---- Python ---------------------------------------------------------------------------------------------------------------------
def _gp(nv, n=30, d=2, seed=3):
  rng = np.random.default_rng(seed)
  f = lambda x: np.sin(3.0 * x[:, :1]) + np.cos(2.0 * x[:, 1:2])
  x = rng.uniform(size=(n, d))
  x2 = rng.uniform(size=(10, d))
  ds = {'t': nv.defs.SubDataset(x, f(x)), 'a': nv.defs.SubDataset(x2, f(x2)), 'b': nv.defs.SubDataset(x2[:4], f(x2[:4]))}
  model_t = {'lengthscale': np.full(d, 0.0), 'signal_variance': np.array(0.5), 'noise_variance': np.array(-5.0), 'constant': np.array(0.3)}
  params = nv.defs.GPParams(model=model_t, config={})
  return nv.gp.GP(ds, nv.mean.constant, nv.kernel.squared_exponential, params, nv.utils.DEFAULT_WARP_FUNC), f


def test_python_pool_values_are_hbo_acq_mes(gpu_ctx):
  nv = _nv()
  model, _ = _gp(nv)
  xq = np.random.default_rng(8).uniform(size=(37, 2))
  ys = nv.acfun.max_value_samples(model, 't', xq, num_maxima=7, key=11, num_features=256)
  assert ys.shape == (7,) and ys.dtype == np.float64 and np.all(ys >= np.max(model.dataset['t'].y))
  out = nv.acfun.mes(model, 't', xq, maxima=ys)
  assert out.shape == (37, 1) and np.all(out >= 0.0) and np.all(np.isfinite(out))
  handle, xq_t, bm, _, _ = nv.acfun._single_model(model, 't', xq)
  _, scale = model.predict_noise_and_scale(False, True)
  assert scale == 1.5
  direct = np.empty((37, 1), dtype=xq_t.dtype)
  handle.ctx.check(nv.nat.lib().hbo_acq_mes(handle.ctx.handle, bm.ref(), handle.handle, nv.nat.ptr(xq_t), 37, _dp(ys), 7, 0.0, scale, nv.nat.ptr(direct)))
  assert same_bits(out, direct)
  # drawn maxima: the same key gives the same values; value_and_grad's values are those of the pool up to the posterior's two routes
  a, b = nv.acfun.mes(model, 't', xq, key=4), nv.acfun.mes(model, 't', xq, key=4)
  assert same_bits(a, b)
  v, g = nv.acfun.mes.value_and_grad(model=model, sub_dataset_key='t', x_queries=xq, maxima=ys)
  assert v.shape == (37, 1) and g.shape == (37, 2) and np.all(np.isfinite(g))
  np.testing.assert_allclose(v, out, rtol=1e-6, atol=1e-9)


def test_python_suggest_inside_bayesopt(gpu_ctx):
  """mes.suggest as the strategy of bayesopt.bayesopt: three iterations on a 2-D squared-exponential model return points in the box, the
  dataset grows by three, and a fixed key gives the same bits twice."""
  nv = _nv()
  runs = []
  for _ in range(2):
    model, f = _gp(nv)
    n0 = model.dataset['t'].x.shape[0]
    ac = nv.acfun.MaxValueEntropySearch(num_maxima=8, num_features=256, starts=3)
    sub = nv.bayesopt.bayesopt(key=17, model=model, sub_dataset_key='t', query_oracle=f, ac_func=ac, iters=3,
                               input_sampler=lambda rng, d: rng.uniform(size=(64, d)))
    assert sub.x.shape == (n0 + 3, 2) and sub.y.shape[0] == n0 + 3
    new = np.asarray(sub.x[n0:], dtype=np.float64)
    assert np.all((new >= 0.0) & (new <= 1.0)) and np.all(np.isfinite(sub.y))
    runs.append(new)
  assert same_bits(runs[0], runs[1])
  # without observations the best candidate comes back unrefined
  model, _ = _gp(nv)
  model.dataset['e'] = nv.defs.SubDataset(np.zeros((0, 2)), np.zeros((0, 1)))
  xc = np.random.default_rng(2).uniform(size=(16, 2))
  x = nv.acfun.mes.suggest(model=model, sub_dataset_key='e', x_candidates=xc, key=3)
  assert x.shape == (1, 2) and any(np.array_equal(x[0], row) for row in xc)
