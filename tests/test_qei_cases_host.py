"""tests/qei_cases.py judged on its own, and the host side of batch expected improvement: no device.  The reference against the oracle's
own posterior, against torch.autograd and against central differences; the constants of the bounds MEASURED (the float64 restatement in
the kernel's order against the long-double reference over the case table); the q = 1 closed form; the mutants; the edges the case table
must hold; the admission condition of every case; the argument checks of the two new entry points."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as spla
from scipy import special

import qei_cases as qc
from hyperbo_amd import _native as nat
from hyperbo_amd.bo_utils import acfun
from oracle import hyperbo_oracle as o

LD = qc.LD
SMALL = [qc.Case('matern32', 'zero', (2,), 3, 2, 33, 1, 'fp64', True),
         qc.Case('dot_product', 'linear', (5,), 3, 3, 33, 1, 'fp64', True),
         qc.Case('squared_exponential', 'constant', (5,), 2, 3, 33, 1, 'fp64', False),
         qc.Case('matern52', 'linear', (7,), 3, 2, 33, 1, 'fp64', True)]


def _pairs(case):
  p = qc.problem(case)
  for s, sm in enumerate(p.smp):
    for m in range(case.M):
      yield p, s, sm, m


def test_reference_in_float64_is_the_oracles_posterior():
  """mu, Sigma' and the factor of K of the float64 reference against the oracle's own solve_gp_linear_system and predict(full_cov) on the
  raw parameters under the default warp, noise on the diagonal first and the scale after it (gp.py:607-619)."""
  for case in SMALL + [qc.CASES[2]]:
    for p, s, sm, m in _pairs(case):
      x, y, xb = sm.x.astype(np.float64), sm.y.astype(np.float64), p.xb[m].astype(np.float64)
      chol, kinvy, _ = o.solve_gp_linear_system(sm.mo, sm.ko, sm.po, x, y, qc.WFO)
      mu, cov = o.predict(sm.mo, sm.ko, sm.po, x, y, xb, qc.WFO, full_cov=True)
      want = (cov + np.eye(case.q) * sm.add_noise) * qc.SCALE
      r = qc.reference(sm, xb, p.z, sm.target, sm.add_noise, qc.SCALE)
      _, l, alpha, *_ = qc._posterior(sm, xb, np.float64)
      np.testing.assert_allclose(l, chol, rtol=1e-10, atol=1e-13)
      np.testing.assert_allclose(alpha, kinvy[:, 0], rtol=1e-8, atol=1e-11)
      np.testing.assert_allclose(r.mu, mu[:, 0], rtol=1e-9, atol=1e-11)
      np.testing.assert_allclose(r.sigma, want, rtol=1e-8, atol=1e-11)
      np.testing.assert_allclose(r.c, spla.cholesky(want, lower=True), rtol=1e-8, atol=1e-11)


def test_restatement_against_longdouble():
  """The worst error of the float64 restatement in the kernel's order against the long-double reference over CASES, in units of
  eps64 x term scale x cond(C)^2 for the value and every gradient row and eps64 x term scale for every entry of Sigma': C_VALUE, C_SIGMA
  and C_GRAD are these numbers rounded up by less than a factor of two.  The selection (j*_b, imp_b > 0) agrees for every base sample."""
  worst, where = [0.0, 0.0, 0.0], [None] * 3
  for case in qc.CASES:
    refs = qc.references(case)
    for p, s, sm, m in _pairs(case):
      ref = refs[s][m]
      rs = qc.restated(sm, p.xb[m], p.z, sm.target, sm.add_noise, qc.SCALE)
      assert np.array_equal(rs.js, ref.js) and np.array_equal(rs.pos, ref.pos), (case.id, s, m)
      unit = qc.EPS64 * ref.cond**2
      got = (float(qc.ratio(float(LD(rs.value) - ref.value), unit * float(ref.value_scale))),
             float(np.max(qc.ratio((np.tril(rs.sigma).astype(LD) - np.tril(ref.sigma)).astype(np.float64),
                                   qc.EPS64 * np.tril(np.asarray(ref.sigma_scale, dtype=np.float64))))),
             float(np.max(qc.ratio((rs.grad.astype(LD) - ref.grad).astype(np.float64), unit * np.asarray(ref.grad_scale, dtype=np.float64)))))
      for k in range(3):
        if got[k] > worst[k]:
          worst[k], where[k] = got[k], (case.id, s, m)
  print(f'\nqei: measured constants (value, Sigma, gradient): {worst[0]:.3f} at {where[0]}, {worst[1]:.3f} at {where[1]}, {worst[2]:.3f} at {where[2]}')
  for w, c in zip(worst, (qc.C_VALUE, qc.C_SIGMA, qc.C_GRAD)):
    assert w <= c <= 2.0 * w, (worst, where)


def _torch_value(sm, xb, z, target, add_noise, scale):
  """The value through torch in float64 (torch.linalg.cholesky for both factors) with xb a leaf: autograd gives the gradient."""
  import torch
  t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
  pr = qc._params(sm, np.float64)
  x, y = t(sm.x), t(sm.y).reshape(-1)
  xb = t(xb).requires_grad_(True)

  def kern(a, b):
    if pr.dot:
      return a @ b.T / float(pr.sigma)**2 + float(pr.bias)**2
    u = (((a[:, None, :] - b[None, :, :]) / t(pr.ls))**2).sum(-1)
    sv = float(pr.sv)
    if sm.kname == 'squared_exponential':
      return sv * torch.exp(-u / 2)
    # (sqrt at u == 0 has no derivative in autograd: its pairs are masked, where the rule says their contribution is 0)
    safe = torch.where(u > 0, u, torch.ones_like(u))
    r = torch.sqrt((3.0 if sm.kname == 'matern32' else 5.0) * safe)
    k = sv * (1 + r) * torch.exp(-r) if sm.kname == 'matern32' else sv * (1 + r + r * r / 3) * torch.exp(-r)
    return torch.where(u > 0, k, torch.full_like(u, sv))

  def mean(a):
    if sm.mname == 'zero':
      return torch.zeros(a.shape[0], dtype=torch.float64)
    if sm.mname == 'constant':
      return torch.full((a.shape[0],), float(np.squeeze(sm.pw.model['constant'])), dtype=torch.float64)
    lm = sm.pw.model['linear_mean']
    return a @ t(lm['kernel']).reshape(-1) + float(np.squeeze(lm['bias']))

  kxx = kern(x, x) + torch.eye(x.shape[0], dtype=torch.float64) * (float(pr.noise) + 1e-6)
  l = torch.linalg.cholesky(kxx)
  alpha = torch.cholesky_solve((y - mean(x))[:, None], l)[:, 0]
  kq = kern(x, xb)
  v = torch.linalg.solve_triangular(l, kq, upper=False)
  mu = kq.T @ alpha + mean(xb)
  sig = (kern(xb, xb) - v.T @ v + torch.eye(xb.shape[0], dtype=torch.float64) * add_noise) * scale
  c = torch.linalg.cholesky(sig)
  f = mu[None, :] + t(z) @ c.T
  val = torch.clamp(f.max(dim=1).values - target, min=0.0).mean()
  val.backward()
  return float(val.detach()), xb.grad.numpy()


def test_reference_gradient_against_autograd_and_central_differences():
  """On admitted cases: the float64 reference's gradient against torch.autograd's, both within the fp64 bound of the long-double
  reference (two float64 evaluations), and the long-double reference's gradient against central differences of its own value with
  h = 1e-7 -- truncation h^2 f''' ~ 1e-14 and rounding eps_ld / h ~ 1e-12 of the value's scale; every kink is 1000 bounds away."""
  for case in SMALL + [qc.CASES[1], qc.CASES[2]]:
    for p, s, sm, m in _pairs(case):
      args = (sm, p.xb[m], p.z, sm.target, sm.add_noise, qc.SCALE)
      ref = qc.reference(*args, LD)
      assert qc.admitted(*args, p.dtype, ref)[0], (case.id, s, m)
      val, g = _torch_value(*args)
      r64 = qc.reference(*args)
      bound = qc.grad_bound(ref, np.float64)
      assert abs(val - float(ref.value)) <= qc.value_bound(ref, np.float64)
      assert np.all(qc.ratio(g - ref.grad.astype(np.float64), bound) <= 1.0), (case.id, s, m)
      assert np.all(qc.ratio(r64.grad - ref.grad.astype(np.float64), bound) <= 1.0), (case.id, s, m)
      if case.ns[s] > 7:
        continue
      h = LD(1e-7)
      for j in range(case.q):
        for d in range(case.d):
          xp, xm = p.xb[m].astype(LD), p.xb[m].astype(LD)
          xp[j, d] += h; xm[j, d] -= h
          fd = (qc.reference(sm, xp, p.z, sm.target, sm.add_noise, qc.SCALE, LD).value -
                qc.reference(sm, xm, p.z, sm.target, sm.add_noise, qc.SCALE, LD).value) / (2 * h)
          assert abs(float(fd - ref.grad[j, d])) <= 1e-9 * float(np.max(ref.grad_scale)) + 1e-11 * float(ref.value_scale), (case.id, j, d)


def test_q1_is_the_closed_form_and_approaches_expected_improvement():
  """q = 1: the value is mean_b max(0, mu + sd z_b - t) with sd = sqrt((var + add_noise) scale), and with z the B = 1024 normal
  mid-quantiles it is within 1 / B of expected_improvement_sub (the midpoint rule on the quantile function, times sd <= 1 here)."""
  case = qc.Case('squared_exponential', 'constant', (7,), 3, 1, 1024, 3, 'fp64', True)
  p = qc.problem(case)
  sm = p.smp[0]
  z = special.ndtri((np.arange(1024) + 0.5) / 1024.0)[:, None]
  for m in range(case.M):
    x, y, xb = sm.x.astype(np.float64), sm.y.astype(np.float64), p.xb[m].astype(np.float64)
    mu, var = o.predict(sm.mo, sm.ko, sm.po, x, y, xb, qc.WFO)
    sd = float(np.sqrt((var[0, 0] + sm.add_noise) * qc.SCALE))
    for t in (float(mu[0, 0]) - 0.5 * sd, float(mu[0, 0]) + 0.7 * sd):
      r = qc.reference(sm, xb, z, t, sm.add_noise, qc.SCALE)
      closed = float(np.mean(np.maximum(0.0, mu[0, 0] + sd * z[:, 0] - t)))
      assert abs(float(r.value) - closed) <= 1e-13
      assert sd <= 1.0 and abs(float(r.value) - float(o.expected_improvement_sub(mu[0, 0], sd, t))) <= 1.0 / 1024


def test_every_mutant_is_rejected_by_a_case():
  """Each mutant of the reference leaves the fp64 bounds of the device on at least one pair of the table (the tie case for the
  lowest-index rule): a device that made that mistake would fail the GPU tier."""
  pairs = [(p, sm, p.xb[m], p.z, sm.target) for case in SMALL + qc.CASES[:4] for p, s, sm, m in _pairs(case) if case.dtype == 'fp64']
  tie = qc.tie_problem()
  pairs.append((tie, tie.smp[0], tie.xb[0], tie.z, float(tie.targets[0])))
  caught = {}
  for mutant in qc.MUTANTS:
    for p, sm, xb, z, target in pairs:
      ref = qc.reference(sm, xb, z, target, sm.add_noise, qc.SCALE, LD)
      mut = qc.reference(sm, xb, z, target, sm.add_noise, qc.SCALE, np.float64, mutant)
      if mut.grad is None or max(qc.device_ratios(mut.value, mut.grad, ref, np.float64)) > 1.0:
        caught[mutant] = p.case.id
        break
  assert set(caught) == set(qc.MUTANTS), sorted(set(qc.MUTANTS) - set(caught))


def test_the_tie_case_ties_exactly():
  tie = qc.tie_problem()
  sm = tie.smp[0]
  for ft in (np.float64, LD):
    r = qc.reference(sm, tie.xb[0], tie.z, float(tie.targets[0]), sm.add_noise, qc.SCALE, ft)
    assert r.f[0, 0] == r.f[0, 1] and r.js[0] == 0 and r.pos[0] and r.mubar[0] > 0
  hi = qc.reference(sm, tie.xb[0], tie.z, float(tie.targets[0]), sm.add_noise, qc.SCALE, np.float64, 'highest_index')
  assert hi.js[0] == 1


def test_the_table_holds_every_edge():
  cs = qc.CASES
  assert {n for c in cs for n in c.ns} >= {1, 2, 63, 64, 65, 127, 128}
  assert {c.q for c in cs} >= {1, 2, 3, 16} and {c.d for c in cs} >= {1, 3, 17, 128, 256} and max(c.q * c.d for c in cs) == 256
  assert {c.B for c in cs} >= {1, 255, 256, 257, 1024}
  assert {c.kname for c in cs} == {'squared_exponential', 'matern32', 'matern52', 'dot_product'}
  assert {c.mname for c in cs} == {'zero', 'constant', 'linear'} and {c.dtype for c in cs} == {'fp64', 'fp32'}
  assert {c.S for c in cs} >= {1, 3} and any(len(set(c.ns)) > 1 for c in cs) and {c.noisy for c in cs} == {True, False}
  assert qc.SCALE != 1.0 and all(c.B <= 32 for c in cs if c.dtype == 'fp32')
  assert all(c.q <= nat.QEI_MAX_Q and c.B <= nat.QEI_MAX_BASE for c in cs)


def test_every_case_is_admitted():
  """The smooth-region condition holds for every (sample, batch) pair of the table, every base sample counted, and part of the base
  samples improve in every case with more than one."""
  for case in qc.CASES:
    refs = qc.references(case)
    for p, s, sm, m in _pairs(case):
      ok, margin, need = qc.admitted(sm, p.xb[m], p.z, sm.target, sm.add_noise, qc.SCALE, p.dtype, refs[s][m])
      assert ok, (case.id, s, m, margin, need)
    if case.B > 1:
      assert any(0 < int(refs[s][0].pos.sum()) < case.B for s in range(case.S)), case.id


def test_argument_errors_come_before_any_device_call():
  err = lambda: (nat.lib().hbo_last_error(None) or b'').decode()
  pd = C.POINTER(C.c_double)
  tp = lambda a: None if a is None else a.ctypes.data_as(pd)
  lib = nat.lib()
  xq, val, grad = np.zeros((1, 2, 2)), np.full((1, 1), 7.0), np.full((1, 1, 2, 2), 7.0)
  models, caches, nse = (nat.Model * 1)(), (C.c_void_p * 1)(), np.zeros(1)
  z, tg = np.zeros((4, 2)), np.array([0.5])
  gs = lambda S=1, q=2, B=4, zz=z, t=tg, ns=nse, sc=1.0, m=models, M=1: lib.hbo_qei_grad_samples(
      None, m, S, caches, nat.ptr(xq), M, q, tp(zz), B, tp(t), tp(ns), sc, tp(val), tp(grad))
  assert gs(zz=None) == nat.HBO_ERR_ARG and 'hbo_qei_grad_samples: null argument' in err()
  assert gs(m=None) == nat.HBO_ERR_ARG and 'null argument' in err()
  assert gs(M=-1) == nat.HBO_ERR_ARG and 'M' in err()
  assert gs(S=0) == nat.HBO_ERR_ARG and gs(S=4097) == nat.HBO_ERR_ARG and '1 <= S <= 4096' in err()
  assert gs(q=0) == nat.HBO_ERR_ARG and gs(q=17) == nat.HBO_ERR_ARG and '1 <= q <= 16' in err()
  assert gs(B=0) == nat.HBO_ERR_ARG and gs(B=1025) == nat.HBO_ERR_ARG and '1 <= B <= 1024' in err()
  bad = z.copy(); bad[3, 1] = np.nan
  assert gs(zz=bad) == nat.HBO_ERR_ARG and 'z holds a value that is not finite' in err()
  assert gs(t=np.array([np.inf])) == nat.HBO_ERR_ARG and 'targets' in err()
  assert gs(ns=np.array([-1e-9])) == nat.HBO_ERR_ARG and gs(ns=np.array([np.nan])) == nat.HBO_ERR_ARG and 'add_noise' in err()
  for sc in (0.0, -1.0, np.inf, np.nan):
    assert gs(sc=sc) == nat.HBO_ERR_ARG and 'scale' in err()
  assert gs() == nat.HBO_ERR_ARG and 'hbo_qei_grad_samples: ctx is null' in err()
  opts = nat.AcqOptOpts(**acfun.ACQ_OPT_DEFAULTS)
  ns_ = lib.hbo_acq_opt_state_doubles(4, opts.memory)
  state, x, v, status = np.zeros((1, ns_)), np.full((1, 2, 2), 7.0), np.full(1, 7.0), np.full(1, 7, dtype=np.int32)
  mx = lambda S=1, q=2, R=1, evals=1, zz=z, o_=opts: lib.hbo_qei_maximize(
      None, models, S, caches, nat.ptr(xq), R, q, None, None, tp(zz), 4, tp(tg), tp(nse), 1.0, C.byref(o_) if o_ is not None else None,
      nat.ptr(state), evals, nat.ptr(x), nat.ptr(v), nat.ptr(status), None)
  assert mx(zz=None) == nat.HBO_ERR_ARG and 'hbo_qei_maximize: null argument' in err()
  assert mx(R=0) == nat.HBO_ERR_ARG and mx(R=4097) == nat.HBO_ERR_ARG and '1 <= R <= 4096' in err()
  assert mx(evals=0) == nat.HBO_ERR_ARG and mx(evals=4097) == nat.HBO_ERR_ARG and '1 <= evals <= 4096' in err()
  assert mx(o_=None) == nat.HBO_ERR_ARG and 'opts is null' in err()
  assert mx(q=17) == nat.HBO_ERR_ARG and '1 <= q <= 16' in err()
  assert mx(S=0) == nat.HBO_ERR_ARG and '1 <= S <= 4096' in err()
  assert mx() == nat.HBO_ERR_ARG and 'hbo_qei_maximize: ctx is null' in err()
  for a in (val, grad, x, v):
    assert np.all(a == 7.0)                               # no output was touched
  assert np.all(status == 7) and not state.any()


def test_python_surface():
  """The constants mirror hbo.h, base_samples is [num_base, q] float64 and reproducible from its key, and a model without observations
  (the prior branch) is refused with ValueError by the value paths while suggest draws distinct candidates."""
  import types
  assert (nat.QEI_MAX_Q, nat.QEI_MAX_BASE) == (16, 1024)
  q = acfun.BatchExpectedImprovement(num_base=33)
  z = q.base_samples(3, 5)
  assert z.shape == (33, 3) and z.dtype == np.float64 and np.array_equal(z, q.base_samples(3, np.random.default_rng(5)))
  assert acfun.q_expected_improvement.num_base == 256 and acfun.q_expected_improvement.starts == 8
  with pytest.raises(ValueError):
    acfun.BatchExpectedImprovement(num_base=1025)
  model = types.SimpleNamespace(has_observations=lambda key: False, rng=None, input_dim=2, dataset={})
  with pytest.raises(ValueError, match='prior branch'):
    q(model=model, sub_dataset_key='t', x_batches=np.zeros((1, 3, 2)), base_samples=z)
  xc = np.random.default_rng(0).uniform(size=(20, 2))
  a = q.suggest(model=model, sub_dataset_key='t', x_candidates=xc, key=3, batch_size=4)
  assert a.shape == (4, 2) and len({tuple(r) for r in a}) == 4 and np.array_equal(a, q.suggest(model=model, sub_dataset_key='t', x_candidates=xc, key=3, batch_size=4))
  assert all(any(np.array_equal(r, c) for c in xc) for r in a)
  with pytest.raises(ValueError):
    q.suggest(model=model, sub_dataset_key='t', x_candidates=xc, key=3, batch_size=17)
