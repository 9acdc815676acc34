"""The O(N^2) row append (hbo_cache_append, csrc/cache.hip) on caches of more than one 128-row block (run with `-m gpu` on an MI355X),
against the oracle's from-scratch factorisation of the same data: tests/append_cases.py holds the cases, the reference, the bounds
and the mutants these checks are known to reject (tests/test_append_cases_host.py).

Everything goes through gp.GP.update_sub_dataset(is_append=True) + predict (the refusal and the failing row also call the C entry
point).  Every call ASSERTS THAT THE APPEND HAPPENED: the cache handle is the same object before and after, except where the case
says that the rows no longer fit (the capacity edge's last call) -- a silent re-factorisation passes every numerical check.

After each call (append_cases.errors): rows n0: of chol on their own, the rows from before the call bit-identical to the export before
it, kinvy over :n0 and n0: each on its own, ymu, and mu / var per query at 40 queries of which three are appended points.
fp64: the bounds of the one-block test (chol 1e-9, kinvy 1e-8, mu / var 1e-8).  The drift case (60 single-row calls) and the fp32
cases: err_append <= 4 err_fresh + 8 eps(dtype) per part, err_fresh from the device's own fresh factorisation of the same data in the
same dtype (append_cases.relative_bounds), and the bounds so measured must still see every mutant (append_cases.unseen_mutants).

Measured on an MI355X: RATIOS_MEASURED below (HBO_APPEND_LOG=<file> records every figure of a run).  No fp64 case uses more
than 1.4e-5 of a chol / kinvy bound, 8.3e-4 of the per-query mu bound (floored at 1e-3 of the largest mean), 9.5e-7 of the var bound."""
import os
import types

import numpy as np
import pytest

import append_cases as A
import helpers
from oracle import hyperbo_oracle as o

pytestmark = pytest.mark.gpu
WFO = o.DEFAULT_WARP_FUNC
IDS = lambda c: c.id

# Worst err_append / err_fresh over all calls of a case, per quantity (part_errors of the appended cache over array_errors of the device's
# fresh factorisation, both against the fp64 oracle), measured on an MI355X.  The bound allows REL_FACTOR = 4 (+ 8 eps); nothing
# measured reaches 2, so 60 appended rows cost less than one more fresh factorisation's error.  ymu is 1.00 throughout fp32 (the same
# rounding of y - m(x) on both sides) and exact in fp64.
RATIOS_MEASURED = {
    #                chol_new kinvy_old kinvy_new  mu    var   mu_new var_new
    'drift fp64':     (1.44,   1.08,     1.09,    1.68, 1.33,  1.23,  1.33),
    'drift fp32':     (1.41,   1.32,     1.83,    1.76, 1.12,  1.38,  1.00),
    '129 +1 fp32':    (0.93,   1.00,     0.13,    0.88, 0.87,  0.19,  0.21),
    '200 +7+1+1 fp32': (0.73,  1.07,     1.14,    0.90, 1.00,  0.78,  0.47),
    '513 +3 fp32':    (0.64,   1.02,     0.31,    1.08, 1.00,  0.67,  0.46),
    '600 +40 fp32':   (0.85,   0.93,     0.38,    1.13, 1.00,  0.58,  0.98),
}


def _native():
  from hyperbo_amd import _model, _native as nat
  from hyperbo_amd.basics import definitions as defs, linalg
  from hyperbo_amd.bo_utils import acfun
  from hyperbo_amd.gp_utils import gp, kernel, mean, utils
  return types.SimpleNamespace(hmodel=_model, nat=nat, defs=defs, linalg=linalg, acfun=acfun, gp=gp, kernel=kernel, mean=mean, utils=utils)


def _log(line):
  print(line)
  path = os.environ.get('HBO_APPEND_LOG')
  if path:
    with open(path, 'a') as f:
      f.write(line + '\n')


def _fmt(d):
  return ' '.join(f'{k} {v:.2e}' for k, v in d.items())


def _gp(case, n):
  """A GP over the first n observations of the case, in the case's dtype."""
  nv = _native()
  model, x, y, _ = A.inputs(case)
  pn = nv.defs.GPParams(model=A.cast(model, case.np_dtype), config=dict(A.config(case)))
  return nv.gp.GP({0: nv.defs.SubDataset(x[:n], y[:n])}, getattr(nv.mean, case.mname), getattr(nv.kernel, case.kernel_name), pn, nv.utils.DEFAULT_WARP_FUNC)


def _state(m, xq):
  """Posterior at the queries and the export of the cache it came from."""
  mu, var = m.predict(xq, 0)
  h = m.params.cache[0].handle
  chol, kinvy, ymu = h.export()
  assert h.n == m.dataset[0].x.shape[0] == chol.shape[0]
  return A.State(h.n, chol, kinvy, ymu, mu[:, 0], var[:, 0])


def _calls(case):
  """The case's append calls through the GP object: per call (index, the GP, the State after it); the handle identity and
  the bit-identity of the rows of chol from before the call are asserted on the way."""
  _, x, y, xq = A.inputs(case)
  m = _gp(case, case.n0)
  before = _state(m, xq)
  for i, ((nb, n1), fits) in enumerate(zip(case.sizes, case.in_place)):
    h0 = m.params.cache[0].handle
    m.update_sub_dataset((x[nb:n1], y[nb:n1]), 0, is_append=True)
    after = _state(m, xq)
    h1 = m.params.cache[0].handle
    assert after.n == n1 and after.mu.dtype == case.np_dtype and after.chol.dtype == case.np_dtype
    if fits:
      assert h1 is h0, f'{case.id} call {i}: {nb} + {n1 - nb} rows fit the cache and were NOT appended in place'
      assert np.array_equal(after.chol[:nb, :nb], before.chol), f'{case.id} call {i}: the append changed rows of chol from before the call'
    else:
      assert h1 is not h0, f'{case.id} call {i}: {nb} + {n1 - nb} rows do not fit the cache'
    yield i, m, after
    before = after
  for c in m.params.cache.values():
    c.handle.close()


@pytest.mark.parametrize('case', A.FIXED_BOUND_CASES, ids=IDS)
def test_append_beyond_one_block_vs_refactorisation_fp64(gpu_ctx, case):
  ref = A.reference(case)
  bad = []
  for i, m, got in _calls(case):
    r = A.ratios(got, ref[i], case.n0)
    _log(f'append fp64 | {case.id} | call {i} | ratios to the bounds: {_fmt(r)}')
    bad += [(i, k, v) for k, v in r.items() if not v <= 1.0]
    if case in A.ONCE_CASES and i == 0:
      bad += [(i,) + b for b in _full_cov_and_acquisition(case, m, case.sizes[0][1])]
  assert not bad, f'{case.id}: (call, part, ratio to its bound) {bad}'


def _full_cov_and_acquisition(case, m, n):
  """predict(full_cov=True), expected_improvement and its value_and_grad on the appended cache against their oracle counterparts
  (tests/test_gpu_full_cov.py: test_full_cov_after_a_row_append; tests/test_gpu_parity.py: test_factor_predict_acquisition_vs_oracle,
  test_acquisition_value_and_grad_vs_oracle), at their bounds; hbo_acq_grad reads the same W through the same mat-vec helpers."""
  nv = _native()
  s = A.oracle_setup(case)
  x, y, xq = s.x[:n], s.y[:n], s.xq
  bad = []
  mu_o, cov_o = o.predict(s.mo, s.ko, s.po, x, y, xq, WFO, full_cov=True)
  mu, cov = m.predict(xq, 0, full_cov=True, with_noise=False, unbiased=False)
  e_cov, e_mu = float(np.max(np.abs(cov - cov_o)) / np.max(np.abs(cov_o))), helpers.rel_err(mu, mu_o)
  target = float(np.max(y))
  ref = A.reference(case)[0]
  ei_o = o.expected_improvement_sub(ref.mu[:, None], np.sqrt(ref.var[:, None]), target)
  ei = nv.acfun.expected_improvement(model=m, sub_dataset_key=0, x_queries=xq)
  e_ei = helpers.rel_err(ei, ei_o)
  vo, go = o.acquisition_value_and_grad('ei', s.mo, s.ko, s.po, x, y, xq, target, WFO, add_noise=s.noise, scale=1.0)
  val, grad = nv.acfun.expected_improvement.value_and_grad(model=m, sub_dataset_key=0, x_queries=xq)
  assert val.shape == (case.M, 1) and grad.shape == (case.M, case.d)
  e_val = float(np.max(np.abs(val - vo) / (1e-10 + 1e-8 * np.abs(vo))))
  e_grad = float(np.max(np.abs(grad - go)) / (1e-7 * max(np.max(np.abs(go)), 1e-3)))
  _log(f'append fp64 | {case.id} | full_cov {e_cov:.2e} (1e-8) mu {e_mu:.2e} (1e-8) EI {e_ei:.2e} (1e-8) value_and_grad: value {e_val:.2e} grad {e_grad:.2e} of their bounds')
  for name, e, b in (('full_cov', e_cov, 1e-8), ('full_cov mu', e_mu, 1e-8), ('ei', e_ei, 1e-8), ('ei value', e_val, 1.0), ('ei grad', e_grad, 1.0)):
    if not e <= b:
      bad.append((name, e / b))
  return bad


@pytest.mark.parametrize('case', [A.DRIFT] + A.FP32_CASES, ids=IDS)
def test_append_is_as_accurate_as_a_fresh_factorisation(gpu_ctx, case):
  """The drift case and the fp32 cases: per part err_append <= 4 err_fresh + 8 eps (append_cases.relative_bounds), both errors against the
  fp64 oracle, err_fresh from the device's own fresh factorisation of the same data in the same dtype -- code no row append runs.
  The 4: each appended row adds one more pair of length-n dot products accumulated in fp64 and rounded to the dtype.
  Worst err_append / err_fresh per quantity over all calls, as measured: RATIOS_MEASURED (1.83 at most)."""
  ref = A.reference(case)
  _, _, _, xq = A.inputs(case)
  bad, bounds, worst = [], [], {}
  for i, m, got in _calls(case):
    fresh_gp = _gp(case, got.n)
    fresh = A.array_errors(_state(fresh_gp, xq), ref[i])
    fresh_gp.params.cache[0].handle.close()
    e = A.part_errors(got, ref[i], case.n0)
    b = A.relative_bounds(fresh, case.np_dtype)
    bounds.append(b)
    for k in e:
      ratio = e[k] / fresh[A.PART_OF[k]] if fresh[A.PART_OF[k]] > 0 else (0.0 if e[k] == 0 else np.inf)
      worst[k] = max(worst.get(k, 0.0), ratio)
      if not e[k] <= b[k]:
        bad.append((i, k, e[k], b[k]))
    if len(case.calls) <= 3 or i % 10 == 9:
      _log(f'append {case.dtype} | {case.id} | call {i} | append: {_fmt(e)} | fresh: {_fmt(fresh)}')
  _log(f'append {case.dtype} | {case.id} | worst err_append / err_fresh: {_fmt(worst)}')
  assert not bad, f'{case.id}: (call, part, err_append, bound) {bad[:8]}; worst err_append / err_fresh {worst}'
  assert A.unseen_mutants(case, bounds) == set()      # the bounds so measured still reject every mutant


def test_one_row_more_than_fits_is_refused_and_changes_nothing(gpu_ctx):
  """250 observations, npad = 256: hbo_cache_append with 7 rows returns HBO_ERR_UNSUPPORTED and leaves the cache as it was, bit for
  bit; the 6 rows that do fit are then appended in place and are right."""
  nv = _native()
  nat = nv.nat
  case = A.EDGE
  _, x, y, xq = A.inputs(case)
  m = _gp(case, 250)
  before = _state(m, xq)
  h = m.params.cache[0].handle
  bm = nv.hmodel.BuiltModel(m.mean_func, m.cov_func, m.params, m.warp_func, np.float64, case.d, eps=1e-6)
  xa, ya = np.ascontiguousarray(x[250:257]), np.ascontiguousarray(y[250:257])
  rc = nat.lib().hbo_cache_append(gpu_ctx.handle, bm.ref(), h.handle, nat.ptr(xa), 7, nat.ptr(ya))
  assert rc == nat.HBO_ERR_UNSUPPORTED
  m.params.cache[0].invalidate_arrays()
  after = _state(m, xq)
  assert m.params.cache[0].handle is h
  for name in ('chol', 'kinvy', 'ymu', 'mu', 'var'):
    assert np.array_equal(getattr(after, name), getattr(before, name)), name
  m.update_sub_dataset((x[250:256], y[250:256]), 0, is_append=True)
  got = _state(m, xq)
  assert m.params.cache[0].handle is h and got.n == 256
  r = A.ratios(got, A.reference(case)[0], case.n0)
  _log(f'append fp64 | {case.id} | after the refusal | ratios to the bounds: {_fmt(r)}')
  assert max(r.values()) <= 1.0, r
  h.close()


def test_append_past_one_block_stops_at_a_row_that_breaks_the_factorisation(gpu_ctx):
  """test_append_stops_at_a_row_that_breaks_the_factorisation (tests/test_gpu_parity.py) at 200 observations, the row with the NaN input
  second of three: HBO_NOT_PD from the C entry point; through the GP object the NaN posterior of a fresh factorisation of the same
  data; a valid dataset works afterwards."""
  nv = _native()
  nat = nv.nat
  rng = np.random.default_rng(37)
  d = 3
  model = helpers.make_model(rng, 'constant', False, d)
  x, y = helpers.synthetic_task(rng, 200, d)
  xa, ya = helpers.synthetic_task(rng, 3, d)
  xa[1, 0] = np.nan
  xq = rng.uniform(size=(10, d))
  wf = nv.utils.DEFAULT_WARP_FUNC
  new = lambda: nv.gp.GP({0: nv.defs.SubDataset(x, y)}, nv.mean.constant, nv.kernel.squared_exponential, nv.defs.GPParams(model=model), wf)
  m = new()
  mu0, _ = m.predict(xq, 0)
  assert np.isfinite(mu0).all()
  bm = nv.hmodel.BuiltModel(nv.mean.constant, nv.kernel.squared_exponential, m.params, wf, np.float64, d, eps=1e-6)
  rc = nat.lib().hbo_cache_append(gpu_ctx.handle, bm.ref(), m.params.cache[0].handle.handle, nat.ptr(np.ascontiguousarray(xa)), 3,
                                  nat.ptr(np.ascontiguousarray(ya)))
  assert rc == nat.HBO_NOT_PD
  m.params.cache[0].handle.close()
  m2 = new()
  m2.predict(xq, 0)
  m2.update_sub_dataset((xa, ya), 0, is_append=True)
  mu, var = m2.predict(xq, 0)
  assert m2.dataset[0].x.shape[0] == 203 and np.isnan(mu).all() and np.isnan(var).all()
  m2.update_sub_dataset((x, y), 0)
  mu1, _ = m2.predict(xq, 0)
  assert helpers.rel_err(mu1, mu0) < 1e-12
  m2.params.cache[0].handle.close()
