"""hbo_acq_grad across feature widths, query counts and cache sizes (run with `-m gpu` on an MI355X): the C entry point itself -- the
gradient bayesopt() hands to L-BFGS-B for every model the fused n <= 128 path refuses -- against oracle/hyperbo_oracle.py:
acquisition_value_and_grad, PER QUERY, for UCB(3), EI and PI at one shared target per case (the median posterior mean of the queries or, for
about a third of the cases, one standard deviation above it: acq_grad_cases.reference).  Cases, reference and bounds live in
tests/acq_grad_cases.py and are judged on their own by tests/test_acq_grad_cases_host.py (conditions, mutants, the oracle against
central differences); conditions 1 - 3 are asserted here again for every case.

What the cases reach that nothing else in the suite does (csrc/post.hip, csrc/acq_grad.hip: hbo_acq_grad):
  A  acq_grad_kernel's thread layout FD = next_pow2(features), G = 256 / FD groups: FD 1 .. 256, G 256 .. 1, the `d += 256` fill of s_fq
  B  the MLP backward to the query: last layers up to 256, a hidden layer wider than both ends, four layers, the gmlp = d_t0 branch
  C  M = 1 (tri_matvec_kernel) against M >= 2 (tri_matmat_*_kernel, partial groups of 8), both sides of the 1024-query pass
  D  cache sizes across the 64-column workgroups and 256-row LDS chunks of tri_matmat_trans_kernel, n = 1 and 2
  E  the prior branch (no cache) at widths 17 and 256
  F  kumar_chain_dx_kernel at widths 1 .. 256

Bounds (acq_grad_cases.py; the project's own): fp64 value rtol 1e-8 + atol 1e-10, gradient max_d |g - g_ref| <= 1e-7 (1 + gamma^2)
max_d |g_ref| per query; fp32 value within 5e-3 of max |v_ref|, gradient 2e-2 (1 + gamma^2) max_d |g_ref| per query at |gamma| <= 3.

Worst ratios to the bounds observed on an MI355X, per group (each test prints its own with -s and appends it to $HBO_GRAD_LOG when set):
           fp64 value        fp64 gradient      fp32 value        fp32 gradient
  A        1.8e-3 (PI, d 2)  4.1e-6 (UCB, d 5)  5.5e-2 (EI, d 5)  9.3e-3 (EI, d 5, gamma 0.84; all four at dot_product + linear)
  B        2.3e-3 (PI)       3.0e-6 (UCB)       2.4e-2 (EI)       3.7e-3 (EI, gamma 0.88; all four at dot_product, stack (12, 33))
  C        1.3e-3 (M 1025)   4.3e-6 (M 2049)    1.1e-2 (M 1024)   1.2e-2 (M 1024, query 53, Kumaraswamy SE, gamma -0.19)
  D        5.5e-4 (n 384)    9.7e-6 (n 383)     3.4e-2 (n 513)    2.0e-2 (n 513, M 1, dot_product + linear, UCB)
  E        4.3e-6            1.7e-8             3.0e-4            4.2e-5 (d 256, squared_exponential + linear, EI)
  F        1.0e-3 (d 1)      2.1e-6 (d 1)       2.1e-2 (d 17)     4.6e-3 (d 1, UCB)
  M = 1 against M = 1025 (of twice the bound): fp64 2.3e-8, fp32 5.1e-4; workspace re-use: value 6.7e-4, gradient 1.2e-6, and the
  second run of the largest case identical to the first in every bit.
  No group comes near its bound (fp64 <= 2.3e-3, fp32 <= 5.5e-2 of it) and no case failed: the new shapes exposed no defect.
hbo_acq_grad never routes to the fused path (hbo_acq_grad_samples); the tests call the entry point directly and assert that the
context's `acq_fused` option is at its default, so nothing in between can route elsewhere."""
import os
import types

import numpy as np
import pytest

import acq_grad_cases as G

pytestmark = pytest.mark.gpu
IDS = lambda c: c.id
_WORST = {}


def _native():
  from hyperbo_amd import _model as hmodel
  from hyperbo_amd import _native as nat
  from hyperbo_amd.basics import definitions as defs, linalg
  from hyperbo_amd.gp_utils import kernel, mean, utils
  return types.SimpleNamespace(hmodel=hmodel, nat=nat, defs=defs, linalg=linalg, kernel=kernel, mean=mean, utils=utils)


def _record(label, ratio, where):
  """Worst ratio to a bound per label: printed (-s) and appended to $HBO_GRAD_LOG."""
  if ratio > _WORST.get(label, (-1.0, None))[0]:
    _WORST[label] = (ratio, where)
  print(f'\nacq grad shapes: {label}: worst ratio to the bound {ratio:.3e} at {where}')
  log = os.environ.get('HBO_GRAD_LOG')
  if log:
    with open(log, 'a') as f:
      f.write(f'{ratio:.3e} acq_grad_shapes {label} at {where} {os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]}\n')


def _hip_or_exit(nat, fn):
  """fn(); a HIP error (a faulted device fails every later call too) ends the session instead of running the remaining few hundred
  cases on it."""
  try:
    return fn()
  except nat.HboError as e:
    if e.code == nat.HBO_ERR_HIP:
      pytest.exit(f'HIP error, nothing more is run on this device: {e}', returncode=3)
    raise


class _Device:
  """The hbo_model of a case and, with observations, its factorised cache: one factorisation per case."""

  def __init__(self, gpu_ctx, case):
    nv = _native()
    model, x, y, xq = G.inputs(case)
    pn = nv.defs.GPParams(model=model, config=dict(G.config(case)))
    kn, mn = getattr(nv.kernel, case.kernel_name), getattr(nv.mean, case.mname)
    wf = nv.utils.DEFAULT_WARP_FUNC
    self.case, self.nat, self.ctx, self.xq = case, nv.nat, gpu_ctx, xq
    self.noise = G.oracle_setup(case).noise
    assert gpu_ctx.get_option('acq_fused') == 0     # the default: nothing routes to the fused n <= 128 path
    self.h = _hip_or_exit(nv.nat, lambda: nv.linalg.factor(mn, kn, pn, x, y, wf, ctx=gpu_ctx)) if case.n else None
    if self.h is not None:
      assert self.h.status == nv.nat.HBO_OK and self.h.dtype == case.np_dtype
    self.bm = nv.hmodel.BuiltModel(mn, kn, pn, wf, case.np_dtype, case.d)

  def acq_grad(self, acq, param, xq=None):
    """hbo_acq_grad itself (not acfun.*.value_and_grad, which is allowed to route elsewhere)."""
    nat, case = self.nat, self.case
    xq = self.xq if xq is None else np.ascontiguousarray(xq)
    assert xq.dtype == case.np_dtype
    m_q = xq.shape[0]
    out = np.full((m_q, 1), np.nan, dtype=case.np_dtype)
    grad = np.full((m_q, case.d), np.nan, dtype=np.float64)
    rc = nat.lib().hbo_acq_grad(self.ctx.handle, self.bm.ref(), self.h.handle if self.h is not None else None, nat.ptr(xq), m_q,
                                G.ACQ_IDS[acq], float(param), self.noise, G.SCALE, nat.ptr(out),
                                grad.ctypes.data_as(nat.C.POINTER(nat.C.c_double)))
    _hip_or_exit(nat, lambda: self.ctx.check(rc, allow_not_pd=False))
    # the fp32 gradient comes back as float64 too (grad_out is double*)
    assert out.dtype == case.np_dtype and grad.dtype == np.float64
    return out[:, 0], grad

  def close(self):
    if self.h is not None:
      self.h.close()


def _judge(case, ref, acq, val, grad, label=None):
  """Value and gradient of one call per query against the module's bounds; records the worst ratios under the case's group."""
  (rv, qv), (rg, qg, gam) = G.worst(case, acq, ref, val, grad)
  label = label or f'{case.group} {case.dtype}'
  _record(f'{label} value', rv, f'query {qv} {acq} {case.id}')
  _record(f'{label} gradient', rg, f'query {qg} gamma {gam:.2f} {acq} {case.id}')
  ratios_v, ratios_g = G.ratios(case, acq, ref, val, grad)
  bad_v = [(int(q), float(val[q]), float(ref.val[acq][q]), float(ratios_v[q])) for q in np.flatnonzero(~(ratios_v <= 1.0))]
  bad_g = [(int(q), round(float(ref.gamma[acq][q]), 3), float(ratios_g[q])) for q in np.flatnonzero(~np.isnan(ratios_g) & ~(ratios_g <= 1.0))]
  assert not bad_v, f'{case.id} {acq}: {len(bad_v)} values beyond the bound; first (query, value, reference, ratio): {bad_v[:5]}'
  assert not bad_g, f'{case.id} {acq}: {len(bad_g)} gradients beyond the bound; first (query, gamma, ratio): {bad_g[:5]}'


def _run_case(gpu_ctx, case, label=None):
  ref = G.reference(case)
  assert G.conditions(case, ref) == [], case.id
  assert all(G.checked(case, acq, ref).any() for acq in G.ACQS), case.id
  dev = _Device(gpu_ctx, case)
  try:
    out = {}
    for acq in G.ACQS:
      val, grad = dev.acq_grad(acq, G.acq_param(acq, ref))
      _judge(case, ref, acq, val, grad, label)
      out[acq] = (val, grad)
    return out
  finally:
    dev.close()


@pytest.mark.parametrize('case', G.CASES_A, ids=IDS)
def test_plain_widths(gpu_ctx, case):
  """A: every layout of acq_grad_kernel's feature reduction; the linear mean's d weights through acq_grad_mean_kernel.  From 32
  features the fp32 cross Gram goes to the matrix cores while the kernel recomputes u directly."""
  _run_case(gpu_ctx, case)


@pytest.mark.parametrize('case', G.CASES_B, ids=IDS)
def test_mlp_widths(gpu_ctx, case):
  """B: the MLP backward to the query, the kernel's features and / or the mean's through it."""
  _run_case(gpu_ctx, case)


@pytest.mark.parametrize('case', G.CASES_C, ids=IDS)
def test_query_counts(gpu_ctx, case):
  """C: M = 1, the groups of 8 right-hand sides, both sides of the 1024-query pass.  At M = 1025 the rows of queries 0, 1023 and 1024
  also agree with three M = 1 calls at those queries (tri_matvec_kernel against the tri_matmat kernels, the first pass against the
  second) within twice the per-query bound: both routes are within the bound of the oracle.  Agreement, not bit identity: the
  summation orders differ."""
  if case.M != 1025:
    _run_case(gpu_ctx, case)
    return
  ref = G.reference(case)
  assert G.conditions(case, ref) == [], case.id
  dev = _Device(gpu_ctx, case)
  try:
    for acq in G.ACQS:
      param = G.acq_param(acq, ref)
      val, grad = dev.acq_grad(acq, param)
      _judge(case, ref, acq, val, grad)
      judged = G.checked(case, acq, ref)
      for q in (0, 1023, 1024):
        v1, g1 = dev.acq_grad(acq, param, xq=dev.xq[q:q + 1])
        gam = float(ref.gamma[acq][q])
        if case.dtype == 'fp64':
          vb = G.FP64_VALUE_ATOL + G.FP64_VALUE_RTOL * abs(float(ref.val[acq][q]))
          gb = G.FP64_GRAD_TOL * (1.0 + gam * gam) * float(np.max(np.abs(ref.grad[acq][q])))
        else:
          vb = G.FP32_VALUE_TOL * float(np.max(np.abs(ref.val[acq])))
          gb = G.FP32_GRAD_TOL * (1.0 + gam * gam) * float(np.max(np.abs(ref.grad[acq][q])))
        rv = abs(float(v1[0]) - float(val[q])) / (2.0 * vb)
        rg = float(np.max(np.abs(g1[0] - grad[q]))) / (2.0 * gb)
        _record(f'C {case.dtype} M = 1 against M = 1025', max(rv, rg if judged[q] else 0.0), f'query {q} {acq} {case.id}')
        assert np.isfinite(v1).all() and np.isfinite(g1).all()
        assert rv <= 1.0, (case.id, acq, q, float(v1[0]), float(val[q]), rv)
        assert rg <= 1.0 or not judged[q], (case.id, acq, q, gam, rg)
  finally:
    dev.close()


@pytest.mark.parametrize('case', G.CASES_D, ids=IDS)
def test_cache_sizes(gpu_ctx, case):
  """D: n on both sides of the 64-column workgroups, the 128-row padding and the 256-row chunks (with the half last chunk at an odd
  number of 128-row blocks), down to one and two observations; M = 1 and M = 9."""
  _run_case(gpu_ctx, case)


@pytest.mark.parametrize('case', G.CASES_E, ids=IDS)
def test_prior_branch(gpu_ctx, case):
  """E: no cache.  The stationary gradient is the mean part only; the dot product keeps its own 2 a_var f / sigma^2 term."""
  _run_case(gpu_ctx, case)


@pytest.mark.parametrize('case', G.CASES_F, ids=IDS)
def test_kumar_widths(gpu_ctx, case):
  """F: d acq / d w(x) * dw/dx per column, every column with its own a, b."""
  _run_case(gpu_ctx, case)


def test_workspaces_are_reused_across_shapes(gpu_ctx):
  """One context, in order: the largest case (n = 513, M = 1025, D = 64: two passes), n = 2 with M = 1 and D = 1, the prior branch at
  D = 256, the largest case again -- each against its own reference, and the last bit-identical to the first: nothing a smaller call
  leaves in a pooled workspace (or a larger one left before it) reaches a result."""
  big, tiny, prior = G.reuse_cases()
  first = _run_case(gpu_ctx, big, 'workspace re-use')
  _run_case(gpu_ctx, tiny, 'workspace re-use')
  _run_case(gpu_ctx, prior, 'workspace re-use')
  again = _run_case(gpu_ctx, big, 'workspace re-use')
  for acq in G.ACQS:
    assert first[acq][0].tobytes() == again[acq][0].tobytes(), acq
    assert first[acq][1].tobytes() == again[acq][1].tobytes(), acq
