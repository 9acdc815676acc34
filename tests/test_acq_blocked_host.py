"""CPU tier of the acquisition gradient and device maximiser beyond 128 observations (hbo_acq_grad_samples_blocked,
hbo_acq_maximize_blocked, model.params.config['acq_blocked']): tests/acq_blocked_cases.py judged on its own -- every edge of the blocked
kernels is covered, every case meets the conditions of acq_grad_cases, the NumPy restatement of the blocked route is inside the GPU
tier's bounds and every mutant of it is outside them on some case, the maximiser cases clear their thresholds -- and the host side of the
feature: the exports and their bindings, the argument checks that run before any device call, the routing helpers with and without
the opt-in."""
import ctypes as C
import functools

import numpy as np
import pytest

import acq_blocked_cases as B
import acq_grad_cases as G
from hyperbo_amd import _native as nat
from hyperbo_amd.basics import definitions as defs
from hyperbo_amd.bo_utils import acfun
from hyperbo_amd.gp_utils import gp, kernel, mean

CASES = [gc.case for gc in B.GRAD_CASES]


def test_every_edge_is_covered():
  assert len(B.GRAD_CASES) == 40 and len({c.id for c in CASES}) == 40
  assert {c.n for c in CASES} == set(B.NS) == {129, 192, 193, 255, 256, 257, 384, 385, 513}
  assert {c.M for c in CASES} == set(B.MS) == {1, 7, 8, 9, 17}
  assert {c.d for c in CASES} == set(B.DS) == {1, 5, 33, 256}
  assert {G.groups_of_reduction(c) for c in CASES} == {256, 32, 4, 1}
  assert {gc.S for gc in B.GRAD_CASES} == {1, 3}
  assert len({(c.kname, c.mname) for c in CASES}) == 12 and {c.mname for c in CASES} == {'zero', 'constant', 'linear'}
  assert set(G.ACQS) == {'ucb', 'ei', 'pi'}                 # every case is judged for all three
  for dt in G.DTYPES:
    sub = [c for c in CASES if c.dtype == dt]
    assert len(sub) >= 12 and {c.kname for c in sub} == set(G.KERNELS) and {c.mname for c in sub} == set(B.MEANS), dt
    # both dtypes: one row in the second block, the 64-column edge, the 256-row chunk edge with a half last chunk, five blocks
    assert {129, 193, 256, 257, 513} <= {c.n for c in sub}, dt
    assert {c.M for c in sub} == set(B.MS) and {c.d for c in sub} == set(B.DS), dt
  # S = 3 meets a cache of more than one 256-row chunk, in both dtypes
  assert {gc.case.dtype for gc in B.GRAD_CASES if gc.S == 3 and gc.case.n > 256} == set(G.DTYPES)
  for gc in B.GRAD_CASES:
    comp = B.companions(gc)
    assert len(comp) == gc.S - 1 and all(c._replace(group=gc.case.group) == gc.case for c in comp)
  assert {c.n for c in B.OPT_CASES} == {129, 257, 385} and {c.S for c in B.OPT_CASES} == {1, 3} and {c.R for c in B.OPT_CASES} == {1, 9}


@pytest.mark.parametrize('gc', B.GRAD_CASES, ids=lambda gc: gc.id)
def test_every_case_meets_the_conditions(gc):
  """acq_grad_cases.conditions from the oracle alone, the cap on fp32 queries left out of the gradient check (at most ceil(M / 9) beyond
  |gamma| = 3) included.  A case that fails here gets another group letter in acq_blocked_cases.RESEED."""
  assert G.conditions(gc.case, G.reference(gc.case)) == []


@functools.lru_cache(maxsize=None)
def _worst(case, name):
  """The largest ratio to the GPU tier's bounds, over the acquisitions and queries, of the restatement (name None) or a mutant."""
  ref = G.reference(case)
  fn = B.blocked_route if name is None else B.MUTANTS[name]
  worst = 0.0
  for acq in G.ACQS:
    rv, rg = G.ratios(case, acq, ref, *fn(case, acq, G.acq_param(acq, ref)))
    worst = max(worst, float(np.max(rv)), float(np.nanmax(rg)))
  return worst


@pytest.mark.parametrize('gc', B.GRAD_CASES, ids=lambda gc: gc.id)
def test_the_blocked_route_restated_is_inside_the_bounds(gc):
  """The restatement the mutants are cut from computes what the oracle computes: within 1 / MUTANT_FACTOR of the bounds, so that a
  mutant MUTANT_FACTOR bounds from the oracle is as far from the route it was cut from, up to a hundredth of a bound."""
  assert _worst(gc.case, None) <= 1.0 / G.MUTANT_FACTOR


@pytest.mark.parametrize('name', sorted(B.MUTANTS))
def test_every_mutant_is_rejected_by_the_bounds_of_the_gpu_tier(name):
  """fp64: some case sees the mutant by MUTANT_FACTOR bounds; fp32: some case's fp32 bounds see it at all."""
  for dtype, factor in (('fp64', G.MUTANT_FACTOR), ('fp32', G.FP32_MUTANT_FACTOR)):
    seen = {c.id: _worst(c, name) for c in CASES if c.dtype == dtype and B.applicable(name, c)}
    assert seen, (name, dtype)
    assert max(seen.values()) >= factor, (name, dtype, seen)


def test_mutant_applicability_follows_the_shapes():
  by_n = {c.n: c for c in CASES if c.M >= 2}
  assert not B.applicable('beta_half_chunk', by_n[192]) and B.applicable('beta_half_chunk', by_n[257]) and not B.applicable('beta_half_chunk', by_n[385])
  assert not B.applicable('ll_first_chunk', by_n[256]) and B.applicable('grad_first_chunk', by_n[257])
  assert not any(B.applicable('neighbour_k', c) for c in CASES if c.M == 1)


def test_maximiser_cases_clear_their_thresholds():
  """As test_acq_opt_host.py::test_cases_clear_their_thresholds: no decision of any start within a relative 1e-6 of its threshold."""
  close = {(c.name, r): B.opt_run(c, r).margin for c in B.OPT_CASES for r in range(c.R)}
  close = {k: m for k, m in close.items() if not m >= 1e-6}
  assert not close, close
  # and the cases have a loop to test: some start takes main steps and line-search probes
  kinds = {e[0] for c in B.OPT_CASES for r in range(c.R) for e in B.opt_run(c, r).log}
  assert {B.ao.START, B.ao.MAIN, B.ao.LINE_SEARCH} <= kinds


# ---- the host side of the feature --------------------------------------------------------------------------------------------------
NEW = ('hbo_acq_grad_samples_blocked', 'hbo_acq_maximize_blocked', 'hbo_probe_acq_grad_samples_blocked64')


def test_entry_points_are_exported_and_bound():
  for name in NEW:
    assert name in nat.SIGNATURES, name
    f = getattr(nat.lib(), name)
    res, args = nat.SIGNATURES[name]
    assert f.restype is res and list(f.argtypes) == args, name
  assert nat.SIGNATURES['hbo_acq_grad_samples_blocked'] == nat.SIGNATURES['hbo_acq_grad_samples']
  assert nat.SIGNATURES['hbo_acq_maximize_blocked'] == nat.SIGNATURES['hbo_acq_maximize']
  old = nat.SIGNATURES['hbo_probe_acq_grad_samples64'][1]
  assert nat.SIGNATURES['hbo_probe_acq_grad_samples_blocked64'][1] == old[:-1] + [C.c_int32, C.c_int64] + old[-1:]


def test_entry_points_are_documented():
  import os
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  hbo, tune = (open(os.path.join(root, 'include', f)).read() for f in ('hbo.h', 'hbo_tune.h'))
  assert 'int hbo_acq_grad_samples_blocked(' in hbo and 'int hbo_acq_maximize_blocked(' in hbo
  assert 'int hbo_probe_acq_grad_samples_blocked64(' in tune and 'force_blocked' in tune and 'chunk_queries' in tune
  for text, name in ((hbo, 'int hbo_acq_grad_samples_blocked('), (tune, 'int hbo_probe_acq_grad_samples_blocked64(')):
    doc = text[:text.index(name)].rsplit('/*', 1)[1]
    assert 'atomics' in doc and 'order' in doc, name      # the determinism statement


def test_argument_errors_come_before_any_device_call():
  err = lambda: (nat.lib().hbo_last_error(None) or b'').decode()
  xq, out, grad, v64 = np.zeros((1, 2)), np.full((1, 1), 7.0), np.full((1, 1, 2), 7.0), np.full((1, 1), 7.0)
  models, caches, prm, nse = (nat.Model * 1)(), (C.c_void_p * 1)(), (C.c_double * 1)(), (C.c_double * 1)()
  pd = C.POINTER(C.c_double)
  call = lambda S=1, acq_id=nat.ACQ_EI, m=models: nat.lib().hbo_acq_grad_samples_blocked(None, m, S, caches, nat.ptr(xq), 1, acq_id, prm, nse, 1.0,
                                                                                         nat.ptr(out), grad.ctypes.data_as(pd))
  assert call(m=None) == nat.HBO_ERR_ARG and 'hbo_acq_grad_samples_blocked: null argument' in err()
  assert call(S=4097) == nat.HBO_ERR_ARG and '1 <= S <= 4096' in err()
  assert call(acq_id=3) == nat.HBO_ERR_ARG and 'bad acq_id' in err()
  assert call() == nat.HBO_ERR_ARG and 'ctx is null' in err()
  probe = lambda chunk, v: nat.lib().hbo_probe_acq_grad_samples_blocked64(None, models, 1, caches, nat.ptr(xq), 1, nat.ACQ_EI, prm, nse, 1.0, nat.ptr(out),
                                                                          grad.ctypes.data_as(pd), 1, chunk, v)
  assert probe(0, None) == nat.HBO_ERR_ARG and 'val64_out is null' in err()
  assert probe(-1, v64.ctypes.data_as(pd)) == nat.HBO_ERR_ARG and 'chunk_queries < 0' in err()
  opts = nat.AcqOptOpts(**acfun.ACQ_OPT_DEFAULTS)
  ns = nat.lib().hbo_acq_opt_state_doubles(2, opts.memory)
  state, x, val, status = np.zeros((1, ns)), np.full((1, 2), 7.0), np.full(1, 7.0), np.full(1, 7, dtype=np.int32)
  mx = lambda S=1, acq_id=nat.ACQ_EI: nat.lib().hbo_acq_maximize_blocked(None, models, S, caches, nat.ptr(xq), 1, None, None, acq_id, prm, nse, 1.0,
                                                                         C.byref(opts), nat.ptr(state), 1, nat.ptr(x), nat.ptr(val), nat.ptr(status), None)
  assert mx() == nat.HBO_ERR_ARG and 'hbo_acq_maximize_blocked: ctx is null' in err()
  assert mx(S=0) == nat.HBO_ERR_ARG and 'hbo_acq_maximize_blocked: 1 <= S <= 4096' in err()
  assert mx(acq_id=-1) == nat.HBO_ERR_ARG and 'bad acq_id' in err()
  for a in (out, grad, v64, x, val):
    assert np.all(a == 7.0)                               # no output was touched
  assert np.all(status == 7) and not state.any()


class _Params:
  def __init__(self, config):
    self.config = config


def _stub(n, config=None, cov=kernel.matern52, mean_func=mean.constant, hgp=True, d=3):
  ds = {'t': defs.SubDataset(np.zeros((n, d)), np.zeros((n, 1))), 'other': defs.SubDataset(np.zeros((4, d)), np.zeros((4, 1)))}
  params = defs.GPParams(model={'constant': 1.0}, samples=[{'constant': 1.0}] * 3 if hgp else None, config=config)
  return (gp.HGP if hgp else gp.GP)(ds, mean_func, cov, params)


def test_the_opt_in_lifts_the_limit_and_nothing_else():
  on, off = {'acq_blocked': True}, {}
  sub = acfun.expected_improvement_sub
  for n in (129, 513):
    m = _stub(n, on)
    assert acfun._acq_blocked(m) and acfun._blocked_max_n(m) is None
    assert acfun._acq_fused_unmet(m, 't', 3, 3, enabled=True, max_n=acfun._blocked_max_n(m)) is None
    assert acfun._acq_opt_unmet(m, 't', sub, 3, 3, max_n=acfun._blocked_max_n(m)) is None
    assert acfun._acq_opt_unmet(_stub(n, on, hgp=False), 't', sub, max_n=None) is None
  # without the key (or with it off) the limit and its message are today's; the defaults of the helpers are untouched
  for cfg in (off, {'acq_blocked': False}, {'acq_blocked': 0}):
    m = _stub(129, cfg)
    assert not acfun._acq_blocked(m) and acfun._blocked_max_n(m) == acfun.ACQ_FUSED_MAX_N == 128
    assert '129 > 128' in acfun._acq_fused_unmet(m, 't', 3, 3, enabled=True, max_n=acfun._blocked_max_n(m))
    assert '129 > 128' in acfun._acq_opt_unmet(m, 't', sub, 3, 3, max_n=acfun._blocked_max_n(m))
  assert '129 > 128' in acfun._acq_fused_unmet(_stub(129, on), 't', 3, 3, enabled=True)
  assert '129 > 128' in acfun._acq_opt_unmet(_stub(129, on), 't', sub)
  # every other refusal stays with the opt-in, in today's order
  unmet = lambda m, *a: acfun._acq_fused_unmet(m, 't', *a, enabled=True, max_n=None)
  assert 'acq_fused' in acfun._acq_fused_unmet(_stub(513, on), 't', 3, 3, max_n=None)      # no default context: the option is off
  assert 'no observations' in unmet(_stub(0, on), 3, 3)
  assert 'MLP basis' in unmet(_stub(513, on, cov=kernel.matern52_mlp), 3, 3)
  assert 'linear_mlp' in unmet(_stub(513, on, mean_func=mean.linear_mlp), 3, 3)
  assert 'Kumaraswamy' in unmet(_stub(513, on, cov=kernel.matern52_kumar), 3, 3)
  assert 'only 2 of the 3' in unmet(_stub(513, on), 3, 2)
  assert 'not one of the native ones' in acfun._acq_opt_unmet(_stub(513, on), 't', lambda mu, std, p: mu, max_n=None)
  # a model without params (the stubs of the other host tests) has not opted in
  assert not acfun._acq_blocked(object()) and not acfun._acq_blocked(type('M', (), {'params': _Params(None)})())


def test_maximize_refuses_129_observations_without_the_opt_in():
  with pytest.raises(nat.HboError) as e:
    acfun.ucb.maximize(model=_stub(129, {}, hgp=False), sub_dataset_key='t', x_init=np.full(3, 0.5))
  assert e.value.code == nat.HBO_ERR_UNSUPPORTED and '129 > 128' in str(e.value)
  # with it the host-side checks pass: what stops the call on a machine without a device is the device, not a refusal
  with pytest.raises(nat.HboError) as e:
    acfun.ucb.maximize(model=_stub(129, {'acq_blocked': True}, cov=kernel.matern52_mlp, hgp=False), sub_dataset_key='t', x_init=np.full(3, 0.5))
  assert e.value.code == nat.HBO_ERR_UNSUPPORTED and 'MLP basis' in str(e.value)


def test_the_opt_in_is_documented():
  import os
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  for f in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
    assert 'acq_blocked' in open(os.path.join(root, f)).read(), f
  from hyperbo_amd.bo_utils import bayesopt
  assert "config['acq_blocked']" in bayesopt.bayesopt.__doc__ and 'raises HboError(HBO_ERR_UNSUPPORTED)' in bayesopt.bayesopt.__doc__
