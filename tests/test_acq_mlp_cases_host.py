"""CPU tier of the acquisition gradient and device maximiser for MLP-basis models (hbo_acq_grad_samples_mlp, hbo_acq_maximize_mlp,
model.params.config['acq_mlp']): tests/acq_mlp_cases.py judged on its own -- every case meets the conditions of acq_grad_cases, the
oracle's gradient agrees with central differences, the NumPy restatement of the device's route is inside a tenth of the GPU tier's
bounds and every mutant of it is outside them on every case it is listed for, the maximiser cases clear their thresholds and catch the
mutants of the optimiser -- and the host side of the feature: the exports and their bindings, the routing helpers with and without the
opt-in, the documents."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import acq_grad_cases as G
import acq_mlp_cases as A
import acq_opt_oracle as ao
from hyperbo_amd import _native as nat
from hyperbo_amd.basics import definitions as defs
from hyperbo_amd.bo_utils import acfun
from hyperbo_amd.gp_utils import gp, kernel, mean

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAM_FRACTION_MIN = 0.5     # condition 4, as tests/test_acq_grad_cases_host.py asks it


def test_the_case_list():
  assert len(A.CASES) == 156 and len({c.id for c in A.CASES}) == 156
  assert [len(g) for g in (A.CASES_S, A.CASES_T, A.CASES_U, A.CASES_V, A.CASES_L)] == [48, 14, 28, 24, 42]
  assert {c.feats for c in A.CASES_S} == set(A.S_STACKS) and {(c.mlp_k, c.mname) for c in A.CASES_S} == set(G.B_PAIRINGS)
  assert {(c.kname, c.ls) for c in A.CASES_T} == {(k, ls) for k in G.KERNELS for ls in G._ls_forms(k)}
  assert {(c.n, c.M) for c in A.CASES_U} == {(n, m) for n in (1, 2, 63, 64, 65, 127, 128) for m in (1, 9)}
  assert {c.d for c in A.CASES_V} == {1, 17, 64, 256} and {c.n for c in A.CASES_L} == {129, 257, 385}
  assert {c.kname for c in A.CASES_L} == {'matern52', 'dot_product'}
  for group in (A.CASES_S, A.CASES_T, A.CASES_U, A.CASES_V, A.CASES_L):
    assert {c.dtype for c in group} == set(G.DTYPES)
  assert all(c.n <= 128 for c in A.SMALL) and all(c.n > 128 for c in A.LARGE) and len(A.SMALL) + len(A.LARGE) == 156
  assert {c.feats for c in A.MULTI} >= set(A.S_STACKS) and {c.n for c in A.MULTI} == {100, 128, 129} and {c.dtype for c in A.MULTI} == set(G.DTYPES)
  assert {oc.acq for oc in A.OPT_CASES} == set(G.ACQS) and {oc.S for oc in A.OPT_CASES} == {1, 3} and {oc.R for oc in A.OPT_CASES} == {3}
  assert {(oc.case.mlp_k, oc.case.mname) for oc in A.OPT_CASES} == set(G.B_PAIRINGS) and {oc.case.n for oc in A.OPT_CASES} == {100, 129}


@pytest.mark.parametrize('case', A.CASES, ids=lambda c: c.id)
def test_every_case_meets_the_conditions(case):
  """acq_grad_cases.conditions from the oracle alone (every fp64 query judged, at most ceil(M / 9) fp32 queries beyond |gamma| = 3), and
  the Gram condition for stationary kernels with at least two observations.  A case that fails here gets another group letter or
  shape, never a looser bound."""
  assert G.conditions(case, G.reference(case)) == []
  if case.kname != 'dot_product' and case.n >= 2 and case.dtype == 'fp64':
    assert G.gram_fraction(case) >= GRAM_FRACTION_MIN, G.gram_fraction(case)


def _fd_cases():
  seen, out = set(), []
  for c in A.CASES:
    key = (c.group, c.mlp_k, c.mname)
    if c.dtype == 'fp64' and key not in seen:
      seen.add(key); out.append(c)
  return out


@pytest.mark.parametrize('case', _fd_cases(), ids=lambda c: c.id)
def test_the_oracle_gradient_agrees_with_central_differences(case):
  ref = G.reference(case)
  xq = G.oracle_setup(case).xq
  h = 1e-6
  for acq in G.ACQS:
    p = G.acq_param(acq, ref)
    for d in range(min(case.d, 3)):
      e = np.zeros(case.d); e[d] = h
      fd = (G.oracle_value_and_grad(case, acq, p, xq + e)[0] - G.oracle_value_and_grad(case, acq, p, xq - e)[0]) / (2 * h)
      scale = np.max(np.abs(ref.grad[acq]), axis=1)
      assert np.all(np.abs(fd - ref.grad[acq][:, d]) <= 1e-5 * scale + 1e-9), (acq, d)


@functools.lru_cache(maxsize=None)
def _worst(case, name):
  """The largest ratio to the GPU tier's bounds, over the acquisitions and queries, of the restatement (name None) or a mutant."""
  ref = G.reference(case)
  worst = 0.0
  for acq in G.ACQS:
    p = G.acq_param(acq, ref)
    val, grad = A.route(case, acq, p) if name is None else A.mutant(name, case, acq, p)
    worst = max(worst, A.distance(case, acq, ref, val, grad))
  return worst


@pytest.mark.parametrize('case', A.CASES, ids=lambda c: c.id)
def test_the_route_restated_is_inside_a_tenth_of_the_bounds(case):
  assert _worst(case, None) <= 0.1


@pytest.mark.parametrize('name', sorted(A.MUTANTS))
def test_every_mutant_is_rejected_on_every_case_it_is_listed_for(name):
  cases = A.mutant_cases(name)
  assert cases and {c.dtype for c in cases} == set(G.DTYPES)
  for c in cases:
    factor = G.MUTANT_FACTOR if c.dtype == 'fp64' else G.FP32_MUTANT_FACTOR
    assert _worst(c, name) >= factor, (name, c.id, _worst(c, name))


@pytest.mark.parametrize('case', A.MULTI, ids=lambda c: c.id)
def test_the_samples_differ_and_a_sample_under_the_first_one_s_weights_is_rejected(case):
  models = A.sample_models(case)
  assert len(models) == A.N_SAMPLES
  for i in range(1, A.N_SAMPLES):
    for leaf in ('lengthscale',):
      assert not np.array_equal(models[0][leaf], models[i][leaf])
    assert not np.array_equal(models[0]['mlp_params']['Dense_0']['kernel'], models[i]['mlp_params']['Dense_0']['kernel'])
    assert not np.array_equal(models[0]['linear_mean']['kernel'], models[i]['linear_mean']['kernel'])
  factor = G.MUTANT_FACTOR if case.dtype == 'fp64' else G.FP32_MUTANT_FACTOR
  ref0 = G.reference(case)
  for s in range(1, A.N_SAMPLES):
    far, near = 0.0, 0.0
    for acq in G.ACQS:
      p = G.acq_param(acq, ref0)
      ref = A.sample_reference(case, s, acq, p)
      near = max(near, A.distance(case, acq, ref, *A.route(case, acq, p, sample=s)))
      far = max(far, A.distance(case, acq, ref, *A.mutant_wrong_sample(case, s, acq, p)))
    assert near <= 0.1 and far >= factor, (s, near, far)


def test_maximiser_cases_clear_their_thresholds_and_catch_the_mutants():
  close = {(oc.name, r): A.opt_run(oc, r).margin for oc in A.OPT_CASES for r in range(oc.R)}
  close = {k: m for k, m in close.items() if not m >= 1e-6}
  assert not close, close
  runs = [A.opt_run(oc, r) for oc in A.OPT_CASES for r in range(oc.R)]
  assert {ao.START, ao.MAIN, ao.LINE_SEARCH} <= {e[0] for run in runs for e in run.log}
  assert all(run.status != ao.RUNNING for run in runs)            # every run ends within the evaluations of a device run
  # the optimiser's own mutants: each changes the decisions or the end point of some start of the list
  pool = [(oc, r) for oc in A.OPT_CASES if oc.S == 1 for r in range(oc.R)]
  for name in ao.MUTANTS:
    caught = False
    for oc, r in pool:
      good, bad = A.opt_run(oc, r), A.opt_run(oc, r, name)
      if [e[:2] for e in good.log] != [e[:2] for e in bad.log] or good.status != bad.status or not np.array_equal(good.x, bad.x):
        caught = True
        break
    assert caught, name


# ---- the host side of the feature --------------------------------------------------------------------------------------------------
NEW = ('hbo_acq_grad_samples_mlp', 'hbo_acq_maximize_mlp', 'hbo_probe_acq_grad_samples_mlp64')


def test_entry_points_are_exported_bound_and_documented():
  for name in NEW:
    assert name in nat.SIGNATURES, name
    f = getattr(nat.lib(), name)
    res, args = nat.SIGNATURES[name]
    assert f.restype is res and list(f.argtypes) == args, name
  assert nat.SIGNATURES['hbo_acq_grad_samples_mlp'] == nat.SIGNATURES['hbo_acq_grad_samples_blocked']
  assert nat.SIGNATURES['hbo_acq_maximize_mlp'] == nat.SIGNATURES['hbo_acq_maximize_blocked']
  assert nat.SIGNATURES['hbo_probe_acq_grad_samples_mlp64'] == nat.SIGNATURES['hbo_probe_acq_grad_samples_blocked64']
  hbo, tune = (open(os.path.join(ROOT, 'include', f)).read() for f in ('hbo.h', 'hbo_tune.h'))
  assert 'int hbo_acq_grad_samples_mlp(' in hbo and 'int hbo_acq_maximize_mlp(' in hbo and 'int hbo_probe_acq_grad_samples_mlp64(' in tune
  doc = hbo[:hbo.index('int hbo_acq_grad_samples_mlp(')].rsplit('/*', 1)[1]
  for word in ('atomics', 'order', 'FIVE', 'Kumaraswamy', 'prior branch', 'hbo_acq_grad'):
    assert word in doc, word


def test_argument_errors_come_before_any_device_call():
  err = lambda: (nat.lib().hbo_last_error(None) or b'').decode()
  xq, out, grad, v64 = np.zeros((1, 2)), np.full((1, 1), 7.0), np.full((1, 1, 2), 7.0), np.full((1, 1), 7.0)
  models, caches, prm, nse = (nat.Model * 1)(), (C.c_void_p * 1)(), (C.c_double * 1)(), (C.c_double * 1)()
  pd = C.POINTER(C.c_double)
  call = lambda S=1, acq_id=nat.ACQ_EI, m=models: nat.lib().hbo_acq_grad_samples_mlp(None, m, S, caches, nat.ptr(xq), 1, acq_id, prm, nse, 1.0,
                                                                                     nat.ptr(out), grad.ctypes.data_as(pd))
  assert call(m=None) == nat.HBO_ERR_ARG and 'hbo_acq_grad_samples_mlp: null argument' in err()
  assert call(S=4097) == nat.HBO_ERR_ARG and '1 <= S <= 4096' in err()
  assert call(acq_id=3) == nat.HBO_ERR_ARG and 'bad acq_id' in err()
  assert call() == nat.HBO_ERR_ARG and 'ctx is null' in err()
  probe = lambda chunk, v: nat.lib().hbo_probe_acq_grad_samples_mlp64(None, models, 1, caches, nat.ptr(xq), 1, nat.ACQ_EI, prm, nse, 1.0, nat.ptr(out),
                                                                      grad.ctypes.data_as(pd), 1, chunk, v)
  assert probe(0, None) == nat.HBO_ERR_ARG and 'val64_out is null' in err()
  assert probe(-1, v64.ctypes.data_as(pd)) == nat.HBO_ERR_ARG and 'chunk_queries < 0' in err()
  opts = nat.AcqOptOpts(**acfun.ACQ_OPT_DEFAULTS)
  ns = nat.lib().hbo_acq_opt_state_doubles(2, opts.memory)
  state, x, val, status = np.zeros((1, ns)), np.full((1, 2), 7.0), np.full(1, 7.0), np.full(1, 7, dtype=np.int32)
  mx = lambda S=1: nat.lib().hbo_acq_maximize_mlp(None, models, S, caches, nat.ptr(xq), 1, None, None, nat.ACQ_EI, prm, nse, 1.0,
                                                  C.byref(opts), nat.ptr(state), 1, nat.ptr(x), nat.ptr(val), nat.ptr(status), None)
  assert mx() == nat.HBO_ERR_ARG and 'hbo_acq_maximize_mlp: ctx is null' in err()
  assert mx(S=0) == nat.HBO_ERR_ARG and 'hbo_acq_maximize_mlp: 1 <= S <= 4096' in err()
  for a in (out, grad, v64, x, val):
    assert np.all(a == 7.0)
  assert np.all(status == 7) and not state.any()


def _stub(n, config=None, cov=kernel.matern52, mean_func=mean.constant, hgp=True, d=3):
  ds = {'t': defs.SubDataset(np.zeros((n, d)), np.zeros((n, 1))), 'other': defs.SubDataset(np.zeros((4, d)), np.zeros((4, 1)))}
  params = defs.GPParams(model={'constant': 1.0}, samples=[{'constant': 1.0}] * 3 if hgp else None, config=config)
  return (gp.HGP if hgp else gp.GP)(ds, mean_func, cov, params)


def test_the_opt_in_lifts_the_two_mlp_conditions_and_nothing_else():
  on = {'acq_mlp': True}
  sub = acfun.expected_improvement_sub
  unmet = lambda m, *a, **k: acfun._acq_fused_unmet(m, 't', *a, enabled=True, max_n=None, **k)
  for cov, mf in ((kernel.matern52_mlp, mean.linear_mlp), (kernel.matern52_mlp, mean.linear), (kernel.matern52, mean.linear_mlp)):
    for n in (100, 513):
      m = _stub(n, on, cov=cov, mean_func=mf)
      assert acfun._acq_mlp(m)
      assert unmet(m, 3, 3, allow_mlp=True) is None
      assert acfun._acq_opt_unmet(m, 't', sub, 3, 3, max_n=None, allow_mlp=True) is None
      # the helpers' defaults are today's: the same model is refused with today's messages
      assert unmet(m, 3, 3) == ('the kernel runs on an MLP basis' if cov is kernel.matern52_mlp else 'the mean is linear_mlp')
      assert acfun._acq_opt_unmet(m, 't', sub, 3, 3, max_n=None) == unmet(m, 3, 3)
  # every other condition stays under allow_mlp, in today's order and words
  full = dict(cov=kernel.matern52_mlp, mean_func=mean.linear_mlp)
  assert acfun._acq_fused_unmet(_stub(100, on, **full), 't', 3, 3, max_n=None, allow_mlp=True) == "the context option 'acq_fused' is off"
  assert unmet(_stub(0, on, **full), 3, 3, allow_mlp=True) == 'the sub-dataset has no observations (the prior branch)'
  assert acfun._acq_fused_unmet(_stub(129, on, **full), 't', 3, 3, enabled=True, allow_mlp=True) == 'the sub-dataset has 129 > 128 observations'
  assert unmet(_stub(100, on, cov=kernel.matern52_kumar), 3, 3, allow_mlp=True) == 'the kernel is input-warped (Kumaraswamy)'
  assert unmet(_stub(100, on, **full), 3, 2, allow_mlp=True) == 'only 2 of the 3 per-sample factors fit the device budget'
  assert 'not one of the native ones' in acfun._acq_opt_unmet(_stub(100, on, **full), 't', lambda mu, std, p: mu, max_n=None, allow_mlp=True)
  # the key is its own: acq_blocked does not set it, a model without params or config has not asked
  for cfg in ({}, {'acq_mlp': False}, {'acq_mlp': 0}, {'acq_blocked': True}):
    assert not acfun._acq_mlp(_stub(100, cfg, **full))
  assert not acfun._acq_mlp(object()) and not acfun._acq_mlp(type('M', (), {'params': type('P', (), {'config': None})()})())
  assert acfun._blocked_max_n(_stub(100, on)) == acfun.ACQ_FUSED_MAX_N == 128      # the existing helpers do not read the new key


def test_maximize_refuses_an_mlp_model_without_the_opt_in():
  full = dict(cov=kernel.matern52_mlp, mean_func=mean.linear_mlp, hgp=False)
  for cfg in ({}, {'acq_blocked': True}):
    with pytest.raises(nat.HboError) as e:
      acfun.ucb.maximize(model=_stub(100, cfg, **full), sub_dataset_key='t', x_init=np.full(3, 0.5))
    assert e.value.code == nat.HBO_ERR_UNSUPPORTED and 'MLP basis' in str(e.value)
  with pytest.raises(nat.HboError) as e:
    acfun.ucb.maximize(model=_stub(100, {}, mean_func=mean.linear_mlp, hgp=False), sub_dataset_key='t', x_init=np.full(3, 0.5))
  assert e.value.code == nat.HBO_ERR_UNSUPPORTED and 'linear_mlp' in str(e.value)
  # with the key the remaining refusals are today's
  with pytest.raises(nat.HboError) as e:
    acfun.ucb.maximize(model=_stub(100, {'acq_mlp': True}, cov=kernel.matern52_kumar, hgp=False), sub_dataset_key='t', x_init=np.full(3, 0.5))
  assert e.value.code == nat.HBO_ERR_UNSUPPORTED and 'Kumaraswamy' in str(e.value)


def test_the_opt_in_is_documented():
  for f in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
    text = open(os.path.join(ROOT, f)).read()
    assert 'acq_mlp' in text and 'hbo_acq_grad_samples_mlp' in text, f
  for f in ('acq_mlp.md', 'acq_mlp_errors.md'):
    assert os.path.exists(os.path.join(ROOT, 'profiles', f)), f
