"""config['acq_opt_on_device'] (hbo_acq_maximize), the parts that need no device: the control code (csrc/acq_opt_ctl.h) driven through its
host hook hbo_probe_acq_opt_ctl by the oracle's value and gradient, against the NumPy restatement (tests/acq_opt_oracle.py) bit for bit;
the properties of what it returns; SciPy's L-BFGS-B from the same starts; the mutants of the restatement, which the case list must
catch; the eligibility messages; and the untouched SciPy branch of bayesopt()."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.optimize

import acq_opt_oracle as ao

# Largest shortfall of our value below SciPy's on the matched cases, (scipy_value - our_value) / max(1, |value|), measured in the CPU
# run of test_against_scipy on the hook's runs (profiles/acq_opt.md): 4.737e-9, on squared_exponential-constant-ucb-n7-D33-S5-R1, where this optimiser
# stops on FTOL 3.7e-4 away from SciPy's point.  The bound is 10 x that, with the floor of 1e-12 max(1, |value|).
SCIPY_SHORTFALL = 4.737e-9
SCIPY_MATCH_DX = 1e-3


def _nat():
  from hyperbo_amd import _native as nat
  return nat


def run_hook(vg, x0, lo=None, hi=None, dtype=np.float64, max_evals=ao.MAX_EVALS, **kw):
  """The hook driven like the device loop; returns an acq_opt_oracle.Run (margin: NaN)."""
  nat = _nat()
  op = dict(ao.DEFAULTS); op.update(kw)
  o = nat.AcqOptOpts(**op)
  d = x0.size
  state = np.zeros(nat.lib().hbo_acq_opt_state_doubles(d, o.memory))
  point, x_next, x_iter = np.ascontiguousarray(x0, dtype=np.float64).copy(), np.zeros(d), np.zeros(d)
  ev, status = nat.AcqOptEval(), C.c_int32(0)
  log = []
  for n in range(max_evals):
    vals, grads = vg(point)
    vals, grads = np.ascontiguousarray(vals, dtype=np.float64), np.ascontiguousarray(grads, dtype=np.float64)
    rc = nat.lib().hbo_probe_acq_opt_ctl(nat.ptr(state), d, nat.dtype_code(dtype), C.byref(o), nat.ptr(lo), nat.ptr(hi),
                                         nat.ptr(point) if n == 0 else None, nat.ptr(vals), nat.ptr(grads), vals.shape[0], nat.ptr(x_next),
                                         nat.ptr(x_iter), C.byref(ev), C.byref(status))
    assert rc == nat.HBO_OK, (nat.lib().hbo_last_error(None) or b'').decode()
    log.append((ev.kind, ev.iter, ev.alpha, point.copy(), ev.value))
    if status.value != nat.ACQ_OPT_RUNNING:
      break
    point = x_next.copy()
  return ao.Run(log, x_iter.copy(), float(state[5]), status.value, float('nan'))


def same_run(a, b):
  """Two runs agree to the bit: kinds, iteration numbers, steps, points, values, the iterate, the status."""
  assert a.status == b.status and len(a.log) == len(b.log), (a.status, b.status, len(a.log), len(b.log))
  for k, (ea, eb) in enumerate(zip(a.log, b.log)):
    assert ea[:2] == eb[:2], (k, ea[:2], eb[:2])
    assert ea[2] == eb[2] and np.array_equal(ea[3], eb[3]) and np.array_equal(ea[4], eb[4], equal_nan=True), (k, ea, eb)
  assert np.array_equal(a.x, b.x) and np.array_equal(a.f, b.f, equal_nan=True)


def _starts(case):
  """The starts of a case the CPU tier runs: the first and the last."""
  return sorted({0, case.R - 1})


IDS = [c.name for c in ao.CASES]


@functools.lru_cache(maxsize=None)
def hook_run(case, r):
  """Start r of the case through the library's hook (hbo_probe_acq_opt_ctl), driven by the oracle's value and gradient: what the
  tests below judge.  Shared, not to be written to."""
  inp = ao.inputs(case)
  return run_hook(ao.oracle_value_and_grad(case), inp.x0[r], inp.lo, inp.hi)


@pytest.mark.parametrize('case', ao.CASES, ids=IDS)
def test_hook_is_the_restatement_bit_for_bit(case):
  for r in _starts(case):
    same_run(hook_run(case, r), ao.oracle_run(case, r))


@pytest.mark.parametrize('memory', [1, 3])
def test_hook_is_the_restatement_bit_for_bit_with_a_short_ring(memory):
  """memory 1 (every pair overwrites the only slot) and 3 on box-matern32-ei: both starts take more than 8 main steps with a
  component on a face of the box, so the ring wraps many times."""
  case = ao.BY_NAME['box-matern32-ei']
  inp, vg = ao.inputs(case), ao.oracle_value_and_grad(case)
  for r in _starts(case):
    got = run_hook(vg, inp.x0[r], inp.lo, inp.hi, memory=memory)
    assert max(e[1] for e in got.log) >= 8 and np.any((got.x == inp.lo) | (got.x == inp.hi))
    same_run(got, ao.minimise(vg, inp.x0[r], inp.lo, inp.hi, memory=memory))


def test_hook_rounds_fp32_points_and_keeps_its_state_across_copies():
  case = ao.BY_NAME['box-matern32-ei']
  inp = ao.inputs(case)
  vg = ao.oracle_value_and_grad(case)
  x0 = inp.x0[0].astype(np.float32).astype(np.float64)
  got = run_hook(vg, x0, inp.lo, inp.hi, dtype=np.float32)
  want = ao.minimise(vg, x0, inp.lo, inp.hi, dtype=np.float32)
  same_run(got, want)
  assert len(got.log) > 3 and all(np.array_equal(e[3], e[3].astype(np.float32).astype(np.float64)) for e in got.log)
  assert np.array_equal(got.x, got.x.astype(np.float32).astype(np.float64))
  nat = _nat()
  o = nat.AcqOptOpts(**ao.DEFAULTS)
  args = lambda st, x: (nat.ptr(st), 3, nat.F32, C.byref(o), None, None, nat.ptr(x), nat.ptr(np.zeros(1)), nat.ptr(np.zeros(3)), 1,
                        nat.ptr(np.zeros(3)), None, C.byref(nat.AcqOptEval()), C.byref(C.c_int32(0)))
  ns = nat.lib().hbo_acq_opt_state_doubles(3, 10)
  assert ns == 16 + 8 * 3 + 2 * 10 * 3 + 2 * 10
  assert nat.lib().hbo_probe_acq_opt_ctl(*args(np.zeros(ns), np.array([0.1, 0.2, 1.5]))) == nat.HBO_ERR_ARG      # outside the box
  assert nat.lib().hbo_probe_acq_opt_ctl(*args(np.zeros(ns), np.array([0.1, 0.2, 0.3]))) == nat.HBO_ERR_ARG      # not fp32 numbers
  assert nat.lib().hbo_probe_acq_opt_ctl(*args(np.full(ns, 3.0), np.array([0.5, 0.5, 0.5]))) == nat.HBO_ERR_ARG  # not a state
  assert nat.lib().hbo_probe_acq_opt_ctl(*args(np.zeros(ns), np.array([0.5, 0.25, 0.5]))) == nat.HBO_OK
  for bad in (dict(tau=1.0), dict(tau=0.0), dict(tau=float('nan')), dict(c1=0.0), dict(c1=1.0), dict(c1=-1e-4), dict(pgtol=-1.0),
              dict(ftol=float('nan')), dict(memory=0), dict(memory=65), dict(ls_steps=0), dict(max_iters=0)):
    o = nat.AcqOptOpts(**dict(ao.DEFAULTS, **bad))
    assert nat.lib().hbo_probe_acq_opt_ctl(*args(np.zeros(ns), np.array([0.5, 0.25, 0.5]))) == nat.HBO_ERR_ARG, bad


def value_at(case, x):
  vals, _ = ao.oracle_value_and_grad(case)(x)
  return -ao.reduce_samples(vals, np.zeros((vals.size, 1)))[0]


def property_failures(case, r, run):
  """Item 2 of the tier: what a returned point must satisfy, judged with the oracle.  A list of what is broken."""
  inp = ao.inputs(case)
  out = []
  if not (np.all(run.x >= inp.lo) and np.all(run.x <= inp.hi)):
    out.append('the result lies outside the box')
  if any(not (np.all(e[3] >= inp.lo) and np.all(e[3] <= inp.hi)) for e in run.log):
    out.append('a probe lies outside the box')
  if case.kind == 'corner' and not np.all((run.x == 0.0) | (run.x == 1.0)):
    out.append(f'a corner case ends at {run.x}, not in a corner')
  clipped = np.clip(run.x, inp.lo, inp.hi)
  v_end, v_start = value_at(case, clipped), value_at(case, inp.x0[r])
  if not v_end >= v_start:
    out.append(f'the value fell from {v_start} to {v_end}')
  if run.status == ao.CONVERGED:
    vals, grads = ao.oracle_value_and_grad(case)(clipped)
    _, g = ao.reduce_samples(vals, grads)
    if not ao.pg_measure(clipped, g, inp.lo, inp.hi) <= ao.DEFAULTS['pgtol']:
      out.append('CONVERGED, but the projected-gradient measure is above pgtol')
  accepted = [e[4] for e in run.log if e[0] in (ao.START, ao.MAIN)]
  if any(b > a for a, b in zip(accepted, accepted[1:])):
    out.append('the accepted values of f increase somewhere')
  return out


@pytest.mark.parametrize('case', ao.CASES, ids=IDS)
def test_properties_of_the_result(case):
  """The properties of the point the library's control code returns (the hook's run, not the restatement's)."""
  for r in _starts(case):
    assert property_failures(case, r, hook_run(case, r)) == []


def test_cases_clear_their_thresholds():
  """What test_gpu_acq_opt.py relies on when it asks the device for the same sequence of decisions as the oracle-driven restatement: no
  decision of any start of any case lies within a relative 1e-6 of its threshold."""
  close = {(c.name, r): ao.oracle_run(c, r).margin for c in ao.CASES for r in range(c.R)}
  close = {k: m for k, m in close.items() if not m >= 1e-6}
  assert not close, close


@functools.lru_cache(maxsize=None)
def scipy_run(case, r):
  """SciPy's L-BFGS-B on the oracle's f from start r: (x, acquisition value).  Shared, not to be written to."""
  inp = ao.inputs(case)
  vg = ao.oracle_value_and_grad(case)

  def f(x):
    vals, grads = vg(x)
    return ao.reduce_samples(vals, grads)
  res = scipy.optimize.minimize(f, inp.x0[r], jac=True, method='L-BFGS-B', bounds=list(zip(inp.lo, inp.hi)))
  return np.asarray(res.x, dtype=np.float64), -float(res.fun)


def scipy_failures(case, r, run):
  """Item 3 for one start: (matched, what is broken)."""
  xs, vs = scipy_run(case, r)
  if not np.max(np.abs(run.x - xs)) <= SCIPY_MATCH_DX:
    return False, []
  ours = -run.f
  tol = max(10 * SCIPY_SHORTFALL, 1e-12) * max(1.0, abs(vs))
  return True, ([] if ours >= vs - tol else [f'value {ours} below SciPy\'s {vs} by {vs - ours:.3e}'])


def test_against_scipy():
  """The library's control code (the hook's runs) against SciPy's L-BFGS-B from the same starts."""
  unmatched, short = [], 0.0
  for case in ao.CASES:
    matched_all = True
    for r in _starts(case):
      run = hook_run(case, r)
      matched, bad = scipy_failures(case, r, run)
      matched_all = matched_all and matched
      if matched:
        _, vs = scipy_run(case, r)
        short = max(short, (vs - (-run.f)) / max(1.0, abs(vs)))
      assert bad == [], (case.name, r, bad)
    if not matched_all:
      unmatched.append(case.name)
  print(f'\nacq opt vs SciPy: {len(ao.CASES) - len(unmatched)} of {len(ao.CASES)} cases matched; largest shortfall {short:.3e}; unmatched: {unmatched}')
  assert 4 * len(unmatched) <= len(ao.CASES), unmatched
  assert sorted(unmatched) == sorted(ao.UNMATCHED)


MUTANT_CASES = [c for c in ao.CASES if c.kind != 'grid' or c.lo != 0.0] + [c for c in ao.GRID if (c.n, c.d) in ((7, 3), (7, 33), (1, 33))]


@pytest.mark.parametrize('mutant', ao.MUTANTS)
def test_the_case_list_catches_the_mutant(mutant):
  """Every mutant of the restatement trips an assertion of test_properties_of_the_result or test_against_scipy (a property, the value
  bound on a matched start, or a case outside UNMATCHED that no longer ends where SciPy does) on at least one case."""
  caught = []
  for case in MUTANT_CASES:
    for r in _starts(case):
      run = ao.oracle_run(case, r, mutant)
      bad = property_failures(case, r, run)
      if not bad:
        matched, bad = scipy_failures(case, r, run)
        if not matched and case.name not in ao.UNMATCHED:
          bad = ['a matched case no longer ends where SciPy does']
      if bad:
        caught.append((case.name, r, bad[0]))
  print(f'\nacq opt mutant {mutant}: caught on {len(caught)} starts, first: {caught[:1]}')
  assert caught, f'no case catches the mutant {mutant}'


class _Model:
  """As much of a GP as _acq_opt_unmet reads."""

  def __init__(self, n, uses_mlp=False, mean_id=None, uses_kumar=False):
    import types
    self.dataset = {'k': types.SimpleNamespace(x=np.zeros((n, 2)), y=np.zeros((n, 1)))}
    self.cov_func = types.SimpleNamespace(uses_mlp=uses_mlp, uses_kumar=uses_kumar)
    self.mean_func = types.SimpleNamespace(mean_id=mean_id)

  def has_observations(self, key):
    return key in self.dataset and self.dataset[key].x.shape[0] > 0


def test_unmet_messages_each_condition_in_turn():
  from hyperbo_amd.bo_utils import acfun
  nat = _nat()
  sub = acfun.ucb_sub
  assert acfun._acq_opt_unmet(_Model(5), 'k', sub) is None
  assert acfun._acq_opt_unmet(_Model(128), 'k', acfun.expected_improvement_sub, 4, 4) is None
  assert 'not one of the native ones' in acfun._acq_opt_unmet(_Model(5), 'k', lambda mu, std, p: mu)
  assert 'no observations' in acfun._acq_opt_unmet(_Model(0), 'k', sub)
  assert 'no observations' in acfun._acq_opt_unmet(_Model(5), 'other', sub)
  assert '129 > 128' in acfun._acq_opt_unmet(_Model(129), 'k', sub)
  assert 'MLP basis' in acfun._acq_opt_unmet(_Model(5, uses_mlp=True), 'k', sub)
  assert 'linear_mlp' in acfun._acq_opt_unmet(_Model(5, mean_id=nat.MEAN_LINEAR_MLP), 'k', sub)
  assert 'Kumaraswamy' in acfun._acq_opt_unmet(_Model(5, uses_kumar=True), 'k', sub)
  assert 'only 3 of the 4' in acfun._acq_opt_unmet(_Model(5), 'k', sub, 4, 3)
  # the context option 'acq_fused' plays no part, and maximize refuses instead of falling back
  with pytest.raises(nat.HboError) as e:
    acfun.ucb.maximize(model=_Model(129), sub_dataset_key='k', x_init=np.zeros(2))
  assert e.value.code == nat.HBO_ERR_UNSUPPORTED and '129 > 128' in str(e.value)


def test_bindings_and_constants():
  nat = _nat()
  for name in ('hbo_acq_maximize', 'hbo_acq_opt_state_doubles', 'hbo_probe_acq_opt_ctl'):
    assert name in nat.SIGNATURES and getattr(nat.lib(), name)
  assert C.sizeof(nat.AcqOptOpts) == 48 and C.sizeof(nat.AcqOptEval) == 24 == nat.ACQ_OPT_EVAL_DTYPE.itemsize
  assert (nat.ACQ_OPT_START, nat.ACQ_OPT_MAIN, nat.ACQ_OPT_LINE_SEARCH, nat.ACQ_OPT_IDLE) == (ao.START, ao.MAIN, ao.LINE_SEARCH, ao.IDLE)
  assert (nat.ACQ_OPT_RUNNING, nat.ACQ_OPT_CONVERGED, nat.ACQ_OPT_FTOL, nat.ACQ_OPT_NO_PROGRESS, nat.ACQ_OPT_NONFINITE_AT_START,
          nat.ACQ_OPT_STEPS_DONE) == (ao.RUNNING, ao.CONVERGED, ao.FTOL, ao.NO_PROGRESS, ao.NONFINITE_AT_START, ao.STEPS_DONE)
  from hyperbo_amd.bo_utils import acfun
  assert {k: acfun.ACQ_OPT_DEFAULTS[k] for k in ao.DEFAULTS} == ao.DEFAULTS
  assert nat.lib().hbo_acq_opt_state_doubles(0, 10) == 0 and nat.lib().hbo_acq_opt_state_doubles(3, 0) == 0


def test_nonfinite_at_the_start_and_an_exhausted_line_search():
  nan = lambda x: (np.array([np.nan, 1.0]), np.zeros((2, x.size)))
  run = run_hook(nan, np.array([0.5, 0.0, 1.0]))
  assert run.status == ao.NONFINITE_AT_START and len(run.log) == 1 and np.array_equal(run.x, [0.5, 0.0, 1.0])
  same_run(run, ao.minimise(nan, np.array([0.5, 0.0, 1.0])))
  # finite at the start only: every probe is rejected, ls_steps of them, and the iterate stays
  x0 = np.array([0.5, 0.5])
  cliff = lambda x: (np.array([1.0]), np.array([[1.0, -2.0]])) if np.array_equal(x, x0) else (np.array([np.nan]), np.full((1, 2), np.nan))
  run = run_hook(cliff, x0, ls_steps=7)
  assert run.status == ao.NO_PROGRESS and [e[0] for e in run.log] == [ao.START] + [ao.LINE_SEARCH] * 7 and np.array_equal(run.x, x0)
  assert [e[2] for e in run.log[1:]] == [2.0**-k / np.sqrt(5.0) for k in range(7)]
  same_run(run, ao.minimise(cliff, x0, ls_steps=7))


def test_bayesopt_with_the_key_off_calls_scipy_as_before(monkeypatch):
  """The spy needs no device: the model's acquisition function is a stand-in."""
  import types
  from hyperbo_amd.bo_utils import bayesopt
  calls = []

  def spy(fun, x0, **kw):
    calls.append((np.array(x0), kw))
    return types.SimpleNamespace(x=np.asarray(x0) * 0.5)
  monkeypatch.setattr(scipy.optimize, 'minimize', spy)

  class Model:
    input_dim = 2
    params = types.SimpleNamespace(config={})
    dataset = {}
    appended = []

    def has_observations(self, key):
      return True

    def update_sub_dataset(self, point, sub_dataset_key, is_append):
      self.appended.append(point[0])

  def ac(*, model, sub_dataset_key, x_queries):
    return np.asarray(x_queries)[:, :1]
  ac.maximize = lambda **kw: pytest.fail('maximize must not be called with the key off')
  for cfg in ({}, {'acq_opt_on_device': False}, {'acq_opt_on_device': 0, 'acq_opt_starts': 4}):
    calls.clear()
    m = Model(); m.params = types.SimpleNamespace(config=cfg); m.appended = []
    cand = np.array([[0.2, 0.9], [0.8, 0.1], [0.5, 0.5]])
    bayesopt.bayesopt(3, m, 'k', lambda x: np.zeros((1, 1)), ac, iters=2, input_sampler=lambda key, dim: cand)
    assert len(calls) == 2
    for x0, kw in calls:
      assert np.array_equal(x0, cand[1]) and kw['jac'] is True and kw['method'] == 'L-BFGS-B' and kw['bounds'] == [(0.0, 1.0)] * 2
      assert set(kw) == {'jac', 'method', 'bounds'}
    assert all(np.array_equal(p, cand[1] * 0.5) for p in m.appended)
  # with the key on the same stand-in goes to maximize, from the k best candidates in order
  seen = []
  ac.maximize = lambda **kw: (seen.append(kw['x_init']), (kw['x_init'][0], 0.0, {}))[1]
  calls.clear()
  m = Model(); m.params = types.SimpleNamespace(config={'acq_opt_on_device': True, 'acq_opt_starts': 2}); m.appended = []
  cand = np.array([[0.5, 0.9], [0.8, 0.1], [0.8, 0.5]])
  bayesopt.bayesopt(3, m, 'k', lambda x: np.zeros((1, 1)), ac, iters=1, input_sampler=lambda key, dim: cand)
  assert calls == [] and len(seen) == 1 and np.array_equal(seen[0], cand[[1, 2]])
