"""CPU tier of the device BO loop (hbo_bo_simulated, config['bo_on_device']): the recurrence csrc/bo_loop.hip runs, restated in NumPy,
against the reference's loop on the oracle for every case of bo_device_cases.py (same sequence, mu / var to 1e-12), the gap
condition of the cases whose sequence the GPU test compares exactly, the export and its argument checks, the routing helper, the
acquisition table, the two scale values and the untouched default path."""
import ctypes as C

import numpy as np
import pytest

import bo_device_cases as cases
import bo_loop_oracle as blo
import family_check_cases as family
import helpers
from hyperbo_amd import _native as nat
from hyperbo_amd.basics import definitions as defs
from hyperbo_amd.bo_utils import acfun, bayesopt, const
from hyperbo_amd.gp_utils import gp, kernel, mean, utils


@pytest.fixture(scope='module')
def oracle_runs():
  return {}


def _oracle(store, case):
  if case.name not in store:
    w = blo.case_world(case)
    store[case.name] = (w, blo.oracle_loop(w))
  return store[case.name]


@pytest.mark.parametrize('case', cases.ALL, ids=lambda c: c.name)
def test_row_recurrence_is_the_reference_loop(case, oracle_runs):
  w, ref = _oracle(oracle_runs, case)
  rec = blo.recurrence_loop(w)
  gap = blo.min_gap(ref)
  print(f'{case.name}: min gap {gap:.3e}, distinct selections {len(set(ref.sel.tolist()))} of {case.iters}')
  if case.exact:
    # the gap condition: no iteration of a case whose sequence is compared exactly is decided by rounding
    assert gap >= cases.GAP, (case.name, gap)
  assert np.isnan(ref.acq).any() == (case.nan_at is not None)
  assert rec.sel.tolist() == ref.sel.tolist()     # every case: the same sequence (the twins of the duplicate case tie exactly in both)
  fin = np.isfinite(ref.mu)
  assert np.array_equal(fin, np.isfinite(rec.mu))
  assert np.max(np.abs(rec.mu - ref.mu)[fin], initial=0.0) <= 1e-12
  assert np.max(np.abs(rec.var - ref.var)[fin], initial=0.0) <= 1e-12
  ok = np.isfinite(ref.acq)
  assert np.array_equal(ok, np.isfinite(rec.acq))
  np.testing.assert_allclose(rec.acq[ok], ref.acq[ok], rtol=1e-8, atol=1e-10)


def test_cases_cover_what_they_are_meant_to(oracle_runs):
  _, m257 = _oracle(oracle_runs, cases.BY_NAME['M257'])
  assert (m257.sel >= 256).any()                      # the winner sits in the partial last workgroup at least once
  _, tie = _oracle(oracle_runs, cases.BY_NAME['tie_prior'])
  assert tie.sel[0] == 0 and np.all(tie.vals[0] == tie.vals[0][0])   # the prior under UCB ties everywhere: index 0
  wdup, dup = _oracle(oracle_runs, cases.BY_NAME['tie_dup'])
  lo, hi = wdup.twins                                  # identical rows in different workgroups of 256 columns
  assert lo // 256 != hi // 256 and np.array_equal(wdup.pool_x[lo], wdup.pool_x[hi]) and wdup.pool_y[lo] == wdup.pool_y[hi]
  assert lo in dup.sel[1:].tolist() and hi not in dup.sel.tolist()   # the lower twin IS selected after rows were appended, the higher never
  assert all(vals[lo] == vals[hi] for vals in dup.vals)             # ... and every one of those selections was an exact tie
  _, nan = _oracle(oracle_runs, cases.BY_NAME['nan_y'])
  first = int(np.argmax(np.isnan(nan.acq)))
  assert np.isnan(nan.acq[first:]).all() and (nan.sel[first:] == 0).all() and first >= 1   # np.argmax over all-NaN: index 0
  assert any(len(set(_oracle(oracle_runs, c)[1].sel.tolist())) < c.iters for c in cases.PARITY)   # re-selected candidates are common


# ---- the C entry point -----------------------------------------------------------------------------------------------------
def test_entry_point_is_exported_and_bound():
  assert 'hbo_bo_simulated' in nat.SIGNATURES
  f = nat.lib().hbo_bo_simulated
  res, args = nat.SIGNATURES['hbo_bo_simulated']
  assert f.restype is res and list(f.argtypes) == args and len(args) == 10
  assert C.sizeof(nat.BoRun) == 6 * 8 + 2 * 4 + 4 * 8
  assert (nat.BO_PARAM_CONST, nat.BO_PARAM_MAX_PLUS, nat.BO_PARAM_MAX_PLUS_STD) == (0, 1, 2)


def bo_args(R=1, iters=3, M=4, D=2, n0=0):
  models = (nat.Model * max(R, 1))()
  ls = np.ones(D)
  for m in models:
    m.kernel_id, m.mean_id, m.dtype, m.input_dim, m.n_lengthscale = nat.KERNEL_SE, nat.MEAN_CONSTANT, nat.F64, D, D
    m.lengthscale, m.signal_variance, m.noise_variance, m.eps = nat.ptr(ls).value, 1.0, 0.1, 1e-6
  xc, yc, x0, y0 = np.zeros((max(M, 1), D)), np.zeros(max(M, 1)), np.zeros((max(n0, 1), D)), np.zeros(max(n0, 1))
  runs = (nat.BoRun * max(R, 1))()
  for r in runs:
    r.xc, r.yc, r.M, r.x0, r.y0, r.n0 = nat.ptr(xc).value, nat.ptr(yc).value, M, nat.ptr(x0).value, nat.ptr(y0).value, n0
    r.acq_id, r.param_mode, r.param, r.add_noise, r.scale0, r.scale = nat.ACQ_EI, nat.BO_PARAM_MAX_PLUS, 0.0, 0.1, 1.0, 1.0
  sel = np.full((max(R, 1), max(iters, 1)), 7, dtype=np.int32)
  acq = np.full((max(R, 1), max(iters, 1)), 7.0)
  status = np.full(max(R, 1), 7, dtype=np.int32)
  return dict(models=models, runs=runs, R=R, iters=iters, sel=sel.ctypes.data_as(C.POINTER(C.c_int32)),
              acq=acq.ctypes.data_as(C.POINTER(C.c_double)), mu=None, var=None, status=status.ctypes.data_as(C.POINTER(C.c_int32)),
              _keep=(ls, xc, yc, x0, y0, sel, acq, status))


def bo_call(a, ctx=None):
  return nat.lib().hbo_bo_simulated(ctx, a['models'], a['runs'], a['R'], a['iters'], a['sel'], a['acq'], a['mu'], a['var'], a['status'])


def check_refusals(ctx, err):
  """The refusals that need no device (the GPU tier runs them again with a context, where they must come before any device work)."""
  for name in ('models', 'runs', 'sel', 'acq', 'status'):
    a = bo_args()
    a[name] = None
    assert bo_call(a, ctx) == nat.HBO_ERR_ARG and 'null argument' in err(), (name, err())
  for R in (0, -1, 4097):
    assert bo_call(bo_args(R=R), ctx) == nat.HBO_ERR_ARG and '1 <= R <= 4096' in err(), (R, err())
  for iters in (0, -2, 65537):
    assert bo_call(bo_args(iters=iters), ctx) == nat.HBO_ERR_ARG and '1 <= iters <= 65536' in err(), (iters, err())
  assert bo_call(bo_args(M=0), ctx) == nat.HBO_ERR_ARG and 'empty candidate pool' in err()
  a = bo_args(n0=2)
  a['runs'][0].y0 = None
  assert bo_call(a, ctx) == nat.HBO_ERR_ARG and 'pool or observations are null' in err()
  a = bo_args()
  a['runs'][0].acq_id = 3
  assert bo_call(a, ctx) == nat.HBO_ERR_ARG and 'bad acq_id' in err()
  a = bo_args()
  a['runs'][0].param_mode = 3
  assert bo_call(a, ctx) == nat.HBO_ERR_ARG and 'bad param_mode' in err()
  a = bo_args(R=2)
  a['models'][1].kernel_id = nat.KERNEL_MATERN32
  assert bo_call(a, ctx) == nat.HBO_ERR_ARG and 'must share' in err()
  a = bo_args(R=2)
  a['models'][1].input_warp = nat.WARP_KUMAR
  assert bo_call(a, ctx) == nat.HBO_ERR_UNSUPPORTED and 'Kumaraswamy' in err()
  sel, acq, status = a['_keep'][5:]
  assert np.all(sel == 7) and np.all(acq == 7.0) and np.all(status == 7)   # no output was touched


def test_argument_errors_come_before_any_device_call():
  err = lambda: (nat.lib().hbo_last_error(None) or b'').decode()
  check_refusals(None, err)
  assert bo_call(bo_args()) == nat.HBO_ERR_ARG and 'ctx is null' in err()


@pytest.mark.parametrize('name', list(family.CASES))
def test_mixed_batches_are_refused_in_the_shared_order(name):
  """A pair of models the batched entry points' shared check refuses (family_check_cases.py), before the context is asked for."""
  err = lambda: (nat.lib().hbo_last_error(None) or b'').decode()
  a = bo_args(R=2)
  a['models'], keep, code, word = family.pair(name)
  assert bo_call(a) == code and word.format(fn='hbo_bo_simulated') in err(), (name, err())
  sel, acq, status = a['_keep'][5:]
  assert np.all(sel == 7) and np.all(acq == 7.0) and np.all(status == 7)   # no output was touched
  del keep


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def _stub(n=6, d=3, cov=kernel.matern52, mean_func=mean.constant, hgp=False, config=None, m_cols=1):
  ds = {'t': defs.SubDataset(np.zeros((n, d)), np.zeros((n, m_cols))), 'other': defs.SubDataset(np.zeros((4, d)), np.zeros((4, 1)))}
  params = defs.GPParams(model=helpers.make_model(np.random.default_rng(0), 'constant', False, d), config=dict(config or {}))
  return (gp.HGP if hgp else gp.GP)(ds, mean_func, cov, params, utils.DEFAULT_WARP_FUNC)


def _pool(M=5, d=3, m_cols=1):
  return defs.SubDataset(np.zeros((M, d)), np.zeros((M, m_cols)))


def test_routing_helper_names_the_first_unmet_condition():
  unmet = bayesopt._bo_on_device_unmet
  assert unmet(_stub(), 't', _pool(), acfun.ei) is None
  assert unmet(_stub(), 'missing', _pool(), acfun.ucb3) is None            # the prior branch is covered
  assert unmet(_stub(cov=kernel.matern52_mlp, mean_func=mean.linear_mlp), 't', _pool(), acfun.pi2) is None
  assert 'HGP' in unmet(_stub(hgp=True), 't', _pool(), acfun.ei)
  assert 'retrain' in unmet(_stub(config={'retrain': 3}), 't', _pool(), acfun.ei)
  assert unmet(_stub(config={'retrain': 0}), 't', _pool(), acfun.ei) is None
  assert 'random search' in unmet(_stub(), 't', _pool(), acfun.rand)
  assert 'not one of the native' in unmet(_stub(), 't', _pool(), lambda **kw: None)
  assert 'Kumaraswamy' in unmet(_stub(cov=kernel.matern52_kumar), 't', _pool(), acfun.ei)
  assert 'more than one column' in unmet(_stub(), 't', _pool(m_cols=2), acfun.ei)
  assert 'more than one column' in unmet(_stub(m_cols=2), 't', _pool(), acfun.ei)
  assert 'pool is empty' in unmet(_stub(), 't', _pool(M=0), acfun.ei)
  # the order of the issue: model class, retrain, acquisition, kernel, data
  assert 'HGP' in unmet(_stub(hgp=True, config={'retrain': 3}), 't', _pool(M=0), acfun.rand)
  assert 'retrain' in unmet(_stub(config={'retrain': 3}, cov=kernel.matern52_kumar), 't', _pool(M=0), acfun.rand)
  assert 'random search' in unmet(_stub(cov=kernel.matern52_kumar), 't', _pool(M=0), acfun.rand)
  assert 'Kumaraswamy' in unmet(_stub(cov=kernel.matern52_kumar), 't', _pool(M=0), acfun.ei)


def test_flag_with_an_unmet_condition_raises_without_touching_the_library(monkeypatch):
  monkeypatch.setattr(nat, 'lib', lambda: pytest.fail('the library was touched'))
  for model, pool, fn, word in ((_stub(hgp=True, config={'bo_on_device': 1}), _pool(), acfun.ei, 'HGP'),
                                (_stub(config={'bo_on_device': True, 'retrain': 2}), _pool(), acfun.ei, 'retrain'),
                                (_stub(config={'bo_on_device': True}), _pool(), acfun.rand, 'random search'),
                                (_stub(config={'bo_on_device': True}), _pool(), lambda **kw: None, 'not one of the native'),
                                (_stub(cov=kernel.matern52_kumar, config={'bo_on_device': True}), _pool(), acfun.ei, 'Kumaraswamy'),
                                (_stub(config={'bo_on_device': True}), _pool(m_cols=2), acfun.ei, 'more than one column'),
                                (_stub(config={'bo_on_device': True}), _pool(M=0), acfun.ucb, 'pool is empty')):
    with pytest.raises(ValueError, match='bo_on_device: .*' + word):
      bayesopt.simulated_bayesopt(model, 't', pool, fn, 3)


def test_batch_of_two_families_raises_before_a_context_exists(monkeypatch):
  monkeypatch.setattr(nat, 'default_context', lambda: pytest.fail('a context was asked for'))
  a, b = _stub(), _stub(cov=kernel.matern32)
  with pytest.raises(ValueError, match='bo_on_device: .*must share'):
    bayesopt.simulated_bayesopt_batch([(a, 't', _pool(), acfun.ei), (b, 't', _pool(), acfun.ei)], 3)


def test_acquisition_table_covers_the_registry():
  table = acfun._BO_DEVICE
  for name, fn in const.ACFUN.items():
    if fn is acfun.rand:
      continue
    assert fn in table, name
  cb_model = _stub(n=0)
  cb_model.dataset['t'] = defs.SubDataset(np.zeros((4, 3)), np.array([[0.3], [-1.0], [2.5], [0.7]]))
  y = cb_model.dataset['t'].y
  for fn, (acq_id, mode, param) in table.items():
    assert acq_id == acfun._NATIVE_ID[_sub_of(fn)]
    want = _default_callback(fn)(cb_model, 't')
    got = {nat.BO_PARAM_CONST: param, nat.BO_PARAM_MAX_PLUS: np.max(y) + param, nat.BO_PARAM_MAX_PLUS_STD: np.max(y) + param * np.std(y)}[mode]
    assert got == pytest.approx(want, rel=1e-15), fn
    empty = _default_callback(fn)(cb_model, 'missing')
    assert empty == (param if mode == nat.BO_PARAM_CONST else 0.0)


def _closure(fn):
  return dict(zip(fn.__code__.co_freevars, (c.cell_contents for c in fn.__closure__)))


def _sub_of(fn):
  return _closure(fn)['acfun_sub']


def _default_callback(fn):
  return fn.__kwdefaults__['acfun_callback']


def test_scale0_and_scale_for_an_absent_key():
  m = _stub()
  noise, s0, s1 = bayesopt._bo_scales(m, 't')
  assert (s0, s1) == (2.0, 2.0) and noise == m.predict_noise_and_scale(True, True)[0]
  _, s0, s1 = bayesopt._bo_scales(m, 'missing')          # the first append creates the third sub-dataset
  assert (s0, s1) == (2.0, 1.5)
  del m.dataset['other']
  _, s0, s1 = bayesopt._bo_scales(m, 'missing')
  assert (s0, s1) == (1.0, 2.0)
  # ... which is what the host loop's predict sees after its first append
  m.update_sub_dataset((np.zeros(3), np.zeros(1)), 'missing', is_append=True)
  assert m.predict_noise_and_scale(True, True)[1] == s1


def test_default_path_never_calls_the_device_loop(monkeypatch):
  calls, touched, real = [], [], nat.lib()

  class Lib:   # the library with a counter on the entry point
    def __getattr__(self, name):
      if name == 'hbo_bo_simulated':
        touched.append(name)
      return getattr(real, name)
  monkeypatch.setattr(nat, 'lib', Lib)
  monkeypatch.setattr(bayesopt, 'simulated_bayesopt_batch', lambda *a, **k: calls.append(a) or [None])
  picked = []

  def fake_acq(*, model, sub_dataset_key, x_queries):
    picked.append(x_queries.shape[0])
    return np.arange(x_queries.shape[0], dtype=np.float64)[:, None]
  fake_acq.__name__ = 'fake'
  for config in ({}, {'bo_on_device': False}, {'bo_on_device': 0}):
    m = _stub(config=config)
    out = bayesopt.simulated_bayesopt(m, 't', _pool(), fake_acq, 2)
    assert out.x.shape[0] == 8
  assert not calls and not touched and picked == [5] * 6
  bayesopt.simulated_bayesopt(_stub(config={'bo_on_device': True}), 't', _pool(), fake_acq, 2)
  assert len(calls) == 1
