"""The simulated BO loop on the device (run with `-m gpu` on an MI355X): hbo_bo_simulated (csrc/bo_loop.hip) and the routing of
bo_utils/bayesopt.py behind config['bo_on_device'].

Reference: the reference's loop on the oracle (bo_loop_oracle.oracle_loop: o.predict from scratch every iteration).  fp64 bounds are
the oracle bounds of test_gpu_acq_fused.py: values rtol 1e-8 / atol 1e-10.  Cases whose sequence is compared exactly meet the gap
condition of test_bo_device_host.py (best and second-best oracle value at least 1e-6 apart in every iteration).

Replay check (every case, fp64 and fp32): the oracle is driven along the device's own selections; at every iteration the oracle value
of the device's choice must be within the bound of the oracle's maximum (an iteration whose oracle values hold a NaN: the device's
choice is np.argmax's, the first NaN).  fp64: max - value <= 1e-10 + 1e-8 |max|.  fp32: max - value <= FP32_REPLAY_BOUND (1 + |max|),
the oracle being run in fp64 on the fp32-rounded inputs.

FP32_REPLAY_BOUND.  Measured on an MI355X over all cases of bo_device_cases.py (test_replay_along_the_device_selections prints the
figures of every case before it asserts; profiles/bo_device.md has the command and the table): the worst (max - value) / (1 + |max|) is
FP32_REPLAY_MEASURED = 0.0 -- in every iteration of every case the fp32 device loop chose the fp64 oracle's maximum.  Ten times that
leaves no room for a single rounding, so the bound is max(10 x measured, 2^-24), one fp32 rounding of the scale 1 + |max|.  This is a
DELIBERATE EXCEPTION to the 10 x measured convention, and looser than it: the values are rounded to fp32 before the arg-max, so two
candidates one fp32 rounding apart are a tie the device may break either way, which a bound of 0 would forbid.

FP32_VALUE_BOUND.  Along the same selections the fp32 run's acq_out, mu_out and var_out against the oracle's, |device - oracle| /
(1 + |oracle|): the worst measured is FP32_VALUE_MEASURED = 3.761e-07 (mu_out of the case linear_mlp; dot_product-ei 3.691e-07 next;
acq_out worst 3.119e-07 at dot_product-pi, var_out worst 2.043e-07 at dot_product-pi2).  The bound is 10 x that.  fp64 holds the same figures to RTOL
(worst measured 9.3e-15)."""
import ctypes as C
import types

import numpy as np
import pytest

import bo_device_cases as cases
import bo_loop_oracle as blo
import test_bo_device_host as host
from oracle import hyperbo_oracle as o

pytestmark = pytest.mark.gpu
KEY = cases.KEY
RTOL, ATOL = 1e-8, 1e-10
FP32_REPLAY_MEASURED = 0.0
FP32_REPLAY_BOUND = max(10 * FP32_REPLAY_MEASURED, 2.0**-24)
FP32_VALUE_MEASURED = 3.761e-07
FP32_VALUE_BOUND = 10 * FP32_VALUE_MEASURED


def _nv():
  from hyperbo_amd import _model as hmodel
  from hyperbo_amd import _native as nat
  from hyperbo_amd.basics import definitions as defs
  from hyperbo_amd.bo_utils import acfun, bayesopt
  from hyperbo_amd.gp_utils import gp, kernel, mean, utils
  return types.SimpleNamespace(hmodel=hmodel, nat=nat, defs=defs, acfun=acfun, bayesopt=bayesopt, gp=gp, kernel=kernel, mean=mean, utils=utils)


def native_funcs(case):
  nv = _nv()
  return getattr(nv.mean, case.mean), getattr(nv.kernel, case.kernel + ('_mlp' if case.mlp_kernel else ''))


def native_model(w, config=None):
  """A gp.GP over the world's dataset (cases.oracle_dataset on the native side)."""
  nv = _nv()
  mean_func, cov_func = native_funcs(w.case)
  ds = {0: nv.defs.SubDataset(w.other_x, w.other_y)}
  if not w.case.key_absent:
    ds[KEY] = nv.defs.SubDataset(w.x0, w.y0)
  params = nv.defs.GPParams(model=cases._cast(w.model, w.dtype), config=dict(config or {}))
  return nv.gp.GP(ds, mean_func, cov_func, params, nv.utils.DEFAULT_WARP_FUNC)


Result = types.SimpleNamespace


def device_call(ctx, worlds, iters):
  """One hbo_bo_simulated call over the worlds (one family): per run sel, acq, status, mu, var."""
  nv = _nv()
  nat = nv.nat
  built, structs, keep = [], [], []
  for w in worlds:
    case = w.case
    mean_func, cov_func = native_funcs(case)
    pn = nv.defs.GPParams(model=cases._cast(w.model, w.dtype), config={})
    bm = nv.hmodel.BuiltModel(mean_func, cov_func, pn, nv.utils.DEFAULT_WARP_FUNC, w.dtype, case.D)
    noise = float(np.squeeze(o.retrieve_params(cases.oracle_params(w), ['noise_variance'], cases.WFO)[0]))
    xc, yc = np.ascontiguousarray(w.pool_x, dtype=w.dtype), np.ascontiguousarray(w.pool_y.reshape(-1), dtype=w.dtype)
    x0, y0 = np.ascontiguousarray(w.x0, dtype=w.dtype), np.ascontiguousarray(w.y0.reshape(-1), dtype=w.dtype)
    fn = getattr(nv.acfun, cases.ACQS[case.acq][2])
    acq_id, mode, param = nv.acfun._BO_DEVICE[fn]
    scale0, scale = (1.0, 2.0) if case.key_absent else (2.0, 2.0)   # one other sub-dataset; the first append creates the second
    structs.append(nat.BoRun(nat.ptr(xc), nat.ptr(yc), case.M, nat.ptr(x0) if case.n0 else None, nat.ptr(y0) if case.n0 else None,
                             case.n0, acq_id, mode, param, noise, scale0, scale))
    built.append(bm); keep.append((xc, yc, x0, y0))
  R = len(worlds)
  sel = np.full((R, iters), -7, dtype=np.int32)
  acq = np.full((R, iters), -7.0)
  status = np.full(R, -7, dtype=np.int32)
  total = sum(w.case.M for w in worlds)
  mu, var = np.full(total, -7.0, dtype=worlds[0].dtype), np.full(total, -7.0, dtype=worlds[0].dtype)
  rc = nat.lib().hbo_bo_simulated(ctx.handle, (nat.Model * R)(*[b.struct for b in built]), (nat.BoRun * R)(*structs), R, iters,
                                  sel.ctypes.data_as(C.POINTER(C.c_int32)), acq.ctypes.data_as(C.POINTER(C.c_double)), nat.ptr(mu),
                                  nat.ptr(var), status.ctypes.data_as(C.POINTER(C.c_int32)))
  ctx.check(rc)
  out, m0 = [], 0
  for r, w in enumerate(worlds):
    out.append(Result(sel=sel[r].copy(), acq=acq[r].copy(), status=int(status[r]), mu=mu[m0:m0 + w.case.M].copy(),
                      var=var[m0:m0 + w.case.M].copy(), rc=rc))
    m0 += w.case.M
  return out


@pytest.fixture(scope='module')
def store():
  return {}


def _world(store, case, dtype):
  k = ('world', case.name, np.dtype(dtype).name)
  if k not in store:
    store[k] = blo.case_world(case, dtype)
  return store[k]


def _reference(store, case):
  """The oracle loop of the fp64 world, computed once per module."""
  k = ('ref', case.name)
  if k not in store:
    store[k] = blo.oracle_loop(_world(store, case, np.float64))
  return store[k]


def _device(store, gpu_ctx, case, dtype):
  k = ('dev', case.name, np.dtype(dtype).name)
  if k not in store:
    store[k] = device_call(gpu_ctx, [_world(store, case, dtype)], case.iters)[0]
  return store[k]


def replay_error(w, sel, ref=None):
  """(worst (max - value) / (1 + |max|), worst (max - value) - (ATOL + RTOL |max|), the loop) of the oracle driven along `sel`; asserts
  np.argmax's choice where the oracle values hold a NaN.  ref: an oracle loop that is known to have taken the same selections."""
  loop = ref if ref is not None and ref.sel.tolist() == list(sel) else blo.oracle_loop(w, selections=sel)
  worst32, worst64 = 0.0, -np.inf
  for i, vals in enumerate(loop.vals):
    if np.isnan(vals).any():
      assert int(sel[i]) == int(np.argmax(vals)), (w.case.name, i, int(sel[i]), int(np.argmax(vals)))
      continue
    vmax, v = float(np.max(vals)), float(vals[int(sel[i])])
    worst32 = max(worst32, (vmax - v) / (1.0 + abs(vmax)))
    worst64 = max(worst64, (vmax - v) - (ATOL + RTOL * abs(vmax)))
  return worst32, worst64, loop


EXACT = [c for c in cases.ALL if c.exact]


@pytest.mark.parametrize('case', EXACT, ids=lambda c: c.name)
def test_parity_with_the_oracle_loop(case, store, gpu_ctx):
  ref = _reference(store, case)
  dev = _device(store, gpu_ctx, case, np.float64)
  assert dev.status == 0 and dev.rc == 0
  assert dev.sel.tolist() == ref.sel.tolist()
  print(f'{case.name}: acq err {np.max(np.abs(dev.acq - ref.acq)):.3e} mu err {np.max(np.abs(dev.mu - ref.mu)):.3e} '
        f'var err {np.max(np.abs(dev.var - ref.var)):.3e}')
  np.testing.assert_allclose(dev.acq, ref.acq, rtol=RTOL, atol=ATOL)
  np.testing.assert_allclose(dev.mu, ref.mu, rtol=RTOL, atol=ATOL)
  np.testing.assert_allclose(dev.var, ref.var, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('case', cases.ALL, ids=lambda c: c.name)
def test_replay_along_the_device_selections(case, dtype, store, gpu_ctx):
  w = _world(store, case, dtype)
  dev = _device(store, gpu_ctx, case, dtype)
  assert dev.status == 0
  assert np.all((dev.sel >= 0) & (dev.sel < case.M))
  worst32, worst64, loop = replay_error(w, dev.sel, _reference(store, case) if dtype == np.float64 else None)
  # the values along the same selections: |device - oracle| / (1 + |oracle|) where the oracle is finite
  rel = lambda got, want: float(np.max((np.abs(got - want) / (1.0 + np.abs(want)))[np.isfinite(want)], initial=0.0))
  errs = rel(dev.acq, loop.acq), rel(dev.mu.astype(np.float64), loop.mu), rel(dev.var.astype(np.float64), loop.var)
  print(f'{case.name} {np.dtype(dtype).name}: replay (max - value) / (1 + |max|) = {worst32:.3e}; value errors acq {errs[0]:.3e} '
        f'mu {errs[1]:.3e} var {errs[2]:.3e}')
  if dtype == np.float64:
    assert worst64 <= 0.0, worst64
    for got, want in ((dev.acq, loop.acq), (dev.mu, loop.mu), (dev.var, loop.var)):
      ok = np.isfinite(want)
      np.testing.assert_allclose(got[ok], want[ok], rtol=RTOL, atol=ATOL)
  else:
    assert worst32 <= FP32_REPLAY_BOUND, (worst32, FP32_REPLAY_BOUND)
    assert max(errs) <= FP32_VALUE_BOUND, (errs, FP32_VALUE_BOUND)


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_exact_ties_take_the_first_index(dtype, store, gpu_ctx):
  prior = _device(store, gpu_ctx, cases.BY_NAME['tie_prior'], dtype)
  assert prior.sel[0] == 0                       # a stationary kernel, a constant mean, UCB, no observations: every value is equal
  # two identical rows in different workgroups, the pair the loop converges on: every tie between them goes to the lower index, through
  # the workgroup partials and the reduction of bo_select_kernel, after rows have been appended
  case = cases.BY_NAME['tie_dup']
  lo, hi = _world(store, case, dtype).twins
  assert lo // 256 != hi // 256
  dup = _device(store, gpu_ctx, case, dtype)
  assert lo in dup.sel[1:].tolist() and hi not in dup.sel.tolist()
  assert dup.sel.tolist() == _reference(store, case).sel.tolist()   # (gap 0.098 apart from the twins' tie: not decided by rounding)


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_nan_value_is_np_argmax_over_nan(dtype, store, gpu_ctx):
  case = cases.BY_NAME['nan_y']
  w = _world(store, case, dtype)
  dev = _device(store, gpu_ctx, case, dtype)
  taken = np.isnan(np.asarray(w.pool_y).reshape(-1)[dev.sel])
  assert taken.any()
  first = int(np.argmax(taken))
  assert not np.isnan(dev.acq[:first + 1]).any()
  assert np.isnan(dev.acq[first + 1:]).all() and (dev.sel[first + 1:] == 0).all()
  assert np.isnan(dev.mu).all() and dev.status == 0   # a NaN value is not an indefinite matrix


def _ind_cases():
  mk = cases._case
  return [mk('ind_a', acq='ei', M=300, n0=5, iters=10, seed=71), mk('ind_b', acq='pi2', M=130, n0=0, iters=10, seed=72, key_absent=True),
          mk('ind_c', acq='ucb3', M=64, n0=3, iters=10, seed=73)]


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_runs_do_not_depend_on_what_shares_the_call(dtype, gpu_ctx):
  worlds = [cases.world(c, dtype) for c in _ind_cases()]
  together = device_call(gpu_ctx, worlds, 10)
  again = device_call(gpu_ctx, worlds, 10)
  alone = [device_call(gpu_ctx, [w], 10)[0] for w in worlds]
  for t, a, b in zip(together, again, alone):
    for name in ('sel', 'acq', 'mu', 'var'):
      assert getattr(t, name).tobytes() == getattr(a, name).tobytes(), name    # identical calls are bit-identical
      assert getattr(t, name).tobytes() == getattr(b, name).tobytes(), name    # ... and a run is the run alone, bit for bit
    assert t.status == 0
  assert len({tuple(t.sel.tolist()) for t in together}) == 3


def test_not_positive_definite_run_is_flagged_and_the_others_are_not(gpu_ctx):
  """A NaN input row in one run's pool: its values are NaN from the first appended row on, np.argmax selects it, its pivot
  l_pp^2 is NaN -- HBO_NOT_PD for that run (the host loop's cache fails to factorise there), index 0 from then on; the runs that share
  the call are unaffected, bit for bit."""
  nat = _nv().nat
  worlds = [cases.world(c, np.float64) for c in _ind_cases()]
  pool_x = worlds[0].pool_x.copy()
  pool_x[7] = np.nan
  worlds[0] = worlds[0]._replace(pool_x=pool_x)
  out = device_call(gpu_ctx, worlds, 10)
  assert [r.status for r in out] == [nat.HBO_NOT_PD, 0, 0] and out[0].rc == nat.HBO_NOT_PD
  assert out[0].sel[0] == 7 and (out[0].sel[1:] == 0).all() and np.isnan(out[0].acq).all() and np.isnan(out[0].mu).all()
  alone = device_call(gpu_ctx, worlds[1:], 10)
  for t, a in zip(out[1:], alone):
    assert t.acq.tobytes() == a.acq.tobytes() and t.sel.tobytes() == a.sel.tobytes() and t.mu.tobytes() == a.mu.tobytes()
    assert np.isfinite(t.acq).all()


# ---- routing -----------------------------------------------------------------------------------------------------------------
def _host_and_device(case, iters=None):
  nv = _nv()
  w = cases.world(case, np.float64)
  fn = getattr(nv.acfun, cases.ACQS[case.acq][2])
  pool = nv.defs.SubDataset(w.pool_x, w.pool_y)
  m_host, m_dev = native_model(w), native_model(w, {'bo_on_device': True})
  iters = case.iters if iters is None else iters
  s_host = nv.bayesopt.simulated_bayesopt(m_host, KEY, pool, fn, iters)
  s_dev = nv.bayesopt.simulated_bayesopt(m_dev, KEY, pool, fn, iters)
  return w, m_host, m_dev, s_host, s_dev


@pytest.mark.parametrize('name', ['matern52-ei', 'dot_product-pi2', 'prior', 'linear_mlp'])
def test_flag_on_returns_what_the_host_loop_returns(name, gpu_ctx):
  case = cases.BY_NAME[name]
  w, m_host, m_dev, s_host, s_dev = _host_and_device(case)
  assert np.array_equal(s_host.x, s_dev.x) and np.array_equal(s_host.y, s_dev.y)
  assert s_dev.x.shape[0] == case.n0 + case.iters
  assert set(m_host.dataset) == set(m_dev.dataset)
  for k in m_host.dataset:
    assert np.array_equal(m_host.dataset[k].x, m_dev.dataset[k].x) and np.array_equal(m_host.dataset[k].y, m_dev.dataset[k].y)
  mu_h, var_h = m_host.predict(w.pool_x, sub_dataset_key=KEY)
  mu_d, var_d = m_dev.predict(w.pool_x, sub_dataset_key=KEY)
  np.testing.assert_allclose(mu_d, mu_h, rtol=RTOL, atol=ATOL)
  np.testing.assert_allclose(var_d, var_h, rtol=RTOL, atol=ATOL)


def test_batch_equals_the_single_runs(gpu_ctx):
  nv = _nv()
  worlds = [cases.world(c, np.float64) for c in _ind_cases()]
  fns = [getattr(nv.acfun, cases.ACQS[w.case.acq][2]) for w in worlds]
  pools = [nv.defs.SubDataset(w.pool_x, w.pool_y) for w in worlds]
  batch_models = [native_model(w) for w in worlds]            # simulated_bayesopt_batch does not need the flag
  subs = nv.bayesopt.simulated_bayesopt_batch([(m, KEY, p, f) for m, p, f in zip(batch_models, pools, fns)], 10)
  for w, p, f, sub in zip(worlds, pools, fns, subs):
    single = nv.bayesopt.simulated_bayesopt(native_model(w, {'bo_on_device': 1}), KEY, p, f, 10)
    assert np.array_equal(single.x, sub.x) and np.array_equal(single.y, sub.y)
    assert sub.x.shape[0] == w.case.n0 + 10
  other = cases.world(cases.BY_NAME['matern52-ei'], np.float64)
  with pytest.raises(ValueError, match='bo_on_device: .*must share'):
    nv.bayesopt.simulated_bayesopt_batch([(native_model(worlds[0]), KEY, pools[0], fns[0]),
                                          (native_model(other), KEY, nv.defs.SubDataset(other.pool_x, other.pool_y), fns[0])], 10)


def test_unmet_conditions_raise_with_the_flag_on(gpu_ctx):
  nv = _nv()
  w = cases.world(cases.BY_NAME['matern52-ei'], np.float64)
  pool = nv.defs.SubDataset(w.pool_x, w.pool_y)
  with pytest.raises(ValueError, match='bo_on_device: .*random search'):
    nv.bayesopt.simulated_bayesopt(native_model(w, {'bo_on_device': True}), KEY, pool, nv.acfun.rand, 3, random_key=0)
  with pytest.raises(ValueError, match='bo_on_device: .*retrain'):
    nv.bayesopt.simulated_bayesopt(native_model(w, {'bo_on_device': True, 'retrain': 5}), KEY, pool, nv.acfun.ei, 3)
  with pytest.raises(ValueError, match='bo_on_device: .*more than one column'):
    nv.bayesopt.simulated_bayesopt(native_model(w, {'bo_on_device': True}), KEY, nv.defs.SubDataset(w.pool_x, np.hstack((w.pool_y, w.pool_y))),
                                   nv.acfun.ei, 3)
  with pytest.raises(ValueError, match='bo_on_device: .*pool is empty'):
    nv.bayesopt.simulated_bayesopt(native_model(w, {'bo_on_device': True}), KEY, nv.defs.SubDataset(w.pool_x[:0], w.pool_y[:0]), nv.acfun.ei, 3)
  with pytest.raises(ValueError, match='bo_on_device: .*not one of the native'):
    nv.bayesopt.simulated_bayesopt(native_model(w, {'bo_on_device': True}), KEY, pool, lambda **kw: np.zeros((w.case.M, 1)), 3)
  m = native_model(w, {'bo_on_device': True})
  with pytest.raises(ValueError, match='bo_on_device: .*HGP'):
    nv.bayesopt.simulated_bayesopt(nv.gp.HGP(m.dataset, m.mean_func, m.cov_func, m.params, m.warp_func), KEY, pool, nv.acfun.ei, 3)
  with pytest.raises(ValueError, match='bo_on_device: .*Kumaraswamy'):
    nv.bayesopt.simulated_bayesopt(nv.gp.GP(m.dataset, m.mean_func, nv.kernel.matern52_kumar, m.params, m.warp_func), KEY, pool, nv.acfun.ei, 3)
  assert m.dataset[KEY].x.shape[0] == w.case.n0   # nothing was appended


def test_refusals_come_before_device_work(gpu_ctx):
  nat = _nv().nat
  err = lambda: (nat.lib().hbo_last_error(gpu_ctx.handle) or b'').decode()
  host.check_refusals(gpu_ctx.handle, err)
  # a workspace above half of the device memory: (n0 + iters) x (M + n0) doubles = 65536 x 2^30 x 8 bytes; refused before anything is read
  a = host.bo_args(iters=65536)
  a['runs'][0].M = 1 << 30
  assert host.bo_call(a, gpu_ctx.handle) == nat.HBO_ERR_UNSUPPORTED and 'half of the device memory' in err()
  sel, acq, status = a['_keep'][5:]
  assert np.all(sel == 7) and np.all(acq == 7.0) and np.all(status == 7)
