"""The cases of the device BO loop's tests (test_bo_device_host.py on the CPU, test_gpu_bo_device.py on the GPU): small simulated-BO
problems -- a pool of pre-evaluated candidates, the observations the test sub-dataset starts with, a model, an acquisition function.

`exact`: the GPU test compares the selected SEQUENCE of the case with the oracle loop's.  That is only meaningful where no iteration
is decided by rounding, so test_bo_device_host.py asserts for every such case that the best and second-best oracle value of every
iteration are at least GAP apart (relative), iterations with an exact tie excepted; a case that does not meet it gets another seed.
The other cases are checked by replay only (the oracle driven along the device's own selections)."""
import collections

import numpy as np

import helpers
from oracle import hyperbo_oracle as o

GAP = 1e-6
KEY = 'test'
WFO = o.DEFAULT_WARP_FUNC

# acquisition name -> (oracle epilogue, oracle callback(dataset, key), native function name in bo_utils/acfun.py)
ACQS = {
    'ei': (o.expected_improvement_sub, o.ei_callback_default, 'expected_improvement'),
    'pi': (o.probability_of_improvement_sub, o.pi_callback_default, 'probability_of_improvement'),
    'pi2': (o.probability_of_improvement_sub, lambda ds, key: o.pi_callback_default(ds, key, use_std=True), 'pi2'),
    'ucb3': (o.ucb_sub, lambda ds, key: 3.0, 'ucb3'),
}

Case = collections.namedtuple('Case', 'name kernel mean mlp_kernel acq D M n0 iters seed key_absent exact dup nan_at')


def _case(name, kernel='squared_exponential', mean='constant', mlp_kernel=False, acq='ei', D=3, M=300, n0=5, iters=40, seed=1,
          key_absent=False, exact=True, dup=None, nan_at=None):
  return Case(name, kernel, mean, mlp_kernel, acq, D, M, n0, iters, seed, key_absent, exact, dup, nan_at)


PARITY = [_case(f'{k}-{a}', kernel=k, acq=a, seed=11 + 4 * i + j)
          for i, k in enumerate(helpers.KERNELS) for j, a in enumerate(('ei', 'pi', 'pi2', 'ucb3'))]
FAMILIES = [
    _case('linear', kernel='matern52', mean='linear', acq='ei', seed=41),
    _case('linear_mlp', kernel='squared_exponential', mean='linear_mlp', acq='ucb3', seed=42),
    _case('mlp_kernel', kernel='matern32', mean='constant', mlp_kernel=True, acq='pi', seed=43),
    _case('D1', kernel='matern52', acq='ei', D=1, seed=44),
    _case('D33', kernel='squared_exponential', acq='ucb3', D=33, seed=45),
]
EDGES = [
    _case('M1', acq='ei', M=1, n0=2, iters=6, seed=51),
    _case('M257', kernel='matern52', acq='ucb3', M=257, n0=3, iters=12, seed=56),        # a partial last workgroup, the winner in it
    _case('prior', kernel='matern32', acq='ei', M=300, n0=0, iters=12, seed=53, key_absent=True),   # prior branch, scale0 != scale
    _case('rows130', kernel='squared_exponential', acq='pi', M=64, n0=0, iters=130, seed=54, key_absent=True),   # no 128-row limit
]
# replay only: exact ties (the prior under UCB ties everywhere; two identical rows in different workgroups of which the loop selects
# one after rows have been appended -- bo_loop_oracle.case_world places them), a NaN value in the pool
TIES = [
    _case('tie_prior', kernel='squared_exponential', acq='ucb3', n0=0, iters=8, seed=61, key_absent=True, exact=False),
    _case('tie_dup', kernel='matern52', acq='ei', iters=30, seed=62, exact=False, dup=(5, 270)),   # dup: where the twin goes when the original sits in workgroup >= 1 / in workgroup 0
]
NAN = [_case('nan_y', kernel='squared_exponential', acq='ucb3', iters=12, seed=63, exact=False, nan_at=3)]   # the candidate of iteration 3 has a NaN value (bo_loop_oracle.case_world)
ALL = PARITY + FAMILIES + EDGES + TIES + NAN
BY_NAME = {c.name: c for c in ALL}
assert len(BY_NAME) == len(ALL)


def _cast(t, dtype):
  return {k: _cast(v, dtype) for k, v in t.items()} if isinstance(t, dict) else np.asarray(t, dtype=dtype)


World = collections.namedtuple('World', 'case dtype model other_x other_y pool_x pool_y x0 y0 twins', defaults=(None,))   # twins: (lower, higher) index of two identical rows


def world(case, dtype=np.float64):
  """The arrays of a case, rounded to `dtype` (the fp32 runs and their fp64 oracle see the same numbers)."""
  rng = np.random.default_rng(1000 + case.seed)
  model = _cast(helpers.make_model(rng, case.mean, case.mlp_kernel, case.D), dtype)
  n_all = case.M + case.n0 + 8
  x, y = helpers.synthetic_task(rng, n_all, case.D, dtype=dtype)
  pool_x, pool_y = x[:case.M].copy(), y[:case.M].copy()
  x0, y0 = x[case.M:case.M + case.n0].copy(), y[case.M:case.M + case.n0].copy()
  return World(case, np.dtype(dtype), model, x[-8:].copy(), y[-8:].copy(), pool_x, pool_y, x0, y0)


def with_twin(w, src, dst):
  """Row `src` of the pool copied over row `dst`."""
  pool_x, pool_y = w.pool_x.copy(), w.pool_y.copy()
  pool_x[dst], pool_y[dst] = pool_x[src], pool_y[src]
  return w._replace(pool_x=pool_x, pool_y=pool_y, twins=(min(src, dst), max(src, dst)))


def with_nan(w, index):
  pool_y = w.pool_y.copy()
  pool_y[index] = np.nan
  return w._replace(pool_y=pool_y)


def oracle_funcs(case):
  kname = case.kernel + ('_mlp' if case.mlp_kernel else '')
  return getattr(o, case.mean), getattr(o, kname)


def oracle_params(w):
  return o.GPParams(model=_cast(w.model, np.float64), config={})


def oracle_dataset(w):
  """The dataset the loop starts from: one other (training) sub-dataset, and the test sub-dataset unless its key is absent."""
  f8 = lambda a: np.asarray(a, dtype=np.float64)
  ds = {0: o.SubDataset(f8(w.other_x), f8(w.other_y))}
  if not w.case.key_absent:
    ds[KEY] = o.SubDataset(f8(w.x0), f8(w.y0))
  return ds
