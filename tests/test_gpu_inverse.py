"""L, W = L^-1 and K^-1 = W^T W per 128-tile across the routes of the inverse -- the one-sweep inverse (each row-group size), the
block-recursive inverse started beside the panel chain (one matrix and batches), the inverse behind the factorisation, both tile sizes,
the three batch_bg forms and the three fp32 product forms -- through the test hook hbo_probe_factor_inverse (include/hbo_tune.h), which
runs the factor and inverse steps of an NLL evaluation with gradient on caller-chosen matrices.

The exact family (tests/inverse_cases.py; its conditions are proved on the host by tests/test_inverse_cases_host.py): integer factors
with an integer inverse, every product and partial sum far below 2^24 -- the device's L, W, K^-1, z and x are the integers, every entry,
every task, in fp64 and fp32, whatever the schedule.  Every option set first asserts the plan it names (hbo_probe_plan).  The
real-valued family covers what unit pivots leave out (1 / sqrt(d), genuine rounding) to a bound derived from LAPACK's own error.
Measured: profiles/inverse_errors.md.
"""
import ctypes as C

import numpy as np
import pytest

from hyperbo_amd import _native as nat

import inverse_cases as ic

pytestmark = pytest.mark.gpu

DTYPES = {'fp64': (nat.F64, np.float64), 'fp32': (nat.F32, np.float32)}
PUBLIC = ('lookahead', 'potrf_group', 'small_nblk', 'bf16x3')


def probe(ctx, dtype, mats, bs=None, beside=1, want=('chol', 'w', 'kinv', 'x', 'z')):
  """hbo_probe_factor_inverse on the matrices `mats` (and right-hand sides `bs`) -> (rc, per-task list of {name: array}, info, plan).
  Every output starts as a sentinel that no result equals."""
  code, npdt = DTYPES[dtype]
  T = len(mats)
  ns = [a.shape[0] for a in mats]
  m = bs[0].shape[1] if bs is not None else 0
  a = np.concatenate([np.ascontiguousarray(x, npdt).ravel() for x in mats])
  b = np.concatenate([np.ascontiguousarray(x, npdt).ravel() for x in bs]) if bs is not None else None
  nn, nm = sum(n * n for n in ns), sum(n * m for n in ns)
  out = {k: np.full(nn if k in ('chol', 'w', 'kinv') else nm, SENTINEL, npdt) for k in want if bs is not None or k not in ('x', 'z')}
  info = np.full(T, -7, np.int32)
  plan = nat.ProbePlan()
  rc = nat.lib().hbo_probe_factor_inverse(ctx.handle, code, T, (C.c_int64 * T)(*ns), nat.ptr(a), nat.ptr(b), m, beside,
                                          nat.ptr(out.get('chol')), nat.ptr(out.get('w')), nat.ptr(out.get('kinv')), nat.ptr(out.get('x')),
                                          nat.ptr(out.get('z')), info.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(plan))
  ctx.check(rc)
  tasks, oa, ob = [], 0, 0
  for n in ns:
    tasks.append({k: (v[oa:oa + n * n].reshape(n, n) if k in ('chol', 'w', 'kinv') else v[ob:ob + n * m].reshape(n, m)) for k, v in out.items()})
    oa += n * n; ob += n * m
  return rc, tasks, info, plan.as_dict()


SENTINEL = -77.5


class Options:
  """sets options on top of the defaults and puts the defaults (the public ones: what they were) back"""

  def __init__(self, ctx, opts):
    self.ctx, self.opts = ctx, opts

  def __enter__(self):
    self.saved = {k: self.ctx.get_option(k) for k in PUBLIC}
    for k, v in self.opts.items():
      self.ctx.set_option(k, v)

  def __exit__(self, *exc):
    for k in self.opts:
      self.ctx.set_option(k, self.saved.get(k, ic.OPTION_DEFAULTS[k]))


def exact_inputs(shape):
  ns, seeds = ic.shape_ns(shape)
  return [ic.exact_case(n, s) for n, s in zip(ns, seeds)]


def assert_task_exact(tag, got, case, plan):
  """every output of one task equal to the integers; on failure the per-tile counts of unequal entries and the plan"""
  msgs = []
  for name, (want, mask) in ic.expected_outputs(case).items():
    if name not in got:
      continue
    bad = ic.compare_tiles(got[name], want, mask)
    if bad.any():
      msgs.append('%s: %d unequal entries; per 128-tile:\n%s' % (name, int(bad.sum()), bad))
  assert not msgs, '%s n=%d plan=%s\n%s' % (tag, case['n'], plan, '\n'.join(msgs))


def assert_plan(tag, plan, want):
  diff = {k: (v, plan[k]) for k, v in want.items() if plan[k] != v}
  assert not diff, '%s: planned %s, the set names (expected, planned) %s' % (tag, plan, diff)


SET_PARAMS = [pytest.param(s, shape, dt, id='%s-%s-%s' % (s.name, shape, dt)) for s in ic.OPTION_SETS for shape in s.shapes for dt in s.dtypes]


@pytest.mark.parametrize('s,shape,dtype', SET_PARAMS)
def test_factor_and_inverse_are_exact_on_integer_factors(gpu_ctx, s, shape, dtype):
  ctx = gpu_ctx
  cases = exact_inputs(shape)
  tag = '%s %s %s' % (s.name, shape, dtype)
  with Options(ctx, s.opts):
    rc, tasks, info, plan = probe(ctx, dtype, [c['A'] for c in cases], [c['b'] for c in cases], s.beside)
    forms = (ctx.get_option('chol_form'), ctx.get_option('inv_forms'))
  print('PLAN %s %s forms=%s' % (tag, plan, forms))
  assert rc == nat.HBO_OK and not info.any(), (tag, rc, info)
  assert_plan(tag, plan, ic.expected_plan(s, shape))
  if dtype == 'fp32' and s.forms is not None:
    assert forms == s.forms, (tag, forms, s.forms)
  if dtype == 'fp64':
    assert forms == (0, 0), (tag, forms)
  for k, (got, case) in enumerate(zip(tasks, cases)):
    assert_task_exact('%s task %d' % (tag, k), got, case, plan)


NOT_PD_SETS = {'default': {}, 'sweep': dict(lookahead=2), 'early': dict(lookahead=2, sweep=0)}
NOT_PD_TASK = 4          # of B1: 1290 points
NOT_PD_ROW = 2 * ic.TILE + 37


@pytest.mark.parametrize('dtype', ['fp64', 'fp32'])
@pytest.mark.parametrize('route', sorted(NOT_PD_SETS))
def test_one_task_not_positive_definite(gpu_ctx, route, dtype):
  """task 4 of B1 with the pivot of a row of its third block at -1: HBO_NOT_PD, info_out names the task and the row, its outputs are
  NaN, the five others exact"""
  cases = exact_inputs('B1')
  mats = [c['A'] for c in cases]
  mats[NOT_PD_TASK], r = ic.not_pd_case(cases[NOT_PD_TASK], row=NOT_PD_ROW)
  with Options(gpu_ctx, NOT_PD_SETS[route]):
    rc, tasks, info, plan = probe(gpu_ctx, dtype, mats, [c['b'] for c in cases])
  print('PLAN not_pd-%s %s %s' % (route, dtype, plan))
  assert plan['sweep'] == (route == 'sweep') and plan['early'] == (route == 'early')
  assert rc == nat.HBO_NOT_PD
  assert info.tolist() == [r + 1 if k == NOT_PD_TASK else 0 for k in range(len(cases))]
  for k, (got, case) in enumerate(zip(tasks, cases)):
    if k == NOT_PD_TASK:
      assert all(np.isnan(v).all() for v in got.values()), {name: int(np.isnan(v).sum()) for name, v in got.items()}
    else:
      assert_task_exact('not_pd-%s %s task %d' % (route, dtype, k), got, case, plan)


REAL_SETS = {'default': {}, 'sweep': dict(lookahead=2, sweep=2), 'early': dict(lookahead=2, sweep=0)}


@pytest.mark.parametrize('n', ic.REAL_NS)
@pytest.mark.parametrize('route', sorted(REAL_SETS))
def test_real_valued_matrices_per_tile(gpu_ctx, route, n):
  """fp64, K = Gram(SE) + 1e-2 I: per 128-tile max |got - ref| / max |ref| against the longdouble reference, within
  REL_FACTOR x (LAPACK's worst tile) + FLOOR_C eps n for L, W and K^-1"""
  case = ic.real_case(n)
  with Options(gpu_ctx, REAL_SETS[route]):
    rc, tasks, info, plan = probe(gpu_ctx, 'fp64', [case['K']], [case['b']], want=('chol', 'w', 'kinv'))
  assert rc == nat.HBO_OK and not info.any()
  nblk = -(-n // ic.TILE)
  assert plan['sweep'] == (route == 'sweep' and nblk >= 8) and plan['early'] == (route == 'early' or (route == 'sweep' and nblk < 8))
  masks = ic.real_masks(n)
  worst = {}
  for name in ('chol', 'w', 'kinv'):
    err = ic.tile_errors(tasks[0][name], case['ref'][name], masks[name])
    bound, yard = ic.real_bound(case, name)
    worst[name] = (err.max(), bound)
    print('REAL n=%d %s %s: worst tile %.3e at %s, yardstick %.3e, bound %.3e, ratio %.3f' % (
        n, route, name, err.max(), np.unravel_index(err.argmax(), err.shape), yard, bound, err.max() / bound))
  # above the diagonal of W: zeros, as in the exact family
  assert not np.triu(tasks[0]['w'], 1).any()
  for name, (e, bound) in worst.items():
    assert e <= bound, (name, e, bound, plan)


def test_hook_rejects_bad_arguments(gpu_ctx):
  """every refusal is HBO_ERR_ARG, names the hook, and leaves the outputs untouched"""
  lib, h = nat.lib(), gpu_ctx.handle
  case = ic.exact_case(129, 0)
  n, m = 129, ic.M_RHS
  a = case['A'].astype(np.float64); b = np.ascontiguousarray(case['b'], np.float64)
  outs = {k: np.full((n, n) if k in ('chol', 'w', 'kinv') else (n, m), SENTINEL) for k in ('chol', 'w', 'kinv', 'x', 'z')}
  info = np.full(1, -7, np.int32)
  plan = nat.ProbePlan()
  C.memset(C.byref(plan), 0x55, C.sizeof(plan))
  one = (C.c_int64 * 1)(n)

  def call(ctx=h, dtype=nat.F64, T=1, ns=one, a_=nat.ptr(a), b_=nat.ptr(b), m_=m, beside=1):
    return lib.hbo_probe_factor_inverse(ctx, dtype, T, ns, a_, b_, m_, beside, nat.ptr(outs['chol']), nat.ptr(outs['w']), nat.ptr(outs['kinv']),
                                        nat.ptr(outs['x']), nat.ptr(outs['z']), info.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(plan))

  bad = [dict(dtype=2), dict(dtype=-1), dict(T=0), dict(T=65), dict(ns=None), dict(a_=None), dict(ns=(C.c_int64 * 1)(0)),
         dict(ns=(C.c_int64 * 1)(4097)), dict(m_=0), dict(m_=9), dict(m_=-1), dict(b_=None), dict(b_=None, m_=1), dict(b_=None, m_=0), dict(beside=2), dict(beside=-1)]
  for kw in bad:
    rc = call(**kw)
    assert rc == nat.HBO_ERR_ARG, (kw, rc)
    assert b'hbo_probe_factor_inverse' in lib.hbo_last_error(h), kw
    assert all((v == SENTINEL).all() for v in outs.values()) and info[0] == -7 and plan.la == 0x55555555, kw
  assert call(ctx=None) == nat.HBO_ERR_ARG
  assert all((v == SENTINEL).all() for v in outs.values())
  assert call() == nat.HBO_OK            # and the context still works
  assert np.array_equal(outs['chol'], case['L'].astype(np.float64)) and info[0] == 0
