"""The five batched entry points refuse the same mixed batches the same way (csrc/api_internal.h: model_family_check): another
covariance -> HBO_ERR_ARG 'must share'; a Kumaraswamy-warped model -> HBO_ERR_UNSUPPORTED naming the entry point; an invalid model ->
validate_model's HBO_ERR_ARG; and, per sample in that order, an invalid model in front of a warped one -> HBO_ERR_ARG.  With a live
context, a real cache and a real dataset behind the calls; no output is written."""
import ctypes as C

import numpy as np
import pytest

import family_check_cases as family
from hyperbo_amd import _native as nat

pytestmark = pytest.mark.gpu

D, N, S, M, R = family.D, 8, 2, 3, 2
SENTINEL = 7.0


@pytest.fixture(scope='module')
def world(gpu_ctx):
  """8 observations in D = 2 as a cache of the good model and as a dataset of one 8-row task."""
  rng = np.random.default_rng(5)
  x, y = rng.uniform(size=(N, D)), rng.normal(size=(N, 1))
  lib, ctx = nat.lib(), gpu_ctx.handle
  model, keep = family.good_model()
  cache, ds = C.c_void_p(), C.c_void_p()
  assert lib.hbo_factor(ctx, C.byref(model), nat.ptr(x), N, nat.ptr(y), 1, C.byref(cache)) == nat.HBO_OK
  task = (nat.Task * 1)()
  task[0].x, task[0].y, task[0].n, task[0].m = nat.ptr(x).value, nat.ptr(y).value, N, 1
  assert lib.hbo_dataset_create(ctx, nat.F64, D, task, 1, C.byref(ds)) == nat.HBO_OK
  yield dict(x=x, y=y, cache=cache, ds=ds, xq=rng.uniform(size=(M, D)), keep=keep)
  lib.hbo_dataset_free(ctx, ds)
  lib.hbo_cache_free(ctx, cache)


def _calls(ctx, w, models):
  """name -> (call, outputs): each entry point on the two models, its outputs pre-filled."""
  lib = nat.lib()
  dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
  ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
  full = lambda *shape: np.full(shape, SENTINEL)
  prm, nse = (C.c_double * S)(3.0, 3.0), (C.c_double * S)(0.1, 0.1)
  caches = (C.c_void_p * S)(w['cache'].value, w['cache'].value)
  x, y, xq = w['x'], w['y'], w['xq']
  out = {}

  acq = full(S, M)
  out['hbo_acq_samples'] = (lambda: lib.hbo_acq_samples(ctx, models, S, nat.ptr(x), N, nat.ptr(y), 1, nat.ptr(xq), M, nat.ACQ_EI, prm, nse,
                                                        1.0, nat.ptr(acq)), [acq])
  nll, per = full(S), full(S, 1)
  out['hbo_nll_samples'] = (lambda: lib.hbo_nll_samples(ctx, models, S, w['ds'], dp(nll), dp(per)), [nll, per])
  val, grad = full(S, M), full(S, M, D)
  out['hbo_acq_grad_samples'] = (lambda: lib.hbo_acq_grad_samples(ctx, models, S, caches, nat.ptr(xq), M, nat.ACQ_UCB, prm, nse, 1.0,
                                                                  nat.ptr(val), dp(grad)), [val, grad])
  opts = nat.AcqOptOpts(memory=4, ls_steps=5, max_iters=5, c1=1e-4, tau=0.5, pgtol=1e-6, ftol=0.0)
  ns = lib.hbo_acq_opt_state_doubles(D, opts.memory)
  x0, state = np.full((R, D), 0.5), np.zeros((R, ns))
  x_out, v_out, status, log = full(R, D), full(R), np.full(R, 7, dtype=np.int32), np.full(4 * R, 7, dtype=nat.ACQ_OPT_EVAL_DTYPE)
  out['hbo_acq_maximize'] = (lambda: lib.hbo_acq_maximize(ctx, models, S, caches, nat.ptr(x0), R, None, None, nat.ACQ_UCB, prm, nse, 1.0,
                                                          C.byref(opts), nat.ptr(state), 4, nat.ptr(x_out), nat.ptr(v_out),
                                                          nat.ptr(status), nat.ptr(log)), [x_out, v_out, status, log, state])
  runs = (nat.BoRun * S)()
  xc, yc = np.ascontiguousarray(x), np.ascontiguousarray(y[:, 0])
  for r in runs:
    r.xc, r.yc, r.M, r.n0 = nat.ptr(xc).value, nat.ptr(yc).value, N, 0
    r.acq_id, r.param_mode, r.param, r.add_noise, r.scale0, r.scale = nat.ACQ_EI, nat.BO_PARAM_MAX_PLUS, 0.0, 0.1, 1.0, 1.0
  sel, bacq, bst, mu, var = np.full((S, 2), 7, dtype=np.int32), full(S, 2), np.full(S, 7, dtype=np.int32), full(S * N), full(S * N)
  out['hbo_bo_simulated'] = (lambda: lib.hbo_bo_simulated(ctx, models, runs, S, 2, ip(sel), dp(bacq), nat.ptr(mu), nat.ptr(var), ip(bst)),
                             [sel, bacq, bst, mu, var, xc, yc])
  return out


@pytest.mark.parametrize('name', list(family.CASES))
def test_batched_entry_points_refuse_the_same_mixed_batches(gpu_ctx, world, name):
  ctx = gpu_ctx.handle
  models, keep, code, word = family.pair(name)
  calls = _calls(ctx, world, models)
  assert sorted(calls) == ['hbo_acq_grad_samples', 'hbo_acq_maximize', 'hbo_acq_samples', 'hbo_bo_simulated', 'hbo_nll_samples']
  for fn, (call, outputs) in calls.items():
    before = [o.copy() for o in outputs]
    rc = call()
    msg = (nat.lib().hbo_last_error(ctx) or b'').decode()
    assert rc == code and word.format(fn=fn) in msg, (fn, name, rc, msg)
    assert all(np.array_equal(b.view(np.uint8), o.view(np.uint8)) for b, o in zip(before, outputs)), (fn, name)   # nothing was written
  del keep
