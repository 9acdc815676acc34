"""[value, per-task values, gradient, return code] of hbo_objective as bytes, over the paths objective_local can take, for an A/B of two
builds of the library ($HBO_LIB picks the build: profiles/objective_refactor.md).

  python tools/objective_bytes.py run <out.npz>                  one process per build and run
  python tools/objective_bytes.py compare <a1.npz> <a2.npz> <b.npz>
  python tools/objective_bytes.py launches                       four of the calls alone: the program to put behind rocprofv3 --kernel-trace
  python tools/objective_bytes.py compare-traces <a_kernel_trace.csv> <b_kernel_trace.csv>

`compare-traces`: kernel names, grids and workgroup sizes of two kernel traces, in dispatch order.  `compare`: an array that already differs between the two runs a1, a2 of ONE build (sums made with floating-point atomics) is listed and
held to max|b - a1| <= 1e-10 max|a1| on the other build; every other array must be identical in all three files.  Exit 1 otherwise.

Paths (each call well under a second): single-workgroup (T = 3, n = 5 / 100 / 128, fp64 and fp32), blocked without look-ahead (n = 129,
300), look-ahead with the early inverse (n = 512, lookahead = 2), the one-sweep inverse (T = 1 and T = 8, n = 1024, lookahead = 2 and
sweep = 2), extra rows (EKL and EUC, n = 130, 128 aligned columns; value-only EKL beside a task of two blocks with few columns), one task
of three that is not positive definite, hbo_objective_sharded without a communicator (T = 2) and on an empty rank, and the first
evaluations of hbo_train_adam / hbo_train_lbfgs (tasks of 64 / 50 / 40 points, batch 32) through GP.train."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def families(rng, d):
  from hyperbo_amd.gp_utils import kernel, mean
  feats = (4, 5)
  base = lambda nls: {'lengthscale': rng.normal(size=nls) * 0.3 + 0.5, 'signal_variance': np.array(0.3), 'noise_variance': np.array(-2.0),
                      'constant': np.array(0.4), 'dot_prod_sigma': np.array(0.7), 'dot_prod_bias': np.array(0.2)}
  fam = {}
  fam['se_constant'] = (mean.constant, kernel.squared_exponential, base(d))
  m = base(d); m['linear_mean'] = {'kernel': rng.normal(size=(d, 1)), 'bias': rng.normal(size=1)}
  fam['matern52_linear'] = (mean.linear, kernel.matern52, m)
  fam['dot_zero'] = (mean.zero, kernel.dot_product, base(d))
  m = base(d); m['kumar_params'] = {'a': rng.uniform(-1.0, 1.0, size=d), 'b': rng.uniform(-1.0, 1.0, size=d)}
  fam['se_kumar_constant'] = (mean.constant, kernel.squared_exponential_kumar, m)
  m = base(feats[-1]); fin = d; m['mlp_params'] = {}
  for l, f in enumerate(feats):
    m['mlp_params'][f'Dense_{l}'] = {'kernel': rng.normal(size=(fin, f)) * 0.7, 'bias': rng.normal(size=f) * 0.1}; fin = f
  m['linear_mean'] = {'kernel': rng.normal(size=(feats[-1], 1)), 'bias': rng.normal(size=1)}
  fam['se_mlp_linear_mlp'] = (mean.linear_mlp, kernel.squared_exponential_mlp, m)
  return fam, feats


def task(rng, n, d, m=1):
  x = rng.uniform(size=(n, d)); w = rng.normal(size=(d, m))
  return x, np.sin(2 * np.pi * x @ w) + 0.1 * rng.normal(size=(n, m))


def run(out_path, launches_only=False):
  from hyperbo_amd import _model, _native as nat
  from hyperbo_amd.basics import definitions as defs
  from hyperbo_amd.gp_utils import gp, objectives, utils
  ctx = nat.default_context()
  rng = np.random.default_rng(2024)
  d = 3
  fam, feats = families(rng, d)
  out = {}

  def iid(sizes):
    return {k: defs.SubDataset(*task(rng, n, d)) for k, n in enumerate(sizes)}

  def aligned(shapes):
    return {k: defs.SubDataset(*task(rng, n, d, m), aligned=k) for k, (n, m) in enumerate(shapes)}

  def call(name, dev, famname, objective, want_grad, sharded=False):
    mu, cov, model = fam[famname]
    bm = _model.BuiltModel(mu, cov, defs.GPParams(model=model, config={'mlp_features': feats}), utils.DEFAULT_WARP_FUNC, dev.dtype, d)
    T = dev.num_tasks
    val, cnt = C.c_double(0.0), C.c_double(0.0)
    pt = (C.c_double * max(T, 1))()
    g = (C.c_double * max(bm.layout.total, 1))() if want_grad else None
    if sharded:
      rc = nat.lib().hbo_objective_sharded(ctx.handle, bm.ref(), dev._h if T else None, objective, C.byref(val), C.byref(cnt), g, None)
    else:
      rc = nat.lib().hbo_objective(ctx.handle, bm.ref(), dev._h, objective, C.byref(val), pt, g)
    key = f'{name}/{famname}/{"grad" if want_grad else "value"}'
    out[key + '/value'] = np.array([val.value, cnt.value])
    out[key + '/per_task'] = np.array(list(pt)[:T])
    out[key + '/rc'] = np.array([rc])
    if want_grad:
      out[key + '/gradient'] = np.array(list(g)[:bm.layout.total])

  def over_families(name, data, objective=objectives.OBJ_NLL, grads=(False, True), dtype=np.float64, only_aligned=False, options=None, sharded=False,
                    names=None):
    dev = objectives.DeviceDataset(data, dtype=dtype, only_aligned=only_aligned)
    try:
      for k_, v_ in (options or {}).items():
        ctx.set_option(k_, v_)
      for famname in (names or fam):
        for want_grad in grads:
          call(name, dev, famname, objective, want_grad, sharded)
    finally:
      for k_ in (options or {}):
        ctx.set_option(k_, {'lookahead': 1, 'sweep': 1}[k_])
      dev.close()

  small = iid((5, 100, 128))
  if launches_only:   # single-workgroup, n = 512 with gradient, the T = 8 sweep, EKL with extra rows
    one = ('se_constant',)
    over_families('small_fp64', small, grads=(True,), names=one)
    over_families('lookahead_512', iid((512,)), grads=(True,), options={'lookahead': 2}, names=one)
    over_families('sweep_T8_1024', iid((1024, 1000, 900, 770, 515, 260, 130, 1)), grads=(True,), options={'lookahead': 2, 'sweep': 2}, names=one)
    over_families('extra_rows_ekl', aligned(((130, 128),)), objective=objectives.OBJ_EKL, grads=(True,), only_aligned=True, names=one)
    print(f'{len(out)} arrays')
    return
  over_families('small_fp64', small)
  over_families('small_fp32', small, dtype=np.float32)
  over_families('blocked_129', iid((129,)))
  over_families('blocked_300', iid((300,)))
  over_families('lookahead_512', iid((512,)), options={'lookahead': 2})
  over_families('sweep_T1_1024', iid((1024,)), options={'lookahead': 2, 'sweep': 2})
  over_families('sweep_T8_1024', iid((1024, 1000, 900, 770, 515, 260, 130, 1)), options={'lookahead': 2, 'sweep': 2})
  wide = aligned(((130, 128),))
  over_families('extra_rows_ekl', wide, objective=objectives.OBJ_EKL, only_aligned=True)
  over_families('extra_rows_euc', wide, objective=objectives.OBJ_EUC, only_aligned=True)
  over_families('extra_rows_ekl_beside_small_m', aligned(((130, 128), (200, 3))), objective=objectives.OBJ_EKL, grads=(False,), only_aligned=True)
  bad = iid((40, 60, 50))
  bad[1].x[7, 0] = np.nan   # its Gram matrix is NaN: the factorisation sets this task's info word
  over_families('not_pd_small', bad)
  bad2 = iid((140, 200, 50))
  bad2[0].x[7, 0] = np.nan
  over_families('not_pd_blocked', bad2)
  over_families('sharded_T2', iid((150, 90)), sharded=True)
  over_families('sharded_T2_small', iid((70, 90)), sharded=True)
  empty_src = iid((10,))
  dev = objectives.DeviceDataset(empty_src, keys=[])
  for famname in fam:
    call('sharded_empty', dev, famname, objectives.OBJ_NLL, True, sharded=True)
  dev.close()

  # the trainers' first evaluation goes through objective_local's sharded door: a few steps of each, the parameters they end at
  def flat(tree):
    return np.concatenate([flat(tree[k]) for k in sorted(tree)]) if isinstance(tree, dict) else np.asarray(tree, dtype=np.float64).ravel()
  train_data = iid((64, 50, 40))
  for method, flag in (('adam', 'adam_on_device'), ('lbfgs', 'lbfgs_on_device')):
    for famname in ('se_constant', 'se_mlp_linear_mlp'):
      mu, cov, model = fam[famname]
      config = {'method': method, 'batch_size': 32, 'max_training_step': 3, 'learning_rate': 1e-3, 'objective': objectives.nll, 'mlp_features': feats,
                flag: True}
      copy = lambda v: {kk: copy(vv) for kk, vv in v.items()} if isinstance(v, dict) else np.array(v)
      unused = ('dot_prod_sigma', 'dot_prod_bias') + (('constant',) if 'linear_mean' in model else ())
      tree = {k: copy(v) for k, v in model.items() if k not in unused}
      g = gp.GP(train_data, mu, cov, defs.GPParams(model=tree, config=config), utils.DEFAULT_WARP_FUNC)
      out[f'train_{method}/{famname}/params'] = flat(g.train(key=0).model)
  np.savez(out_path, **out)
  print(f'{len(out)} arrays -> {out_path}')


def compare(a1, a2, b):
  A1, A2, B = np.load(a1), np.load(a2), np.load(b)
  same = lambda x, y: x.shape == y.shape and x.tobytes() == y.tobytes()
  if sorted(A1.files) != sorted(B.files) or sorted(A1.files) != sorted(A2.files):
    print('the files hold different arrays'); return 1
  noisy, failed = [], []
  for k in sorted(A1.files):
    if same(A1[k], A2[k]):
      if not same(A1[k], B[k]):
        failed.append(k)
    else:
      noisy.append(k)
      scale = np.nanmax(np.abs(A1[k])) if A1[k].size else 0.0
      if A1[k].shape != B[k].shape or not np.array_equal(np.isnan(A1[k]), np.isnan(B[k])) or np.nanmax(np.abs(A1[k] - B[k]), initial=0.0) > 1e-10 * scale:
        failed.append(k)
  print(f'{len(A1.files)} arrays; {len(A1.files) - len(noisy)} identical in the two runs of the first build')
  for k in noisy:
    print('  differs between two runs of ONE build (held to 1e-10 of its largest entry):', k)
  for k in failed:
    print('  DIFFERENT in the other build:', k)
  print('identical' if not failed else f'{len(failed)} array(s) differ')
  return 1 if failed else 0


def compare_traces(a, b):
  import csv

  def launches(path):
    with open(path, newline='') as f:
      rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r['Dispatch_Id']))
    cols = [c for c in rows[0] if c.startswith(('Grid_Size', 'Workgroup_Size'))]
    return [(r['Kernel_Name'],) + tuple(r[c] for c in cols) for r in rows]
  la, lb = launches(a), launches(b)
  first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), None)
  print(f'{len(la)} and {len(lb)} launches')
  if first is not None or len(la) != len(lb):
    i = first if first is not None else min(len(la), len(lb))
    print('first difference at launch', i, la[i:i + 1], lb[i:i + 1])
    return 1
  print('same kernel names, grids and workgroup sizes in the same order')
  return 0


if __name__ == '__main__':
  if len(sys.argv) >= 3 and sys.argv[1] == 'run':
    run(sys.argv[2])
  elif len(sys.argv) == 2 and sys.argv[1] == 'launches':
    run(None, launches_only=True)
  elif len(sys.argv) == 4 and sys.argv[1] == 'compare-traces':
    sys.exit(compare_traces(*sys.argv[2:]))
  elif len(sys.argv) == 5 and sys.argv[1] == 'compare':
    sys.exit(compare(*sys.argv[2:]))
  else:
    sys.exit(__doc__)
