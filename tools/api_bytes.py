"""Outputs, return codes and error texts of the entry points that left api.hip (dense.hip: hbo_gram, hbo_mean, hbo_chol_solve,
hbo_spd_solve; cache.hip: hbo_cache_export; dataset.hip: hbo_dataset_create / hbo_dataset_subsample; probe.hip; the options of api.hip)
as bytes, for an A/B of two builds of the library ($HBO_LIB picks the build: profiles/api_refactor.md).

  python tools/api_bytes.py run <out.npz>                  one process per build and run
  python tools/api_bytes.py compare <a1.npz> <a2.npz> <b.npz>
  python tools/api_bytes.py compare-traces <a_kernel_trace.csv> <b_kernel_trace.csv>

`compare`: every array must be equal (np.array_equal, NaN = NaN) in the two runs a1, a2 of one build and in the other build b; error
texts are arrays of bytes.  Exit 1 otherwise.  hbo_tune "poison" is on for the whole run.  Messages of a failed HIP call carry file and
line and are not produced here: every error case is an argument error, none launches anything.
`compare-traces`: launch count, multiset of (kernel, grid, workgroup, LDS) and per-queue order of kernel names of two rocprofv3 kernel traces."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D = 3
FEATS = (4, 5)


def run(out_path):
  from hyperbo_amd import _model, _native as nat
  from hyperbo_amd.basics import definitions as defs
  from hyperbo_amd.gp_utils import kernel, mean, utils
  lib = nat.lib()
  ctx = nat.default_context()
  h = ctx.handle
  ctx.set_option('poison', 1)
  rng = np.random.default_rng(31)
  out, cases = {}, [0]

  def put(key, *arrays_and_rc):
    cases[0] += 1
    for i, a in enumerate(arrays_and_rc):
      out[f'{key}/{i}'] = np.asarray(a)

  def err_text():
    return np.frombuffer(lib.hbo_last_error(h) or b'', dtype=np.uint8)

  def params(cov=None, mu=None):
    nls = FEATS[-1] if cov is not None and getattr(cov, 'uses_mlp', False) else D
    m = {'lengthscale': rng.normal(size=nls) * 0.3 + 0.5, 'signal_variance': np.array(0.3), 'noise_variance': np.array(-2.0),
         'constant': np.array(0.4), 'dot_prod_sigma': np.array(0.7), 'dot_prod_bias': np.array(0.2)}
    fm = FEATS[-1] if mu is mean.linear_mlp else D
    m['linear_mean'] = {'kernel': rng.normal(size=(fm, 1)), 'bias': rng.normal(size=1)}
    m['kumar_params'] = {'a': rng.uniform(-1.0, 1.0, size=D), 'b': rng.uniform(-1.0, 1.0, size=D)}
    fin, m['mlp_params'] = D, {}
    for l, f in enumerate(FEATS):
      m['mlp_params'][f'Dense_{l}'] = {'kernel': rng.normal(size=(fin, f)) * 0.7, 'bias': rng.normal(size=f) * 0.1}; fin = f
    return defs.GPParams(model=m, config={'mlp_features': FEATS})

  def built(mu, cov, dtype, p=None):
    return _model.BuiltModel(mu, cov, p or params(cov, mu), utils.DEFAULT_WARP_FUNC, np.dtype(dtype), D)

  # ---- hbo_gram / hbo_mean ----
  def gram(key, bm, dtype, n1, n2, diag):
    x1 = rng.uniform(size=(n1, D)).astype(dtype)
    x2 = None if n2 is None else rng.uniform(size=(n2, D)).astype(dtype)
    res = np.full((n1,) if diag else (n1, n1 if n2 is None else n2), np.nan, dtype=dtype)
    rc = lib.hbo_gram(h, bm.ref(), nat.ptr(x1), n1, nat.ptr(x2), 0 if n2 is None else n2, int(diag), nat.ptr(res))
    put(key, res, [rc])

  covs = {'se': kernel.squared_exponential, 'matern32': kernel.matern32, 'matern52': kernel.matern52, 'dot': kernel.dot_product}
  for dtype in (np.float32, np.float64):
    for name, cov in list(covs.items()) + [('se_mlp', kernel.squared_exponential_mlp), ('matern52_kumar', kernel.matern52_kumar)]:
      bm = built(mean.constant, cov, dtype)
      for n1 in (1, 127, 129):
        if name in ('se_mlp', 'matern52_kumar') and n1 != 129:
          continue
        tag = f'gram/{name}/{np.dtype(dtype).name}/{n1}'
        gram(tag + '/square', bm, dtype, n1, None, False)
        gram(tag + '/cross', bm, dtype, n1, n1 + 70, False)
        gram(tag + '/diag', bm, dtype, n1, None, True)
    for name, mu in (('zero', mean.zero), ('constant', mean.constant), ('linear', mean.linear), ('linear_mlp', mean.linear_mlp)):
      bm = built(mu, kernel.squared_exponential, dtype)
      for n in (1, 127, 129):
        x = rng.uniform(size=(n, D)).astype(dtype)
        res = np.full(n, np.nan, dtype=dtype)
        rc = lib.hbo_mean(h, bm.ref(), nat.ptr(x), n, nat.ptr(res))
        put(f'mean/{name}/{np.dtype(dtype).name}/{n}', res, [rc])

  # ---- hbo_chol_solve / hbo_spd_solve ----
  def spd(n, dtype, scale=1.0):
    a = rng.normal(size=(n, n + 3))
    return np.ascontiguousarray((a @ a.T / (n + 3) + 0.5 * np.eye(n)) * scale, dtype=dtype)

  for dtype in (np.float32, np.float64):
    for n in (1, 63, 64, 65, 130):
      for m in (1, 3):
        L = np.ascontiguousarray(np.linalg.cholesky(spd(n, np.float64)), dtype=dtype)
        b = rng.normal(size=(n, m)).astype(dtype)
        x = np.full((n, m), np.nan, dtype=dtype)
        rc = lib.hbo_chol_solve(h, nat.dtype_code(dtype), nat.ptr(L), n, nat.ptr(b), m, nat.ptr(x))
        put(f'chol_solve/{np.dtype(dtype).name}/{n}/{m}', x, [rc])

  def spd_solve(key, a, b, dtype, want):
    n = a.shape[0]
    m = 0 if b is None else b.shape[1]
    chol = np.full((n, n), 7.0, dtype=dtype) if 'chol' in want else None
    inv = np.full((n, n), 7.0, dtype=dtype) if 'inv' in want else None
    x = np.full((n, max(m, 1)), 7.0, dtype=dtype) if 'x' in want else None
    ld = C.c_double(7.0)
    rc = lib.hbo_spd_solve(h, nat.dtype_code(dtype), nat.ptr(a), n, nat.ptr(b), m, nat.ptr(chol), nat.ptr(inv), nat.ptr(x), C.byref(ld) if 'logdet' in want else None)
    put(key, *[v for v in (chol, inv, x) if v is not None], [ld.value], [rc], [ctx.get_option('chol_form'), ctx.get_option('inv_forms')])

  everything = ('chol', 'inv', 'x', 'logdet')
  for dtype in (np.float32, np.float64):
    for n in (1, 127, 128, 129, 300):
      a, b = spd(n, dtype), rng.normal(size=(n, 3)).astype(dtype)
      tag = f'spd_solve/{np.dtype(dtype).name}/{n}'
      spd_solve(tag + '/all', a, b, dtype, everything)
      if n in (1, 129):
        for w in everything:
          spd_solve(tag + '/only_' + w, a, b, dtype, (w,))
        spd_solve(tag + '/no_b', a, None, dtype, ('chol', 'inv', 'logdet'))
        bad = a.copy(); bad[n // 2, n // 2] = -1.0
        spd_solve(tag + '/not_pd', bad, b, dtype, everything)
  ctx.set_option('spd_diag_bound', 1)
  spd_solve('spd_solve/float32/300/diag_bound', spd(300, np.float32), rng.normal(size=(300, 3)).astype(np.float32), np.float32, everything)
  ctx.set_option('spd_diag_bound', 0)

  # ---- hbo_factor -> hbo_cache_export ----
  def factor_export(key, dtype, n, m, poison_x=False):
    x = rng.uniform(size=(n, D)).astype(dtype); y = rng.normal(size=(n, m)).astype(dtype)
    if poison_x:
      x[n // 2, 0] = np.nan   # its Gram matrix is NaN: not positive definite
    bm = built(mean.constant, kernel.matern32, dtype)
    k = C.c_void_p()
    rc = lib.hbo_factor(h, bm.ref(), nat.ptr(x), n, nat.ptr(y), m, C.byref(k))
    chol = np.full((n, n), 7.0, dtype=dtype); kinvy = np.full((n, m), 7.0, dtype=dtype); ymu = np.full((n, m), 7.0, dtype=dtype)
    rc2 = lib.hbo_cache_export(h, k, nat.ptr(chol), nat.ptr(kinvy), nat.ptr(ymu))
    kinvy2 = np.full((n, m), 7.0, dtype=dtype)
    rc3 = lib.hbo_cache_export(h, k, None, nat.ptr(kinvy2), None)
    lib.hbo_cache_free(h, k)
    put(key, chol, kinvy, ymu, kinvy2, [rc, rc2, rc3])

  for dtype in (np.float32, np.float64):
    for n in (1, 129):
      for m in (1, 3):
        factor_export(f'factor_export/{np.dtype(dtype).name}/{n}/{m}', dtype, n, m)
    factor_export(f'factor_export/{np.dtype(dtype).name}/not_pd', dtype, 129, 3, poison_x=True)

  # ---- datasets ----
  def make_tasks(shapes, dtype):
    keep, tasks = [], (nat.Task * len(shapes))()
    for i, (n, m) in enumerate(shapes):
      x = rng.uniform(size=(max(n, 0), D)).astype(dtype); y = rng.normal(size=(max(n, 0), m)).astype(dtype)
      keep.append((x, y))
      tasks[i].x, tasks[i].y, tasks[i].n, tasks[i].m = x.ctypes.data, y.ctypes.data, n, m
    return tasks, keep

  def objectives_of(key, ds, T, dtype):
    for name, mu, cov in (('se_constant', mean.constant, kernel.squared_exponential), ('matern52_linear', mean.linear, kernel.matern52),
                          ('mlp', mean.linear_mlp, kernel.squared_exponential_mlp)):
      bm = built(mu, cov, dtype)
      for obj in (0, 1, 2):   # OBJ_NLL, OBJ_EKL, OBJ_EUC
        # (the MLP gradient is summed with floating-point atomics: two runs of ONE build differ in its last bits, so only its value is here)
        for want_grad in (False,) if name == 'mlp' else (False, True):
          val = C.c_double(0.0); pt = (C.c_double * max(T, 1))(); g = (C.c_double * bm.layout.total)()
          rc = lib.hbo_objective(h, bm.ref(), ds, obj, C.byref(val), pt, g if want_grad else None)
          put(f'{key}/{name}/obj{obj}/grad{int(want_grad)}', [val.value], list(pt)[:T], list(g) if want_grad else [], [rc])

  def nll_fresh(key, dtype=np.float64):
    tasks, keep = make_tasks(((40, 1), (130, 1), (40, 1)), dtype)
    ds = C.c_void_p()
    rc = lib.hbo_dataset_create(h, nat.dtype_code(dtype), D, tasks, 3, C.byref(ds))
    bm = built(mean.constant, kernel.squared_exponential, dtype)
    val = C.c_double(0.0); pt = (C.c_double * 3)(); g = (C.c_double * bm.layout.total)()
    rc2 = lib.hbo_nll(h, bm.ref(), ds, C.byref(val), pt, g)
    lib.hbo_dataset_free(h, ds)
    put(key, [val.value], list(pt), list(g), [rc, rc2])

  for dtype in (np.float32, np.float64):
    shapes = ((60, 2), (0, 2), (130, 2), (60, 2), (5, 2), (130, 2), (1, 2))   # an empty task, ties in n
    tasks, keep = make_tasks(shapes, dtype)
    ds = C.c_void_p()
    rc = lib.hbo_dataset_create(h, nat.dtype_code(dtype), D, tasks, len(shapes), C.byref(ds))
    put(f'dataset/{np.dtype(dtype).name}/create_rc', [rc])
    T = sum(1 for n, _ in shapes if n > 0)
    objectives_of(f'dataset/{np.dtype(dtype).name}/created', ds, T, dtype)
    # sub-sample in device order (130, 130, 60, 60, 5, 1): the whole task, all rows permuted, fewer rows
    sizes = sorted((n for n, _ in shapes if n > 0), reverse=True)
    counts = np.array([-1, 130, 20, 60, -1, 1], dtype=np.int64)
    idx = np.concatenate([rng.permutation(sizes[k])[:c] for k, c in enumerate(counts) if c >= 0]).astype(np.int32)
    sub = C.c_void_p()
    rc = lib.hbo_dataset_subsample(h, ds, counts.ctypes.data_as(C.POINTER(C.c_int64)), idx.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(sub))
    put(f'dataset/{np.dtype(dtype).name}/subsample_rc', [rc])
    objectives_of(f'dataset/{np.dtype(dtype).name}/subsampled', sub, T, dtype)
    lib.hbo_dataset_free(h, sub)
    lib.hbo_dataset_free(h, ds)
    del keep

  # ---- probes ----
  n, M = 200, 70
  W = np.tril(rng.normal(size=(n, n))).astype(np.float32); K = rng.normal(size=(n, M)).astype(np.float32)
  for form, kb in ((0, 0.0), (1, float(np.abs(K).max()))):
    for counter in (0, 1):
      res = np.full(((n + 127) // 128, M), np.nan, dtype=np.float32)
      rc = lib.hbo_probe_post_product(h, form, nat.ptr(W), n, nat.ptr(K), M, kb, counter, nat.ptr(res))
      put(f'probe_post_product/{form}/{counter}', res, [rc])
  for dtype in (np.float32, np.float64):
    bm = built(mean.constant, kernel.squared_exponential, dtype)
    models = (nat.Model * 1)(bm.struct)
    for form, ns, n2 in ((1, [130], 50), (2, [130, 5, 140], 0)):
      x = rng.uniform(size=(sum(ns), D)).astype(dtype)
      x2 = rng.uniform(size=(n2, D)).astype(dtype) if n2 else None
      cap = sum((k + 256) * (max(k, n2) + 384) for k in ns)
      res = np.full(cap, np.nan, dtype=dtype)
      rows, ld = (C.c_int64 * len(ns))(), (C.c_int64 * len(ns))()
      rc = lib.hbo_probe_gram(h, form, C.cast(models, C.c_void_p), 1, nat.ptr(x), (C.c_int64 * len(ns))(*ns), len(ns), nat.ptr(x2), n2, 0, -77.0, nat.ptr(res),
                              cap, rows, ld)
      used = sum(r * l for r, l in zip(rows, ld))
      put(f'probe_gram/{np.dtype(dtype).name}/{form}', res[:used], list(rows), list(ld), [rc])
  tf = C.c_double(0.0)
  rc = lib.hbo_mfma_peak_probe(h, 2.0, C.byref(tf))
  put('mfma_peak_probe', [rc, int(tf.value > 0)])
  print('hbo_mfma_peak_probe: %.1f TFLOP/s' % tf.value)

  # ---- options ----
  publics = {'potrf_group': (3, 16, 0), 'lookahead': (0, 2, 1), 'small_nblk': (-1, 7, -1), 'pool_cap_mb': (4096, 1 << 14), 'post_chunk': (128, 65536, 8192),
             'bf16x3': (0, 5, 1), 'spectral': (1, 0), 'acq_fused': (1, 0)}
  for name, values in publics.items():
    got = []
    for v in values:
      rc = lib.hbo_set_option(h, name.encode(), v)
      o = C.c_int64(-5)
      rc2 = lib.hbo_get_option(h, name.encode(), C.byref(o))
      got += [rc, rc2, o.value]
    put(f'option/{name}', got)
  o = C.c_int64(-5)
  rc = lib.hbo_tune(h, b'lauum_bf16x3', 0); rc2 = lib.hbo_get_option(h, b'bf16x3', C.byref(o)); first = o.value
  rc3 = lib.hbo_tune(h, b'lauum_bf16x3', 1); rc4 = lib.hbo_get_option(h, b'bf16x3', C.byref(o))
  put('option/bf16x3_one_leg', [rc, rc2, first, rc3, rc4, o.value])

  # ---- argument errors: return code and hbo_last_error, none of them launches anything ----
  def error(key, rc):
    put('error/' + key, [rc], err_text())

  tasks, keep = make_tasks(((10, 1), (12, 0)), np.float64)   # m = 0: a bad task, found after the dataset object exists
  ds = C.c_void_p()
  error('dataset_create/bad_task', lib.hbo_dataset_create(h, nat.F64, D, tasks, 2, C.byref(ds)))
  tasks, keep = make_tasks(((10, 1), (12, 1)), np.float64)
  error('dataset_create/ok', lib.hbo_dataset_create(h, nat.F64, D, tasks, 2, C.byref(ds)))
  sub = C.c_void_p()
  i64 = lambda *v: np.array(v, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
  i32 = lambda *v: np.array(v, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
  error('dataset_subsample/count_too_large', lib.hbo_dataset_subsample(h, ds, i64(13, -1), i32(*range(13)), C.byref(sub)))
  error('dataset_subsample/count_zero', lib.hbo_dataset_subsample(h, ds, i64(-1, 0), i32(0), C.byref(sub)))
  error('dataset_subsample/null_idx', lib.hbo_dataset_subsample(h, ds, i64(3, -1), None, C.byref(sub)))
  error('dataset_subsample/index_out_of_range', lib.hbo_dataset_subsample(h, ds, i64(3, 2), i32(0, 1, 2, 0, 10), C.byref(sub)))
  error('dataset_subsample/negative_index', lib.hbo_dataset_subsample(h, ds, i64(-1, 2), i32(0, -1), C.byref(sub)))
  lib.hbo_dataset_free(h, ds)
  bm = built(mean.constant, kernel.squared_exponential, np.float64)
  x = rng.uniform(size=(4, D)); res = np.zeros((4, 4))
  error('gram/diag_with_x2', lib.hbo_gram(h, bm.ref(), nat.ptr(x), 4, nat.ptr(x), 4, 1, nat.ptr(res)))
  a = spd(4, np.float64); b = np.zeros((4, 129))
  error('spd_solve/m_129', lib.hbo_spd_solve(h, nat.F64, nat.ptr(a), 4, nat.ptr(b), 129, None, None, nat.ptr(np.zeros((4, 129))), None))
  error('spd_solve/n_0', lib.hbo_spd_solve(h, nat.F64, nat.ptr(a), 0, None, 0, None, None, None, None))
  error('chol_solve/bad_dtype', lib.hbo_chol_solve(h, 9, nat.ptr(a), 4, nat.ptr(b), 1, nat.ptr(b)))
  for fn in ('hbo_set_option', 'hbo_tune'):
    for name, v in (('potrf_group', 17), ('lookahead', -1), ('post_chunk', 127), ('pool_cap_mb', -1), ('spectral', 2), ('acq_fused', 2), ('gram_mfma', 4097),
                    ('sweep_free', 0), ('eig_sweeps', 1), ('no_such_option', 1)):
      error(f'{fn}/{name}', getattr(lib, fn)(h, name.encode(), v))
  o = C.c_int64(-5)
  for name in ('gram_mfma', 'poison', 'no_such_option'):
    error(f'hbo_get_option/{name}', lib.hbo_get_option(h, name.encode(), C.byref(o)))
  error('hbo_get_option/null_out', lib.hbo_get_option(h, b'lookahead', None))
  # the error paths left the pool and the context usable
  nll_fresh('after_errors/nll')
  np.savez(out_path, **out)
  print(f'{cases[0]} cases, {len(out)} arrays -> {out_path}')


def compare(a1, a2, b):
  A1, A2, B = np.load(a1), np.load(a2), np.load(b)
  if sorted(A1.files) != sorted(B.files) or sorted(A1.files) != sorted(A2.files):
    print('the files hold different arrays'); return 1
  same = lambda x, y: x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == 'f')
  noisy = [k for k in sorted(A1.files) if not same(A1[k], A2[k])]
  failed = [k for k in sorted(A1.files) if not same(A1[k], B[k])]
  nan = sum(1 for k in A1.files if A1[k].dtype.kind == 'f' and np.isnan(A1[k]).any())
  print(f'{len(A1.files)} arrays ({nan} hold NaN); the first build equals itself in {len(A1.files) - len(noisy)}, the other build equals it in {len(A1.files) - len(failed)}')
  for k in noisy:
    print('  differs between two runs of ONE build:', k)
  for k in failed:
    print('  DIFFERENT in the other build:', k)
  print('identical' if not (failed or noisy) else 'NOT identical')
  return 1 if (failed or noisy) else 0


def compare_traces(a, b):
  import collections
  import csv

  def launches(path):
    with open(path, newline='') as f:
      rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r['Dispatch_Id']))
    cols = [c for c in rows[0] if c.startswith(('Grid_Size', 'Workgroup_Size', 'LDS_Block_Size'))]
    shapes = collections.Counter((r['Kernel_Name'],) + tuple(r[c] for c in cols) for r in rows)
    queues = collections.defaultdict(list)
    for r in rows:
      queues[r['Queue_Id']].append(r['Kernel_Name'])
    return len(rows), shapes, sorted(queues.values(), key=lambda q: (-len(q), q))   # (queue ids differ from run to run: by content)
  na, sa, qa = launches(a)
  nb, sb, qb = launches(b)
  print(f'launches {na} and {nb}; distinct (kernel, grid, workgroup, LDS) {len(sa)} and {len(sb)}; queues {[len(q) for q in qa]} and {[len(q) for q in qb]}')
  ok = na == nb and sa == sb and qa == qb
  print('same launches, same shapes, same order of kernel names per queue' if ok else
        f'DIFFERENT: count {na == nb}, shapes {sa == sb}, per-queue order {qa == qb}')
  return 0 if ok else 1


if __name__ == '__main__':
  if len(sys.argv) == 3 and sys.argv[1] == 'run':
    run(sys.argv[2])
  elif len(sys.argv) == 4 and sys.argv[1] == 'compare-traces':
    sys.exit(compare_traces(*sys.argv[2:]))
  elif len(sys.argv) == 5 and sys.argv[1] == 'compare':
    sys.exit(compare(*sys.argv[2:]))
  else:
    sys.exit(__doc__)
