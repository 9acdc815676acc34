"""Shared builders for the oracle / native parameter containers used by the tests."""
import numpy as np

KERNELS = ['squared_exponential', 'matern32', 'matern52', 'dot_product']
MEANS = ['zero', 'constant', 'linear', 'linear_mlp']
MLP_FEATURES = (4, 5)


def inv_softplus(v):
  return np.log(np.expm1(np.asarray(v, dtype=np.float64)))


def make_model(rng, mean_name, mlp_kernel, d, dtype=np.float64):
  """Raw (un-warped) params.model with every key the given mean/kernel combination needs."""
  feat = MLP_FEATURES[-1] if mlp_kernel else d
  model = {
      'lengthscale': (rng.normal(size=feat) * 0.3 + 0.5).astype(dtype),
      'signal_variance': np.array(0.3, dtype=dtype),
      'noise_variance': np.array(-2.0, dtype=dtype),
      'constant': np.array(0.4, dtype=dtype),
      'dot_prod_sigma': np.array(0.7, dtype=dtype),
      'dot_prod_bias': np.array(0.2, dtype=dtype),
  }
  if mlp_kernel or mean_name == 'linear_mlp':
    fin = d
    mlp = {}
    for l, f in enumerate(MLP_FEATURES):
      mlp[f'Dense_{l}'] = {'kernel': (rng.normal(size=(fin, f)) * 0.7).astype(dtype),
                           'bias': (rng.normal(size=f) * 0.1).astype(dtype)}
      fin = f
    model['mlp_params'] = mlp
  if mean_name in ('linear', 'linear_mlp'):
    fin = MLP_FEATURES[-1] if mean_name == 'linear_mlp' else d
    model['linear_mean'] = {'kernel': rng.normal(size=(fin, 1)).astype(dtype),
                            'bias': rng.normal(size=1).astype(dtype)}
  return model


def lengthscale(rng, fdim, ls):
  """Raw length-scales.  ARD: fdim length-scales around 0.5 sqrt(fdim) (a Gram matrix that neither decays to the diagonal nor fills
  with ones on inputs in [0, 1]^fdim or on tanh features), each its own; scalar: one length-scale (the n_ls == 1 sums)."""
  return inv_softplus(0.5 * np.sqrt(fdim) * np.exp(rng.uniform(-0.4, 0.4, size=(fdim if ls == 'ard' else 1))))


def mlp_model(rng, d, feats, kname, ls):
  """Raw params.model of a kernel on the MLP basis d -> feats under a linear_mlp mean (signal variance 0.8, noise 0.1)."""
  flast = feats[-1]
  model = {'signal_variance': inv_softplus(0.8), 'noise_variance': inv_softplus(0.1),
           'linear_mean': {'kernel': rng.normal(size=(flast, 1)) / np.sqrt(flast), 'bias': rng.normal(size=1)}, 'mlp_params': {}}
  if kname == 'dot_product':
    model['dot_prod_sigma'] = inv_softplus(0.5 * np.sqrt(flast))
    model['dot_prod_bias'] = np.array(0.2)
  else:
    model['lengthscale'] = lengthscale(rng, flast, ls)
  fin = d
  for l, f in enumerate(feats):
    model['mlp_params'][f'Dense_{l}'] = {'kernel': rng.normal(size=(fin, f)) * (2.0 / np.sqrt(fin)), 'bias': rng.normal(size=f) * 0.1}
    fin = f
  return model


def flatten(tree):
  out = []
  def rec(t):
    if isinstance(t, dict):
      for k in sorted(t):
        rec(t[k])
    else:
      out.append(np.asarray(t, dtype=np.float64).ravel())
  rec(tree)
  return np.concatenate(out) if out else np.zeros(0)


def unflatten_like(tree, vec):
  pos = [0]
  def rec(t):
    if isinstance(t, dict):
      return {k: rec(t[k]) for k in sorted(t)}
    a = np.asarray(t, dtype=np.float64)
    v = vec[pos[0]:pos[0] + a.size].reshape(a.shape)
    pos[0] += a.size
    return v
  return rec(tree)


def tree_leaves(tree, prefix=''):
  """(path, float64 array) of every leaf, in flatten()'s order."""
  if isinstance(tree, dict):
    for k in sorted(tree):
      yield from tree_leaves(tree[k], prefix + '/' + str(k) if prefix else str(k))
  else:
    yield prefix, np.asarray(tree, dtype=np.float64)


def grad_leaf_errors(got, ref):
  """Per leaf: (path, max |got - ref|, ||ref leaf||_inf).  Either side may be a flat vector in flatten()'s order."""
  if not isinstance(ref, dict) and isinstance(got, dict):
    ref = unflatten_like(got, np.asarray(ref, dtype=np.float64).ravel())
  if not isinstance(got, dict) and isinstance(ref, dict):
    got = unflatten_like(ref, np.asarray(got, dtype=np.float64).ravel())
  if not isinstance(ref, dict):
    got, ref = {'flat': got}, {'flat': ref}
  gl, rl = dict(tree_leaves(got)), dict(tree_leaves(ref))
  assert set(gl) == set(rl), (sorted(gl), sorted(rl))
  out = []
  for path, r in rl.items():
    g = gl[path]
    assert g.size == r.size, (path, g.shape, r.shape)
    out.append((path, float(np.max(np.abs(g.ravel() - r.ravel()))) if r.size else 0.0, float(np.max(np.abs(r))) if r.size else 0.0))
  return out


def assert_grad_close(got, ref, tol, floor_rel=1e-3, label='', leaf_scales=None):
  """PER-LEAF gradient check: every leaf L must satisfy max|got_L - ref_L| <= tol * max(||ref_L||_inf, floor_rel * max|ref|).
  (A bound relative to the largest entry of the FLATTENED tree lets a wrong leaf that is 1e4 x smaller than the lengthscale
  gradient pass; the floor keeps leaves that are zero by cancellation testable: their error scales with the un-cancelled terms.)
  leaf_scales: path -> the scale of a leaf's un-cancelled terms, from the reference (tests/mlp_cases.py); the floor of such a leaf is
  min(floor_rel * max|ref|, that scale) -- a leaf whose terms themselves are smaller than the floor is held to its terms.
  The failure message names the worst leaf; with HBO_GRAD_LOG=<file> every call appends its worst ratio (tolerance audits)."""
  errs = grad_leaf_errors(got, ref)
  gmax = max((n for _, _, n in errs), default=0.0)
  worst = (0.0, '', 0.0, 0.0)
  for path, err, norm in errs:
    if not np.isfinite(err):
      raise AssertionError(f'{label}: leaf {path} is not finite')
    floor = floor_rel * gmax
    if leaf_scales is not None and path in leaf_scales:
      floor = min(floor, leaf_scales[path])
    bound = tol * max(norm, floor, 1e-300)
    if err / bound > worst[0]:
      worst = (err / bound, path, err, norm)
  import os
  log = os.environ.get('HBO_GRAD_LOG')
  if log:
    with open(log, 'a') as f:
      test = os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0]
      f.write(f'{worst[0]:.3e} tol={tol:g} leaf={worst[1]} err={worst[2]:.3e} norm={worst[3]:.3e} gmax={gmax:.3e} {label} {test}\n')
  assert worst[0] <= 1.0, (f'{label}: worst leaf {worst[1]}: |err| {worst[2]:.3e} = {worst[0]:.2f} x the bound '
                           f'(tol {tol:g}, leaf norm {worst[3]:.3e}, max|g| {gmax:.3e})')


def rel_err(a, b):
  a = np.asarray(a, dtype=np.float64)
  b = np.asarray(b, dtype=np.float64)
  return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-300)) if a.size else 0.0


_TORCH_PROCESS = None


def in_torch_process(fn, *args):
  """fn(*args) in a spawned child process (one, reused), its exception raised here; skips when torch is not installed.  The
  tests that use torch go through this: torch-ROCm loads its own HIP runtime and librccl.so, and in one process with libhbo
  either libhbo's dlopen("librccl.so") returns torch's RCCL (ncclCommInitRank fails) or, with libhbo's RCCL loaded first,
  the process aborts at exit (double free between the two runtimes)."""
  import concurrent.futures
  import importlib.util
  import multiprocessing
  import pytest
  global _TORCH_PROCESS
  if importlib.util.find_spec('torch') is None:
    pytest.skip('torch is not installed')
  if _TORCH_PROCESS is None:
    _TORCH_PROCESS = concurrent.futures.ProcessPoolExecutor(max_workers=1, mp_context=multiprocessing.get_context('spawn'))
  return _TORCH_PROCESS.submit(fn, *args).result()


def synthetic_task(rng, n, d, m=1, dtype=np.float64):
  x = rng.uniform(size=(n, d))
  w = rng.normal(size=(d, m))
  y = np.sin(2 * np.pi * x @ w) + 0.1 * rng.normal(size=(n, m))
  return x.astype(dtype), y.astype(dtype)


class TorchDistComm:
  """Test-only communicator: torch.distributed all_reduce (gloo, world_size 2 on CPU) behind the `allreduce_sum` interface of
  hyperbo_amd.parallel's communicators.  Lives here, not in the package: the product path is torch-free."""

  def __init__(self, device=None, group=None):
    import torch.distributed as dist
    if not dist.is_initialized():
      raise RuntimeError('torch.distributed is not initialised')
    self._dist = dist
    self.rank, self.world_size = dist.get_rank(), dist.get_world_size()
    self.device = device
    self.group = group

  def allreduce_sum(self, buf):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(buf, dtype=np.float64).copy())
    if self.device is not None:
      t = t.to(self.device)
    self._dist.all_reduce(t, op=self._dist.ReduceOp.SUM, group=self.group)
    return t.cpu().numpy()
