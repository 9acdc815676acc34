"""Model families and datasets shared by the tests of config['adam_on_device'] (hbo_train_adam): test_train_device_host.py (CPU)
and test_gpu_train_device.py (GPU)."""
import numpy as np

D = 4
FEATS = (6, 5)


def model_of(kernel_name, mean_name, d=D, feats=FEATS, seed=0, dtype=np.float64):
  """params.model for one kernel x mean of the closed registry, DEFAULT_WARP_FUNC-style raw values.  Beyond 16 features the
  length-scales grow with sqrt(features / 16), so that the covariance of a wide feature space does not decay to the diagonal."""
  rng = np.random.default_rng(seed)
  mlp = kernel_name.endswith('_mlp') or mean_name == 'linear_mlp'
  kumar = kernel_name.endswith('_kumar')
  fdim = feats[-1] if kernel_name.endswith('_mlp') else d
  m = {'noise_variance': np.array(-2.0, dtype=dtype), 'signal_variance': np.array(0.2, dtype=dtype)}
  if kernel_name.startswith('dot_product'):
    m['dot_prod_sigma'] = np.array(-0.5, dtype=dtype)
    m['dot_prod_bias'] = np.array(0.3, dtype=dtype)
  else:
    ls = rng.uniform(-0.5, 0.5, size=fdim)
    if fdim > 16:
      ls = np.log(np.expm1(np.log1p(np.exp(ls)) * np.sqrt(fdim / 16)))
    m['lengthscale'] = ls.astype(dtype)
  if mean_name == 'constant':
    m['constant'] = np.array(0.1, dtype=dtype)
  if mlp:
    m['mlp_params'] = {}
    fin = d
    for l, f in enumerate(feats):
      m['mlp_params'][f'Dense_{l}'] = {'kernel': (rng.normal(size=(fin, f)) / np.sqrt(fin)).astype(dtype),
                                       'bias': (0.1 * rng.normal(size=(f,))).astype(dtype)}
      fin = f
  if mean_name in ('linear', 'linear_mlp'):
    fin = feats[-1] if mean_name == 'linear_mlp' else d
    m['linear_mean'] = {'kernel': (rng.normal(size=(fin, 1)) / np.sqrt(fin)).astype(dtype), 'bias': np.array([0.05], dtype=dtype)}
  if kumar:
    m['kumar_params'] = {'a': (0.3 * rng.normal(size=(d,))).astype(dtype), 'b': (0.3 * rng.normal(size=(d,))).astype(dtype)}
  return m


def funcs(kernel_name, mean_name):
  from hyperbo_amd.gp_utils import kernel, mean
  return getattr(mean, mean_name), getattr(kernel, kernel_name)


FAMILIES = [(k, mu) for k in ('squared_exponential', 'matern32', 'matern52', 'dot_product')
            for mu in ('zero', 'constant', 'linear')] + \
           [(k + '_mlp', mu) for k in ('squared_exponential', 'matern52', 'dot_product') for mu in ('constant', 'linear_mlp')] + \
           [('matern32_mlp', 'linear_mlp'), ('squared_exponential', 'linear_mlp'),
            ('squared_exponential_kumar', 'constant'), ('matern52_kumar', 'linear')]

# (kernel, mean, input dim, MLP features): feature spaces wider than the 16-feature chunk of the single-workgroup evaluation
# (small.hip), which every step of the device loop runs.  GPU tier only.
WIDE_FAMILIES = [('matern52', 'linear', 33, FEATS), ('squared_exponential_mlp', 'linear_mlp', D, (6, 33))]


def dataset(sizes, d=D, dtype=np.float64, seed=1):
  from hyperbo_amd.basics import definitions as defs
  rng = np.random.default_rng(seed)
  out = {}
  for i, n in enumerate(sizes):
    x = rng.uniform(size=(n, d)); w = rng.normal(size=(d, 1))
    y = np.sin(2 * np.pi * x @ w) + 0.1 * rng.normal(size=(n, 1))
    out[i] = defs.SubDataset(x.astype(dtype), y.astype(dtype))
  return out
