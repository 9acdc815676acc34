"""Translation between the reference's (mean_func, cov_func, GPParams, warp_func) and hbo_model.

Warping stays on the host (hyperbo/basics/params_utils.py:97-111): the C ABI receives already
warped values and returns gradients w.r.t. the warped values; `unflatten_grad` applies the chain
rule of the warp (what jax.grad does for the reference at hyperbo/gp_utils/gp.py:134).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from hyperbo_amd import _native as nat
from hyperbo_amd.basics import params_utils
from hyperbo_amd.gp_utils import utils as gp_utils_utils


def _mlp_layers(mlp_params):
  layers = []
  l = 0
  while f'Dense_{l}' in mlp_params:
    layers.append(mlp_params[f'Dense_{l}'])
    l += 1
  if not layers:
    raise ValueError("mlp_params must hold flax-style 'Dense_0', 'Dense_1', ... entries")
  return layers


class BuiltModel:
  """hbo_model plus the NumPy buffers it points into (kept alive here)."""

  def __init__(self, mean_func, cov_func, params, warp_func, dtype, input_dim, eps=1e-6):
    kernel_id = getattr(cov_func, 'kernel_id', None)
    mean_id = getattr(mean_func, 'mean_id', None)
    if kernel_id is None:
      raise TypeError(f'cov_func {cov_func!r} is not one of hyperbo_amd.gp_utils.kernel (closed registry '
                      'hyperbo/bo_utils/const.py:29-35); arbitrary Python pair-kernels cannot run natively')
    if mean_id is None:
      raise TypeError(f'mean_func {mean_func!r} is not one of hyperbo_amd.gp_utils.mean')
    self.dtype = np.dtype(dtype)
    self.code = nat.dtype_code(self.dtype)
    self.uses_mlp_kernel = bool(getattr(cov_func, 'uses_mlp', False))
    self.uses_kumar = bool(getattr(cov_func, 'uses_kumar', False))
    self.kernel_id, self.mean_id = kernel_id, mean_id
    self.warp_func = warp_func
    self.params = params
    self._keep = []
    m = nat.Model()
    m.kernel_id, m.mean_id, m.dtype, m.input_dim = kernel_id, mean_id, self.code, int(input_dim)
    m.kernel_uses_mlp = int(self.uses_mlp_kernel)
    m.eps = float(eps)
    need_mlp = self.uses_mlp_kernel or mean_id == nat.MEAN_LINEAR_MLP
    retrieve = lambda keys: params_utils.retrieve_params(params, keys, warp_func)

    def arr(v):
      a = np.ascontiguousarray(np.asarray(v), dtype=self.dtype)
      self._keep.append(a)
      return a

    feat_dim = int(input_dim)
    if need_mlp:
      mlp_params, = retrieve(['mlp_params'])
      layers = _mlp_layers(mlp_params)
      if len(layers) > nat.MAX_MLP_LAYERS:
        raise ValueError('too many MLP layers')
      m.n_layers = len(layers)
      fin = int(input_dim)
      for l, layer in enumerate(layers):
        w = arr(layer['kernel'])
        b = arr(np.reshape(layer['bias'], (-1,)))
        if w.shape[0] != fin or b.shape[0] != w.shape[1]:
          raise ValueError(f'mlp layer {l}: kernel {w.shape} / bias {b.shape} do not chain from {fin}')
        m.features[l] = w.shape[1]
        m.mlp_kernel[l] = nat.ptr(w).value
        m.mlp_bias[l] = nat.ptr(b).value
        fin = w.shape[1]
      self.mlp_shapes = [(np.shape(l['kernel']), np.shape(l['bias'])) for l in layers]
      if self.uses_mlp_kernel:
        feat_dim = fin
      self.mlp_out = fin
    else:
      self.mlp_shapes = []
      self.mlp_out = 0
    self.feat_dim = feat_dim

    noise, = retrieve(['noise_variance'])
    m.noise_variance = float(np.squeeze(noise))
    if kernel_id == nat.KERNEL_DOT:
      sigma, bias = retrieve(['dot_prod_sigma', 'dot_prod_bias'])
      m.dot_prod_sigma = float(np.squeeze(sigma))
      m.dot_prod_bias = float(np.squeeze(bias))
      m.n_lengthscale = 0
    else:
      ls, sv = retrieve(['lengthscale', 'signal_variance'])
      ls = arr(np.reshape(ls, (-1,)))
      if ls.size not in (1, feat_dim):
        raise ValueError(f'lengthscale has {ls.size} entries, expected 1 or {feat_dim}')
      m.lengthscale = nat.ptr(ls).value
      m.n_lengthscale = ls.size
      m.signal_variance = float(np.squeeze(sv))
    if mean_id == nat.MEAN_CONSTANT:
      const, = retrieve(['constant'])
      m.constant = float(np.squeeze(const))
    if mean_id in (nat.MEAN_LINEAR, nat.MEAN_LINEAR_MLP):
      lm, = retrieve(['linear_mean'])
      w = arr(np.reshape(lm['kernel'], (-1,)))
      fin = int(input_dim) if mean_id == nat.MEAN_LINEAR else self.mlp_out
      if w.size != fin:
        raise ValueError(f'linear_mean kernel has {w.size} entries, expected {fin}')
      m.linear_kernel = nat.ptr(w).value
      m.linear_bias = float(np.squeeze(lm['bias']))
    self.kumar_raw = None
    if self.uses_kumar:
      # hyperbo/gp_utils/kernel.py:190-217: KumarWarp applies squareplus to kumar_params itself (warp_func never touches them)
      if 'kumar_params' not in params.model:
        raise ValueError(f'{getattr(cov_func, "__name__", cov_func)} is a Kumaraswamy kernel but params.model has no '
                         "'kumar_params'; create them with kernel.init_kumar_warp_with_shape(key, params, input_shape)")
      kp = params.model['kumar_params']
      a_raw = np.reshape(np.asarray(kp['a'], dtype=np.float64), (-1,))
      b_raw = np.reshape(np.asarray(kp['b'], dtype=np.float64), (-1,))
      if a_raw.size != int(input_dim) or b_raw.size != int(input_dim):
        raise ValueError(f"kumar_params 'a' / 'b' have {a_raw.size} / {b_raw.size} entries, expected {int(input_dim)}")
      self.kumar_raw = (a_raw, b_raw)
      ka, kb = arr(gp_utils_utils.squareplus_warp(a_raw)), arr(gp_utils_utils.squareplus_warp(b_raw))
      m.input_warp = nat.WARP_KUMAR
      self.kstruct = nat.ModelKumar()
      self.kstruct.base = m
      self.kstruct.kumar_a = nat.ptr(ka).value
      self.kstruct.kumar_b = nat.ptr(kb).value
      m = self.kstruct.base   # (a view into kstruct: one struct, the one the library reads)
    self.struct = m
    self.layout = nat.GradLayout()
    rc = nat.lib().hbo_grad_layout_of(self.ref(), C.byref(self.layout))
    if rc != nat.HBO_OK:
      raise nat.HboError(rc, 'hbo_grad_layout_of: ' + (nat.lib().hbo_last_error(None) or b'').decode())
    if self.uses_kumar:
      ao, bo = C.c_int32(-1), C.c_int32(-1)
      nat.lib().hbo_grad_layout_kumar_of(self.ref(), C.byref(ao), C.byref(bo))
      self.kumar_offsets = (ao.value, bo.value)

  def ref(self):
    if self.uses_kumar:
      return C.cast(C.pointer(self.kstruct), C.POINTER(nat.Model))
    return C.byref(self.struct)

  # -- gradient pytree -----------------------------------------------------------------
  def unflatten_grad(self, flat):
    """flat d/d(warped) -> pytree shaped like params.model with d/d(raw) (warp chain rule)."""
    model = self.params.model
    lay = self.layout
    wf = self.warp_func or {}

    def chain(key, g):
      raw = np.asarray(model[key], dtype=np.float64)
      g = np.reshape(np.asarray(g, dtype=np.float64), raw.shape) if np.size(g) == raw.size else \
          np.full(raw.shape, np.sum(g))
      if key in wf:
        g = g * gp_utils_utils.warp_derivative(wf[key], raw)
      return g

    def zeros_like_tree(t):
      if isinstance(t, dict):
        return {k: zeros_like_tree(v) for k, v in t.items()}
      return np.zeros(np.shape(t), dtype=np.float64)

    grads = zeros_like_tree(model)
    if lay.lengthscale >= 0 and 'lengthscale' in model:
      n_ls = self.struct.n_lengthscale
      grads['lengthscale'] = chain('lengthscale', flat[lay.lengthscale:lay.lengthscale + n_ls])
    for key, off in (('signal_variance', lay.signal_variance), ('noise_variance', lay.noise_variance),
                     ('constant', lay.constant), ('dot_prod_sigma', lay.dot_prod_sigma),
                     ('dot_prod_bias', lay.dot_prod_bias)):
      if off >= 0 and key in model:
        grads[key] = chain(key, flat[off:off + 1])
    if lay.linear_kernel >= 0:
      lm = model['linear_mean']
      fin = np.size(lm['kernel'])
      grads['linear_mean'] = {
          'kernel': np.reshape(flat[lay.linear_kernel:lay.linear_kernel + fin], np.shape(lm['kernel'])),
          'bias': np.reshape(flat[lay.linear_bias:lay.linear_bias + 1], np.shape(lm['bias'])),
      }
    if self.mlp_shapes and 'mlp_params' in model:
      g = {}
      for l, (wshape, bshape) in enumerate(self.mlp_shapes):
        wo, bo = lay.mlp_kernel[l], lay.mlp_bias[l]
        g[f'Dense_{l}'] = {
            'kernel': np.reshape(flat[wo:wo + int(np.prod(wshape))], wshape),
            'bias': np.reshape(flat[bo:bo + int(np.prod(bshape))], bshape),
        }
      grads['mlp_params'] = g
    if self.uses_kumar and 'kumar_params' in model:
      # d/d squareplus(raw) -> d/d raw (squareplus'(t) = (1 + t / sqrt(t^2 + 4)) / 2), shaped like the raw leaves
      kp = model['kumar_params']
      ao, bo = self.kumar_offsets
      d = self.kumar_raw[0].size
      sp = lambda t: gp_utils_utils.warp_derivative(gp_utils_utils.squareplus_warp, t)
      grads['kumar_params'] = {
          'a': np.reshape(np.asarray(flat[ao:ao + d], dtype=np.float64) * sp(self.kumar_raw[0]), np.shape(kp['a'])),
          'b': np.reshape(np.asarray(flat[bo:bo + d], dtype=np.float64) * sp(self.kumar_raw[1]), np.shape(kp['b'])),
      }
    return grads


_TRAIN_WARPS = ((gp_utils_utils.identity_warp, nat.TRAIN_WARP_IDENTITY), (gp_utils_utils.softplus_warp, nat.TRAIN_WARP_SOFTPLUS),
                (gp_utils_utils.DEFAULT_SOFTPLUS, nat.TRAIN_WARP_SOFTPLUS_EPS), (gp_utils_utils.squareplus_warp, nat.TRAIN_WARP_SQUAREPLUS))


def train_warp_code(fn):
  """hbo_train_warp of a warp function of the closed set, None for any other callable."""
  for f, code in _TRAIN_WARPS:
    if fn is f:
      return code
  return None


def train_leaf_map(bm, model):
  """hbo_train_leaf of every element of lbfgs.tree_flatten(model) (sorted keys, row-major leaves), for the model family of `bm` (a
  BuiltModel of `model`): which field of hbo_model the element becomes, through which warp -- what BuiltModel reads (warped values)
  and what its unflatten_grad chains.  A leaf the model does not read gets HBO_TRAIN_NONE.  Raises ValueError for a warp outside
  the closed set on a leaf the model reads."""
  lay = bm.layout
  wf = bm.warp_func or {}
  scalar_targets = {'signal_variance': (nat.TRAIN_SIGNAL_VARIANCE, lay.signal_variance),
                    'noise_variance': (nat.TRAIN_NOISE_VARIANCE, lay.noise_variance),
                    'constant': (nat.TRAIN_CONSTANT, lay.constant),
                    'dot_prod_sigma': (nat.TRAIN_DOT_PROD_SIGMA, lay.dot_prod_sigma),
                    'dot_prod_bias': (nat.TRAIN_DOT_PROD_BIAS, lay.dot_prod_bias)}
  rows = []

  def warp_of(key):
    if key not in wf:
      return nat.TRAIN_WARP_IDENTITY
    code = train_warp_code(wf[key])
    if code is None:
      raise ValueError(f"adam_on_device: warp_func['{key}'] = {wf[key]!r} is outside the closed set (identity, softplus, "
                       'DEFAULT_SOFTPLUS, squareplus)')
    return code

  def emit(leaf, target, warp=nat.TRAIN_WARP_IDENTITY, layer=0):
    a = np.asarray(leaf)
    f32 = int(a.dtype == np.float32)
    for i in range(a.size):
      rows.append((warp, target, layer, i, f32) if target != nat.TRAIN_NONE else (nat.TRAIN_WARP_IDENTITY, nat.TRAIN_NONE, 0, 0, f32))

  def rec_none(t):
    if isinstance(t, dict):
      for k in sorted(t):
        rec_none(t[k])
    else:
      emit(t, nat.TRAIN_NONE)

  for key in sorted(model):
    val = model[key]
    if key == 'lengthscale' and lay.lengthscale >= 0:
      emit(val, nat.TRAIN_LENGTHSCALE, warp_of(key))
    elif key in scalar_targets and scalar_targets[key][1] >= 0:
      emit(val, scalar_targets[key][0], warp_of(key))
    elif key == 'linear_mean' and lay.linear_kernel >= 0:
      for sub in sorted(val):
        emit(val[sub], nat.TRAIN_LINEAR_BIAS if sub == 'bias' else nat.TRAIN_LINEAR_KERNEL if sub == 'kernel' else nat.TRAIN_NONE)
    elif key == 'mlp_params' and bm.mlp_shapes:
      for name in sorted(val):
        layer = int(name[len('Dense_'):]) if name.startswith('Dense_') and name[len('Dense_'):].isdigit() else -1
        if not 0 <= layer < len(bm.mlp_shapes):
          rec_none(val[name])
          continue
        for sub in sorted(val[name]):
          tgt = nat.TRAIN_MLP_BIAS if sub == 'bias' else nat.TRAIN_MLP_KERNEL if sub == 'kernel' else nat.TRAIN_NONE
          emit(val[name][sub], tgt, layer=layer)
    elif key == 'kumar_params' and bm.uses_kumar:
      for sub in sorted(val):
        tgt = nat.TRAIN_KUMAR_A if sub == 'a' else nat.TRAIN_KUMAR_B if sub == 'b' else nat.TRAIN_NONE
        emit(val[sub], tgt, nat.TRAIN_WARP_SQUAREPLUS)
    else:
      rec_none(val)
  leaves = (nat.TrainLeaf * max(len(rows), 1))()
  for i, r in enumerate(rows):
    leaves[i].warp, leaves[i].target, leaves[i].layer, leaves[i].index, leaves[i].round_f32 = r
  return leaves, len(rows)


def infer_dtype(*arrays):
  """Computation dtype for the given inputs, following JAX's promotion under JAX_ENABLE_X64: float32 only when every
  FLOATING input is float32; any float64 input -- and integer / bool / list inputs, which x64 JAX widens -- gives
  float64 (mixed float32 / float64 inputs are promoted, never silently narrowed)."""
  saw32 = False
  for a in arrays:
    if a is None:
      continue
    dt = np.asarray(a).dtype
    if dt == np.float32 or dt == np.float16:
      saw32 = True
    elif np.issubdtype(dt, np.integer) or dt == np.bool_:
      continue   # JAX: int + float32 -> float32, int alone -> float64 under x64
    else:
      return np.dtype(np.float64)
  return np.dtype(np.float32) if saw32 else np.dtype(np.float64)


def infer_input_dim(mean_func, cov_func, params):
  """Input dimension D implied by the parameters alone (first MLP layer, linear mean, ARD lengthscale), or None.
  Used where no data is at hand: a rank whose task shard is empty must still build the same model as its peers."""
  model = params.model
  uses_mlp = bool(getattr(cov_func, 'uses_mlp', False)) or getattr(mean_func, 'mean_id', None) == nat.MEAN_LINEAR_MLP
  if uses_mlp and isinstance(model.get('mlp_params'), dict) and 'Dense_0' in model['mlp_params']:
    return int(np.shape(model['mlp_params']['Dense_0']['kernel'])[0])
  if getattr(mean_func, 'mean_id', None) == nat.MEAN_LINEAR and isinstance(model.get('linear_mean'), dict):
    return int(np.size(model['linear_mean']['kernel']))
  if getattr(cov_func, 'kernel_id', None) != nat.KERNEL_DOT and 'lengthscale' in model and np.size(model['lengthscale']) > 1:
    return int(np.size(model['lengthscale']))
  return None
