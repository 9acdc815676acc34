"""The mixed batches that every batched entry point (hbo_acq_samples, hbo_nll_samples, hbo_acq_grad_samples, hbo_acq_maximize,
hbo_bo_simulated) refuses through the one check they share (csrc/api_internal.h: model_family_check), per sample in the order
input warp -> validate_model -> family.  Each case is a pair of models, the code expected and a word its message must hold
('{fn}' stands for the name of the entry point).  Used by test_gpu_family_check.py (all five, with a context) and by
test_bo_device_host.py (hbo_bo_simulated, whose checks run before the context is touched)."""
import numpy as np

from hyperbo_amd import _native as nat

D = 2


def _base(ls):
  m = nat.Model()
  m.kernel_id, m.mean_id, m.dtype, m.input_dim, m.n_lengthscale = nat.KERNEL_SE, nat.MEAN_CONSTANT, nat.F64, D, D
  m.lengthscale, m.signal_variance, m.noise_variance, m.eps = nat.ptr(ls).value, 1.0, 0.1, 1e-6
  return m


def _other_cov(m0, m1):
  m1.kernel_id = nat.KERNEL_MATERN32


def _warped(m0, m1):   # (a packed array element: no hbo_model_kumar tail behind it, so the check must not look for one)
  m1.input_warp = nat.WARP_KUMAR


def _invalid(m0, m1):   # an MLP basis without layers: validate_model's 'bad n_layers'
  m1.kernel_uses_mlp, m1.n_layers = 1, 0


def _invalid_then_warped(m0, m1):   # the order is per sample: the invalid model at index 0 is reported, not the warp at index 1
  m0.kernel_uses_mlp, m0.n_layers = 1, 0
  m1.input_warp = nat.WARP_KUMAR


CASES = {
    'other_covariance': (_other_cov, nat.HBO_ERR_ARG, 'must share'),
    'warped': (_warped, nat.HBO_ERR_UNSUPPORTED, '{fn}'),
    'invalid': (_invalid, nat.HBO_ERR_ARG, 'bad n_layers'),
    'invalid_then_warped': (_invalid_then_warped, nat.HBO_ERR_ARG, 'bad n_layers'),
}


def good_model():
  """(model, keep): a valid model of the family; `keep` holds the arrays it points to."""
  ls = np.ones(D)
  return _base(ls), ls


def pair(name):
  """(models, keep, code, word): the two models of case `name` as a packed array."""
  edit, code, word = CASES[name]
  ls = np.ones(D)
  models = (nat.Model * 2)(_base(ls), _base(ls))
  edit(models[0], models[1])
  return models, ls, code, word
