"""ctypes binding of libhbo.so (C ABI declared in include/hbo.h).

There is deliberately NO CPU fallback: if the shared library is missing or no GPU is visible
the calls raise.  (`python -c "import __graft_entry__ as g; g.build()"` builds the library.)
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

HBO_OK, HBO_ERR_ARG, HBO_ERR_HIP, HBO_ERR_NODEV, HBO_ERR_UNSUPPORTED, HBO_ERR_COMM = 0, -1, -2, -3, -4, -5
HBO_NOT_PD = 1
HBO_NOT_CONVERGED = 2
KERNEL_SE, KERNEL_MATERN32, KERNEL_MATERN52, KERNEL_DOT = 0, 1, 2, 3
MEAN_ZERO, MEAN_CONSTANT, MEAN_LINEAR, MEAN_LINEAR_MLP = 0, 1, 2, 3
F32, F64 = 0, 1
WARP_NONE, WARP_KUMAR = 0, 1
ACQ_EI, ACQ_PI, ACQ_UCB = 0, 1, 2
MES_MAX_K = 256   # HBO_MES_MAX_K
QEI_MAX_Q, QEI_MAX_BASE = 16, 1024   # HBO_QEI_MAX_Q, HBO_QEI_MAX_BASE
BO_PARAM_CONST, BO_PARAM_MAX_PLUS, BO_PARAM_MAX_PLUS_STD = 0, 1, 2
MAX_MLP_LAYERS = 8
MAX_FEATURE_DIM = 256
MAX_PROFILE_STAGES = 32
UNIQUE_ID_BYTES = 128

# ($HBO_LIB: another build of the same library, for the A/B tools under tools/)
_LIB_PATH = os.environ.get('HBO_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libhbo.so')


class HboError(RuntimeError):
  def __init__(self, code, msg):
    super().__init__(f'libhbo error {code}: {msg}')
    self.code = code


class Model(C.Structure):
  _fields_ = [
      ('kernel_id', C.c_int32), ('mean_id', C.c_int32), ('dtype', C.c_int32), ('input_dim', C.c_int32),
      ('kernel_uses_mlp', C.c_int32), ('n_layers', C.c_int32), ('features', C.c_int32 * MAX_MLP_LAYERS),
      ('n_lengthscale', C.c_int32), ('input_warp', C.c_int32),
      ('eps', C.c_double), ('signal_variance', C.c_double), ('noise_variance', C.c_double),
      ('constant', C.c_double), ('dot_prod_sigma', C.c_double), ('dot_prod_bias', C.c_double),
      ('linear_bias', C.c_double),
      ('lengthscale', C.c_void_p),
      ('mlp_kernel', C.c_void_p * MAX_MLP_LAYERS), ('mlp_bias', C.c_void_p * MAX_MLP_LAYERS),
      ('linear_kernel', C.c_void_p),
  ]


class ModelKumar(C.Structure):
  """hbo_model_kumar: an hbo_model with input_warp = WARP_KUMAR followed by the squareplus-warped a, b ([input_dim] each)."""
  _fields_ = [('base', Model), ('kumar_a', C.c_void_p), ('kumar_b', C.c_void_p)]


class GradLayout(C.Structure):
  _fields_ = [
      ('lengthscale', C.c_int32), ('signal_variance', C.c_int32), ('noise_variance', C.c_int32),
      ('constant', C.c_int32), ('dot_prod_sigma', C.c_int32), ('dot_prod_bias', C.c_int32),
      ('linear_kernel', C.c_int32), ('linear_bias', C.c_int32),
      ('mlp_kernel', C.c_int32 * MAX_MLP_LAYERS), ('mlp_bias', C.c_int32 * MAX_MLP_LAYERS),
      ('total', C.c_int32),
  ]


class Task(C.Structure):
  _fields_ = [('x', C.c_void_p), ('y', C.c_void_p), ('n', C.c_int64), ('m', C.c_int32),
              ('reserved0', C.c_int32)]


class BoRun(C.Structure):
  """hbo_bo_run: one run of hbo_bo_simulated (candidate pool, initial observations, acquisition and its per-iteration parameter)."""
  _fields_ = [('xc', C.c_void_p), ('yc', C.c_void_p), ('M', C.c_int64), ('x0', C.c_void_p), ('y0', C.c_void_p), ('n0', C.c_int64),
              ('acq_id', C.c_int32), ('param_mode', C.c_int32), ('param', C.c_double),
              ('add_noise', C.c_double), ('scale0', C.c_double), ('scale', C.c_double)]


class TrainLeaf(C.Structure):
  """hbo_train_leaf: how one element of the flat raw vector becomes a field of the model (hbo_train_adam)."""
  _fields_ = [('warp', C.c_int32), ('target', C.c_int32), ('layer', C.c_int32), ('index', C.c_int32), ('round_f32', C.c_int32)]


class LbfgsOpts(C.Structure):
  """hbo_lbfgs_opts: the arguments of lbfgs.lbfgs and its line search (hbo_train_lbfgs)."""
  _fields_ = [('memory', C.c_int32), ('ls_steps', C.c_int32), ('max_iters', C.c_int32), ('alpha', C.c_double), ('tol', C.c_double),
              ('c1', C.c_double), ('c2', C.c_double), ('grow', C.c_double), ('tau', C.c_double)]


class LbfgsEval(C.Structure):
  """hbo_lbfgs_eval: one evaluation of the log of hbo_train_lbfgs."""
  _fields_ = [('kind', C.c_int32), ('iter', C.c_int32), ('alpha', C.c_double), ('value', C.c_double)]


# hbo_lbfgs_kind / hbo_lbfgs_status
LBFGS_START, LBFGS_MAIN, LBFGS_LINE_SEARCH, LBFGS_IDLE = 0, 1, 2, 3
(LBFGS_RUNNING, LBFGS_CONVERGED_AT_START, LBFGS_CONVERGED, LBFGS_NO_PROGRESS, LBFGS_INSTABILITY, LBFGS_STEPS_DONE) = range(6)

class AcqOptOpts(C.Structure):
  """hbo_acq_opt_opts: the options of the projected L-BFGS of hbo_acq_maximize."""
  _fields_ = [('memory', C.c_int32), ('ls_steps', C.c_int32), ('max_iters', C.c_int32), ('c1', C.c_double), ('tau', C.c_double),
              ('pgtol', C.c_double), ('ftol', C.c_double)]


class AcqOptEval(C.Structure):
  """hbo_acq_opt_eval: one record of the log of hbo_acq_maximize."""
  _fields_ = [('kind', C.c_int32), ('iter', C.c_int32), ('alpha', C.c_double), ('value', C.c_double)]


class ProbePlan(C.Structure):
  """hbo_probe_plan (include/hbo_tune.h): what the test hook hbo_probe_factor_inverse planned."""
  _fields_ = [(k, C.c_int32) for k in ('la', 'q', 'q_inner', 'early_at', 'tgran', 'split_f1', 'yield_', 'sweep', 'qs', 'early',
                                       'small_shape', 'batch_bg', 'd_own_stream')]

  def as_dict(self):
    return {k.rstrip('_'): int(getattr(self, k)) for k, _ in self._fields_}


class ProbePostPlan(C.Structure):
  """hbo_probe_post_plan (include/hbo_tune.h): what the test hook hbo_probe_posterior ran."""
  _fields_ = [(k, C.c_int32) for k in ('form', 'kchunk', 'nch', 'nchunks', 'nbuf', 'resident_chunks', 'direct_form')]

  def as_dict(self):
    return {k: int(getattr(self, k)) for k, _ in self._fields_}


# the same record as a NumPy dtype ([evals, R] logs)
ACQ_OPT_EVAL_DTYPE = np.dtype([('kind', np.int32), ('iter', np.int32), ('alpha', np.float64), ('value', np.float64)])

ACQ_OPT_S_EVALS = 8   # csrc/acq_opt_ctl.h: the header word of a start's state that counts its evaluations
# hbo_acq_opt_kind / hbo_acq_opt_status
ACQ_OPT_START, ACQ_OPT_MAIN, ACQ_OPT_LINE_SEARCH, ACQ_OPT_IDLE = 0, 1, 2, 3
(ACQ_OPT_RUNNING, ACQ_OPT_CONVERGED, ACQ_OPT_FTOL, ACQ_OPT_NO_PROGRESS, ACQ_OPT_NONFINITE_AT_START, ACQ_OPT_STEPS_DONE) = range(6)

# hbo_train_warp / hbo_train_target
TRAIN_WARP_IDENTITY, TRAIN_WARP_SOFTPLUS, TRAIN_WARP_SOFTPLUS_EPS, TRAIN_WARP_SQUAREPLUS = 0, 1, 2, 3
(TRAIN_NONE, TRAIN_LENGTHSCALE, TRAIN_SIGNAL_VARIANCE, TRAIN_NOISE_VARIANCE, TRAIN_CONSTANT, TRAIN_DOT_PROD_SIGMA, TRAIN_DOT_PROD_BIAS,
 TRAIN_LINEAR_KERNEL, TRAIN_LINEAR_BIAS, TRAIN_MLP_KERNEL, TRAIN_MLP_BIAS, TRAIN_KUMAR_A, TRAIN_KUMAR_B) = range(13)


# every symbol include/hbo.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SIGNATURES = {
    'hbo_ctx_create': (C.c_int, [C.c_int, C.POINTER(_P)]),
    'hbo_ctx_destroy': (C.c_int, [_P]),
    'hbo_last_error': (C.c_char_p, [_P]),
    'hbo_version': (C.c_char_p, []),
    'hbo_device_count': (C.c_int, []),
    'hbo_grad_layout_of': (C.c_int, [C.POINTER(Model), C.POINTER(GradLayout)]),
    'hbo_grad_layout_kumar_of': (C.c_int, [C.POINTER(Model), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'hbo_gram': (C.c_int, [_P, C.POINTER(Model), _P, C.c_int64, _P, C.c_int64, C.c_int, _P]),
    'hbo_mean': (C.c_int, [_P, C.POINTER(Model), _P, C.c_int64, _P]),
    'hbo_dataset_create': (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(Task), C.c_int, C.POINTER(_P)]),
    'hbo_dataset_free': (C.c_int, [_P, _P]),
    'hbo_dataset_subsample': (C.c_int, [_P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(_P)]),
    'hbo_nll': (C.c_int, [_P, C.POINTER(Model), _P, C.POINTER(C.c_double), C.POINTER(C.c_double),
                          C.POINTER(C.c_double)]),
    'hbo_objective': (C.c_int, [_P, C.POINTER(Model), _P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                C.POINTER(C.c_double)]),
    'hbo_factor': (C.c_int, [_P, C.POINTER(Model), _P, C.c_int64, _P, C.c_int32, C.POINTER(_P)]),
    'hbo_cache_export': (C.c_int, [_P, _P, _P, _P, _P]),
    'hbo_cache_free': (C.c_int, [_P, _P]),
    'hbo_cache_append': (C.c_int, [_P, C.POINTER(Model), _P, _P, C.c_int64, _P]),
    'hbo_acq_grad': (C.c_int, [_P, C.POINTER(Model), _P, _P, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_double,
                               _P, C.POINTER(C.c_double)]),
    'hbo_acq_grad_samples': (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P), _P, C.c_int64, C.c_int, C.POINTER(C.c_double),
                                       C.POINTER(C.c_double), C.c_double, _P, C.POINTER(C.c_double)]),
    'hbo_probe_acq_grad_samples64': (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P), _P, C.c_int64, C.c_int, C.POINTER(C.c_double),
                                               C.POINTER(C.c_double), C.c_double, _P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),   # hbo_tune.h (test hook)
    'hbo_acq_grad_samples_blocked': (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P), _P, C.c_int64, C.c_int, C.POINTER(C.c_double),
                                               C.POINTER(C.c_double), C.c_double, _P, C.POINTER(C.c_double)]),
    'hbo_probe_acq_grad_samples_blocked64': (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P), _P, C.c_int64, C.c_int, C.POINTER(C.c_double),
                                                       C.POINTER(C.c_double), C.c_double, _P, C.POINTER(C.c_double), C.c_int32, C.c_int64,
                                                       C.POINTER(C.c_double)]),   # hbo_tune.h (test hook)
    'hbo_acq_grad_samples_mlp': (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P), _P, C.c_int64, C.c_int, C.POINTER(C.c_double),
                                           C.POINTER(C.c_double), C.c_double, _P, C.POINTER(C.c_double)]),
    'hbo_probe_acq_grad_samples_mlp64': (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P), _P, C.c_int64, C.c_int, C.POINTER(C.c_double),
                                                   C.POINTER(C.c_double), C.c_double, _P, C.POINTER(C.c_double), C.c_int32, C.c_int64,
                                                   C.POINTER(C.c_double)]),   # hbo_tune.h (test hook)
    'hbo_acq_opt_state_doubles': (C.c_int64, [C.c_int32, C.c_int32]),
    'hbo_acq_maximize': (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P), _P, C.c_int32, _P, _P, C.c_int, C.POINTER(C.c_double),
                                   C.POINTER(C.c_double), C.c_double, C.POINTER(AcqOptOpts), _P, C.c_int32, _P, _P, _P, _P]),
    'hbo_acq_maximize_blocked': (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P), _P, C.c_int32, _P, _P, C.c_int, C.POINTER(C.c_double),
                                           C.POINTER(C.c_double), C.c_double, C.POINTER(AcqOptOpts), _P, C.c_int32, _P, _P, _P, _P]),
    'hbo_acq_maximize_mlp': (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P), _P, C.c_int32, _P, _P, C.c_int, C.POINTER(C.c_double),
                                       C.POINTER(C.c_double), C.c_double, C.POINTER(AcqOptOpts), _P, C.c_int32, _P, _P, _P, _P]),
    'hbo_acq_mes': (C.c_int, [_P, C.POINTER(Model), _P, _P, C.c_int64, C.POINTER(C.c_double), C.c_int32, C.c_double, C.c_double, _P]),
    'hbo_mes_grad_samples': (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P), _P, C.c_int64, C.POINTER(C.c_double), C.c_int32,
                                       C.POINTER(C.c_double), C.c_double, _P, C.POINTER(C.c_double)]),
    'hbo_probe_mes_grad_samples64': (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P), _P, C.c_int64, C.POINTER(C.c_double), C.c_int32,
                                               C.POINTER(C.c_double), C.c_double, _P, C.POINTER(C.c_double), C.c_int32, C.c_int64,
                                               C.POINTER(C.c_double)]),   # hbo_tune.h (test hook)
    'hbo_mes_maximize': (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P), _P, C.c_int32, _P, _P, C.POINTER(C.c_double), C.c_int32,
                                   C.POINTER(C.c_double), C.c_double, C.POINTER(AcqOptOpts), _P, C.c_int32, _P, _P, _P, _P]),
    'hbo_acq_logei': (C.c_int, [_P, C.POINTER(Model), _P, _P, C.c_int64, C.c_double, C.c_double, C.c_double, _P]),
    'hbo_logei_grad_samples': (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P), _P, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                         C.c_double, _P, C.POINTER(C.c_double)]),
    'hbo_probe_logei_grad_samples64': (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P), _P, C.c_int64, C.POINTER(C.c_double),
                                                 C.POINTER(C.c_double), C.c_double, _P, C.POINTER(C.c_double), C.c_int32, C.c_int64,
                                                 C.POINTER(C.c_double)]),   # hbo_tune.h (test hook)
    'hbo_logei_maximize': (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P), _P, C.c_int32, _P, _P, C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.c_double, C.POINTER(AcqOptOpts), _P, C.c_int32, _P, _P, _P, _P]),
    'hbo_qei_grad_samples': (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P), _P, C.c_int64, C.c_int32, C.POINTER(C.c_double), C.c_int32,
                                       C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double),
                                       C.POINTER(C.c_double)]),
    'hbo_qei_maximize': (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P), _P, C.c_int32, C.c_int32, _P, _P, C.POINTER(C.c_double), C.c_int32,
                                   C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.POINTER(AcqOptOpts), _P, C.c_int32, _P, _P,
                                   _P, _P]),
    'hbo_probe_acq_opt_ctl': (C.c_int, [_P, C.c_int32, C.c_int, C.POINTER(AcqOptOpts), _P, _P, _P, _P, _P, C.c_int32, _P, _P,
                                        C.POINTER(AcqOptEval), C.POINTER(C.c_int32)]),   # include/hbo_tune.h (test hook)
    'hbo_bo_simulated': (C.c_int, [_P, _P, C.POINTER(BoRun), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), _P, _P,
                                   C.POINTER(C.c_int32)]),
    'hbo_predict': (C.c_int, [_P, C.POINTER(Model), _P, _P, C.c_int64, C.c_int, _P, _P]),
    'hbo_acq': (C.c_int, [_P, C.POINTER(Model), _P, _P, C.c_int64, C.c_int, C.c_double, C.c_double,
                          C.c_double, _P]),
    'hbo_sample_paths': (C.c_int, [_P, C.POINTER(Model), _P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    'hbo_sample_paths_grad': (C.c_int, [_P, C.POINTER(Model), _P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_double, _P,
                                        C.POINTER(C.c_double)]),
    'hbo_paths_maximize': (C.c_int, [_P, C.POINTER(Model), _P, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_double, _P, C.c_int32, _P, _P,
                                     C.POINTER(AcqOptOpts), _P, C.c_int32, _P, _P, _P, _P]),
    'hbo_acq_samples': (C.c_int, [_P, _P, C.c_int32, _P, C.c_int64, _P, C.c_int32, _P, C.c_int64, C.c_int, C.POINTER(C.c_double),
                                  C.POINTER(C.c_double), C.c_double, _P]),
    'hbo_nll_samples': (C.c_int, [_P, _P, C.c_int32, _P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    'hbo_spd_solve': (C.c_int, [_P, C.c_int, _P, C.c_int64, _P, C.c_int32, _P, _P, _P,
                                C.POINTER(C.c_double)]),
    'hbo_chol_solve': (C.c_int, [_P, C.c_int, _P, C.c_int64, _P, C.c_int32, _P]),
    'hbo_profile_enable': (C.c_int, [_P, C.c_int]),
    'hbo_profile_get': (C.c_int, [_P, _P, C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_int32)]),
    'hbo_set_option': (C.c_int, [_P, C.c_char_p, C.c_int64]),
    'hbo_get_option': (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_int64)]),
    'hbo_sym_eig': (C.c_int, [_P, C.c_int, _P, C.c_int64, C.c_int32, _P, _P]),
    'hbo_nll_spectral': (C.c_int, [_P, C.POINTER(Model), _P, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                   C.POINTER(C.c_double)]),
    'hbo_tune': (C.c_int, [_P, C.c_char_p, C.c_int64]),   # include/hbo_tune.h: measurement hooks, not the boundary
    'hbo_mfma_peak_probe': (C.c_int, [_P, C.c_double, C.POINTER(C.c_double)]),   # include/hbo_tune.h
    'hbo_probe_post_product': (C.c_int, [_P, C.c_int, _P, C.c_int64, _P, C.c_int64, C.c_double, C.c_int, _P]),   # include/hbo_tune.h (test hook)
    'hbo_probe_gram': (C.c_int, [_P, C.c_int, _P, C.c_int32, _P, C.POINTER(C.c_int64), C.c_int32, _P, C.c_int64, C.c_int, C.c_double, _P,
                                 C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),   # include/hbo_tune.h (test hook)
    'hbo_probe_factor_inverse': (C.c_int, [_P, C.c_int, C.c_int32, C.POINTER(C.c_int64), _P, _P, C.c_int32, C.c_int, _P, _P, _P, _P, _P,
                                           C.POINTER(C.c_int32), _P]),   # include/hbo_tune.h (test hook; the last: hbo_probe_plan*)
    'hbo_probe_kumar_warp': (C.c_int, [_P, C.POINTER(Model), _P, C.c_int64, _P, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_double)]),   # include/hbo_tune.h (test hook)
    'hbo_probe_grad_contract': (C.c_int, [_P, C.POINTER(Model), C.c_int, C.c_int32, C.POINTER(C.c_int64), _P, _P, _P, C.c_int32,
                                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double,
                                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(C.c_int32)]),   # include/hbo_tune.h (test hook)
    'hbo_probe_posterior': (C.c_int, [_P, C.c_int, _P, C.c_int64, _P, _P, _P, _P, C.c_int64, C.c_double, _P, _P, _P, _P,
                                      _P]),   # include/hbo_tune.h (test hook; the last: hbo_probe_post_plan*)
    'hbo_comm_unique_id': (C.c_int, [_P]),
    'hbo_comm_init': (C.c_int, [_P, C.c_int, C.c_int, _P]),
    'hbo_comm_allreduce_sum': (C.c_int, [_P, C.POINTER(C.c_double), C.c_int32]),
    'hbo_comm_destroy': (C.c_int, [_P]),
    'hbo_objective_sharded': (C.c_int, [_P, C.POINTER(Model), _P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    'hbo_train_adam': (C.c_int, [_P, C.POINTER(Model), _P, C.POINTER(TrainLeaf), C.c_int32, _P, _P, _P, _P, _P, C.c_int32,
                                 C.c_double, C.c_double, C.c_double, C.c_double, _P, _P, _P, _P, C.POINTER(C.c_int32)]),
    'hbo_lbfgs_state_doubles': (C.c_int64, [C.c_int32, C.c_int32]),
    'hbo_train_lbfgs': (C.c_int, [_P, C.POINTER(Model), _P, C.POINTER(TrainLeaf), C.c_int32, C.POINTER(LbfgsOpts), _P, _P, C.c_int32,
                                  C.POINTER(LbfgsEval), _P, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'hbo_probe_lbfgs_ctl': (C.c_int, [_P, C.c_int32, C.POINTER(LbfgsOpts), _P, C.c_double, _P, _P, _P, C.POINTER(LbfgsEval),
                                      C.POINTER(C.c_int32)]),   # include/hbo_tune.h (test hook)
    'hbo_device_info': (C.c_int, [C.c_int, C.c_char_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
}

_lib = None
_lib_lock = threading.Lock()


def lib():
  """Loads libhbo.so (once).  Raises if it has not been built -- never falls back."""
  global _lib
  with _lib_lock:
    if _lib is None:
      if not os.path.exists(_LIB_PATH):
        raise HboError(HBO_ERR_NODEV, f'{_LIB_PATH} not found: build it with '
                       '`make -C hyperbo_amd/csrc` (or __graft_entry__.build()); there is no CPU fallback')
      l = C.CDLL(_LIB_PATH)
      for name, (res, args) in SIGNATURES.items():
        f = getattr(l, name)
        f.restype, f.argtypes = res, args
      _lib = l
    return _lib


def np_dtype(code):
  return np.float64 if code == F64 else np.float32


def dtype_code(dt):
  dt = np.dtype(dt)
  if dt == np.float64:
    return F64
  if dt == np.float32:
    return F32
  raise TypeError(f'unsupported dtype {dt}: float32 or float64 required')


def ptr(a):
  return None if a is None else a.ctypes.data_as(C.c_void_p)


class Context:
  """One hbo_ctx (one GPU).  Not thread-safe by design (hbo.h: not re-entrant per ctx)."""

  def __init__(self, device=0):
    self._h = _P()
    rc = lib().hbo_ctx_create(int(device), C.byref(self._h))
    if rc != HBO_OK:
      raise HboError(rc, (lib().hbo_last_error(None) or b'').decode())
    self.device = device

  def check(self, rc, allow_not_pd=True):
    if rc == HBO_OK or (allow_not_pd and rc == HBO_NOT_PD):
      return rc
    raise HboError(rc, (lib().hbo_last_error(self._h) or b'').decode())

  @property
  def handle(self):
    return self._h

  def close(self):
    if self._h:
      lib().hbo_ctx_destroy(self._h)
      self._h = _P()

  # (the routing switches 'spectral' and 'acq_fused' of hbo_set_option are documented on their own in include/hbo.h, not among these six tuning options;
  #  set_option reaches it through hbo_tune, which passes every name it does not know to hbo_set_option)
  PUBLIC_OPTIONS = ('potrf_group', 'lookahead', 'small_nblk', 'pool_cap_mb', 'post_chunk', 'bf16x3')

  def set_option(self, name, value):
    """The options of include/hbo.h; any other name goes to the measurement hook hbo_tune (include/hbo_tune.h)."""
    f = lib().hbo_set_option if name in self.PUBLIC_OPTIONS else lib().hbo_tune
    self.check(f(self._h, name.encode(), int(value)))

  def get_option(self, name):
    """An option of include/hbo.h read back (also the read-only 'eig_sweeps', 'chol_form', 'inv_forms' and 'post_resident'); unknown names raise."""
    out = C.c_int64(0)
    self.check(lib().hbo_get_option(self._h, name.encode(), C.byref(out)), allow_not_pd=False)
    return out.value

  def profile_enable(self, level):
    self.check(lib().hbo_profile_enable(self._h, int(level)))

  def profile_get(self):
    names = ((C.c_char * 32) * MAX_PROFILE_STAGES)()
    ms = (C.c_double * MAX_PROFILE_STAGES)()
    cnt = (C.c_int32 * MAX_PROFILE_STAGES)()
    n = C.c_int32(0)
    self.check(lib().hbo_profile_get(self._h, C.cast(names, _P), ms, cnt, C.byref(n)))
    return {names[i].value.decode(): (ms[i], cnt[i]) for i in range(n.value)}

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass


_default_ctx = None


def spectral_enabled():
  """True when the default context has the option 'spectral' set (include/hbo.h): the reference's SVD call sites then run on
  hbo_sym_eig / hbo_nll_spectral.  Without a default context nothing can have set it (and nothing touches the GPU)."""
  return _default_ctx is not None and bool(_default_ctx._h) and _default_ctx.get_option('spectral') == 1


def acq_fused_enabled():
  """True when the default context has the option 'acq_fused' set (include/hbo.h): value_and_grad calls over small caches then
  run as one hbo_acq_grad_samples launch.  Without a default context nothing can have set it (and nothing touches the GPU)."""
  return _default_ctx is not None and bool(_default_ctx._h) and _default_ctx.get_option('acq_fused') == 1


def default_context():
  """Process-wide context on device $HBO_DEVICE / $LOCAL_RANK / 0 (one process per GPU)."""
  global _default_ctx
  if _default_ctx is None:
    dev = int(os.environ.get('HBO_DEVICE', os.environ.get('LOCAL_RANK', '0')))
    ndev = lib().hbo_device_count()
    if ndev <= 0:
      raise HboError(HBO_ERR_NODEV, 'no HIP device visible; hyperbo_amd has no CPU fallback')
    _default_ctx = Context(dev % ndev)
  return _default_ctx
