"""CPU tier of the one-launch acquisition gradient (hbo_acq_grad_samples, context option 'acq_fused'): the export and its binding,
the argument checks that run before any device call, and the host-side routing helper of bo_utils/acfun.py."""
import ctypes as C

import numpy as np

from hyperbo_amd import _native as nat
from hyperbo_amd.basics import definitions as defs
from hyperbo_amd.bo_utils import acfun
from hyperbo_amd.gp_utils import gp, kernel, mean


def test_entry_point_is_exported_and_bound():
  assert 'hbo_acq_grad_samples' in nat.SIGNATURES
  f = nat.lib().hbo_acq_grad_samples
  res, args = nat.SIGNATURES['hbo_acq_grad_samples']
  assert f.restype is res and list(f.argtypes) == args and len(args) == 12


def _args(S=1, M=1, D=2):
  models = (nat.Model * max(S, 1))()
  caches = (C.c_void_p * max(S, 1))()
  xq = np.zeros((M, D))
  prm = (C.c_double * max(S, 1))()
  nse = (C.c_double * max(S, 1))()
  out = np.full((max(S, 1), M), 7.0)
  grad = np.full((max(S, 1), M, D), 7.0)
  return dict(models=models, S=S, caches=caches, xq=nat.ptr(xq), M=M, acq_id=nat.ACQ_EI, prm=prm, nse=nse, scale=1.0, out=nat.ptr(out),
              grad=grad.ctypes.data_as(C.POINTER(C.c_double)), _keep=(xq, out, grad))


def _call(a, ctx=None):
  return nat.lib().hbo_acq_grad_samples(ctx, a['models'], a['S'], a['caches'], a['xq'], a['M'], a['acq_id'], a['prm'], a['nse'], a['scale'],
                                        a['out'], a['grad'])


def test_argument_errors_come_before_any_device_call():
  err = lambda: (nat.lib().hbo_last_error(None) or b'').decode()
  for name in ('models', 'caches', 'xq', 'prm', 'nse', 'out', 'grad'):
    a = _args()
    a[name] = None
    assert _call(a) == nat.HBO_ERR_ARG and 'null argument' in err(), (name, err())
  for S in (0, -3, 4097):
    a = _args(S=S)
    assert _call(a) == nat.HBO_ERR_ARG and '1 <= S <= 4096' in err(), (S, err())
  for acq_id in (-1, 3):
    a = _args()
    a['acq_id'] = acq_id
    assert _call(a) == nat.HBO_ERR_ARG and 'bad acq_id' in err(), (acq_id, err())
  a = _args()
  assert _call(a) == nat.HBO_ERR_ARG and 'ctx is null' in err()
  out, grad = a['_keep'][1:]
  assert np.all(out == 7.0) and np.all(grad == 7.0)   # no output was touched


def _stub(n=30, d=3, cov=kernel.matern52, mean_func=mean.constant, hgp=True):
  x, y = np.zeros((n, d)), np.zeros((n, 1))
  ds = {'t': defs.SubDataset(x, y), 'other': defs.SubDataset(np.zeros((4, d)), np.zeros((4, 1)))}
  params = defs.GPParams(model={'constant': 1.0}, samples=[{'constant': 1.0}] * 3) if hgp else defs.GPParams(model={'constant': 1.0})
  return (gp.HGP if hgp else gp.GP)(ds, mean_func, cov, params)


def test_routing_helper_names_the_first_unmet_condition():
  unmet = acfun._acq_fused_unmet
  m = _stub()
  assert unmet(m, 't', 3, 3, enabled=True) is None
  assert unmet(m, 't', 3, None, enabled=True) is None          # handles not counted yet
  assert unmet(_stub(hgp=False), 't', enabled=True) is None    # a plain GP is S = 1
  assert unmet(_stub(n=128), 't', 3, 3, enabled=True) is None
  assert 'acq_fused' in unmet(m, 't', 3, 3, enabled=False)
  assert 'acq_fused' in unmet(m, 't', 3, 3)                    # no default context: nothing can have set the option
  assert 'no observations' in unmet(m, 'missing', 3, 3, enabled=True)
  assert 'no observations' in unmet(_stub(n=0), 't', 3, 3, enabled=True)
  assert '129 > 128' in unmet(_stub(n=129), 't', 3, 3, enabled=True)
  assert 'MLP basis' in unmet(_stub(cov=kernel.matern52_mlp), 't', 3, 3, enabled=True)
  assert 'linear_mlp' in unmet(_stub(mean_func=mean.linear_mlp), 't', 3, 3, enabled=True)
  assert 'Kumaraswamy' in unmet(_stub(cov=kernel.matern52_kumar), 't', 3, 3, enabled=True)
  assert 'only 2 of the 3' in unmet(m, 't', 3, 2, enabled=True)
  # the order: the option first, then the data, then the model family, then the budget
  assert 'acq_fused' in unmet(_stub(n=129, cov=kernel.matern52_mlp), 't', 3, 1, enabled=False)
  assert '129 > 128' in unmet(_stub(n=129, cov=kernel.matern52_mlp), 't', 3, 1, enabled=True)
  assert 'MLP basis' in unmet(_stub(cov=kernel.matern52_mlp, mean_func=mean.linear_mlp), 't', 3, 1, enabled=True)


def test_option_is_documented_next_to_spectral():
  import os
  text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'hbo.h')).read()
  block = text[text.index('int hbo_set_option'):text.index('int hbo_get_option')]
  import re
  assert re.search(r'\bacq_fused\s+0/1\s+\(default 0\)', block) and re.search(r'\bspectral\s+0/1', block)
