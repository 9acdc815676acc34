"""CPU tier of pathwise posterior sampling (hbo_sample_paths; gp_utils/pathwise.py; acfun.thompson_sampling / thompson_batch): the export
and its binding, the argument checks that run before any device call, the draws against their restatement, the host-side refusals, and
tests/pathwise_cases.py judged on its own -- the spectral recipe against the kernels, the restated formulas against the posterior moments,
the conditioning of every GPU case and the distance of every mutant."""
import ctypes as C

import numpy as np
import pytest

import helpers
import pathwise_cases as pc
from hyperbo_amd import _native as nat
from hyperbo_amd.basics import definitions as defs
from hyperbo_amd.bo_utils import acfun, bayesopt
from hyperbo_amd.gp_utils import gp, kernel, mean, pathwise, utils
from oracle import hyperbo_oracle as o


# ---- export and argument errors --------------------------------------------------------------------------------------------------------
def test_entry_point_is_exported_and_bound():
  assert 'hbo_sample_paths' in nat.SIGNATURES
  f = nat.lib().hbo_sample_paths
  res, args = nat.SIGNATURES['hbo_sample_paths']
  assert f.restype is res and list(f.argtypes) == args and len(args) == 12


def _model(kernel_id=nat.KERNEL_SE, d=2):
  m = nat.Model()
  m.kernel_id, m.mean_id, m.dtype, m.input_dim = kernel_id, nat.MEAN_ZERO, nat.F64, d
  ls = np.ones(d)
  m.lengthscale, m.n_lengthscale, m.signal_variance, m.noise_variance, m.eps = nat.ptr(ls).value, d, 1.0, 0.1, 1e-6
  m.dot_prod_sigma, m.dot_prod_bias = 1.0, 0.1
  return m, ls


def _args(S=1, F=4, M=3, d=2, kernel_id=nat.KERNEL_SE):
  m, ls = _model(kernel_id, d)
  xq, om, ph, w = np.zeros((M, d)), np.zeros((F, d)), np.zeros(F), np.zeros((max(F, 1), max(S, 1)))
  out = np.full((M, max(S, 1)), 7.0)
  return dict(model=C.byref(m), cache=None, xq=nat.ptr(xq), M=M, S=S, F=F, omega=nat.ptr(om), phase=nat.ptr(ph), w=nat.ptr(w), eps=None,
              out=nat.ptr(out), _keep=(m, ls, xq, om, ph, w, out))


def _call(a, ctx=None):
  return nat.lib().hbo_sample_paths(ctx, a['model'], a['cache'], a['xq'], a['M'], a['S'], a['F'], a['omega'], a['phase'], a['w'], a['eps'], a['out'])


def test_argument_errors_come_before_any_device_call():
  err = lambda: (nat.lib().hbo_last_error(None) or b'').decode()
  for name in ('model', 'xq', 'omega', 'phase', 'w', 'out'):
    a = _args()
    a[name] = None
    assert _call(a) == nat.HBO_ERR_ARG and 'null argument' in err(), (name, err())
  for S in (0, -1, 1025):
    assert _call(_args(S=S)) == nat.HBO_ERR_ARG and '1 <= S <= 1024' in err(), (S, err())
  for F in (0, -2, 65537):
    a = _args()
    a['F'] = F
    assert _call(a) == nat.HBO_ERR_ARG and '1 <= F <= 65536' in err(), (F, err())
  for F in (2, 4):   # a dot-product model over D = 2 takes F = 3
    assert _call(_args(F=F, kernel_id=nat.KERNEL_DOT)) == nat.HBO_ERR_ARG and 'F = feature dim + 1' in err(), (F, err())
  a = _args()
  a['eps'] = a['w']   # eps without a cache
  assert _call(a) == nat.HBO_ERR_ARG and 'eps goes with a cache' in err()
  a = _args()
  assert _call(a) == nat.HBO_ERR_ARG and 'ctx is null' in err()
  a3 = _args(F=3, kernel_id=nat.KERNEL_DOT)
  assert _call(a3) == nat.HBO_ERR_ARG and 'ctx is null' in err()   # F = fdim + 1 passes the dot-product check
  assert np.all(a['_keep'][-1] == 7.0) and np.all(a3['_keep'][-1] == 7.0)   # no output was touched


def test_header_documents_the_entry_point():
  import os
  text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'hbo.h')).read()
  block = text[text.index('S posterior sample paths'):text.index('int hbo_sample_paths')]
  for word in ('Matheron', 'omega', 'phase', 'F = fdim + 1', 'HBO_ERR_ARG', 'post_chunk', 'bit-identical'):
    assert word in block, word


# ---- the draws and the host-side refusals --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kname', helpers.KERNELS)
def test_draws_follow_the_contract_order(kname):
  kid = getattr(kernel, kname).kernel_id
  for fdim, ls, F, S, n in ((3, np.array([0.4, 1.1, 0.7]), 9, 2, 5), (4, np.array([0.8]), 5, 1, 0)):
    got = pathwise.draw(np.random.default_rng(5), kid, fdim, ls, F, S, n)
    ref = pc.draws(np.random.default_rng(5), kname, fdim, ls, F, S, n)
    for g, r in zip(got, ref):
      assert (g is None and r is None) or (g.shape == r.shape and g.dtype == np.float64 and np.array_equal(g, r))
    assert got[2].shape == ((fdim + 1) if kname == 'dot_product' else F, S) and (got[3] is None) == (n == 0)


def test_lengthscale_is_warped_in_fp64_whatever_the_model_dtype():
  raw = np.array([0.3, -0.2, 1.5], dtype=np.float32)
  got = pathwise.warped_lengthscale(defs.GPParams(model={'lengthscale': raw}), utils.DEFAULT_WARP_FUNC)
  assert got.dtype == np.float64 and np.array_equal(got, pc.warped_lengthscale({'lengthscale': raw}))


def test_keys():
  g = np.random.default_rng(3)
  assert pathwise.as_generator(g) is g
  assert pathwise.as_generator(11).standard_normal() == np.random.default_rng(11).standard_normal()
  for bad in (None, 1.5, 'seed', True):
    with pytest.raises(ValueError):
      pathwise.as_generator(bad)


def _gp(cls=gp.GP, n=6, d=2):
  ds = {0: defs.SubDataset(np.zeros((n, d)), np.zeros((n, 1)))}
  return cls(ds, mean.constant, kernel.matern52, defs.GPParams(model={'constant': 1.0}))


def test_sample_paths_refusals_are_host_side():
  m = _gp()
  assert m.rng is None
  with pytest.raises(ValueError, match='random key'):
    m.sample_paths(np.zeros((3, 2)))
  with pytest.raises(ValueError, match='HGP'):
    _gp(gp.HGP).sample_paths(np.zeros((3, 2)), key=1)
  with pytest.raises(ValueError, match='HGP'):
    acfun.thompson_sampling(_gp(gp.HGP), 0, np.zeros((3, 2)), key=1)
  with pytest.raises(ValueError, match='HGP'):
    acfun.thompson_batch(_gp(gp.HGP), 0, np.zeros((3, 2)), 2, key=1)


def test_thompson_sampling_is_a_host_loop_acquisition_function():
  assert acfun.thompson_sampling.__name__ == 'thompson_sampling'
  assert not hasattr(acfun.thompson_sampling, 'value_and_grad') and not hasattr(acfun.thompson_sampling, 'maximize')
  assert acfun.thompson_sampling not in acfun._BO_DEVICE
  m = _gp()
  m.params.config['bo_on_device'] = 1
  pool = defs.SubDataset(np.zeros((4, 2)), np.zeros((4, 1)))
  with pytest.raises(ValueError, match='bo_on_device: ac_func .* is not one of the native acquisition functions'):
    bayesopt.simulated_bayesopt(m, 0, pool, acfun.thompson_sampling, 2)


def test_bayesopt_keeps_the_best_candidate_of_a_function_without_gradient():
  """bayesopt.bayesopt with an ac_func that has neither value_and_grad nor maximize (thompson_sampling's case): the best candidate is
  queried as it is.  (One that has either keeps its refinement: test_acq_opt_host.py.)"""
  m = _gp()
  seen, asked = [], []

  def first_coordinate(*, model, sub_dataset_key, x_queries):
    seen.append(np.array(x_queries))
    return x_queries[:, :1]

  def oracle(x):
    asked.append(np.array(x[0]))
    return np.zeros((1, 1))

  bayesopt.bayesopt(np.random.default_rng(2), m, 0, oracle, first_coordinate, 2, lambda rng, d: rng.uniform(size=(8, d)))
  assert len(seen) == 2 and len(asked) == 2
  for xs, xa in zip(seen, asked):
    assert np.array_equal(xa, xs[np.argmax(xs[:, 0])])
  assert m.dataset[0].x.shape[0] == 8


# ---- the spectral recipe ---------------------------------------------------------------------------------------------------------------
STATIONARY = ('squared_exponential', 'matern32', 'matern52')


def _spectral_setup():
  rng = np.random.default_rng(77)
  x = rng.uniform(size=(40, 3))
  model = {'lengthscale': helpers.inv_softplus(np.array([0.35, 0.6, 1.0])), 'signal_variance': helpers.inv_softplus(0.7)}
  return x, model


def _spectral_error(kname, F, mutant=None, seed=0):
  x, model = _spectral_setup()
  po = o.GPParams(model=model)
  sv = float(o.default_softplus(model['signal_variance']))
  om, ph, _, _ = pc.draws(np.random.default_rng([seed, F]), kname, 3, pc.warped_lengthscale(model), F, 1, 0, mutant)
  phi = pc.amplitude(sv, F, mutant) * np.cos(x @ om.T + ph[None, :])
  return float(np.max(np.abs(phi @ phi.T - getattr(o, kname)(po, x, warp_func=pc.WFO)))) / sv


@pytest.mark.parametrize('kname', STATIONARY)
def test_feature_products_reproduce_the_kernel(kname):
  for F in pc.SPECTRAL_F:
    for seed in range(3):
      e = _spectral_error(kname, F, seed=seed)
      assert e <= pc.SPECTRAL_C / np.sqrt(F), (kname, F, seed, e * np.sqrt(F))


@pytest.mark.parametrize('mutant', sorted(set(pc.SPECTRAL_MUTANTS) - {'half_phase'}))
def test_spectral_mutants_break_the_bound(mutant):
  knames = ('matern32', 'matern52') if mutant in ('gauss_matern', 'nu_dof') else STATIONARY
  for kname in knames:
    ratios = [_spectral_error(kname, F, mutant) * np.sqrt(F) / pc.SPECTRAL_C for F in pc.SPECTRAL_F]
    assert max(ratios) > 1.0, (mutant, kname, ratios)


def test_phases_from_half_the_circle_leave_the_second_moments_alone():
  """Phases from [0, pi) were listed as a mutant that must break the bound.  They cannot, at any F: 2 cos(a + b) cos(a' + b) =
  cos(a - a') + cos(a + a' + 2 b), and 2 b is still uniform on the whole circle, so E[Phi Phi^T] = K exactly (measured: 0.39 and 0.28
  of the bound at F = 4096 and 16384, squared exponential, as the correct recipe).  A feature-product check cannot tell the two apart;
  the same holds for any other interval once omega is averaged too (its density is symmetric, E sin(omega . (x + x')) = 0).  The phase
  defect the check does see is the degenerate one, no phases at all ('zero_phase' above): E cos(a) cos(a') keeps k(x, -x') / 2."""
  for kname in STATIONARY:
    for F in pc.SPECTRAL_F:
      assert _spectral_error(kname, F, 'half_phase') <= pc.SPECTRAL_C / np.sqrt(F), (kname, F)


# ---- the restated formulas against the posterior's moments -----------------------------------------------------------------------------
VAL_S, VAL_F = 4000, 4096


def _validation_problem(kname):
  rng = np.random.default_rng([helpers.KERNELS.index(kname), 5])
  d, n, mq = 2, 12, 6
  # short lengthscales and noise = signal variance: the omitted noise draw costs the covariance noise k* Kt^-2 k*, at an isolated
  # observation sv / 4, well above the bound's ~0.08 sv
  model = {'lengthscale': helpers.inv_softplus(np.array([0.15, 0.2])), 'signal_variance': helpers.inv_softplus(0.8),
           'noise_variance': helpers.inv_softplus(0.8), 'constant': np.array(0.3), 'dot_prod_sigma': helpers.inv_softplus(0.9),
           'dot_prod_bias': np.array(0.4)}
  x, y = helpers.synthetic_task(rng, n, d)
  xq = np.vstack([x[:3] + 0.01, rng.uniform(size=(mq - 3, d))])   # three queries next to observations: where the noise draw matters most
  ls = pc.warped_lengthscale(model)
  om, ph, w, eps = pc.draws(rng, kname, d, ls, VAL_F, VAL_S, n)
  return pc.Problem(kname, False, 'constant', False, model, x, y, xq, om, ph, w, eps)


def _moments(prob):
  po = o.GPParams(model=prob.model)
  mu, cov = o.predict(o.constant, getattr(o, prob.kname), po, prob.x, prob.y, prob.xq, pc.WFO, full_cov=True)
  return np.asarray(mu)[:, 0], np.asarray(cov)


@pytest.mark.parametrize('kname', helpers.KERNELS)
def test_restated_paths_have_the_posterior_moments(kname):
  prob = _validation_problem(kname)
  mu, cov = _moments(prob)
  sv = 0.0 if kname == 'dot_product' else float(o.default_softplus(prob.model['signal_variance']))   # the dot product's basis is exact
  cov_bound = pc.SPECTRAL_C / np.sqrt(VAL_F) * sv + 4 * np.sqrt(2 / VAL_S) * np.max(np.diag(cov))
  f = pc.restate(prob, np.float64)
  z = np.abs(f.mean(axis=1) - mu) / np.sqrt(np.diag(np.cov(f)) / VAL_S)
  assert np.max(z) <= 4.5, (kname, z)
  cov_err = float(np.max(np.abs(np.cov(f) - cov)))
  assert cov_err <= cov_bound, (kname, cov_err, cov_bound)
  assert pc.helpers.rel_err(pc.restate(prob, np.float64, zero=True)[:, 0], mu) <= 1e-10   # w = 0, eps = 0: the posterior mean
  # the counter-example the noise level was chosen for: without the noise draw the covariance is short by noise k* Kt^-2 k*
  f0 = pc.restate(prob, np.float64, no_eps=True)
  assert float(np.max(np.abs(np.cov(f0) - cov))) > cov_bound, kname


# ---- every GPU case: conditioning and mutants --------------------------------------------------------------------------------------------
FP64_CASES = [c for c in pc.CASES if c.dtype == 'fp64']


def test_case_list_covers_the_issue():
  cs = pc.CASES
  assert {c.n for c in cs} >= {0, 1, 127, 128, 129, 300} and {c.M for c in cs} >= {1, 130, 300}
  assert {c.F for c in cs if c.kname != 'dot_product'} >= {1, 63, 64, 65, 200} and {c.S for c in cs} >= {1, 3, 65}
  assert {c.d for c in cs} >= {1, 3, 17} and {c.kname for c in cs} == set(helpers.KERNELS) and {c.mname for c in cs} == set(helpers.MEANS)
  assert any(c.mlp for c in cs) and any(c.kumar for c in cs) and {c.dtype for c in cs} == {'fp64', 'fp32'}
  assert all(c.chunk and c.M > 2 * c.chunk for c in cs if c.M == 300)   # M = 300 spans three chunks
  assert all(c.F == c.fdim + 1 for c in cs if c.kname == 'dot_product')
  assert len({c.id for c in cs}) == len(cs)


@pytest.mark.parametrize('case', pc.CASES, ids=lambda c: c.id)
def test_case_is_well_conditioned_and_sees_every_mutant(case):
  prob, ref = pc.problem(case), pc.reference(case)
  assert ref.dtype == pc.LD and ref.shape == (case.M, case.S) and np.isfinite(ref.astype(np.float64)).all()
  cond = float(np.max(pc.col_errors(pc.restate(prob, np.float64), ref)))
  assert cond <= pc.COND_BOUND, cond
  if case.dtype == 'fp32':
    assert np.isfinite(pc.f32_level(case)) and pc.bound(case) < 1e-2, pc.f32_level(case)   # (an fp32 bound that still means something)
  for mutant in sorted(set(pc.MUTANTS) - pc.not_applicable(prob)):
    far = float(np.max(pc.col_errors(pc.restate(prob, np.float64, mutant), ref)))
    assert far >= pc.MUTANT_FACTOR * pc.FP64_BOUND, (mutant, far)


def test_thompson_loop_has_no_argmax_decided_by_rounding():
  ts = pc.ts_setup()
  sel, gap = pc.thompson_loop(ts.model, ts.x0, ts.y0, ts.pool_x, ts.pool_y, ts.iters, ts.F, ts.seed)
  assert len(sel) == ts.iters and gap >= pc.TS_GAP, gap
