"""Cases of the streamed posterior (hbo_predict / hbo_acq without full_cov; csrc/cache.hip: posterior) shared by the CPU judge
tests/test_posterior_cases_host.py and the GPU test tests/test_gpu_posterior.py.

Exact tier.  Integer operands on which every product and every partial sum of the route is an integer below 2^24, so that the result is
known to the last bit in fp32 and fp64, on every product form and in any summation order:
  W     [n, n]  per row r eight entries of +-1 / +-2 at random columns <= r, then a diagonal of 1 or 2
  Kxq   [n, M]  in {-2..2}       alpha [n] in {-3..3}       mu0 [M] in {-5..5}
  kdiag [M]     sum_i colsq[i, q] + r_q with r_q in {0, 1, 2, 3}: the expected variance is exactly r_q, zero included, and a lost or
                doubled square is at least 100 % of it.
(The last three rows of Kxq and alpha hold no zero: the rows of post_mupart_kernel's scalar tail loop always count.)
direct() computes the outputs from the definition; simulate() walks the route as posterior() does -- query chunks of post_chunk through
two alternating workspaces with their own padded leading dimension, K chunks of kchunk blocks summed before they are squared, the mean's
products per row block with a four-way unrolled loop and a tail -- and takes a MUTANT, one of the faults the GPU test has to see.
plan() is the host twin of post_plan (csrc/api_internal.h): the route a case must report through hbo_probe_post_plan.

Real-kernel tier.  hbo_factor + hbo_predict against the fp64 oracle per query: families, shapes and the heterogeneous queries (a third
like the data, a third exact copies of training rows, a third far away), the reference with each query's own scales and the bounds'
constants are below; the measured errors they come from are in profiles/posterior_errors.md."""
import dataclasses
import functools

import numpy as np
import scipy.sparse as sp

TILE = 128
DEFAULT_CHUNK = 8192
FORMS = {'mfma': 0, 'bf16x3': 1, 'f16x2': 2}   # hbo_probe_post_plan.form
K_BOUND = 2.0                                   # |Kxq| <= 2: what the exact tier hands over as the signal variance


def padded_ld(extent, dtype):
  """runtime.h: padded_ld -- 128 bytes beyond the padded extent."""
  return extent + (16 if dtype == 'fp64' else 32)


def round_up(v, m):
  return (v + m - 1) // m * m


# ---- the exact design --------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True, eq=False)
class Design:
  n: int
  M: int
  W: np.ndarray        # [n, n] float64 integers, lower triangular
  alpha: np.ndarray    # [n]
  Kxq: np.ndarray      # [n, M]
  mu0: np.ndarray      # [M]
  r: np.ndarray        # [M] the expected variance
  kdiag: np.ndarray    # [M]

  @property
  def nblk(self):
    return (self.n + TILE - 1) // TILE


@functools.lru_cache(maxsize=None)
def design(n, M):
  rng = np.random.default_rng([n, M, 20])
  W = np.zeros((n, n))
  cols = (rng.random((n, 8)) * (np.arange(n)[:, None] + 1)).astype(np.int64)   # columns <= r
  vals = rng.choice([-2.0, -1.0, 1.0, 2.0], size=(n, 8))
  for j in range(8):
    W[np.arange(n), cols[:, j]] = vals[:, j]
  W[np.arange(n), np.arange(n)] = rng.choice([1.0, 2.0], size=n)
  Kxq = rng.integers(-2, 3, size=(n, M)).astype(np.float64)
  alpha = rng.integers(-3, 4, size=n).astype(np.float64)
  tail = slice(max(n - 3, 0), n)
  Kxq[tail] = np.where(Kxq[tail] == 0, 1.0, Kxq[tail])
  alpha[tail] = np.where(alpha[tail] == 0, 1.0, alpha[tail])
  mu0 = rng.integers(-5, 6, size=M).astype(np.float64)
  r = rng.integers(0, 4, size=M).astype(np.float64)
  d = Design(n, M, W, alpha, Kxq, mu0, r, np.zeros(M))
  kdiag = block_sums(product(d) ** 2).sum(axis=0) + r
  d = dataclasses.replace(d, kdiag=kdiag)
  for a in (d.W, d.alpha, d.Kxq, d.mu0, d.r, d.kdiag):
    a.setflags(write=False)
  return d


def product(d, Kxq=None):
  """V = W Kxq (W is sparse: eight entries and the diagonal per row)."""
  return np.asarray(sp.csr_matrix(d.W) @ (d.Kxq if Kxq is None else Kxq))


def block_sums(a):
  """[nblk, M]: the column sums of a [n, M] over each 128-row block."""
  n = a.shape[0]
  return np.add.reduceat(a, np.arange(0, n, TILE), axis=0)


@dataclasses.dataclass
class Outputs:
  mu: np.ndarray
  var: np.ndarray
  colsq: np.ndarray     # [nblk, M] of the LAST chunk's workspace layout is not modelled: whole-call arrays, compared on single-chunk calls
  mupart: np.ndarray

  def differs(self, other, single_chunk):
    names = ['mu', 'var'] + (['colsq', 'mupart'] if single_chunk else [])
    return [k for k in names if not np.array_equal(getattr(self, k), getattr(other, k))]


@functools.lru_cache(maxsize=None)
def direct(n, M):
  """The outputs from the definition (fp64 integers, exact).  Shared and read-only."""
  d = design(n, M)
  colsq = block_sums(product(d) ** 2)
  mupart = block_sums(d.Kxq * d.alpha[:, None])
  out = Outputs(mupart.sum(axis=0) + d.mu0, d.kdiag - colsq.sum(axis=0), colsq, mupart)
  for a in (out.mu, out.var, out.colsq, out.mupart):
    a.setflags(write=False)
  return out


def magnitudes(d):
  """The three sums of absolute values that bound every partial sum of the route: max_q sum_k |W| |Kxq| (any element of V or of a K
  chunk's partial), max_q sum_i colsq (any partial of the variance; kdiag itself is this plus at most 3) and
  max_q (sum |Kxq alpha| + |mu0|) (any partial of the mean)."""
  vabs = np.asarray(sp.csr_matrix(np.abs(d.W)) @ np.abs(d.Kxq))
  return (float(vabs.max()), float((vabs ** 2).sum(axis=0).max()) + 3.0,
          float((np.abs(d.Kxq) * np.abs(d.alpha)[:, None]).sum(axis=0).max() + np.abs(d.mu0).max()))


def dead_pairs(d):
  """Liveness per K block: for every 128 x 128 block (i, k <= i) of W, the queries whose colsq[i, q] does NOT change when the block is
  zeroed.  Returns (unchanged pairs, all pairs)."""
  V = product(d)
  dead = total = 0
  for i in range(d.nblk):
    rows = slice(i * TILE, min((i + 1) * TILE, d.n))
    base = (V[rows] ** 2).sum(axis=0)
    for k in range(i + 1):
      ks = slice(k * TILE, min((k + 1) * TILE, d.n))
      dv = d.W[rows, ks] @ d.Kxq[ks]
      dead += int(np.sum(((V[rows] - dv) ** 2).sum(axis=0) == base))
      total += d.M
  return dead, total


# ---- the route, walked on the host ---------------------------------------------------------------------------------------------------
MUTANTS = ('ragged_k_dropped', 'squared_before_sum', 'colsq_row_reversed', 'last_block_not_in_var', 'mupart_tail_dropped',
           'chunk_written_at_previous_q0', 'ragged_chunk_read_with_ldq_max', 'workspace_reused_one_chunk_early')


def simulate(n, M, post_chunk, kchunk, dtype='fp64', mutant=None):
  """posterior()'s route over design(n, M): Outputs, exact.  kchunk as plan() gives it (0: the product is not split along K)."""
  assert mutant is None or mutant in MUTANTS
  d = design(n, M)
  nblk, npad = d.nblk, round_up(n, TILE)
  CH = max(post_chunk, TILE)
  nchunks = (M + CH - 1) // CH
  nbuf = 2 if M > CH else 1
  ldq_max = padded_ld(round_up(min(M, CH), TILE), dtype)
  chunks = [(c * CH, min(CH, M - c * CH)) for c in range(nchunks)]
  # producer: chunk c's padded cross Gram in workspace c % nbuf, rows ldq apart, zero padding
  def produced(c):
    q0, mc = chunks[c]
    ldq = padded_ld(round_up(mc, TILE), dtype)
    K = np.zeros((npad, ldq))
    K[:n, :mc] = d.Kxq[:, q0:q0 + mc]
    return K
  mu, var = np.full(M, np.nan), np.full(M, np.nan)
  colsq_all, mupart_all = np.full((nblk, M), np.nan), np.full((nblk, M), np.nan)
  for c, (q0, mc) in enumerate(chunks):
    src = c + 2 if (mutant == 'workspace_reused_one_chunk_early' and c + 2 < nchunks) else c
    K = produced(src)
    ldq = padded_ld(round_up(mc, TILE), dtype)
    if K.shape[1] != ldq:   # (the early reuse: the consumer still reads with ITS chunk's leading dimension)
      flat = np.zeros(npad * max(ldq, K.shape[1])); flat[:K.size] = K.ravel(); K = flat[:npad * ldq].reshape(npad, ldq)
    if mutant == 'ragged_chunk_read_with_ldq_max' and ldq != ldq_max:
      flat = np.zeros(npad * ldq_max); flat[:K.size] = K.ravel(); K = flat.reshape(npad, ldq_max)[:, :ldq].copy()
    Kc = K[:n, :mc]
    # product: per row tile the K chunks' partials, summed, squared, summed over the tile's rows
    colsq = np.zeros((nblk, mc))
    for i in range(nblk):
      rows = slice(i * TILE, min((i + 1) * TILE, n))
      kc = kchunk if kchunk > 0 else i + 1
      parts = []
      for k0 in range(0, i + 1, kc):
        kb = min(kc, i + 1 - k0)
        if mutant == 'ragged_k_dropped' and kchunk > 0 and kb < kc:
          continue
        ks = slice(k0 * TILE, min((k0 + kb) * TILE, n))
        parts.append(d.W[rows, ks] @ Kc[ks])
      if mutant == 'squared_before_sum':
        colsq[i] = sum((p ** 2).sum(axis=0) for p in parts)
      else:
        colsq[i] = (sum(parts) ** 2).sum(axis=0) if parts else 0.0
    if mutant == 'colsq_row_reversed':
      colsq = colsq[::-1].copy()
    # mean: per row block four running sums over i, i + 1, i + 2, i + 3 and a scalar tail
    mupart = np.zeros((nblk, mc))
    for b in range(nblk):
      i0, i1 = b * TILE, min((b + 1) * TILE, n)
      if mutant == 'mupart_tail_dropped':
        i1 -= (i1 - i0) % 4
      mupart[b] = (Kc[i0:i1] * d.alpha[i0:i1, None]).sum(axis=0)
    # epilogue
    nb_var = nblk - 1 if mutant == 'last_block_not_in_var' else nblk
    out0 = chunks[c - 1][0] if (mutant == 'chunk_written_at_previous_q0' and c > 0) else q0
    mu[out0:out0 + mc] = mupart.sum(axis=0) + d.mu0[q0:q0 + mc]
    var[out0:out0 + mc] = d.kdiag[q0:q0 + mc] - colsq[:nb_var].sum(axis=0)
    colsq_all[:, q0:q0 + mc] = colsq
    mupart_all[:, q0:q0 + mc] = mupart
  return Outputs(mu, var, colsq_all, mupart_all)


# ---- routes -------------------------------------------------------------------------------------------------------------------------
def plan(n, M, post_chunk, cus, dtype='fp64', form='f16x2', k_bound=K_BOUND, lauum_persist=1):
  """post_plan + PostPlan::chunk + launch_post3's rule, as hbo_probe_post_plan reports them.  form: what the options allow an fp32
  product ('mfma': post_bf16x3 = 0; 'bf16x3': post_f16x2 = 0; 'f16x2': the defaults)."""
  nblk = (n + TILE - 1) // TILE
  CH = max(post_chunk, TILE)
  nchunks = (M + CH - 1) // CH
  kchunk = nch = 0
  if nblk >= 2 and ((M + TILE - 1) // TILE) * nblk < 2 * cus:
    kchunk = 1 if nblk < 8 else max(2, min(8, nblk // 8))
    nch = (nblk + kchunk - 1) // kchunk
  f = 'mfma'
  if dtype == 'fp32' and kchunk == 0 and form != 'mfma':
    f = 'f16x2' if (form == 'f16x2' and k_bound > 0) else 'bf16x3'
  resident = 0
  for c in range(nchunks):
    mc = min(CH, M - c * CH)
    if kchunk == 0 and lauum_persist and (round_up(mc, TILE) // TILE) * nblk > 4 * cus:
      resident += 1
  nbuf = 2 if M > CH else 1
  return {'form': FORMS[f], 'kchunk': kchunk, 'nch': nch, 'nchunks': nchunks, 'nbuf': nbuf, 'resident_chunks': resident,
          'direct_form': int(nbuf == 2)}


def plain_streamed_M(cus, nblk=2):
  """The smallest M whose product over nblk blocks is not split along K, plus one: ceil(M / 128) * nblk >= 2 * cus."""
  return ((2 * cus + nblk - 1) // nblk - 1) * TILE + 1


def resident_Ms(cus, nblk=9):
  """(ragged M of the resident grid, largest M of the plain grid): the smallest tile count with tiles * nblk > 4 * cus, less 57
  queries; and one tile fewer, full."""
  t = (4 * cus) // nblk + 1
  return t * TILE - 57, (t - 1) * TILE


@dataclasses.dataclass(frozen=True)
class RouteCase:
  name: str
  n: int
  M: int
  post_chunk: int
  route: str          # 'one_block', 'splitk', 'plain', 'resident'

  @property
  def id(self):
    return f'{self.name}-n{self.n}-M{self.M}-ch{self.post_chunk}'

  @property
  def single_chunk(self):
    return self.M <= max(self.post_chunk, TILE)


def route_cases(cus):
  res_M, plain_M = resident_Ms(cus)
  return [
      RouteCase('one', 1, 1, DEFAULT_CHUNK, 'one_block'),
      RouteCase('one_full', 128, 128, DEFAULT_CHUNK, 'one_block'),
      RouteCase('one_3chunks', 100, 300, 128, 'one_block'),
      RouteCase('one_own_ldq', 100, 300, 256, 'one_block'),        # chunks of 256 and 44: the last one's mpad and ldq are its own
      RouteCase('k1_one_query', 129, 1, DEFAULT_CHUNK, 'splitk'),
      RouteCase('k1', 300, 130, DEFAULT_CHUNK, 'splitk'),
      RouteCase('k1_3chunks', 300, 300, 128, 'splitk'),            # vpart shared by the chunks in flight
      RouteCase('k1_own_ldq', 300, 300, 256, 'splitk'),
      RouteCase('k2', 1100, 130, DEFAULT_CHUNK, 'splitk'),
      RouteCase('k3', 3100, 130, DEFAULT_CHUNK, 'splitk'),
      RouteCase('plain_streamed', 129, plain_streamed_M(cus), DEFAULT_CHUNK, 'plain'),
      RouteCase('resident', 1100, res_M, 65536, 'resident'),
      RouteCase('plain_edge', 1100, plain_M, 65536, 'plain'),
  ]


EXPECT_KCHUNK = {'k1_one_query': 1, 'k1': 1, 'k1_3chunks': 1, 'k1_own_ldq': 1, 'k2': 2, 'k3': 3}

# which case has to see which mutant (tests/test_posterior_cases_host.py proves it on the CPU, at 256 CUs)
MUTANT_CASE = {
    'ragged_k_dropped': 'k2',
    'squared_before_sum': 'k1',
    'colsq_row_reversed': 'k3',
    'last_block_not_in_var': 'k2',
    'mupart_tail_dropped': 'k1_one_query',
    'chunk_written_at_previous_q0': 'one_3chunks',
    'ragged_chunk_read_with_ldq_max': 'k1_own_ldq',
    'workspace_reused_one_chunk_early': 'one_3chunks',
}

# (dtype, what the options allow, k_bound) of the exact tier's runs; a product split along K is GEMM_POST whatever the options say
RUNS = [('fp64', 'f16x2', K_BOUND), ('fp32', 'mfma', K_BOUND), ('fp32', 'bf16x3', K_BOUND), ('fp32', 'f16x2', K_BOUND), ('fp32', 'f16x2', 0.0)]


def runs_of(case):
  return RUNS[:1] + RUNS[3:4] if case.route == 'splitk' else RUNS


# ---- real-kernel tier -----------------------------------------------------------------------------------------------------------------
REAL_FAMILIES = [('squared_exponential', 'constant'), ('matern32', 'linear'), ('dot_product', 'zero')]
REAL_D = 4
REAL_DTYPES = ('fp64', 'fp32')
# Per-query bounds: |mu - ref| <= C_MU * (|mu0_q| + sum_i |Kxq_iq alpha_i|), |var - ref| <= C_VAR * (kdiag_q + sum_i V_iq^2), with
# (C_MU, C_VAR) = 10 x the worst device error measured on the MI355X over the whole list (profiles/posterior_errors.md),
# one row per dtype and fp32 product form.  The reference's own two-route gap has to stay below a tenth of them
# (tests/test_posterior_cases_host.py).
# The mean's worst query is a far one under the linear mean: there Kxq is nothing and mu0_q = x_q . w + b is a difference of terms up to
# twenty times its own size, so that relative to |mu0_q| the rounding of the mean's own dot product shows (fp64 1.459e-13, fp32
# 6.215e-05 at n = 129, M = 32641).  Without that family the worst is 3.422e-16 / 6.362e-08: the other two families are held to that.
REAL_BOUNDS = {
    ('fp64', 'mfma'): (1.5e-12, 1.1e-14),
    ('fp32', 'mfma'): (6.2e-4, 4.0e-6),
    ('fp32', 'bf16x3'): (6.2e-4, 4.1e-6),
    ('fp32', 'f16x2'): (6.2e-4, 4.5e-6),
}
# (fp32 only.  In fp64 ten times 3.422e-16 would leave the reference's own gap, 5.0e-16 on the dot product at n = 129, above a tenth of
#  the bound: there the device is as accurate as the reference and the one row stands.)
REAL_MU_BOUND_NO_LINEAR_MEAN = {'fp32': 6.4e-7}


def real_bounds(case, form):
  """(C_MU, C_VAR) of a case: the row of its dtype and form; in fp32 the mean of a family without a linear mean by the tighter constant."""
  c_mu, c_var = REAL_BOUNDS[(case.dtype, form)]
  return (c_mu if case.mname == 'linear' else REAL_MU_BOUND_NO_LINEAR_MEAN.get(case.dtype, c_mu)), c_var


@dataclasses.dataclass(frozen=True)
class RealCase:
  kname: str
  mname: str
  n: int
  M: int
  post_chunk: int
  dtype: str

  @property
  def id(self):
    return f'{self.kname}+{self.mname}-n{self.n}-M{self.M}-ch{self.post_chunk}-{self.dtype}'

  @property
  def np_dtype(self):
    return np.float64 if self.dtype == 'fp64' else np.float32


def real_shapes(cus):
  return [(100, 300, 128), (300, 130, DEFAULT_CHUNK), (1100, 257, 128), (129, plain_streamed_M(cus), DEFAULT_CHUNK)]


def real_cases(cus):
  return [RealCase(k, m, n, M, ch, dt) for (k, m) in REAL_FAMILIES for (n, M, ch) in real_shapes(cus) for dt in REAL_DTYPES]


def real_forms(case, cus):
  """The fp32 forms a case can reach through the options (the form hbo_predict takes by default last); fp64 and products split along K
  have one."""
  if case.dtype == 'fp64' or plan(case.n, case.M, case.post_chunk, cus)['kchunk'] > 0:
    return ['mfma']
  return ['mfma', 'bf16x3'] + ([] if case.kname == 'dot_product' else ['f16x2'])


def _cast(tree, dtype):
  return {k: _cast(v, dtype) for k, v in tree.items()} if isinstance(tree, dict) else np.asarray(tree, dtype=dtype)


@functools.lru_cache(maxsize=None)
def real_inputs(case):
  """model, x, y, xq in the case's dtype.  Queries: a third drawn like the data, a third exact copies of training rows, a third far away
  (stationary kernels: ten length-scales off along a random direction; dot product: rows scaled by 1e-2 and by 10), interleaved so that
  every chunk and tile holds all three kinds."""
  import helpers
  from oracle import hyperbo_oracle as o
  fam = REAL_FAMILIES.index((case.kname, case.mname))
  rng = np.random.default_rng([fam, case.n, case.M, 23])
  model = helpers.make_model(rng, case.mname, False, REAL_D)
  x, y = helpers.synthetic_task(rng, case.n, REAL_D)
  xq = rng.uniform(size=(case.M, REAL_D))
  kind = np.arange(case.M) % 3
  copies = np.flatnonzero(kind == 1)
  xq[copies] = x[rng.integers(0, case.n, size=len(copies))]
  far = np.flatnonzero(kind == 2)
  if case.kname == 'dot_product':
    xq[far] = xq[far] * np.where(np.arange(len(far)) % 2 == 0, 1e-2, 10.0)[:, None]
  else:
    po = o.GPParams(model=_cast(model, np.float64))
    ls, = o.retrieve_params(po, ['lengthscale'], warp_func=o.DEFAULT_WARP_FUNC)
    u = rng.normal(size=(len(far), REAL_D))
    xq[far] =xq[far] + 10.0 * np.asarray(ls).reshape(-1) * u / np.linalg.norm(u, axis=1, keepdims=True) * np.sqrt(REAL_D)
  dt = case.np_dtype
  out = _cast(model, dt), x.astype(dt), y.astype(dt), xq.astype(dt)
  for a in out[1:]:
    a.setflags(write=False)
  return out


@dataclasses.dataclass
class RealRef:
  mu: np.ndarray         # [M] the oracle's predict
  var: np.ndarray
  mu_scale: np.ndarray   # [M] |mu0_q| + sum_i |Kxq_iq alpha_i|
  var_scale: np.ndarray  # [M] kdiag_q + sum_i V_iq^2
  gap_mu: np.ndarray     # [M] |second route - oracle|
  gap_var: np.ndarray


@functools.lru_cache(maxsize=2)
def real_reference(case):
  """The fp64 oracle on the case's (for fp32: fp32-rounded) inputs, per query, with each query's own scales and the gap to a
  Cholesky-free second route (np.linalg.solve on K + noise).  Shared and read-only."""
  import scipy.linalg as spla
  from oracle import hyperbo_oracle as o
  wf = o.DEFAULT_WARP_FUNC
  model, x, y, xq = real_inputs(case)
  po = o.GPParams(model=_cast(model, np.float64))
  x, y, xq = (a.astype(np.float64) for a in (x, y, xq))
  mo, ko = getattr(o, case.mname), getattr(o, case.kname)
  mu, var = o.predict(mo, ko, po, x, y, xq, wf)
  chol, kinvy, ydelta = o.solve_gp_linear_system(mo, ko, po, x, y, wf)
  kxq = ko(po, x, xq, warp_func=wf)
  mu0 = np.asarray(mo(po, xq, warp_func=wf)).reshape(-1)
  kdiag = np.asarray(ko(po, xq, warp_func=wf, diag=True)).reshape(-1)
  v = spla.solve_triangular(chol, kxq, lower=True, check_finite=False)
  _, a = o.compute_delta_y_and_cov(mo, ko, po, x, y, wf)
  sol = np.linalg.solve(a, np.concatenate([ydelta, kxq], axis=1))
  # (the contractions over n in long double: the gap then shows the routes' difference, not the rounding of an unordered fp64 sum)
  ld = np.longdouble
  mu2 = ((kxq.astype(ld) * sol[:, :1].astype(ld)).sum(axis=0) + mu0).astype(np.float64)
  var2 = (kdiag - (kxq.astype(ld) * sol[:, 1:].astype(ld)).sum(axis=0)).astype(np.float64)
  mu, var = np.asarray(mu).reshape(-1), np.asarray(var).reshape(-1)
  ref = RealRef(mu, var, np.abs(mu0) + (np.abs(kxq) * np.abs(np.asarray(kinvy).reshape(-1, 1))).sum(axis=0), kdiag + (v * v).sum(axis=0),
                np.abs(mu2 - mu), np.abs(var2 - var))
  for arr in dataclasses.astuple(ref):
    arr.setflags(write=False)
  return ref
