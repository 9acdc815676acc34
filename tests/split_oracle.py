"""Host-side twin of the split-operand fp32 products (hyperbo_amd/csrc/post3.hip) and operands on which they are EXACT.

The emulation mirrors the device code: hbo_split3 (three round-to-nearest-even bf16 casts of the running remainder), hbo_split2h (two
fp16 casts of x * s), hbo_h2_scale_for / post2h_scale_for (the power of two that maps a bound into [2^13, 2^14)), and the retained
product from the planes in fp64 -- bf16x3 keeps the six pairs (i, j) with i + j <= 2, f16x2 keeps h h', h l', l h' and divides by the
two scales.  Nothing here rounds like an accumulator: the designs below are built so that every product and every partial sum is exact
in fp32, and the tests (tests/test_split_products_host.py) prove that before tests/test_gpu_split_products.py relies on it.

A design is a lower-triangular W [n, n], a Kxq [n, M] and the exact colsq[i, j] = sum over the rows r of 128-row block i of V[r, j]^2,
V = W Kxq.  `quantum` is the weight of the lowest bit any product of the design carries (after the f16x2 scales: in scaled units).
"""
import dataclasses

import numpy as np

TILE = 128
PAIRS3 = tuple((i, j) for i in range(3) for j in range(3) if i + j <= 2)   # bf16x3: a_i b_j retained
PAIRS2 = ((0, 0), (0, 1), (1, 0))                                            # f16x2: h h', h l', l h'


# ---- number formats ------------------------------------------------------------------------------------------------------------
def bf16_rne(x):
  """float32 -> nearest bfloat16 (ties to even), returned as float32.  Finite inputs."""
  b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
  b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
  return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def split3(x):
  """hbo_split3: x = x0 + x1 + x2, three bf16 numbers (as float32 arrays)."""
  x = np.asarray(x, dtype=np.float32)
  x0 = bf16_rne(x)
  r1 = (x - x0).astype(np.float32)
  x1 = bf16_rne(r1)
  r2 = (r1 - x1).astype(np.float32)
  return x0, x1, bf16_rne(r2)


def split2h(x, s):
  """hbo_split2h on x * s: h = fp16(x s), l = fp16(x s - h) (as float32 arrays), and the scaled value itself."""
  y = (np.asarray(x, dtype=np.float32) * np.float32(s)).astype(np.float32)
  with np.errstate(over='ignore'):
    h = y.astype(np.float16).astype(np.float32)
    l = (y - h).astype(np.float32).astype(np.float16).astype(np.float32)
  return h, l, y


def h2_scale_for(amax):
  """hbo_h2_scale_for: the power of two that maps amax into [2^13, 2^14); 1 for 0 / not finite; exponent clamped at -40."""
  amax = float(np.float32(amax))
  if not (amax > 0) or not np.isfinite(amax):
    return 1.0
  _, e = np.frexp(amax)
  return float(np.ldexp(1.0, 14 - max(int(e), -40)))


def post2h_scale_for(bound):
  """post2h_scale_for: the host-side twin (no clamp; 1 outside (0, 1e30))."""
  if not (bound > 0) or not (bound < 1e30):
    return 1.0
  _, e = np.frexp(float(bound))
  return float(np.ldexp(1.0, 14 - int(e)))


# ---- designs -------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Design:
  name: str
  form: str              # 'bf16x3' or 'f16x2'
  W: np.ndarray          # [n, n] float32, lower triangular
  K: np.ndarray          # [n, M] float32
  k_bound: float         # f16x2: the bound on |Kxq| the caller hands over
  quantum: float         # lowest bit of any product (f16x2: of the scaled operands' products)
  own: tuple = None      # pair designs: the one retained cross product V consists of
  exact: bool = True

  @property
  def n(self):
    return self.W.shape[0]

  @property
  def M(self):
    return self.K.shape[1]

  @property
  def pairs(self):
    return PAIRS3 if self.form == 'bf16x3' else PAIRS2


def npad_of(n):
  return (n + TILE - 1) // TILE * TILE


def _pad(d):
  n, np_ = d.n, npad_of(d.n)
  W = np.zeros((np_, np_), np.float32); W[:n, :n] = d.W
  K = np.zeros((np_, d.M), np.float32); K[:n] = d.K
  return W, K


def exact_V(d):
  """V = W Kxq in fp64: exact for every design here (products of few-bit numbers, sums far inside 53 bits)."""
  return d.W.astype(np.float64) @ d.K.astype(np.float64)


def colsq_of(V, n):
  """[nblk, M]: per 128-row block the column sums of V^2 (fp64)."""
  nblk = npad_of(n) // TILE
  Vp = np.zeros((nblk * TILE, V.shape[1])); Vp[:V.shape[0]] = V
  return (Vp.reshape(nblk, TILE, -1) ** 2).sum(axis=1)


def exact_colsq(d):
  return colsq_of(exact_V(d), d.n)


def design_dense(n, M, form='bf16x3', seed=0):
  """Small integers everywhere on and below the diagonal and in Kxq.  Both operands hold {1, 2} in the first 8 values of k of every
  16-block and {2, 3} in the last 8; Kxq carries a sign that is constant inside a 16-block and alternates from block to block.
  Every 16-block then contributes at least 16 + 32 in magnitude to every output of the rows that reach it, exchanging the halves of a
  block on one operand alone lowers every block's contribution systematically (1.5^2 + 2.5^2 against 2 * 1.5 * 2.5 per pair on
  average), and the alternating signs keep |V| -- and the 128-row sums of V^2, below 2^24 -- small.  Quantum 1 (f16x2, both
  operands scaled by 2^12: 2^24)."""
  rng = np.random.default_rng(seed)
  hi = ((np.arange(n) % 16) >= 8).astype(np.int64)
  W = np.tril(rng.integers(1, 3, size=(n, n)) + hi[None, :]).astype(np.float32)
  sign = np.where((np.arange(n) // 16) % 2 == 0, 1, -1)[:, None]
  K = ((rng.integers(1, 3, size=(n, M)) + hi[:, None]) * sign).astype(np.float32)
  return Design('dense', form, W, K, 3.0, 1.0 if form == 'bf16x3' else 2.0 ** 24)


def _pair_slots(n, rng, per_row=12, width=2):
  """For every row r up to `per_row` aligned groups of `width` adjacent k, all of them <= r, at most one per 16-block of k (both
  16-byte halves of a stage are used).  -> list of (r, k0) arrays."""
  rows, k0s = [], []
  for r in range(n):
    nfull = (r + 1) // 16                       # 16-blocks wholly at or below the diagonal
    blocks = list(range(nfull))
    rem = (r + 1) - 16 * nfull                  # k values of the diagonal 16-block that are <= r
    if rem >= width:
      blocks.append(nfull)
    if not blocks:
      continue
    pick = rng.choice(len(blocks), size=min(per_row, len(blocks)), replace=False)
    for b in np.asarray(blocks)[pick]:
      nslot = (16 if b < nfull else rem) // width
      rows.append(r); k0s.append(16 * b + width * rng.integers(0, nslot))
  return np.asarray(rows), np.asarray(k0s)


def design_pair(i, j, n, M, form='bf16x3', seed=0):
  """V consists of the cross product a_i b_j alone (a: planes of W, b: planes of Kxq); every other retained product cancels exactly
  inside every dot product.  Entries come in aligned pairs of adjacent k: the wide operand holds x and -y there, the narrow one the
  same small integer c in {+-1, +-2} twice, so that the pair contributes c (x - y) and the planes x and y share cancel:
    bf16x3 plane 2:  x = 1 + 2^-9 + s 2^-18, y = 1 + 2^-9 - s 2^-18   -> 2 c s 2^-18  (planes 0 and 1 equal, plane 2 = +-s 2^-18)
    bf16x3 plane 1:  x = 1 + s 2^-9,          y = 1 - s 2^-9           -> 2 c s 2^-9
    f16x2  l plane:  x = 1 + s 2^-12,         y = 1 - s 2^-12          -> 2 c s 2^-12
  (1, 1): aligned groups of four k, W = t (1+e, 1-e, 1+e, 1-e), Kxq = (1+se, 1-se, -(1-se), -(1+se)), e = 2^-9, t in {+-1, +-2}:
  a0 b0 = a0 b1 = a1 b0 = 0 and a1 b1 = 4 t s e^2.
  The wide operand is W for (p, 0) and Kxq for (0, p); never both at the same k (f16x2 drops l l' by design).
  Quantum: 2^-18 for the plane-2 and the (1, 1) designs, 2^-9 for plane 1; f16x2 in scaled units (W by 2^13, Kxq by 2^12 or
  2^13): 2^13."""
  rng = np.random.default_rng(seed + 17 * i + 5 * j)
  h2 = form == 'f16x2'
  assert (i, j) != (0, 0) and (i, j) in (PAIRS2 if h2 else PAIRS3)
  W = np.zeros((n, n), np.float64)
  K = np.zeros((n, M), np.float64)
  if (i, j) == (1, 1):
    e = 2.0 ** -9
    rows, k0 = _pair_slots(n, rng, width=4)
    t = rng.choice([-2, -1, 1, 2], size=rows.size)
    for q, f in enumerate((1 + e, 1 - e, 1 + e, 1 - e)):
      W[rows, k0 + q] = t * f
    s = rng.choice([-1.0, 1.0], size=((n + 3) // 4, M))[np.arange(n) // 4]          # one sign per group of four k and candidate
    sign = np.array([1, 1, -1, -1])[np.arange(n) % 4][:, None]
    u = np.array([1, -1, -1, 1])[np.arange(n) % 4][:, None]
    K = sign * (1 + u * s * e)
    return Design('pair(1,1)', form, W.astype(np.float32), K.astype(np.float32), 1 + e, 2.0 ** -18, own=(1, 1))
  p = max(i, j)
  if h2:
    lo, mid = 2.0 ** -12, 0.0
  else:
    lo, mid = (2.0 ** -18, 2.0 ** -9) if p == 2 else (2.0 ** -9, 0.0)
  rows, k0 = _pair_slots(n, rng, width=2)
  c = rng.choice([-2, -1, 1, 2], size=rows.size)
  if j == 0:   # W wide, Kxq narrow
    s = rng.choice([-1.0, 1.0], size=rows.size)
    W[rows, k0] = 1 + mid + s * lo
    W[rows, k0 + 1] = -(1 + mid - s * lo)
    Kh = rng.choice([-2, -1, 1, 2], size=((n + 1) // 2, M))
    K = np.repeat(Kh, 2, axis=0)[:n].astype(np.float64)            # the two rows of a pair are equal
    k_bound = 2.0
  else:        # Kxq wide, W narrow
    W[rows, k0] = c
    W[rows, k0 + 1] = c
    s = rng.choice([-1.0, 1.0], size=((n + 1) // 2, M))
    s2 = np.repeat(s, 2, axis=0)[:n]
    odd = (np.arange(n) % 2 == 1)[:, None]
    K = np.where(odd, -(1 + mid - s2 * lo), 1 + mid + s2 * lo)
    k_bound = 1 + mid + lo
  quantum = 2.0 ** 13 if h2 else lo
  return Design('pair(%d,%d)' % (i, j), form, W.astype(np.float32), K.astype(np.float32), k_bound, quantum, own=(i, j))


# the range design: what its numbers are (tests derive the bound from these and from post3.hip's header statement)
RANGE_BIG = 2.0 ** 18              # the one large entry of W; scale 2^-5 maps it to 2^13
RANGE_SMALL = (2.0 ** -2 + 2.0 ** -14) * 2.0 ** 5   # |typical entry| without its lowest bit
RANGE_LOST = 2.0 ** -25 * 2.0 ** 5                    # its lowest bit: half a subnormal fp16 step after scaling -- what the l plane loses


def design_range(n, M, seed=0):
  """f16x2 only, NOT exact.  One entry of W is 2^18, in a column of W whose row of Kxq is zero: it contributes nothing but sets the
  scale (2^-5: the split must take the maximum over ALL blocks, and the product must unscale by the same word).  The typical entries
  are +-2^5 (2^-2 + 2^-14 + t 2^-25), t = +-1: scaled, h = 2^-2, l = 2^-14 (the smallest normal fp16; the tie t 2^-25 rounds to
  even) and t 2^-25 is lost -- exactly the `absolute error <= 2^-25 against a largest entry of 2^13` of post3.hip's header.  Kxq is
  narrow ({+-1, +-2}), so h h' and l h' and all their partial sums are exact: the kernel's V is sum (2^-2 + 2^-14) 2^5 sgn c, and
  differs from the exact V by at most RANGE_LOST * sum_k |Kxq[k, j]| over the row's typical entries."""
  rng = np.random.default_rng(seed + 99)
  W = np.zeros((n, n), np.float64)
  rows, k0 = _pair_slots(n, rng, width=1)
  kbig, rbig = n - 2, n - 1
  keep = k0 != kbig
  rows, k0 = rows[keep], k0[keep]
  sg = rng.choice([-1.0, 1.0], size=rows.size); t = rng.choice([-1.0, 1.0], size=rows.size)
  W[rows, k0] = sg * (RANGE_SMALL + t * RANGE_LOST)
  W[rbig, kbig] = RANGE_BIG
  K = rng.choice([-2, -1, 1, 2], size=(n, M)).astype(np.float64)
  K[kbig] = 0
  return Design('range', 'f16x2', W.astype(np.float32), K.astype(np.float32), 2.0, 2.0 ** -14 * 2.0 ** 12, exact=False)


def range_bounds(d):
  """(kernel-side V the header's statement predicts, bound on |V_kernel - V_exact|): per typical entry the scaled value loses at most
  2^-25 absolutely, i.e. RANGE_LOST unscaled; the entry multiplies Kxq[k, j]."""
  Wt = d.W.astype(np.float64).copy()
  Wt[np.abs(Wt) >= RANGE_BIG] = 0
  dV = RANGE_LOST * ((Wt != 0).astype(np.float64) @ np.abs(d.K.astype(np.float64)))
  return dV


# ---- the retained product, with mutants ------------------------------------------------------------------------------------------
def planes_of(d):
  """(planes of W [npad, npad], planes of Kxq [npad, M], scale of W, scale of Kxq), planes as float64 arrays."""
  W, K = _pad(d)
  if d.form == 'bf16x3':
    return [p.astype(np.float64) for p in split3(W)], [p.astype(np.float64) for p in split3(K)], 1.0, 1.0
  sw, sk = h2_scale_for(np.abs(W).max()), post2h_scale_for(d.k_bound)
  return [p.astype(np.float64) for p in split2h(W, sw)[:2]], [p.astype(np.float64) for p in split2h(K, sk)[:2]], sw, sk


def emulate_V(d, mutant=None):
  """V [n, M] as the kernels form it: sum over the retained plane pairs of a_i b_j in fp64 (f16x2: divided by the scales).  mutant:
    ('drop', (i, j))           the retained cross product a_i b_j is left out
    ('swap_planes', op, p, q)  planes p and q of operand op ('W', 'K' or 'both') exchanged
    ('drop_kblock', where)     every row tile loses the first ('start') or last ('end') 16-block of its K range [0, 128 (R + 1))
    ('swap_halves', op, p)     the two 8-element halves of every 16-block of k exchanged on plane p of operand op only
    ('scale2', op)             f16x2: operand op is split with twice the scale the product divides by"""
  a, b, sw, sk = planes_of(d)
  pairs = list(d.pairs)
  kind = mutant[0] if mutant else None
  if kind == 'drop':
    pairs.remove(tuple(mutant[1]))
  elif kind == 'swap_planes':
    _, op, p, q = mutant
    if op in ('W', 'both'): a[p], a[q] = a[q], a[p]
    if op in ('K', 'both'): b[p], b[q] = b[q], b[p]
  elif kind == 'drop_kblock':
    npad = a[0].shape[0]
    for R in range(npad // TILE):
      k0 = 0 if mutant[1] == 'start' else TILE * (R + 1) - 16
      for pl in a: pl[R * TILE:(R + 1) * TILE, k0:k0 + 16] = 0
  elif kind == 'swap_halves':
    _, op, p = mutant
    perm = np.arange(a[0].shape[0]) ^ 8
    if op == 'W': a[p] = a[p][:, perm]
    else: b[p] = b[p][perm]
  elif kind == 'scale2':
    W, K = _pad(d)
    if mutant[1] == 'W': a = [p.astype(np.float64) for p in split2h(W, 2 * sw)[:2]]
    else: b = [p.astype(np.float64) for p in split2h(K, 2 * sk)[:2]]
  elif kind is not None:
    raise ValueError(mutant)
  V = sum(a[i] @ b[j] for i, j in pairs)
  return (V / (sw * sk))[:d.n]


def headroom_bits(d):
  """log2 of the largest magnitude any partial sum can reach, over the design's quantum, when the 16-blocks of k are taken in
  ascending order and the plane pairs and the k inside a block in ANY order: |sum of the blocks before| + sum over the block of
  sum_i |a_i| sum_j |b_j|  (an upper bound on every subset sum of the block's retained products).  Scaled units for f16x2."""
  a, b, _, _ = planes_of(d)
  A = sum(np.abs(p) for p in a); B = sum(np.abs(p) for p in b)
  full = sum(a[i] @ b[j] for i, j in d.pairs) * 0
  worst = 0.0
  prefix = full
  for kb in range(a[0].shape[0] // 16):
    sl = slice(16 * kb, 16 * kb + 16)
    worst = max(worst, float((np.abs(prefix) + A[:, sl] @ B[sl]).max()))
    prefix = prefix + sum(a[i][:, sl] @ b[j][sl] for i, j in d.pairs)
  return float(np.log2(worst / d.quantum)) if worst > 0 else 0.0


def is_fp32(x):
  x = np.asarray(x, dtype=np.float64)
  return bool(np.array_equal(x.astype(np.float32).astype(np.float64), x))


def killed_fraction(ref, mut, mask=None, rel=2.0 ** -10):
  """share of the (masked) outputs the mutant moves by at least `rel` relative to the reference"""
  hit = np.abs(mut - ref) >= rel * np.abs(ref)
  hit &= ref != 0
  if mask is not None:
    hit, n = hit[mask], int(mask.sum())
  else:
    n = hit.size
  return float(hit.sum()) / max(n, 1)


def all_designs(n, M, seed=0):
  """every design, in both forms where it applies"""
  out = [design_dense(n, M, 'bf16x3', seed), design_dense(n, M, 'f16x2', seed)]
  out += [design_pair(i, j, n, M, 'bf16x3', seed) for i, j in PAIRS3 if (i, j) != (0, 0)]
  out += [design_pair(i, j, n, M, 'f16x2', seed) for i, j in PAIRS2 if (i, j) != (0, 0)]
  return out


def _mm(*ms):
  """integer matrix product through fp64 BLAS (exact: every entry and partial sum here is far below 2^53)"""
  out = ms[0].astype(np.float64)
  for m in ms[1:]:
    out = out @ m.astype(np.float64)
  return np.rint(out).astype(np.int64)


# ---- matrices with exact factors (factorisation, inverse and K^-1 through hbo_spd_solve) ------------------------------------------
def exact_spd(n, seed=0, per_row=5):
  """A = L L^T with L unit lower triangular, off-diagonal entries sparse in {-1, 0, 1}.  Every index gets a class 0..3 and L[i, j]
  (j < i) may be non-zero only when class(j) < class(i): N = L - I then has no path longer than three, N^4 = 0, and
  W = L^-1 = I - N + N^2 - N^3 has small integer entries.  -> (A, L, W) as int64 arrays."""
  rng = np.random.default_rng(seed)
  cls = rng.integers(0, 4, size=n)
  N = np.zeros((n, n), np.int64)
  for i in range(1, n):
    cand = np.nonzero(cls[:i] < cls[i])[0]
    if cand.size:
      # (near and far columns: entries inside the diagonal block and in every block column to its left)
      pick = rng.choice(cand, size=min(per_row, cand.size), replace=False)
      N[i, pick] = rng.choice([-1, 1], size=pick.size)
  L = N + np.eye(n, dtype=np.int64)
  N2 = _mm(N, N)
  W = np.eye(n, dtype=np.int64) - N + N2 - _mm(N2, N)
  assert not _mm(N2, N2).any() and np.array_equal(_mm(L, W), np.eye(n, dtype=np.int64))
  return _mm(L, L.T), L, W


def sig_bits(x):
  """significant bits of the integers in x (0 for 0): position of the highest set bit minus that of the lowest, plus one"""
  x = np.abs(np.asarray(x, dtype=np.int64)).ravel()
  x = x[x != 0]
  if x.size == 0:
    return 0
  hi = np.floor(np.log2(x)).astype(np.int64)
  lo = np.log2(x & -x).astype(np.int64)
  return int((hi - lo + 1).max())


def spd_case(n, m, big_b=False, seed=0):
  """One exact hbo_spd_solve input: A = L L^T, right-hand sides b [n, m] (small integers, or integers near 2^10) and everything the
  call returns or forms on the way, as int64: W = L^-1, Kinv = W^T W, z = W b (the augmented rows after the factorisation),
  x = A^-1 b = W^T z."""
  A, L, W = exact_spd(n, seed)
  rng = np.random.default_rng(seed + 1000 + m)
  b = rng.integers(1000, 1048, size=(n, m)) * rng.choice([-1, 1], size=(n, m)) if big_b else rng.integers(-3, 4, size=(n, m))
  z = _mm(W, b)
  return dict(A=A, L=L, W=W, Kinv=_mm(W.T, W), b=b, z=z, x=_mm(W.T, z))


def spd_operand_report(case):
  """What the products of the factorisation, the inverse and K^-1 read and reach on `case`, for the fit conditions of the two forms:
  max significant bits of the factor-side operands (L, W, every level's S21 = L21 W11) and of z, and the largest magnitude any
  partial sum of any of the products can reach (sums of |.| |.|)."""
  L, W, z, b = (case[k] for k in ('L', 'W', 'z', 'b'))
  n = L.shape[0]
  nblk = npad_of(n) // TILE
  s21_bits, s21_max = 0, 0
  s = 1
  while s < nblk:
    for g in range(0, nblk, 2 * s):
      o, h = g * TILE, s * TILE
      if o + h >= n:
        continue
      S21 = _mm(L[o + h:o + 2 * h, o:o + h], W[o:o + h, o:o + h])
      s21_bits = max(s21_bits, sig_bits(S21)); s21_max = max(s21_max, int(np.abs(S21).max(initial=0)))
    s *= 2
  aL, aW, az = np.abs(L), np.abs(W), np.abs(z)
  reach = max(int(_mm(aL, aL.T).max()), int(_mm(aL, az).max() + np.abs(b).max()), int(_mm(aW.T, aW).max()), int(_mm(aW, aL, aW).max()),
              int(_mm(aW.T, az).max()))
  return dict(factor_bits=max(sig_bits(L), sig_bits(W), s21_bits), factor_max=max(int(aL.max()), int(aW.max()), s21_max),
              z_bits=sig_bits(z), z_max=int(az.max()), reach=reach, out_max=max(int(np.abs(case['Kinv']).max()), int(np.abs(case['x']).max())))
