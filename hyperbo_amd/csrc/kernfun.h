// Device helpers shared by the elementwise / reduction kernels of the GP hot path (gram.hip, taskvec.hip, grad.hip, post.hip): the pair
// kernels of hyperbo/gp_utils/kernel.py:63-145 and their derivatives, LDS staging of feature blocks, the means of
// hyperbo/gp_utils/mean.py:30-79, block reductions, the normal pdf / cdf of the acquisition functions (acfun.py:96-142).
#pragma once
#include "hbo_internal.h"
#include <limits.h>
#include <math.h>

namespace {

template <typename T> struct V16;
template <> struct V16<double> { typedef double type __attribute__((ext_vector_type(2))); };
template <> struct V16<float> { typedef float type __attribute__((ext_vector_type(4))); };

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// sum over a 256-thread block; sred must hold 4 doubles. Result valid in every thread.
__device__ __forceinline__ double block_sum(double v, double* sred) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = v;
  __syncthreads();
  return sred[0] + sred[1] + sred[2] + sred[3];
}

// exp for the pair kernels (hyperbo/gp_utils/kernel.py:63-123: exp(-u/2), exp(-sqrt(3u)), exp(-sqrt(5u))): the Gram build and the
// gradient contraction are bound by their 32 / 64 fp64 exponentials per thread, and the library exp spends half of its ~40
// instructions on special cases these arguments never hit.  Cody-Waite reduction x = k ln2 + r (|r| <= 0.3466, ln2 split so that
// k * ln2_hi is exact), degree-13 Taylor polynomial in Horner form (truncation 4e-18), v_ldexp_f64 for 2^k: < 1.5 ulp on the
// arguments the kernels produce (tests/test_gpu_parity.py::test_device_exp_against_numpy), ~20 instructions.  Arguments below -746
// give 0 through the ldexp underflow; NaN stays NaN (the clamp is two compares, which a NaN fails; fmax / fmin would swallow it);
// large positive arguments are clamped (the kernels only pass x <= 0).
// Coefficients 1/13! ... 1/0! of the polynomial, held in VGPRs for the whole epilogue of a kernel (hbo_exp_coef once per thread):
// as literals they sit in scalar registers, and the compiler then evaluates Horner's p = p r + c with the two-address v_fmac_f64,
// whose accumulator must first be LOADED with c -- two v_mov_b32 per step, a fifth of the Gram kernel's instructions.  Against
// live vector registers it takes the three-address v_fma_f64.
struct ExpCoef { double c[14]; };
__device__ __forceinline__ ExpCoef hbo_exp_coef() {
  ExpCoef e = {{1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0,
                1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0}};
#pragma unroll
  for (int i = 0; i < 14; ++i) asm volatile("" : "+v"(e.c[i]));   // opaque: not folded back into literals
  return e;
}
// (the same polynomial with literal coefficients: kernels that have no 28 registers to spare for them, see grad_contract_kernel)
struct ExpLit {
  static constexpr double c[14] = {1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0,
                                   1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0};
};
template <typename C>
__device__ __forceinline__ double hbo_exp(double x, const C& ec) {
  x = x < -746.0 ? -746.0 : (x > 709.0 ? 709.0 : x);
  const double k = rint(x * 1.4426950408889634074);
  double r = fma(k, -6.93147180369123816490e-01, x);
  r = fma(k, -1.90821492927058770002e-10, r);
  double p = fma(ec.c[0], r, ec.c[1]);
#pragma unroll
  for (int i = 2; i < 14; ++i) p = fma(p, r, ec.c[i]);
  return ldexp(p, (int)k);
}
template <typename C>
__device__ __forceinline__ float hbo_exp(float x, const C&) { return expf(x); }

template <typename T, typename C>
__device__ __forceinline__ T kfun(int kid, T acc, T sv, T inv_sigma2, T bias2, const C& ec) {
  switch (kid) {
    case HBO_KERNEL_SE: return sv * hbo_exp((T)-0.5 * acc, ec);
    case HBO_KERNEL_MATERN32: { T r = sqrt((T)3 * acc); return sv * ((T)1 + r) * hbo_exp(-r, ec); }
    case HBO_KERNEL_MATERN52: { T r = sqrt((T)5 * acc); return sv * ((T)1 + r + r * r / (T)3) * hbo_exp(-r, ec); }
    default: return acc * inv_sigma2 + bias2;
  }
}
// d k / d u (u = scaled squared distance); 0 where u == 0 for Matern (linalg.py:183-188)
template <typename T, typename C>
__device__ __forceinline__ T dk_du(int kid, T u, T k, T sv, const C& ec) {
  switch (kid) {
    case HBO_KERNEL_SE: return (T)-0.5 * k;
    case HBO_KERNEL_MATERN32: { T r = sqrt((T)3 * u); return u == (T)0 ? (T)0 : -sv * (T)1.5 * hbo_exp(-r, ec); }
    case HBO_KERNEL_MATERN52: { T r = sqrt((T)5 * u); return u == (T)0 ? (T)0 : -sv * ((T)5 / (T)6) * hbo_exp(-r, ec) * ((T)1 + r); }
    default: return (T)0;
  }
}

// outer-product vectors of a task: (pointer, row stride, count)
template <typename T>
__device__ __forceinline__ const T* outer_vecs(const TaskDesc& t, int obj, int64_t& stride, int& count) {
  if (obj == OBJ_EUC) {
    if (t.nvec) { stride = t.npad; count = t.nvec - 1; return static_cast<const T*>(t.svec) + t.npad; }   // data rows in svec columns 1..m
    stride = t.ld; count = t.naug - 1;
    return static_cast<const T*>(t.A) + (int64_t)t.npad * t.ld;
  }
  stride = t.npad; count = t.nvec ? t.nvec : t.naug;
  return static_cast<const T*>(t.svec);
}

constexpr int DC = 16;     // feature chunk staged in LDS
constexpr int SXS = 132;   // LDS row stride of a staged [DC][128] block

// stage rows [r0, r0+128) x features [d0, d0+DC) of x (n x fdim) into s[dd][row], scaled
template <typename T, int NQ = 8>
__device__ __forceinline__ void stage_x(T* s, const T* __restrict__ x, int64_t n, int fdim, int64_t r0,
                                        int d0, const double* inv_ls, bool scale, int tid) {
  const int dd = tid & 15, rr0 = tid >> 4;
  const int d = d0 + dd;
  const bool dok = d < fdim;
  const T sc = (scale && dok) ? (T)inv_ls[d] : (T)1;
  // every load is issued -- from a clamped, always valid address -- before the first one is waited for: with the bounds test around the
  // load the compiler put each in a branch of its own with a full wait behind it (8 L2 round trips in a row per operand and chunk)
  const int dc = dok ? d : 0;
  T v[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int64_t row = r0 + rr0 + 16 * q;
    const int64_t rc = row < n ? row : (n > 0 ? n - 1 : 0);   // (callers never come here with n = 0: empty sub-datasets are skipped)
    v[q] = gld(x + rc * fdim + dc);
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int rr = rr0 + 16 * q;
    s[dd * SXS + rr] = (r0 + rr < n && dok) ? v[q] * sc : (T)0;
  }
}

template <typename T>
__device__ __forceinline__ T mean_at(const ModelDev* md, const T* fm, int fmean, int64_t i) {
  switch (md->mean_id) {
    case HBO_MEAN_ZERO: return (T)0;
    case HBO_MEAN_CONSTANT: return (T)md->constant;
    default: {
      T s = (T)md->linear_bias;
      for (int d = 0; d < fmean; ++d) s += fm[i * fmean + d] * (T)md->lin_w[d];
      return s;
    }
  }
}

// Gram / contraction tile = 64 rows x 128 columns per 256-thread workgroup, 4x8 register micro-tile per thread
// (an 8x8 micro-tile needs 256 VGPRs in fp64 -> 1 wave/SIMD and exposed exp/store latency).
constexpr int GRA = 4;            // rows per thread
constexpr int GTR = 16 * GRA;     // tile rows
__device__ __forceinline__ double norm_pdf(double x) { return exp(-0.5 * x * x) * 0.3989422804014327; }
__device__ __forceinline__ double norm_cdf(double x) { return 0.5 * erfc(-x * 0.7071067811865476); }
// EI / sd at u = (mu - target) / sd = -gamma: acfun.py:108-110, pdf(gamma) - gamma * (1 - cdf(gamma)), with 1 - cdf(gamma) taken as
// cdf(u) from erfc -- the literal 1 - cdf cancels (relative error 2e-3 at gamma = 7, negative values at 8).  The one expression behind
// the values of hbo_acq, hbo_acq_samples and hbo_acq_grad.  Floor at 0: where pdf is a denormal (gamma > 37.6) the two rounded terms can
// differ by a few quanta of either sign; a NaN (negative variance) stays a NaN.
__device__ __forceinline__ double ei_over_sd(double u) {
  const double e = norm_pdf(u) + u * norm_cdf(u);
  return e < 0.0 ? 0.0 : e;
}
// The scalar step of the acquisition gradient, from the posterior mean and variance at one query (acq_small.hip, acq_blocked.hip):
// the value, a_mu = d value / d mu and a_var = d value / d var (through sd = sqrt((var + add_noise) scale)).
struct AcqScalars { double val, amu, avar; };
__device__ __forceinline__ AcqScalars acq_scalars(int acq_id, double mu, double var, double add_noise, double scale, double param) {
  const double v2 = (var + add_noise) * scale;
  const double sd = sqrt(v2);
  double val, amu, asd;
  if (acq_id == HBO_ACQ_UCB) { val = mu + param * sd; amu = 1.0; asd = param; }
  else if (acq_id == HBO_ACQ_PI) { val = (mu - param) / sd; amu = 1.0 / sd; asd = -(mu - param) / (sd * sd); }
  else { const double uu = (mu - param) / sd; val = sd * ei_over_sd(uu); amu = norm_cdf(uu); asd = norm_pdf(uu); }
  AcqScalars r;
  r.val = val; r.amu = amu; r.avar = asd / (2.0 * sd) * scale;
  return r;
}

// Max-value entropy search (Wang & Jegelka 2017) for a maximised objective: one term of the mean over the sampled maxima y*_k, at
// gamma = (y*_k - mu) / sd, with r = pdf(gamma) / cdf(gamma):
//   h(gamma)  = gamma r / 2 - log cdf(gamma)            (>= 0, decreasing, h(+inf) = 0)
//   h'(gamma) = -(r / 2) (1 + gamma^2 + gamma r)
// The one expression behind hbo_acq_mes, hbo_mes_grad_samples and hbo_mes_maximize.  Neither side is evaluated literally:
//   gamma >= 0: cdf = 1 - q with q = cdf(-gamma) from erfc, log cdf = log1p(-q) (the literal log(cdf) is 0 from gamma = 8.3 on);
//               every term of h and of h' has one sign.  Where pdf underflows (gamma > 38.6) both are 0.
//   gamma < 0:  with t = -gamma / sqrt 2 and e = erfcx(t): r = sqrt(2 / pi) / e and log cdf = log(e / 2) - gamma^2 / 2.  r + gamma is
//               formed first (r ~ -gamma - 1 / gamma: the difference of two neighbours is exact), so h = gamma (r + gamma) / 2 - log(e / 2)
//               and h' = -(r / 2) (1 + gamma (r + gamma)) lose what the rounding of r costs at the scale gamma^2 r -- about 10 digits of
//               h' are left at gamma = -30, 14 at -8 -- and nothing more.
// gamma = -inf: (inf, -0), the limits; a NaN stays a NaN.  The floor at 0 guards the sign of h against the last rounding only.
struct MesTerms { double h, dh; };
__device__ __forceinline__ MesTerms mes_terms(double g) {
  MesTerms m;
  if (g < 0.0) {
    const double e = erfcx(-g * 0.7071067811865476);
    const double r = 0.7978845608028654 / e;
    const double rg = g * (r + g);
    m.h = 0.5 * rg - log(0.5 * e);
    m.dh = -0.5 * r * (1.0 + rg);
    if (g == -INFINITY) { m.h = INFINITY; m.dh = -0.0; }
  } else {
    // pdf(gamma) with gamma^2 = s + e taken exactly (e: the rounding of the square, from the fma): the rounded square alone costs
    // gamma^2 / 2 ulp of the pdf -- 700 at gamma = 37 -- and h' is that pdf times a positive factor
    const double s = g * g, e = fma(g, g, -s);
    const double q = norm_cdf(-g);
    const double r = exp(-0.5 * s) * (1.0 - 0.5 * e) * 0.3989422804014327 / (1.0 - q);
    m.h = 0.5 * g * r - log1p(-q);
    m.dh = -0.5 * r * (1.0 + s + g * r);
    if (r == 0.0 || g == INFINITY) m.dh = -0.0;   // (gamma = inf: inf * 0, and e = nan)
    if (g == INFINITY) m.h = 0.0;
  }
  if (m.h < 0.0) m.h = 0.0;
  return m;
}
// The scalar step of hbo_mes_grad_samples (acq_small.hip, acq_blocked.hip), by the whole 256-thread workgroup that owns the (sample, query)
// pair; every thread comes with the same mu and var and leaves with the same result:
//   value = (1 / K) sum_k h(gamma_k),  a_mu = -(1 / K) sum_k h'(gamma_k) / sd,  a_sd = -(1 / K) sum_k h'(gamma_k) gamma_k / sd,
// a_var from a_sd as acq_scalars forms it.  Thread k < K takes term k; the three sums then run in index order, one thread each, whatever
// K is.  v2 = (var + add_noise) scale <= 0: no posterior uncertainty, no information -- value and both slopes are 0 (a NaN would win
// an argmax); a NaN v2 stays NaN.  s_t: [3][HBO_MES_MAX_K] doubles of LDS, s_sum: [3].  Holds barriers: call it from uniform code.
__device__ __forceinline__ AcqScalars mes_scalars_block(double mu, double var, double add_noise, double scale, const double* ystar, int K,
                                                         double* s_t, double* s_sum) {
  const int tid = threadIdx.x;
  const double v2 = (var + add_noise) * scale;
  AcqScalars r;
  r.val = 0.0; r.amu = 0.0; r.avar = 0.0;
  if (v2 <= 0.0) return r;   // (uniform: every thread holds the same v2)
  const double sd = sqrt(v2);
  if (tid < K) {
    const double g = (ystar[tid] - mu) / sd;
    const MesTerms m = mes_terms(g);
    s_t[tid] = m.h; s_t[HBO_MES_MAX_K + tid] = m.dh; s_t[2 * HBO_MES_MAX_K + tid] = m.dh * g;
  }
  __syncthreads();
  if (tid < 3) {
    const double* t = s_t + tid * HBO_MES_MAX_K;
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += t[k];
    s_sum[tid] = s;
  }
  __syncthreads();
  const double asd = -(s_sum[2] / K) / sd;
  r.val = s_sum[0] / K; r.amu = -(s_sum[1] / K) / sd; r.avar = asd / (2.0 * sd) * scale;
  return r;
}

// Log expected improvement (Ament et al. 2023) at u = (mu - target) / sd, with h(u) = pdf(u) + u cdf(u) = EI / sd: log h and the two
// ratios cdf / h and pdf / h, from which the value log sd + log h and its slopes a_mu = (cdf / h) / sd, a_sd = (pdf / h) / sd follow.
// The one expression behind hbo_acq_logei, hbo_logei_grad_samples and hbo_logei_maximize.
//   u > -1:       literally, pdf and cdf from erfc as ei_over_sd takes them; nothing cancels by more than a factor of about 5.
//   u <= -1:      with e = erfcx(-u / sqrt 2): Mills ratio m = cdf / pdf = sqrt(pi / 2) e, w = h / pdf = 1 + u m, and
//                 log h = -u^2 / 2 - log sqrt(2 pi) + log w, cdf / h = m / w, pdf / h = 1 / w.  w falls like 1 / u^2 and the sum 1 + u m
//                 cancels: a relative error of about eps u^2 in w, the accepted loss.
//   u < -LOGEI_SERIES_U: the asymptotic series  w u^2 = 1 - 3 / u^2 + 15 / u^4 - 105 / u^6,  m |u| = 1 - 1 / u^2 + 3 / u^4 - 15 / u^6
//                 (first term left out: 945 / u^8 < 2^-54 from |u| = 235 on), exact to eps where the form above has lost eps u^2 --
//                 4 digits at the switch, everything from |u| = 6.7e7 on, where w rounds to 0.  Finite for every finite u whose
//                 square does not overflow.
// u = +inf: (inf, 0, 0); u = -inf: (-inf, inf, inf), the limits; a NaN stays a NaN.
#define LOGEI_SERIES_U 256.0
struct LogEiTerms { double logh, cdf_h, pdf_h; };
__device__ __forceinline__ LogEiTerms logei_terms(double u) {
  LogEiTerms r;
  if (u > -1.0) {
    const double p = norm_pdf(u), c = norm_cdf(u);
    const double h = p + u * c;
    r.logh = log(h); r.cdf_h = c / h; r.pdf_h = p / h;
  } else if (u >= -LOGEI_SERIES_U) {
    const double m = 1.2533141373155003 * erfcx(-u * 0.7071067811865476);
    const double w = 1.0 + u * m;
    r.logh = -0.5 * u * u - 0.9189385332046727 + log(w);
    r.cdf_h = m / w; r.pdf_h = 1.0 / w;
  } else {
    const double i2 = 1.0 / (u * u);
    const double ws = 1.0 + i2 * (-3.0 + i2 * (15.0 - 105.0 * i2));   // w u^2
    const double ms = 1.0 + i2 * (-1.0 + i2 * (3.0 - 15.0 * i2));    // m |u|
    r.logh = -0.5 * u * u - 0.9189385332046727 + (log(ws) - 2.0 * log(-u));
    r.cdf_h = -u * (ms / ws); r.pdf_h = u * u / ws;
  }
  return r;
}
// The scalar step of hbo_logei_grad_samples, per thread like acq_scalars: value = log sd + log h(u), a_mu = (cdf / h) / sd,
// a_var = (pdf / h) / sd / (2 sd) * scale.  v2 = (var + add_noise) scale <= 0 (no posterior uncertainty): EI = max(mu - target, 0), so
// value = log(mu - target), a_mu = 1 / (mu - target), a_var = 0 above the target and (-inf, 0, 0) at or below it -- -inf loses every
// argmax, and the maximiser's line search rejects it.  A NaN v2 fails the compare and stays NaN.  Wherever the value is -inf both slopes
// are 0: such a row has weight exp(-inf) = 0 in the combination over an HGP's samples, and 0 times an infinite slope would be a NaN.
__device__ __forceinline__ AcqScalars logei_scalars(double mu, double var, double add_noise, double scale, double target) {
  const double v2 = (var + add_noise) * scale;
  AcqScalars r;
  if (v2 <= 0.0) {
    const double d = mu - target;
    r.avar = 0.0;
    if (d > 0.0) { r.val = log(d); r.amu = 1.0 / d; }
    else if (d <= 0.0) { r.val = -INFINITY; r.amu = 0.0; }
    else { r.val = NAN; r.amu = NAN; }
    return r;
  }
  const double sd = sqrt(v2);
  const LogEiTerms t = logei_terms((mu - target) / sd);
  r.val = log(sd) + t.logh; r.amu = t.cdf_h / sd; r.avar = t.pdf_h / sd / (2.0 * sd) * scale;
  if (r.val == -INFINITY) { r.amu = 0.0; r.avar = 0.0; }   // (u^2 overflows: the same rule -- a -inf row carries no slope into a sum)
  return r;
}
// The scalar step of a (sample, query) pair's 256-thread workgroup in acq_small_kernel and acq_blk_finish_kernel, by STEP
// (hbo_internal.h: ACQ_STEP_*): acq_scalars by a.acq_id or logei_scalars on thread 0, against sm.param, handed over through LDS behind a
// barrier; mes_scalars_block over the sample's K maxima by the whole workgroup.  Thread 0 writes the value to *acq (model dtype) and to
// a.val64_out where that is set; every thread leaves with the same amu, avar.  Call it from uniform code.  The MES step returns WITHOUT
// a barrier behind its LDS when v2 <= 0: the caller places one before it reuses LDS of its own.
// (`a` by value: a reference to acq_small_kernel's own argument costs its plain instantiations 4 VGPRs and a wave of occupancy)
template <typename T, int STEP>
__device__ __forceinline__ void acq_scalar_step(const AcqSmallArgs a, const AcqSmallSample& sm, int s, int64_t q, double mu, double var, T* acq,
                                                double& amu, double& avar) {
  const int tid = threadIdx.x;
  if constexpr (STEP == ACQ_STEP_MES) {
    __shared__ double s_mes[3 * HBO_MES_MAX_K], s_mes_sum[3];
    const AcqScalars sc = mes_scalars_block(mu, var, sm.add_noise, a.scale, a.ystar + (int64_t)s * a.K, a.K, s_mes, s_mes_sum);
    if (tid == 0) {
      *acq = (T)sc.val;
      if (a.val64_out) a.val64_out[(int64_t)s * a.M + q] = sc.val;
    }
    amu = sc.amu; avar = sc.avar;   // (every thread holds them: nothing is handed over through LDS)
  } else {
    __shared__ double s_amu, s_avar;
    if (tid == 0) {   // (STEP is a constant: one of the two is compiled)
      const AcqScalars sc = STEP == ACQ_STEP_LOGEI ? logei_scalars(mu, var, sm.add_noise, a.scale, sm.param)
                                                   : acq_scalars(a.acq_id, mu, var, sm.add_noise, a.scale, sm.param);
      s_amu = sc.amu; s_avar = sc.avar;
      *acq = (T)sc.val;
      if (a.val64_out) a.val64_out[(int64_t)s * a.M + q] = sc.val;
    }
    __syncthreads();
    amu = s_amu; avar = s_avar;
  }
}
}  // namespace
