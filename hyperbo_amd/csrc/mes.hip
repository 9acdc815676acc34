// Max-value entropy search (Wang & Jegelka 2017; include/hbo.h has the formulas): the entry points hbo_acq_mes, hbo_mes_grad_samples and
// hbo_mes_maximize, and the epilogue kernel of the first.  The one expression behind all three is kernfun.h: mes_terms.  Each entry point
// is its sibling's body under the request acq_what_mes (api_internal.h: AcqWhat): the values over a pool run through posterior()
// (cache.hip) with mes_epilogue_kernel behind post_epilogue_kernel's mean and variance; value + gradient and the maximiser are
// acq_grad_samples (acq_grad.hip) and acq_maximize (acq_opt.hip) on the blocked route, where the kernels of acq_small.hip /
// acq_blocked.hip take mes_scalars_block as their scalar step (kernfun.h: acq_scalar_step); everything around it is shared.
#include "kernfun.h"
#include "api_internal.h"
#include "../../include/hbo_tune.h"

namespace {
// a thread per query: mu and var as post_epilogue_kernel left them, v2 and sd in the model dtype as it forms them, the K terms in fp64 in
// index order, one rounding.  v2 <= 0: 0; a NaN v2 fails the compare and stays NaN.  (ystar is read at one address by the whole wave)
template <typename T>
__global__ __launch_bounds__(256) void mes_epilogue_kernel(const T* __restrict__ mu_in, const T* __restrict__ var_in, int64_t M,
                                                           const double* __restrict__ ystar, int K, double add_noise, double scale, T* out) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= M) return;
  const T mu = mu_in[q], var = var_in[q];
  const T v2 = (var + (T)add_noise) * (T)scale;
  const T sd = sqrt(v2);
  double val = 0.0;
  if (!(v2 <= (T)0)) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += mes_terms((ystar[k] - (double)mu) / (double)sd).h;
    val = s / K;
  }
  out[q] = (T)val;
}
}  // namespace

void launch_mes_epilogue(int dtype, const void* mu, const void* var, int64_t M, const double* ystar, int K, double add_noise, double scale,
                         void* out, hipStream_t st) {
  if (M <= 0) return;
  const dim3 grid((unsigned)((M + 255) / 256));
  if (dtype == HBO_F64)
    hipLaunchKernelGGL((mes_epilogue_kernel<double>), grid, dim3(256), 0, st, static_cast<const double*>(mu), static_cast<const double*>(var), M, ystar, K,
                       add_noise, scale, static_cast<double*>(out));
  else
    hipLaunchKernelGGL((mes_epilogue_kernel<float>), grid, dim3(256), 0, st, static_cast<const float*>(mu), static_cast<const float*>(var), M, ystar, K,
                       add_noise, scale, static_cast<float*>(out));
}

extern "C" int hbo_acq_mes(hbo_ctx* c, const hbo_model* m, hbo_cache* k, const void* xq, int64_t M, const double* ystar, int32_t K,
                           double add_noise, double scale, void* out) {
  const std::string fn = "hbo_acq_mes: ";
  if (!m || !xq || !ystar || !out) return fail(c, HBO_ERR_ARG, fn + "null argument");
  const AcqWhat what = acq_what_mes(ystar, K);
  if (int rc = acq_what_check(c, fn, what, 1)) return rc;
  if (!c) return fail(c, HBO_ERR_ARG, fn + "ctx is null");
  return posterior(c, m, k, xq, M, 0, nullptr, nullptr, out, what, add_noise, scale);
}

extern "C" int hbo_mes_grad_samples(hbo_ctx* c, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq, int64_t M,
                                    const double* ystar, int32_t K, const double* add_noise, double scale, void* acq_out, double* grad_out) {
  return acq_grad_samples(c, ACQ_ROUTE_BLOCKED.named("hbo_mes_grad_samples"), acq_what_mes(ystar, K), models, S, caches, xq, M, add_noise, scale,
                          acq_out, grad_out, nullptr);
}

// include/hbo_tune.h (TEST HOOK): hbo_mes_grad_samples with the fp64 values, the blocked kernels on request and a chunk size
extern "C" int hbo_probe_mes_grad_samples64(hbo_ctx* c, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq, int64_t M,
                                            const double* ystar, int32_t K, const double* add_noise, double scale, void* acq_out, double* grad_out,
                                            int32_t force_blocked, int64_t chunk_queries, double* val64_out) {
  if (int rc = acq_probe_check(c, "hbo_probe_mes_grad_samples64", val64_out, chunk_queries)) return rc;
  return acq_grad_samples(c, ACQ_ROUTE_BLOCKED.probed("hbo_mes_grad_samples", force_blocked, chunk_queries), acq_what_mes(ystar, K), models, S, caches,
                          xq, M, add_noise, scale, acq_out, grad_out, val64_out);
}

extern "C" int hbo_mes_maximize(hbo_ctx* c, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* x0, int32_t R,
                                const double* lo, const double* hi, const double* ystar, int32_t K, const double* add_noise, double scale,
                                const hbo_acq_opt_opts* opts, double* state, int32_t evals, double* x_out, double* val_out, int32_t* status,
                                hbo_acq_opt_eval* log) {
  return acq_maximize(c, ACQ_ROUTE_BLOCKED.named("hbo_mes_maximize"), acq_what_mes(ystar, K), models, S, caches, x0, R, lo, hi, add_noise, scale, opts,
                      state, evals, x_out, val_out, status, log);
}
