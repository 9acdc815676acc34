/*
 * hbo.h -- C ABI of libhbo: MI355X-native (gfx950) implementation of HyperBO's GP hot path.
 *
 * The reference (google-research/hyperbo) has no FFI: the path sits behind plain Python
 * callables traced by JAX.  Each entry point below names the reference callable it replaces
 * (file:line relative to the reference repo root); hyperbo_amd/ binds them with ctypes and
 * re-exposes the reference's Python signatures.
 *
 * Conventions
 *   - all host arrays are C-contiguous row-major, element type = hbo_model.dtype
 *     (HBO_F32 -> float, HBO_F64 -> double); gradients and NLL values are always double.
 *   - every function returns an int status: 0 ok, <0 usage/runtime error, >0 numerical
 *     (HBO_NOT_PD: the jittered Gram matrix was not positive definite; outputs are NaN-filled,
 *     mirroring jax.scipy.linalg.cholesky which yields NaNs instead of raising).
 *   - never aborts, never throws across the ABI; hbo_last_error(ctx) returns a message.
 *   - a ctx is not re-entrant; use one ctx per GPU / per thread.  Calls are synchronous.
 *   - hyper-parameters in hbo_model are ALREADY WARPED (softplus etc. stay in Python so that
 *     arbitrary warp_func dicts keep working: hyperbo/basics/params_utils.py:97-111).
 */
#ifndef HBO_H_
#define HBO_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HBO_OK 0
#define HBO_ERR_ARG (-1)
#define HBO_ERR_HIP (-2)
#define HBO_ERR_NODEV (-3)
#define HBO_ERR_UNSUPPORTED (-4)
#define HBO_ERR_COMM (-5)
#define HBO_NOT_PD 1
#define HBO_NOT_CONVERGED 2   /* hbo_sym_eig / hbo_nll_spectral: the sweep cap was hit or the input held NaN / inf (outputs NaN-filled) */

/* closed registries: hyperbo/bo_utils/const.py:22-50 */
enum hbo_kernel_id { HBO_KERNEL_SE = 0, HBO_KERNEL_MATERN32 = 1, HBO_KERNEL_MATERN52 = 2, HBO_KERNEL_DOT = 3 };
enum hbo_mean_id { HBO_MEAN_ZERO = 0, HBO_MEAN_CONSTANT = 1, HBO_MEAN_LINEAR = 2, HBO_MEAN_LINEAR_MLP = 3 };
enum hbo_dtype { HBO_F32 = 0, HBO_F64 = 1 };
enum hbo_acq_id { HBO_ACQ_EI = 0, HBO_ACQ_PI = 1, HBO_ACQ_UCB = 2 };

#define HBO_MAX_MLP_LAYERS 8
#define HBO_MAX_FEATURE_DIM 256

typedef struct hbo_ctx hbo_ctx;
typedef struct hbo_dataset hbo_dataset; /* device-resident sub-datasets (x, y) */
typedef struct hbo_cache hbo_cache;     /* device-resident GPCache: x, chol, chol^-1, kinvy */

/* Model descriptor: kernel (hyperbo/gp_utils/kernel.py:63-183), mean (gp_utils/mean.py:54-79),
 * MLP basis (gp_utils/basis_functions.py:24-36, flax Dense: y = x @ kernel + bias, tanh on every
 * layer) and the jitter eps of hyperbo/basics/linalg.py:42,78 (default 1e-6). */
typedef struct hbo_model {
  int32_t kernel_id;        /* hbo_kernel_id */
  int32_t mean_id;          /* hbo_mean_id */
  int32_t dtype;            /* hbo_dtype */
  int32_t input_dim;        /* D */
  int32_t kernel_uses_mlp;  /* 1: base kernel evaluated on MLP features (kernel.py:148-183) */
  int32_t n_layers;         /* MLP depth (0 if unused) */
  int32_t features[HBO_MAX_MLP_LAYERS]; /* params.config['mlp_features'] */
  int32_t n_lengthscale;    /* 1 (broadcast) or the kernel's feature dimension */
  int32_t input_warp;       /* 0: none; HBO_WARP_KUMAR: the pointer is really an hbo_model_kumar (below) */
  double eps;
  double signal_variance;
  double noise_variance;
  double constant;          /* mean.constant */
  double dot_prod_sigma;
  double dot_prod_bias;
  double linear_bias;       /* linear_mean['bias'] */
  const void* lengthscale;                       /* [n_lengthscale] */
  const void* mlp_kernel[HBO_MAX_MLP_LAYERS];    /* [in, out] row-major */
  const void* mlp_bias[HBO_MAX_MLP_LAYERS];      /* [out] */
  const void* linear_kernel;                     /* [Fin] (linear_mean['kernel'][:,0]) */
} hbo_model;

/* Kumaraswamy input warping (hyperbo/gp_utils/kernel.py:186-222 with_kumar_bases, basis_functions.py:48-70 KumarWarp): the
 * *_kumar kernels evaluate the base kernel on w(x) = 1 - (1 - x^a)^b, per input column, a = squareplus(a_raw),
 * b = squareplus(b_raw) (utils.py:59-71; the squareplus stays with the caller, as every other warp).  Only the covariance sees w(x):
 * a linear mean still reads the raw x, as in the reference.  Inputs are not clamped (x < 0 gives NaN, as the formula does).
 *   An hbo_model with input_warp = HBO_WARP_KUMAR is the first member of an hbo_model_kumar; kumar_a / kumar_b hold input_dim
 *   elements of the model dtype each, ALREADY squareplus-warped.  Exactly a == 1 evaluates x^a as x and exactly b == 1 evaluates
 *   w as x^a (1 - (1 - u) == u in exact arithmetic), so raw zeros give the plain kernel bit for bit.
 *   Not supported (HBO_ERR_UNSUPPORTED): together with kernel_uses_mlp (not a reference combination), any other input_warp value,
 *   and hbo_acq_samples / hbo_acq_grad_samples.
 *   Gradient: the layout of such a model ends with 2 D more doubles, d/da at [total - 2D, total - D) and d/db at [total - D, total)
 *   (hbo_grad_layout_kumar_of), summed over rows and tasks in a fixed order (per-workgroup partials, one ordered finalisation):
 *   dw/da = b (1 - x^a)^(b-1) x^a ln x,  dw/db = -(1 - x^a)^b ln(1 - x^a).  At x = 0 and x = 1 both are DEFINED as their limit 0
 *   (a deliberate choice: 0 ln 0 never enters the sum; the reference's autodiff value at these endpoints has not been compared).
 *   hbo_acq_grad chains d acq / d w(x) with dw/dx = a b x^(a-1) (1 - x^a)^(b-1), evaluated as written in the model dtype. */
#define HBO_WARP_NONE 0
#define HBO_WARP_KUMAR 1
typedef struct hbo_model_kumar {
  hbo_model base;
  const void* kumar_a;   /* [input_dim], squareplus(a_raw) */
  const void* kumar_b;   /* [input_dim], squareplus(b_raw) */
} hbo_model_kumar;

/* Flat layout (in doubles) of the gradient w.r.t. the WARPED parameters written by hbo_nll / hbo_objective.
 * Offsets of absent parameters are -1.  total = number of doubles (for a Kumaraswamy model: including the 2 D doubles of a, b
 * at the end, which this struct has no field for -- hbo_grad_layout_kumar_of). */
typedef struct hbo_grad_layout {
  int32_t lengthscale;      /* n_lengthscale entries */
  int32_t signal_variance;
  int32_t noise_variance;
  int32_t constant;
  int32_t dot_prod_sigma;
  int32_t dot_prod_bias;
  int32_t linear_kernel;    /* Fin entries */
  int32_t linear_bias;
  int32_t mlp_kernel[HBO_MAX_MLP_LAYERS]; /* in*out entries each, row-major [in,out] */
  int32_t mlp_bias[HBO_MAX_MLP_LAYERS];
  int32_t total;
} hbo_grad_layout;

typedef struct hbo_task {
  const void* x; /* [n, input_dim] */
  const void* y; /* [n, m] */
  int64_t n;
  int32_t m;
  int32_t reserved0;
} hbo_task;

/* ---- context ------------------------------------------------------------------------- */
int hbo_ctx_create(int device, hbo_ctx** out);
int hbo_ctx_destroy(hbo_ctx* ctx);
const char* hbo_last_error(hbo_ctx* ctx); /* ctx may be NULL: last error of ctx-less calls */
const char* hbo_version(void);
int hbo_device_count(void);
/* name_out (nullable, cap bytes): marketing / arch name of the device; cus / mem_bytes (nullable): compute units, device memory */
int hbo_device_info(int device, char* name_out, int32_t cap, int32_t* cus, int64_t* mem_bytes);

int hbo_grad_layout_of(const hbo_model* model, hbo_grad_layout* out);
/* offsets of d/da and d/db (input_dim doubles each) in the gradient of a Kumaraswamy model; -1 / -1 for a model without warp */
int hbo_grad_layout_kumar_of(const hbo_model* model, int32_t* a_off, int32_t* b_off);

/* ---- kernel.py:33-58 cov_func(params, vx1, vx2=None, diag=False) ------------------------ */
/* out: [n1,n2] (x2 may be NULL -> x2 = x1), or [n1] when diag != 0 (requires x2 == NULL). */
int hbo_gram(hbo_ctx* ctx, const hbo_model* model, const void* x1, int64_t n1, const void* x2,
             int64_t n2, int diag, void* out);
/* ---- mean.py:34-49 mean_func(params, vx) -> [n,1] -------------------------------------- */
int hbo_mean(hbo_ctx* ctx, const hbo_model* model, const void* x, int64_t n, void* out);

/* ---- objectives.py:109-210 neg_log_marginal_likelihood + its jax.value_and_grad
 *      (gp.py:134, lbfgs.py:238) over device-resident sub-datasets ------------------------ */
int hbo_dataset_create(hbo_ctx* ctx, int dtype, int input_dim, const hbo_task* tasks, int n_tasks,
                       hbo_dataset** out);
int hbo_dataset_free(hbo_ctx* ctx, hbo_dataset* ds);
/* A random sub-sample of a resident dataset, drawn by the caller, gathered on the device: what every Adam step of
 * infer_parameters does with sub_sample_dataset_iterator (hyperbo/gp_utils/gp.py:101-111, hyperbo/basics/data_utils.py:72-100;
 * the reference indexes device arrays with jax.random.permutation).  Task k of `src` IN THE ORDER src HOLDS THEM (largest n first,
 * stable in the order of hbo_dataset_create's `tasks`) keeps counts[k] rows: rows idx[off_k + r], r < counts[k], off_k = sum of the
 * non-negative counts before k -- or all of its rows, in order, when counts[k] < 0 (no indices consumed).  Only the indices travel
 * (4 bytes per kept row); the new dataset is independent of `src` afterwards. */
int hbo_dataset_subsample(hbo_ctx* ctx, const hbo_dataset* src, const int64_t* counts, const int32_t* idx, hbo_dataset** out);
/* nll_sum: sum over the tasks of this dataset of the per-task Cholesky NLL (objectives.py:144-156,
 * incl. the (m,m)+scalar broadcast quirk for m>1); the caller divides by the number of tasks
 * (objectives.py:192-195) -- a sum so that task shards on different GPUs can be all-reduced.
 * nll_per_task (nullable): [n_tasks].  grad_sum (nullable): [layout.total] sum over tasks of
 * d nll_task / d warped-parameter.  Returns HBO_NOT_PD if any task failed (its values are NaN). */
int hbo_nll(hbo_ctx* ctx, const hbo_model* model, hbo_dataset* ds, double* nll_sum,
            double* nll_per_task, double* grad_sum);

/* ---- objectives.py:29-106 multivariate_normal_divergence (+ jax.value_and_grad) over the ALIGNED
 *      sub-datasets of `ds`: distance between N(mean_a y, cov_a y) of the m aligned columns and the GP prior
 *      N(mean_func(x), cov_func(x,x) + noise I) -- no jitter, model->eps is ignored.
 *        HBO_OBJ_NLL  = hbo_nll
 *        HBO_OBJ_EKL  utils.py:84-148 kl_multivariate_normal(partial=True, eps=0, weight=1)  ('ekl' / 'kl')
 *        HBO_OBJ_EUC  utils.py:151-173 euclidean_multivariate_normal(mean_weight=cov_weight=1) ('euc')
 *      Same output convention as hbo_nll (sums over tasks; the caller divides by the task count,
 *      objectives.py:98-101).  Any number m of aligned columns: up to 127 ride through the factorisation as augmented rows, beyond
 *      that the data rows go through the explicit inverse (objective.hip: extra_rows). */
enum hbo_objective_id { HBO_OBJ_NLL = 0, HBO_OBJ_EKL = 1, HBO_OBJ_EUC = 2 };
int hbo_objective(hbo_ctx* ctx, const hbo_model* model, hbo_dataset* ds, int objective, double* value_sum,
                  double* value_per_task, double* grad_sum);

/* ---- linalg.py:72-110 solve_gp_linear_system -> GPCache(chol, kinvy) (gp.py:540-560) ----- */
int hbo_factor(hbo_ctx* ctx, const hbo_model* model, const void* x, int64_t n, const void* y,
               int32_t m, hbo_cache** out);
/* chol_out [n,n] (lower, zeros above the diagonal), kinvy_out [n,m], y_minus_mu_out [n,m];
 * any may be NULL. */
int hbo_cache_export(hbo_ctx* ctx, hbo_cache* cache, void* chol_out, void* kinvy_out,
                     void* y_minus_mu_out);
int hbo_cache_free(hbo_ctx* ctx, hbo_cache* cache);
/* O(N^2) in-place append of n_new observations (x_new [n_new, D], y_new [n_new, m]) to a cache built with the
 * SAME hyper-parameters -- what GP.update_sub_dataset(is_append=True) + setup_predictor recompute from
 * scratch in the reference (gp.py:426-452,540-560; "One can potentially support rank-1 updates", gp.py:284).
 * HBO_ERR_UNSUPPORTED: padded capacity exhausted, re-factorise with hbo_factor. */
int hbo_cache_append(hbo_ctx* ctx, const hbo_model* model, hbo_cache* cache, const void* x_new, int64_t n_new,
                     const void* y_new);

/* ---- gp.py:242-305 predict ------------------------------------------------------------- */
/* cache == NULL -> prior branch (gp.py:275-282).  mu_out [M,1]; var_out [M,1] or [M,M] if
 * full_cov.  No noise / unbiased scaling here (that is GP.predict, gp.py:607-619). */
int hbo_predict(hbo_ctx* ctx, const hbo_model* model, hbo_cache* cache, const void* xq, int64_t M,
                int full_cov, void* mu_out, void* var_out);
/* ---- acfun.py:51-142 acquisition on top of GP.predict(full_cov=False) ------------------- */
/* var' = (var + add_noise) * scale (gp.py:607-619); EI/PI: param = target; UCB: param = beta.
 * EI equals the reference's formula (acfun.py:108-110), evaluated without its `1 - cdf(gamma)` cancellation (cdf(-gamma) from erfc):
 * it differs from a literal evaluation only where that one has lost its digits (gamma = (target - mu) / sd > ~5 in fp64). */
int hbo_acq(hbo_ctx* ctx, const hbo_model* model, hbo_cache* cache, const void* xq, int64_t M,
            int acq_id, double param, double add_noise, double scale, void* out);

/* ---- S posterior sample paths over one shared basis of F features (pathwise / Matheron sampling; no counterpart in the reference,
 *      whose only joint draw is predict(full_cov=True): M^2 memory and an M^3 factorisation on top).  With phi(x) what the covariance
 *      sees (the raw x, the last MLP layer, the Kumaraswamy-warped x; width fdim), m the mean function and Ktilde the matrix the cache
 *      factorised, k(X,X) + (noise_variance + eps) I:
 *        SE / Matern, A = sqrt(2 signal_variance / F):   p_s(x) = A sum_j w[j,s] cos(omega_j . phi(x) + phase_j)
 *        dot product (F = fdim + 1, exact; omega, phase unused): p_s(x) = sum_d w[d,s] phi_d(x) / dot_prod_sigma + dot_prod_bias w[fdim,s]
 *        v[:,s] = Ktilde^-1 (y - m(X) - p_s(X) - sqrt(noise_variance + eps) eps[:,s])
 *        out[q,s] = m(x_q) + p_s(x_q) + sum_i k(x_q, X_i) v[i,s]          (cache == NULL, the prior branch: m(x_q) + p_s(x_q))
 *      out is the latent, noise-free function; with w = 0 and eps = 0 it is hbo_predict's mean.  The caller draws omega [F,fdim]
 *      (already divided by the lengthscale: the device never sees it for the prior term), phase [F], w [F,S] and eps [n,S] (NULL if and
 *      only if cache is NULL), all in the model dtype (hyperbo_amd/gp_utils/pathwise.py holds the spectral recipe); out [M,S], model
 *      dtype.  Cost: one O(n^2) solve per path, then O(M (F + n)) per path; every cosine and every cross-Gram entry is shared by the S
 *      paths.  Queries stream in chunks of post_chunk; a row of out does not depend on the chunk size, a column not on the other columns
 *      of the call, and identical calls are bit-identical (fp64 sums in a fixed order, no atomics).
 *      HBO_ERR_ARG, before any device call and with out untouched: a null ctx or argument, S outside 1..1024, F outside 1..65536, a
 *      dot-product model with F != fdim + 1, eps without a cache or a cache without eps, a cache/model mismatch.  A cache that is not
 *      positive definite: out is NaN, HBO_NOT_PD (as hbo_predict). */
int hbo_sample_paths(hbo_ctx* ctx, const hbo_model* model, hbo_cache* cache /* nullable */, const void* xq, int64_t M, int32_t S, int32_t F,
                     const void* omega, const void* phase, const void* w, const void* eps, void* out);

/* ---- value and d/dx of those paths at single points (csrc/path_opt.hip).  With c = dev_scale, the factor the deviation of a path
 *      from the posterior mean is scaled by (GP.sample_paths' unbiased sqrt(T / (T - 1)); 1 gives hbo_sample_paths' paths):
 *        f_s(x) = m(x) + c p_s(x) + sum_i k(x, X_i) u[i,s],   u[:,s] = Ktilde^-1 (y - m(X) - c p_s(X) - c sqrt(noise_variance + eps) eps[:,s])
 *        SE / Matern:  df_s/dx_d = -c A sum_j w[j,s] sin(omega_j . x + phase_j) omega_jd + sum_i u[i,s] dk/du_i 2 (x_d - X_id) / ls_d^2
 *                      (a Matern pair at zero distance contributes 0, as hbo_acq_grad)
 *        dot product:  df_s/dx_d = c w[d,s] / dot_prod_sigma + sum_i u[i,s] X_id / dot_prod_sigma^2;   a linear mean adds its weight d.
 *      u comes from the solve of hbo_sample_paths; after it a point costs O(F D + n D) per path and needs no factor: no limit on n, and
 *      the prior branch (cache == NULL) is served.  The features are the raw x.  xq [M, input_dim], the draws and eps as
 *      hbo_sample_paths; out [M,S] (model dtype), grad_out [M,S,input_dim] doubles.  One workgroup per (query, path) pair; sine and
 *      cosine in the model dtype, every sum in fp64 in an order fixed by (n, F, input_dim) alone, no atomics: an entry does not depend
 *      on the queries and paths that share the call (bit for bit), and identical calls are bit-identical.
 *      HBO_ERR_ARG, before any device call and with the outputs untouched: those of hbo_sample_paths, and a dev_scale that is not
 *      finite or not > 0.  HBO_ERR_UNSUPPORTED (before any device work; these stay with hbo_sample_paths): kernel_uses_mlp, a
 *      linear_mlp mean, an input-warped (Kumaraswamy) model.  A cache that is not positive definite: out and grad_out are NaN,
 *      HBO_NOT_PD.  M == 0 returns HBO_OK. */
int hbo_sample_paths_grad(hbo_ctx* ctx, const hbo_model* model, hbo_cache* cache /* nullable */, const void* xq, int64_t M, int32_t S,
                          int32_t F, const void* omega, const void* phase, const void* w, const void* eps, double dev_scale, void* out,
                          double* grad_out);

/* ---- S hyper-parameter samples of ONE model family as one batch: what acquisition functions do on an HGP
 *      (hyperbo/bo_utils/acfun.py:72-82 loops model.predict over model.params.samples, gp.py:666-682; the jax counterpart is a
 *      vmap over the draws).  models[s]: sample s (same dtype, covariance, mean and MLP architecture for all); x [n,D], y [n,m]
 *      the observations every sample conditions on; the S Gram matrices are built, factorised and inverted as ONE batch, the S
 *      posteriors + acquisition epilogues queue up on the device; out [S,M] (model dtype), row s = hbo_acq of sample s with
 *      params[s] / add_noise[s] (the caller averages: acfun.py:82).  Rows of samples whose Gram matrix is not PD are NaN
 *      (HBO_NOT_PD). */
int hbo_acq_samples(hbo_ctx* ctx, const hbo_model* models, int32_t S, const void* x, int64_t n, const void* y, int32_t m,
                    const void* xq, int64_t M, int acq_id, const double* params, const double* add_noise, double scale, void* out);

/* ---- the value-only NLL of S hyper-parameter samples of one model family over every task of a resident dataset: the log
 *      density of the slice sampler config['method'] = 'slice_sample' asks for (hyperbo/bo_utils/bayesopt.py:247-255 -- HBO_SS:
 *      burnin 50, nsamples 50, NLL objective, DEFAULT_PRIORS; hyperbo/gp_utils/slice_sampling_test.py:56-153), which calls it for the
 *      pending points of all its chains at once.  nll_sum[s] = what hbo_nll(ctx, &models[s], ds, ...) returns (a sum over the tasks;
 *      the caller divides by the task count), nll_per_task (nullable): [S][n_tasks] in the dataset's order.  The samples share dtype,
 *      covariance, mean, input_dim and MLP architecture (HBO_ERR_ARG otherwise, the rule of hbo_acq_samples); an input-warped
 *      (Kumaraswamy) sample gives HBO_ERR_UNSUPPORTED before any device work.  A task whose Gram matrix is not PD is NaN, and so is its
 *      sample's sum; the call returns HBO_NOT_PD and the other samples are unaffected.  Every task of n <= 128: one launch of the
 *      single-workgroup evaluation over the S x T pairs, each pair's value independent of the other samples in the call (bit for
 *      bit); otherwise Gram -> factorisation -> reduction as one batch per chunk of samples that fits half the free device memory.
 *      No float atomics: identical calls are bit-identical. */
int hbo_nll_samples(hbo_ctx* ctx, const hbo_model* models, int32_t S, hbo_dataset* ds, double* nll_sum, double* nll_per_task);

/* ---- d acquisition / d x_query: the gradient jaxopt.ScipyBoundedMinimize(L-BFGS-B) takes of
 *      f(x) = -ac_func(model, key, x[None]) in bayesopt() (hyperbo/bo_utils/bayesopt.py:116-125).
 *      Queries are independent rows: out [M,1] (model dtype) as hbo_acq, grad_out [M, input_dim] doubles.
 *      Matern kernels: a query at zero distance from a training point contributes 0 (linalg.py:183-188). */
int hbo_acq_grad(hbo_ctx* ctx, const hbo_model* model, hbo_cache* cache, const void* xq, int64_t M,
                 int acq_id, double param, double add_noise, double scale, void* out, double* grad_out);

/* ---- the same for S hyper-parameter samples of ONE model family over their finished caches, in one launch: what bayesopt()'s inner
 *      L-BFGS-B asks of an HGP at every evaluation (acfun.py:72-82 under bayesopt.py:116-125; the caller averages over s).
 *      models[s] / caches[s]: sample s and the cache hbo_factor built for it (same observations or not: each pair is on its own);
 *      acq_out [S,M] (model dtype) and grad_out [S,M,input_dim] doubles: row s is what
 *      hbo_acq_grad(ctx, &models[s], caches[s], xq, M, acq_id, params[s], add_noise[s], scale, ...) returns, up to the order of
 *      summation.  One upload, one launch (one workgroup per (sample, query) pair, csrc/acq_small.hip), one copy back and one
 *      synchronisation whatever S is.  Every sum is fp64 in a fixed order and there are no atomics: a row does not depend on which
 *      other samples or queries share the call (bit for bit), and identical calls are bit-identical.
 *      HBO_ERR_ARG (before any device call): null arguments, S outside 1..4096, a bad acq_id, samples that do not share dtype /
 *      covariance / mean / input_dim, a cache whose dtype / input_dim / input warp does not match its model.
 *      HBO_ERR_UNSUPPORTED (before any device work; these stay with hbo_acq_grad): a cache with n > 128, a null or empty cache (the
 *      prior branch), kernel_uses_mlp, a linear_mlp mean, an input-warped (Kumaraswamy) model (a packed array element has no
 *      hbo_model_kumar tail, as in hbo_acq_samples).
 *      A sample whose cache is not positive definite gets NaN rows and the call returns HBO_NOT_PD; the other samples are unaffected.
 *      M == 0 returns HBO_OK. */
int hbo_acq_grad_samples(hbo_ctx* ctx, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq, int64_t M,
                         int acq_id, const double* params, const double* add_noise, double scale, void* acq_out, double* grad_out);

/* ---- hbo_acq_grad_samples for caches of ANY n >= 1: same arguments, same checks (before any device work), same return codes and the
 *      same NaN rows / HBO_NOT_PD for a sample that is not positive definite -- minus the refusal of n > 128; the prior branch, MLP
 *      bases, a linear_mlp mean and input-warped models stay refused.  When every cache of the call has n <= 128 this IS
 *      hbo_acq_grad_samples: the same launch, the same bits.  Otherwise every sample of the call, those of n <= 128 included, takes
 *      four stream-ordered launches per chunk of queries (csrc/acq_blocked.hip: k = k(x, X); l = W k; beta = W^T l; one workgroup
 *      per (sample, query) pair for the sums, the scalars and the gradient) over an fp64 workspace of three [S, chunk, npad] arrays,
 *      the chunk chosen so that they stay under 256 MiB; one upload, one copy back and one synchronisation whatever S and M are.  A
 *      phase boundary is a launch boundary: no grid-wide barrier, no wait between workgroups, no atomics.  Every sum is fp64 in an
 *      order fixed by the cache's n and input_dim alone: a row does not depend on which samples or queries share the call, on its
 *      place among them, on the other caches' sizes or on the chunking (bit for bit), and identical calls are bit-identical. */
int hbo_acq_grad_samples_blocked(hbo_ctx* ctx, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq, int64_t M,
                                 int acq_id, const double* params, const double* add_noise, double scale, void* acq_out,
                                 double* grad_out);

/* ---- bayesopt()'s inner maximisation of the acquisition function on the device (hyperbo/bo_utils/bayesopt.py:116-125), R starts
 *      in ONE call: a box-constrained projected L-BFGS that minimises f(x) = -(mean over the S samples of the acquisition) over
 *      lo <= x <= hi (csrc/acq_opt_ctl.h; the algorithm: DESIGN.md section 6).  One upload, then `evals` rounds of two stream-ordered
 *      launches -- hbo_acq_grad_samples' kernel on grid (R, S) over the starts' pending points, then one control workgroup per start,
 *      which sums the S per-sample results in sample order (fp64), runs one step of the state machine and writes the next pending
 *      point -- and one synchronisation and one copy back.  No atomics, every sum in a fixed order, no fused multiply-adds in the
 *      control code: identical calls are bit-identical, a start does not depend on what shares the call, and a run gives the same
 *      bits however it is cut into calls.
 *      models, S, caches, acq_id, params, add_noise, scale: as hbo_acq_grad_samples (same checks, same refusals, same return codes).
 *      x0 [R, input_dim] (model dtype): the starts.  lo, hi [input_dim] doubles (both null: 0 and 1); for an fp32 model they must be
 *        fp32 numbers.  Every probe is clipped to the box component by component and rounded to the model dtype, so bounds are hit
 *        exactly and x_out is representable in the model dtype.
 *      opts: memory (10; at most 64), ls_steps (20), max_iters (200), c1 (1e-4), tau (0.5), pgtol (1e-5), ftol (2.2e-9) -- the defaults are
 *        the caller's to fill in.  memory 1..64, ls_steps and max_iters >= 1, 0 < c1 < 1, 0 < tau < 1, pgtol and ftol >= 0.
 *      state [R, hbo_acq_opt_state_doubles(input_dim, memory)], in / out: all zero = a fresh run from x0; otherwise the run goes on
 *        where the call that left the state stopped (x0 is then not read).  A call that returns an error has not written it.
 *      x_out [R, input_dim]: the iterate (the last accepted point).  val_out [R]: the acquisition value there (+mean, not f; NaN
 *        before the first evaluation and after NONFINITE_AT_START).  status [R]: hbo_acq_opt_status.
 *      log (nullable) [evals, R]: one record per round and start.  kind START (the first evaluation), LINE_SEARCH (a rejected probe),
 *        MAIN (an accepted probe: main step `iter` is taken) or IDLE (the start had stopped: its evaluation ran on the old pending
 *        point and was ignored; value 0); alpha: the probe's step; value: f at the point evaluated.
 *      HBO_ERR_ARG (before any device work): those of hbo_acq_grad_samples, R outside 1..4096, evals outside 1..4096, bad opts,
 *      lo > hi or not finite, an x0 outside the box or not finite, a state that is neither all zero nor one an earlier call left.
 *      HBO_ERR_UNSUPPORTED (before any device work): those of hbo_acq_grad_samples, and a state (input_dim, opts.memory) beyond the
 *      64 KB of LDS the control kernel stages it in (memory 10 fits every input_dim up to 256).
 *      HBO_NOT_PD: a cache is not positive definite (every start then stops with NONFINITE_AT_START). */
enum hbo_acq_opt_kind { HBO_ACQ_OPT_START = 0, HBO_ACQ_OPT_MAIN = 1, HBO_ACQ_OPT_LINE_SEARCH = 2, HBO_ACQ_OPT_IDLE = 3 };
enum hbo_acq_opt_status {
  HBO_ACQ_OPT_RUNNING = 0, HBO_ACQ_OPT_CONVERGED = 1, HBO_ACQ_OPT_FTOL = 2, HBO_ACQ_OPT_NO_PROGRESS = 3, HBO_ACQ_OPT_NONFINITE_AT_START = 4,
  HBO_ACQ_OPT_STEPS_DONE = 5
};
typedef struct hbo_acq_opt_opts {
  int32_t memory, ls_steps, max_iters;
  double c1, tau, pgtol, ftol;
} hbo_acq_opt_opts;
typedef struct hbo_acq_opt_eval {
  int32_t kind, iter;
  double alpha, value;
} hbo_acq_opt_eval;
int64_t hbo_acq_opt_state_doubles(int32_t input_dim, int32_t memory);
int hbo_acq_maximize(hbo_ctx* ctx, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* x0, int32_t R,
                     const double* lo, const double* hi, int acq_id, const double* params, const double* add_noise, double scale,
                     const hbo_acq_opt_opts* opts, double* state, int32_t evals, double* x_out, double* val_out, int32_t* status,
                     hbo_acq_opt_eval* log);

/* ---- hbo_acq_maximize for caches of ANY n >= 1: same arguments, checks, state and log format, return codes and determinism (a run
 *      gives the same bits however it is cut into calls), minus the refusal of n > 128.  The evaluation of a round is that of
 *      hbo_acq_grad_samples_blocked over the R pending points: hbo_acq_maximize's one launch when every cache has n <= 128 (then the
 *      two entry points agree to the bit: state, log, x_out, val_out, status), four launches otherwise, so five stream-ordered
 *      launches per round, still without a host wait.  HBO_ERR_UNSUPPORTED (before any device work) also when the evaluation
 *      workspace, 3 * S * R * npad doubles, exceeds half of the device memory: use fewer starts per call. */
int hbo_acq_maximize_blocked(hbo_ctx* ctx, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* x0, int32_t R,
                             const double* lo, const double* hi, int acq_id, const double* params, const double* add_noise, double scale,
                             const hbo_acq_opt_opts* opts, double* state, int32_t evals, double* x_out, double* val_out, int32_t* status,
                             hbo_acq_opt_eval* log);

/* ---- hbo_acq_grad_samples_blocked with MLP-basis kernels (kernel_uses_mlp) and the linear_mlp mean served: same arguments, same
 *      checks (before any device work), same return codes and the same NaN rows / HBO_NOT_PD -- minus the refusals of kernel_uses_mlp
 *      and of a linear_mlp mean.  All pairings are taken: MLP kernel + linear_mlp, MLP kernel + linear (raw) / constant / zero mean, raw
 *      kernel + linear_mlp mean.  xq [M, input_dim] is the RAW input and grad_out [S, M, input_dim] is d value / d raw x (fp64): the
 *      workgroup that owns a (sample, query) pair runs the query's forward pass through sample s's own weights (all layers in fp64
 *      LDS), works in the kernel's own space, takes the mean in the mean's own space and ends with the backward pass
 *      (csrc/acq_mlp.h).  Weights and biases are read in the model dtype; every product and sum is fp64.  The S weight sets ride up
 *      in the call's one staged upload: still one upload, one copy back, one synchronisation.
 *      Launches: ONE when every cache has n <= 128; otherwise FIVE per chunk of queries -- a forward launch, grid (chunk, S), writes
 *      every layer's activations into a further fp64 plane [S, chunk, sum of the layer widths] of the blocked workspace, then the four
 *      of hbo_acq_grad_samples_blocked, whose first reads the query in the kernel's space from that plane and whose last reads the
 *      activations back; the chunk keeps the whole workspace under 256 MiB.
 *      Determinism, as the siblings promise it: no atomics, every sum in an order fixed by the cache's n, the layers' shapes and
 *      input_dim alone; identical calls are bit-identical and a row does not depend on which samples or queries share the call, its
 *      place among them, the other caches' sizes or the chunking.
 *      For a model family WITHOUT any MLP the call IS hbo_acq_grad_samples_blocked: same launches, same bytes of every output.
 *      HBO_ERR_UNSUPPORTED (before any device work, with the advice to evaluate the samples with hbo_acq_grad): a null or empty cache
 *      (the prior branch) and input-warped (Kumaraswamy) models.  HBO_ERR_ARG also: samples whose MLP architectures differ. */
int hbo_acq_grad_samples_mlp(hbo_ctx* ctx, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq, int64_t M,
                             int acq_id, const double* params, const double* add_noise, double scale, void* acq_out, double* grad_out);

/* ---- hbo_acq_maximize_blocked with those models served: same arguments, checks, state and log format (hbo_acq_opt_state_doubles
 *      is unchanged), return codes and determinism (identical calls, a start alone or among others, a run cut into calls: the same
 *      bits).  The evaluation of a round is that of hbo_acq_grad_samples_mlp over the R pending points; the control kernel is the same
 *      and sees raw points and raw gradients.  Launches per round: two for n <= 128 (evaluation, control), six otherwise (forward,
 *      the four, control), without a host wait.  The evaluation workspace of the blocked route is S * R * (3 npad + sum of the layer
 *      widths) doubles (HBO_ERR_UNSUPPORTED beyond half of the device memory).  Refusals: those of hbo_acq_grad_samples_mlp.  For a
 *      family without any MLP the call IS hbo_acq_maximize_blocked: state, log, x_out, val_out and status to the bit. */
int hbo_acq_maximize_mlp(hbo_ctx* ctx, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* x0, int32_t R,
                         const double* lo, const double* hi, int acq_id, const double* params, const double* add_noise, double scale,
                         const hbo_acq_opt_opts* opts, double* state, int32_t evals, double* x_out, double* val_out, int32_t* status,
                         hbo_acq_opt_eval* log);

/* ---- max-value entropy search (MES, Wang & Jegelka 2017; no counterpart in the reference): the information a query carries about the
 *      maximum of the objective, from K sampled maxima y*_1..y*_K (hbo_sample_paths / hbo_paths_maximize draw them).  For posterior mean
 *      mu and variance var at a query, with pdf and cdf of the standard normal:
 *        v2 = (var + add_noise) * scale,  sd = sqrt(v2),  gamma_k = (y*_k - mu) / sd,  r = pdf(gamma) / cdf(gamma)
 *        h(gamma)  = gamma r / 2 - log cdf(gamma)                    (>= 0, decreasing, h(+inf) = 0)
 *        h'(gamma) = -(r / 2) (1 + gamma^2 + gamma r)
 *        value = (1 / K) sum_k h(gamma_k)                            fp64, summed in index order
 *        a_mu  = -(1 / K) sum_k h'(gamma_k) / sd,   a_sd = -(1 / K) sum_k h'(gamma_k) gamma_k / sd,   a_var = a_sd / (2 sd) * scale
 *      v2 <= 0: the value, a_mu and a_var are 0 (no posterior uncertainty, no information; a NaN there would win an argmax); a NaN v2
 *      stays NaN.  For every finite gamma the value is finite and >= 0: it reaches 0 by underflow for large gamma and is never
 *      negative.  Neither tail is evaluated literally (csrc/kernfun.h: mes_terms): log cdf is log1p(-cdf(-gamma)) from erfc for
 *      gamma >= 0, and r and log cdf come from the scaled complementary error function erfcx for gamma < 0; what is left of the
 *      cancellation in h' for gamma << 0 is about 10 digits at gamma = -30 and 14 at -8, relative to the un-cancelled terms.
 *      MES is not a fourth acq_id: hbo_acq, hbo_acq_grad_samples[_blocked] and hbo_acq_maximize[_blocked] keep refusing acq_id = 3.
 *      K is 1..HBO_MES_MAX_K.  HBO_ERR_ARG (before any device work, outputs untouched) for every entry point below: K outside that
 *      range, a null ystar or one that holds a value that is not finite, plus what the sibling entry point checks. */
#define HBO_MES_MAX_K 256
/* ---- the values over a pool: hbo_acq's posterior pipeline (any n, every model family hbo_acq serves, cache == NULL -> the prior
 *      branch, queries in chunks of post_chunk) under an epilogue of its own: a thread per query, mu, var and sd in the model dtype as
 *      hbo_acq forms them, the K terms in fp64 in index order, rounded once to the model dtype.  ystar [K] doubles; out [M,1] model
 *      dtype.  A row does not depend on post_chunk nor on what the other rows of the call hold (bit for bit); as in hbo_acq, the form
 *      of the posterior product follows from the TOTAL number of queries M, so calls of different M may differ in the order of the
 *      sums behind mu and var.  Not positive definite: NaN and HBO_NOT_PD, as hbo_acq. */
int hbo_acq_mes(hbo_ctx* ctx, const hbo_model* model, hbo_cache* cache /* nullable */, const void* xq, int64_t M, const double* ystar,
                int32_t K, double add_noise, double scale, void* out);
/* ---- value and d value / d x_query for S samples over their finished caches: hbo_acq_grad_samples_blocked with ystar [S,K] (row s:
 *      the maxima of sample s) in the place of acq_id and params -- its semantics, checks, refusals and return codes, for any n >= 1:
 *      one launch when every cache has n <= 128 (csrc/acq_small.hip), four per chunk of queries otherwise (csrc/acq_blocked.hip).  Only
 *      the scalar step differs: the K terms are taken by K threads of the workgroup that owns the (sample, query) pair and the three
 *      sums then run in index order out of LDS, whatever K is; a_mu and a_var feed the unchanged gradient code.  No atomics, every sum
 *      in a fixed order: a row does not depend on which samples or queries share the call nor on the chunking (bit for bit), and
 *      identical calls are bit-identical.  acq_out [S,M] model dtype, grad_out [S,M,input_dim] doubles. */
int hbo_mes_grad_samples(hbo_ctx* ctx, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq, int64_t M,
                         const double* ystar, int32_t K, const double* add_noise, double scale, void* acq_out, double* grad_out);
/* ---- the maximisation of the MES value (mean over the S samples) over a box, R starts in one call: hbo_acq_maximize_blocked with
 *      ystar [S,K], K in the place of acq_id, params -- the same control kernel, state format, log, checks, return codes and
 *      determinism (no atomics, sums in a fixed order; a run gives the same bits however it is cut into calls); the evaluation of a
 *      round is hbo_mes_grad_samples' over the R pending points, and val_out the mean over s of its fp64 values at x_out. */
int hbo_mes_maximize(hbo_ctx* ctx, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* x0, int32_t R,
                     const double* lo, const double* hi, const double* ystar, int32_t K, const double* add_noise, double scale,
                     const hbo_acq_opt_opts* opts, double* state, int32_t evals, double* x_out, double* val_out, int32_t* status,
                     hbo_acq_opt_eval* log);

/* ---- log expected improvement (LogEI, Ament et al. 2023, "Unexpected improvements to expected improvement"; no counterpart in the
 *      reference): the logarithm of EI, with EI's maximiser, in a form that stays representable where EI and its gradient underflow
 *      (u < -8 in fp32 pools, -38 in fp64).  For posterior mean mu and variance var at a query and the target t (EI's param):
 *        v2 = (var + add_noise) * scale,  sd = sqrt(v2),  u = (mu - t) / sd
 *        h(u)  = pdf(u) + u cdf(u)                                   EI = sd h(u)
 *        value = log sd + log h(u)
 *        a_mu  = cdf(u) / (sd h(u)),   a_sd = pdf(u) / (sd h(u)),   a_var = a_sd / (2 sd) * scale
 *      log h, cdf / h and pdf / h come from one function (csrc/kernfun.h: logei_terms): literally for u > -1; from the scaled
 *      complementary error function for -256 <= u <= -1 (Mills ratio m = sqrt(pi / 2) erfcx(-u / sqrt 2), w = h / pdf = 1 + u m,
 *      log h = -u^2 / 2 - log sqrt(2 pi) + log w, cdf / h = m / w, pdf / h = 1 / w; the cancellation in w costs a relative error of
 *      about eps u^2); from the asymptotic series w u^2 = 1 - 3 / u^2 + 15 / u^4 - 105 / u^6 (and its counterpart for m) beyond,
 *      exact to eps.  The value is finite for every finite u whose square does not overflow, and its gradient grows like |u| in the
 *      tail instead of vanishing.  u = +inf and u = -inf give the limits, never NaN.
 *      v2 <= 0 (no posterior uncertainty): value = log(mu - t), a_mu = 1 / (mu - t), a_var = 0 if mu > t; otherwise value = -inf and
 *      both slopes are 0.  -inf loses every argmax, is a probe the maximiser's line search rejects, and at a start gives
 *      HBO_ACQ_OPT_NONFINITE_AT_START.  Wherever the value is -inf both slopes are 0.  A NaN v2 stays NaN.
 *      Several samples (HGP): the acquisition is the log of the MEAN of the samples' EI, not the mean of their logs.  From per-sample
 *      values v_s and gradients g_s, with m = max_s v_s and w_s = exp(v_s - m):  value = m + log(sum_s w_s / S),
 *      grad = sum_s w_s g_s / sum_s w_s, fp64 sums in sample order; m = -inf: value -inf, gradient 0; any NaN row: NaN; S = 1: v_0 and
 *      g_0 to the bit.  hbo_logei_maximize combines so on the device; the other two entry points return per-sample rows.
 *      LogEI is not a fourth acq_id: hbo_acq, hbo_acq_samples, hbo_acq_grad*, hbo_acq_maximize* and hbo_bo_simulated keep refusing
 *      acq_id = 3.  HBO_ERR_ARG (before any device work, outputs untouched) for every entry point below: a target that is not
 *      finite, null targets, plus what the sibling entry point checks. */
/* ---- the values over a pool: hbo_acq's posterior pipeline (any n, every model family hbo_acq serves, cache == NULL -> the prior
 *      branch, queries in chunks of post_chunk) under an epilogue of its own: a thread per query, mu, var, v2 and sd in the model dtype
 *      as hbo_acq forms them, u and the terms in fp64, rounded once to the model dtype.  out [M,1] model dtype.  A row does not depend
 *      on post_chunk nor on what the other rows of the call hold (bit for bit); as in hbo_acq, the form of the posterior product
 *      follows from the TOTAL number of queries M.  Not positive definite: NaN and HBO_NOT_PD, as hbo_acq. */
int hbo_acq_logei(hbo_ctx* ctx, const hbo_model* model, hbo_cache* cache /* nullable */, const void* xq, int64_t M, double target,
                  double add_noise, double scale, void* out);
/* ---- value and d value / d x_query for S samples over their finished caches, PER SAMPLE: hbo_acq_grad_samples_mlp with targets [S] in
 *      the place of acq_id and params -- its semantics, checks, refusals (the prior branch, Kumaraswamy-warped models) and return
 *      codes, for any n >= 1, MLP-basis kernels and the linear_mlp mean included: one launch when every cache has n <= 128, four or
 *      five per chunk of queries otherwise.  Only the scalar step differs, a per-thread function like EI's; a_mu and a_var feed the
 *      unchanged gradient code, the MLP backward pass included.  No atomics, every sum in a fixed order: a row does not depend on which
 *      samples or queries share the call nor on the chunking (bit for bit), and identical calls are bit-identical.
 *      acq_out [S,M] model dtype, grad_out [S,M,input_dim] doubles. */
int hbo_logei_grad_samples(hbo_ctx* ctx, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq, int64_t M,
                           const double* targets, const double* add_noise, double scale, void* acq_out, double* grad_out);
/* ---- the maximisation of LogEI (combined over the S samples by the rule above) over a box, R starts in one call:
 *      hbo_acq_maximize_mlp with targets [S] in the place of acq_id, params -- the same control kernel, state format, log, checks,
 *      return codes and determinism (a run gives the same bits however it is cut into calls); the control kernel's reduction over the
 *      samples is the log-mean-exp rule in the place of the mean (csrc/acq_opt_ctl.h), and val_out the combined value at x_out. */
int hbo_logei_maximize(hbo_ctx* ctx, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* x0, int32_t R,
                       const double* lo, const double* hi, const double* targets, const double* add_noise, double scale,
                       const hbo_acq_opt_opts* opts, double* state, int32_t evals, double* x_out, double* val_out, int32_t* status,
                       hbo_acq_opt_eval* log);

/* ---- batch (q-point) expected improvement (qEI, Ginsbourger et al. 2010, in the reparameterised Monte-Carlo form of Wilson et al.
 *      2018; no counterpart in the reference): the expected improvement of the BEST of q points evaluated together, under their JOINT
 *      posterior.  For a batch x_1..x_q over a finished cache (X, W = L^-1 lower, alpha), a target t and B base samples z [B, q]
 *      (standard normals the caller draws once; every sample, batch and start reads the same z):
 *        k_j = k(x_j, X),  l_j = W k_j,  beta_j = W^T l_j,  mu_j = k_j . alpha + m(x_j)
 *        Sigma_jl = k(x_j, x_l) - l_j . l_l,  Sigma' = (Sigma + add_noise I) scale,  C = chol(Sigma') lower    (noise first, then the
 *                                                                                     scale: GP.predict(full_cov, with_noise, unbiased))
 *        f_bj = mu_j + sum_{l<=j} C_jl z_bl,  j*_b = the LOWEST index of the largest f_bj,  imp_b = f_{b j*_b} - t
 *        value = (1 / B) sum_b max(0, imp_b)                       (imp_b == 0 contributes nothing)
 *      grad_out is the exact gradient of that sample average (z is fixed: the function is deterministic and piecewise smooth):
 *        w_bj = [j == j*_b and imp_b > 0] / B,  mubar_j = sum_b w_bj,  Cbar_jl = sum_b w_bj z_bl (l <= j)
 *        P = tril(C^T Cbar) with its diagonal halved,  Sbar = C^-T P C^-1,  G = scale (Sbar + Sbar^T) / 2       (= d value / d Sigma)
 *        coef_j = mubar_j alpha - 2 sum_l G_jl beta_l
 *        d value / d x_j = sum_i coef_ji dk(x_j, X_i)/dx_j + 2 sum_{l != j} G_jl dk(x_j, x_l)/dx_j + G_jj dk(x_j, x_j)/dx_j + mubar_j dm/dx_j
 *      (the G_jj term is 0 for SE and Matern and 2 x_j / sigma^2 G_jj for the dot product; a Matern pair at zero distance -- a query on
 *      an observation, two equal batch points -- contributes 0, as in hbo_acq_grad).  With q = 1 this is hbo_acq_grad's formula with
 *      a_mu = mubar and a_var = G_11.
 *      One 256-thread workgroup owns one (batch, sample) pair and reads the sample's W once for all q points (csrc/qei.hip).  Every
 *      product and sum is fp64 whatever the model dtype (X, W, alpha and the points are read in the model dtype), in an order fixed by
 *      (n, input_dim, q, B) alone; no atomics: a pair does not depend on what shares the call (bit for bit) and identical calls are
 *      bit-identical.
 *      A pivot of the q x q factorisation that is not > 0 (duplicate points with add_noise == 0, a non-finite input): the value and
 *      every gradient component of that (sample, batch) pair are NaN, the other pairs are unaffected and the call still returns
 *      HBO_OK.  A cache that is not positive definite: NaN rows for that sample and HBO_NOT_PD, as the siblings.
 *      HBO_ERR_ARG (before any device work, outputs and state untouched): null arguments, S outside 1..4096, q outside
 *      1..HBO_QEI_MAX_Q, B outside 1..HBO_QEI_MAX_BASE, a z, target, add_noise or scale that is not finite, add_noise < 0,
 *      scale <= 0, samples that do not share dtype, covariance, mean or input_dim, a cache that does not match its model.
 *      HBO_ERR_UNSUPPORTED (before any device work, the message names the reason): a cache of n > 128, a null or empty cache (the
 *      prior branch), kernel_uses_mlp or a linear_mlp mean, a Kumaraswamy-warped model.  These three are OUT OF SCOPE of this entry
 *      point: caches beyond 128 observations (a blocked route in the manner of csrc/acq_blocked.hip), MLP bases, Kumaraswamy warps. */
#define HBO_QEI_MAX_Q 16
#define HBO_QEI_MAX_BASE 1024
/* ---- value and gradient, PER SAMPLE: xq [M, q, input_dim] model dtype, z [B, q], targets [S], add_noise [S];
 *      val_out [S, M] fp64 (not rounded to the model dtype), grad_out [S, M, q, input_dim].  The acquisition of an HGP is the mean
 *      over s of the rows.  M == 0 returns HBO_OK. */
int hbo_qei_grad_samples(hbo_ctx* ctx, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq, int64_t M, int32_t q,
                         const double* z, int32_t B, const double* targets, const double* add_noise, double scale, double* val_out,
                         double* grad_out);
/* ---- the maximisation of qEI (mean over the S samples) over the box, R starting batches in one call: hbo_acq_maximize over a
 *      variable of dimension q * input_dim -- the same control kernel, state format (hbo_acq_opt_state_doubles(q * input_dim,
 *      memory)), log, status codes and opts, the box lo, hi [input_dim] tiled q times.  One upload, then `evals` rounds of two
 *      stream-ordered launches (the qEI kernel on grid (R, S) over the pending batches, then the control kernel), one synchronisation
 *      and one copy back.  A run gives the same bits however it is cut into calls, a start does not depend on what shares the call,
 *      bounds are hit exactly and points are rounded to the model dtype.  x0, x_out [R, q, input_dim]; val_out [R]: the mean over s of
 *      hbo_qei_grad_samples' values at x_out.  The line search rejects a non-finite probe; a non-finite start ends with
 *      HBO_ACQ_OPT_NONFINITE_AT_START.  Checks: those above and the R, evals, opts, box, start and state checks of hbo_acq_maximize;
 *      HBO_ERR_UNSUPPORTED also for a state (q * input_dim, opts.memory) beyond the control kernel's 64 KB of LDS (memory 10 fits
 *      q * input_dim <= 256). */
int hbo_qei_maximize(hbo_ctx* ctx, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* x0, int32_t R, int32_t q,
                     const double* lo, const double* hi, const double* z, int32_t B, const double* targets, const double* add_noise,
                     double scale, const hbo_acq_opt_opts* opts, double* state, int32_t evals, double* x_out, double* val_out,
                     int32_t* status, hbo_acq_opt_eval* log);

/* ---- the maximisation of S posterior sample paths over a box, R starts each, in ONE call: continuous Thompson sampling -- q
 *      suggestions from q paths (no counterpart in the reference).  The optimiser is that of hbo_acq_maximize, run on
 *      f(x) = -f_s(x) for each of the S * R (path, start) pairs: one upload and one solve for u (hbo_sample_paths_grad), then `evals`
 *      rounds of two stream-ordered launches -- the kernel of hbo_sample_paths_grad over the S * R pending points, each under its own
 *      path, then hbo_acq_maximize's control kernel with one workgroup per pair -- and one synchronisation and one copy back.
 *      model, cache, S, F, omega, phase, w, eps, dev_scale: as hbo_sample_paths_grad.  x0 [S, R, input_dim] (model dtype): the
 *      starts of path s.  lo, hi, opts, evals, log: as hbo_acq_maximize, with S * R in the place of its R everywhere: state
 *      [S * R, hbo_acq_opt_state_doubles(input_dim, memory)], x_out [S, R, input_dim], val_out [S, R] (the path's value at x_out),
 *      status [S, R], log [evals, S * R].  All zero = a fresh run, otherwise the run goes on; a run gives the same bits however it is
 *      cut into calls; a pair does not depend on what shares the call; bounds are hit exactly; an fp32 model takes fp32 numbers for
 *      the box; the evaluation of a pending point is, to the bit, hbo_sample_paths_grad's at that point
 *      (the optimiser sees the value as that call returns it: a number of the model dtype).
 *      HBO_ERR_ARG (before any device work, nothing written): those of hbo_sample_paths_grad, R < 1, S * R > 4096, evals outside
 *      1..4096, bad opts, lo > hi or not finite, an x0 outside the box or not finite, a state that is neither all zero nor one an
 *      earlier call left.  HBO_ERR_UNSUPPORTED (before any device work): those of hbo_sample_paths_grad, and a state beyond the 64 KB
 *      of LDS of the control kernel.  HBO_NOT_PD: the cache is not positive definite (val_out is NaN and every pair stops with
 *      NONFINITE_AT_START). */
int hbo_paths_maximize(hbo_ctx* ctx, const hbo_model* model, hbo_cache* cache /* nullable */, int32_t S, int32_t F, const void* omega,
                       const void* phase, const void* w, const void* eps, double dev_scale, const void* x0, int32_t R, const double* lo,
                       const double* hi, const hbo_acq_opt_opts* opts, double* state, int32_t evals, double* x_out, double* val_out,
                       int32_t* status, hbo_acq_opt_eval* log);

/* ---- the simulated BO loop over a pool of pre-evaluated candidates (hyperbo/bo_utils/bayesopt.py:136-190), every iteration of R
 *      independent runs in ONE call: all launches are queued up front and the results come back behind them: one synchronisation, at the end.
 *      Per iteration the host loop evaluates the acquisition function at the pool, takes np.argmax and appends the chosen (x, y); here
 *      the posterior at the pool is carried along as one more row of forward substitution per appended observation
 *      (csrc/bo_loop.hip; O(n M) per iteration, no factor, no limit on the number of observations).
 *      models[r] may differ in values; they share dtype, covariance, mean, input_dim and MLP architecture (the rule of hbo_acq_samples).
 *      Run r: pool xc [M, input_dim] with values yc [M], initial observations x0 [n0, input_dim] / y0 [n0] (n0 may be 0: the prior
 *      branch; x0 / y0 may then be null), all in the model dtype.  add_noise, scale0, scale: GP.predict's post-processing
 *      (gp.py:607-619), scale0 for iteration 0 and scale for the rest -- they differ when the first append creates the sub-dataset.
 *      The acquisition parameter of an iteration comes from the observed y (initial and appended) on the device, as acfun.py's default
 *      callbacks: CONST: param (ucb*: beta);  MAX_PLUS: max y + param (EI: 0, pi / pi3: zeta);  MAX_PLUS_STD: max y + param * np.std(y)
 *      (pi2);  over an empty y the two MAX modes give 0.0.
 *      Selection = np.argmax on the values rounded to the model dtype: the first index among equal values, the first NaN if there is
 *      one; a selected candidate stays in the pool.
 *      sel_out / acq_out [R][iters]: selected index and its acquisition value (NaN where np.argmax ran over NaN).  mu_out / var_out
 *      (nullable): the runs' posteriors at their pools after the last append, before noise and scale, back to back ([sum of M], model
 *      dtype).  status [R]: HBO_OK, or HBO_NOT_PD for a run one of whose pivots l_pp^2 was <= 0 or NaN -- from that row on its
 *      values are NaN and its selections index 0, what the host loop gets from a cache that fails to factorise; the call then returns
 *      HBO_NOT_PD and the other runs are unaffected.
 *      No atomics; every sum is fp64 in a fixed order: identical calls are bit-identical, and a run does not depend on what shares
 *      the call.
 *      HBO_ERR_ARG (before any device work): null arguments, R outside 1..4096, iters outside 1..65536, a run with M <= 0, n0 < 0,
 *      M + n0 >= 2^31, null pool or (n0 > 0) null observations, a bad acq_id / param_mode, models of different families.
 *      HBO_ERR_UNSUPPORTED (before any device work): an input-warped (Kumaraswamy) model; a workspace ((n0 + iters) x (M + n0) doubles
 *      per run) above half of the device memory. */
enum hbo_bo_param_mode { HBO_BO_PARAM_CONST = 0, HBO_BO_PARAM_MAX_PLUS = 1, HBO_BO_PARAM_MAX_PLUS_STD = 2 };
typedef struct hbo_bo_run {
  const void* xc; const void* yc; int64_t M;      /* candidate pool [M, D], its pre-evaluated values [M] */
  const void* x0; const void* y0; int64_t n0;     /* observations the sub-dataset starts with (n0 may be 0) */
  int32_t acq_id; int32_t param_mode; double param;
  double add_noise, scale0, scale;                /* gp.py:607-619; scale0 for iteration 0, scale for the rest */
} hbo_bo_run;
int hbo_bo_simulated(hbo_ctx* ctx, const hbo_model* models, const hbo_bo_run* runs, int32_t R, int32_t iters,
                     int32_t* sel_out, double* acq_out, void* mu_out, void* var_out, int32_t* status);

/* ---- dense building blocks (linalg.py:29-33 solve_linear_system); host in/out ----------- */
/* a: [n,n] SPD (only the lower triangle is read).  chol_out: lower factor (zeros above diag);
 * inv_out (nullable): full symmetric a^-1;  b/x_out (nullable): [n,m] solve a x = b. */
int hbo_spd_solve(hbo_ctx* ctx, int dtype, const void* a, int64_t n, const void* b, int32_t m,
                  void* chol_out, void* inv_out, void* x_out, double* logdet_half);
/* linalg.py:139-145, inverse_spdmatrix_vector_product(cached_cholesky=...): x = L^-T L^-1 b for a lower factor the caller holds
 * as an array (chol_lower: [n,n] row-major, only the lower triangle is read; b / x_out: [n,m]).  Two substitution sweeps on the
 * device; nothing is factorised. */
int hbo_chol_solve(hbo_ctx* ctx, int dtype, const void* chol_lower, int64_t n, const void* b, int32_t m, void* x_out);

/* ---- profiling: per-stage device time of the last hbo_nll / hbo_factor / hbo_acq call,
 *      measured with HIP events on the stream the kernels were launched on ---------------- */
#define HBO_MAX_PROFILE_STAGES 32
int hbo_profile_enable(hbo_ctx* ctx, int level); /* 0 off, 1 per stage, 2 per launch; -1: only the launches of the
                                                    bulk trailing update ("syrk_bulk", the roofline kernel of bench.py) */
/* names: array of HBO_MAX_PROFILE_STAGES char[32]; ms: total ms; launches: count */
int hbo_profile_get(hbo_ctx* ctx, char names[][32], double* ms, int32_t* launches, int32_t* n);

/* Options (integers by name).  Unknown names are an error.  The placement / overlap knobs of the launch schedules that the
 * measurement tools vary live behind hbo_tune (include/hbo_tune.h); they are not part of this boundary.
 *   potrf_group     0..16 128-wide panels per trailing update, K = 128*group (0 = auto: 3 up to 96 blocks, then 4, 8 from 256
 *                         blocks on and for fp32 factorisations on the bf16 matrix cores)
 *   lookahead       0..2  panel chain on its own stream one group ahead of the bulk update, inverse overlapped.  1 (default): where
 *                         it pays -- more than 4 blocks and (>= 18 blocks or tasks x blocks >= 80); below that everything runs
 *                         on one stream in order (5-13 % faster there).  0 = never, 2 = whenever there is more than one block
 *   small_nblk      int   matrices up to this many 128-blocks use 64x64 tiles in the inverse and in K^-1 = W^T W (default -1: auto --
 *                         48 blocks in fp64, 32 in fp32)
 *   pool_cap_mb     >=0   device buffers of freed datasets / caches are parked for the next one of the same shape (GP.train()
 *                         re-creates its sub-sampled batch every step); at most this many MB stay parked (default: a quarter
 *                         of the device memory, at most 49152; 0 = off)
 *   post_chunk      128..65536 posterior / acquisition: query candidates per pass (cross-Gram workspace = npad x post_chunk
 *                         elements whatever M; two workspaces alternate so that the Gram build of a chunk runs beside the
 *                         triangular product of the previous one)
 *   bf16x3          0/1   fp32 only: the GEMM-shaped work -- trailing updates of the factorisation, the products of the inverse
 *                         and K^-1 = W^T W (above small_nblk blocks), the posterior product V = L^-1 Kxq -- runs on the bf16 matrix cores
 *                         from exact three-way splits of both operands (six bf16 MFMAs per fp32 product, fp32 accumulate:
 *                         fp32-class accuracy at 1.3-1.5x the fp32-MFMA rate).  Default 1; 0 = fp32 MFMA.  The posterior product of
 *                         the stationary covariances goes one step further (hbo_tune post_f16x2, default on): two-way fp16 splits of
 *                         operands scaled by powers of two, three fp16 MFMAs per product (2^-22 per product: as close to fp64 as
 *                         the fp32-MFMA product) -- cfg 3's EI 97 -> 59 ms; and so do the factorisation's trailing updates, the inverse's
 *                         upper levels and K^-1 = W^T W of those covariances (hbo_tune chol_f16x2, default on: cfg 3's factor 21.5 -> 17.6 ms) */
int hbo_set_option(hbo_ctx* ctx, const char* name, int64_t value);
/*   spectral        0/1   (default 0) route the reference's SVD call sites -- neg_log_marginal_likelihood(use_cholesky=False),
 *                         GP / HGP.stats, svd_matrix_sqrt, sample_from_gp(method='svd' | 'eigh') -- to hbo_sym_eig / hbo_nll_spectral
 *                         instead of host LAPACK.  The library only stores it: the Python layer reads it back and routes its calls.
 *   acq_fused       0/1   (default 0) route acquisition value_and_grad calls (bo_utils/acfun.py: an HGP's mean over its parameter samples,
 *                         and a plain GP as S = 1) over caches of at most 128 observations to hbo_acq_grad_samples -- one launch per
 *                         call instead of about eight launches and a host round trip per sample.  Models it does not cover (no
 *                         observations, n > 128, an MLP basis, a linear_mlp mean, a Kumaraswamy kernel) keep the per-sample path.
 *                         The library only stores it: the Python layer reads it back and routes its calls.
 * hbo_get_option reads an option back (the same names; unknown names are an error), and the read-only eig_sweeps: the outer Jacobi
 * sweeps of the last hbo_sym_eig / hbo_nll_spectral call (largest over its batches); and the read-only post_resident: 1 when the
 * product V = L^-1 Kxq of the context's last hbo_predict / hbo_acq call (of its last chunk) ran as a resident grid drawing its tiles
 * from a counter, 0 when it ran as a plain grid, was split along K, or the call had no cache or was refused.  The results do not
 * depend on it; it is there for the tests to know which launch they checked (chol_form / inv_forms: hbo_tune.h). */
int hbo_get_option(hbo_ctx* ctx, const char* name, int64_t* out);

/* ---- symmetric eigensolver: the device form of the reference's SVD routines (objectives.py:157-176, linalg.py:113-126,
 *      gp.py:198-240 multivariate_normal 'svd' / 'eigh').  fp64 two-sided Jacobi (csrc/eig.hip): the matrix is padded to a multiple
 *      of 64 and cut into blocks of 32; a sweep pairs the blocks round-robin, each pair's 64 x 64 sub-matrix is diagonalised in LDS
 *      by one workgroup (32 disjoint rotations per step, Rutishauser's formulas, exact-zero rotations skipped so padding never
 *      couples) and the two-sided update J_k^T A_(k,l) J_l is applied tile by tile.  A problem stops when off(A) = |A - diag A|_F
 *      <= sqrt(npad) eps |A|_F (per-tile partials, one fixed-order sum: identical calls are bit-identical) or after a sweep without
 *      any rotation; at most 40 sweeps (over the cap: HBO_NOT_CONVERGED).  Each diagonalised pair leaves its eigenvalues sorted, the
 *      larger ones in the lower block, which halves the sweep count on Gram matrices.  All arithmetic is fp64; an fp32 input is promoted first.
 *      Matrices of the same padded order run as one batch.  What stays on the host: the promotion, the exact power-of-two scaling
 *      of the input (max |a| into [0.5, 1)), the ordering of the eigenvalues and the O(n) sums of the NLL. */
/* a: [count, n, n] (dtype), only the lower triangle is read.  w_out: [count, n] ascending (numpy.linalg.eigh).  v_out (nullable):
 * [count, n, n], column j belongs to w[j].  w_out does not depend on whether v_out is given (bit for bit).  A matrix that did not
 * converge or held NaN / inf gets NaN outputs and the call returns HBO_NOT_CONVERGED. */
int hbo_sym_eig(hbo_ctx* ctx, int dtype, const void* a, int64_t n, int32_t count, double* w_out, double* v_out);
/* The SVD variant of the NLL (objectives.py:157-176) over the device-resident tasks of `ds`: per task, K = Gram + (noise + eps) I
 * (built on the device exactly as hbo_gram, the diagonal added in the model dtype, then promoted to fp64) = Q diag(w) Q^T, the
 * column y~ = (Y - mu) 1 carried through the rotations (no eigenvectors are formed), and
 *   nll = 0.5 (sum_i (Q^T y~)_i^2 / w_i + m^2 (sum_i log |w_i| + n log 2 pi))
 * -- the reference's value incl. the (m,m)+scalar broadcast for m > 1 (s = |w|; K^-1 keeps the sign of w as the SVD's V S^-1 U^T
 * does; an exact zero eigenvalue gives the IEEE result, inf or NaN, as its 1/s).  Output conventions of hbo_nll (sums over tasks,
 * per task in the dataset's order); abs_eig_min_per_task (nullable): min |w_i|, the reference's s[-1].  No gradient. */
int hbo_nll_spectral(hbo_ctx* ctx, const hbo_model* model, hbo_dataset* ds, double* nll_sum, double* nll_per_task,
                     double* abs_eig_min_per_task);

/* ---- multi-GPU: one process per GPU; sum-all-reduce of [nll, grads] over RCCL (xGMI) ------ */
#define HBO_UNIQUE_ID_BYTES 128
int hbo_comm_unique_id(void* out128);
int hbo_comm_init(hbo_ctx* ctx, int rank, int nranks, const void* unique_id128);
int hbo_comm_allreduce_sum(hbo_ctx* ctx, double* buf, int32_t count);   /* host buffer: up, all-reduce, down (tests, small ad-hoc sums) */
int hbo_comm_destroy(hbo_ctx* ctx);
/* The task-sharded objective (objectives.py:181-195 is an independent sum over sub-datasets; `ds` = this rank's shard, may be
 * NULL / empty: a rank beyond the task count contributes zeros).  Like hbo_objective, but value_sum / count / grad_sum are the sums
 * over ALL ranks of the communicator bound with hbo_comm_init: every rank reduces its own tasks' [value, count, gradient] on the
 * device (same summation order as hbo_objective's host loop), ONE ncclAllReduce runs in place on the context's stream (RCCL over
 * xGMI, no host hop) and the result comes back in one copy.  timing (nullable, 2 doubles): [0] ms of device time this rank spent
 * on its own shard before the collective, [1] us from there to the end of the all-reduce (HIP events on the context's stream).
 * Without a communicator the sums are the local ones.  Returns HBO_NOT_PD when the reduced value is NaN. */
int hbo_objective_sharded(hbo_ctx* ctx, const hbo_model* model, hbo_dataset* ds, int objective, double* value_sum,
                          double* count, double* grad_sum, double* timing);

/* ---- gp.py:53-195 infer_parameters(method='adam'): K Adam steps queued on the device ------------------------------------
 * Each step is stream-ordered launches with no host wait: [gather this step's rows] -> the single-workgroup evaluation (with the
 * MLP / Kumaraswamy forward and backward passes around it) -> the reduction of [nll_sum, T, grad] in the caller's layout (the order
 * of summation of hbo_objective) -> one Adam step in one workgroup, which chains the gradient through the warps, updates x and
 * writes the next (warped) model where the following step's launches read it.  One copy back and one synchronisation per call.
 *
 * The raw parameter vector x is lbfgs.tree_flatten(params.model); leaves[i] says how x[i] becomes a field of the model:
 *   warp      hbo_train_warp (utils.py:28-81, the closed set the host chain rule knows)
 *   target    hbo_train_target; NONE = the model does not read it (zero gradient: Adam leaves it where it is)
 *   layer     MLP layer of an MLP_KERNEL / MLP_BIAS leaf, else 0
 *   index     element within the target ([in, out] row-major for MLP_KERNEL); 0 for the scalar targets
 *   round_f32 1: the leaf is float32 in params.model (the host rounds x to float32 before the warp, and the warp result too)
 * Array targets (lengthscale, linear kernel, MLP weights, Kumaraswamy a, b) are rounded to the model dtype as the host's copy is.
 * `model` supplies the family and the starting values (its warped fields must be the ones x gives); fields no leaf targets keep
 * the model's value.  x, adam_m, adam_v [P]: in / out, the Adam state carried from call to call.  bias1[s], bias2[s]: 1 - b1**t,
 * 1 - b2**t of step s as the host computes them.  Adam is evaluated operation by operation as gp.py:_Adam.step (no contraction):
 * from the same gradient the update is bit-identical to the host's.
 *   batch_counts / batch_rows (both null: the whole of `ds` every step): per step, hbo_dataset_subsample's counts [T] and rows
 *   (steps x T counts, the rows of the steps back to back); every step must keep the same counts (only the rows change).
 *   losses [steps]: nll_sum / T of each step (written up to and including the first non-finite one).  x_trace (nullable)
 *   [steps][P]: x as evaluated at each step.  *steps_done: the first step whose loss was not finite (x, adam_m, adam_v are then
 *   the ones evaluated there, not updated), or `steps`.
 * Only the fused regime is accepted: every task of the batch has n <= 128, the hbo_tune option small_fused is on and the device
 * gives the single-workgroup evaluation its LDS; otherwise HBO_ERR_UNSUPPORTED.  The arguments are checked before any HIP call
 * (HBO_ERR_ARG, hbo_last_error names the argument). */
enum hbo_train_warp { HBO_TRAIN_WARP_IDENTITY = 0, HBO_TRAIN_WARP_SOFTPLUS = 1, HBO_TRAIN_WARP_SOFTPLUS_EPS = 2, HBO_TRAIN_WARP_SQUAREPLUS = 3 };
enum hbo_train_target {
  HBO_TRAIN_NONE = 0, HBO_TRAIN_LENGTHSCALE = 1, HBO_TRAIN_SIGNAL_VARIANCE = 2, HBO_TRAIN_NOISE_VARIANCE = 3, HBO_TRAIN_CONSTANT = 4,
  HBO_TRAIN_DOT_PROD_SIGMA = 5, HBO_TRAIN_DOT_PROD_BIAS = 6, HBO_TRAIN_LINEAR_KERNEL = 7, HBO_TRAIN_LINEAR_BIAS = 8,
  HBO_TRAIN_MLP_KERNEL = 9, HBO_TRAIN_MLP_BIAS = 10, HBO_TRAIN_KUMAR_A = 11, HBO_TRAIN_KUMAR_B = 12
};
typedef struct hbo_train_leaf {
  int32_t warp;
  int32_t target;
  int32_t layer, index;
  int32_t round_f32;
} hbo_train_leaf;
int hbo_train_adam(hbo_ctx* ctx, const hbo_model* model, hbo_dataset* ds, const hbo_train_leaf* leaves, int32_t P,
                   double* x, double* adam_m, double* adam_v, const double* bias1, const double* bias2,
                   int32_t steps, double lr, double b1, double b2, double adam_eps,
                   const int64_t* batch_counts, const int32_t* batch_rows,
                   double* losses, double* x_trace, int32_t* steps_done);

/* ---- gp.py:53-195 infer_parameters(method='lbfgs'): the evaluations of basics/lbfgs.py queued on the device ----------------
 * L-BFGS evaluates one batch over and over: at the start, once per main step, and up to ls_steps times per line search.  One call
 * queues `evals` evaluations on the stream with no host wait between them; each is the launches of hbo_train_adam's resident batch
 * (single-workgroup evaluation with its MLP / Kumaraswamy passes -> reduction of [nll_sum, T, grad]) followed by one control
 * workgroup.  That workgroup chains [nll_sum / T, grad / T] through the leaves' warps (as the Adam step does, round_f32 included),
 * runs the state machine of lbfgs.lbfgs / backtracking_linesearch / lbfgs_descent_dir_nocedal on it (csrc/lbfgs_ctl.h: every decision
 * as the host takes it, NaN comparisons included; dot products in one fixed order, no fused multiply-adds, no atomics), writes the
 * warped model of the next point where the following evaluation reads it, and appends one entry to the log.  One upload, one copy back
 * and one synchronisation per call.
 *
 * leaves, P: as hbo_train_adam.  opts: lbfgs()'s memory, ls_steps, steps (max_iters), alpha, tol, and the line search's c1, c2, growth
 * factor (2.1) and ls_tau.
 *   state [hbo_lbfgs_state_doubles(P, memory)], in / out: the whole run -- iterate, pending point, old_x, old_g, direction, the
 *     ring of s / y pairs, alpha, cur_val, g.d, phase and counters.  All zero: the run starts at x.  Otherwise the run continues
 *     where the call that left the state stopped (same P and memory), and x is not read.
 *   model: the family, and the warped fields of the point evaluated first -- x for a fresh state, the x_next of the previous call
 *     otherwise.  A continued run evaluates that point again with the model the device derives from the state (the device's own
 *     warps), so a run gives the same bits however it is cut into calls.
 *   x [P]: in, the start (fresh state); out, the iterate lbfgs() would return if it stopped now.
 *   log [evals]: one entry per queued evaluation, in order.  kind START (the first evaluation; iter 0), MAIN (the evaluation that
 *     opens main step `iter`, 1..max_iters) or LINE_SEARCH (a probe of step `iter`'s search at x + alpha d); value = nll_sum / T there.
 *     START and MAIN entries are lbfgs()'s callback points (step = iter, loss = value, the parameters = the point evaluated), with
 *     one exception: the MAIN entry at which the run stops with CONVERGED (lbfgs() leaves its loop before the callback).  Once a stop
 *     status is set every later slot is IDLE: its evaluation ran on the last model and was ignored.
 *   x_trace (nullable) [evals][P]: the point of each evaluation (rows of IDLE slots are not written).
 *   x_next (nullable) [P]: the point the next call evaluates first.
 *   *evals_done: entries of the log before the first IDLE one.  *status: hbo_lbfgs_status after the last of them.
 * A state that has already stopped returns at once with *evals_done = 0.  L-BFGS never fails on NaN: a NaN value at the start runs
 * ls_steps probes and stops with NO_PROGRESS, x unchanged.
 * NLL only, and only the fused regime (every task n <= 128, small_fused on, enough LDS; otherwise HBO_ERR_UNSUPPORTED).  The arguments
 * are checked before any HIP call (HBO_ERR_ARG, hbo_last_error names the argument): those of hbo_train_adam, and memory < 1,
 * ls_steps < 1, max_iters < 1, options that are not numbers, null state / log / evals_done / status, a state that is neither all zero
 * nor one an earlier call left. */
enum hbo_lbfgs_kind { HBO_LBFGS_START = 0, HBO_LBFGS_MAIN = 1, HBO_LBFGS_LINE_SEARCH = 2, HBO_LBFGS_IDLE = 3 };
enum hbo_lbfgs_status {
  HBO_LBFGS_RUNNING = 0, HBO_LBFGS_CONVERGED_AT_START = 1, HBO_LBFGS_CONVERGED = 2, HBO_LBFGS_NO_PROGRESS = 3, HBO_LBFGS_INSTABILITY = 4,
  HBO_LBFGS_STEPS_DONE = 5
};
typedef struct hbo_lbfgs_opts {
  int32_t memory, ls_steps, max_iters;
  double alpha, tol, c1, c2, grow, tau;
} hbo_lbfgs_opts;
typedef struct hbo_lbfgs_eval {
  int32_t kind, iter;
  double alpha, value;
} hbo_lbfgs_eval;
int64_t hbo_lbfgs_state_doubles(int32_t P, int32_t memory);
int hbo_train_lbfgs(hbo_ctx* ctx, const hbo_model* model, hbo_dataset* ds, const hbo_train_leaf* leaves, int32_t P,
                    const hbo_lbfgs_opts* opts, double* x, double* state, int32_t evals, hbo_lbfgs_eval* log, double* x_trace,
                    double* x_next, int32_t* evals_done, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* HBO_H_ */
