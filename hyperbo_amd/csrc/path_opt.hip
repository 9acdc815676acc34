// Value and d/dx of posterior sample paths at single points, and their maximisation over a box (hbo_sample_paths_grad,
// hbo_paths_maximize; include/hbo.h).  With v the weights paths.hip: path_solve leaves (the solve of hbo_sample_paths with the
// deviation scale c on the amplitude and the noise draw), a path is a closed-form function of x that needs no factor:
//   f_s(x) = m(x) + c p_s(x) + sum_i k(x, X_i) v[i,s]                      O(F D + n D) per point
//   SE / Matern:  p_s = A sum_j w[j,s] cos(omega_j . x + b_j)
//                 df/dx_d = -c A sum_j w[j,s] sin(omega_j . x + b_j) omega_jd + sum_i v[i,s] dk/du_i 2 (x_d - X_id) / ls_d^2
//   dot product:  p_s = sum_d w[d,s] x_d / sigma + bias w[D,s];   df/dx_d = c w[d,s] / sigma + sum_i v[i,s] X_id / sigma^2
//   a linear mean adds lin_w[d].  A Matern pair at zero distance contributes 0 (kernfun.h: dk_du), as hbo_acq_grad.
// path_vg_kernel: one workgroup of 256 threads per (point, path) pair; the features are the raw x.
//   Tiles.  Observations are walked PO_OT = 256 at a time (one per thread).  Features are walked FT(D) at a time, the largest power of
//   two in 16..256 with FT x D <= PO_OM = 4096 elements (D <= 16: 256, <= 32: 128, <= 64: 64, <= 128: 32, <= 256: 16): the tile of
//   omega [FT][D] is staged in LDS ONCE and read twice, for the arguments omega_j . x (256 / FT threads per feature, d strided among
//   them, their partials added in thread order) and for the gradient sum over j.
//   Sums.  Sine and cosine are taken in the model dtype, everything else in fp64.  The gradient sums over features / observations run
//   in G = 256 / pow2(D) groups (group g: j or i = g, g + G, ... within each tile, tiles in order), added group by group at the end;
//   the value sums per thread, then kernfun.h: block_sum.  No atomics: the order is fixed by (n, F, D) alone, a pair reads nothing
//   another pair writes, so its result does not depend on what shares the launch and identical calls are bit-identical.
//   Loads come from clamped, valid addresses; what lies beyond F or n is masked to zero by a select.
// hbo_paths_maximize puts this kernel in front of the control kernel of hbo_acq_maximize (acq_opt.hip: acq_opt_ctl_kernel over
// acq_opt_ctl.h), one "start" per (path, start) pair and one "sample" each: `evals` rounds of two launches, one synchronisation.
#include "acq_opt_host.h"
#include "kernfun.h"

namespace {
constexpr int PO_OT = 256;    // observations per tile
constexpr int PO_OM = 4096;   // elements of omega per feature tile
constexpr int PO_FT_MIN = 16, PO_FT_MAX = 256;

__host__ __device__ inline int path_opt_feature_tile(int D) {
  int ft = PO_FT_MAX;
  while (ft > PO_FT_MIN && ft * D > PO_OM) ft >>= 1;
  return ft;
}

__device__ __forceinline__ void po_sincos(double x, double* s, double* c) { *s = sin(x); *c = cos(x); }
__device__ __forceinline__ void po_sincos(float x, double* s, double* c) { *s = (double)sinf(x); *c = (double)cosf(x); }

struct PathOptArgs {
  const void* x;                    // [P][D] points, model dtype
  int S, R;                         // R > 0: grid (P): pair p is path p / R at point p.  R == 0: grid (P, S): every path at every point
  int D, F, n, is_dot, bad;         // bad: the cache is not positive definite -- NaN results
  const void* omega; const void* phase; const void* w;   // [F][D], [F], [F][S], model dtype (omega / phase unused by the dot product)
  const void* X;                    // [n][D] the cached observations, model dtype
  const double* v; int64_t vld;     // [S][vld] weights of the update term
  double c, cA;                     // deviation scale; scale x amplitude
  void* out;                        // nullable: [pairs] values in the model dtype
  double* val64;                    // nullable: the same in fp64
  double* grad;                     // [pairs][D]
};

template <typename T>
__global__ __launch_bounds__(256) void path_vg_kernel(PathOptArgs a, const ModelDev* __restrict__ md) {
  __shared__ T s_om[PO_OM + PO_FT_MAX];   // the feature tile, row stride D | 1
  __shared__ double s_x[HBO_MAX_FEATURE_DIM], s_il[HBO_MAX_FEATURE_DIM];
  __shared__ double s_part[256];          // partial arguments; then the observations' weights
  __shared__ double s_cf[PO_FT_MAX];      // w[j,s] sin(arg_j) of the tile
  __shared__ double s_acc[256];
  __shared__ double sred[4];
  const int tid = threadIdx.x;
  const int D = a.D, F = a.F, S = a.S, n = a.n;
  const int64_t p = blockIdx.x;
  const int s = a.R ? (int)(p / a.R) : (int)blockIdx.y;
  const int64_t o = a.R ? p : p * S + s;
  double* g = a.grad + o * D;
  if (a.bad) {   // (uniform)
    if (tid == 0) { if (a.out) static_cast<T*>(a.out)[o] = (T)NAN; if (a.val64) a.val64[o] = NAN; }
    for (int d = tid; d < D; d += 256) g[d] = NAN;
    return;
  }
  const T* x = static_cast<const T*>(a.x) + p * D;
  const T* w = static_cast<const T*>(a.w);
  const int kid = md->kernel_id, mean_id = md->mean_id;
  const bool is_dot = a.is_dot;
  for (int d = tid; d < D; d += 256) { s_x[d] = (double)x[d]; s_il[d] = md->inv_ls[d]; }
  int FD = 1; while (FD < D) FD <<= 1;
  const int G = 256 / FD, grp = tid / FD, dl = tid % FD;
  const int dc = dl < D ? dl : D - 1;
  const double inv_sigma = 1.0 / md->dot_sigma, inv_sigma2 = inv_sigma * inv_sigma, bias = md->dot_bias;
  __syncthreads();
  // ---- the prior path: value sum in vacc (per thread), gradient sum in gacc (thread = (group, d))
  double vacc = 0, gacc = 0;
  if (is_dot) {
    if (tid < D) vacc = s_x[tid] * inv_sigma * (double)w[(int64_t)tid * S + s];
  } else {
    const T* om = static_cast<const T*>(a.omega);
    const T* ph = static_cast<const T*>(a.phase);
    const int ft = path_opt_feature_tile(D), lpf = 256 / ft, DS = D | 1;
    const int jl = tid / lpf, l = tid % lpf;
    for (int j0 = 0; j0 < F; j0 += ft) {
      __syncthreads();   // the previous tile is no longer read
      const int64_t last = (int64_t)F * D - 1;
      for (int idx = tid; idx < ft * D; idx += 256) {
        const int jj = idx / D, dd = idx - jj * D;
        const int64_t ga = (int64_t)j0 * D + idx;   // (the rows of a tile are contiguous)
        const T val = om[ga < last ? ga : last];
        s_om[jj * DS + dd] = j0 + jj < F ? val : (T)0;
      }
      __syncthreads();
      double part = 0;
      for (int d = l; d < D; d += lpf) part += (double)s_om[jl * DS + d] * s_x[d];
      s_part[tid] = part;
      __syncthreads();
      if (l == 0) {
        double arg = 0;
        for (int k = 0; k < lpf; ++k) arg += s_part[tid + k];
        const int j = j0 + jl, jc = j < F ? j : F - 1;
        const double wj = (double)w[(int64_t)jc * S + s];
        double sn, cs;
        po_sincos((T)(arg + (double)ph[jc]), &sn, &cs);
        vacc += j < F ? cs * wj : 0.0;
        s_cf[jl] = j < F ? sn * wj : 0.0;
      }
      __syncthreads();
      const int jn = min(ft, F - j0);
      if (dl < D)
        for (int jj = grp; jj < jn; jj += G) gacc += s_cf[jj] * (double)s_om[jj * DS + dl];
    }
  }
  const double psum = block_sum(vacc, sred);
  // ---- the update term over the observations: value sum in kacc, gradient sum in oacc
  double kacc = 0, oacc = 0;
  if (n > 0) {
    const ExpCoef ec = hbo_exp_coef();
    const T* X = static_cast<const T*>(a.X);
    const double* v = a.v + (int64_t)s * a.vld;
    const double sv = md->sv;
    for (int i0 = 0; i0 < n; i0 += PO_OT) {
      const int i = i0 + tid, ic = i < n ? i : n - 1;
      const T* Xi = X + (int64_t)ic * D;
      const double vi = i < n ? v[ic] : 0.0;
      double u = 0, k, wt;
      if (is_dot) {
        for (int d = 0; d < D; ++d) u += s_x[d] * (double)Xi[d];
        k = u * inv_sigma2 + bias * bias;
        wt = vi * inv_sigma2;
      } else {
        for (int d = 0; d < D; ++d) { const double df = (s_x[d] - (double)Xi[d]) * s_il[d]; u += df * df; }
        k = kfun(kid, u, sv, 1.0, 0.0, ec);
        wt = vi * dk_du(kid, u, k, sv, ec) * 2.0;
      }
      kacc += k * vi;
      __syncthreads();   // the previous tile's weights are no longer read
      s_part[tid] = i < n ? wt : 0.0;
      __syncthreads();
      const int lim = min(PO_OT, n - i0);
      for (int ii = grp; ii < lim; ii += G) {
        const double fi = (double)X[(int64_t)(i0 + ii) * D + dc];
        oacc += is_dot ? s_part[ii] * fi : s_part[ii] * (s_x[dc] - fi);
      }
    }
  }
  const double ksum = block_sum(kacc, sred);
  double mean = 0;
  if (mean_id == HBO_MEAN_CONSTANT) mean = md->constant;
  else if (mean_id == HBO_MEAN_LINEAR) mean = md->linear_bias + block_sum(tid < D ? s_x[tid] * md->lin_w[tid] : 0.0, sred);
  if (tid == 0) {
    const double prior = is_dot ? psum + bias * (double)w[(int64_t)D * S + s] : psum;
    const double val = (mean + a.cA * prior) + ksum;
    if (a.out) static_cast<T*>(a.out)[o] = (T)val;
    if (a.val64) a.val64[o] = (double)(T)val;   // the optimiser sees the value hbo_sample_paths_grad returns: a number of the model dtype
  }
  // ---- the groups' partial gradient sums meet in group order
  __syncthreads();
  s_acc[tid] = gacc;
  __syncthreads();
  double pr = 0;
  if (grp == 0 && dl < D) for (int gg = 0; gg < G; ++gg) pr += s_acc[gg * FD + dl];
  __syncthreads();
  s_acc[tid] = oacc;
  __syncthreads();
  if (grp == 0 && dl < D) {
    double ob = 0;
    for (int gg = 0; gg < G; ++gg) ob += s_acc[gg * FD + dl];
    double r;
    if (is_dot) r = a.c * inv_sigma * (double)w[(int64_t)dl * S + s] + ob;
    else r = -a.cA * pr + ob * (s_il[dl] * s_il[dl]);
    if (mean_id == HBO_MEAN_LINEAR) r += md->lin_w[dl];
    g[dl] = r;
  }
}

void launch_path_vg(int dtype, const PathOptArgs& a, int64_t P, const ModelDev* md, hipStream_t st) {
  if (P <= 0) return;
  const dim3 grid((unsigned)P, a.R ? 1u : (unsigned)a.S);
  if (dtype == HBO_F64) hipLaunchKernelGGL((path_vg_kernel<double>), grid, dim3(256), 0, st, a, md);
  else hipLaunchKernelGGL((path_vg_kernel<float>), grid, dim3(256), 0, st, a, md);
}

// the checks both entry points share beyond path_check: the deviation scale, then the models the kernel does not cover
int path_opt_check(hbo_ctx* c, const std::string& fn, const hbo_model* m, double dev_scale) {
  if (!isfinite(dev_scale) || !(dev_scale > 0.0)) return fail(c, HBO_ERR_ARG, fn + "dev_scale must be a finite number > 0");
  if (m->kernel_uses_mlp) return fail(c, HBO_ERR_UNSUPPORTED, fn + "a kernel on an MLP basis is not supported; evaluate the paths with hbo_sample_paths");
  if (m->mean_id == HBO_MEAN_LINEAR_MLP) return fail(c, HBO_ERR_UNSUPPORTED, fn + "a linear_mlp mean is not supported; evaluate the paths with hbo_sample_paths");
  if (is_kumar(m)) return fail(c, HBO_ERR_UNSUPPORTED, fn + "input-warped (Kumaraswamy) models are not supported; evaluate the paths with hbo_sample_paths");
  return HBO_OK;
}

// the kernel's arguments once the draws and the weights are on the device
PathOptArgs path_opt_args(const hbo_model* m, const hbo_cache* k, int32_t S, int32_t F, const PathSolve& sol, double dev_scale) {
  PathOptArgs a = {};
  a.S = S; a.D = m->input_dim; a.F = F; a.n = k ? (int)k->t->n : 0; a.is_dot = m->kernel_id == HBO_KERNEL_DOT; a.bad = k && k->info != INT_MAX;
  a.omega = sol.om; a.phase = sol.ph; a.w = sol.w; a.X = k ? k->h_desc.F : nullptr; a.v = sol.v; a.vld = sol.vld;
  a.c = dev_scale; a.cA = dev_scale * sol.A;
  return a;
}
}  // namespace

extern "C" int hbo_sample_paths_grad(hbo_ctx* c, const hbo_model* m, hbo_cache* k, const void* xq, int64_t M, int32_t S, int32_t F,
                                     const void* omega, const void* phase, const void* w, const void* eps, double dev_scale, void* out,
                                     double* grad_out) {
  const std::string fn = "hbo_sample_paths_grad: ";
  // ---- every argument check, before any device call ----
  if (!m || !xq || !omega || !phase || !w || !out || !grad_out) return fail(c, HBO_ERR_ARG, fn + "null argument");
  if (int rc = path_check(c, fn, m, k, S, F, eps != nullptr)) return rc;
  if (int rc = path_opt_check(c, fn, m, dev_scale)) return rc;
  if (M > (int64_t)INT_MAX) return fail(c, HBO_ERR_ARG, fn + "M must be below 2^31");
  if (!c) return fail(c, HBO_ERR_ARG, fn + "ctx is null");
  if (M <= 0) return HBO_OK;
  const int dtype = m->dtype, D = m->input_dim;
  const bool bad = k && k->info != INT_MAX;
  if (bad) { fill_nan(out, (size_t)M * S, dtype); fill_nan(grad_out, (size_t)M * S * D, HBO_F64); return HBO_NOT_PD; }
  HIPCHK(c, hipSetDevice(c->device));
  prof_begin(c);
  if (int rc = upload_model(c, m)) return rc;
  const size_t es = esize(dtype);
  hipStream_t st = c->stream;
  const size_t grad_b = align256(sizeof(double) * (size_t)M * S * D), val_b = (size_t)M * S * es;
  void* d_xq = ws_get(c, WS_XQ, (size_t)M * D * es);
  char* d_out = static_cast<char*>(ws_get(c, WS_PO_OUT, grad_b + val_b));
  if (!d_xq || !d_out) return HBO_ERR_HIP;
  HIPCHK(c, hipMemcpyAsync(d_xq, xq, (size_t)M * D * es, hipMemcpyHostToDevice, st));
  PathSolve sol = {};
  if (int rc = path_solve(c, m, k, S, F, omega, phase, w, eps, dev_scale, 0, &sol)) return rc;
  PathOptArgs a = path_opt_args(m, k, S, F, sol, dev_scale);
  a.x = d_xq; a.R = 0; a.grad = reinterpret_cast<double*>(d_out); a.out = d_out + grad_b;
  { ProfScope ps(c, "path_vg", 1);
    launch_path_vg(dtype, a, M, c->d_model, st); }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(grad_out, d_out, sizeof(double) * (size_t)M * S * D, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(out, d_out + grad_b, val_b, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  prof_collect(c);
  return HBO_OK;
}

extern "C" int hbo_paths_maximize(hbo_ctx* c, const hbo_model* m, hbo_cache* k, int32_t S, int32_t F, const void* omega, const void* phase,
                                  const void* w, const void* eps, double dev_scale, const void* x0, int32_t R, const double* lo,
                                  const double* hi, const hbo_acq_opt_opts* opts, double* state, int32_t evals, double* x_out,
                                  double* val_out, int32_t* status, hbo_acq_opt_eval* log) {
  const std::string fn = "hbo_paths_maximize: ";
  // ---- every argument check, before any device call ----
  if (!m || !omega || !phase || !w || !x0 || !state || !x_out || !val_out || !status) return fail(c, HBO_ERR_ARG, fn + "null argument");
  if (int rc = path_check(c, fn, m, k, S, F, eps != nullptr)) return rc;
  if (!isfinite(dev_scale) || !(dev_scale > 0.0)) return fail(c, HBO_ERR_ARG, fn + "dev_scale must be a finite number > 0");
  if (R < 1 || (int64_t)S * R > 4096) return fail(c, HBO_ERR_ARG, fn + "need R >= 1 and S * R <= 4096");
  if (evals <= 0 || evals > 4096) return fail(c, HBO_ERR_ARG, fn + "1 <= evals <= 4096");
  if (int rc = acq_opt_check_opts(c, fn, opts)) return rc;
  const int dtype = m->dtype, D = m->input_dim, P = S * R;
  if (int rc = acq_opt_check_box(c, fn, lo, hi, D, dtype)) return rc;
  const int64_t ns = hbo_acq_opt_state_size(D, opts->memory);
  std::vector<double> xs(D);
  bool lds_ok = acq_opt_lds_bytes(ns) <= ACQ_OPT_LDS_MAX;
  for (int r = 0; r < P && lds_ok; ++r) {
    double* sr = state + r * ns;
    bool fresh = false;
    if (int rc = acq_opt_check_state(c, fn, sr, opts, &fresh)) return rc;
    if (!fresh) continue;
    for (int i = 0; i < D; ++i) xs[i] = host_elem(x0, dtype, (int64_t)r * D + i);
    if (!acq_opt_in_box(xs.data(), lo, hi, D)) return fail(c, HBO_ERR_ARG, fn + "a start lies outside the box (or is not finite)");
  }
  if (int rc = path_opt_check(c, fn, m, dev_scale)) return rc;
  if (!lds_ok) return fail(c, HBO_ERR_UNSUPPORTED, fn + "the state of a start (input_dim, opts.memory) does not fit 64 KB of LDS");
  if (!c) return fail(c, HBO_ERR_ARG, fn + "ctx is null");

  HIPCHK(c, hipSetDevice(c->device));
  prof_begin(c);
  if (int rc = upload_model(c, m)) return rc;
  const size_t es = esize(dtype);
  hipStream_t st = c->stream;
  PathSolve sol = {};
  if (int rc = path_solve(c, m, k, S, F, omega, phase, w, eps, dev_scale, 0, &sol)) return rc;
  // one block up: [lo, hi][P x D pending points][P states]; the log follows the states, and one copy brings [states | log] back.
  // Scratch of the rounds: [P x D gradients][P values fp64]
  const size_t box_b = align256(sizeof(double) * 2 * D), pend_b = align256((size_t)P * D * es), state_b = align256(sizeof(double) * (size_t)P * ns);
  const size_t log_b = log ? sizeof(hbo_acq_opt_eval) * (size_t)evals * P : 0;
  const size_t o_state = box_b + pend_b, up_b = o_state + state_b, down_b = state_b + log_b;
  const size_t grad_b = align256(sizeof(double) * (size_t)P * D), val_b = align256(sizeof(double) * (size_t)P);
  char* d_in = static_cast<char*>(ws_get(c, WS_PO_IN, up_b + log_b));
  char* d_out = static_cast<char*>(ws_get(c, WS_PO_OUT, grad_b + val_b));
  if (!d_in || !d_out) return HBO_ERR_HIP;
  char* stage = static_cast<char*>(stage_begin(c, fn.c_str(), up_b + log_b));
  if (!stage) return HBO_ERR_HIP;
  double* hbox = reinterpret_cast<double*>(stage);
  for (int i = 0; i < D; ++i) { hbox[i] = lo ? lo[i] : 0.0; hbox[D + i] = hi ? hi[i] : 1.0; }
  // the states go up from a copy, and a fresh one is started in that copy: the caller's array is written once, by the copy back
  double* hstate = reinterpret_cast<double*>(stage + o_state);
  memcpy(hstate, state, sizeof(double) * (size_t)P * ns);
  char* hpend = stage + box_b;
  for (int r = 0; r < P; ++r) {
    double* sr = hstate + r * ns;
    bool fresh = true;
    for (int q = 0; q < HBO_ACQ_OPT_S_HEADER; ++q) fresh = fresh && sr[q] == 0.0;
    if (fresh) {
      for (int i = 0; i < D; ++i) xs[i] = host_elem(x0, dtype, (int64_t)r * D + i);
      hbo_acq_opt_state_start(sr, D, opts->memory, xs.data());
    }
    const hbo_acq_opt_view v = hbo_acq_opt_view_of(sr, D, opts->memory);
    for (int i = 0; i < D; ++i) {
      if (dtype == HBO_F64) reinterpret_cast<double*>(hpend)[(size_t)r * D + i] = v.xt[i];
      else reinterpret_cast<float*>(hpend)[(size_t)r * D + i] = (float)v.xt[i];
    }
  }
  HIPCHK(c, stage_upload(c, d_in, stage, up_b, st));

  PathOptArgs a = path_opt_args(m, k, S, F, sol, dev_scale);
  a.x = d_in + box_b; a.R = R; a.grad = reinterpret_cast<double*>(d_out); a.val64 = reinterpret_cast<double*>(d_out + grad_b);
  AcqOptArgs ctl = {};
  ctl.o = acq_opt_ctl_opts(opts);
  ctl.state = reinterpret_cast<double*>(d_in + o_state); ctl.ns = ns;
  ctl.lo = reinterpret_cast<const double*>(d_in); ctl.hi = ctl.lo + D;
  ctl.pending = d_in + box_b;
  ctl.vals = a.val64; ctl.grads = a.grad;
  ctl.log = log ? reinterpret_cast<hbo_acq_opt_eval_ctl*>(d_in + up_b) : nullptr;
  ctl.D = D; ctl.R = P; ctl.S = 1;
  if (c->opt_poison && log_b) HIPCHK(c, hipMemsetAsync(d_in + up_b, 0xFF, log_b, st));
  { ProfScope ps(c, "path_maximize", 1);
    for (int e = 0; e < evals; ++e) {
      launch_path_vg(dtype, a, P, c->d_model, st);
      launch_acq_opt_ctl(dtype, ctl, e, st);
    } }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(stage + o_state, d_in + o_state, down_b, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  prof_collect(c);
  memcpy(state, stage + o_state, sizeof(double) * (size_t)P * ns);
  if (log) memcpy(log, stage + up_b, log_b);
  for (int r = 0; r < P; ++r) {
    const hbo_acq_opt_view v = hbo_acq_opt_view_of(state + r * ns, D, opts->memory);
    memcpy(x_out + (size_t)r * D, v.x, sizeof(double) * D);
    val_out[r] = -v.hdr[HBO_ACQ_OPT_S_CUR];
    status[r] = (int32_t)v.hdr[HBO_ACQ_OPT_S_STATUS];
  }
  return a.bad ? HBO_NOT_PD : HBO_OK;
}
