// hbo_acq_maximize: bayesopt()'s inner maximisation of the acquisition function (bayesopt.py:116-125) for R starts in one call.  One
// upload, then per evaluation two stream-ordered launches with no host wait -- acq_small_kernel on grid (R, S) over the starts'
// pending points (acq_small.hip; hbo_acq_maximize_blocked over a cache of n > 128: the four launches of acq_blocked.hip in its
// place), then acq_opt_ctl_kernel, one workgroup per start, which reduces the S per-sample results of its start,
// runs one step of the state machine of acq_opt_ctl.h and writes the next pending point -- and one synchronisation and one copy back.
// A start reads and writes only its own state, its own row of the pending points and its own columns of the per-sample results.
// Also here: the host hook hbo_probe_acq_opt_ctl, the same control text on one thread.
#include "acq_opt_host.h"
#include "../../include/hbo_tune.h"

namespace {
enum { ACQ_OPT_THREADS = 256 };

// One evaluation of one start: the step of acq_opt_ctl.h, the log record, the next pending point in the model dtype (the state's copy
// already holds that rounded value).  The start's state is staged in LDS for the step -- its dot products are chains of dependent
// reads -- and written back whole.  A start that has stopped logs IDLE and leaves its pending point alone.
// Dynamic LDS: [ns doubles: the state][HBO_LBFGS_PARTIALS doubles: the scratch of the sums].
// REDUCE (acq_opt_ctl.h): how the S per-sample results become f -- the mean, or (hbo_logei_maximize) the log of the mean of the exponentials.
template <typename T, int REDUCE>
__global__ __launch_bounds__(ACQ_OPT_THREADS) void acq_opt_ctl_kernel(AcqOptArgs a, int slot) {
  extern __shared__ double acq_opt_lds[];
  double* state = acq_opt_lds;
  double* scratch = acq_opt_lds + a.ns;
  const int tid = threadIdx.x, nthr = ACQ_OPT_THREADS, D = a.D;
  const int64_t r = blockIdx.x;
  double* gstate = a.state + r * a.ns;
  for (int64_t i = tid; i < a.ns; i += nthr) state[i] = gstate[i];
  __syncthreads();
  hbo_acq_opt_eval_ctl ev;
  hbo_acq_opt_ctl_step_t<REDUCE>(state, D, a.o, a.lo, a.hi, sizeof(T) == 4, a.vals + r, a.R, a.grads + r * D, (int64_t)a.R * D, a.S, tid, nthr, scratch, &ev);
  if (tid == 0 && a.log) a.log[(int64_t)slot * a.R + r] = ev;
  if (ev.kind == HBO_ACQ_OPT_CTL_IDLE) return;   // (uniform; nothing of the state has changed)
  for (int64_t i = tid; i < a.ns; i += nthr) gstate[i] = state[i];
  const hbo_acq_opt_view v = hbo_acq_opt_view_of(state, D, a.o.memory);
  T* p = static_cast<T*>(a.pending) + r * D;
  for (int i = tid; i < D; i += nthr) p[i] = (T)v.xt[i];
}
}  // namespace

// ---- shared with path_opt.hip (acq_opt_host.h) ----
size_t acq_opt_lds_bytes(int64_t ns) { return sizeof(double) * (size_t)(ns + HBO_LBFGS_PARTIALS); }

int acq_opt_check_opts(hbo_ctx* c, const std::string& fn, const hbo_acq_opt_opts* o) {
  if (!o) return fail(c, HBO_ERR_ARG, fn + "opts is null");
  if (o->memory < 1 || o->memory > 64) return fail(c, HBO_ERR_ARG, fn + "opts.memory must be in 1..64");
  if (o->ls_steps < 1) return fail(c, HBO_ERR_ARG, fn + "opts.ls_steps must be at least 1");
  if (o->max_iters < 1) return fail(c, HBO_ERR_ARG, fn + "opts.max_iters must be at least 1");
  if (!(o->c1 > 0.0 && o->c1 < 1.0)) return fail(c, HBO_ERR_ARG, fn + "opts.c1 must lie in (0, 1)");
  if (!(o->tau > 0.0 && o->tau < 1.0)) return fail(c, HBO_ERR_ARG, fn + "opts.tau must lie in (0, 1)");
  if (!(o->pgtol >= 0.0) || !(o->ftol >= 0.0)) return fail(c, HBO_ERR_ARG, fn + "opts.pgtol and ftol must be numbers >= 0");
  return HBO_OK;
}
hbo_acq_opt_opts_ctl acq_opt_ctl_opts(const hbo_acq_opt_opts* o) {
  hbo_acq_opt_opts_ctl r;
  r.memory = o->memory; r.ls_steps = o->ls_steps; r.max_iters = o->max_iters; r.c1 = o->c1; r.tau = o->tau; r.pgtol = o->pgtol; r.ftol = o->ftol;
  return r;
}
// A state the control code can index with: a header of zeros (a fresh run), or one hbo_acq_opt_ctl_step left
int acq_opt_check_state(hbo_ctx* c, const std::string& fn, const double* h, const hbo_acq_opt_opts* o, bool* fresh) {
  bool zero = true;
  for (int k = 0; k < HBO_ACQ_OPT_S_HEADER; ++k) zero = zero && h[k] == 0.0;
  *fresh = zero;
  if (zero) return HBO_OK;
  auto whole = [&](int k, double lo, double hi) { return h[k] >= lo && h[k] <= hi && h[k] == (double)(int64_t)h[k]; };
  const bool ok = h[HBO_ACQ_OPT_S_MAGIC] == HBO_ACQ_OPT_MAGIC && whole(HBO_ACQ_OPT_S_PHASE, 0, 1) && whole(HBO_ACQ_OPT_S_STATUS, 0, HBO_ACQ_OPT_CTL_STEPS_DONE) &&
                  whole(HBO_ACQ_OPT_S_ITER, 0, INT_MAX) && whole(HBO_ACQ_OPT_S_PROBES, 0, INT_MAX) && whole(HBO_ACQ_OPT_S_NHIST, 0, o->memory) &&
                  whole(HBO_ACQ_OPT_S_HEAD, 0, o->memory - 1) && whole(HBO_ACQ_OPT_S_EVALS, 0, INT_MAX);
  if (!ok) return fail(c, HBO_ERR_ARG, fn + "state is neither all zero nor one an earlier call with the same input_dim and memory left");
  return HBO_OK;
}
// lo <= hi, both finite, and (fp32 models) fp32 numbers, so that a clipped probe is still inside the box once it is rounded
int acq_opt_check_box(hbo_ctx* c, const std::string& fn, const double* lo, const double* hi, int D, int dtype) {
  if (!lo != !hi) return fail(c, HBO_ERR_ARG, fn + "lo and hi must both be given or both be null");
  if (!lo) return HBO_OK;
  for (int i = 0; i < D; ++i) {
    if (!isfinite(lo[i]) || !isfinite(hi[i]) || lo[i] > hi[i]) return fail(c, HBO_ERR_ARG, fn + "need finite lo <= hi");
    if (dtype == HBO_F32 && ((double)(float)lo[i] != lo[i] || (double)(float)hi[i] != hi[i]))
      return fail(c, HBO_ERR_ARG, fn + "lo and hi of an fp32 model must be fp32 numbers");
  }
  return HBO_OK;
}
bool acq_opt_in_box(const double* x, const double* lo, const double* hi, int D) {
  for (int i = 0; i < D; ++i) {
    const double l = lo ? lo[i] : 0.0, h = hi ? hi[i] : 1.0;
    if (!(x[i] >= l && x[i] <= h)) return false;
  }
  return true;
}
void launch_acq_opt_ctl(int dtype, const AcqOptArgs& a, int slot, hipStream_t st) {
  const dim3 grid(a.R), block(ACQ_OPT_THREADS);
  const size_t lds = acq_opt_lds_bytes(a.ns);
  if (a.reduce == HBO_ACQ_OPT_REDUCE_LME) {
    if (dtype == HBO_F64) hipLaunchKernelGGL((acq_opt_ctl_kernel<double, HBO_ACQ_OPT_REDUCE_LME>), grid, block, lds, st, a, slot);
    else hipLaunchKernelGGL((acq_opt_ctl_kernel<float, HBO_ACQ_OPT_REDUCE_LME>), grid, block, lds, st, a, slot);
    return;
  }
  if (dtype == HBO_F64) hipLaunchKernelGGL((acq_opt_ctl_kernel<double, HBO_ACQ_OPT_REDUCE_MEAN>), grid, block, lds, st, a, slot);
  else hipLaunchKernelGGL((acq_opt_ctl_kernel<float, HBO_ACQ_OPT_REDUCE_MEAN>), grid, block, lds, st, a, slot);
}

extern "C" int64_t hbo_acq_opt_state_doubles(int32_t D, int32_t memory) {
  if (D <= 0 || memory < 1) return 0;
  return hbo_acq_opt_state_size(D, memory);
}

// The body of the maximisers (api_internal.h: AcqRoute, AcqWhat).  The routes differ in the largest cache they take (route.max_n) and,
// with it, in the evaluation step -- one launch of acq_small.hip when every cache has n <= 128, the four launches of acq_blocked.hip
// otherwise.
// (route.allow_mlp -- hbo_acq_maximize_mlp: MLP-basis kernels and linear_mlp means are served; the S weight sets ride up between the
//  pending points and the states, the evaluation runs the pair's forward and backward pass (acq_mlp.h) and the control kernel sees raw
//  points and raw gradients as ever)
// (the MES step -- hbo_mes_maximize, mes.hip: the S x K maxima ride up behind the box)
// (the LogEI step -- hbo_logei_maximize, logei.hip: the S targets ride in the records where the registry's parameters do, and the control
//  kernel combines the samples as the log of the mean of their exponentials (acq_opt_ctl.h: HBO_ACQ_OPT_REDUCE_LME))
int acq_maximize(hbo_ctx* c, const AcqRoute& route, const AcqWhat& what, const hbo_model* models, int32_t S, hbo_cache* const* caches,
                 const void* x0, int32_t R, const double* lo, const double* hi, const double* add_noise, double scale,
                 const hbo_acq_opt_opts* opts, double* state, int32_t evals, double* x_out, double* val_out, int32_t* status,
                 hbo_acq_opt_eval* log) {
  const std::string fn = std::string(route.fn) + ": ";
  const bool mes = what.step == ACQ_STEP_MES, logei = what.step == ACQ_STEP_LOGEI;
  if (!models || !caches || !x0 || !what.given() || !add_noise || !state || !x_out || !val_out || !status) return fail(c, HBO_ERR_ARG, fn + "null argument");
  if (S <= 0 || S > 4096) return fail(c, HBO_ERR_ARG, fn + "1 <= S <= 4096");
  if (int rc = acq_what_check(c, fn, what, S)) return rc;
  if (!c) return fail(c, HBO_ERR_ARG, fn + "ctx is null");
  if (R <= 0 || R > 4096) return fail(c, HBO_ERR_ARG, fn + "1 <= R <= 4096");
  if (evals <= 0 || evals > 4096) return fail(c, HBO_ERR_ARG, fn + "1 <= evals <= 4096");
  if (int rc = acq_opt_check_opts(c, fn, opts)) return rc;
  bool any_bad = false;
  if (int rc = acq_samples_check(c, fn, models, S, caches, route.max_n, &any_bad, route.allow_mlp)) return rc;
  const hbo_model* m0 = &models[0];
  const int dtype = m0->dtype, D = m0->input_dim;
  if (int rc = acq_opt_check_box(c, fn, lo, hi, D, dtype)) return rc;
  const int64_t ns = hbo_acq_opt_state_size(D, opts->memory);
  if (acq_opt_lds_bytes(ns) > ACQ_OPT_LDS_MAX)
    return fail(c, HBO_ERR_UNSUPPORTED, fn + "the state of a start (input_dim, opts.memory) does not fit 64 KB of LDS");
  std::vector<double> xs(D);
  for (int r = 0; r < R; ++r) {
    double* sr = state + r * ns;
    bool fresh = false;
    if (int rc = acq_opt_check_state(c, fn, sr, opts, &fresh)) return rc;
    if (!fresh) continue;
    for (int i = 0; i < D; ++i) xs[i] = host_elem(x0, dtype, (int64_t)r * D + i);
    if (!acq_opt_in_box(xs.data(), lo, hi, D)) return fail(c, HBO_ERR_ARG, fn + "a start lies outside the box (or is not finite)");
  }

  HIPCHK(c, hipSetDevice(c->device));
  const size_t es = esize(dtype);
  hipStream_t st = c->stream;
  const int ldv = acq_blocked_ldv(S, caches);
  const bool blocked = ldv > HBO_TILE;
  const size_t plane = (size_t)S * R * ldv;   // k, l, beta of the blocked evaluation: [S][R][ldv] doubles each
  const AcqVecWidths vw = acq_vec_widths(m0);   // (without an MLP: D and D)
  const AcqMlpPack mlp = acq_mlp_layout(m0, S);
  const size_t work = 3 * plane + (size_t)S * R * mlp.ftot;   // ... and (MLP basis) the activations [S][R][ftot]
  if (blocked) {
    size_t total = 0;
    HIPCHK(c, hipDeviceTotalMem(&total, c->device));
    if (sizeof(double) * work > total / 2)
      return fail(c, HBO_ERR_UNSUPPORTED, fn + "the evaluation workspace (3 x S x R x npad doubles) exceeds half of the device memory; use fewer starts per call");
  }
  // one block up: [S records][S x 2 D doubles][lo, hi][R x D pending points][R states]; the log follows the states, and one copy brings
  // [states | log] back.  Scratch of the rounds: [S x R x D gradients][S x R values fp64][S x R values in the model dtype]
  // (MES: the S x K maxima sit behind the box, in its part of the block)
  const size_t ys_b = mes ? sizeof(double) * (size_t)S * what.K : 0;
  const size_t smp_b = align256(sizeof(AcqSmallSample) * S), vec_b = align256(sizeof(double) * ((size_t)vw.fdim + vw.mdim) * S), box_b = align256(sizeof(double) * 2 * D + ys_b);
  const size_t pend_b = align256((size_t)R * D * es), state_b = align256(sizeof(double) * (size_t)R * ns);
  const size_t log_b = log ? sizeof(hbo_acq_opt_eval) * (size_t)evals * R : 0;
  const size_t o_mlp = smp_b + vec_b + box_b + pend_b, o_state = o_mlp + mlp.bytes, up_b = o_state + state_b, down_b = state_b + log_b;
  const size_t grad_b = align256(sizeof(double) * (size_t)S * R * D), val_b = align256(sizeof(double) * (size_t)S * R), acq_b = (size_t)S * R * es;
  char* d_in = static_cast<char*>(ws_get(c, WS_AO_IN, up_b + log_b));
  char* d_out = static_cast<char*>(ws_get(c, WS_AO_OUT, grad_b + val_b + acq_b));
  if (!d_in || !d_out) return HBO_ERR_HIP;
  double* d_work = blocked ? static_cast<double*>(ws_get(c, WS_AB_WORK, sizeof(double) * work)) : nullptr;
  if (blocked && !d_work) return HBO_ERR_HIP;
  char* stage = static_cast<char*>(stage_begin(c, fn.c_str(), up_b + log_b));
  if (!stage) return HBO_ERR_HIP;
  acq_small_pack(reinterpret_cast<AcqSmallSample*>(stage), reinterpret_cast<double*>(stage + smp_b), models, S, caches, what.params, add_noise);
  double* hbox = reinterpret_cast<double*>(stage + smp_b + vec_b);
  for (int i = 0; i < D; ++i) { hbox[i] = lo ? lo[i] : 0.0; hbox[D + i] = hi ? hi[i] : 1.0; }
  if (mes) memcpy(hbox + 2 * D, what.ystar, ys_b);
  // the states go up from a copy, and a fresh one is started in that copy: the caller's array is written once, by the copy back, so a
  // call that fails on the way (an argument, an allocation, the device) leaves it as it was
  double* hstate = reinterpret_cast<double*>(stage + o_state);
  memcpy(hstate, state, sizeof(double) * (size_t)R * ns);
  char* hpend = stage + smp_b + vec_b + box_b;
  for (int r = 0; r < R; ++r) {
    double* sr = hstate + r * ns;
    bool fresh = true;
    for (int k = 0; k < HBO_ACQ_OPT_S_HEADER; ++k) fresh = fresh && sr[k] == 0.0;
    if (fresh) {
      for (int i = 0; i < D; ++i) xs[i] = host_elem(x0, dtype, (int64_t)r * D + i);
      hbo_acq_opt_state_start(sr, D, opts->memory, xs.data());
    }
    // the pending point, as the state holds it (a number of the model dtype)
    const hbo_acq_opt_view v = hbo_acq_opt_view_of(sr, D, opts->memory);
    for (int i = 0; i < D; ++i) {
      if (dtype == HBO_F64) reinterpret_cast<double*>(hpend)[(size_t)r * D + i] = v.xt[i];
      else reinterpret_cast<float*>(hpend)[(size_t)r * D + i] = (float)v.xt[i];
    }
  }
  AcqSmallArgs a = {};
  acq_mlp_fill(mlp, stage + o_mlp, d_in + o_mlp, models, S, a);
  HIPCHK(c, stage_upload(c, d_in, stage, up_b, st));

  a.smp = reinterpret_cast<const AcqSmallSample*>(d_in); a.vec = reinterpret_cast<const double*>(d_in + smp_b);
  a.xq = d_in + smp_b + vec_b + box_b;
  a.D = D; a.M = R; a.kernel_id = m0->kernel_id; a.mean_id = m0->mean_id; a.step = what.step; a.acq_id = what.acq_id; a.scale = scale;
  a.grad_out = reinterpret_cast<double*>(d_out); a.val64_out = reinterpret_cast<double*>(d_out + grad_b); a.acq_out = d_out + grad_b + val_b;
  if (mes) { a.ystar = reinterpret_cast<const double*>(d_in + smp_b + vec_b) + 2 * D; a.K = what.K; }
  AcqOptArgs k = {};
  k.reduce = logei ? HBO_ACQ_OPT_REDUCE_LME : HBO_ACQ_OPT_REDUCE_MEAN;
  k.o = acq_opt_ctl_opts(opts);
  k.state = reinterpret_cast<double*>(d_in + o_state); k.ns = ns;
  k.lo = reinterpret_cast<const double*>(d_in + smp_b + vec_b); k.hi = k.lo + D;
  k.pending = d_in + smp_b + vec_b + box_b;
  k.vals = a.val64_out; k.grads = a.grad_out;
  k.log = log ? reinterpret_cast<hbo_acq_opt_eval_ctl*>(d_in + up_b) : nullptr;
  k.D = D; k.R = R; k.S = S;
  // hbo_tune poison: the log is written record by record by the control launches; one that was skipped must not pass for an earlier call's
  if (c->opt_poison && log_b) HIPCHK(c, hipMemsetAsync(d_in + up_b, 0xFF, log_b, st));
  AcqBlockedArgs b = {};
  b.a = a; b.ldv = ldv; b.q0 = 0; b.mc = R;
  b.k = d_work; b.l = d_work + plane; b.beta = d_work + 2 * plane;
  b.acts = d_work + 3 * plane; b.ftot = mlp.ftot;
  for (int e = 0; e < evals; ++e) {
    if (blocked) launch_acq_blocked(dtype, b, S, st);
    else launch_acq_small(dtype, a, S, st);
    launch_acq_opt_ctl(dtype, k, e, st);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(stage + o_state, d_in + o_state, down_b, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  memcpy(state, stage + o_state, sizeof(double) * (size_t)R * ns);
  if (log) memcpy(log, stage + up_b, log_b);
  for (int r = 0; r < R; ++r) {
    const hbo_acq_opt_view v = hbo_acq_opt_view_of(state + r * ns, D, opts->memory);
    memcpy(x_out + (size_t)r * D, v.x, sizeof(double) * D);
    val_out[r] = -v.hdr[HBO_ACQ_OPT_S_CUR];
    status[r] = (int32_t)v.hdr[HBO_ACQ_OPT_S_STATUS];
  }
  return any_bad ? HBO_NOT_PD : HBO_OK;
}
extern "C" int hbo_acq_maximize(hbo_ctx* c, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* x0, int32_t R,
                                const double* lo, const double* hi, int acq_id, const double* params, const double* add_noise, double scale,
                                const hbo_acq_opt_opts* opts, double* state, int32_t evals, double* x_out, double* val_out, int32_t* status,
                                hbo_acq_opt_eval* log) {
  return acq_maximize(c, ACQ_ROUTE_SMALL.named("hbo_acq_maximize"), acq_what_registry(acq_id, params), models, S, caches, x0, R, lo, hi, add_noise,
                      scale, opts, state, evals, x_out, val_out, status, log);
}
extern "C" int hbo_acq_maximize_blocked(hbo_ctx* c, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* x0, int32_t R,
                                        const double* lo, const double* hi, int acq_id, const double* params, const double* add_noise,
                                        double scale, const hbo_acq_opt_opts* opts, double* state, int32_t evals, double* x_out,
                                        double* val_out, int32_t* status, hbo_acq_opt_eval* log) {
  return acq_maximize(c, ACQ_ROUTE_BLOCKED.named("hbo_acq_maximize_blocked"), acq_what_registry(acq_id, params), models, S, caches, x0, R, lo, hi,
                      add_noise, scale, opts, state, evals, x_out, val_out, status, log);
}
extern "C" int hbo_acq_maximize_mlp(hbo_ctx* c, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* x0, int32_t R,
                                    const double* lo, const double* hi, int acq_id, const double* params, const double* add_noise,
                                    double scale, const hbo_acq_opt_opts* opts, double* state, int32_t evals, double* x_out,
                                    double* val_out, int32_t* status, hbo_acq_opt_eval* log) {
  return acq_maximize(c, ACQ_ROUTE_MLP.named("hbo_acq_maximize_mlp"), acq_what_registry(acq_id, params), models, S, caches, x0, R, lo, hi, add_noise,
                      scale, opts, state, evals, x_out, val_out, status, log);
}

// include/hbo_tune.h (TEST HOOK): the control code of acq_opt_ctl.h on the host, one thread, for one evaluation of one start
extern "C" int hbo_probe_acq_opt_ctl(double* state, int32_t D, int dtype, const hbo_acq_opt_opts* opts, const double* lo, const double* hi,
                                     const double* x0, const double* vals, const double* grads, int32_t S, double* x_next, double* x_iter,
                                     hbo_acq_opt_eval* eval, int32_t* status) {
  const std::string fn = "hbo_probe_acq_opt_ctl: ";
  if (D <= 0 || D > HBO_MAX_FEATURE_DIM) return fail(nullptr, HBO_ERR_ARG, fn + "bad input_dim");
  if (dtype != HBO_F32 && dtype != HBO_F64) return fail(nullptr, HBO_ERR_ARG, fn + "bad dtype");
  if (S <= 0 || S > 4096) return fail(nullptr, HBO_ERR_ARG, fn + "1 <= S <= 4096");
  if (!state || !vals || !grads || !x_next || !eval || !status) return fail(nullptr, HBO_ERR_ARG, fn + "null argument (state, vals, grads, x_next, eval, status)");
  if (int rc = acq_opt_check_opts(nullptr, fn, opts)) return rc;
  if (int rc = acq_opt_check_box(nullptr, fn, lo, hi, D, dtype)) return rc;
  bool fresh = false;
  if (int rc = acq_opt_check_state(nullptr, fn, state, opts, &fresh)) return rc;
  if (fresh) {
    if (!x0) return fail(nullptr, HBO_ERR_ARG, fn + "an all-zero state needs x0");
    if (!acq_opt_in_box(x0, lo, hi, D)) return fail(nullptr, HBO_ERR_ARG, fn + "the start lies outside the box (or is not finite)");
    if (dtype == HBO_F32) for (int i = 0; i < D; ++i) if ((double)(float)x0[i] != x0[i]) return fail(nullptr, HBO_ERR_ARG, fn + "the start of an fp32 run must hold fp32 numbers");
    hbo_acq_opt_state_start(state, D, opts->memory, x0);
  }
  const hbo_acq_opt_view v = hbo_acq_opt_view_of(state, D, opts->memory);
  double scratch[HBO_LBFGS_PARTIALS];
  hbo_acq_opt_eval_ctl ev;
  hbo_acq_opt_ctl_step(state, D, acq_opt_ctl_opts(opts), lo, hi, dtype == HBO_F32, vals, 1, grads, D, S, 0, 1, scratch, &ev);
  eval->kind = ev.kind; eval->iter = ev.iter; eval->alpha = ev.alpha; eval->value = ev.value;
  memcpy(x_next, v.xt, sizeof(double) * D);
  if (x_iter) memcpy(x_iter, v.x, sizeof(double) * D);
  *status = (int32_t)state[HBO_ACQ_OPT_S_STATUS];
  return HBO_OK;
}
