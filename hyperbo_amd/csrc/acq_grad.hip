// d acquisition / d x_query over a cache, what jaxopt's L-BFGS-B differentiates in bayesopt() (bayesopt.py:116-125): hbo_acq_grad for
// one model and any cache (the launches: post.hip, trisolve.hip, mlp.hip, kumar.hip), and hbo_acq_grad_samples for S parameter samples
// of one model family over finished caches: of n <= 128 as one launch (acq_small.hip), and hbo_acq_grad_samples_blocked for any n
// (acq_blocked.hip: four launches per chunk of queries).  Host code only.
#include "api_internal.h"

extern "C" int hbo_acq_grad(hbo_ctx* c, const hbo_model* m, hbo_cache* k, const void* xq, int64_t M, int acq_id,
                            double param, double add_noise, double scale, void* acq_out, double* grad_out) {
  if (!c || !xq || !acq_out || !grad_out || !m) return fail(c, HBO_ERR_ARG, "hbo_acq_grad: null argument");
  if (acq_id < 0 || acq_id > HBO_ACQ_UCB) return fail(c, HBO_ERR_ARG, "hbo_acq_grad: bad acq_id");
  if (M <= 0) return HBO_OK;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = validate_model(c, m);
  if (rc) return rc;
  rc = upload_model(c, m);
  if (rc) return rc;
  const int dtype = m->dtype;
  if (k && (k->dtype != dtype || k->D != m->input_dim)) return fail(c, HBO_ERR_ARG, "hbo_acq_grad: cache/model mismatch");
  if (k && k->input_warp != m->input_warp) return fail(c, HBO_ERR_ARG, "hbo_acq_grad: the cache was factorised with another input warp");
  const bool kumar = is_kumar(m);
  const size_t es = esize(dtype);
  hipStream_t st = c->stream;
  const int D = m->input_dim, fdim = feature_dim(m);
  const bool mlp = needs_mlp(m);
  const MlpShape sh = mlp_shape(m);
  const int L = sh.L, flast = mlp ? m->features[L - 1] : 0;
  TaskHost* t = (k && k->t->n > 0) ? k->t : nullptr;
  const int64_t CH = 1024;   // queries per pass: three [CH][npad] panels of workspace
  const int64_t mc_max = std::min<int64_t>(M, CH);
  int maxf = D;
  size_t nparam = 1;
  for (int l = 0; l < L; ++l) { maxf = std::max(maxf, sh.fout[l]); nparam = std::max(nparam, (size_t)(sh.fin[l] + 1) * sh.fout[l]); }
  void* d_xq = ws_get(c, WS_XQ, (size_t)mc_max * D * es);
  void* d_mu0 = ws_get(c, WS_MU0, (size_t)mc_max * es);
  void* d_kd = ws_get(c, WS_KD, (size_t)mc_max * es);
  void* d_acq = ws_get(c, WS_ACQ, (size_t)mc_max * es);
  double* d_gf = (double*)ws_get(c, WS_AG_GF, (size_t)mc_max * fdim * sizeof(double));
  double* d_dmu = (double*)ws_get(c, WS_AG_DMU, (size_t)mc_max * sizeof(double));
  double* d_gx = (double*)ws_get(c, WS_AG_GX, (size_t)mc_max * D * sizeof(double));
  double* d_t0 = (double*)ws_get(c, WS_AG_T0, (size_t)mc_max * maxf * sizeof(double));
  double* d_t1 = (double*)ws_get(c, WS_AG_T1, (size_t)mc_max * maxf * sizeof(double));
  double* d_dw = (double*)ws_get(c, WS_AG_DW, nparam * sizeof(double));   // weight-gradient sink of the shared MLP backward
  if (!d_xq || !d_mu0 || !d_kd || !d_acq || !d_gf || !d_dmu || !d_gx || !d_t0 || !d_t1 || !d_dw) return HBO_ERR_HIP;
  void* d_kwq = kumar ? ws_get(c, WS_KW_Q, (size_t)mc_max * D * es) : nullptr;
  if (kumar && !d_kwq) return HBO_ERR_HIP;
  void *d_K = nullptr, *d_L = nullptr, *d_B = nullptr;
  if (t) {
    d_K = ws_get(c, WS_AG_K, (size_t)mc_max * t->npad * es); d_L = ws_get(c, WS_AG_L, (size_t)mc_max * t->npad * es);
    d_B = ws_get(c, WS_AG_B, (size_t)mc_max * t->npad * es);
    if (!d_K || !d_L || !d_B) return HBO_ERR_HIP;
  }
  void* fq_acts[HBO_MAX_MLP_LAYERS] = {nullptr};
  if (mlp) for (int l = 0; l < L; ++l) { fq_acts[l] = ws_get(c, WS_FQ0 + l, (size_t)mc_max * m->features[l] * es); if (!fq_acts[l]) return HBO_ERR_HIP; }
  const bool bad = k && k->info != INT_MAX;
  for (int64_t q0 = 0; q0 < M; q0 += CH) {
    const int64_t mc = std::min<int64_t>(CH, M - q0);
    HIPCHK(c, hipMemcpyAsync(d_xq, (const char*)xq + (size_t)q0 * D * es, (size_t)mc * D * es, hipMemcpyHostToDevice, st));
    const void* Fq = query_features(c, m, c->d_model, c->d_mlp_w, c->d_mlp_b, d_xq, mc, fq_acts, d_kwq, d_mu0, d_kd, st).Fq;
    if (t) {
      HIPCHK(c, hipMemsetAsync(d_K, 0, (size_t)mc * t->npad * es, st));
      GramArgs g = {}; g.kernel_id = c->h_model->kernel_id; g.mfma_min_f = c->opt_gram_mfma; g.x1 = Fq; g.x2 = k->h_desc.F; g.out = d_K; g.n1 = mc; g.n2 = t->n; g.ldo = t->npad; g.fdim = fdim;
      launch_gram(dtype, g, c->d_model, dim3((unsigned)((t->n + 127) / 128), (unsigned)((mc + 127) / 128), 1), st);
      launch_tri_matvec(dtype, t->W, t->ld, t->npad, d_K, t->npad, (int)mc, 0, d_L, t->npad, st);
      launch_tri_matvec(dtype, t->W, t->ld, t->npad, d_L, t->npad, (int)mc, 1, d_B, t->npad, st);
    }
    AcqGradArgs a = {};
    a.Fq = Fq; a.F = t ? k->h_desc.F : nullptr; a.fdim = fdim; a.n = t ? t->n : 0; a.npad = t ? t->npad : 0;
    a.Kq = d_K; a.L = d_L; a.B = d_B; a.alpha = t ? t->svec : nullptr; a.kdiag = d_kd; a.muq = d_mu0;
    a.acq_id = acq_id; a.param = param; a.add_noise = add_noise; a.scale = scale;
    a.acq_out = d_acq; a.gfeat = d_gf; a.dmu = d_dmu; a.M = mc;
    launch_acq_grad(dtype, a, c->d_model, st);
    // assemble d/dx: kernel part (direct or through the MLP) + mean part (mean.py:62-79)
    double* gmlp = nullptr;   // gradient w.r.t. the MLP output
    if (m->kernel_uses_mlp) {
      gmlp = d_gf;
      if (m->mean_id == HBO_MEAN_LINEAR_MLP) launch_acq_grad_mean(d_dmu, c->d_model, mc, flast, gmlp, 1, st);
      HIPCHK(c, hipMemsetAsync(d_gx, 0, (size_t)mc * D * sizeof(double), st));
      if (m->mean_id == HBO_MEAN_LINEAR) launch_acq_grad_mean(d_dmu, c->d_model, mc, D, d_gx, 1, st);
    } else {
      if (kumar) launch_kumar_chain_dx(dtype, d_xq, mc, D, c->d_model, d_gf, d_gx, st);   // d acq / d w(x) * dw/dx
      else HIPCHK(c, hipMemcpyAsync(d_gx, d_gf, (size_t)mc * D * sizeof(double), hipMemcpyDeviceToDevice, st));
      if (m->mean_id == HBO_MEAN_LINEAR) launch_acq_grad_mean(d_dmu, c->d_model, mc, D, d_gx, 1, st);
      if (m->mean_id == HBO_MEAN_LINEAR_MLP) { gmlp = d_t0; launch_acq_grad_mean(d_dmu, c->d_model, mc, flast, gmlp, 0, st); }
    }
    if (gmlp) {
      double* cur = gmlp; double* other = (gmlp == d_t0) ? d_t1 : d_t0;
      for (int l = L - 1; l >= 0; --l) {
        const int fin = sh.fin[l];
        const void* in = l ? fq_acts[l - 1] : d_xq;
        launch_dense_bwd(dtype, in, fq_acts[l], c->d_mlp_w[l], cur, other, d_dw, d_dw + (size_t)fin * sh.fout[l], mc, fin, sh.fout[l], st);
        cur = other; other = (cur == d_t0) ? d_t1 : d_t0;
      }
      launch_add_inplace(d_gx, cur, mc * D, st);
    }
    HIPCHK(c, hipMemcpyAsync((char*)acq_out + (size_t)q0 * es, d_acq, (size_t)mc * es, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(grad_out + (size_t)q0 * D, d_gx, (size_t)mc * D * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
  }
  HIPCHK(c, hipGetLastError());
  if (bad) {
    fill_nan(acq_out, (size_t)M, dtype);
    for (int64_t i = 0; i < M * D; ++i) grad_out[i] = NAN;
    return HBO_NOT_PD;
  }
  return HBO_OK;
}

// ---- the same for S parameter samples of one model family over their FINISHED caches: one upload, the launches, one copy back, one
//      wait -- whatever S is.  Row s = hbo_acq_grad of sample s up to the order of summation.  The prior branch, MLP bases and
//      input-warped models stay with hbo_acq_grad (HBO_ERR_UNSUPPORTED here, before any device work).
//      Every cache of n <= 128 (and no force_blocked): ONE launch (acq_small.hip: a workgroup per (sample, query) pair).  Otherwise every
//      sample takes the four launches of acq_blocked.hip, the queries in chunks whose workspace ([S][chunk][ldv] doubles, three times)
//      stays under ACQ_BLOCKED_WS_BYTES; a row's bits do not depend on the chunking.
//      val64_out (nullable, [S][M]): the values before they are rounded to the model dtype (include/hbo_tune.h:
//      hbo_probe_acq_grad_samples64); without it the call is hbo_acq_grad_samples, to the byte of every buffer.
namespace {
constexpr size_t ACQ_BLOCKED_WS_BYTES = (size_t)256 << 20;
constexpr int64_t ACQ_BLOCKED_MAX_CHUNK = 65535;   // grid.y of the first launch
}  // namespace
// (api_internal.h: AcqRoute, AcqWhat.  The MES step -- hbo_mes_grad_samples, mes.hip: the S x K maxima ride up behind the per-feature
//  values.  The LogEI step -- hbo_logei_grad_samples, logei.hip: the S targets ride in the records where the registry's parameters do)
int acq_grad_samples(hbo_ctx* c, const AcqRoute& route, const AcqWhat& what, const hbo_model* models, int32_t S, hbo_cache* const* caches,
                     const void* xq, int64_t M, const double* add_noise, double scale, void* acq_out, double* grad_out, double* val64_out) {
  const std::string fn = std::string(route.fn) + ": ";
  if (!models || !caches || !xq || !what.given() || !add_noise || !acq_out || !grad_out) return fail(c, HBO_ERR_ARG, fn + "null argument");
  if (S <= 0 || S > 4096) return fail(c, HBO_ERR_ARG, fn + "1 <= S <= 4096");
  if (int rc = acq_what_check(c, fn, what, S)) return rc;
  if (!c) return fail(c, HBO_ERR_ARG, fn + "ctx is null");
  if (M < 0) return fail(c, HBO_ERR_ARG, fn + "M < 0");
  const hbo_model* m0 = &models[0];
  const bool mes = what.step == ACQ_STEP_MES;
  bool any_bad = false;
  if (int rc = acq_samples_check(c, fn, models, S, caches, route.max_n, &any_bad, route.allow_mlp)) return rc;
  if (M == 0) return HBO_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const int dtype = m0->dtype, D = m0->input_dim;
  const size_t es = esize(dtype);
  hipStream_t st = c->stream;
  const int ldv = acq_blocked_ldv(S, caches);
  const bool blocked = route.force_blocked || ldv > HBO_TILE;
  // one block up: [S records][S x 2 D doubles + (MES) S x K maxima][M x D queries][(MLP basis) the S weight sets and their address
  // tables]; one block down: [S x M x D doubles][S x M values]
  const AcqVecWidths vw = acq_vec_widths(m0);   // (without an MLP: D and D)
  const AcqMlpPack mlp = acq_mlp_layout(m0, S);
  const size_t hv_b = sizeof(double) * ((size_t)vw.fdim + vw.mdim) * S, ys_b = mes ? sizeof(double) * (size_t)S * what.K : 0;
  const size_t smp_b = align256(sizeof(AcqSmallSample) * S), vec_b = align256(hv_b + ys_b);
  const size_t xq_b = mlp.bytes ? align256((size_t)M * D * es) + mlp.bytes : (size_t)M * D * es, o_mlp = smp_b + vec_b + align256((size_t)M * D * es);
  const size_t grad_b = align256(sizeof(double) * (size_t)S * M * D), acq_b = (size_t)S * M * es;
  const size_t v64_o = align256(grad_b + acq_b), v64_b = val64_out ? sizeof(double) * (size_t)S * M : 0;
  const size_t in_b = smp_b + vec_b + xq_b, out_b = val64_out ? v64_o + v64_b : grad_b + acq_b;
  char* d_in = static_cast<char*>(ws_get(c, WS_AF_IN, in_b));
  char* d_out = static_cast<char*>(ws_get(c, WS_AF_OUT, out_b));
  if (!d_in || !d_out) return HBO_ERR_HIP;
  int64_t chunk = 0;
  double* d_work = nullptr;
  if (blocked) {
    const size_t per_query = sizeof(double) * (size_t)S * (3 * (size_t)ldv + mlp.ftot);   // k, l, beta and (MLP basis) the activations
    chunk = route.chunk_queries > 0 ? route.chunk_queries : std::max<int64_t>(1, (int64_t)(ACQ_BLOCKED_WS_BYTES / per_query));
    chunk = std::min(std::min(chunk, M), ACQ_BLOCKED_MAX_CHUNK);
    d_work = static_cast<double*>(ws_get(c, WS_AB_WORK, per_query * (size_t)chunk));
    if (!d_work) return HBO_ERR_HIP;
  }
  char* stage = static_cast<char*>(stage_begin(c, fn.c_str(), align256(in_b) + out_b));
  if (!stage) return HBO_ERR_HIP;
  char* stage_out = stage + align256(in_b);
  AcqSmallSample* hs = reinterpret_cast<AcqSmallSample*>(stage);
  double* hv = reinterpret_cast<double*>(stage + smp_b);
  acq_small_pack(hs, hv, models, S, caches, what.params, add_noise);
  if (mes) memcpy(stage + smp_b + hv_b, what.ystar, ys_b);
  memcpy(stage + smp_b + vec_b, xq, (size_t)M * D * es);
  AcqSmallArgs a = {};
  acq_mlp_fill(mlp, stage + o_mlp, d_in + o_mlp, models, S, a);
  HIPCHK(c, stage_upload(c, d_in, stage, in_b, st));
  a.smp = reinterpret_cast<const AcqSmallSample*>(d_in); a.vec = reinterpret_cast<const double*>(d_in + smp_b); a.xq = d_in + smp_b + vec_b;
  a.D = D; a.M = M; a.kernel_id = m0->kernel_id; a.mean_id = m0->mean_id; a.step = what.step; a.acq_id = what.acq_id; a.scale = scale;
  a.grad_out = reinterpret_cast<double*>(d_out); a.acq_out = d_out + grad_b;
  if (val64_out) a.val64_out = reinterpret_cast<double*>(d_out + v64_o);
  if (mes) { a.ystar = reinterpret_cast<const double*>(d_in + smp_b + hv_b); a.K = what.K; }
  if (!blocked) launch_acq_small(dtype, a, S, st);
  else {
    AcqBlockedArgs b = {};
    b.a = a; b.ldv = ldv;
    const size_t plane = (size_t)S * chunk * ldv;
    b.k = d_work; b.l = d_work + plane; b.beta = d_work + 2 * plane;
    b.acts = d_work + 3 * plane; b.ftot = mlp.ftot;
    for (int64_t q0 = 0; q0 < M; q0 += chunk) {   // (stream order: a chunk's launches run after the ones before it have read the workspace)
      b.q0 = q0; b.mc = std::min(chunk, M - q0);
      launch_acq_blocked(dtype, b, S, st);
    }
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(stage_out, d_out, out_b, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  memcpy(grad_out, stage_out, sizeof(double) * (size_t)S * M * D);
  memcpy(acq_out, stage_out + grad_b, acq_b);
  if (val64_out) memcpy(val64_out, stage_out + v64_o, v64_b);
  return any_bad ? HBO_NOT_PD : HBO_OK;
}
extern "C" int hbo_acq_grad_samples(hbo_ctx* c, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq, int64_t M,
                                    int acq_id, const double* params, const double* add_noise, double scale, void* acq_out,
                                    double* grad_out) {
  return acq_grad_samples(c, ACQ_ROUTE_SMALL.named("hbo_acq_grad_samples"), acq_what_registry(acq_id, params), models, S, caches, xq, M, add_noise,
                          scale, acq_out, grad_out, nullptr);
}
extern "C" int hbo_acq_grad_samples_blocked(hbo_ctx* c, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq,
                                            int64_t M, int acq_id, const double* params, const double* add_noise, double scale,
                                            void* acq_out, double* grad_out) {
  return acq_grad_samples(c, ACQ_ROUTE_BLOCKED.named("hbo_acq_grad_samples_blocked"), acq_what_registry(acq_id, params), models, S, caches, xq, M,
                          add_noise, scale, acq_out, grad_out, nullptr);
}
// include/hbo_tune.h (TEST HOOK): hbo_acq_grad_samples with the fp64 values hbo_acq_maximize's control kernel reads
extern "C" int hbo_probe_acq_grad_samples64(hbo_ctx* c, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq, int64_t M,
                                            int acq_id, const double* params, const double* add_noise, double scale, void* acq_out,
                                            double* grad_out, double* val64_out) {
  if (int rc = acq_probe_check(c, "hbo_probe_acq_grad_samples64", val64_out, 0)) return rc;
  return acq_grad_samples(c, ACQ_ROUTE_SMALL.named("hbo_acq_grad_samples"), acq_what_registry(acq_id, params), models, S, caches, xq, M, add_noise,
                          scale, acq_out, grad_out, val64_out);
}
// include/hbo_tune.h (TEST HOOK): hbo_acq_grad_samples_blocked with those values, the blocked kernels on request and a chunk size
extern "C" int hbo_probe_acq_grad_samples_blocked64(hbo_ctx* c, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq,
                                                    int64_t M, int acq_id, const double* params, const double* add_noise, double scale,
                                                    void* acq_out, double* grad_out, int32_t force_blocked, int64_t chunk_queries,
                                                    double* val64_out) {
  if (int rc = acq_probe_check(c, "hbo_probe_acq_grad_samples_blocked64", val64_out, chunk_queries)) return rc;
  return acq_grad_samples(c, ACQ_ROUTE_BLOCKED.probed("hbo_acq_grad_samples_blocked", force_blocked, chunk_queries), acq_what_registry(acq_id, params),
                          models, S, caches, xq, M, add_noise, scale, acq_out, grad_out, val64_out);
}
// ---- the same with MLP-basis kernels and linear_mlp means served (acq_mlp.h): the pair's workgroup runs the forward and backward pass
//      itself (n <= 128: still ONE launch; otherwise a forward launch in front of the four: five per chunk).  The S weight sets ride up
//      in the call's one staged upload.  A family without any MLP takes hbo_acq_grad_samples_blocked's launches over the same bytes.
extern "C" int hbo_acq_grad_samples_mlp(hbo_ctx* c, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq, int64_t M,
                                        int acq_id, const double* params, const double* add_noise, double scale, void* acq_out,
                                        double* grad_out) {
  return acq_grad_samples(c, ACQ_ROUTE_MLP.named("hbo_acq_grad_samples_mlp"), acq_what_registry(acq_id, params), models, S, caches, xq, M, add_noise,
                          scale, acq_out, grad_out, nullptr);
}
// include/hbo_tune.h (TEST HOOK): hbo_acq_grad_samples_mlp with the fp64 values, the blocked kernels on request and a chunk size
extern "C" int hbo_probe_acq_grad_samples_mlp64(hbo_ctx* c, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq,
                                                int64_t M, int acq_id, const double* params, const double* add_noise, double scale,
                                                void* acq_out, double* grad_out, int32_t force_blocked, int64_t chunk_queries,
                                                double* val64_out) {
  if (int rc = acq_probe_check(c, "hbo_probe_acq_grad_samples_mlp64", val64_out, chunk_queries)) return rc;
  return acq_grad_samples(c, ACQ_ROUTE_MLP.probed("hbo_acq_grad_samples_mlp", force_blocked, chunk_queries), acq_what_registry(acq_id, params), models,
                          S, caches, xq, M, add_noise, scale, acq_out, grad_out, val64_out);
}
