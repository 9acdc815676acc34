// GPCache side of the C ABI: hbo_factor (hyperbo/basics/linalg.py:72-110 behind gp.py:540-560), the O(N^2) row append, the
// posterior behind hbo_predict (gp.py:242-305) and hbo_acq (acfun.py:36-142), hbo_acq_samples, the batch form of factor plus
// posterior, and hbo_cache_export / hbo_cache_free.  (The acquisition gradient over a cache: acq_grad.hip; the simulated BO loop: bo_loop.hip.)
#include "api_internal.h"

// ---- one cache builder and one factor pipeline (hbo_factor: one cache; hbo_acq_samples: S of them as one batch) --------------------
// y (n x m, host) as y^T (m x n), so that aug row a = column a of y
static std::vector<unsigned char> transpose_y(const void* y, int64_t n, int mcols, size_t es) {
  std::vector<unsigned char> yt((size_t)n * mcols * es);
  cols_to_rows(yt.data(), y, n, mcols, n, es);
  return yt;
}
// A cache over n observations and m target columns with everything a factorisation and its readers need allocated, and its descriptor
// filled on the host: nothing is uploaded or computed (the callers' uploads differ: from the host / from the first sample's cache).
static int cache_alloc(hbo_ctx* c, const hbo_model* m, int64_t n, int mcols, hbo_cache** out) {
  const int dtype = m->dtype;
  const size_t es = esize(dtype);
  hbo_cache* k = new hbo_cache();
  k->dtype = dtype; k->D = m->input_dim; k->m = mcols; k->input_warp = m->input_warp;
  TaskHost* t = k->t = new TaskHost();
  task_shape(t, n, mcols, dtype);
  auto bail = [&](int code) { hbo_cache_free(c, k); return code; };
  HIPCHK_OR(c, dev_alloc(c, &t->X, (size_t)t->npad * m->input_dim * es), bail(0));   // capacity npad rows (row appends)
  HIPCHK_OR(c, dev_alloc(c, &t->ysum, (size_t)n * mcols * es), bail(0));
  int rc = ensure_task_workspace(c, dtype, t, true, mcols);
  if (rc) return bail(rc);
  if (needs_mlp(m)) { rc = t->feat.ensure(c, m, t->npad); if (rc) return bail(rc); }
  if (is_kumar(m)) { rc = ensure_kumar_buffers(c, m, t, t->npad, false); if (rc) return bail(rc); }   // capacity npad rows (row appends)
  fill_desc(k->h_desc, t, m, dtype, ROLE_FACTOR);
  HIPCHK_OR(c, hbo_malloc(c, (void**)&k->d_desc, sizeof(TaskDesc)), bail(0));
  HIPCHK_OR(c, hbo_malloc(c, (void**)&k->d_info, sizeof(int)), bail(0));
  HIPCHK_OR(c, hbo_malloc(c, &k->resid, (size_t)mcols * t->npad * es), bail(0));
  HIPCHK_OR(c, hbo_malloc(c, &k->zvec, (size_t)mcols * t->npad * es), bail(0));
  *out = k;
  return HBO_OK;
}

// S caches of one shape over one model family (their inputs and descriptors uploaded), factorised as one batch
struct FactorBatch {
  const hbo_model* models; int S;                // host models; models[0] shapes every launch
  hbo_cache* const* ks;
  const TaskDesc* d_batch; int* d_infos;         // device: the S descriptors; the S info words, INT_MAX
  const ModelDev* d_models; int model_stride;    // device models: task s reads d_models[s * model_stride] (0: one model for the batch)
  void* const* w_dev; void* const* b_dev;        // device MLP weights, [S][HBO_MAX_MLP_LAYERS] (null: the context's last upload)
  bool keep_rows;                                // every cache keeps resid = y - mu and zvec = L^-1 (y - mu): what a row append reads
};
// The one pipeline behind them, enqueued on the main stream and not waited for: poison -> features (per cache, with its own weights) ->
// residual rows -> Gram -> factorisation -> inverse -> alpha = K^-1 (y - mu) per column
static int enqueue_factor(hbo_ctx* c, const FactorBatch& fb) {
  const hbo_model* m0 = fb.models;
  const int dtype = m0->dtype, S = fb.S;
  const size_t es = esize(dtype);
  const TaskHost* t0 = fb.ks[0]->t;
  const int npad = t0->npad, nblk = t0->nblk, mcols = t0->m;
  hipStream_t st = c->stream;
  // the augmented rows of A (below its npad rows), as they stand, into each cache's resid or zvec
  auto keep_aug = [&](bool z) -> hipError_t {
    for (int s = 0; s < S; ++s) {
      hbo_cache* k = fb.ks[s]; const TaskHost* t = k->t;
      hipError_t e = hipMemcpy2DAsync(z ? k->zvec : k->resid, (size_t)npad * es, (char*)t->A + (size_t)npad * t->ld * es, (size_t)t->ld * es,
                                      (size_t)npad * es, mcols, hipMemcpyDeviceToDevice, st);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  };
  if (c->opt_poison) launch_poison(dtype, fb.d_batch, S, npad, st);
  { ProfScope ps(c, "features", 1);
    for (int s = 0; s < S; ++s) {
      TaskHost* t = fb.ks[s]->t;
      if (needs_mlp(m0)) run_mlp(c, m0, t->X, t->n, t->feat.acts.data(), fb.w_dev ? fb.w_dev + (size_t)s * HBO_MAX_MLP_LAYERS : nullptr,
                                 fb.b_dev ? fb.b_dev + (size_t)s * HBO_MAX_MLP_LAYERS : nullptr);
      if (is_kumar(m0)) launch_kumar_forward(dtype, nullptr, 0, 0, t->X, t->KW, nullptr, t->n, m0->input_dim, fb.d_models + (size_t)s * fb.model_stride, st);
    }
    launch_aug_rows(dtype, fb.d_batch, S, npad, fb.d_models, st, fb.model_stride); }
  if (fb.keep_rows) HIPCHK(c, keep_aug(false));
  { ProfScope ps(c, "gram", 1);
    GramArgs g = {}; g.kernel_id = m0->kernel_id; g.mfma_min_f = c->opt_gram_mfma; g.tasks = fb.d_batch; g.fdim = feature_dim(m0); g.symmetric = 1; g.padded = 1;
    g.model_stride = fb.model_stride;
    launch_gram(dtype, g, fb.d_models, dim3(nblk, nblk, S), st); }
  // the inverse W = L^-1 (kept for the posterior products) starts beside the panel chain, as in the objective path
  InvRun inv = inv_run(c, dtype, fb.d_batch, S, nblk, S == 1 ? &fb.ks[0]->h_desc : nullptr, INV_W);
  CholBoundScope bound_scope(c, chol_diag_bound_of(fb.models, S));
  { ProfScope ps(c, "potrf", 1); run_potrf(c, dtype, fb.d_batch, S, nblk, fb.d_infos, &inv); }
  if (fb.keep_rows) HIPCHK(c, keep_aug(true));
  { ProfScope ps(c, "trtri", 1); run_trtri(inv); }
  { ProfScope ps(c, "wt_z", 1);
    for (int a = 0; a < mcols; ++a) launch_wt_z(dtype, fb.d_batch, S, nblk, a, a, npad, st); }
  return HBO_OK;
}

extern "C" int hbo_factor(hbo_ctx* c, const hbo_model* m, const void* x, int64_t n, const void* y, int32_t mcols,
                          hbo_cache** out) {
  if (!c || !out || !x || !y) return fail(c, HBO_ERR_ARG, "hbo_factor: null argument");
  if (n <= 0 || mcols <= 0 || mcols > HBO_TILE) return fail(c, HBO_ERR_ARG, "hbo_factor: need n>0 and 1<=m<=128");
  HIPCHK(c, hipSetDevice(c->device));
  prof_begin(c);
  int rc = upload_model(c, m);
  if (rc) return rc;
  const size_t es = esize(m->dtype);
  hipStream_t st = c->stream;
  hbo_cache* k = nullptr;
  rc = cache_alloc(c, m, n, mcols, &k);
  if (rc) return rc;
  auto bail = [&](int code) { hbo_cache_free(c, k); return code; };
  const std::vector<unsigned char> yt = transpose_y(y, n, mcols, es);
  int inf = INT_MAX;
  HIPCHK_OR(c, hipMemcpy(k->t->X, x, (size_t)n * m->input_dim * es, hipMemcpyHostToDevice), bail(0));
  HIPCHK_OR(c, hipMemcpy(k->t->ysum, yt.data(), (size_t)n * mcols * es, hipMemcpyHostToDevice), bail(0));
  HIPCHK_OR(c, hipMemcpy(k->d_desc, &k->h_desc, sizeof(TaskDesc), hipMemcpyHostToDevice), bail(0));
  HIPCHK_OR(c, hipMemcpy(k->d_info, &inf, sizeof(int), hipMemcpyHostToDevice), bail(0));
  FactorBatch fb = {m, 1, &k, k->d_desc, k->d_info, c->d_model, 0, nullptr, nullptr, true};
  rc = enqueue_factor(c, fb);
  if (rc) return bail(rc);
  HIPCHK_OR(c, hipMemcpyAsync(&k->info, k->d_info, sizeof(int), hipMemcpyDeviceToHost, st), bail(0));
  HIPCHK_OR(c, hipStreamSynchronize(st), bail(0));
  HIPCHK_OR(c, hipGetLastError(), bail(0));
  prof_collect(c);
  *out = k;
  return k->info != INT_MAX ? HBO_NOT_PD : HBO_OK;
}

extern "C" int hbo_cache_free(hbo_ctx* c, hbo_cache* k) {
  if (!k) return HBO_OK;
  if (c) hipSetDevice(c->device);
  free_task(c, k->t);
  for (void* p : {(void*)k->d_desc, (void*)k->d_info, k->resid, k->zvec, (void*)k->w3, (void*)k->d_wmax}) if (p) hipFree(p);
  delete k;
  return HBO_OK;
}

extern "C" int hbo_cache_export(hbo_ctx* c, hbo_cache* k, void* chol_out, void* kinvy_out, void* ymu_out) {
  if (!c || !k) return fail(c, HBO_ERR_ARG, "hbo_cache_export: null argument");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t es = esize(k->dtype);
  TaskHost* t = k->t;
  const int64_t n = t->n;
  const bool bad = k->info != INT_MAX;
  if (chol_out) {
    if (bad) fill_nan(chol_out, (size_t)n * n, k->dtype);
    else {
      DevBuf buf;
      void* tmp = nullptr;
      HIPCHK(c, buf.get(c, &tmp, (size_t)n * n * es));
      launch_extract_lower(k->dtype, t->A, t->ld, n, tmp, c->stream);
      HIPCHK(c, hipMemcpyAsync(chol_out, tmp, (size_t)n * n * es, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
  }
  std::vector<unsigned char> buf((size_t)k->m * t->npad * es);
  auto export_cols = [&](const void* dev, void* outp, bool nanfill) -> int {
    if (nanfill) { fill_nan(outp, (size_t)n * k->m, k->dtype); return HBO_OK; }
    HIPCHK(c, hipMemcpy(buf.data(), dev, buf.size(), hipMemcpyDeviceToHost));
    rows_to_cols(outp, buf.data(), n, k->m, t->npad, es);
    return HBO_OK;
  };
  if (kinvy_out) { int rc = export_cols(t->svec, kinvy_out, bad); if (rc) return rc; }
  if (ymu_out) { int rc = export_cols(k->resid, ymu_out, false); if (rc) return rc; }
  return HBO_OK;
}

// O(N^2) row append (the reference re-factorises from scratch after every BO
// observation, hyperbo/bo_utils/bayesopt.py:186-190, and notes "One can potentially support rank-1
// updates", hyperbo/gp_utils/gp.py:284).  For each new point (x*, y*), with W = L^-1 resident:
//   l = W k(X,x*),  d = sqrt(k(x*,x*) + sigma^2 + eps - l.l),  L' = [[L,0],[l^T,d]],
//   W' = [[W,0],[-(l^T W)/d, 1/d]],  z' = [z; (r* - l.z)/d],  alpha' = [alpha + w' z'_n ; z'_n/d].
// Two triangular mat-vecs on the device, O(n) arithmetic on the host.  Returns HBO_ERR_UNSUPPORTED
// when the padded capacity (npad) is exhausted -- the caller then re-factorises.
namespace {
// One new observation joins a cached factorisation (GP.update_sub_dataset(is_append=True) + setup_predictor, gp.py:426-452,540-560),
// entirely on the device: with l = W k(X, x*) and wl = W^T l from the two triangular mat-vecs before it, ONE workgroup
//   d = sqrt(k(x*, x*) + noise + eps - l.l)        (not positive: *fail_at = n + 1, nothing is written)
//   row n of L = [l, d],   row n of W = [-wl / d, 1 / d]
//   per column a of y:  z_a[n] = (y*_a - mu(x*) - l.z_a) / d,   alpha_a += W[n, :] z_a[n],   resid_a[n] = y*_a - mu(x*)
// Sums in fp64 for both dtypes (as the host loop this replaces did).
template <typename T>
__global__ __launch_bounds__(1024) void append_row_kernel(T* L, T* W, int64_t ld, int64_t n, const T* l, const T* wl, const T* mu_new,
                                                          const T* kdiag, double kadd, const T* y_new, int mc, int64_t npad, T* z,
                                                          T* alpha, T* resid, int* fail_at) {
  __shared__ double red[16];
  __shared__ double bc;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  auto block_sum = [&](double v) -> double {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();               // red[] / bc of the previous call are no longer read
    if (lane == 0) red[wave] = v;
    __syncthreads();
    if (tid == 0) { double s = 0; for (int k = 0; k < 16; ++k) s += red[k]; bc = s; }
    __syncthreads();
    return bc;
  };
  if (*fail_at) return;            // an earlier row of this call failed (uniform)
  double s = 0;
  for (int64_t i = tid; i < n; i += 1024) { const double v = (double)l[i]; s += v * v; }
  const double d2 = (double)kdiag[0] + kadd - block_sum(s);
  if (!(d2 > 0)) { if (tid == 0) *fail_at = (int)n + 1; return; }
  const double d = sqrt(d2);
  for (int64_t i = tid; i < n; i += 1024) { L[n * ld + i] = l[i]; W[n * ld + i] = (T)(-(double)wl[i] / d); }
  if (tid == 0) { L[n * ld + n] = (T)d; W[n * ld + n] = (T)(1.0 / d); }
  for (int a = 0; a < mc; ++a) {
    T* za = z + (int64_t)a * npad; T* aa = alpha + (int64_t)a * npad;
    double lz = 0;
    for (int64_t i = tid; i < n; i += 1024) lz += (double)l[i] * (double)za[i];
    lz = block_sum(lz);
    const double r_new = (double)y_new[a] - (double)mu_new[0];
    const double zn = (r_new - lz) / d;
    for (int64_t i = tid; i < n; i += 1024) aa[i] = (T)((double)aa[i] + (-(double)wl[i] / d) * zn);
    if (tid == 0) { za[n] = (T)zn; aa[n] = (T)(zn / d); resid[(int64_t)a * npad + n] = (T)r_new; }
  }
}
}  // namespace

extern "C" int hbo_cache_append(hbo_ctx* c, const hbo_model* m, hbo_cache* k, const void* x_new, int64_t n_new,
                                const void* y_new) {
  if (!c || !k || !x_new || !y_new) return fail(c, HBO_ERR_ARG, "hbo_cache_append: null argument");
  if (n_new <= 0) return HBO_OK;
  HIPCHK(c, hipSetDevice(c->device));
  TaskHost* t = k->t;
  if (k->dtype != m->dtype || k->D != m->input_dim) return fail(c, HBO_ERR_ARG, "hbo_cache_append: cache/model mismatch");
  if (k->input_warp != m->input_warp) return fail(c, HBO_ERR_ARG, "hbo_cache_append: the cache was factorised with another input warp");
  if (k->info != INT_MAX) return HBO_NOT_PD;
  if (t->n + n_new > t->npad) return fail(c, HBO_ERR_UNSUPPORTED, "hbo_cache_append: capacity exhausted (re-factorise)");
  k->w3_valid = false;   // W changes: its bf16 planes are rebuilt at the next posterior call
  int rc = upload_model(c, m);
  if (rc) return rc;
  const int dtype = k->dtype; const size_t es = esize(dtype);
  hipStream_t st = c->stream;
  const int fdim = feature_dim(m), mc = k->m;
  void* d_kx = ws_get(c, WS_AP_KX, (size_t)t->npad * es); void* d_l = ws_get(c, WS_AP_L, (size_t)t->npad * es);
  void* d_w = ws_get(c, WS_AP_W, (size_t)t->npad * es); void* d_mu = ws_get(c, WS_AP_MU, 16); void* d_kd = ws_get(c, WS_AP_KD, 16);
  // per call: the new targets (n_new x m) and the failure word
  unsigned char* d_y = static_cast<unsigned char*>(ws_get(c, WS_AP_Y, (size_t)n_new * mc * es + 16));
  if (!d_kx || !d_l || !d_w || !d_mu || !d_kd || !d_y) return HBO_ERR_HIP;
  int* d_fail = reinterpret_cast<int*>(d_y + (((size_t)n_new * mc * es + 15) & ~(size_t)15));
  HIPCHK(c, hipMemsetAsync(d_fail, 0, sizeof(int), st));
  HIPCHK(c, hipMemcpyAsync(d_y, y_new, (size_t)n_new * mc * es, hipMemcpyHostToDevice, st));
  const int64_t n0 = t->n;
  for (int64_t q = 0; q < n_new; ++q) {
    const int64_t n = n0 + q;
    // new input row -> X[n], features -> acts[.][n]; the cached inputs of a Kumaraswamy model are warped: so is the new row, into KW[n]
    void* xrow = (char*)t->X + (size_t)n * m->input_dim * es;
    HIPCHK(c, hipMemcpyAsync(xrow, (const char*)x_new + (size_t)q * m->input_dim * es, (size_t)m->input_dim * es, hipMemcpyHostToDevice, st));
    void* rows[HBO_MAX_MLP_LAYERS];
    if (needs_mlp(m)) for (int lyr = 0; lyr < m->n_layers; ++lyr) rows[lyr] = (char*)t->feat.acts[lyr] + (size_t)n * m->features[lyr] * es;
    void* wrow = is_kumar(m) ? (char*)t->KW + (size_t)n * m->input_dim * es : nullptr;
    const void* Fq = query_features(c, m, c->d_model, c->d_mlp_w, c->d_mlp_b, xrow, 1, rows, wrow, d_mu, d_kd, st).Fq;
    // k(X, x*)  (n x 1), zero-padded to npad
    HIPCHK(c, hipMemsetAsync(d_kx, 0, (size_t)t->npad * es, st));
    { GramArgs g = {}; g.kernel_id = c->h_model->kernel_id; g.mfma_min_f = c->opt_gram_mfma; g.x1 = k->h_desc.F; g.x2 = Fq; g.out = d_kx; g.n1 = n; g.n2 = 1; g.ldo = 1; g.fdim = fdim;
      launch_gram(dtype, g, c->d_model, dim3(1, (unsigned)((n + 127) / 128), 1), st); }
    // l = W kx ; wl = W^T l ; then the new rows and the updated z, alpha in one workgroup (no host round trip)
    launch_tri_matvec(dtype, t->W, t->ld, t->npad, d_kx, t->npad, 1, 0, d_l, t->npad, st);
    launch_wt_z(dtype, k->d_desc, 1, t->nblk, 0, 0, t->npad, st, d_l, d_w);   // W^T l (two-stage, uses its own scratch)
    const double kadd = m->noise_variance + m->eps;
    if (dtype == HBO_F64)
      hipLaunchKernelGGL(append_row_kernel<double>, dim3(1), dim3(1024), 0, st, (double*)t->A, (double*)t->W, t->ld, n, (const double*)d_l,
                         (const double*)d_w, (const double*)d_mu, (const double*)d_kd, kadd, (const double*)d_y + q * mc, mc, (int64_t)t->npad,
                         (double*)k->zvec, (double*)t->svec, (double*)k->resid, d_fail);
    else
      hipLaunchKernelGGL(append_row_kernel<float>, dim3(1), dim3(1024), 0, st, (float*)t->A, (float*)t->W, t->ld, n, (const float*)d_l,
                         (const float*)d_w, (const float*)d_mu, (const float*)d_kd, kadd, (const float*)d_y + q * mc, mc, (int64_t)t->npad,
                         (float*)k->zvec, (float*)t->svec, (float*)k->resid, d_fail);
  }
  int failed_at = 0;
  HIPCHK(c, hipMemcpyAsync(&failed_at, d_fail, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  int status = HBO_OK;
  if (failed_at) { status = HBO_NOT_PD; k->info = failed_at; t->n = failed_at - 1; }   // the rows before it were appended
  else t->n = n0 + n_new;
  k->h_desc.n = (int)t->n;
  HIPCHK(c, hipMemcpy(k->d_desc, &k->h_desc, sizeof(TaskDesc), hipMemcpyHostToDevice));
  HIPCHK(c, hipGetLastError());
  return status;
}

// ---- the three launches of the fp32 posterior product on the 16-bit matrix cores (post3.hip) -----------------------------------
// Shared by the posterior below and by hbo_probe_post_product (probe.hip), which feeds them caller-chosen operands.
// W [nblk * 128 rows, ld], lower triangular: its split copy w3 (blocks up to each row tile's diagonal block).  h2: two fp16 planes
// by the scale that follows from max |W|, measured first into *d_wmax; else three bf16 planes
void post3_split_w(const float* W, int64_t ld, int nblk, bool h2, unsigned short* w3, unsigned int* d_wmax, hipStream_t st) {
  Split3Block sw = {}; sw.in = W; sw.ld = ld; sw.out = w3; sw.row_tiles = sw.last_rows = nblk;
  sw.nkb = nblk * (HBO_TILE / 16); sw.last_krows = nblk * HBO_TILE; sw.tri = 1;
  if (h2) { (void)hipMemsetAsync(d_wmax, 0, sizeof(unsigned int), st); sw.h2 = 1; sw.max_out = d_wmax; }   // max |W| first, then the split
  launch_split3_block(sw, 1, false, st);
}
// the cross Gram of one chunk, Kxq [npad, ldq] with mpad candidates (columns), transposed on the way: K3 rows = candidates
void post3_split_kxq(const float* K, int64_t ldq, int mpad, int npad, bool h2, float kscale, unsigned short* K3, hipStream_t st) {
  Split3Block sk = {}; sk.in = K; sk.ld = ldq; sk.out = K3; sk.row_tiles = sk.last_rows = mpad / HBO_TILE;
  sk.nkb = npad / 16; sk.last_krows = npad; sk.h2 = h2; sk.scale = kscale;
  launch_split3_block(sk, 1, true, st);
}
// colsq [nblk, ldc] = per row block of W the column sums of (W Kxq)^2.  counter (nullable): zeroed here and handed to launch_post3,
// which turns a large product into a resident grid drawing its tiles from it (returns whether it did)
bool post3_product(const unsigned short* w3, const unsigned short* K3, int nblk, int mpad, bool h2, const unsigned int* d_wmax,
                          float kscale, float* colsq, int64_t ldc, int* counter, hipStream_t st) {
  Post3Args a = {}; a.Wp = w3; a.Kp = K3; a.nkb = nblk * (HBO_TILE / 16); a.h2 = h2; a.wmax_bits = d_wmax; a.kscale = kscale;
  a.colsq = colsq; a.ldc = ldc; a.nblk = nblk;
  if (counter) { a.work_counter = counter; hipMemsetAsync(counter, 0, sizeof(int), st); }
  return launch_post3(a, mpad / HBO_TILE, st);
}


// ---- posterior / acquisition ---------------------------------------------------------------
// posterior() is plan (post_plan, api_internal.h: every decision, from sizes and options) -> workspaces (post_acquire: PostWs, and the
// plan again without a form whose memory the device could not spare) -> steps (ensure_w_split once; per chunk produce_chunk,
// consume_chunk and full_cov_tail, with the event hand-offs between their two streams in the loop).
// `ov` (hbo_acq_samples): the model and its MLP weights are already on the device at ov->md / ov->mlp_w / ov->mlp_b, the queries at
// ov->xq_dev; the acquisition values go to ov->acq_dev and stay there -- nothing is uploaded, copied back or waited for, so that
// the posteriors of many parameter samples queue up behind one another on the stream.
// `lane` > 0 (single-chunk calls only): the pass runs on the context's side stream `lane` with its own set of workspaces, so that
// the latency-bound launch chains of different samples overlap.
struct PosteriorOverride { const ModelDev* md; void* const* mlp_w; void* const* mlp_b; const void* xq_dev; void* acq_dev; int lane; };
// what the steps of one call share
struct PostCall {
  hbo_ctx* c; const hbo_model* m; hbo_cache* k;
  const ModelDev* md; void* const* mw; void* const* mb;   // the model and its MLP weights on the device
  AcqWhat what;                 // the caller's request with `ystar` on the DEVICE (hbo_acq_mes: the K maxima); params is not read here:
  double param;                 // its first entry -- the registry's parameter, hbo_acq_logei's target
  double add_noise, scale;
  PostProbe* probe;             // test hook (hbo_probe_posterior): the chunk's cross Gram, prior variance and prior mean come from here
};
// one chunk's view of the workspaces: its buffer of each per-workspace array, its rows of the M-sized results
struct PostSlice {
  char *xq, *mu0, *kd, *kwq, *K, *colsq, *mupart; unsigned short* K3; void *mu, *var, *acq;
  void* acts[HBO_MAX_MLP_LAYERS];
};
struct PostWs {
  size_t es = 0, row_b = 0;   // bytes of an element, of a query row
  char *xq = nullptr, *mu0 = nullptr, *kd = nullptr, *kwq = nullptr, *K = nullptr, *colsq = nullptr, *mupart = nullptr;
  void *mu = nullptr, *var = nullptr, *acq = nullptr, *V = nullptr, *Kqq = nullptr, *cov = nullptr, *vpart = nullptr;
  unsigned short* K3 = nullptr;
  int* counters = nullptr;    // the context's tile counters (null: every product a plain grid)
  char* fq[HBO_MAX_MLP_LAYERS] = {nullptr};
  size_t vec_b = 0, kwq_b = 0, K_b = 0, colsq_b = 0, k3_b = 0, fq_b[HBO_MAX_MLP_LAYERS] = {0};   // bytes per workspace
  PostSlice at(const PostChunk& ch) const {
    const size_t b = (size_t)ch.b;
    PostSlice s = {};
    s.xq = xq + (size_t)ch.q0 * row_b; s.mu0 = mu0 + b * vec_b; s.kd = kd + b * vec_b; s.kwq = kwq ? kwq + b * kwq_b : nullptr;
    if (K) { s.K = K + b * K_b; s.colsq = colsq + b * colsq_b; s.mupart = mupart + b * colsq_b; }
    s.K3 = K3 ? K3 + b * (k3_b / sizeof(unsigned short)) : nullptr;
    s.mu = (char*)mu + (size_t)ch.q0 * es; s.var = (char*)var + (size_t)ch.q0 * es; s.acq = acq ? (char*)acq + (size_t)ch.q0 * es : nullptr;
    for (int l = 0; l < HBO_MAX_MLP_LAYERS; ++l) s.acts[l] = fq[l] ? fq[l] + b * fq_b[l] : nullptr;
    return s;
  }
};

// Every workspace of the call.  Three of them belong to a form the plan can do without: when the device cannot spare them the plan is made
// again without that form (p changes) -- d_vpart first: the split-operand form is only open to a product that is not split along K.
static int post_acquire(const PostCall& pc, int64_t M, const PosteriorOverride* ov, bool want_acq, PostPlan& p, PostWs& w) {
  hbo_ctx* c = pc.c; const hbo_model* m = pc.m; hbo_cache* k = pc.k;
  const int wso = p.wso, nbuf = p.nbuf;
  auto get = [&](int slot, size_t bytes) { return (char*)ws_get(c, slot + wso, bytes); };
  w.es = esize(p.dtype); w.row_b = (size_t)m->input_dim * w.es;
  const size_t es = w.es;
  w.vec_b = align256((size_t)p.mc_max * es);
  if (ov) w.xq = (char*)const_cast<void*>(ov->xq_dev);
  else if (!(w.xq = (char*)ws_get(c, WS_XQ, (size_t)M * w.row_b))) return HBO_ERR_HIP;
  if (!(w.mu0 = get(WS_MU0, w.vec_b * nbuf)) || !(w.kd = get(WS_KD, w.vec_b * nbuf))) return HBO_ERR_HIP;
  if (!(w.mu = get(WS_MU, (size_t)M * es)) || !(w.var = get(WS_VAR, (size_t)M * es))) return HBO_ERR_HIP;
  if (ov) w.acq = ov->acq_dev;
  else if (want_acq && !(w.acq = get(WS_ACQ, (size_t)M * es))) return HBO_ERR_HIP;
  w.kwq_b = align256((size_t)p.mc_max * w.row_b);   // Kumaraswamy: w(queries) per workspace
  if (is_kumar(m) && !(w.kwq = get(WS_KW_Q, w.kwq_b * nbuf))) return HBO_ERR_HIP;
  if (needs_mlp(m)) for (int l = 0; l < m->n_layers; ++l) {
    w.fq_b[l] = align256((size_t)p.mc_max * m->features[l] * es);
    if (!(w.fq[l] = get(WS_FQ0 + l, w.fq_b[l] * nbuf))) return HBO_ERR_HIP;
  }
  TaskHost* t = k ? k->t : nullptr;
  if (k) {
    w.K_b = align256((size_t)t->npad * p.ldq_max * es); w.colsq_b = align256((size_t)t->nblk * p.ldq_max * es);
    if (!(w.K = get(WS_K, w.K_b * nbuf)) || !(w.colsq = get(WS_COLSQ, w.colsq_b * nbuf)) || !(w.mupart = get(WS_MUPART, w.colsq_b * nbuf))) return HBO_ERR_HIP;
    if (p.full_cov && !(w.V = get(WS_V, (size_t)t->npad * p.ldq_max * es))) return HBO_ERR_HIP;
  }
  // full covariance: Kqq goes into an mpad x ldq buffer (the candidates' padded leading dimension) and V^T V is subtracted in
  // place by a GEMM (gemm.hip: GEMM_VTV); with no cache (prior branch) the M x M Gram is the answer
  if (p.full_cov) {
    if (k && !(w.Kqq = get(WS_KQQ, (size_t)p.mpad_max * p.ldq_max * es))) return HBO_ERR_HIP;
    if (!(w.cov = get(WS_COV, (size_t)M * M * es))) return HBO_ERR_HIP;
  }
  const int* ov_lane = ov ? &ov->lane : nullptr;
  int deny = 0;
  auto replan = [&](int form) { deny |= form; p = post_plan(c, m, M, p.nblk, p.full_cov, ov_lane, deny); };
  if (p.kchunk > 0 && !(w.vpart = get(WS_VPART, (size_t)p.nch * t->npad * p.ldq_max * es))) { c->err.clear(); replan(POST_NO_SPLITK); }
  if (p.form != FORM_MFMA) {
    if (k->w3_valid && k->w3_planes != p.planes) k->w3_valid = false;
    if (!k->w3_valid) {
      // the split copy of W costs 1.5 x its bytes (fp16: 1 x): when the device cannot spare them the fp32-MFMA product takes over
      const size_t elems = (size_t)t->npad * t->npad * p.planes;
      bool ok = true;
      if (p.form == FORM_F16X2 && !k->d_wmax && hbo_malloc(c, (void**)&k->d_wmax, sizeof(unsigned int)) != hipSuccess) { (void)hipGetLastError(); k->d_wmax = nullptr; ok = false; }
      if (ok && (!k->w3 || k->w3_elems != elems)) {
        if (k->w3) hipFree(k->w3);
        k->w3 = nullptr; k->w3_elems = 0;
        if (hbo_malloc(c, (void**)&k->w3, elems * sizeof(unsigned short)) != hipSuccess) { (void)hipGetLastError(); k->w3 = nullptr; ok = false; }
        else k->w3_elems = elems;
      }
      if (!ok) replan(POST_NO_SPLIT3);
    }
  }
  if (p.form != FORM_MFMA) {
    w.k3_b = align256((size_t)p.mpad_max * t->npad * p.planes * sizeof(unsigned short));   // (mpad / 128) x nkb blocks of `planes` x 128 x 16
    if (!(w.K3 = (unsigned short*)get(WS_K3, w.k3_b * nbuf))) { c->err.clear(); replan(POST_NO_SPLIT3); }
  }
  if (p.chunk(0).counter >= 0) w.counters = (int*)ws_get(c, WS_COUNTERS, sizeof(int) * HBO_N_COUNTERS);   // (the first chunk is the largest)
  return HBO_OK;
}

// fp32 split forms: W changes only with the cache, so its split copy is built at the first posterior that wants it (and again after a
// row append, or when the other form is asked for)
static void ensure_w_split(const PostCall& pc, const PostPlan& p) {
  hbo_cache* k = pc.k;
  if (p.form == FORM_MFMA || k->w3_valid) return;
  ProfScope ps(pc.c, "split_w", 1, p.sa);
  post3_split_w(static_cast<const float*>(k->t->W), k->t->ld, k->t->nblk, p.form == FORM_F16X2, k->w3, k->d_wmax, p.sa);
  k->w3_valid = true; k->w3_planes = p.planes;
}

// The acquisition of a chunk from the mean and variance post_epilogue_kernel (or the prior branch) left, for the steps that kernel does
// not take itself: the MES epilogue (mes.hip), the LogEI epilogue (logei.hip).  false: the registry's step, nothing was launched.
static bool step_epilogue(const PostCall& pc, int dtype, const PostChunk& ch, const PostSlice& s, hipStream_t st) {
  switch (pc.what.step) {
    case ACQ_STEP_MES: launch_mes_epilogue(dtype, s.mu, s.var, ch.mc, pc.what.ystar, pc.what.K, pc.add_noise, pc.scale, s.acq, st); return true;
    case ACQ_STEP_LOGEI: launch_logei_epilogue(dtype, s.mu, s.var, ch.mc, pc.param, pc.add_noise, pc.scale, s.acq, st); return true;
    default: return false;
  }
}

// ---- producer side (sb): features, prior mean / variance, then the prior branch's results or the cross Gram into the chunk's workspace ----
static int produce_chunk(const PostCall& pc, const PostPlan& p, const PostWs& w, const PostChunk& ch, const PostSlice& s, const void** Fq_out) {
  hbo_ctx* c = pc.c; const hbo_model* m = pc.m; hbo_cache* k = pc.k;
  const int dtype = p.dtype, fdim = feature_dim(m);
  const size_t es = w.es;
  hipStream_t sb = p.sb;
  if (pc.probe) {   // the caller's columns [q0, q0 + mc) in place of the features and the cross Gram; what follows them stays
    TaskHost* t = k->t;
    const PostProbe& pr = *pc.probe;
    *Fq_out = nullptr;
    HIPCHK(c, hipMemsetAsync(s.K, 0, (size_t)t->npad * ch.ldq * es, sb));
    HIPCHK(c, hipMemcpy2DAsync(s.K, (size_t)ch.ldq * es, (const char*)pr.Kxq + (size_t)ch.q0 * es, (size_t)p.M * es, (size_t)ch.mc * es, (size_t)t->n,
                               hipMemcpyDeviceToDevice, sb));
    HIPCHK(c, hipMemcpyAsync(s.kd, (const char*)pr.kdiag + (size_t)ch.q0 * es, (size_t)ch.mc * es, hipMemcpyDeviceToDevice, sb));
    HIPCHK(c, hipMemcpyAsync(s.mu0, (const char*)pr.mu0 + (size_t)ch.q0 * es, (size_t)ch.mc * es, hipMemcpyDeviceToDevice, sb));
    if (p.form != FORM_MFMA) post3_split_kxq(reinterpret_cast<const float*>(s.K), ch.ldq, ch.mpad, t->npad, p.form == FORM_F16X2, p.kscale, s.K3, sb);
    return HBO_OK;
  }
  const void* Fq = *Fq_out = query_features(c, m, pc.md, pc.mw, pc.mb, s.xq, ch.mc, s.acts, s.kwq, s.mu0, s.kd, sb, true).Fq;
  if (!k) {  // prior branch (gp.py:275-282)
    HIPCHK(c, hipMemcpyAsync(s.mu, s.mu0, (size_t)ch.mc * es, hipMemcpyDeviceToDevice, sb));
    if (p.full_cov) {
      GramArgs g = {}; g.kernel_id = m->kernel_id; g.mfma_min_f = c->opt_gram_mfma; g.x1 = Fq; g.x2 = Fq; g.out = w.cov; g.n1 = ch.mc; g.n2 = ch.mc; g.ldo = ch.mc; g.fdim = fdim;
      launch_gram(dtype, g, pc.md, dim3((unsigned)((ch.mc + 127) / 128), (unsigned)((ch.mc + 127) / 128), 1), sb);
    } else {
      HIPCHK(c, hipMemcpyAsync(s.var, s.kd, (size_t)ch.mc * es, hipMemcpyDeviceToDevice, sb));
    }
    if (s.acq && !step_epilogue(pc, dtype, ch, s, sb)) {   // acquisition on the prior
      PostArgs pa = {}; pa.Kxq = nullptr; pa.n = 0; pa.nblk = 0; pa.ldq = ch.ldq; pa.alpha = nullptr; pa.colsq = nullptr;
      pa.kdiag = s.kd; pa.muq = s.mu0; pa.acq_out = s.acq; pa.M = ch.mc; pa.acq_id = pc.what.acq_id; pa.param = pc.param; pa.add_noise = pc.add_noise; pa.scale = pc.scale;
      launch_post_epilogue(dtype, pa, sb);
    }
    return HBO_OK;
  }
  TaskHost* t = k->t;
  { ProfScope ps(c, "cross_gram", 1, sb);
    GramArgs g = {}; g.kernel_id = m->kernel_id; g.mfma_min_f = c->opt_gram_mfma; g.x1 = k->h_desc.F; g.x2 = Fq; g.out = s.K; g.n1 = t->n; g.n2 = ch.mc; g.ldo = ch.ldq;
    g.n1pad = t->npad; g.n2pad = ch.mpad; g.fdim = fdim; g.symmetric = 0; g.padded = 1;
    g.direct_form = p.direct_form;
    launch_gram(dtype, g, pc.md, dim3(ch.mpad / HBO_TILE, t->nblk, 1), sb); }
  if (p.form != FORM_MFMA) {
    ProfScope ps(c, "split_kxq", 1, sb);
    post3_split_kxq(reinterpret_cast<const float*>(s.K), ch.ldq, ch.mpad, t->npad, p.form == FORM_F16X2, p.kscale, s.K3, sb);
  }
  return HBO_OK;
}

// ---- consumer side (sa): V = L^-1 Kxq on MFMA (column sums of squares), then mean / variance / acquisition ----
static void consume_chunk(const PostCall& pc, const PostPlan& p, const PostWs& w, const PostChunk& ch, const PostSlice& s) {
  hbo_ctx* c = pc.c; hbo_cache* k = pc.k; TaskHost* t = k->t;
  const int dtype = p.dtype;
  hipStream_t sa = p.sa;
  int* counter = (ch.counter >= 0 && w.counters) ? w.counters + ch.counter : nullptr;
  if (p.form != FORM_MFMA) {
    ProfScope ps(c, "post_gemm", 1, sa);
    c->last_post_resident = post3_product(k->w3, s.K3, t->nblk, ch.mpad, p.form == FORM_F16X2, k->d_wmax, p.kscale, reinterpret_cast<float*>(s.colsq), ch.ldq, counter, sa);
  } else {
    ProfScope ps(c, "post_gemm", 1, sa);
    GemmArgs a = {}; a.tasks = k->d_desc; a.mode = GEMM_POST; a.B = s.K; a.ldb = ch.ldq; a.V = p.full_cov ? w.V : nullptr; a.colsq = s.colsq;
    if (p.kchunk > 0) {
      int pairs = 0;
      for (int i = 0; i < t->nblk; ++i) pairs += (i + p.kchunk) / p.kchunk;
      a.kchunk = p.kchunk; a.V = w.vpart; a.colsq = nullptr;
      launch_gemm(dtype, a, dim3(ch.mpad / HBO_TILE, pairs, 1), sa);
      c->last_post_resident = 0;
      launch_post_colsq_split(dtype, w.vpart, t->npad, ch.ldq, ch.mpad, t->nblk, p.kchunk, s.colsq, sa);
    } else {
      if (counter) { a.work_counter = counter; hipMemsetAsync(counter, 0, sizeof(int), sa); a.persistent = 2 * p.n_cus; }
      launch_gemm(dtype, a, dim3(ch.mpad / HBO_TILE, t->nblk, 1), sa);
      c->last_post_resident = a.work_counter && a.persistent > 0;   // (gemm.hip: gemm_plan keeps a one-task GEMM_POST with both resident)
    } }
  if (pc.probe) pc.probe->resident_chunks += c->last_post_resident;
  { ProfScope ps(c, "post_epilogue", 1, sa);
    PostArgs pa = {}; pa.Kxq = s.K; pa.ldq = ch.ldq; pa.npad = t->npad; pa.n = (int)t->n; pa.nblk = t->nblk; pa.alpha = t->svec; pa.colsq = s.colsq; pa.mupart = s.mupart;
    pa.kdiag = s.kd; pa.muq = s.mu0; pa.mu_out = s.mu; pa.var_out = s.var; pa.acq_out = pc.what.step == ACQ_STEP_REGISTRY ? s.acq : nullptr; pa.M = ch.mc;
    pa.acq_id = pc.what.acq_id; pa.param = pc.param; pa.add_noise = pc.add_noise; pa.scale = pc.scale;
    launch_post_epilogue(dtype, pa, sa);
    step_epilogue(pc, dtype, ch, s, sa); }
}

// full covariance with a cache: Kqq - V^T V in the Kqq buffer
static void full_cov_tail(const PostCall& pc, const PostPlan& p, const PostWs& w, const PostChunk& ch, const void* Fq) {
  hbo_ctx* c = pc.c; const hbo_model* m = pc.m;
  ProfScope ps(c, "full_cov", 1, p.sa);
  GramArgs g = {}; g.kernel_id = m->kernel_id; g.mfma_min_f = c->opt_gram_mfma; g.x1 = Fq; g.x2 = Fq; g.out = w.Kqq; g.n1 = ch.mc; g.n2 = ch.mc; g.ldo = ch.ldq; g.fdim = feature_dim(m);
  launch_gram(p.dtype, g, pc.md, dim3((unsigned)((ch.mc + 127) / 128), (unsigned)((ch.mc + 127) / 128), 1), p.sa);
  // (columns of V beyond the candidates are zero: Kxq is zero-padded; the padded part of the Kqq buffer is never copied out)
  GemmArgs a = {}; a.tasks = pc.k->d_desc; a.mode = GEMM_VTV; a.B = w.V; a.ldb = ch.ldq; a.V = w.Kqq;
  launch_gemm(p.dtype, a, dim3(ch.mpad / HBO_TILE, ch.mpad / HBO_TILE, 1), p.sa);
}

int posterior(hbo_ctx* c, const hbo_model* m, hbo_cache* k, const void* xq, int64_t M, int full_cov, void* mu_out, void* var_out,
              void* acq_out, const AcqWhat& what, double add_noise, double scale, const PosteriorOverride* ov, PostProbe* probe) {
  if (!c || !xq) return fail(c, HBO_ERR_ARG, "posterior: null argument");
  if (M <= 0) return HBO_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if (!ov) prof_begin(c);
  int rc = ov ? validate_model(c, m) : upload_model(c, m);
  if (rc) return rc;
  const int dtype = m->dtype;
  if (k && (k->dtype != dtype || k->D != m->input_dim)) return fail(c, HBO_ERR_ARG, "posterior: cache/model mismatch");
  if (k && k->input_warp != m->input_warp) return fail(c, HBO_ERR_ARG, "posterior: the cache was factorised with another input warp");
  const size_t es = esize(dtype);
  double* d_ystar = nullptr;   // hbo_acq_mes: the maxima go up on the consumer stream, ahead of everything that reads them
  const bool mes = what.step == ACQ_STEP_MES;
  if (mes && !(d_ystar = static_cast<double*>(ws_get(c, WS_MES_YSTAR, sizeof(double) * what.K)))) return HBO_ERR_HIP;
  AcqWhat on_dev = what;
  on_dev.ystar = d_ystar;
  const PostCall pc = {c, m, k, ov ? ov->md : c->d_model, ov ? ov->mlp_w : c->d_mlp_w, ov ? ov->mlp_b : c->d_mlp_b, on_dev,
                       what.params ? what.params[0] : 0.0, add_noise, scale, probe};
  PostPlan p = post_plan(c, m, M, k ? k->t->nblk : 0, full_cov != 0, ov ? &ov->lane : nullptr);
  c->last_post_resident = 0;
  if (p.refuse) return fail(c, p.refuse, "posterior: full_cov limited to 65536 queries");
  PostWs w;
  rc = post_acquire(pc, M, ov, acq_out != nullptr, p, w);
  if (rc) return rc;
  if (probe) { probe->plan = p; probe->resident_chunks = 0; }
  hipStream_t sa = p.sa, sb = p.sb;
  const int nbuf = p.nbuf;
  // the queries go up in ONE copy (M x D elements: small beside the N x CH workspace): a pageable host-to-device copy
  // inside the chunk loop waits for the products in flight on the other stream -- it serialised the two streams and
  // took cfg 3 from 142 to 197 ms
  if (!ov) HIPCHK(c, hipMemcpyAsync(w.xq, xq, (size_t)M * w.row_b, hipMemcpyHostToDevice, sa));
  if (mes) HIPCHK(c, hipMemcpyAsync(d_ystar, what.ystar, sizeof(double) * what.K, hipMemcpyHostToDevice, sa));
  if (k) ensure_w_split(pc, p);
  const bool bad = k && k->info != INT_MAX;
  hipEvent_t ev_free[2] = {nullptr, nullptr};
  size_t evi = 0;
  if (nbuf == 2) {   // the side stream starts behind whatever the main stream still holds (model upload)
    hipEvent_t e = pool_event(c, evi++); hipEventRecord(e, sa); hipStreamWaitEvent(sb, e, 0);
  }
  for (int64_t i = 0; i < p.nchunks; ++i) {
    const PostChunk ch = p.chunk(i);
    const PostSlice s = w.at(ch);
    const int b = ch.b;
    if (ev_free[b]) hipStreamWaitEvent(sb, ev_free[b], 0);   // workspace b was read by the products of chunk - 2
    const void* Fq = nullptr;
    rc = produce_chunk(pc, p, w, ch, s, &Fq);
    if (rc) return rc;
    if (k) {
      if (nbuf == 2) { hipEvent_t e = pool_event(c, evi++); hipEventRecord(e, sb); hipStreamWaitEvent(sa, e, 0); }   // the chunk's cross Gram is ready
      consume_chunk(pc, p, w, ch, s);
    }
    if (nbuf == 2) { ev_free[b] = pool_event(c, evi++); hipEventRecord(ev_free[b], k ? sa : sb); }
    if (k && full_cov) full_cov_tail(pc, p, w, ch, Fq);
  }
  if (nbuf == 2) {   // join: everything the side stream produced (the prior branch runs there entirely)
    hipEvent_t e = pool_event(c, evi++); hipEventRecord(e, sb); hipStreamWaitEvent(sa, e, 0);
  }
  if (ov) return (k && k->info != INT_MAX) ? HBO_NOT_PD : HBO_OK;   // (the caller copies back and waits once for all samples)
  if (mu_out) HIPCHK(c, hipMemcpyAsync(mu_out, w.mu, (size_t)M * es, hipMemcpyDeviceToHost, sa));
  if (var_out) {
    // (dense on the device first: a pitched copy to pageable host memory goes row by row)
    if (full_cov && k) HIPCHK(c, hipMemcpy2DAsync(w.cov, (size_t)M * es, w.Kqq, (size_t)p.ldq_max * es, (size_t)M * es, (size_t)M, hipMemcpyDeviceToDevice, sa));
    if (full_cov) HIPCHK(c, hipMemcpyAsync(var_out, w.cov, (size_t)M * M * es, hipMemcpyDeviceToHost, sa));
    else HIPCHK(c, hipMemcpyAsync(var_out, w.var, (size_t)M * es, hipMemcpyDeviceToHost, sa));
  }
  if (acq_out) HIPCHK(c, hipMemcpyAsync(acq_out, w.acq, (size_t)M * es, hipMemcpyDeviceToHost, sa));
  HIPCHK(c, hipStreamSynchronize(sa));
  if (nbuf == 2) HIPCHK(c, hipStreamSynchronize(sb));
  HIPCHK(c, hipGetLastError());
  prof_collect(c);
  if (bad) {
    if (mu_out) fill_nan(mu_out, (size_t)M, dtype);
    if (var_out) fill_nan(var_out, full_cov ? (size_t)M * M : (size_t)M, dtype);
    if (acq_out) fill_nan(acq_out, (size_t)M, dtype);
    return HBO_NOT_PD;
  }
  return HBO_OK;
}

extern "C" int hbo_predict(hbo_ctx* c, const hbo_model* m, hbo_cache* k, const void* xq, int64_t M, int full_cov,
                           void* mu_out, void* var_out) {
  return posterior(c, m, k, xq, M, full_cov, mu_out, var_out, nullptr, acq_what_registry(0, nullptr), 0, 1);
}
extern "C" int hbo_acq(hbo_ctx* c, const hbo_model* m, hbo_cache* k, const void* xq, int64_t M, int acq_id,
                       double param, double add_noise, double scale, void* out) {
  if (acq_id < 0 || acq_id > HBO_ACQ_UCB) return fail(c, HBO_ERR_ARG, "hbo_acq: bad acq_id");
  if (!out) return fail(c, HBO_ERR_ARG, "hbo_acq: out is null");
  return posterior(c, m, k, xq, M, 0, nullptr, nullptr, out, acq_what_registry(acq_id, &param), add_noise, scale);
}

// ---- S hyper-parameter samples of one model family as ONE batch ------------------------------------------------------------
// hyperbo/bo_utils/acfun.py:72-82 evaluates an acquisition function on an HGP by looping `predict` over the model-parameter
// samples (gp.py:666-682: every sample re-factorises the same observations under its own hyper-parameters); with jax that loop is
// what one would `vmap`.  Here the S Gram matrices are built and factorised as one batch of S tasks -- the kernels that depend on
// the model read one ModelDev per task (GramArgs::model_stride, launch_aug_rows) -- the inverses and alpha = K^-1 (y - mu)
// likewise, and the S posteriors + acquisition epilogues then queue up on the stream without a host round trip between them:
// one upload, one copy back, one wait.  out: [S, M] acquisition values (model dtype), row s = sample s.
extern "C" int hbo_acq_samples(hbo_ctx* c, const hbo_model* models, int32_t S, const void* x, int64_t n, const void* y, int32_t mcols,
                               const void* xq, int64_t M, int acq_id, const double* params, const double* add_noise, double scale,
                               void* out) {
  if (!c || !models || !x || !y || !xq || !out || !params || !add_noise) return fail(c, HBO_ERR_ARG, "hbo_acq_samples: null argument");
  if (S <= 0 || S > 4096) return fail(c, HBO_ERR_ARG, "hbo_acq_samples: 1 <= S <= 4096");
  if (n <= 0 || mcols <= 0 || mcols > HBO_TILE) return fail(c, HBO_ERR_ARG, "hbo_acq_samples: need n>0 and 1<=m<=128");
  if (acq_id < 0 || acq_id > HBO_ACQ_UCB) return fail(c, HBO_ERR_ARG, "hbo_acq_samples: bad acq_id");
  if (M <= 0) return HBO_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const hbo_model* m0 = &models[0];
  if (int rc = model_family_check(c, "hbo_acq_samples: ", models, S, "evaluate the samples with hbo_acq")) return rc;
  prof_begin(c);
  const int dtype = m0->dtype;
  const size_t es = esize(dtype);
  hipStream_t st = c->stream;
  const int D = m0->input_dim;
  const bool mlp = needs_mlp(m0);
  std::vector<hbo_cache*> ks(S, nullptr);
  auto cleanup = [&]() { for (hbo_cache* k : ks) if (k) hbo_cache_free(c, k); };
  // ---- the S models with their MLP weights (one block, through the pinned stage) and the queries: device copies that live for the whole call
  // (the stage keeps twice models_b of pinned host memory, pinned_stage, until a larger request replaces it: S ModelDevs, and S times the weights of the MLP where there is one)
  const MlpShape sh = mlp_shape(m0);
  const size_t models_b = models_pack_bytes(sh, S);
  ModelDev* d_models = static_cast<ModelDev*>(ws_get(c, WS_SMP_MODELS, models_b));
  TaskDesc* d_batch = static_cast<TaskDesc*>(ws_get(c, WS_SMP_DESC, sizeof(TaskDesc) * S));
  int* d_infos = static_cast<int*>(ws_get(c, WS_SMP_INFO, sizeof(int) * S));
  char* d_acq = static_cast<char*>(ws_get(c, WS_SMP_ACQ, (size_t)S * M * es));
  char* d_xq = static_cast<char*>(ws_get(c, WS_SMP_XQ, (size_t)M * D * es));
  if (!d_models || !d_batch || !d_infos || !d_acq || !d_xq) return HBO_ERR_HIP;
  std::vector<void*> w_dev((size_t)S * HBO_MAX_MLP_LAYERS, nullptr), b_dev((size_t)S * HBO_MAX_MLP_LAYERS, nullptr);
  char* h_models = static_cast<char*>(stage_begin(c, "hbo_acq_samples: ", models_b));
  if (!h_models) return HBO_ERR_HIP;
  memset(h_models, 0, models_b);
  models_pack(h_models, reinterpret_cast<char*>(d_models), models, S, sh, w_dev.data(), b_dev.data());
  HIPCHK_OR(c, stage_upload(c, d_models, h_models, models_b, st), cleanup());
  HIPCHK_OR(c, hipMemcpyAsync(d_xq, xq, (size_t)M * D * es, hipMemcpyHostToDevice, st), cleanup());
  // ---- S caches over the same observations (each a complete hbo_cache: everything that reads one works on them)
  const std::vector<unsigned char> yt = transpose_y(y, n, mcols, es);
  std::vector<TaskDesc> h_batch(S);
  for (int s = 0; s < S; ++s) {
    int rc = cache_alloc(c, &models[s], n, mcols, &ks[s]);
    if (rc) { cleanup(); return rc; }
    hbo_cache* k = ks[s]; TaskHost* t = k->t;
    if (s == 0) {
      HIPCHK_OR(c, hipMemcpyAsync(t->X, x, (size_t)n * D * es, hipMemcpyHostToDevice, st), cleanup());
      HIPCHK_OR(c, hipMemcpyAsync(t->ysum, yt.data(), (size_t)n * mcols * es, hipMemcpyHostToDevice, st), cleanup());
    } else {
      HIPCHK_OR(c, hipMemcpyAsync(t->X, ks[0]->t->X, (size_t)n * D * es, hipMemcpyDeviceToDevice, st), cleanup());
      HIPCHK_OR(c, hipMemcpyAsync(t->ysum, ks[0]->t->ysum, (size_t)n * mcols * es, hipMemcpyDeviceToDevice, st), cleanup());
    }
    h_batch[s] = k->h_desc;
    HIPCHK_OR(c, hipMemcpyAsync(k->d_desc, &k->h_desc, sizeof(TaskDesc), hipMemcpyHostToDevice, st), cleanup());
  }
  HIPCHK_OR(c, hipMemcpyAsync(d_batch, h_batch.data(), sizeof(TaskDesc) * S, hipMemcpyHostToDevice, st), cleanup());
  HIPCHK_OR(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_infos), INT_MAX, S, st), cleanup());
  // ---- one batched pipeline: features (per sample: its own weights), residual rows, Gram, factorisation, inverse, alpha
  FactorBatch fb = {models, S, ks.data(), d_batch, d_infos, d_models, 1, mlp ? w_dev.data() : nullptr, mlp ? b_dev.data() : nullptr, false};
  { int rc = enqueue_factor(c, fb); if (rc) { cleanup(); return rc; } }
  std::vector<int> h_infos(S, INT_MAX);
  HIPCHK_OR(c, hipMemcpyAsync(h_infos.data(), d_infos, sizeof(int) * S, hipMemcpyDeviceToHost, st), cleanup());
  HIPCHK_OR(c, hipStreamSynchronize(st), cleanup());   // (the samples' info words decide NaN rows below; the caller's x / y / weights have been consumed)
  // ---- S posteriors + acquisition epilogues: three independent launch chains (main stream + the two side streams, each with its
  //      own workspaces) -- a pass is ~7 latency-bound launches of 10-20 us, and the passes of different samples share nothing
  const int lanes = (M <= std::max<int64_t>(c->opt_post_chunk, HBO_TILE)) ? 3 : 1;
  hipStream_t lane_stream[3] = {st, c->stream2, c->stream4};
  if (lanes > 1) { hipEvent_t e = pool_event(c, 0); hipEventRecord(e, st); hipStreamWaitEvent(c->stream2, e, 0); hipStreamWaitEvent(c->stream4, e, 0); }
  bool any_bad = false;
  for (int s = 0; s < S; ++s) {
    ks[s]->info = h_infos[s];
    PosteriorOverride ov = {d_models + s, mlp ? &w_dev[(size_t)s * HBO_MAX_MLP_LAYERS] : nullptr, mlp ? &b_dev[(size_t)s * HBO_MAX_MLP_LAYERS] : nullptr, d_xq,
                            d_acq + (size_t)s * M * es, lanes > 1 ? s % lanes : 0};
    int rc = posterior(c, &models[s], ks[s], xq, M, 0, nullptr, nullptr, out, acq_what_registry(acq_id, &params[s]), add_noise[s], scale, &ov);
    if (rc == HBO_NOT_PD) any_bad = true;
    else if (rc) { for (hipStream_t q : lane_stream) hipStreamSynchronize(q); cleanup(); return rc; }
  }
  for (int l = 1; l < lanes; ++l) { hipEvent_t e = pool_event(c, (size_t)l); hipEventRecord(e, lane_stream[l]); hipStreamWaitEvent(st, e, 0); }
  HIPCHK_OR(c, hipMemcpyAsync(out, d_acq, (size_t)S * M * es, hipMemcpyDeviceToHost, st), cleanup());
  HIPCHK_OR(c, hipStreamSynchronize(st), cleanup());
  HIPCHK_OR(c, hipStreamSynchronize(c->stream2), cleanup());
  HIPCHK_OR(c, hipGetLastError(), cleanup());
  prof_collect(c);
  for (int s = 0; s < S; ++s) if (h_infos[s] != INT_MAX) fill_nan((char*)out + (size_t)s * M * es, (size_t)M, dtype);
  cleanup();
  return any_bad ? HBO_NOT_PD : HBO_OK;
}

