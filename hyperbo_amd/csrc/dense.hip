// The dense entry points of the C ABI on host arrays (include/hbo.h): hbo_gram, hbo_mean, hbo_chol_solve, hbo_spd_solve.  Each uploads,
// runs the kernels of the hot path once and copies back; its device temporaries live in a DevBuf (runtime.h) until it returns.
#include "api_internal.h"

// ---- Gram / mean on host arrays --------------------------------------------------------------
extern "C" int hbo_gram(hbo_ctx* c, const hbo_model* m, const void* x1, int64_t n1, const void* x2, int64_t n2, int diag, void* out) {
  if (!c || !x1 || !out) return fail(c, HBO_ERR_ARG, "hbo_gram: null argument");
  if (diag && x2) return fail(c, HBO_ERR_ARG, "hbo_gram: diag requires x2 == NULL (kernel.py:54-57)");
  if (n1 <= 0) return HBO_OK;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = upload_model(c, m);
  if (rc) return rc;
  const int dtype = m->dtype; const size_t es = esize(dtype);
  hipStream_t st = c->stream;
  if (!x2) n2 = n1;
  if (n2 <= 0) return HBO_OK;
  DevBuf buf;
  void *d1 = nullptr, *d2 = nullptr, *dout = nullptr, *w1 = nullptr, *w2 = nullptr;
  FeatBuf f1, f2;
  HIPCHK(c, buf.get(c, &d1, (size_t)n1 * m->input_dim * es));
  HIPCHK(c, hipMemcpyAsync(d1, x1, (size_t)n1 * m->input_dim * es, hipMemcpyHostToDevice, st));
  const void* F1 = d1; const void* F2 = d1;
  if (m->kernel_uses_mlp) { rc = f1.ensure(c, m, n1); if (rc) return rc; run_mlp(c, m, d1, n1, f1.acts.data()); F1 = F2 = f1.acts[m->n_layers - 1]; }
  if (is_kumar(m)) {   // kernel.py:190-217: K(w(x1), w(x2))
    HIPCHK(c, buf.get(c, &w1, (size_t)n1 * m->input_dim * es));
    launch_kumar_forward(dtype, nullptr, 0, 0, d1, w1, nullptr, n1, m->input_dim, c->d_model, st);
    F1 = F2 = w1;
  }
  if (x2) {
    HIPCHK(c, buf.get(c, &d2, (size_t)n2 * m->input_dim * es));
    HIPCHK(c, hipMemcpyAsync(d2, x2, (size_t)n2 * m->input_dim * es, hipMemcpyHostToDevice, st));
    F2 = d2;
    if (m->kernel_uses_mlp) { rc = f2.ensure(c, m, n2); if (rc) return rc; run_mlp(c, m, d2, n2, f2.acts.data()); F2 = f2.acts[m->n_layers - 1]; }
    if (is_kumar(m)) {
      HIPCHK(c, buf.get(c, &w2, (size_t)n2 * m->input_dim * es));
      launch_kumar_forward(dtype, nullptr, 0, 0, d2, w2, nullptr, n2, m->input_dim, c->d_model, st);
      F2 = w2;
    }
  }
  const int fdim = feature_dim(m);
  if (diag) {
    HIPCHK(c, buf.get(c, &dout, (size_t)n1 * es));
    launch_kdiag(dtype, F1, n1, fdim, c->d_model, dout, st);
    HIPCHK(c, hipMemcpyAsync(out, dout, (size_t)n1 * es, hipMemcpyDeviceToHost, st));
  } else {
    HIPCHK(c, buf.get(c, &dout, (size_t)n1 * n2 * es));
    GramArgs g = {}; g.kernel_id = c->h_model->kernel_id; g.mfma_min_f = c->opt_gram_mfma; g.x1 = F1; g.x2 = F2; g.out = dout; g.n1 = n1; g.n2 = n2; g.ldo = n2; g.fdim = fdim;
    launch_gram(dtype, g, c->d_model, dim3((unsigned)((n2 + 127) / 128), (unsigned)((n1 + 127) / 128), 1), st);
    HIPCHK(c, hipMemcpyAsync(out, dout, (size_t)n1 * n2 * es, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  return HBO_OK;
}

extern "C" int hbo_mean(hbo_ctx* c, const hbo_model* m, const void* x, int64_t n, void* out) {
  if (!c || !x || !out) return fail(c, HBO_ERR_ARG, "hbo_mean: null argument");
  if (n <= 0) return HBO_OK;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = upload_model(c, m);
  if (rc) return rc;
  const int dtype = m->dtype; const size_t es = esize(dtype);
  hipStream_t st = c->stream;
  DevBuf buf;
  void *dx = nullptr, *dout = nullptr;
  FeatBuf f;
  hipError_t e = buf.get(c, &dx, (size_t)n * m->input_dim * es);
  if (e == hipSuccess) e = buf.get(c, &dout, (size_t)n * es);
  if (e == hipSuccess) e = hipMemcpyAsync(dx, x, (size_t)n * m->input_dim * es, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return fail(c, HBO_ERR_HIP, hipGetErrorString(e));
  const void* Fm = (m->mean_id == HBO_MEAN_LINEAR) ? dx : nullptr;
  if (m->mean_id == HBO_MEAN_LINEAR_MLP) { rc = f.ensure(c, m, n); if (rc) return rc; run_mlp(c, m, dx, n, f.acts.data()); Fm = f.acts[m->n_layers - 1]; }
  launch_mean(dtype, Fm, n, mean_feature_dim(m), c->d_model, dout, st);
  e = hipMemcpyAsync(out, dout, (size_t)n * es, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return fail(c, HBO_ERR_HIP, hipGetErrorString(e));
  return HBO_OK;
}

// ---- dense SPD building block ---------------------------------------------------------------
// x = L^-T L^-1 b with a factor the caller already holds (linalg.py:139-145, the `cached_cholesky=` branch): the factor and the
// right-hand sides go up, two substitution sweeps run on the device (trisolve.hip), the solution comes back.
void launch_chol_solve(int dtype, const void* L, int64_t n, void* rhs, int64_t npad, int m, hipStream_t st);   // trisolve.hip
extern "C" int hbo_chol_solve(hbo_ctx* c, int dtype, const void* chol_lower, int64_t n, const void* b, int32_t mcols, void* x_out) {
  if (!c || !chol_lower || !b || !x_out) return fail(c, HBO_ERR_ARG, "hbo_chol_solve: null argument");
  if (n <= 0 || mcols <= 0) return fail(c, HBO_ERR_ARG, "hbo_chol_solve: n and m must be positive");
  if (dtype != HBO_F32 && dtype != HBO_F64) return fail(c, HBO_ERR_ARG, "hbo_chol_solve: bad dtype");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t es = esize(dtype);
  hipStream_t st = c->stream;
  const int64_t npad = round_up(n, 64);
  DevBuf buf;
  void *d_l = nullptr, *d_r = nullptr;
  // right-hand sides as rows (m x npad, zero padding)
  std::vector<unsigned char> rt((size_t)mcols * npad * es, 0);
  cols_to_rows(rt.data(), b, n, mcols, npad, es);
  HIPCHK(c, buf.get(c, &d_l, (size_t)n * n * es));
  HIPCHK(c, buf.get(c, &d_r, rt.size()));
  HIPCHK(c, hipMemcpyAsync(d_l, chol_lower, (size_t)n * n * es, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_r, rt.data(), rt.size(), hipMemcpyHostToDevice, st));
  launch_chol_solve(dtype, d_l, n, d_r, npad, mcols, st);
  HIPCHK(c, hipMemcpyAsync(rt.data(), d_r, rt.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  rows_to_cols(x_out, rt.data(), n, mcols, npad, es);
  return HBO_OK;
}

extern "C" int hbo_spd_solve(hbo_ctx* c, int dtype, const void* a, int64_t n, const void* b, int32_t mcols, void* chol_out, void* inv_out, void* x_out,
                             double* logdet_half) {
  if (!c || !a) return fail(c, HBO_ERR_ARG, "hbo_spd_solve: null argument");
  if (n <= 0) return fail(c, HBO_ERR_ARG, "hbo_spd_solve: n must be positive");
  if (b && (mcols <= 0 || mcols > HBO_TILE)) return fail(c, HBO_ERR_ARG, "hbo_spd_solve: 1 <= m <= 128");
  if (dtype != HBO_F32 && dtype != HBO_F64) return fail(c, HBO_ERR_ARG, "hbo_spd_solve: bad dtype");
  HIPCHK(c, hipSetDevice(c->device));
  prof_begin(c);
  const size_t es = esize(dtype);
  hipStream_t st = c->stream;
  DevBuf buf;
  void *d_a = nullptr, *d_b = nullptr, *d_tmp = nullptr; TaskDesc* d_desc = nullptr; int* d_info = nullptr;
  struct TaskGuard { hbo_ctx* c; TaskHost* t; ~TaskGuard() { free_task(c, t); } } guard = {c, new TaskHost()};   // (its buffers are pooled)
  TaskHost* t = guard.t;
  task_shape(t, n, b ? mcols : 1, dtype);
  const bool need_inv = inv_out != nullptr || x_out != nullptr;
  { int rc = ensure_task_workspace(c, dtype, t, need_inv, t->m); if (rc) return rc; }
  HIPCHK(c, buf.get(c, &d_a, (size_t)n * n * es));
  HIPCHK(c, hipMemcpyAsync(d_a, a, (size_t)n * n * es, hipMemcpyHostToDevice, st));
  if (b) { HIPCHK(c, buf.get(c, &d_b, (size_t)n * mcols * es)); HIPCHK(c, hipMemcpyAsync(d_b, b, (size_t)n * mcols * es, hipMemcpyHostToDevice, st)); }
  launch_fill_spd(dtype, d_a, n, t->A, t->ld, t->npad, st);
  launch_set_aug(dtype, d_b, n, b ? mcols : 0, t->A, t->ld, t->npad, st);
  TaskDesc h; memset(&h, 0, sizeof h);
  h.A = t->A; h.W = t->W; h.S = t->S; h.wscr = t->wscr; h.svec = t->svec; h.n = (int)n; h.npad = t->npad; h.nblk = t->nblk; h.m = t->m; h.ld = t->ld;
  h.naug = t->m;
  HIPCHK(c, buf.get(c, &d_desc, sizeof h));
  HIPCHK(c, buf.get(c, &d_info, sizeof(int)));
  int inf = INT_MAX;
  HIPCHK(c, hipMemcpyAsync(d_desc, &h, sizeof h, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_info, &inf, sizeof(int), hipMemcpyHostToDevice, st));
  HIPCHK(c, hipStreamSynchronize(st));
  // hbo_tune "spd_diag_bound" (test hook): max_i A_ii off the caller's matrix -- what potrf_plan, trtri_level3 and run_lauum need to
  // take the f16x2 form, as hbo_factor does from the model's signal variance.  Default: 0 = unknown, the bf16x3 form
  double diag_bound = 0;
  if (c->opt_spd_diag_bound) for (int64_t i = 0; i < n; ++i) diag_bound = std::max(diag_bound, host_elem(a, dtype, i * n + i));
  CholBoundScope bound_scope(c, diag_bound);
  // (the inverse and K^-1 = W^T W behind the factorisation, nothing beside it)
  InvRun inv = inv_run(c, dtype, d_desc, 1, t->nblk, &h, inv_out ? INV_W_KINV : (need_inv ? INV_W : INV_NONE), false);
  { ProfScope ps(c, "potrf", 1); run_potrf(c, dtype, d_desc, 1, t->nblk, d_info, &inv); }
  if (need_inv) {
    { ProfScope ps(c, "trtri", 1); run_trtri(inv); }
    if (x_out && b) for (int col = 0; col < mcols; ++col) launch_wt_z(dtype, d_desc, 1, t->nblk, col, col, t->npad, st);
    if (inv_out) { ProfScope ps(c, "lauum", 1); run_lauum(inv); }
  }
  HIPCHK(c, hipMemcpyAsync(&inf, d_info, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(c, buf.get(c, &d_tmp, (size_t)n * n * es));
  std::vector<unsigned char> hchol;
  if (chol_out || logdet_half) {
    launch_extract_lower(dtype, t->A, t->ld, n, d_tmp, st);
    void* dst = chol_out;
    if (!dst) { hchol.resize((size_t)n * n * es); dst = hchol.data(); }
    HIPCHK(c, hipMemcpyAsync(dst, d_tmp, (size_t)n * n * es, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (logdet_half) { double s = 0; for (int64_t i = 0; i < n; ++i) s += log(host_elem(dst, dtype, i * n + i)); *logdet_half = s; }
  }
  if (inv_out) {
    launch_symmetrize_from_lower(dtype, t->S, t->ld, n, d_tmp, st);
    HIPCHK(c, hipMemcpyAsync(inv_out, d_tmp, (size_t)n * n * es, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(c, hipStreamSynchronize(st));
  if (x_out && b) {
    std::vector<unsigned char> xr((size_t)mcols * t->npad * es);
    HIPCHK(c, hipMemcpy(xr.data(), t->svec, xr.size(), hipMemcpyDeviceToHost));
    rows_to_cols(x_out, xr.data(), n, mcols, t->npad, es);
  }
  HIPCHK(c, hipGetLastError());
  prof_collect(c);
  const bool bad = inf != INT_MAX;
  if (bad) {
    if (chol_out) fill_nan(chol_out, (size_t)n * n, dtype);
    if (inv_out) fill_nan(inv_out, (size_t)n * n, dtype);
    if (x_out && b) fill_nan(x_out, (size_t)n * mcols, dtype);
    if (logdet_half) *logdet_half = NAN;
  }
  return bad ? HBO_NOT_PD : HBO_OK;
}
