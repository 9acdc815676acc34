// What include/hbo_tune.h declares apart from hbo_tune itself (api.hip): the MFMA rate probe of bench.py and the test hooks that run
// single launches of the posterior and the Gram, and the factor, inverse and gradient-contraction steps of an evaluation, on caller-chosen operands.  (hbo_probe_acq_grad_samples64 is a second door to
// acq_grad.hip's acq_grad_samples and stays beside it; the control-text probes stay with their kernels in train.hip and acq_opt.hip.)
#include "api_internal.h"
#include "../../include/hbo_tune.h"

// Sustained fp64 MFMA rate of THIS device, measured now (include/hbo_tune.h): every SIMD of every CU runs two waves of
// back-to-back independent v_mfma_f64_16x16x4_f64 (4 accumulators per wave, no memory traffic) for ~`ms` milliseconds between two
// HIP events.  What bench.py reports beside the 78.6 TFLOP/s datasheet figure: the denominator a kernel can actually reach at the
// clock the chip holds under an fp64 MFMA load.  (Four accumulators per wave, the loop in assembly: see the kernel.)
namespace {
typedef double probe_d4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void mfma_probe_kernel(double* out, int iters) {
  probe_d4 acc[4];
  const double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = (probe_d4){0, 0, 0, 0};
  // the whole loop is ONE assembly block: around a builtin (or a per-instruction asm) inside a C loop the register allocator parks
  // the loop-carried accumulators in VGPRs and copies them to AGPRs and back every iteration (16 v_accvgpr moves per MFMA)
  int n = iters;
  asm volatile(
      "1:\n"
      "v_mfma_f64_16x16x4_f64 %0, %5, %6, %0\n"
      "v_mfma_f64_16x16x4_f64 %1, %5, %6, %1\n"
      "v_mfma_f64_16x16x4_f64 %2, %5, %6, %2\n"
      "v_mfma_f64_16x16x4_f64 %3, %5, %6, %3\n"
      "s_sub_u32 %4, %4, 1\n"
      "s_cmp_lg_u32 %4, 0\n"
      "s_cbranch_scc1 1b\n"
      "s_nop 15\n"
      : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+s"(n)
      : "v"(a), "v"(b)
      : "scc");
  double sacc = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) sacc += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = sacc;
}
}  // namespace
extern "C" int hbo_mfma_peak_probe(hbo_ctx* c, double ms, double* tflops_out) {
  if (!c || !tflops_out || !(ms > 0) || ms > 1000) return fail(c, HBO_ERR_ARG, "hbo_mfma_peak_probe: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  const int blocks = 2 * c->n_cus;   // two 4-wave workgroups per CU: two waves per SIMD
  double* d_out = static_cast<double*>(ws_get(c, WS_PROBE, sizeof(double) * 256 * blocks));
  if (!d_out) return HBO_ERR_HIP;
  hipEvent_t e0 = pool_event_timed(c, 0), e1 = pool_event_timed(c, 1);
  double best = 0;
  int iters = 8192;
  for (int rep = 0; rep < 3; ++rep) {   // the first pass sizes the second and third to ~ms
    HIPCHK(c, hipEventRecord(e0, c->stream));
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(blocks), dim3(256), 0, c->stream, d_out, iters);
    HIPCHK(c, hipEventRecord(e1, c->stream));
    HIPCHK(c, hipEventSynchronize(e1));
    float el = 0;
    HIPCHK(c, hipEventElapsedTime(&el, e0, e1));
    const double flops = (double)blocks * 4 * (double)iters * 4 * 2048.0;   // waves x MFMAs x 16*16*4*2
    if (rep > 0) best = std::max(best, flops / (el * 1e-3) / 1e12);
    if (rep == 0) iters = (int)std::min(4.0e6, std::max(1024.0, iters * ms / std::max((double)el, 1e-3)));
  }
  HIPCHK(c, hipGetLastError());
  *tflops_out = best;
  return HBO_OK;
}

// Test hook (include/hbo_tune.h): the fp32 split-operand posterior product on caller-chosen operands -- W and Kxq go up padded as a
// cache holds them, the three launches of the posterior (cache.hip: post3_*) run once over all M candidates, the per-row-block column sums of V^2
// come back.  The split buffers are filled with 0xFF (NaN in bf16 and fp16) first: a block the product reads but no split wrote shows.
extern "C" int hbo_probe_post_product(hbo_ctx* c, int form, const float* W, int64_t n, const float* Kxq, int64_t M, double k_bound,
                                      int use_counter, float* colsq_out) {
  if (!c || !W || !Kxq || !colsq_out) return fail(c, HBO_ERR_ARG, "hbo_probe_post_product: null argument");
  if (form != 0 && form != 1) return fail(c, HBO_ERR_ARG, "hbo_probe_post_product: form is 0 (bf16x3) or 1 (f16x2)");
  if (n <= 0 || n > 16384 || M <= 0 || M > (1 << 20)) return fail(c, HBO_ERR_ARG, "hbo_probe_post_product: need 1 <= n <= 16384 and 1 <= M <= 2^20");
  if (use_counter != 0 && use_counter != 1) return fail(c, HBO_ERR_ARG, "hbo_probe_post_product: use_counter is 0 or 1");
  if (form == 1 && (!(k_bound > 0) || !(k_bound < 1e30))) return fail(c, HBO_ERR_ARG, "hbo_probe_post_product: f16x2 needs a positive finite k_bound");
  HIPCHK(c, hipSetDevice(c->device));
  const bool h2 = form == 1;
  const int planes = h2 ? 2 : 3;
  const int npad = round_up(n, HBO_TILE), nblk = npad / HBO_TILE, mpad = round_up(M, HBO_TILE);
  const int64_t ld = padded_ld(npad, HBO_F32), ldq = padded_ld(mpad, HBO_F32);
  const float kscale = h2 ? post2h_scale_for(k_bound) : 1.f;
  const size_t w_b = (size_t)npad * ld * sizeof(float), k_b = (size_t)npad * ldq * sizeof(float), c_b = (size_t)nblk * ldq * sizeof(float);
  const size_t w3_b = (size_t)npad * npad * planes * sizeof(unsigned short), k3_b = (size_t)mpad * npad * planes * sizeof(unsigned short);
  hipStream_t st = c->stream;
  DevBuf buf;
  void *d_w = nullptr, *d_k = nullptr, *d_c = nullptr, *d_w3 = nullptr, *d_k3 = nullptr, *d_words = nullptr;
  HIPCHK(c, buf.get(c, &d_w, w_b)); HIPCHK(c, buf.get(c, &d_k, k_b)); HIPCHK(c, buf.get(c, &d_c, c_b));
  HIPCHK(c, buf.get(c, &d_w3, w3_b)); HIPCHK(c, buf.get(c, &d_k3, k3_b)); HIPCHK(c, buf.get(c, &d_words, 2 * sizeof(unsigned int)));
  HIPCHK(c, hipMemsetAsync(d_w, 0, w_b, st)); HIPCHK(c, hipMemsetAsync(d_k, 0, k_b, st)); HIPCHK(c, hipMemsetAsync(d_c, 0, c_b, st));
  HIPCHK(c, hipMemsetAsync(d_w3, 0xFF, w3_b, st)); HIPCHK(c, hipMemsetAsync(d_k3, 0xFF, k3_b, st));
  HIPCHK(c, hipMemcpy2DAsync(d_w, (size_t)ld * sizeof(float), W, (size_t)n * sizeof(float), (size_t)n * sizeof(float), (size_t)n, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpy2DAsync(d_k, (size_t)ldq * sizeof(float), Kxq, (size_t)M * sizeof(float), (size_t)M * sizeof(float), (size_t)n, hipMemcpyHostToDevice, st));
  unsigned int* d_wmax = static_cast<unsigned int*>(d_words);
  post3_split_w(static_cast<const float*>(d_w), ld, nblk, h2, static_cast<unsigned short*>(d_w3), d_wmax, st);
  post3_split_kxq(static_cast<const float*>(d_k), ldq, mpad, npad, h2, kscale, static_cast<unsigned short*>(d_k3), st);
  post3_product(static_cast<const unsigned short*>(d_w3), static_cast<const unsigned short*>(d_k3), nblk, mpad, h2, d_wmax, kscale,
                static_cast<float*>(d_c), ldq, use_counter ? reinterpret_cast<int*>(d_wmax + 1) : nullptr, st);
  HIPCHK(c, hipMemcpy2DAsync(colsq_out, (size_t)M * sizeof(float), d_c, (size_t)ldq * sizeof(float), (size_t)M * sizeof(float), (size_t)nblk, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  return HBO_OK;
}

// Test hook (include/hbo_tune.h): the streamed posterior on caller-chosen operands.  A cache-shaped object is built with the shipped
// helpers (task_shape, ensure_task_workspace, fill_desc; W in t->W, alpha in t->svec, info = INT_MAX) and posterior() (cache.hip) runs
// over it with a PostProbe: its produce_chunk then copies the caller's columns of Kxq, kdiag and mu0 into each chunk's slices instead of
// launching the features and the cross Gram.  Plan, workspaces, split of W, the products, the epilogue, the chunk loop and its events
// are posterior()'s own; the model handed to it only carries what post_plan reads (dtype; stationary with signal variance k_bound, or the
// dot product) and a zero mean that is never evaluated.
extern "C" int hbo_probe_posterior(hbo_ctx* c, int dtype, const void* W, int64_t n, const void* alpha, const void* Kxq, const void* kdiag,
                                   const void* mu0, int64_t M, double k_bound, void* mu_out, void* var_out, void* colsq_out,
                                   void* mupart_out, hbo_probe_post_plan* plan_out) {
  if (!c || !W || !alpha || !Kxq || !kdiag || !mu0 || !mu_out || !var_out) return fail(c, HBO_ERR_ARG, "hbo_probe_posterior: null argument");
  if (dtype != HBO_F32 && dtype != HBO_F64) return fail(c, HBO_ERR_ARG, "hbo_probe_posterior: bad dtype");
  if (n <= 0 || n > 4096 || M <= 0 || M > (1 << 17)) return fail(c, HBO_ERR_ARG, "hbo_probe_posterior: need 1 <= n <= 4096 and 1 <= M <= 2^17");
  if (!(k_bound >= 0) || !(k_bound < 1e30)) return fail(c, HBO_ERR_ARG, "hbo_probe_posterior: k_bound is 0 (unbounded kernel) or positive and finite");
  for (int64_t i = 0; i < n; ++i) for (int64_t j = i + 1; j < n; ++j)
    if (host_elem(W, dtype, i * n + j) != 0) return fail(c, HBO_ERR_ARG, "hbo_probe_posterior: W must hold zeros above the diagonal");
  const size_t es = esize(dtype);
  const double one64 = 1.0; const float one32 = 1.f;
  hbo_model model; memset(&model, 0, sizeof model);
  model.dtype = dtype; model.input_dim = 1; model.mean_id = HBO_MEAN_ZERO;
  model.kernel_id = k_bound > 0 ? HBO_KERNEL_SE : HBO_KERNEL_DOT;
  model.signal_variance = k_bound > 0 ? k_bound : 1.0; model.dot_prod_sigma = 1.0;
  model.n_lengthscale = 1; model.lengthscale = dtype == HBO_F64 ? (const void*)&one64 : (const void*)&one32;
  const int nblk = (int)(round_up(n, HBO_TILE) / HBO_TILE);
  const PostPlan pre = post_plan(c, &model, M, nblk, false, nullptr);
  if ((colsq_out || mupart_out) && pre.nchunks != 1) return fail(c, HBO_ERR_ARG, "hbo_probe_posterior: colsq_out and mupart_out need a single-chunk call (option post_chunk)");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  hbo_cache* k = new hbo_cache();
  // (the cache leaves when the call does, behind a wait: its buffers go back to the pool.  Before buf's memory is freed.)
  DevBuf buf;
  struct CacheGuard { hbo_ctx* c; hbo_cache* k; ~CacheGuard() { hipDeviceSynchronize(); hbo_cache_free(c, k); } } guard = {c, k};
  k->dtype = dtype; k->D = 1; k->m = 1; k->input_warp = HBO_WARP_NONE; k->info = INT_MAX;
  TaskHost* t = k->t = new TaskHost();
  task_shape(t, n, 1, dtype);
  int rc = ensure_task_workspace(c, dtype, t, false, 1);
  if (rc) return rc;
  fill_desc(k->h_desc, t, &model, dtype, ROLE_FACTOR);
  HIPCHK(c, hbo_malloc(c, (void**)&k->d_desc, sizeof(TaskDesc)));
  void *d_kxq = nullptr, *d_kd = nullptr, *d_mu0 = nullptr;
  HIPCHK(c, buf.get(c, &d_kxq, (size_t)n * M * es)); HIPCHK(c, buf.get(c, &d_kd, (size_t)M * es)); HIPCHK(c, buf.get(c, &d_mu0, (size_t)M * es));
  const size_t w_b = (size_t)t->npad * t->ld * es;
  HIPCHK(c, hipMemcpyAsync(k->d_desc, &k->h_desc, sizeof(TaskDesc), hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(t->W, 0, w_b, st));   // (a pooled W keeps what its last owner left below the diagonal)
  HIPCHK(c, hipMemcpy2DAsync(t->W, (size_t)t->ld * es, W, (size_t)n * es, (size_t)n * es, (size_t)n, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(t->svec, 0, (size_t)t->npad * es, st));
  HIPCHK(c, hipMemcpyAsync(t->svec, alpha, (size_t)n * es, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_kxq, Kxq, (size_t)n * M * es, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_kd, kdiag, (size_t)M * es, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_mu0, mu0, (size_t)M * es, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const std::vector<unsigned char> xq0((size_t)M * es, 0);   // the queries posterior() uploads; nothing reads them here
  PostProbe probe = {}; probe.Kxq = d_kxq; probe.kdiag = d_kd; probe.mu0 = d_mu0;
  rc = posterior(c, &model, k, xq0.data(), M, 0, mu_out, var_out, nullptr, acq_what_registry(0, nullptr), 0, 1, nullptr, &probe);
  if (rc) return rc;
  const PostPlan& p = probe.plan;
  if (plan_out) *plan_out = {(int32_t)p.form, p.kchunk, p.nch, (int32_t)p.nchunks, p.nbuf, probe.resident_chunks, p.direct_form ? 1 : 0};
  // single-chunk calls: the partials the epilogue summed stand in workspace 0 of their slots, rows ldq apart
  const size_t pitch = (size_t)p.chunk(0).ldq * es;
  if (colsq_out) HIPCHK(c, hipMemcpy2D(colsq_out, (size_t)M * es, c->ws[WS_COLSQ].first, pitch, (size_t)M * es, (size_t)nblk, hipMemcpyDeviceToHost));
  if (mupart_out) HIPCHK(c, hipMemcpy2D(mupart_out, (size_t)M * es, c->ws[WS_MUPART].first, pitch, (size_t)M * es, (size_t)nblk, hipMemcpyDeviceToHost));
  return HBO_OK;
}

// Test hook (include/hbo_tune.h): launch_gram in the two forms hbo_gram never takes, on caller-chosen inputs, with every element of the
// output buffer preset to a sentinel so that what the kernel leaves alone shows.  Form 1 is the launch of cache.hip's produce_chunk (sizes from
// post_plan), form 2 the launch of objective_local / enqueue_factor over a dataset built by hbo_dataset_create, its workspaces by
// ensure_task_workspace and its descriptors by fill_desc.
extern "C" int hbo_probe_gram(hbo_ctx* c, int form, const hbo_model* models, int32_t n_models, const void* x, const int64_t* ns, int32_t T,
                              const void* x2, int64_t n2, int direct_form, double sentinel, void* out, int64_t out_cap, int64_t* rows_out,
                              int64_t* ld_out) {
  if (!c || !models || !x || !ns || !out || !rows_out || !ld_out) return fail(c, HBO_ERR_ARG, "hbo_probe_gram: null argument");
  if (form != 1 && form != 2) return fail(c, HBO_ERR_ARG, "hbo_probe_gram: form is 1 (padded cross Gram) or 2 (batched task form)");
  if (T <= 0 || T > 64) return fail(c, HBO_ERR_ARG, "hbo_probe_gram: 1 <= T <= 64");
  if (form == 1 && (T != 1 || n_models != 1 || !x2 || n2 <= 0)) return fail(c, HBO_ERR_ARG, "hbo_probe_gram: form 1 takes one task, one model and x2 [n2 > 0, D]");
  if (form == 2 && (x2 || n2 != 0 || direct_form != 0)) return fail(c, HBO_ERR_ARG, "hbo_probe_gram: form 2 takes neither x2 nor direct_form");
  if (form == 2 && n_models != 1 && n_models != T) return fail(c, HBO_ERR_ARG, "hbo_probe_gram: form 2 takes one model or one per task");
  if (direct_form != 0 && direct_form != 1) return fail(c, HBO_ERR_ARG, "hbo_probe_gram: direct_form is 0 or 1");
  for (int k = 0; k < T; ++k) if (ns[k] <= 0 || ns[k] > 4096) return fail(c, HBO_ERR_ARG, "hbo_probe_gram: need 1 <= n <= 4096 for every task");
  if (out_cap <= 0) return fail(c, HBO_ERR_ARG, "hbo_probe_gram: out_cap must be positive");
  const hbo_model* m0 = &models[0];
  for (int s = 0; s < n_models; ++s) {
    const hbo_model* m = &models[s];
    if (m->input_warp != HBO_WARP_NONE || needs_mlp(m)) return fail(c, HBO_ERR_ARG, "hbo_probe_gram: models with an MLP basis or an input warp are not taken");
    if (validate_model(c, m)) return HBO_ERR_ARG;
    if (!same_model_family(m, m0)) return fail(c, HBO_ERR_ARG, "hbo_probe_gram: the models must share dtype, covariance, mean and input_dim");
  }
  const int dtype = m0->dtype, D = m0->input_dim, fdim = feature_dim(m0);
  const size_t es = esize(dtype);
  PostPlan plan = {};
  if (form == 1) {
    plan = post_plan(c, m0, n2, round_up(ns[0], HBO_TILE) / HBO_TILE, false, nullptr);
    if (plan.refuse || plan.nchunks != 1) return fail(c, HBO_ERR_ARG, "hbo_probe_gram: n2 must fit one posterior chunk (option post_chunk)");
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  auto fill = [&](std::vector<unsigned char>& h, size_t count) {
    h.resize(count * es);
    if (dtype == HBO_F64) for (size_t i = 0; i < count; ++i) ((double*)h.data())[i] = sentinel;
    else for (size_t i = 0; i < count; ++i) ((float*)h.data())[i] = (float)sentinel;
  };

  if (form == 1) {
    const int64_t n1 = ns[0];
    const PostChunk ch = plan.chunk(0);
    const int npad = round_up(n1, HBO_TILE), nblk = npad / HBO_TILE;
    rows_out[0] = npad; ld_out[0] = ch.ldq;
    const size_t count = (size_t)npad * ch.ldq;
    if ((size_t)out_cap < count) return fail(c, HBO_ERR_ARG, "hbo_probe_gram: out_cap is smaller than the padded buffer");
    int rc = upload_model(c, m0);
    if (rc) return rc;
    DevBuf buf;
    void *d1 = nullptr, *d2 = nullptr, *dk = nullptr;
    std::vector<unsigned char> hs;
    fill(hs, count);
    HIPCHK(c, buf.get(c, &d1, (size_t)n1 * D * es)); HIPCHK(c, buf.get(c, &d2, (size_t)n2 * D * es));
    HIPCHK(c, buf.get(c, &dk, count * es));
    HIPCHK(c, hipMemcpyAsync(d1, x, (size_t)n1 * D * es, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d2, x2, (size_t)n2 * D * es, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(dk, hs.data(), count * es, hipMemcpyHostToDevice, st));
    GramArgs g = {}; g.kernel_id = m0->kernel_id; g.mfma_min_f = c->opt_gram_mfma; g.x1 = d1; g.x2 = d2; g.out = dk; g.n1 = n1; g.n2 = ch.mc; g.ldo = ch.ldq;
    g.n1pad = npad; g.n2pad = ch.mpad; g.fdim = fdim; g.symmetric = 0; g.padded = 1;
    g.direct_form = direct_form;
    launch_gram(dtype, g, c->d_model, dim3(ch.mpad / HBO_TILE, nblk, 1), st);
    HIPCHK(c, hipMemcpyAsync(out, dk, count * es, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    return HBO_OK;
  }

  // form 2: the dataset of the T tasks (targets: zeros, one column), the workspaces and descriptors of an NLL evaluation
  int64_t max_n = 0, rows = 0;
  for (int k = 0; k < T; ++k) max_n = std::max(max_n, ns[k]);
  const std::vector<unsigned char> y0((size_t)max_n * es, 0);
  std::vector<hbo_task> tasks(T);
  for (int k = 0; k < T; ++k) {
    memset(&tasks[k], 0, sizeof(hbo_task));
    tasks[k].x = (const char*)x + (size_t)rows * D * es; tasks[k].y = y0.data(); tasks[k].n = ns[k]; tasks[k].m = 1;
    rows += ns[k];
  }
  hbo_dataset* ds = nullptr;
  int rc = hbo_dataset_create(c, dtype, D, tasks.data(), T, &ds);
  if (rc) return rc;
  DevBuf buf;
  void* d_models = nullptr;
  // (the dataset leaves when the call does, behind a wait: launches may still read its pooled buffers.  Before buf's memory is freed.)
  struct DatasetGuard { hbo_ctx* c; hipStream_t st; hbo_dataset* ds; ~DatasetGuard() { hipStreamSynchronize(st); hbo_dataset_free(c, ds); } } guard = {c, st, ds};
  // the dataset holds its tasks largest first; its inputs lie in the caller's order: order[z] = the caller's index of dataset task z
  std::vector<TaskHost*> by_x(ds->tasks);
  std::sort(by_x.begin(), by_x.end(), [](TaskHost* a, TaskHost* b) { return (const char*)a->X < (const char*)b->X; });
  std::vector<int> order(T);
  for (int z = 0; z < T; ++z) order[z] = (int)(std::find(by_x.begin(), by_x.end(), ds->tasks[z]) - by_x.begin());
  size_t total = 0;
  for (int k = 0; k < T; ++k) { rows_out[k] = by_x[k]->npad; ld_out[k] = by_x[k]->ld; total += (size_t)by_x[k]->npad * by_x[k]->ld; }
  if ((size_t)out_cap < total) return fail(c, HBO_ERR_ARG, "hbo_probe_gram: out_cap is smaller than the padded buffers");
  const ModelDev* md = c->d_model;
  int model_stride = 0;
  std::vector<ModelDev> hm;
  if (n_models == 1) {
    rc = upload_model(c, m0);
    if (rc) return rc;
  } else {
    hm.resize(T);
    for (int z = 0; z < T; ++z) fill_model_dev(hm[z], &models[order[z]]);
    HIPCHK(c, buf.get(c, &d_models, sizeof(ModelDev) * T));
    HIPCHK(c, hipMemcpyAsync(d_models, hm.data(), sizeof(ModelDev) * T, hipMemcpyHostToDevice, st));
    md = static_cast<const ModelDev*>(d_models); model_stride = 1;
  }
  ds->h_desc.resize(T);
  std::vector<std::vector<unsigned char>> hs(T);
  for (int z = 0; z < T; ++z) {
    TaskHost* t = ds->tasks[z];
    rc = ensure_task_workspace(c, dtype, t, false, 1);
    if (rc) return rc;
    fill_desc(ds->h_desc[z], t, m0, dtype, OBJ_NLL);
    const size_t count = (size_t)(t->npad + HBO_TILE) * t->ld;   // all of A, its augmented tile row too
    fill(hs[z], count);
    HIPCHK(c, hipMemcpyAsync(t->A, hs[z].data(), count * es, hipMemcpyHostToDevice, st));
  }
  HIPCHK(c, dev_alloc(c, (void**)&ds->d_desc, sizeof(TaskDesc) * T));
  HIPCHK(c, hipMemcpyAsync(ds->d_desc, ds->h_desc.data(), sizeof(TaskDesc) * T, hipMemcpyHostToDevice, st));
  const int max_nblk = ds->max_nblk;
  GramArgs g = {}; g.kernel_id = m0->kernel_id; g.mfma_min_f = c->opt_gram_mfma; g.tasks = ds->d_desc; g.fdim = fdim; g.symmetric = 1; g.padded = 1;
  g.model_stride = model_stride;
  launch_gram(dtype, g, md, dim3(max_nblk, max_nblk, T), st);
  size_t off = 0;
  for (int k = 0; k < T; ++k) {
    const size_t count = (size_t)by_x[k]->npad * by_x[k]->ld;
    HIPCHK(c, hipMemcpyAsync((char*)out + off * es, by_x[k]->A, count * es, hipMemcpyDeviceToHost, st));
    off += count;
  }
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  return HBO_OK;
}

// Test hook (include/hbo_tune.h): the factor and inverse steps of an NLL evaluation with gradient on caller-chosen SPD matrices.  The
// batch is form 2's of hbo_probe_gram (dataset, workspaces, descriptors; one input column of zeros stands for x), A is filled as
// hbo_spd_solve fills it, and the steps are the objective's own: run_potrf with the InvRun of the plan, then obj_inverse_step
// (objective.hip).  Only the main stream is waited for before the copies back, as in the objective: a join that a schedule forgot shows.
extern "C" int hbo_probe_factor_inverse(hbo_ctx* c, int dtype, int32_t T, const int64_t* ns, const void* a, const void* b, int32_t m,
                                        int beside_chain, void* chol_out, void* w_out, void* kinv_out, void* x_out, void* z_out,
                                        int32_t* info_out, hbo_probe_plan* plan_out) {
  if (!c || !ns || !a) return fail(c, HBO_ERR_ARG, "hbo_probe_factor_inverse: null argument");
  if (dtype != HBO_F32 && dtype != HBO_F64) return fail(c, HBO_ERR_ARG, "hbo_probe_factor_inverse: bad dtype");
  if (T <= 0 || T > 64) return fail(c, HBO_ERR_ARG, "hbo_probe_factor_inverse: 1 <= T <= 64");
  for (int k = 0; k < T; ++k) if (ns[k] <= 0 || ns[k] > 4096) return fail(c, HBO_ERR_ARG, "hbo_probe_factor_inverse: need 1 <= n <= 4096 for every task");
  if (b ? (m < 1 || m > 8) : m != 0) return fail(c, HBO_ERR_ARG, "hbo_probe_factor_inverse: 1 <= m <= 8 with b, m = 0 without");
  if (!b && (x_out || z_out)) return fail(c, HBO_ERR_ARG, "hbo_probe_factor_inverse: x_out and z_out need b");
  if (beside_chain != 0 && beside_chain != 1) return fail(c, HBO_ERR_ARG, "hbo_probe_factor_inverse: beside_chain is 0 or 1");
  HIPCHK(c, hipSetDevice(c->device));
  prof_begin(c);
  const size_t es = esize(dtype);
  const int naug = b ? m : 1;   // (without right-hand sides: one augmented row of zeros)
  hipStream_t st = c->stream;
  // the dataset of the T tasks: one input column and naug target columns of zeros
  int64_t max_n = 0;
  std::vector<size_t> a_off(T), b_off(T);   // element offsets of task k in a / the [n, n] outputs, and in b / the [n, m] outputs
  size_t a_total = 0, b_total = 0;
  for (int k = 0; k < T; ++k) { a_off[k] = a_total; b_off[k] = b_total; a_total += (size_t)ns[k] * ns[k]; b_total += (size_t)ns[k] * m; max_n = std::max(max_n, ns[k]); }
  const std::vector<unsigned char> zeros((size_t)max_n * naug * es, 0);
  std::vector<hbo_task> tasks(T);
  int64_t rows = 0;
  std::vector<unsigned char> x0;
  for (int k = 0; k < T; ++k) rows += ns[k];
  x0.assign((size_t)rows * es, 0);
  rows = 0;
  for (int k = 0; k < T; ++k) {
    memset(&tasks[k], 0, sizeof(hbo_task));
    tasks[k].x = x0.data() + (size_t)rows * es; tasks[k].y = zeros.data(); tasks[k].n = ns[k]; tasks[k].m = naug;
    rows += ns[k];
  }
  hbo_dataset* ds = nullptr;
  int rc = hbo_dataset_create(c, dtype, 1, tasks.data(), T, &ds);
  if (rc) return rc;
  DevBuf buf;
  // (the dataset leaves when the call does, behind a wait: launches may still read its pooled buffers.  Before buf's memory is freed.)
  struct DatasetGuard { hbo_ctx* c; hipStream_t st; hbo_dataset* ds; ~DatasetGuard() { hipStreamSynchronize(st); hbo_dataset_free(c, ds); } } guard = {c, st, ds};
  // the dataset holds its tasks largest first; its inputs lie in the caller's order: order[z] = the caller's index of dataset task z
  std::vector<TaskHost*> by_x(ds->tasks);
  std::sort(by_x.begin(), by_x.end(), [](TaskHost* p, TaskHost* q) { return (const char*)p->X < (const char*)q->X; });
  std::vector<int> order(T);
  for (int z = 0; z < T; ++z) order[z] = (int)(std::find(by_x.begin(), by_x.end(), ds->tasks[z]) - by_x.begin());
  hbo_model model; memset(&model, 0, sizeof model);
  model.dtype = dtype; model.input_dim = 1;
  ds->h_desc.resize(T);
  for (int z = 0; z < T; ++z) {
    TaskHost* t = ds->tasks[z];
    rc = ensure_task_workspace(c, dtype, t, true, naug);
    if (rc) return rc;
    fill_desc(ds->h_desc[z], t, &model, dtype, ROLE_FACTOR);   // (naug = the task's m columns, as hbo_spd_solve sets it)
  }
  const int max_nblk = ds->max_nblk, max_npad = max_nblk * HBO_TILE;
  void *d_a = nullptr, *d_b = nullptr, *d_tmp = nullptr; int* d_info = nullptr;
  HIPCHK(c, dev_alloc(c, (void**)&ds->d_desc, sizeof(TaskDesc) * T));
  HIPCHK(c, buf.get(c, &d_info, sizeof(int) * T));
  HIPCHK(c, buf.get(c, &d_a, a_total * es));
  if (b) HIPCHK(c, buf.get(c, &d_b, b_total * es));
  if (chol_out) HIPCHK(c, buf.get(c, &d_tmp, a_total * es));
  HIPCHK(c, hipMemcpyAsync(ds->d_desc, ds->h_desc.data(), sizeof(TaskDesc) * T, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_info), INT_MAX, T, st));
  HIPCHK(c, hipMemcpyAsync(d_a, a, a_total * es, hipMemcpyHostToDevice, st));
  if (b) HIPCHK(c, hipMemcpyAsync(d_b, b, b_total * es, hipMemcpyHostToDevice, st));
  if (c->opt_poison) launch_poison(dtype, ds->d_desc, T, max_npad, st);
  for (int z = 0; z < T; ++z) {
    TaskHost* t = ds->tasks[z];
    const int k = order[z];
    launch_fill_spd(dtype, (const char*)d_a + a_off[k] * es, t->n, t->A, t->ld, t->npad, st);
    launch_set_aug(dtype, b ? (const char*)d_b + b_off[k] * es : nullptr, t->n, m, t->A, t->ld, t->npad, st);
  }
  // option spd_diag_bound: the largest max_i A_ii of the batch, as hbo_spd_solve takes it off its one matrix
  double diag_bound = 0;
  if (c->opt_spd_diag_bound) for (int k = 0; k < T; ++k) for (int64_t i = 0; i < ns[k]; ++i) diag_bound = std::max(diag_bound, host_elem(a, dtype, (int64_t)a_off[k] + i * ns[k] + i));
  CholBoundScope bound_scope(c, diag_bound);
  // the steps of an evaluation with gradient (objective.hip: step_factor without its Gram, step_reduce's fork, step_inverse)
  InvRun inv = {c, dtype, ds->d_desc, T, max_nblk, T == 1 ? &ds->h_desc[0] : nullptr, inv_plan(c, dtype, T, max_nblk, INV_W_KINV, T == 1, beside_chain != 0)};
  const PotrfPlan pp = potrf_plan(c, dtype, T, max_nblk, &inv.pl);
  if (plan_out) {
    *plan_out = {pp.la, pp.q, pp.q_inner, pp.early_at, pp.tgran, pp.split_f1, (int32_t)pp.yield,
                 inv.pl.sweep, inv.pl.qs, inv.pl.early, inv.pl.small_shape, inv.pl.batch_bg, inv.pl.d_own_stream};
  }
  { ProfScope ps(c, "potrf", 1); run_potrf(c, dtype, ds->d_desc, T, max_nblk, d_info, &inv); }
  hipStream_t side = obj_fork_side(c, pp.la);
  obj_inverse_step(c, inv, naug, side, -1);
  // the copies back, main stream only
  std::vector<int> h_info(T, INT_MAX);
  HIPCHK(c, hipMemcpyAsync(h_info.data(), d_info, sizeof(int) * T, hipMemcpyDeviceToHost, st));
  std::vector<unsigned char> xr, zr;
  for (int z = 0; z < T; ++z) {
    TaskHost* t = ds->tasks[z];
    const int k = order[z];
    const size_t n = (size_t)t->n, row_b = n * es, pitch = (size_t)t->ld * es;
    if (chol_out) {
      launch_extract_lower(dtype, t->A, t->ld, t->n, (char*)d_tmp + a_off[k] * es, st);
      HIPCHK(c, hipMemcpyAsync((char*)chol_out + a_off[k] * es, (char*)d_tmp + a_off[k] * es, n * n * es, hipMemcpyDeviceToHost, st));
    }
    if (w_out) HIPCHK(c, hipMemcpy2DAsync((char*)w_out + a_off[k] * es, row_b, t->W, pitch, row_b, n, hipMemcpyDeviceToHost, st));
    if (kinv_out) HIPCHK(c, hipMemcpy2DAsync((char*)kinv_out + a_off[k] * es, row_b, t->S, pitch, row_b, n, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(c, hipStreamSynchronize(st));
  for (int z = 0; z < T && b; ++z) {
    TaskHost* t = ds->tasks[z];
    const int k = order[z];
    if (x_out) {   // alpha: m rows of npad elements
      xr.resize((size_t)m * t->npad * es);
      HIPCHK(c, hipMemcpy(xr.data(), t->svec, xr.size(), hipMemcpyDeviceToHost));
      rows_to_cols((char*)x_out + b_off[k] * es, xr.data(), t->n, m, t->npad, es);
    }
    if (z_out) {   // the augmented rows of A: m rows of ld elements, repacked to npad
      zr.resize((size_t)m * t->npad * es);
      HIPCHK(c, hipMemcpy2D(zr.data(), (size_t)t->npad * es, (const char*)t->A + (size_t)t->npad * t->ld * es, (size_t)t->ld * es, (size_t)t->npad * es, (size_t)m,
                            hipMemcpyDeviceToHost));
      rows_to_cols((char*)z_out + b_off[k] * es, zr.data(), t->n, m, t->npad, es);
    }
  }
  HIPCHK(c, hipGetLastError());
  prof_collect(c);
  bool bad = false;
  for (int z = 0; z < T; ++z) {
    const int k = order[z];
    const bool bad_k = h_info[z] != INT_MAX;
    if (info_out) info_out[k] = bad_k ? h_info[z] : 0;
    if (!bad_k) continue;
    bad = true;
    const size_t nn = (size_t)ns[k] * ns[k], nm = (size_t)ns[k] * m;
    for (void* o : {chol_out, w_out, kinv_out}) if (o) fill_nan((char*)o + a_off[k] * es, nn, dtype);
    for (void* o : {x_out, z_out}) if (o) fill_nan((char*)o + b_off[k] * es, nm, dtype);
  }
  return bad ? HBO_NOT_PD : HBO_OK;
}

// Test hook (include/hbo_tune.h): the element-wise Kumaraswamy kernels of kumar.hip on caller-chosen rows -- launch_kumar_forward in its
// gradient form (h != nullptr: w, dw/da, dw/db) and launch_kumar_chain_dx with gf = 1 in every element (dw/dx), nothing else.
extern "C" int hbo_probe_kumar_warp(hbo_ctx* c, const hbo_model* m, const void* x, int64_t n, void* w_out, double* dwda_out, double* dwdb_out,
                                    double* dwdx_out) {
  if (!c || !m || !x || !w_out || !dwda_out || !dwdb_out || !dwdx_out) return fail(c, HBO_ERR_ARG, "hbo_probe_kumar_warp: null argument");
  if (!is_kumar(m)) return fail(c, HBO_ERR_ARG, "hbo_probe_kumar_warp: the model has no Kumaraswamy input warp");
  if (n <= 0 || n > (1 << 20)) return fail(c, HBO_ERR_ARG, "hbo_probe_kumar_warp: need 1 <= n <= 2^20");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = upload_model(c, m);
  if (rc) return rc;
  const int dtype = m->dtype, D = m->input_dim;
  const size_t es = esize(dtype), cnt = (size_t)n * D;
  hipStream_t st = c->stream;
  DevBuf buf;
  void *d_x = nullptr, *d_w = nullptr; double *d_h = nullptr, *d_gf = nullptr, *d_gx = nullptr;
  HIPCHK(c, buf.get(c, &d_x, cnt * es)); HIPCHK(c, buf.get(c, &d_w, cnt * es));
  HIPCHK(c, buf.get(c, &d_h, 2 * cnt * sizeof(double))); HIPCHK(c, buf.get(c, &d_gf, cnt * sizeof(double))); HIPCHK(c, buf.get(c, &d_gx, cnt * sizeof(double)));
  const std::vector<double> ones(cnt, 1.0);
  HIPCHK(c, hipMemcpyAsync(d_x, x, cnt * es, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_gf, ones.data(), cnt * sizeof(double), hipMemcpyHostToDevice, st));
  launch_kumar_forward(dtype, nullptr, 0, 0, d_x, d_w, d_h, n, D, c->d_model, st);
  launch_kumar_chain_dx(dtype, d_x, n, D, c->d_model, d_gf, d_gx, st);
  HIPCHK(c, hipMemcpyAsync(w_out, d_w, cnt * es, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(dwda_out, d_h, cnt * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(dwdb_out, d_h + cnt, cnt * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(dwdx_out, d_gx, cnt * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  return HBO_OK;
}

// Test hook (include/hbo_tune.h): the gradient contraction of an evaluation on a caller-chosen G.  The batch is form 2's of hbo_probe_gram
// (dataset, workspaces, descriptors from the set-up of an evaluation with gradient of `obj`, the MLP activations and dF as obj_setup
// allocates them; sizes from obj_plan), poisoned first where the option says so.  Then the operands go where step_inverse and
// step_extra_rows would have left them -- S (K^-1), the outer-product vectors where outer_vecs finds them (svec rows; EUC: the augmented
// tile row of A), d f / d mu -- and the shipped launches run in objective.hip's order with its arguments: launch_grad_contract,
// launch_grad_finalize with `pre` behind the partials, and for an MLP kernel launch_grad_feat (+ launch_scale_dF for EUC) on a zeroed dF.
// Padding: everything beyond a task's n rows / columns and every 128-tile of S strictly above the tile diagonal holds the sentinel; the
// kernels mask by row < n && col < n and rely on no zero the pipeline writes there.  One exception, said here: an EKL task carries
// naug = m + 1 >= 2 vectors, so nvec = 1 is given as m = 1 with a second vector of zeros in its n data elements (0 * 0 added to the outer
// product; its padding holds the sentinel as well).  Partials, the gradient block and `pre` are preset to NaN: a slot no launch wrote shows.
extern "C" int hbo_probe_grad_contract(hbo_ctx* c, const hbo_model* m, int obj, int32_t T, const int64_t* ns, const void* x, const void* s,
                                       const void* vecs, int32_t nvec, const double* coef_lh, const double* coef_c, const double* dmu,
                                       double sentinel, double* grad_out, double* partials_out, double* fro_out, double* dF_out,
                                       int32_t* prereduced_out) {
  if (!c || !m || !ns || !x || !vecs || !coef_lh || !coef_c) return fail(c, HBO_ERR_ARG, "hbo_probe_grad_contract: null argument");
  if (obj != OBJ_NLL && obj != OBJ_EKL && obj != OBJ_EUC) return fail(c, HBO_ERR_ARG, "hbo_probe_grad_contract: obj is 0 (NLL), 1 (EKL) or 2 (EUC)");
  if (T <= 0 || T > 64) return fail(c, HBO_ERR_ARG, "hbo_probe_grad_contract: 1 <= T <= 64");
  for (int k = 0; k < T; ++k) if (ns[k] <= 0 || ns[k] > 4096) return fail(c, HBO_ERR_ARG, "hbo_probe_grad_contract: need 1 <= n <= 4096 for every task");
  if (obj == OBJ_NLL ? nvec != 1 : (nvec < 1 || nvec > 9)) return fail(c, HBO_ERR_ARG, "hbo_probe_grad_contract: nvec is 1 for NLL, 1..9 otherwise");
  if (obj != OBJ_EUC && !s) return fail(c, HBO_ERR_ARG, "hbo_probe_grad_contract: NLL and EKL need s");
  if (m->input_warp != HBO_WARP_NONE) return fail(c, HBO_ERR_ARG, "hbo_probe_grad_contract: models with an input warp are not taken");
  if (validate_model(c, m)) return HBO_ERR_ARG;
  if (needs_mlp(m) && !m->kernel_uses_mlp) return fail(c, HBO_ERR_ARG, "hbo_probe_grad_contract: a linear_mlp mean is taken with an MLP kernel only");
  if (m->kernel_uses_mlp && m->mean_id == HBO_MEAN_LINEAR) return fail(c, HBO_ERR_ARG, "hbo_probe_grad_contract: an MLP kernel is taken with a zero, constant or linear_mlp mean");
  if (fro_out && obj != OBJ_EUC) return fail(c, HBO_ERR_ARG, "hbo_probe_grad_contract: fro_out needs EUC");
  if (dF_out && !m->kernel_uses_mlp) return fail(c, HBO_ERR_ARG, "hbo_probe_grad_contract: dF_out needs an MLP kernel");
  HIPCHK(c, hipSetDevice(c->device));
  const int dtype = m->dtype, D = m->input_dim, fdim = feature_dim(m);
  const bool euc = obj == OBJ_EUC, mlp = m->kernel_uses_mlp != 0;
  const size_t es = esize(dtype);
  const int mcols = obj == OBJ_NLL ? 1 : (euc ? nvec : std::max(nvec - 1, 1));   // target columns: NLL 1 vector, EUC naug - 1 = m, EKL naug = m + 1
  hipStream_t st = c->stream;
  auto fill = [&](std::vector<unsigned char>& h, size_t count) {
    h.resize(count * es);
    if (dtype == HBO_F64) for (size_t i = 0; i < count; ++i) ((double*)h.data())[i] = sentinel;
    else for (size_t i = 0; i < count; ++i) ((float*)h.data())[i] = (float)sentinel;
  };
  // the dataset of the T tasks: targets of zeros; an MLP kernel reads x as its features F, its raw inputs are zeros
  int64_t max_n = 0, rows = 0;
  std::vector<size_t> r_off(T), a_off(T);   // first row of task k in x / dmu / dF; first element in s
  size_t a_total = 0;
  for (int k = 0; k < T; ++k) { r_off[k] = (size_t)rows; a_off[k] = a_total; rows += ns[k]; a_total += (size_t)ns[k] * ns[k]; max_n = std::max(max_n, ns[k]); }
  const std::vector<unsigned char> y0((size_t)max_n * mcols * es, 0), x0(mlp ? (size_t)max_n * D * es : 0, 0);
  std::vector<hbo_task> tasks(T);
  for (int k = 0; k < T; ++k) {
    memset(&tasks[k], 0, sizeof(hbo_task));
    tasks[k].x = mlp ? (const void*)x0.data() : (const void*)((const char*)x + r_off[k] * D * es);
    tasks[k].y = y0.data(); tasks[k].n = ns[k]; tasks[k].m = mcols;
  }
  hbo_dataset* ds = nullptr;
  int rc = hbo_dataset_create(c, dtype, D, tasks.data(), T, &ds);
  if (rc) return rc;
  DevBuf buf;
  // (the dataset leaves when the call does, behind a wait: launches may still read its pooled buffers.  Before buf's memory is freed.)
  struct DatasetGuard { hbo_ctx* c; hipStream_t st; hbo_dataset* ds; ~DatasetGuard() { hipStreamSynchronize(st); hbo_dataset_free(c, ds); } } guard = {c, st, ds};
  // the dataset holds its tasks largest first; its inputs lie in the caller's order: order[z] = the caller's index of dataset task z
  std::vector<TaskHost*> by_x(ds->tasks);
  std::sort(by_x.begin(), by_x.end(), [](TaskHost* p, TaskHost* q) { return (const char*)p->X < (const char*)q->X; });
  std::vector<int> order(T);
  for (int z = 0; z < T; ++z) order[z] = (int)(std::find(by_x.begin(), by_x.end(), ds->tasks[z]) - by_x.begin());
  rc = upload_model(c, m);
  if (rc) return rc;
  hbo_grad_layout lay; memset(&lay, 0, sizeof lay);
  const ObjPlan p = obj_plan(c, m, ds, lay, obj, true, false);
  const int max_nblk = ds->max_nblk, max_npad = max_nblk * HBO_TILE, nacc = p.nacc, out_stride = p.out_stride;
  ds->h_desc.resize(T);
  for (int z = 0; z < T; ++z) {
    TaskHost* t = ds->tasks[z];
    rc = ensure_task_workspace(c, dtype, t, p.need_S, obj == OBJ_NLL ? 1 : t->m + 1);
    if (rc) return rc;
    if (mlp) {
      rc = t->feat.ensure(c, m, t->n);
      if (rc) return rc;
      int maxf = m->input_dim;
      for (int l = 0; l < m->n_layers; ++l) maxf = std::max(maxf, (int)m->features[l]);
      const size_t need = (size_t)t->n * maxf;
      HIPCHK(c, dev_alloc(c, (void**)&t->dF, need * sizeof(double)));
      HIPCHK(c, dev_alloc(c, (void**)&t->dtmp, need * sizeof(double)));
      t->dF_elems = need;
    }
    fill_desc(ds->h_desc[z], t, m, dtype, obj);
    ds->h_desc[z].coef_lh = coef_lh[order[z]]; ds->h_desc[z].coef_c = coef_c[order[z]];   // the caller's, where fill_desc put the objective's
  }
  // partials + their pre-reduction, placed as obj_plan sizes them (also for a one-block NLL batch, which the product sends to small.hip)
  const size_t part_elems = (size_t)p.stride_task * T, pre_elems = (size_t)HBO_GRAD_PRE_ROWS * nacc * T;
  double *d_part = nullptr, *d_out = nullptr, *d_val = nullptr;
  HIPCHK(c, dev_alloc(c, (void**)&ds->d_desc, sizeof(TaskDesc) * T));
  HIPCHK(c, buf.get(c, &d_part, (part_elems + pre_elems) * sizeof(double)));
  HIPCHK(c, buf.get(c, &d_out, (size_t)T * out_stride * sizeof(double)));
  HIPCHK(c, buf.get(c, &d_val, (size_t)T * sizeof(double)));
  HIPCHK(c, hipMemcpyAsync(ds->d_desc, ds->h_desc.data(), sizeof(TaskDesc) * T, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(d_part, 0xFF, (part_elems + pre_elems) * sizeof(double), st));
  HIPCHK(c, hipMemsetAsync(d_out, 0xFF, (size_t)T * out_stride * sizeof(double), st));
  HIPCHK(c, hipMemsetAsync(d_val, 0xFF, (size_t)T * sizeof(double), st));
  if (c->opt_poison) launch_poison(dtype, ds->d_desc, T, max_npad, st);
  // the operands, padded with the sentinel (the staging buffers live until the wait below)
  std::vector<std::vector<unsigned char>> hS(T), hV(T);
  std::vector<std::vector<double>> hM(T);
  size_t v_off = 0;
  std::vector<size_t> v_offs(T);
  for (int k = 0; k < T; ++k) { v_offs[k] = v_off; v_off += (size_t)nvec * ns[k]; }
  for (int z = 0; z < T; ++z) {
    TaskHost* t = ds->tasks[z];
    const int k = order[z];
    const size_t n = (size_t)t->n, npad = (size_t)t->npad, ld = (size_t)t->ld;
    if (!euc) {
      fill(hS[z], npad * ld);
      const char* sk = (const char*)s + a_off[k] * es;
      for (size_t i = 0; i < n; ++i) {
        const size_t cols = std::min(n, (i / HBO_TILE + 1) * HBO_TILE);   // up to the end of the row's diagonal tile
        memcpy(hS[z].data() + i * ld * es, sk + i * n * es, cols * es);
      }
      HIPCHK(c, hipMemcpyAsync(t->S, hS[z].data(), npad * ld * es, hipMemcpyHostToDevice, st));
    }
    const char* vk = (const char*)vecs + v_offs[k] * es;
    if (euc) {   // rows npad ... of A, ld apart
      fill(hV[z], (size_t)HBO_TILE * ld);
      for (int b = 0; b < nvec; ++b) memcpy(hV[z].data() + (size_t)b * ld * es, vk + (size_t)b * n * es, n * es);
      HIPCHK(c, hipMemcpyAsync((char*)t->A + npad * ld * es, hV[z].data(), (size_t)HBO_TILE * ld * es, hipMemcpyHostToDevice, st));
    } else {     // svec: naug rows of npad
      const int ncol = ds->h_desc[z].naug;
      fill(hV[z], (size_t)ncol * npad);
      for (int b = 0; b < ncol; ++b) {
        if (b < nvec) memcpy(hV[z].data() + (size_t)b * npad * es, vk + (size_t)b * n * es, n * es);
        else memset(hV[z].data() + (size_t)b * npad * es, 0, n * es);
      }
      HIPCHK(c, hipMemcpyAsync(t->svec, hV[z].data(), (size_t)ncol * npad * es, hipMemcpyHostToDevice, st));
    }
    hM[z].assign(npad, sentinel);
    for (size_t i = 0; i < n; ++i) hM[z][i] = dmu ? dmu[r_off[k] + i] : 0.0;
    HIPCHK(c, hipMemcpyAsync(t->dmu, hM[z].data(), npad * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(t->fnorm, 0, 2 * sizeof(double), st));
    if (mlp) {
      HIPCHK(c, hipMemcpyAsync(t->feat.acts[m->n_layers - 1], (const char*)x + r_off[k] * fdim * es, n * fdim * es, hipMemcpyHostToDevice, st));
      HIPCHK(c, hipMemsetAsync(t->dF, 0, n * fdim * sizeof(double), st));
    }
  }
  // the launches of step_contract and enqueue_backward (objective.hip)
  launch_grad_contract(dtype, ds->d_desc, T, max_nblk, c->d_model, m->kernel_id, p.fdim, obj, d_part, p.stride_task, st);
  launch_grad_finalize(dtype, ds->d_desc, T, c->d_model, m->kernel_id, p.fdim, obj, d_part, p.stride_task, d_out, out_stride, euc ? d_val : nullptr, st,
                       d_part + p.stride_task * T, max_nblk);
  if (mlp) {
    launch_grad_feat(dtype, ds->d_desc, T, max_nblk, c->d_model, m->kernel_id, fdim, obj, st);
    if (euc) launch_scale_dF(ds->d_desc, T, (int64_t)max_npad, fdim, st);
  }
  // the copies back, in the caller's order
  std::vector<double> h_out((size_t)T * out_stride), h_fro(T, 0.0);
  double pre0 = 0;
  HIPCHK(c, hipMemcpyAsync(h_out.data(), d_out, h_out.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(&pre0, d_part + part_elems, sizeof(double), hipMemcpyDeviceToHost, st));
  std::vector<size_t> p_off(T);
  size_t p_total = 0;
  for (int k = 0; k < T; ++k) { p_off[k] = p_total; p_total += (size_t)by_x[k]->nblk * (by_x[k]->nblk + 1) * nacc; }
  for (int z = 0; z < T; ++z) {
    TaskHost* t = ds->tasks[z];
    const int k = order[z];
    if (partials_out) HIPCHK(c, hipMemcpyAsync(partials_out + p_off[k], d_part + (size_t)z * p.stride_task, (size_t)t->nblk * (t->nblk + 1) * nacc * sizeof(double), hipMemcpyDeviceToHost, st));
    if (fro_out) HIPCHK(c, hipMemcpyAsync(&h_fro[k], t->fnorm, sizeof(double), hipMemcpyDeviceToHost, st));
    if (dF_out) HIPCHK(c, hipMemcpyAsync(dF_out + r_off[k] * fdim, t->dF, (size_t)t->n * fdim * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  for (int z = 0; z < T && grad_out; ++z) memcpy(grad_out + (size_t)order[z] * out_stride, h_out.data() + (size_t)z * out_stride, out_stride * sizeof(double));
  if (fro_out) memcpy(fro_out, h_fro.data(), T * sizeof(double));
  if (prereduced_out) *prereduced_out = pre0 == pre0 ? 1 : 0;   // `pre` was preset to NaN: its first slot holds a number once grad_prereduce_kernel ran
  return HBO_OK;
}
