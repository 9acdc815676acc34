// hbo_nll_samples: the value-only Cholesky NLL of S hyper-parameter samples of one model family over every task of a resident
// dataset, as one batch of S x T (sample, task) pairs -- the log density a slice sampler over the hyper-parameters calls thousands
// of times (hyperbo/bo_utils/bayesopt.py:247-255, gp_utils/slice_sampling_test.py:56-153 ask for config['method'] =
// 'slice_sample'; the chains' pending evaluations of one lockstep round are one call here instead of one hbo_nll each).
//
//   fused path (every task n <= 128): ONE launch of small_eval_kernel over S x T workgroups, sample-major, workgroup b reading the
//     model of sample b / T; value only (no gradient, nothing written back).  An MLP basis / linear_mlp mean: the features of all
//     pairs from one launch per layer, each pair with its sample's weights (launch_mlp_forward_batch, model_weights).  A pair's value
//     is computed by its own workgroup from its own inputs: it does not depend on which other samples share the call (bit for bit).
//   blocked path (any task > 128): S x T descriptors, task-major (the largest tasks first, as the dataset holds them), one ModelDev
//     per descriptor (GramArgs::model_stride, launch_aug_rows), Gram -> potrf with the augmented row (log-det and |z|^2 come out of
//     the factorisation) -> the NLL reduction.  No inverse, no K^-1: one matrix per pair (the leaf inverses the panel solve needs
//     live in the matrix's own unused upper block triangle, see below).  Samples go in chunks that fit half the free device memory.
// No float atomics: every task value comes from one workgroup, the sum over tasks is taken on the host in the dataset's order --
// the order hbo_nll sums in -- so identical calls are bit-identical.
#include "api_internal.h"

namespace {
static_assert(sizeof(ModelDev) % sizeof(uint64_t) == 0, "ModelDev is copied as 64-bit words");
// dst[p] = src[p % S]: the model of every (task, sample) descriptor of the task-major blocked batch
__global__ void expand_models_kernel(const ModelDev* __restrict__ src, ModelDev* __restrict__ dst, int S) {
  constexpr int NW = (int)(sizeof(ModelDev) / sizeof(uint64_t));
  const uint64_t* s = reinterpret_cast<const uint64_t*>(src + blockIdx.x % S);
  uint64_t* d = reinterpret_cast<uint64_t*>(dst + blockIdx.x);
  for (int i = threadIdx.x; i < NW; i += blockDim.x) d[i] = s[i];
}
}  // namespace

extern "C" int hbo_nll_samples(hbo_ctx* c, const hbo_model* models, int32_t S, hbo_dataset* ds, double* nll_sum,
                               double* nll_per_task) {
  if (!c || !models || !ds || !nll_sum) return fail(c, HBO_ERR_ARG, "hbo_nll_samples: null argument");
  if (S <= 0 || S > 4096) return fail(c, HBO_ERR_ARG, "hbo_nll_samples: 1 <= S <= 4096");
  if (int rc = model_family_check(c, "hbo_nll_samples: ", models, S, "evaluate them with hbo_nll")) return rc;
  const hbo_model* m0 = &models[0];
  const int T = ds->ntasks;
  if (T > 0 && (m0->dtype != ds->dtype || m0->input_dim != ds->D)) return fail(c, HBO_ERR_ARG, "hbo_nll_samples: model/dataset dtype or input_dim mismatch");
  for (int s = 0; s < S; ++s) nll_sum[s] = 0;
  if (T == 0) return HBO_OK;
  HIPCHK(c, hipSetDevice(c->device));
  prof_begin(c);
  const int dtype = ds->dtype;
  const size_t es = esize(dtype);
  hipStream_t st = c->stream;
  const bool mlp = needs_mlp(m0);
  const MlpShape sh = mlp_shape(m0);
  const int L = sh.L;
  const int fdim = feature_dim(m0);
  const int max_nblk = ds->max_nblk, max_npad = max_nblk * HBO_TILE;
  int64_t max_n = 0;
  for (TaskHost* t : ds->tasks) max_n = std::max<int64_t>(max_n, t->n);
  const bool fused = c->opt_small_fused && max_nblk == 1 && small_eval_lds(dtype) <= c->lds_per_block;

  // ---- the S models and their MLP weights: one upload each for the whole call
  ModelDev* d_models = static_cast<ModelDev*>(ws_get(c, WS_NS_MODELS, sizeof(ModelDev) * S));
  if (!d_models) return HBO_ERR_HIP;
  std::vector<ModelDev> h_models(S);
  for (int s = 0; s < S; ++s) fill_model_dev(h_models[s], &models[s]);
  HIPCHK(c, hipMemcpyAsync(d_models, h_models.data(), sizeof(ModelDev) * S, hipMemcpyHostToDevice, st));
  // layer-major, as launch_mlp_forward_batch indexes them -- layer l: [S][fin][fout] weights, then [S][fout] biases
  std::vector<size_t> woff(L), boff(L);
  std::vector<unsigned char> h_w;
  char* d_wblk = nullptr;
  if (mlp) {
    BlockLayout lay;
    for (int l = 0; l < L; ++l) { woff[l] = lay.take(sh.wb[l] * S); boff[l] = lay.take(sh.bb[l] * S); }
    h_w.assign(lay.off, 0);
    for (int s = 0; s < S; ++s)
      for (int l = 0; l < L; ++l) {
        memcpy(h_w.data() + woff[l] + sh.wb[l] * s, models[s].mlp_kernel[l], sh.wb[l]);
        memcpy(h_w.data() + boff[l] + sh.bb[l] * s, models[s].mlp_bias[l], sh.bb[l]);
      }
    d_wblk = static_cast<char*>(ws_get(c, WS_NS_MLP_W, lay.off));
    if (!d_wblk) return HBO_ERR_HIP;
    HIPCHK(c, hipMemcpyAsync(d_wblk, h_w.data(), lay.off, hipMemcpyHostToDevice, st));
  }
  size_t act_pair = 0;   // bytes of one pair's activations, all layers
  if (mlp) for (int l = 0; l < L; ++l) act_pair += align256((size_t)std::max<int64_t>(max_n, 1) * m0->features[l] * es);
  // blocked path: one matrix per pair, (npad + 256) rows x ld: W = rows [0, npad), A = rows [128, npad + 256).  The panel solve
  // reads the leaf inverses potf2 stores at W's diagonal blocks; with this offset W's block (p, p) is A's block (p - 1, p), strictly
  // above the diagonal, which neither the Gram build (lower tiles), the factorisation nor the reduction touch -- and block 0 lands in
  // the 128 rows in front of A.
  std::vector<size_t> mat_bytes(T, 0);
  size_t mat_sample = 0;
  if (!fused)
    for (int k = 0; k < T; ++k) { const TaskHost* t = ds->tasks[k]; mat_bytes[k] = align256((size_t)(t->npad + 2 * HBO_TILE) * t->ld * es); mat_sample += mat_bytes[k]; }
  int chunk = S;
  if (!fused) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)16 << 30; }
    const size_t per = mat_sample + act_pair * T + sizeof(TaskDesc) * T + sizeof(ModelDev) * T;
    chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)S, (free_b / 2) / std::max<size_t>(per, 1)));
  }
  void* small_scratch = nullptr;
  if (fused) {   // every workgroup writes its leaf inverses there (leaf_cholesky4): never read
    small_scratch = ws_get(c, WS_SMALL_W, (size_t)HBO_TILE * padded_ld(HBO_TILE, dtype) * es);
    if (!small_scratch) return HBO_ERR_HIP;
  }

  std::vector<double> h_nll((size_t)S * T);
  std::vector<int> h_info((size_t)S * T);
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int sc = std::min(chunk, S - s0);
    const int P = sc * T;
    auto pair = [&](int s, int k) { return fused ? s * T + k : k * sc + s; };
    TaskDesc* d_desc = static_cast<TaskDesc*>(ws_get(c, WS_NS_DESC, sizeof(TaskDesc) * P));
    char* d_pack = static_cast<char*>(ws_get(c, WS_NS_PACK, (sizeof(double) + sizeof(int)) * P));
    char* d_mat = fused ? nullptr : static_cast<char*>(ws_get(c, WS_NS_MAT, mat_sample * sc));
    char* d_acts = mlp ? static_cast<char*>(ws_get(c, WS_NS_ACTS, act_pair * P)) : nullptr;
    MlpTaskDev* d_mlpt = mlp ? static_cast<MlpTaskDev*>(ws_get(c, WS_NS_MLPT, sizeof(MlpTaskDev) * P)) : nullptr;
    if (!d_desc || !d_pack || (!fused && !d_mat) || (mlp && (!d_acts || !d_mlpt))) return HBO_ERR_HIP;
    double* d_nll = reinterpret_cast<double*>(d_pack);
    int* d_info = reinterpret_cast<int*>(d_pack + sizeof(double) * P);
    std::vector<TaskDesc> hd(P);
    std::vector<MlpTaskDev> hm(mlp ? P : 0);
    size_t mat_off = 0;
    for (int k = 0; k < T; ++k) {
      TaskHost* t = ds->tasks[k];
      for (int s = 0; s < sc; ++s) {
        const int p = pair(s, k);
        TaskDesc& d = hd[p];
        fill_desc(d, t, &models[s0 + s], dtype, OBJ_NLL);
        d.A = d.W = d.S = d.wscr = d.svec = d.dF = nullptr; d.dmu = nullptr; d.fnorm = nullptr; d.kh = nullptr;
        if (fused) {
          d.W = small_scratch;
        } else {
          char* base = d_mat + mat_off + mat_bytes[k] * s;
          d.W = base; d.A = base + (size_t)HBO_TILE * t->ld * es;
        }
        if (mlp) {
          MlpTaskDev& mt = hm[p];
          memset(&mt, 0, sizeof mt);
          mt.x = t->X; mt.n = t->n; mt.model = s;
          char* a = d_acts + act_pair * p;
          for (int l = 0; l < L; ++l) { mt.acts[l] = a; a += align256((size_t)std::max<int64_t>(max_n, 1) * m0->features[l] * es); }
          const void* last = mt.acts[L - 1];
          d.F = m0->kernel_uses_mlp ? last : t->X;
          d.Fm = m0->mean_id == HBO_MEAN_LINEAR_MLP ? last : d.Fm;
        }
      }
      if (!fused) mat_off += mat_bytes[k] * sc;
    }
    HIPCHK(c, hipMemcpyAsync(d_desc, hd.data(), sizeof(TaskDesc) * P, hipMemcpyHostToDevice, st));
    if (mlp) {
      HIPCHK(c, hipMemcpyAsync(d_mlpt, hm.data(), sizeof(MlpTaskDev) * P, hipMemcpyHostToDevice, st));
      ProfScope ps(c, "features", 1);
      for (int l = 0; l < L; ++l)
        launch_mlp_forward_batch(dtype, d_mlpt, P, max_n, l, d_wblk + woff[l] + sh.wb[l] * s0, d_wblk + boff[l] + sh.bb[l] * s0, sh.fin[l],
                                 sh.fout[l], st, 1);
    }
    if (fused) {
      ProfScope ps(c, "small_eval", 1);
      launch_small_eval(dtype, d_desc, P, d_models + s0, m0->kernel_id, fdim, d_info, d_nll, nullptr, 0, 0, st, T);
    } else {
      ModelDev* d_mx = static_cast<ModelDev*>(ws_get(c, WS_NS_MODELS_X, sizeof(ModelDev) * P));
      if (!d_mx) return HBO_ERR_HIP;
      HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_info), INT_MAX, P, st));
      if (c->opt_poison) launch_poison(dtype, d_desc, P, max_npad, st);
      { ProfScope ps(c, "aug_rows", 1);
        hipLaunchKernelGGL(expand_models_kernel, dim3(P), dim3(256), 0, st, d_models + s0, d_mx, sc);
        launch_aug_rows(dtype, d_desc, P, max_npad, d_mx, st, 1); }
      { ProfScope ps(c, "gram", 1);
        GramArgs g = {}; g.kernel_id = m0->kernel_id; g.mfma_min_f = c->opt_gram_mfma; g.tasks = d_desc; g.fdim = fdim; g.symmetric = 1; g.padded = 1; g.model_stride = 1;
        launch_gram(dtype, g, d_mx, dim3(max_nblk, max_nblk, P), st); }
      CholBoundScope bound_scope(c, chol_diag_bound_of(models + s0, sc));
      { ProfScope ps(c, "potrf", 1); run_potrf(c, dtype, d_desc, P, max_nblk, d_info); }
      { ProfScope ps(c, "nll_reduce", 1); launch_nll_reduce(dtype, d_desc, P, d_info, d_nll, st); }
    }
    unsigned char* stage = static_cast<unsigned char*>(pinned_stage(c, (sizeof(double) + sizeof(int)) * P));
    if (!stage) return fail(c, HBO_ERR_HIP, "hbo_nll_samples: pinned staging buffer");
    HIPCHK(c, hipMemcpyAsync(stage, d_pack, (sizeof(double) + sizeof(int)) * P, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    const double* s_nll = reinterpret_cast<const double*>(stage);
    const int* s_info = reinterpret_cast<const int*>(stage + sizeof(double) * P);
    for (int s = 0; s < sc; ++s)
      for (int k = 0; k < T; ++k) { h_nll[(size_t)(s0 + s) * T + k] = s_nll[pair(s, k)]; h_info[(size_t)(s0 + s) * T + k] = s_info[pair(s, k)]; }
  }
  prof_collect(c);
  // per sample: the sum over tasks in the dataset's order, as hbo_nll takes it
  bool notpd = false;
  for (int s = 0; s < S; ++s) {
    double total = 0;
    for (int k = 0; k < T; ++k) {
      const size_t i = (size_t)s * T + k;
      total += h_nll[i];
      if (h_info[i] != INT_MAX) notpd = true;
      if (nll_per_task) nll_per_task[i] = h_nll[i];
    }
    nll_sum[s] = total;
  }
  return notpd ? HBO_NOT_PD : HBO_OK;
}
