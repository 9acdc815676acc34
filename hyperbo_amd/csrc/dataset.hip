// Datasets of the C ABI (include/hbo.h): hbo_dataset_create from host arrays, hbo_dataset_subsample on the device (the row gather that
// hbo_train_adam reuses, train.hip) and hbo_dataset_free.  Both builders lay all inputs of all tasks out in ONE block (dataset_place) and
// leave the tasks largest first (dataset_finish); those steps and the host statistics of a task are dataset_host.h's.
#include "dataset_host.h"

extern "C" int hbo_dataset_free(hbo_ctx* c, hbo_dataset* ds) {
  if (!ds) return HBO_OK;
  if (c) hipSetDevice(c->device);
  // (the buffers go back to the pool while kernels of the last evaluation may still run only if a call returned without
  //  draining its streams -- none does: every entry point synchronises before it returns)
  for (TaskHost* t : ds->tasks) free_task(c, t);
  dev_free(c, ds->d_inputs);
  dev_free(c, ds->d_svec);
  for (void* p : {(void*)ds->d_desc, (void*)ds->d_pack, (void*)ds->d_partials, (void*)ds->d_mlpgrad, (void*)ds->d_mlp}) dev_free(c, p);
  delete ds;
  return HBO_OK;
}

extern "C" int hbo_dataset_create(hbo_ctx* c, int dtype, int input_dim, const hbo_task* tasks, int n_tasks, hbo_dataset** out) {
  if (!c || !out || (n_tasks > 0 && !tasks)) return fail(c, HBO_ERR_ARG, "hbo_dataset_create: null argument");
  if (dtype != HBO_F32 && dtype != HBO_F64) return fail(c, HBO_ERR_ARG, "hbo_dataset_create: bad dtype");
  if (input_dim <= 0 || input_dim > HBO_MAX_FEATURE_DIM) return fail(c, HBO_ERR_ARG, "hbo_dataset_create: bad input_dim");
  HIPCHK(c, hipSetDevice(c->device));
  hbo_dataset* ds = new hbo_dataset();
  ds->dtype = dtype; ds->D = input_dim;
  const size_t es = esize(dtype);
  // All inputs of all tasks travel in ONE block: laid out in a pinned staging buffer (x, the column sums of y, the
  // divergence rows), one host-to-device copy, the tasks point into the block.  (Three synchronous copies per task cost
  // ~1 ms for 24 small tasks -- what an Adam step of GP.train() pays when it re-samples its batch, gp.py:101-111.)
  std::vector<TaskOff> offs(std::max(n_tasks, 0));   // (n_tasks <= 0: an empty dataset)
  BlockLayout lay;
  for (int k = 0; k < n_tasks; ++k) {
    const hbo_task& tk = tasks[k];
    if (tk.n <= 0) continue;  // objectives.py:184-185: empty sub-datasets are skipped
    if (tk.m <= 0 || !tk.x || !tk.y) { hbo_dataset_free(c, ds); return fail(c, HBO_ERR_ARG, "hbo_dataset_create: bad task"); }
    offs[k] = dataset_place(lay, tk.n, input_dim, tk.m, true, es);
  }
  const size_t total = lay.off;
  unsigned char* stage = nullptr;
  if (total) {
    stage = static_cast<unsigned char*>(stage_begin(c, "hbo_dataset_create: ", total));
    hipError_t e = stage ? dev_alloc(c, &ds->d_inputs, total) : hipErrorOutOfMemory;
    if (e != hipSuccess) { hbo_dataset_free(c, ds); return fail(c, HBO_ERR_HIP, std::string("hbo_dataset_create: ") + hipGetErrorString(e)); }
  }
  for (int k = 0; k < n_tasks; ++k) {
    const hbo_task& tk = tasks[k];
    if (tk.n <= 0) continue;
    dataset_add_task(ds, tk.n, tk.m, offs[k], true);
    memcpy(stage + offs[k].x, tk.x, (size_t)tk.n * input_dim * es);
    task_stats(tk.y, tk.n, tk.m, dtype, stage + offs[k].ysum, stage + offs[k].ydiv);
  }
  if (total) {
    hipError_t e = stage_upload(c, ds->d_inputs, stage, total, c->stream);
    if (e != hipSuccess) { hbo_dataset_free(c, ds); return fail(c, HBO_ERR_HIP, std::string("hbo_dataset_create: ") + hipGetErrorString(e)); }
  }
  dataset_finish(ds);
  *out = ds;
  return HBO_OK;
}

namespace {
// row r of task blockIdx.y of the sub-sample = row idx[idx_off + r] (or r) of the resident task: inputs, column sum of y, divergence rows
template <typename T>
__global__ __launch_bounds__(256) void gather_rows_kernel(const GatherTask* __restrict__ tasks, const int32_t* __restrict__ idx, int D) {
  const GatherTask t = tasks[blockIdx.y];
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= t.n_dst) return;
  const int64_t s = t.has_idx ? (int64_t)idx[t.idx_off + r] : r;
  const T* sx = static_cast<const T*>(t.sx) + s * D; T* dx = static_cast<T*>(t.dx) + r * D;
  for (int d = 0; d < D; ++d) dx[d] = sx[d];
  static_cast<T*>(t.dys)[r] = static_cast<const T*>(t.sys)[s];
  if (t.syd) for (int a = 0; a <= t.m; ++a) static_cast<T*>(t.dyd)[(int64_t)a * t.n_dst + r] = static_cast<const T*>(t.syd)[(int64_t)a * t.n_src + s];
}
}  // namespace
void launch_gather_rows(int dtype, const GatherTask* tasks, const int32_t* idx, int T, int64_t max_dst, int D, hipStream_t st) {
  const dim3 grid((unsigned)((max_dst + 255) / 256), (unsigned)T);
  if (dtype == HBO_F64) hipLaunchKernelGGL(gather_rows_kernel<double>, grid, dim3(256), 0, st, tasks, idx, D);
  else hipLaunchKernelGGL(gather_rows_kernel<float>, grid, dim3(256), 0, st, tasks, idx, D);
}

extern "C" int hbo_dataset_subsample(hbo_ctx* c, const hbo_dataset* src, const int64_t* counts, const int32_t* idx, hbo_dataset** out) {
  if (!c || !src || !counts || !out) return fail(c, HBO_ERR_ARG, "hbo_dataset_subsample: null argument");
  HIPCHK(c, hipSetDevice(c->device));
  const int T = src->ntasks, dtype = src->dtype, D = src->D;
  const size_t es = esize(dtype);
  std::vector<TaskOff> offs(T);
  BlockLayout lay;
  int64_t nidx = 0, max_dst = 0;
  for (int k = 0; k < T; ++k) {
    const TaskHost* t = src->tasks[k];
    const int64_t nd = counts[k] < 0 ? t->n : counts[k];
    if (nd <= 0 || nd > t->n) return fail(c, HBO_ERR_ARG, "hbo_dataset_subsample: counts[k] must be in 1..n_k (or negative: the whole task)");
    if (counts[k] >= 0) { if (!idx) return fail(c, HBO_ERR_ARG, "hbo_dataset_subsample: idx is null"); nidx += nd; }
    offs[k] = dataset_place(lay, nd, D, t->m, t->ydiv != nullptr, es);
    max_dst = std::max(max_dst, nd);
  }
  const size_t total = lay.off;
  hbo_dataset* ds = new hbo_dataset();
  ds->dtype = dtype; ds->D = D;
  if (T == 0) { *out = ds; return HBO_OK; }
  // descriptors + indices through the pinned staging buffer, one copy
  const size_t desc_b = align256(sizeof(GatherTask) * T), idx_b = align256(sizeof(int32_t) * (size_t)std::max<int64_t>(nidx, 1));
  unsigned char* stage = static_cast<unsigned char*>(stage_begin(c, "hbo_dataset_subsample: ", desc_b + idx_b));
  unsigned char* d_args = static_cast<unsigned char*>(ws_get(c, WS_GATHER, desc_b + idx_b));
  hipError_t e = (stage && d_args) ? dev_alloc(c, &ds->d_inputs, total) : hipErrorOutOfMemory;
  if (e != hipSuccess) { hbo_dataset_free(c, ds); return fail(c, HBO_ERR_HIP, std::string("hbo_dataset_subsample: ") + hipGetErrorString(e)); }
  GatherTask* g = reinterpret_cast<GatherTask*>(stage);
  int64_t ioff = 0;
  for (int k = 0; k < T; ++k) {
    const TaskHost* s = src->tasks[k];
    const int64_t nd = counts[k] < 0 ? s->n : counts[k];
    const TaskHost* t = dataset_add_task(ds, nd, s->m, offs[k], s->ydiv != nullptr);
    g[k] = GatherTask{s->X, s->ysum, s->ydiv, t->X, t->ysum, t->ydiv, s->n, nd, ioff, s->m, counts[k] >= 0 ? 1 : 0};
    if (counts[k] >= 0) {
      for (int64_t r = 0; r < nd; ++r) if (idx[ioff + r] < 0 || idx[ioff + r] >= s->n) { hbo_dataset_free(c, ds); return fail(c, HBO_ERR_ARG, "hbo_dataset_subsample: index out of range"); }
      ioff += nd;
    }
  }
  if (nidx) memcpy(stage + desc_b, idx, sizeof(int32_t) * (size_t)nidx);
  hipStream_t st = c->stream;
  e = stage_upload(c, d_args, stage, desc_b + idx_b, st);
  if (e == hipSuccess) {
    launch_gather_rows(dtype, reinterpret_cast<const GatherTask*>(d_args), reinterpret_cast<const int32_t*>(d_args + desc_b), T, max_dst, D, st);
    e = hipGetLastError();
  }
  if (e != hipSuccess) { hbo_dataset_free(c, ds); return fail(c, HBO_ERR_HIP, std::string("hbo_dataset_subsample: ") + hipGetErrorString(e)); }
  dataset_finish(ds);
  *out = ds;
  return HBO_OK;
}
