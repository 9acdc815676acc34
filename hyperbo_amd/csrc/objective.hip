// The objectives of the C ABI: hbo_nll / hbo_objective (hyperbo/gp_utils/objectives.py:29-210 -- NLL, EKL, Euclid, value and
// gradient in one pass: features -> Gram -> blocked Cholesky with the augmented rows -> inverse -> K^-1 -> contraction) and its
// task-sharded form hbo_objective_sharded (device-side reduction + one in-place all-reduce).
// On the host one evaluation (objective_local) reads top to bottom: checks -> obj_plan (api_internal.h: every decision, no HIP call)
// -> obj_setup (workspaces, descriptors, the pinned stage) -> obj_steps over an ObjState (features, factor, reduce, inverse, extra
// rows, contract) -> enqueue_backward -> obj_shard_reduce or obj_copy_back, both over ONE gradient scatter table (api_internal.h:
// GradScatter).  objective_impl adds the sharded form's collective.
#include "api_internal.h"
#include <chrono>

extern "C" int hbo_nll(hbo_ctx* c, const hbo_model* m, hbo_dataset* ds, double* nll_sum, double* nll_per_task,
                       double* grad_sum) {
  return hbo_objective(c, m, ds, HBO_OBJ_NLL, nll_sum, nll_per_task, grad_sum);
}

// The launches of one evaluation that do not depend on the path taken (objective_local) or that hbo_train_adam (train.hip) queues once
// per step without the host-side set-up: the batched MLP basis (one launch per layer), the Kumaraswamy forward (w(X) and dw/da, dw/db
// of every task in one launch, before the Gram -- the fused path stays the fused path), the single-workgroup evaluation of a batch
// whose tasks all fit one 128-block (small.hip) and the backward passes of both paths.
static void enqueue_mlp_forward(hbo_ctx* c, const hbo_model* m, hbo_dataset* ds, int64_t max_n) {
  int fin = m->input_dim;
  for (int l = 0; l < m->n_layers; ++l) {
    launch_mlp_forward_batch(ds->dtype, ds->d_mlp, ds->ntasks, max_n, l, c->d_mlp_w[l], c->d_mlp_b[l], fin, m->features[l], c->stream);
    fin = m->features[l];
  }
}
static void enqueue_kumar_forward(hbo_ctx* c, const hbo_model* m, hbo_dataset* ds, int64_t max_n) {
  launch_kumar_forward(ds->dtype, ds->d_desc, ds->ntasks, max_n, nullptr, nullptr, nullptr, 0, m->input_dim, c->d_model, c->stream);
}
void enqueue_fused_forward(hbo_ctx* c, const hbo_model* m, hbo_dataset* ds, int64_t max_n, int out_stride, bool want_grad) {
  const bool kumar = is_kumar(m);
  if (needs_mlp(m)) { ProfScope ps(c, "features", 1); enqueue_mlp_forward(c, m, ds, max_n); }
  if (kumar) { ProfScope ps(c, "kumar_forward", 1); enqueue_kumar_forward(c, m, ds, max_n); }
  ProfScope ps(c, "small_eval", 1);
  launch_small_eval(ds->dtype, ds->d_desc, ds->ntasks, c->d_model, m->kernel_id, feature_dim(m), ds->d_info, ds->d_nll,
                    want_grad ? ds->d_gradout : nullptr, out_stride, want_grad && (needs_mlp(m) || kumar), c->stream);
}
int enqueue_backward(hbo_ctx* c, const hbo_model* m, hbo_dataset* ds, int64_t max_n, int obj, bool want_grad) {
  const int dtype = ds->dtype, T = ds->ntasks, max_nblk = ds->max_nblk, max_npad = max_nblk * HBO_TILE;
  const bool kumar = is_kumar(m), euc = obj == OBJ_EUC;
  hipStream_t st = c->stream;
  if (want_grad && kumar) {
    // d f / d a, d f / d b (kumar.hip): per-tile partials, one ordered sum over tiles and tasks -> ds->d_mlpgrad[0, 2D)
    ProfScope ps(c, "kumar_backward", 1);
    const int D = m->input_dim;
    const size_t tot = (size_t)2 * D;
    if (ds->mlpgrad_elems < tot) { if (ds->d_mlpgrad) dev_free(c, ds->d_mlpgrad); HIPCHK(c, dev_alloc(c, (void**)&ds->d_mlpgrad, tot * sizeof(double))); ds->mlpgrad_elems = tot; }
    double* part = static_cast<double*>(ws_get(c, WS_KU_PART, sizeof(double) * (size_t)T * max_nblk * max_nblk * 2 * D));
    if (!part) return HBO_ERR_HIP;
    launch_kumar_grad(dtype, ds->d_desc, T, max_nblk, c->d_model, m->kernel_id, D, obj, part, ds->d_mlpgrad, st);
  }
  if (want_grad && needs_mlp(m)) {
    // d nll / d features -> MLP backward (hyperbo/gp_utils/basis_functions.py:24-36), summed over tasks; every pass one launch
    // for the whole batch (mlp.hip)
    ProfScope ps(c, "mlp_backward", 1);
    const int L = m->n_layers, flast = m->features[L - 1];
    size_t tot = 0; int fin0 = m->input_dim;
    std::vector<size_t> woff(L), boff(L);
    for (int l = 0; l < L; ++l) { woff[l] = tot; tot += (size_t)fin0 * m->features[l]; boff[l] = tot; tot += m->features[l]; fin0 = m->features[l]; }
    if (ds->mlpgrad_elems < tot) { if (ds->d_mlpgrad) dev_free(c, ds->d_mlpgrad); HIPCHK(c, dev_alloc(c, (void**)&ds->d_mlpgrad, tot * sizeof(double))); ds->mlpgrad_elems = tot; }
    HIPCHK(c, hipMemsetAsync(ds->d_mlpgrad, 0, tot * sizeof(double), st));
    launch_mlp_zero_dF_batch(ds->d_mlp, T, max_n, flast, st);
    if (m->kernel_uses_mlp) {
      launch_grad_feat(dtype, ds->d_desc, T, max_nblk, c->d_model, m->kernel_id, flast, obj, st);
      if (euc) launch_scale_dF(ds->d_desc, T, (int64_t)max_npad, flast, st);
    }
    if (m->mean_id == HBO_MEAN_LINEAR_MLP) launch_grad_feat_mean(dtype, ds->d_desc, T, (int64_t)max_npad, c->d_model, flast, st);
    for (int l = L - 1; l >= 0; --l) {
      const int fin = l ? m->features[l - 1] : m->input_dim;
      launch_dense_bwd_batch(dtype, ds->d_mlp, T, max_n, l, ((L - 1 - l) % 2) == 0, c->d_mlp_w[l], ds->d_mlpgrad + woff[l], ds->d_mlpgrad + boff[l],
                             fin, m->features[l], l > 0, st);
    }
  }
  return HBO_OK;
}

// ---- what hbo_probe_factor_inverse (probe.hip) runs too: api_internal.h ------------------------------------------------------
hipStream_t obj_fork_side(hbo_ctx* c, bool side_reduce) {
  hipStream_t st = c->stream, side = side_reduce ? c->stream2 : st;
  if (side != st) { hipEvent_t e = pool_event(c, 2); hipEventRecord(e, st); hipStreamWaitEvent(side, e, 0); }
  return side;
}
hipEvent_t obj_inverse_step(hbo_ctx* c, InvRun& inv, int max_naug, hipStream_t side, int dmu_obj) {
  const int dtype = inv.dtype, T = inv.ntasks, max_nblk = inv.max_nblk, max_npad = max_nblk * HBO_TILE;
  hipStream_t st = c->stream;
  hipEvent_t ev_side = nullptr;
  hipEvent_t w_done = side != st ? pool_event(c, 3) : nullptr;   // W is complete
  if (inv.pl.sweep) {
    // what the chain left: the last row group(s).  W is complete behind the last group's rows (event), K^-1 behind its update
    ProfScope ps(c, "sweep_tail", 1);
    sweep_advance(inv, max_nblk, st, w_done);
  } else {
    { ProfScope ps(c, "trtri", 1); run_trtri(inv); }
    if (w_done) hipEventRecord(w_done, st);
  }
  if (w_done) hipStreamWaitEvent(side, w_done, 0);
  { ProfScope ps(c, "wt_z", 1, side);
    for (int b = 0; b < max_naug; ++b) launch_wt_z(dtype, inv.d_tasks, T, max_nblk, b, b, max_npad, side); }
  if (side != st) {
    if (dmu_obj >= 0) launch_dmu(dtype, inv.d_tasks, T, dmu_obj, side);
    ev_side = pool_event(c, 4); hipEventRecord(ev_side, side);
  }
  // One sequence for both forms: record; [K^-1 = W^T W of the recursive form]; the main stream's wait.  The sweep has its K^-1
  // already and queues nothing on the main stream between the record and the wait, so its wait follows the record at once.
  if (!inv.pl.sweep) { ProfScope ps(c, "lauum", 1); run_lauum(inv); }
  if (ev_side) hipStreamWaitEvent(st, ev_side, 0);
  return ev_side;
}

namespace {
// what set-up and the steps of one evaluation share: the call, its plan (api_internal.h: obj_plan), and the events in flight
struct ObjState {
  hbo_ctx* c; const hbo_model* m; hbo_dataset* ds; ObjPlan p;
  unsigned char* stage = nullptr;   // the pinned buffer, at its final size (obj_setup)
  int max_naug = 1;                 // augmented rows of the largest task: needs the filled descriptors
  InvRun inv = {};                  // the inverse side of this evaluation (step_factor)
  hipStream_t side = nullptr;       // where the small reductions run: the panel stream, or the main one (step_reduce)
  hipEvent_t ev_side = nullptr;     // behind d nll / d mu on the side stream, once the main stream has been told to wait for it
};

// a rank beyond the task count: zeros into the collective
int obj_empty_rank(hbo_ctx* c, int red_count, ShardOut* so) {
  hipStream_t st = c->stream;
  double* d_red = static_cast<double*>(ws_get(c, WS_SHARD_RED, sizeof(double) * red_count));
  if (!d_red) return HBO_ERR_HIP;
  hipEvent_t ev0 = pool_event_timed(c, 0), ev1 = pool_event_timed(c, 1);
  HIPCHK(c, hipEventRecord(ev0, st));
  HIPCHK(c, hipMemsetAsync(d_red, 0, sizeof(double) * red_count, st));
  HIPCHK(c, hipEventRecord(ev1, st));
  so->d_red = d_red; so->ev0 = ev0; so->ev1 = ev1;
  return HBO_OK;
}

// workspaces + descriptors: everything the launches read, allocated and uploaded (what the plan's lds_only spares a batch is said there)
int obj_setup(ObjState& s) {
  hbo_ctx* c = s.c; const hbo_model* m = s.m; hbo_dataset* ds = s.ds; const ObjPlan& p = s.p;
  const int T = p.T, dtype = p.dtype, obj = p.obj;
  const bool lds_only = p.lds_only, want_grad = p.want_grad;
  hipStream_t st = c->stream;
  int rc;
  void* small_scratch = nullptr;
  if (lds_only) {
    small_scratch = ws_get(c, WS_SMALL_W, (size_t)HBO_TILE * padded_ld(HBO_TILE, ds->dtype) * esize(ds->dtype));
    if (!small_scratch) return HBO_ERR_HIP;
  }
  if (!lds_only && !ds->d_svec && T > 1) {
    // first evaluation of this dataset: every task's alpha vector from ONE zeroed block
    const size_t es = esize(ds->dtype);
    size_t tot = 0;
    for (TaskHost* t : ds->tasks) tot += align256((size_t)t->npad * es * (obj == OBJ_NLL ? 1 : t->m + 1));
    bool fresh = true;
    for (TaskHost* t : ds->tasks) if (t->svec) fresh = false;
    if (fresh && dev_alloc(c, &ds->d_svec, tot) == hipSuccess) {
      HIPCHK(c, hipMemsetAsync(ds->d_svec, 0, tot, st));
      size_t off = 0;
      for (TaskHost* t : ds->tasks) {
        const int cols = obj == OBJ_NLL ? 1 : t->m + 1;
        t->svec = (char*)ds->d_svec + off; t->svec_cols = cols; t->svec_shared = true;
        off += align256((size_t)t->npad * es * cols);
      }
    } else { (void)hipGetLastError(); ds->d_svec = nullptr; }
  }
  ds->h_desc.resize(T);
  for (int k = 0; k < T; ++k) {
    TaskHost* t = ds->tasks[k];
    if (!lds_only) {
      rc = ensure_task_workspace(c, dtype, t, p.need_S, obj == OBJ_NLL ? 1 : t->m + 1);
      if (rc) return rc;
    }
    if (p.mlp) { rc = t->feat.ensure(c, m, t->n); if (rc) return rc; }
    if (p.kumar) { rc = ensure_kumar_buffers(c, m, t, t->n, want_grad); if (rc) return rc; }
    if (p.mlp && want_grad) {
      int maxf = m->input_dim;
      for (int l = 0; l < m->n_layers; ++l) maxf = std::max(maxf, (int)m->features[l]);
      const size_t need = (size_t)t->n * maxf;
      if (t->dF_elems < need) {
        if (t->dF) dev_free(c, t->dF);
        if (t->dtmp) dev_free(c, t->dtmp);
        t->dF = t->dtmp = nullptr;
        HIPCHK(c, dev_alloc(c, (void**)&t->dF, need * sizeof(double)));
        HIPCHK(c, dev_alloc(c, (void**)&t->dtmp, need * sizeof(double)));
        t->dF_elems = need;
      }
    }
    fill_desc(ds->h_desc[k], t, m, dtype, obj);
    if (lds_only && !ds->h_desc[k].W) ds->h_desc[k].W = small_scratch;   // (every task writes its leaf inverses there: never read)
  }
  for (int k = 0; k < T; ++k) s.max_naug = std::max(s.max_naug, ds->h_desc[k].naug);
  if (p.mlp) {
    // per-task pointers of the batched MLP passes (mlp.hip); uploaded when an allocation moved
    std::vector<MlpTaskDev> hm(T);
    for (int k = 0; k < T; ++k) {
      TaskHost* t = ds->tasks[k];
      memset(&hm[k], 0, sizeof(MlpTaskDev));
      hm[k].x = t->X; hm[k].n = t->n; hm[k].dF = t->dF; hm[k].dtmp = t->dtmp;
      for (int l = 0; l < m->n_layers; ++l) hm[k].acts[l] = t->feat.acts[l];
    }
    if (!ds->d_mlp) HIPCHK(c, dev_alloc(c, (void**)&ds->d_mlp, sizeof(MlpTaskDev) * T));
    if (ds->h_mlp_dev.size() != (size_t)T || memcmp(ds->h_mlp_dev.data(), hm.data(), sizeof(MlpTaskDev) * T) != 0) {
      HIPCHK(c, hipStreamSynchronize(st));   // (the previous table may still be read by queued work; happens once per dataset)
      ds->h_mlp_dev = hm;
      HIPCHK(c, hipMemcpyAsync(ds->d_mlp, ds->h_mlp_dev.data(), sizeof(MlpTaskDev) * T, hipMemcpyHostToDevice, st));
    }
  }
  // (per-dataset buffers come from the context's pool: a fresh batch per Adam step paid three hipMalloc + three synchronising
  //  hipFree for its descriptors, results and gradient partials)
  if (!ds->d_desc) HIPCHK(c, dev_alloc(c, (void**)&ds->d_desc, sizeof(TaskDesc) * T));
  const int out_stride = p.out_stride;
  const size_t pack_bytes = p.pack_bytes;
  if (ds->pack_bytes < pack_bytes) {
    if (ds->d_pack) dev_free(c, ds->d_pack);
    ds->d_pack = nullptr; ds->pack_bytes = 0;
    HIPCHK(c, dev_alloc(c, (void**)&ds->d_pack, pack_bytes));
    ds->pack_bytes = pack_bytes;
  }
  ds->d_nll = ds->d_pack; ds->d_gradout = ds->d_pack + T; ds->d_info = reinterpret_cast<int*>(ds->d_pack + T + (size_t)T * out_stride);
  // small transfers go through one pinned buffer: descriptors up (only when they changed), results down in one copy
  // (fetched at its final size here, and not waited for: a call whose descriptors stand only uses it as the target of the copy back)
  s.stage = static_cast<unsigned char*>(pinned_stage(c, std::max(sizeof(TaskDesc) * T, pack_bytes)));
  if (!s.stage) return fail(c, HBO_ERR_HIP, "hbo_objective: pinned staging buffer");
  if (ds->h_desc_dev.size() != (size_t)T || memcmp(ds->h_desc_dev.data(), ds->h_desc.data(), sizeof(TaskDesc) * T) != 0) {
    HIPCHK(c, stage_wait(c));   // the upload before this one may still read the buffer
    memcpy(s.stage, ds->h_desc.data(), sizeof(TaskDesc) * T);
    HIPCHK(c, stage_upload(c, ds->d_desc, s.stage, sizeof(TaskDesc) * T, st));   // the pinned buffer is written again later (sharded: the scatter table, obj_shard_reduce)
    ds->h_desc_dev = ds->h_desc;
  }
  if (!p.fused_small) HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ds->d_info), INT_MAX, T, st));
  return HBO_OK;
}

// ---- the steps of the blocked pipeline, in launch order (obj_steps) ---------------------------------------------------------
// the MLP basis, the augmented rows, the Kumaraswamy forward
void step_features(ObjState& s) {
  hbo_ctx* c = s.c; hbo_dataset* ds = s.ds; const ObjPlan& p = s.p;
  if (c->opt_poison) launch_poison(p.dtype, ds->d_desc, p.T, p.max_npad, c->stream);
  {
    ProfScope ps(c, "features", 1);
    if (p.mlp) enqueue_mlp_forward(c, s.m, ds, p.max_n);
    launch_aug_rows(p.dtype, ds->d_desc, p.T, p.max_npad, c->d_model, c->stream);
  }
  if (p.kumar) { ProfScope ps(c, "kumar_forward", 1); enqueue_kumar_forward(c, s.m, ds, p.max_n); }
}
// the Gram matrices and their blocked factorisation, with the inverse beside or behind the chain where the plan says so
void step_factor(ObjState& s) {
  hbo_ctx* c = s.c; hbo_dataset* ds = s.ds; const ObjPlan& p = s.p;
  {
    ProfScope ps(c, "gram", 1);
    GramArgs g = {}; g.kernel_id = c->h_model->kernel_id; g.mfma_min_f = c->opt_gram_mfma; g.tasks = ds->d_desc; g.fdim = p.fdim; g.symmetric = 1; g.padded = 1;
    launch_gram(p.dtype, g, c->d_model, dim3(p.max_nblk, p.max_nblk, p.T), c->stream);
  }
  s.inv = {c, p.dtype, ds->d_desc, p.T, p.max_nblk, p.T == 1 ? &ds->h_desc[0] : nullptr, p.inv};
  c->run.chol_diag_bound = chol_diag_bound_of(s.m);   // (cleared where the evaluation leaves: objective_local's bound_scope)
  ProfScope ps(c, "potrf", 1);
  run_potrf(c, p.dtype, ds->d_desc, p.T, p.max_nblk, ds->d_info, &s.inv);
}
// the fork to the side stream (where the plan sends the small reductions there) and the first of them
void step_reduce(ObjState& s) {
  hbo_ctx* c = s.c; hbo_dataset* ds = s.ds; const ObjPlan& p = s.p;
  s.side = obj_fork_side(c, p.side_reduce);
  ProfScope ps(c, "nll_reduce", 1, s.side);
  launch_nll_reduce(p.dtype, ds->d_desc, p.T, ds->d_info, ds->d_nll, s.side);
}
// W = L^-1 and K^-1 in either form, alpha = W^T z and (side stream) d nll / d mu beside them
void step_inverse(ObjState& s) { s.ev_side = obj_inverse_step(s.c, s.inv, s.max_naug, s.side, s.p.obj); }
// the data rows of tasks with more than 127 aligned columns, as outer-product vectors in svec columns 1..m (objectives.py:29-106
// has no limit on m).  EUC: the rows themselves.  EKL: tr(K1^-1 C0) = sum_b |W row_b|^2 and alpha_b = W^T W row_b from the explicit
// inverse (two triangular products over all m rows), the quadratic forms added to the task's value.  Main stream, W complete.
int step_extra_rows(ObjState& s) {
  hbo_ctx* c = s.c; hbo_dataset* ds = s.ds;
  const int T = s.p.T, dtype = s.p.dtype; const bool euc = s.p.euc;
  hipStream_t st = c->stream;
  ProfScope ps(c, "extra_rows", 1);
  // one scratch buffer for the largest of them, taken BEFORE the loop: growing it between two tasks would free memory that the
  // first task's queued products still read
  size_t zbytes = 0;
  if (!euc) for (int k = 0; k < T; ++k) if (ds->h_desc[k].nvec) zbytes = std::max(zbytes, (size_t)ds->tasks[k]->m * ds->tasks[k]->npad * esize(dtype));
  void* const zb = zbytes ? ws_get(c, WS_EXTRA_Z, zbytes) : nullptr;
  if (zbytes && !zb) return HBO_ERR_HIP;
  for (int k = 0; k < T; ++k) {
    if (!ds->h_desc[k].nvec) continue;
    TaskHost* t = ds->tasks[k];
    const size_t es = esize(dtype);
    char* cols = static_cast<char*>(t->svec) + (size_t)t->npad * es;   // column 1
    launch_expand_rows(dtype, t->ydiv, t->n, t->npad, cols, t->m, st);
    if (euc) continue;
    launch_tri_matvec(dtype, t->W, t->ld, t->npad, cols, t->npad, t->m, 0, zb, t->npad, st);
    launch_add_sumsq(dtype, zb, t->npad, t->m, ds->h_desc[k].coef_c, ds->d_nll + k, st);
    launch_tri_matvec(dtype, t->W, t->ld, t->npad, zb, t->npad, t->m, 1, cols, t->npad, st);
  }
  return HBO_OK;
}
// d f / d mu (where the side stream has not done it), the per-tile contraction and its finalisation into the tasks' gradient blocks
void step_contract(ObjState& s) {
  hbo_ctx* c = s.c; const hbo_model* m = s.m; hbo_dataset* ds = s.ds; const ObjPlan& p = s.p;
  hipStream_t st = c->stream;
  ProfScope ps(c, "grad_contract", 1);
  if (!s.ev_side) launch_dmu(p.dtype, ds->d_desc, p.T, p.obj, st);
  launch_grad_contract(p.dtype, ds->d_desc, p.T, p.max_nblk, c->d_model, m->kernel_id, p.fdim, p.obj, ds->d_partials, p.stride_task, st);
  launch_grad_finalize(p.dtype, ds->d_desc, p.T, c->d_model, m->kernel_id, p.fdim, p.obj, ds->d_partials, p.stride_task, ds->d_gradout, p.out_stride, p.euc ? ds->d_nll : nullptr, st,
                       ds->d_partials + p.stride_task * p.T, p.max_nblk);
}
// the blocked pipeline: what a batch runs that does not take the single-workgroup evaluation
int obj_steps(ObjState& s) {
  hbo_ctx* c = s.c; hbo_dataset* ds = s.ds; const ObjPlan& p = s.p;
  s.side = c->stream;
  step_features(s);
  if (!p.euc) { step_factor(s); step_reduce(s); }
  if (p.value_inverse) {
    { ProfScope ps(c, "trtri", 1); run_trtri(s.inv); }
    if (int rc = step_extra_rows(s)) return rc;
  }
  if (!p.contract) return HBO_OK;
  if (ds->partials_bytes < p.partials_bytes) { if (ds->d_partials) dev_free(c, ds->d_partials); HIPCHK(c, dev_alloc(c, (void**)&ds->d_partials, p.partials_bytes)); ds->partials_bytes = p.partials_bytes; }
  if (!p.euc) step_inverse(s);
  if (p.extras) if (int rc = step_extra_rows(s)) return rc;
  step_contract(s);
  return HBO_OK;
}

// sharded: [nll, count, grad] of this rank's tasks in the caller's gradient layout, on the device, with the scatter table uploaded in
// its device format (api_internal.h: GradScatter); returns without waiting
int obj_shard_reduce(ObjState& s, const GradScatter& tab, hipEvent_t ev_sh0, ShardOut* so) {
  hbo_ctx* c = s.c; hbo_dataset* ds = s.ds; const ObjPlan& p = s.p;
  hipStream_t st = c->stream;
  int* d_map = static_cast<int*>(ws_get(c, WS_SHARD_MAP, tab.bytes()));
  double* d_red = static_cast<double*>(ws_get(c, WS_SHARD_RED, sizeof(double) * p.red_count));
  if (!d_map || !d_red) return HBO_ERR_HIP;
  s.stage = static_cast<unsigned char*>(stage_begin(c, "hbo_objective: ", tab.bytes()));
  if (!s.stage) return HBO_ERR_HIP;
  memcpy(s.stage, tab.w, tab.bytes());
  HIPCHK(c, stage_upload(c, d_map, s.stage, tab.bytes(), st));
  launch_shard_reduce(ds->d_nll, p.want_grad ? ds->d_gradout : nullptr, ds->d_info, p.T, p.out_stride, d_map, ds->d_mlpgrad, d_map + p.out_stride, tab.nseg,
                      d_red, p.red_count, st);
  hipEvent_t ev1 = pool_event_timed(c, 1);
  HIPCHK(c, hipEventRecord(ev1, st));
  HIPCHK(c, hipGetLastError());
  so->d_red = d_red; so->ev0 = ev_sh0; so->ev1 = ev1;
  so->d_map = d_map; so->nseg = tab.nseg; so->out_stride = p.out_stride;
  return HBO_OK;
}
// not sharded: results down in one copy through the pinned buffer (and the summed leaves in one more), one wait, the host finish
int obj_copy_back(ObjState& s, const GradScatter& tab, std::chrono::steady_clock::time_point host_t0, double* nll_sum, double* nll_per_task, double* grad_sum) {
  hbo_ctx* c = s.c; hbo_dataset* ds = s.ds; const ObjPlan& p = s.p;
  const int T = p.T;
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(s.stage, ds->d_pack, p.pack_bytes, hipMemcpyDeviceToHost, st));
  const double* h_nll = reinterpret_cast<const double*>(s.stage);
  const double* h_grad = h_nll + T;
  const int* h_info = reinterpret_cast<const int*>(h_grad + (size_t)T * p.out_stride);
  std::vector<double> h_mlp;
  if (tab.nseg) {
    h_mlp.resize(ds->mlpgrad_elems);
    HIPCHK(c, hipMemcpyAsync(h_mlp.data(), ds->d_mlpgrad, sizeof(double) * ds->mlpgrad_elems, hipMemcpyDeviceToHost, st));
  }
  const double host_enqueue_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count();
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  prof_collect(c);
  if (c->prof_level >= 1) { c->prof_names.push_back("host_enqueue"); c->prof_ms.push_back(host_enqueue_ms); c->prof_count.push_back(1); }

  bool notpd = false;
  double total = 0;
  for (int k = 0; k < T; ++k) { total += h_nll[k]; if (h_info[k] != INT_MAX) notpd = true; if (nll_per_task) nll_per_task[k] = h_nll[k]; }
  *nll_sum = total;
  if (p.want_grad) grad_scatter_host(tab, T, h_grad, h_info, h_mlp.data(), notpd, grad_sum);
  return notpd ? HBO_NOT_PD : HBO_OK;
}
}  // namespace

int objective_local(hbo_ctx* c, const hbo_model* m_in, hbo_dataset* ds, int objective, double* nll_sum,
                    double* nll_per_task, double* grad_sum, const ShardReq* sh, ShardOut* so) {
  if (!c || !nll_sum || !m_in || (!ds && !sh)) return fail(c, HBO_ERR_ARG, "hbo_objective: null argument");
  if (objective != HBO_OBJ_NLL && objective != HBO_OBJ_EKL && objective != HBO_OBJ_EUC) return fail(c, HBO_ERR_ARG, "hbo_objective: unknown objective id");
  HIPCHK(c, hipSetDevice(c->device));
  ModelCopy mcopy(m_in);   // (a Kumaraswamy model keeps its a, b)
  if (objective != HBO_OBJ_NLL) mcopy.get()->eps = 0.0;   // objectives.py:63-65: cov_model = K + noise I, no jitter
  const hbo_model* m = mcopy.get();
  CholBoundScope bound_scope(c, 0.0);   // (set where the factorisation starts; cleared on every way out)
  int rc = validate_model(c, m);
  if (rc) return rc;
  if (ds && ds->ntasks > 0 && (m->dtype != ds->dtype || m->input_dim != ds->D)) return fail(c, HBO_ERR_ARG, "hbo_objective: model/dataset dtype or input_dim mismatch");
  hbo_grad_layout lay;
  hbo_grad_layout_of(m, &lay);
  const bool want_grad = grad_sum != nullptr;
  *nll_sum = 0;
  if (want_grad) for (int i = 0; i < lay.total; ++i) grad_sum[i] = 0;
  ObjState s = {c, m, ds, obj_plan(c, m, ds, lay, objective, want_grad, sh != nullptr)};
  const ObjPlan& p = s.p;
  if (so) so->red_count = p.red_count;
  if (p.T == 0) return sh ? obj_empty_rank(c, p.red_count, so) : HBO_OK;
  if (p.obj != OBJ_NLL) for (TaskHost* t : ds->tasks) if (!t->ydiv) return fail(c, HBO_ERR_ARG, "hbo_objective: the dataset carries no divergence rows");
  prof_begin(c);
  const auto host_t0 = std::chrono::steady_clock::now();   // host time spent queueing this evaluation (stage "host_enqueue", level 1)
  hipEvent_t ev_sh0 = nullptr;
  if (sh) { ev_sh0 = pool_event_timed(c, 0); HIPCHK(c, hipEventRecord(ev_sh0, c->stream)); }
  rc = upload_model(c, m);
  if (rc) return rc;
  rc = obj_setup(s);
  if (rc) return rc;
  if (p.fused_small) enqueue_fused_forward(c, m, ds, p.max_n, p.out_stride, want_grad);
  else if ((rc = obj_steps(s))) return rc;
  rc = enqueue_backward(c, m, ds, p.max_n, p.obj, want_grad);
  if (rc) return rc;
  // where the gradient goes in the caller's layout: ONE table for the device reduction and for the host finish
  int32_t kumar_a = -1, kumar_b = -1;
  if (p.kumar) hbo_grad_layout_kumar_of(m, &kumar_a, &kumar_b);
  GradScatter tab;
  grad_scatter_fill(tab, m, lay, kumar_a, kumar_b, p.out_stride, want_grad);
  if (sh) return obj_shard_reduce(s, tab, ev_sh0, so);
  return obj_copy_back(s, tab, host_t0, nll_sum, nll_per_task, grad_sum);
}
static int objective_impl(hbo_ctx* c, const hbo_model* m_in, hbo_dataset* ds, int objective, double* nll_sum,
                          double* nll_per_task, double* grad_sum, const ShardReq* sh) {
  if (!sh) return objective_local(c, m_in, ds, objective, nll_sum, nll_per_task, grad_sum, nullptr, nullptr);
  if (c && c->comm_aborted)
    return fail(c, HBO_ERR_COMM, "hbo_objective_sharded: the communicator was aborted after a failed evaluation; call hbo_comm_init again");
  ShardOut so;
  int rc_local = objective_local(c, m_in, ds, objective, nll_sum, nll_per_task, grad_sum, sh, &so);
  if (!c || !nll_sum || !m_in) return rc_local;   // argument errors are the same on every rank: nobody reaches the collective
  // one-shot fault injection (hbo_tune "fault_shard", tests only): 1 = this rank's local part counts as failed (NaN contribution
  // path below), 2 = and it cannot even produce the NaN buffer (abort path)
  const int fault = c->opt_fault_shard; c->opt_fault_shard = 0;
  if (fault && rc_local == HBO_OK) { rc_local = fail(c, HBO_ERR_HIP, "hbo_objective_sharded: injected local failure (fault_shard)"); so.d_red = nullptr; }
  hipStream_t st = c->stream;
  int red_count = so.red_count;
  if (red_count <= 0) {   // failed before the model was looked at: the layout still fixes the length the peers reduce
    hbo_grad_layout lay;
    if (hbo_grad_layout_of(m_in, &lay) != HBO_OK) return rc_local;
    red_count = 2 + (grad_sum ? lay.total : 0);
  }
  if (rc_local != HBO_OK || !so.d_red) {
    // local failure: NaN into every slot of the collective (0x7FF800007FF80000 is a quiet NaN).  The failed pipeline may have left
    // launches queued on the side streams (look-ahead panels, the early inverse): join them before the workspaces are reused
    (void)hipGetLastError();
    for (hipStream_t q : {c->stream2, c->stream3, c->stream4}) if (q) (void)hipStreamSynchronize(q);
    (void)hipGetLastError();
    so.d_red = static_cast<double*>(ws_get(c, WS_SHARD_RED, sizeof(double) * red_count));
    so.ev0 = pool_event_timed(c, 0); so.ev1 = pool_event_timed(c, 1);
    const bool ok = fault != 2 && so.d_red && hipEventRecord(so.ev0, st) == hipSuccess &&
                    hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(so.d_red), 0x7FF80000, 2 * (size_t)red_count, st) == hipSuccess &&
                    hipEventRecord(so.ev1, st) == hipSuccess;
    if (!ok) { if (c->comm) comm_abort(c); return rc_local ? rc_local : HBO_ERR_HIP; }
  }
  hipEvent_t ev2 = pool_event_timed(c, 2);
  int rc = c->comm ? comm_allreduce_device(c, so.d_red, red_count, st) : HBO_OK;
  if (rc) return rc_local ? rc_local : rc;
  HIPCHK(c, hipEventRecord(ev2, st));
  double* stage = static_cast<double*>(pinned_stage(c, sizeof(double) * red_count));
  if (!stage) return fail(c, HBO_ERR_HIP, "hbo_objective_sharded: pinned staging buffer");
  HIPCHK(c, stage_wait(c));
  HIPCHK(c, hipMemcpyAsync(stage, so.d_red, sizeof(double) * red_count, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  prof_collect(c);
  *nll_sum = stage[0];
  *sh->count = stage[1];
  if (grad_sum) for (int i = 0; i < red_count - 2; ++i) grad_sum[i] = stage[2 + i];
  if (sh->timing) {
    float ms_local = 0, ms_comm = 0;
    hipEventElapsedTime(&ms_local, so.ev0, so.ev1); hipEventElapsedTime(&ms_comm, so.ev1, ev2);
    sh->timing[0] = ms_local; sh->timing[1] = 1e3 * ms_comm;
  }
  if (rc_local) return rc_local;
  return std::isnan(*nll_sum) ? HBO_NOT_PD : HBO_OK;
}
extern "C" int hbo_objective(hbo_ctx* c, const hbo_model* m, hbo_dataset* ds, int objective, double* nll_sum,
                             double* nll_per_task, double* grad_sum) {
  if (!ds) return fail(c, HBO_ERR_ARG, "hbo_objective: null argument");
  return objective_impl(c, m, ds, objective, nll_sum, nll_per_task, grad_sum, nullptr);
}
extern "C" int hbo_objective_sharded(hbo_ctx* c, const hbo_model* m, hbo_dataset* ds, int objective, double* value_sum,
                                     double* count, double* grad_sum, double* timing) {
  if (!count) return fail(c, HBO_ERR_ARG, "hbo_objective_sharded: null argument");
  ShardReq sh{count, timing};
  return objective_impl(c, m, ds, objective, value_sum, nullptr, grad_sum, &sh);
}
