// Context object of libhbo and the error plumbing shared by its host translation units (api.hip: the C ABI and the
// orchestration of the kernels; comm.hip: the RCCL binding).
#pragma once
#include "hbo_internal.h"

#include <stdio.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

extern thread_local std::string hbo_g_err;   // last error of ctx-less calls (hbo_last_error(NULL))

struct ProfEntry { const char* name; hipEvent_t e0, e1; };
// a region of the zeroed tile-counter array whose words the resident launches take in turn (sched.hip: resident_grid)
struct TileCounters { int* base = nullptr; int next = 0; int limit = 0; };

struct hbo_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;   // panel stream of the look-ahead Cholesky (high priority)
  hipStream_t stream3 = nullptr;   // the later block columns of F1 (run_potrf: split_f1), beside the next diagonal block's factorisation and solve
  hipStream_t stream4 = nullptr;   // early part of trtri, overlapped with the tail of potrf
  int* d_yield = nullptr;    // per-CU table (cu_token() -> panel-chain workgroups running there)
  // What one factorisation hands to the schedules that run beside and behind it (sched.hip): launch-time facts, which those
  // combine with their plan (sched.h: InvPlan) where a launch is made.  The callers of run_potrf set chol_diag_bound before it and
  // clear it when the evaluation leaves (CholBoundScope; objective.hip); everything else is set by run_potrf.  (The host copy of a
  // single task's descriptor is no part of this: it travels in the caller's InvRun.)
  struct Run {
    double chol_diag_bound = 0;        // max_i A_ii (signal variance + noise + jitter), 0: unknown.  Read by run_potrf and trtri_level3 (the
                                       // a-priori scale of the f16x2 products); valid until the last product of the inverse
    unsigned int* h2_words = nullptr;  // measured operand maxima of the f16x2 products (null: bf16x3).  Read by trtri_level3 and run_lauum;
                                       // valid until the next run_potrf, i.e. through the last product of the inverse and of K^-1 = W^T W
    int* gemm_yield = nullptr;         // GemmArgs::yield_flag of the launches that co-run with the panel chain on the side stream.  Read by
                                       // trtri_level, trtri_level3 and sweep_advance; cleared when run_potrf returns
    TileCounters side;                 // tile counters of those launches (resident_grid); base is cleared when run_potrf returns
    int post_counter_next = 0;         // next zeroed counter for a resident launch BEHIND the factorisation (post_counter): reset by
                                       // run_potrf, which zeroes the whole array; read by trtri_level, trtri_level3 and run_lauum
  } run;
  // ---- schedule options (hbo_set_option / hbo_tune; sched.hip) ----
  int opt_lookahead = 1;
  int opt_overlap_trtri = 1;
  int opt_group = 0;         // 128-wide panels per trailing update (K = 128*group); 0: auto, see potrf_plan
  int opt_group_inner = -1;  // two-level panel groups: column updates on the chain inside inner groups of this many panels (0: one level; -1: auto, see potrf_plan)
  int opt_cu_yield = 2;      // background GEMM workgroups pause while a panel-chain workgroup runs on their CU (single matrix,
                             // look-ahead): 1 = potf2 only, 2 = trsm and the chain's column updates too
  int opt_small_nblk = -1;   // matrices up to this many 128-blocks use 64x64 GEMM tiles in trtri / lauum / the sweep (-1: auto, sched.h: small_limit)
  int opt_persist_free = -1; // bulk trailing update runs as 2*(CUs - this) persistent workgroups (-1: auto, see potrf_plan)
  int opt_trtri_bf16x3 = 1;    // fp32, one matrix: the products of the block-recursive inverse on the bf16 cores from level trtri3_min_s on
  int opt_trtri3_min_s = 8;
  int opt_lauum_bf16x3 = 1;    // fp32, one matrix: K^-1 = W^T W on the bf16 cores too
  int opt_syrk3_free = 32;     // CUs the bulk update on the bf16 / fp16 cores leaves with a single workgroup (room for the panel kernels)
  int opt_syrk_bf16x3 = 1;     // fp32 factorisations: trailing updates on the bf16 matrix cores (exact three-way split of the panels, post3.hip)
  int opt_chol_f16x2 = 1;      // fp32 factorisations of the stationary covariances: trailing updates, inverse levels and K^-1 = W^T W on two-way fp16 splits
                               // (three MFMAs per product instead of bf16x3's six; needs run.chol_diag_bound, i.e. a caller that knows max_i A_ii)
  int opt_trtri_at = 0;        // single matrix: panel count (in 64ths of the block count) after which the inverse starts beside the chain (0: 5/8)
  int opt_sweep = 1;           // one-sweep inverse (sched.hip:sweep_advance): 0 never, 1 where measured faster (use_sweep), 2 wherever look-ahead is on
  int opt_sweep_big = 4000;    // a sweep launch of a small / batched shape with at least this many 128-tiles (x tasks) runs on 128-tiles
  int opt_sweep_side = 1;      // one matrix on 128-tiles: the sweep's K^-1 updates (d) on a stream of their own beside its (a) (b) (c) chain
  int opt_sweep_free = 24;     // CUs the sweep's persistent launches beside the chain leave with one workgroup (at most trtri_free)
  int opt_sweep_qs = 0;        // its row-group size in 128-blocks (power of two; 0: auto)
  int opt_batch_bg = -1;       // batches: the sweep's launches beside the panel chain are 0 plain grids, 1 persistent and slot-limited (-1: auto = 1 up to 8 tasks),
                               // (tiles x tasks from one counter), 2 also yielding to the chain's kernels through the per-CU table
  int opt_split_f1 = 1;        // panel chain: F1 updates only the next block column on the panel stream, the group's later columns on a third stream:
                               // 0 never, 1 for batches (where it was measured faster), 2 always
  int opt_lauum_persist = 1;   // one large matrix: K^-1 = W^T W as a resident grid drawing its tiles from a counter (0: plain grid; 1: two workgroups
                               // on all but 16 CUs; n > 1: on all but n CUs)
  int opt_trtri_free = 48;   // CUs the inverse products that co-run with the panel chain leave free (0: one tile per workgroup)
  int opt_poison = 0;          // tests: every evaluation first fills what it is about to recompute with NaN (taskvec.hip: poison_kernel)
  // ---- posterior options ----
  int opt_post_chunk = 8192;   // posterior / acquisition: candidates per pass (the cross-Gram workspace is npad x this, whatever M)
  int opt_post_f16x2 = 1;      // fp32 posterior product of the stationary covariances: two-way fp16 split, three MFMAs per product (post3.hip: post2h_kernel) instead of bf16x3's six
  int opt_post_bf16x3 = 1;     // fp32 posterior product on the bf16 matrix cores (three-way exact split of both operands, post3.hip); 0: fp32 MFMA
  int n_cus = 256;
  std::vector<hipEvent_t> ev_pool;
  std::vector<hipEvent_t> ev_pool_sweep;   // sweep_advance's own events (its calls interleave with run_potrf's use of ev_pool)
  hipEvent_t ev_timed[3] = {nullptr, nullptr, nullptr};   // hbo_objective_sharded: start / local shard done / all-reduce done
  std::map<int, std::pair<void*, size_t>> ws;   // grow-only device scratch buffers by slot (no per-call hipMalloc/hipFree)
  // Device buffers of freed datasets / caches, kept for the next one of the same shape (dev_alloc / dev_free in api.hip):
  // GP.train()'s Adam loop re-creates its sub-sampled batch every step (gp.py:101-111) and 64 tasks x 8 buffers of
  // hipMalloc + hipFree cost 40 of its 50 ms.  Key: (class, bytes); class 1 / 2 = an fp32 / fp64 inverse factor W, whose
  // "zeros above the diagonal" survive a reuse in the same role only.
  std::map<std::pair<int, size_t>, std::vector<void*>> pool_free;
  std::map<void*, std::pair<int, size_t>> pool_live;
  size_t pool_bytes = 0;                       // bytes parked in pool_free
  size_t pool_cap = (size_t)48 << 30;          // lowered to a quarter of the device memory at context creation
  std::string err;
  ModelDev* h_model = nullptr;      // pinned: uploaded without a staging copy or a synchronisation
  void* hp_stage = nullptr; size_t hp_stage_bytes = 0;   // pinned staging (descriptors up, results down)
  hipEvent_t ev_upload = nullptr;   // last host->device copy out of the pinned buffers
  ModelDev* d_model = nullptr;
  void* d_mlp_w[HBO_MAX_MLP_LAYERS] = {nullptr};
  void* d_mlp_b[HBO_MAX_MLP_LAYERS] = {nullptr};
  size_t mlp_w_bytes[HBO_MAX_MLP_LAYERS] = {0};
  size_t mlp_b_bytes[HBO_MAX_MLP_LAYERS] = {0};
  int prof_level = 0;
  std::vector<ProfEntry> prof_pending;
  std::vector<hipEvent_t> prof_events; size_t prof_next = 0;   // event pool of the timing scopes
  std::vector<std::string> prof_names;
  std::vector<double> prof_ms;
  std::vector<int> prof_count;
  // RCCL
  void* rccl_lib = nullptr;
  void* comm = nullptr;
  int lds_per_block = 160 * 1024;   // hipDeviceProp_t::sharedMemPerBlock of the context's device (hbo_ctx_create)
  int opt_gram_mfma = 32;      // hbo_tune("gram_mfma"): fp32 Gram matrices of the stationary covariances with at least this many features take gram_mfma_kernel (0: never)
  int opt_small_fused = 1;     // hbo_tune("small_fused"): batches whose tasks all have n <= 128 take the single-workgroup evaluation (small.hip)
  int opt_spectral = 0;        // hbo_set_option("spectral"): stored for the Python layer, which routes its SVD call sites by it (hbo.h)
  int opt_acq_fused = 0;      // hbo_set_option("acq_fused"): stored for the Python layer, which routes value_and_grad of small caches to hbo_acq_grad_samples (hbo.h)
  int eig_last_sweeps = 0;     // outer Jacobi sweeps of the last hbo_sym_eig / hbo_nll_spectral (largest over its batches; eig.hip)
  int opt_post_serial = 0;     // hbo_tune("post_serial"): the streamed posterior's producer side (cross Gram) on the SAME stream as its products: isolated stage times
  int opt_spd_diag_bound = 0;  // hbo_tune("spd_diag_bound"), test hook: hbo_spd_solve reads max_i A_ii off its host matrix, so that it can take the f16x2 form
  int last_chol_form = 0;      // Fp32Form of the last run_potrf's trailing updates (hbo_get_option "chol_form")
  int last_post_resident = 0;  // the last posterior product (V = W Kxq: GEMM_POST, or post3.hip's) ran as a resident grid drawing tiles from a counter (hbo_get_option "post_resident")
  int last_inv_forms = 0;      // since the last run_potrf: 1 / 2 a level of the inverse ran on bf16x3 / f16x2 (trtri_level3), 4 / 8 K^-1 = W^T W did (hbo_get_option "inv_forms")
  int opt_fault_shard = 0;     // hbo_tune("fault_shard"): ONE-SHOT fault injection for the tests of the sharded objective's failure paths
  bool comm_aborted = false;   // set by comm_abort: sharded calls fail with HBO_ERR_COMM until hbo_comm_init builds a new communicator
  double* d_comm_buf = nullptr;
  int comm_buf_count = 0;
};

// The one error check of the host code: a failing HIP call leaves "<call> failed: <why> (<file>:<line>)" as the context's error (or as the
// ctx-less one), runs `action` -- what the caller has to undo: cleanup(), bail(...), nothing -- and returns HBO_ERR_HIP.
#define HIPCHK_OR(ctx, call, action)                                                          \
  do {                                                                                        \
    hipError_t e__ = (call);                                                                  \
    if (e__ != hipSuccess) {                                                                  \
      char buf__[512];                                                                        \
      snprintf(buf__, sizeof buf__, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__),   \
               __FILE__, __LINE__);                                                           \
      if (ctx) (ctx)->err = buf__; else hbo_g_err = buf__;                                        \
      action;                                                                                 \
      return HBO_ERR_HIP;                                                                     \
    }                                                                                         \
  } while (0)
#define HIPCHK(ctx, call) HIPCHK_OR(ctx, call, (void)0)

static inline int fail(hbo_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg; else hbo_g_err = msg;
  return code;
}
