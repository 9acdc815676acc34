// Launch schedules of the blocked factorisation, the block-recursive inverse and K^-1 = W^T W (sched.hip).
#pragma once
#include "runtime.h"

// progress of the block-recursive inverse (see trtri_advance)
struct TrtriProgress { int diag = 0; int a[12] = {0}; int b[12] = {0}; };

// The one-sweep inverse (sweep_advance): W = L^-1 and K^-1 = W^T W built row group by row group BEHIND the panel chain, so that
// what is left when the factorisation ends is one group's worth of O(N^2 q) work instead of the O(N^3) tail of the block-recursive
// inverse and of K^-1 = W^T W (which needs every row of W).
struct SweepState {
  int qs = 4; int done = 0; TrtriProgress pg;
  int nev = 0;                                   // events of ev_pool_sweep used so far
  // behind the last processed group's (c) and (d), and the streams they ran on: a later call on ANOTHER stream (the tail behind the
  // factorisation, on the main stream) waits for (c) before its (a) / (b) and for (d) only before its own (d)
  hipEvent_t ev_c = nullptr, ev_d = nullptr;
  hipStream_t st_c = nullptr, st_d = nullptr;
};
int sweep_group(int ntasks, int max_nblk);   // row-group size of the one-sweep inverse where use_sweep() says yes

hipEvent_t pool_event(hbo_ctx* c, size_t i);
// Look-ahead (panel chain, bulk update and inverse on separate streams) pays once there is something to overlap; below that the
// events and cross-stream waits cost more than they hide.  Measured (NLL+grad, look-ahead on / off, ms): one matrix of 2 / 8 / 16 / 20 /
// 24 blocks: 0.282 / 0.253, 0.714 / 0.682, 1.362 / 1.328, 1.724 / 1.741, 2.154 / 2.204; 64 tasks of 2 / 4 / 6 / 12 blocks: 0.344 / 0.298,
// 0.790 / 0.761, 1.569 / 1.598, 6.89 / 7.05; 8 tasks of 4 / 8 / 12 / 16-19 blocks: 0.457 / 0.415, 0.847 / 0.827, 1.508 / 1.591, 3.34 / 3.61.
// Option lookahead: 0 = never, 1 = this rule (default), 2 = whenever there is more than one block.
static inline bool use_lookahead(const hbo_ctx* c, int ntasks, int max_nblk) {
  if (!c->opt_lookahead || max_nblk <= 1) return false;
  if (c->opt_lookahead >= 2) return true;
  return max_nblk > 4 && (max_nblk >= 18 || (int64_t)ntasks * max_nblk >= 80);
}
// The block-recursive inverse starts beside the panel chain (run_potrf's `early`) where there is a chain to run beside and at least
// one early piece (four final panels) to hand over.  Option overlap_trtri: 0 = never.
static inline bool use_early_trtri(const hbo_ctx* c, int ntasks, int max_nblk) {
  return use_lookahead(c, ntasks, max_nblk) && c->opt_overlap_trtri && max_nblk >= 4;
}
// Every decision of one blocked factorisation (sched.hip: potrf_plan has the measurements behind each value).
enum YieldMode { YIELD_NONE, YIELD_POTF2, YIELD_CHAIN };     // who announces itself in the per-CU yield table: nobody / potf2 / the chain's wide kernels too
enum Fp32Form { FORM_MFMA, FORM_BF16X3, FORM_F16X2 };        // trailing updates: fp32 MFMA (and all of fp64) / three-way bf16 split / two-way fp16 split
struct PotrfPlan {
  bool la;            // look-ahead: the panel chain on its own stream, the bulk update beside it
  int q, q_inner;     // panels per trailing update; panels per inner group of the chain's column updates (0: one level)
  int persist_free;   // CUs the resident bulk update leaves to the panel chain
  int tgran, early_at;   // the early inverse gets its work after every tgran-th panel, and after panel early_at (-1: never)
  YieldMode yield;
  bool split_f1;      // F1's later block columns on the third stream
  Fp32Form form;
  bool h2_scales;     // the f16x2 products of the inverse and of K^-1 = W^T W get their measured-maximum words
};
PotrfPlan potrf_plan(const hbo_ctx* c, int dtype, int ntasks, int max_nblk, bool sweep);
void run_potrf(hbo_ctx* c, int dtype, const TaskDesc* d_tasks, int ntasks, int max_nblk, int* d_info, TrtriProgress* early = nullptr,
               SweepState* sweep = nullptr);
// does the objective pipeline of this shape take the one-sweep inverse?  (sched.hip)
bool use_sweep(const hbo_ctx* c, int dtype, int ntasks, int max_nblk);
// every row group whose block columns [.., cfin) are final and that was not swept before; `w_done` (optional): recorded on `st`
// as soon as W is complete (behind the last group's rows), so that alpha = W^T z can start beside the last K^-1 update
void sweep_advance(hbo_ctx* c, int dtype, const TaskDesc* d_tasks, int ntasks, int max_nblk, int cfin, hipStream_t st, SweepState& sw,
                   hipEvent_t w_done = nullptr);
void trtri_advance(hbo_ctx* c, int dtype, const TaskDesc* d_tasks, int ntasks, int max_nblk, int cfin, hipStream_t st, TrtriProgress& pg,
                   int max_s = 1 << 30);
void run_trtri(hbo_ctx* c, int dtype, const TaskDesc* d_tasks, int ntasks, int max_nblk, TrtriProgress* pg = nullptr);
void run_lauum(hbo_ctx* c, int dtype, const TaskDesc* d_tasks, int ntasks, int max_nblk, hipStream_t st = nullptr);
