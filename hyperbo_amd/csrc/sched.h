// Launch schedules of the blocked factorisation, the block-recursive inverse and K^-1 = W^T W (sched.hip), and their plans: potrf_plan
// and inv_plan answer "what does the factorisation / the inverse of this shape do" from the options and the shape alone, as inline
// host code that a stand-alone program can check (tools/inverse_plan_check.cpp).
#pragma once
#include "runtime.h"

#include <algorithm>

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
// Matrices of up to this many 128-blocks take 64 x 64 GEMM tiles in the inverse, K^-1 = W^T W and the sweep (option small_nblk; auto:
// fp64 48 -- tools/scan_thresholds.py, profiles/r05_sched_thresholds.md: 40 / 48 at N = 6144 (48 blocks) 5.73 / 5.64 ms, equal below, 64 loses at 56 blocks --
// fp32 32, where the larger matrices' products move to the bf16 cores instead)
static inline int small_limit(const hbo_ctx* c, int dtype) { return c->opt_small_nblk >= 0 ? c->opt_small_nblk : (dtype == HBO_F64 ? 48 : 32); }
// Batches: the sweep's launches beside the panel chain as plain grids (0), persistent and slot-limited over tiles x tasks from one
// counter (1), also polling the chain's yield table (2).  Auto: persistent up to 8 tasks -- measured with the pipelined cores, ms per
// NLL + gradient, plain / persistent: 4 tasks 1.781 / 1.747, 8 tasks 2.521 / 2.442, 16 tasks 4.200 / 4.223, 32 tasks 7.520 / 7.603,
// 64 tasks 14.13 / 14.31
static inline int batch_bg(const hbo_ctx* c, int ntasks) { return c->opt_batch_bg >= 0 ? c->opt_batch_bg : (ntasks <= 8 ? 1 : 0); }
// Does a caller that wants W and K^-1 beside the chain take the one-sweep inverse (sched.hip: sweep_advance)?
// Option sweep: 0 = never, 1 = this rule (default), 2 = wherever look-ahead is on and there are eight blocks.
static inline bool use_sweep(const hbo_ctx* c, int dtype, int ntasks, int max_nblk) {
  if (!c->opt_sweep || !use_lookahead(c, ntasks, max_nblk) || max_nblk < 8) return false;
  if (c->opt_sweep >= 2) return true;
  // one matrix: at N = 8192 the rank-q updates of this form run at a lower rate than the long-K products of the recursive inverse
  // and of K^-1 = W^T W, and the phase has no idle machine to give them (13.4 against 11.5 ms in round 4's first measurement; with
  // the pipelined GEMM cores 11.14 against 10.71 at q = 16).  In between it wins -- fp64, ms per NLL + gradient, recursive / sweep:
  //   N = 2048 1.193 / 1.193, 2560 1.580 / 1.417 (q = 4), 3072 1.944 / 1.740 (4), 3584 2.261 / 2.167 (4), 4096 2.780 / 2.671 (8),
  //   5120 4.404 / 4.179 (8), 6144 6.053 / 6.010 (8)        (profiles/r04_gemm_pipeline.md)
  // (fp32, one matrix: never -- beyond the small sizes the block-recursive products and K^-1 run on the bf16 matrix cores (post3.hip),
  //  which this form does not)
  return ntasks != 1 || (dtype == HBO_F64 && max_nblk > 16 && max_nblk <= 48);
}
static inline int sweep_group(int ntasks, int max_nblk) { return (ntasks == 1 && max_nblk > 28) ? 8 : 4; }   // its row-group size

// ---- the placement rule of the resident grids ----------------------------------------------------------------------------------
// A launch with more tiles than the machine has slots can run as a resident grid whose workgroups draw tiles from a zeroed counter:
//   beside the panel chain, if it has more tiles than that: two workgroups on all but `free_cus` CUs -- the panel kernels beside it
//     always find a CU with room (see trtri_level) -- with a counter of `pool`;
//   otherwise, where the caller allows the whole-machine form and the launch has at least `whole_min` tiles: two workgroups on all
//     but `whole_free` CUs, with a counter of `whole_pool` or (null) one of those kept for the launches behind the factorisation.
// A launch that gets no counter stays a plain grid, unless `static_ok`: the workgroups then stride over the tiles (GemmArgs).
// The callers' differences are recorded in profiles/sched_refactor.md.
struct GridRule {
  bool beside = false; int free_cus = 0; TileCounters* pool = nullptr;
  bool whole = false; int64_t whole_min = 0; int whole_free = 0; TileCounters* whole_pool = nullptr;
  bool static_ok = false;
};

// ---- the plan of the inverse side ----------------------------------------------------------------------------------------------
// Every decision of W = L^-1 and K^-1 = W^T W for one shape, made once: no HIP call, no allocation, nothing of hbo_ctx::run.  What
// only the launch knows -- the stream it is on, whether this factorisation has side counters, a yield table or measured f16x2
// words, whether a workspace could be had, how many post-pool counters the call has taken -- is combined with it where the launch
// is made (inv_grid, level_grid and the two *_small_tiles below; sched.hip).
enum InvWant { INV_NONE, INV_W, INV_W_KINV };   // what the caller needs behind the factorisation
constexpr int INV_NEVER = 1 << 30;
struct InvPlan {
  // the route: one-sweep (row groups of qs blocks) or block-recursive, the latter started beside the chain or behind it
  bool sweep; int qs; bool early;
  bool small_shape;    // 64-tiles throughout (max_nblk <= small_limit)
  int few_tiles;       // a level of the recursive inverse with fewer 128-tiles than this takes 64-tiles whatever the shape
  int lvl3_min_s;      // fp32, one matrix: levels s >= this run on the 16-bit matrix cores (post3.hip); INV_NEVER: none does
  bool kinv3;          // K^-1 = W^T W on the 16-bit cores
  // where each kind of launch may run as a resident grid, as the policy half of a GridRule (no counters yet: inv_grid): the
  // levels of the recursive inverse (the 16-bit form as it stands; the fp32 / fp64 form only on 128-tiles and twice per call behind the
  // factorisation), the sweep's (b) (c) (d), K^-1 = W^T W
  GridRule level, swept, kinv;
  int batch_bg;        // batches: see batch_bg() -- 2 also makes the chain keep its yield table (potrf_plan)
  int sweep_big;       // a sweep launch of a small shape with at least this many 128-tiles (x tasks) runs on 128-tiles
  bool d_own_stream;   // the sweep's K^-1 updates (d) on the third stream
};
// host_desc: a host copy of the single task's descriptor is at hand (the 16-bit forms split their operands by host-side pointers).
// beside_chain: the caller lets the inverse start while the factorisation runs (hbo_spd_solve and value-only evaluations do not).
static inline InvPlan inv_plan(const hbo_ctx* c, int dtype, int ntasks, int max_nblk, InvWant want, bool host_desc, bool beside_chain = true) {
  InvPlan p = {};
  const bool one = ntasks == 1;
  p.sweep = beside_chain && want == INV_W_KINV && use_sweep(c, dtype, ntasks, max_nblk);
  p.qs = !p.sweep ? 0 : (c->opt_sweep_qs > 0 ? c->opt_sweep_qs : sweep_group(ntasks, max_nblk));
  // the block-recursive inverse starts beside the panel chain where there is a chain to run beside and at least one early piece (four
  // final panels) to hand over.  Option overlap_trtri: 0 = never.
  p.early = beside_chain && want != INV_NONE && !p.sweep && use_lookahead(c, ntasks, max_nblk) && c->opt_overlap_trtri && max_nblk >= 4;
  // few or short tiles (small levels, small / batched matrices): 64x64 tiles -- a lone 128-tile runs its K loop latency-bound, four
  // 64-tiles expose 4x the parallelism for the same flops
  p.small_shape = max_nblk <= small_limit(c, dtype);
  p.few_tiles = 600;
  // fp32, one matrix beyond the small sizes: both operands of each product split exactly into bf16 / fp16 planes
  const bool cores16 = dtype == HBO_F32 && one && host_desc && !p.small_shape;
  p.lvl3_min_s = (cores16 && c->opt_trtri_bf16x3) ? c->opt_trtri3_min_s : INV_NEVER;
  p.kinv3 = cores16 && c->opt_lauum_bf16x3;
  p.batch_bg = batch_bg(c, ntasks);
  // products that co-run with the panel chain (single matrix, side stream): persistent, 2 workgroups on all but `trtri_free` CUs,
  // tiles from a counter; behind the factorisation, one large matrix: the big levels as a resident grid over the whole machine
  // (the dispatcher spreads a grid over the CUs breadth-first, so "free CUs" really means free room on every CU: a panel
  //  kernel (potf2 78 KB, trsm 87 KB of LDS, 128 VGPRs) fits beside ONE 128-tile workgroup (72 KB) or TWO 64-tile
  //  workgroups (2 x 40 KB), not beside more -- with 4 x (CUs - free) 64-tile workgroups every CU held three or four of
  //  them and potf2 waited 330 us for the whole launch to end: rocprofv3 kernel trace, profiles/r02_potrf_chain.md)
  p.level = {one && c->opt_trtri_free > 0, c->opt_trtri_free, nullptr, one && c->opt_lauum_persist != 0, 4 * (int64_t)c->n_cus, 0};
  // (the sweep's launches leave fewer CUs free than the recursive inverse's big products: N = 5120 3.785 -> 3.70 ms at 16-32 instead of 48)
  p.swept = {c->opt_trtri_free > 0 && (one || p.batch_bg >= 1), std::min(c->opt_trtri_free, c->opt_sweep_free)};
  // one large matrix: a resident grid of two workgroups per CU draws the tiles from a counter (gemm.hip: launch_gemm_t)
  // (16 CUs stay free for alpha = W^T z and d nll / d mu, which run beside this launch on the panel stream: isolated the
  //  launch takes the same time with 480 as with 512 workgroups)
  p.kinv = {false, 0, nullptr, one && !p.small_shape && c->opt_lauum_persist != 0, 4 * (int64_t)c->n_cus + 1, c->opt_lauum_persist > 1 ? c->opt_lauum_persist : 16};
  p.sweep_big = c->opt_sweep_big;
  // (d) has no successor but the next group's (d) and the final consumers of K^-1: on a stream of its own it runs beside the
  // (a) -> (b) -> (c) chain of the following groups instead of holding it up.  Measured (ms, same stream / own stream): one matrix on
  // 128-tiles N = 5120 4.26 / 4.15, 6144 6.07 / 5.71, 7168 8.39 / 7.96, 8192 11.44 / 10.97; on 64-tiles N = 2560 1.43 / 1.48,
  // 4096 2.65 / 2.79; batches 14.11 / 14.48 (64 tasks), 2.57 / 2.74 (8): where the launches are small the extra hop costs more
  p.d_own_stream = c->opt_sweep_side && c->stream3 && one && !p.small_shape;
  return p;
}
// a site's rule at launch time: beside the chain only on the side stream of a factorisation that has counters at hand
static inline GridRule inv_grid(GridRule r, bool on_side_stream, TileCounters* side) {
  r.beside = r.beside && on_side_stream && side->base; r.pool = side; return r;
}
static inline bool level_small_tiles(const InvPlan& p, int64_t tiles128) { return p.small_shape || tiles128 < p.few_tiles; }
// a level's fp32 / fp64 launch: behind the factorisation only the big levels are resident grids, like K^-1 = W^T W (run_lauum), and
// the counters below the very last one are kept for this -- at most two launches of a call (`post_taken` so far) take one
static inline GridRule level_grid(const InvPlan& p, bool small_tiles, int post_taken, bool on_side_stream, TileCounters* side) {
  GridRule r = inv_grid(p.level, on_side_stream, side); r.whole = r.whole && !small_tiles && post_taken < 2; return r;
}
// (the sweep: 64-tiles for small / batched matrices as everywhere else -- except where a launch has enough 128-tiles to fill the machine
//  several times over: all tiles of a sweep launch have the same K, so the larger tile's better MFMA rate is not lost in a tail)
static inline bool sweep_small_tiles(const InvPlan& p, int64_t tiles128) { return p.small_shape && tiles128 < p.sweep_big; }

// progress of the block-recursive inverse (see trtri_advance)
struct TrtriProgress { int diag = 0; int a[12] = {0}; int b[12] = {0}; };
// The one-sweep inverse (sweep_advance): W = L^-1 and K^-1 = W^T W built row group by row group BEHIND the panel chain, so that
// what is left when the factorisation ends is one group's worth of O(N^2 q) work instead of the O(N^3) tail of the block-recursive
// inverse and of K^-1 = W^T W (which needs every row of W).
struct SweepState {
  int done = 0;
  int nev = 0;                                   // events of ev_pool_sweep used so far
  // behind the last processed group's (c) and (d), and the streams they ran on: a later call on ANOTHER stream (the tail behind the
  // factorisation, on the main stream) waits for (c) before its (a) / (b) and for (d) only before its own (d)
  hipEvent_t ev_c = nullptr, ev_d = nullptr;
  hipStream_t st_c = nullptr, st_d = nullptr;
};
// One call's inverse side: what it runs on, its plan, and how far it has come.  Made by the caller of run_potrf, which hands pieces
// to it while the chain runs; the same object then goes to run_trtri / sweep_advance and run_lauum behind the factorisation.
struct InvRun {
  hbo_ctx* c; int dtype; const TaskDesc* d_tasks; int ntasks, max_nblk;
  const TaskDesc* host;   // host copy of the single task's descriptor (pointers, ld), null for batches: must outlive the last launch call
  InvPlan pl;
  TrtriProgress pg;       // of the recursive inverse, or of the sweep's diagonal groups
  SweepState sw;
};
static inline InvRun inv_run(hbo_ctx* c, int dtype, const TaskDesc* d_tasks, int ntasks, int max_nblk, const TaskDesc* host, InvWant want, bool beside_chain = true) {
  return {c, dtype, d_tasks, ntasks, max_nblk, host, inv_plan(c, dtype, ntasks, max_nblk, want, host != nullptr, beside_chain)};
}

// Every decision of one blocked factorisation (potrf_plan below has the measurements behind each value).
enum YieldMode { YIELD_NONE, YIELD_POTF2, YIELD_CHAIN };     // who announces itself in the per-CU yield table: nobody / potf2 / the chain's wide kernels too
enum Fp32Form { FORM_MFMA, FORM_BF16X3, FORM_F16X2 };        // trailing updates: fp32 MFMA (and all of fp64) / three-way bf16 split / two-way fp16 split
struct PotrfPlan {
  bool la;            // look-ahead: the panel chain on its own stream, the bulk update beside it
  int q, q_inner;     // panels per trailing update; panels per inner group of the chain's column updates (0: one level)
  int persist_free;   // CUs the resident bulk update leaves to the panel chain
  int syrk3_free;     // the same for the bulk update on the bf16 / fp16 cores
  bool bulk_whole;    // a large trailing matrix's bulk update as a resident grid over the whole machine
  int tgran, early_at;   // the early inverse gets its work after every tgran-th panel, and after panel early_at (-1: never)
  YieldMode yield;
  bool split_f1;      // F1's later block columns on the third stream
  Fp32Form form;
  bool h2_scales;     // the f16x2 products of the inverse and of K^-1 = W^T W get their measured-maximum words
};
// ---- the plan of one factorisation ---------------------------------------------------------------------------------------------
// Every decision of run_potrf, made once, from the options and the shape alone (no HIP call).  Whether the workspaces of a product
// form can be had is not policy: potrf_setup falls back where an allocation fails.  inv: the plan of the inverse that runs beside this
// factorisation, or null.
static inline PotrfPlan potrf_plan(const hbo_ctx* c, int dtype, int ntasks, int max_nblk, const InvPlan* inv) {
  PotrfPlan pl = {};
  // (a single block column has no trailing matrix to look ahead over: it stays on the caller's stream)
  // (without look-ahead -- small problems, see use_lookahead -- there is no chain / bulk distinction to group for: one panel per
  //  trailing update, the plain right-looking form: N = 512 / 1024 / 2048: 0.399 -> 0.383, 0.686 -> 0.654, 1.33 -> 1.28 ms; up to
  //  eight tasks -- 64 tasks of 4 blocks: 0.761 with groups of three, 0.796 with one)
  pl.la = use_lookahead(c, ntasks, max_nblk);
  // fp32: every trailing update on the bf16 matrix cores from an exact three-way split of the group's panels (post3.hip:
  // syrk3_kernel; 1.4x the fp32-MFMA rate at fp32 accuracy) ... or, when the caller knows the largest diagonal entry (|L_ij| <=
  // sqrt(max A_ii) gives the panels' scale without a pass), on the fp16 cores from a TWO-way split: three MFMAs per product instead
  // of six (Syrk3Args::h2)
  const bool s3 = dtype == HBO_F32 && c->opt_syrk_bf16x3;
  // (the inverse's f16x2 levels and K^-1 = W^T W take their measured scales whatever form the trailing updates have)
  pl.h2_scales = dtype == HBO_F32 && c->opt_chol_f16x2 && c->run.chol_diag_bound > 0;
  pl.form = (s3 && max_nblk > 1) ? (pl.h2_scales ? FORM_F16X2 : FORM_BF16X3) : FORM_MFMA;
  // panels per trailing update and CUs the persistent bulk update leaves to the panel chain.  Measured (NLL+grad, ms):
  //   N = 4096: (4, 32) 3.61, (3, 32) 3.54, (3, 64) 3.51;   N = 8192: (4, 32) 13.49, (3, 32) 13.34, (3, 64) 13.25,
  //   (3, 96) 13.43, (2, 64) 13.57, (5, 32) 13.61;   N = 16384: (4, 32) 78.4, (3, 32) 79.1, (3, 64) 79.5
  const bool small_mat = max_nblk <= 96;
  //   round 2, N = 65536: group 4 / 6 / 8 / 12 / 16: 60.2 / 60.7 / 62.0 / 62.6 / 62.0 TFLOP/s; N = 32768: 4 / 6 / 8: 56.8 / 57.2 / 57.9; N = 16384: 48.1 / 47.4 / 47.8
  //   round 3, fp32 with the updates on the bf16 cores, N = 16384 (factor, ms): group 4 / 5 / 6 / 7 / 8: 23.1 / 22.5 / 22.3 / 22.4 / 22.0
  const bool s3_large = s3 && !small_mat;
  //   round 5 (tools/ab_suite.py; fp64 one matrix, group 3 / 5 / 6 / 7 / 8): N = 8192 10.57 / 10.54 / 10.58 / 10.56 / 10.56 (flat), 12288 31.98 / 31.21 / 31.16 /
  //   30.97 / 31.02; fp32 with the trailing updates on the fp16 cores (they are short: the chain and the launch count decide): N = 8192 group 3 / 6 / 8 / 12
  //   6.09 / 5.82-5.87 / 5.92 / 6.16-6.19; N = 16384 (factor, ms) 8 / 12 / 16 18.5 / 18.3-18.5 / 18.7-19.0 and, with two-level groups (outer / inner: see
  //   q_inner below), 16 / 8 18.0-18.2, 12 / 6 18.2-18.5, 8 / 4 18.6
  const int q_small = (s3 && ntasks == 1 && max_nblk >= 56) ? 6 : ((ntasks == 1 && max_nblk > 64) ? 7 : 3);
  pl.q = c->opt_group > 0 ? c->opt_group : ((!pl.la && ntasks <= 8) ? 1 : (small_mat ? q_small : (s3_large ? 16 : (max_nblk >= 256 ? 8 : 4))));
  // two-level groups (group_inner = qi, 0 < qi < q): the chain's column updates stay short -- inside the inner group [gi, gi + qi) --
  // and at every inner boundary ONE update brings the group's remaining columns up to date with the inner group just finished
  // (K = 128 qi, on the chain); the trailing updates F1 / F2 keep the outer group's K = 128 q
  const int q_inner = c->opt_group_inner >= 0 ? c->opt_group_inner : ((s3_large && pl.q == 16) ? 8 : 0);
  pl.q_inner = (q_inner > 0 && q_inner < pl.q) ? q_inner : 0;
  //   with the CU yield (below): N = 8192 (3, 64) 12.58, (3, 48) 12.52, (3, 32) 12.61, (3, 16) 13.24, (4, 48) 12.66
  //   round 2 (chain kernels mark their CUs, background workgroups there pause): 32 beats 48 at N = 8192 (11.73 / 11.81)
  pl.persist_free = c->opt_persist_free >= 0 ? c->opt_persist_free : 32;
  // (on the bf16 / fp16 cores: two workgroups on all but `syrk3_free` CUs, the panel kernels beside it always find a CU with room)
  pl.syrk3_free = c->opt_syrk3_free;
  // (for large trailing matrices the bulk update dominates and gets the whole machine, but still as a resident grid drawing
  //  tiles from the counter: see launch_gemm_t, LAUUM)
  pl.bulk_whole = c->opt_lauum_persist != 0;
  // (measured: batches gain -- 64 tasks 14.32 -> 14.12 ms, the 8-task shard 2.60 -> 2.53; one matrix does not -- N = 8192
  //  factorisation 5.35 -> 5.41, N = 4096 2.63 -> 2.68: the two cross-stream hops cost what the shorter launch saves)
  pl.split_f1 = pl.la && c->stream3 && (c->opt_split_f1 >= 2 || (c->opt_split_f1 == 1 && ntasks > 1));
  // early inverse: a batch takes every piece as soon as four more panels are final (16.9 against 17.35 ms for 64 tasks
  // of ~2000 points, 3.77 against 3.92 for 8); one large matrix only at half time -- more launches on the side stream
  // take slots from the panel chain (N = 8192: 13.63 ms at 32 panels, 13.8 at 4, 14.0 at 2)
  pl.tgran = 4;
  // (one large matrix, measured later with the CU yield below: a single call after 13/16 of the panels instead of half --
  //  N = 8192, call after panel 32 / 40 / 44 / 48 / 52 / 56 / 60: 12.42 / 12.37 / 12.34 / 12.25 / 12.21 / 12.30 / 12.50 ms)
  pl.early_at = -1;   // single-task form: the one panel count after which the side stream gets its work
  if (ntasks == 1) {
    // (round 2, with the persistent / yielding forms of the co-running products -- they no longer stall the chain --
    //  N = 8192, (start after panel, CUs left free by the inverse, by the bulk update): (40, 48, 32) 11.73 ms,
    //  (36, 64, 32) 11.74, (40, 32, 32) 11.80, (44, 48, 32) 11.92, (52, 16, 48) 12.27, (48, 96, 32) 12.37)
    pl.early_at = c->opt_trtri_at > 0 ? std::min(c->opt_trtri_at * max_nblk / 64, max_nblk - 1) : (max_nblk * 5 / 8) & ~3;
    if (pl.early_at < 4) pl.early_at = -1;
    pl.tgran = 1 << 30;
  }
  // CU yield (up to 96 blocks: N = 4096 3.37 -> 3.29 ms, N = 8192 12.61 -> 12.52; N = 16384 loses 0.9 % to the polling)
  // fp32 with the trailing updates on the bf16 cores: the bulk update is 1.5x shorter and the panel chain sets the pace at
  // every size, so the chain's kernels are protected as for the small matrices
  const bool batch_yield = ntasks > 1 && inv && inv->sweep && inv->batch_bg >= 2;
  const bool yield = pl.la && c->opt_cu_yield && ((ntasks == 1 && (small_mat || pl.form != FORM_MFMA)) || batch_yield);
  pl.yield = !yield ? YIELD_NONE : (c->opt_cu_yield >= 2 ? YIELD_CHAIN : YIELD_POTF2);   // (CHAIN: the chain's wide kernels mark their CUs too)
  return pl;
}

void run_potrf(hbo_ctx* c, int dtype, const TaskDesc* d_tasks, int ntasks, int max_nblk, int* d_info, InvRun* inv = nullptr);
// every row group whose block columns [.., cfin) are final and that was not swept before; `w_done` (optional): recorded on `st`
// as soon as W is complete (behind the last group's rows), so that alpha = W^T z can start beside the last K^-1 update
void sweep_advance(InvRun& r, int cfin, hipStream_t st, hipEvent_t w_done = nullptr);
void trtri_advance(InvRun& r, int cfin, hipStream_t st, int max_s = 1 << 30);
void run_trtri(InvRun& r);   // what is left of the recursive inverse, on the main stream
void run_lauum(InvRun& r);   // K^-1 = W^T W, on the main stream
