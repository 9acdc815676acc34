// Launch schedules: the right-looking blocked Cholesky with look-ahead (panel chain on its own stream, bulk trailing update
// persistent beside it), the block-recursive inverse W = L^-1 walked while the factorisation still runs, and K^-1 = W^T W.
// Everything here launches WHICH kernels of gemm.hip / chol.hip the plans of sched.h (potrf_plan, inv_plan) chose, on WHICH stream
// in WHAT order, and adds what only a launch knows; no option is read here.  The measurements behind the choices are in
// profiles/r01_potrf_chain.md and profiles/r02_potrf_chain.md.
#include "sched.h"

#include <cmath>

// ---- debug timeline (-DHBO_TIMELINE builds only; tools/timeline.py) ----------------------------------------------------------------
// Every tagged launch gets a pair of device words [first workgroup start, last workgroup end] (100 MHz wall clock) and a host-side
// label; hbo_dbg_timeline(1) starts a recording, hbo_dbg_timeline(0, times, names, ps) ends it and copies everything out.
#ifdef HBO_TIMELINE
namespace {
constexpr int TL_MAX = 16384;
unsigned long long* g_tl_dev = nullptr;
int g_tl_n = 0;
bool g_tl_on = false;
struct TlEntry { char name[16]; int p; };
TlEntry g_tl_entries[TL_MAX];
}
unsigned long long* tl_slot(const char* name, int p) {
  if (!g_tl_on || g_tl_n >= TL_MAX) return nullptr;
  strncpy(g_tl_entries[g_tl_n].name, name, 15); g_tl_entries[g_tl_n].name[15] = 0;
  g_tl_entries[g_tl_n].p = p;
  return g_tl_dev + 2 * g_tl_n++;
}
extern "C" int hbo_dbg_timeline(int begin, unsigned long long* times, char* names, int* ps) {
  if (begin) {
    if (!g_tl_dev && hipMalloc(reinterpret_cast<void**>(&g_tl_dev), sizeof(unsigned long long) * 2 * TL_MAX) != hipSuccess) return -1;
    static unsigned long long init[2 * TL_MAX];
    for (int i = 0; i < TL_MAX; ++i) { init[2 * i] = ~0ull; init[2 * i + 1] = 0; }
    hipMemcpy(g_tl_dev, init, sizeof init, hipMemcpyHostToDevice);
    g_tl_n = 0; g_tl_on = true;
    return 0;
  }
  g_tl_on = false;
  hipDeviceSynchronize();
  if (times) hipMemcpy(times, g_tl_dev, sizeof(unsigned long long) * 2 * g_tl_n, hipMemcpyDeviceToHost);
  for (int i = 0; i < g_tl_n; ++i) { if (names) memcpy(names + 16 * i, g_tl_entries[i].name, 16); if (ps) ps[i] = g_tl_entries[i].p; }
  return g_tl_n;
}
#else
unsigned long long* tl_slot(const char*, int) { return nullptr; }
#endif

// ---- blocked factorisation drivers -----------------------------------------------------------

static hipEvent_t event_of(std::vector<hipEvent_t>& pool, size_t i) {
  while (pool.size() <= i) {
    hipEvent_t ev;
    hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    pool.push_back(ev);
  }
  return pool[i];
}
hipEvent_t pool_event(hbo_ctx* c, size_t i) { return event_of(c->ev_pool, i); }


// ---- the resident grids (sched.h: GridRule) -----------------------------------------------------------------------------------
static int* take_counter(TileCounters* t) { return (t && t->base && t->next < t->limit) ? t->base + t->next++ : nullptr; }
// A zeroed tile counter for a resident launch BEHIND the factorisation (the big levels of the inverse, K^-1 = W^T W): run_potrf clears the
// whole counter array once per factorisation, and these launches take the words of its top region in turn -- each used to clear its
// own word with a fill kernel on its stream first (6.5 us + a launch boundary, three of them on the tail of a cfg-2 evaluation).
static int* post_counter(hbo_ctx* c, hipStream_t st) {
  constexpr int POST_POOL = 400;
  int* counters = (int*)ws_get(c, WS_COUNTERS, sizeof(int) * HBO_N_COUNTERS);
  if (!counters) return nullptr;
  if (c->run.post_counter_next < POST_POOL) return counters + HBO_N_COUNTERS - 16 - c->run.post_counter_next++;
  int* p = counters + HBO_N_COUNTERS - 1;   // (pool exhausted: a word of its own, cleared on the spot)
  hipMemsetAsync(p, 0, sizeof(int), st);
  return p;
}
// (GemmArgs and Syrk3Args both carry the pair `persistent`, `work_counter`; they go to their kernels by value and stay as they are)
template <typename Args>
static void resident_grid(hbo_ctx* c, Args& a, const GridRule& r, int64_t tiles, hipStream_t st) {
  a.persistent = 0; a.work_counter = nullptr;
  if (r.beside) {
    const int pblocks = 2 * (c->n_cus - r.free_cus);
    if (tiles > pblocks && ((a.work_counter = take_counter(r.pool)) || r.static_ok)) a.persistent = pblocks;
  } else if (r.whole && tiles >= r.whole_min) {
    if ((a.work_counter = r.whole_pool ? take_counter(r.whole_pool) : post_counter(c, st)) || r.static_ok) a.persistent = 2 * (c->n_cus - r.whole_free);
  }
}

// ---- the steps of one factorisation --------------------------------------------------------------------------------------------
namespace {
// what the steps share: the call's arguments, the streams, the workspaces potrf_setup made, and the events in flight
struct PotrfState {
  hbo_ctx* c; int dtype; const TaskDesc* d_tasks; int ntasks, max_nblk; int* d_info;
  hipStream_t sm, sp;           // main stream (bulk updates: CU-masked queues of their own were measured slower); panel stream (= sm without look-ahead)
  int* yield_flag = nullptr;    // per-CU table the background launches poll, or null
  int* chain_mark = nullptr;    // the same table where the chain's wide kernels mark their CUs too, or null
  TileCounters bulk = {};       // one tile counter per bulk launch (dynamic tile assignment of the persistent form)
  Fp32Form form = FORM_MFMA;    // the plan's, or what the workspaces allow
  Syrk3Args s3a = {};
  unsigned short* s3buf[2] = {nullptr, nullptr};
  float* h2_aug = nullptr;
  size_t evi = 0;               // next event of ev_pool
  hipEvent_t ev_f1b = nullptr;  // behind the third-stream half of the last F1, until a launch of the chain has waited for it
  hipEvent_t ev_f2 = nullptr;   // behind the last bulk update
};
int tiles_of(const PotrfState& s, int c_lo, int c_hi) { int n = 0; for (int cc = c_lo; cc < std::min(c_hi, s.max_nblk); ++cc) n += s.max_nblk + 1 - cc; return n; }
void wait_f1b(PotrfState& s) { if (s.ev_f1b) { hipStreamWaitEvent(s.sp, s.ev_f1b, 0); s.ev_f1b = nullptr; } }

void potrf_setup(const PotrfPlan& pl, PotrfState& s) {
  hbo_ctx* c = s.c;
  s.yield_flag = pl.yield != YIELD_NONE ? c->d_yield : nullptr;
  if (s.yield_flag) hipMemsetAsync(s.yield_flag, 0, sizeof(int) * HBO_YIELD_TAB_ENTRIES, s.sm);
  s.chain_mark = pl.yield == YIELD_CHAIN ? s.yield_flag : nullptr;
  c->run.gemm_yield = s.yield_flag;
  // the tile counters, zeroed up front: the first for the bulk updates, the rest for the persistent inverse products beside the
  // chain (trtri_level, sweep_advance) and, from the top, the launches behind this factorisation (post_counter)
  int* counters = (int*)ws_get(c, WS_COUNTERS, sizeof(int) * HBO_N_COUNTERS);
  if (counters) hipMemsetAsync(counters, 0, sizeof(int) * HBO_N_COUNTERS, s.sm);
  s.bulk = {counters, 0, HBO_N_BULK_COUNTERS};
  c->run.side = {counters ? counters + HBO_N_BULK_COUNTERS : nullptr, 0, HBO_N_COUNTERS - HBO_N_BULK_COUNTERS - 512};
  c->run.post_counter_next = 0;
  // Each panel is split right behind its solve; two buffers alternate by group, because the bulk update of group g still reads its
  // panels while group g + 1 is being solved.
  s.form = pl.form;
  if (s.form != FORM_MFMA) {
    s.s3a.tasks = s.d_tasks; s.s3a.nkb = pl.q * (HBO_TILE / 16);
    s.s3a.task_stride = (int64_t)(s.max_nblk + 1) * s.s3a.nkb * 3 * (HBO_TILE * 16);
    const size_t bytes = sizeof(unsigned short) * (size_t)s.s3a.task_stride * s.ntasks;
    s.s3buf[0] = static_cast<unsigned short*>(ws_get(c, WS_SYRK3_A, bytes));
    s.s3buf[1] = static_cast<unsigned short*>(ws_get(c, WS_SYRK3_B, bytes));
    if (!s.s3buf[0] || !s.s3buf[1]) s.form = FORM_MFMA;
  }
  c->run.h2_words = nullptr;
  if (pl.h2_scales) {
    // measured maxima of the inverse's operands (trtri_level3, run_lauum), zeroed once per factorisation
    c->run.h2_words = static_cast<unsigned int*>(ws_get(c, WS_H2_SCALES, sizeof(unsigned int) * HBO_H2_WORDS));
    if (c->run.h2_words) hipMemsetAsync(c->run.h2_words, 0, sizeof(unsigned int) * HBO_H2_WORDS, s.sm);
  }
  if (s.form == FORM_F16X2) {
    // (the augmented tile-row carries measured scales per 16 rows x 64 columns, one array per panel buffer)
    s.form = FORM_BF16X3;
    if (c->run.h2_words) {
      s.s3a.aug_stride = (int64_t)(s.s3a.nkb / 4) * 8;
      s.h2_aug = static_cast<float*>(ws_get(c, WS_H2_AUG, sizeof(float) * 2 * (size_t)s.s3a.aug_stride * s.ntasks));
      if (s.h2_aug) { s.form = FORM_F16X2; s.s3a.h2 = 1; s.s3a.sx = s.s3a.sy = post2h_scale_for(std::sqrt(c->run.chol_diag_bound)); }
    }
  }
}

// inner boundary of a two-level group: the inner group [gi - qi, gi) just finished updates the group's remaining columns [gi, g1)
void step_inner_update(const PotrfPlan& pl, PotrfState& s, int g0, int g1, int gi, int p) {
  hbo_ctx* c = s.c;
  const int qi = pl.q_inner;
  if (s.form != FORM_MFMA) {   // the inner group just finished, as split planes (its rows below; blocks [gi - qi - g0 ..) of the buffer)
    ProfScope ps(c, "split3", 2, s.sp);
    Syrk3Args a = s.s3a; a.kcol0 = (gi - qi) * HBO_TILE; a.nk_split = qi * (HBO_TILE / 16); a.r_lo = gi; a.kb_off = (gi - qi - g0) * (HBO_TILE / 16);
    launch_split3_panel(a, s.max_nblk + 1 - gi, s.ntasks, s.sp);
  }
  wait_f1b(s);
  ProfScope ps(c, "syrk_inner", 2, s.sp);
  if (s.form != FORM_MFMA) {
    Syrk3Args a = s.s3a; a.kb_off = (gi - qi - g0) * (HBO_TILE / 16); a.nk = qi * (HBO_TILE / 16); a.c_lo = gi; a.c_hi = g1;
    a.yield_mark = s.chain_mark;
    launch_syrk3(a, tiles_of(s, gi, g1), s.ntasks, s.sp);
  } else {
    GemmArgs a = {}; a.tasks = s.d_tasks; a.mode = GEMM_SYRK; a.p0 = gi - qi; a.kt = qi; a.c_lo = gi; a.c_hi = g1; a.aug = 1;
    a.small_tiles = (int64_t)(s.max_nblk + 1 - gi) * (g1 - gi) * s.ntasks < 600;
    a.yield_mark = s.chain_mark; a.tl = tl_slot("syrk_inner", p);
    launch_gemm(s.dtype, a, dim3(s.max_nblk + 1 - gi, g1 - gi, s.ntasks), s.sp);
  }
}
// left-looking update of block column p with the (inner) group's earlier panels [gi, p): on fp32 MFMA (64x64 tiles) in every form
void step_column_update(PotrfState& s, int gi, int p) {
  wait_f1b(s);   // (the previous group's contribution to this column)
  ProfScope ps(s.c, "syrk_col", 2, s.sp);
  GemmArgs a = {}; a.tasks = s.d_tasks; a.mode = GEMM_SYRK; a.p0 = gi; a.kt = p - gi; a.c_lo = p; a.c_hi = p + 1; a.aug = 1; a.small_tiles = 1;
  a.yield_mark = s.chain_mark; a.tl = tl_slot("syrk_col", p);
  launch_gemm(s.dtype, a, dim3(s.max_nblk + 1 - p, 1, s.ntasks), s.sp);
}
// diagonal block, panel solve and -- behind the group's last solve -- ONE split of the (inner) group's panels [gi, p] for the wide
// updates F1 / F2 (two-level groups: the earlier inner groups were split at their boundaries; the f16x2 split needs the augmented
// rows' maxima first, so it is a kernel of its own in every form)
void step_panel(PotrfState& s, int g0, int g1, int gi, int p) {
  hbo_ctx* c = s.c;
  { ProfScope ps(c, "potf2", 2, s.sp); launch_potf2(s.dtype, s.d_tasks, s.ntasks, p, s.d_info, s.sp, s.yield_flag, tl_slot("potf2", p)); }
  { ProfScope ps(c, "trsm", 2, s.sp); launch_trsm(s.dtype, s.d_tasks, s.ntasks, p, s.max_nblk, s.sp, s.chain_mark, tl_slot("trsm", p)); }
  if (s.form != FORM_MFMA && p + 1 == g1 && p + 1 < s.max_nblk) {
    ProfScope ps(c, "split3", 2, s.sp);
    Syrk3Args a = s.s3a; a.kcol0 = gi * HBO_TILE; a.nk_split = (p + 1 - gi) * (HBO_TILE / 16); a.r_lo = p + 1; a.kb_off = (gi - g0) * (HBO_TILE / 16);
    launch_split3_panel(a, s.max_nblk + 1 - (p + 1), s.ntasks, s.sp);
  }
}
// block columns 0..p of L are final: what the inverse can do with them goes to the side stream
// (the panel chain leaves most of the machine idle in the second half of the factorisation)
void step_hand_over(const PotrfPlan& pl, PotrfState& s, int p, InvRun* inv) {
  hbo_ctx* c = s.c;
  if (!inv || p + 1 >= s.max_nblk) return;
  const bool to_sweep = inv->pl.sweep && (p + 1) % inv->pl.qs == 0;   // the row group that ends here goes through the one-sweep inverse
  if (!to_sweep && !(inv->pl.early && ((p + 1) % pl.tgran == 0 || p + 1 == pl.early_at))) return;
  hipEvent_t e = pool_event(c, s.evi++);
  hipEventRecord(e, s.sp);
  hipStreamWaitEvent(c->stream4, e, 0);
  ProfScope ps(c, to_sweep ? "sweep_early" : "trtri_early", 1, c->stream4);
  if (to_sweep) sweep_advance(*inv, p + 1, c->stream4);
  else trtri_advance(*inv, p + 1, c->stream4);
}
// F1 (next group's block columns [g1, g2); without look-ahead the whole trailing matrix) is on the critical path: it is launched on
// the panel stream itself -- no cross-stream event hop before and after it -- once the previous bulk update, which wrote the same
// tiles, is done (ev_f2).
void step_f1(const PotrfPlan& pl, PotrfState& s, int g0, int g1, int g2) {
  hbo_ctx* c = s.c;
  GemmArgs a = {}; a.tasks = s.d_tasks; a.mode = GEMM_SYRK; a.p0 = g0; a.kt = g1 - g0; a.aug = 1;
  // F1 is a chain kernel: it marks its CUs instead of polling
  a.yield_flag = s.chain_mark ? nullptr : s.yield_flag;
  a.yield_mark = s.chain_mark;
  if (s.ev_f2) hipStreamWaitEvent(s.sp, s.ev_f2, 0);
  wait_f1b(s);   // (a group of one panel never waited for it)
  ProfScope ps(c, "syrk_trailing", 1, s.sp);
  a.c_lo = g1; a.c_hi = pl.la ? g2 : s.max_nblk;
  if (s.form != FORM_MFMA) {
    Syrk3Args b = s.s3a; b.kb_off = 0; b.nk = (g1 - g0) * (HBO_TILE / 16); b.c_lo = a.c_lo; b.c_hi = a.c_hi;
    b.yield_mark = a.yield_mark; b.yield_flag = a.yield_flag;
    launch_syrk3(b, tiles_of(s, b.c_lo, b.c_hi), s.ntasks, s.sp);
    return;
  }
  if (pl.split_f1 && a.c_hi - a.c_lo > 1) {
    // only the NEXT block column is on the critical path (potf2 and the solve of panel g1 read nothing else): the group's later
    // columns go to a third stream and are waited for by the first column update that touches them
    hipEvent_t e = pool_event(c, s.evi++);
    hipEventRecord(e, s.sp); hipStreamWaitEvent(c->stream3, e, 0);
    GemmArgs b = a; b.c_lo = a.c_lo + 1;
    b.small_tiles = (int64_t)(s.max_nblk + 1 - b.c_lo) * (b.c_hi - b.c_lo) * s.ntasks < 600;
    b.tl = tl_slot("f1b", g1);
    launch_gemm(s.dtype, b, dim3(s.max_nblk + 1 - b.c_lo, b.c_hi - b.c_lo, s.ntasks), c->stream3);
    s.ev_f1b = pool_event(c, s.evi++);
    hipEventRecord(s.ev_f1b, c->stream3);
    a.c_hi = a.c_lo + 1;
  }
  // few tiles (one group's block columns, or a small remainder): 64x64 tiles for latency
  a.small_tiles = (int64_t)(s.max_nblk + 1 - a.c_lo) * (a.c_hi - a.c_lo) * s.ntasks < 600;
  a.tl = tl_slot("f1", g1);
  launch_gemm(s.dtype, a, dim3(s.max_nblk + 1 - a.c_lo, a.c_hi - a.c_lo, s.ntasks), s.sp);
}
// F2, the bulk of the flops (look-ahead only): the rest of the trailing matrix, block columns [g2, max_nblk), on the main stream
// beside the next group's panel chain.  It runs after F1(g) (they share no C columns, but F2(g) must precede F1(g+1) / F2(g+1),
// which accumulate into the same tiles); ev_f2 behind it is what the next F1 (and nothing else on the chain) waits for.
void step_f2(const PotrfPlan& pl, PotrfState& s, int g0, int g1, int g2) {
  hbo_ctx* c = s.c;
  const int64_t m = s.max_nblk - g2;
  const bool small_tiles = m * (m + 1) / 2 * s.ntasks < 600;
  const int nt = tiles_of(s, g2, s.max_nblk);
  {
    // "syrk_bulk" = the 128x128-tile bulk trailing update (the roofline kernel of bench.py)
    ProfScope ps(c, small_tiles ? "syrk_trailing" : "syrk_bulk", 1, s.sm);
    GridRule r; r.pool = &s.bulk;
    if (s.form != FORM_MFMA) {
      Syrk3Args b = s.s3a; b.kb_off = 0; b.nk = (g1 - g0) * (HBO_TILE / 16); b.c_lo = g2; b.c_hi = s.max_nblk;
      r.beside = s.ntasks == 1 && pl.syrk3_free > 0; r.free_cus = pl.syrk3_free;
      resident_grid(c, b, r, nt, s.sm);
      b.yield_flag = s.yield_flag;   // the bulk update is background work
      launch_syrk3(b, nt, s.ntasks, s.sm);
    } else {
      GemmArgs a = {}; a.tasks = s.d_tasks; a.mode = GEMM_SYRK; a.p0 = g0; a.kt = g1 - g0; a.aug = 1;
      a.yield_flag = s.yield_flag;   // the bulk update is background work
      a.c_lo = g2; a.c_hi = s.max_nblk; a.small_tiles = small_tiles;
      // (round 6: leaving the chain 16 CUs while the trailing matrix has >= 48 tile columns and 48-64 afterwards -- early groups wait for the bulk
      //  update, later ones for the chain -- measured neutral: N = 8192 10.64 -> 10.57-10.75 ms, N = 6144 5.60 -> 5.54-5.60; removed)
      // (round 6: the leading columns -- what the NEXT F1 accumulates into -- as a launch of their own with ev_f2 behind THAT, so that
      //  the chain runs up to one bulk launch ahead: measured neutral, the two launches take 457 us where the one took 414;
      //  DESIGN.md section 6, 1 (a); removed)
      const int pblocks = 2 * (c->n_cus - pl.persist_free);
      const int64_t ntiles = (int64_t)nt * (small_tiles ? 4 : 1);
      // persistent form (single task, enough tiles to fill the machine): leave CUs for the panel chain
      r.beside = s.ntasks == 1 && pl.persist_free > 0 && m <= 96; r.free_cus = pl.persist_free;
      r.whole = s.ntasks == 1 && pl.persist_free > 0 && m > 96 && pl.bulk_whole && !small_tiles; r.whole_pool = &s.bulk;
      r.static_ok = true;
      resident_grid(c, a, r, ntiles, s.sm);
      if (a.persistent && a.work_counter && !small_tiles) {
        // a partly filled last round (fewer than half of the workgroups would get a 128-tile) runs on 64-tiles
        // (the whole last round on 64-tiles, or never: measured equal or slower, profiles/r02_potrf_chain.md)
        const int64_t rem = ntiles % pblocks;
        if (rem > 0 && rem * 2 <= pblocks) a.n_big = (int)(ntiles - rem);
      }
      a.tl = tl_slot("f2", g1);
      launch_gemm(s.dtype, a, dim3(s.max_nblk + 1 - a.c_lo, a.c_hi - a.c_lo, s.ntasks), s.sm);
    }
  }
  s.ev_f2 = pool_event(c, s.evi++);
  hipEventRecord(s.ev_f2, s.sm);
}
}  // namespace

// Right-looking blocked Cholesky with look-ahead.  Panels are 128 wide; `q` consecutive panels
// are factored left-looking (the later ones first receive the group's earlier panels: syrk_col),
// then one trailing update with K = 128*q is applied.  The trailing update is split in two
// launches: F1 updates only the NEXT group's block columns, F2 the rest; the next group's panel
// work (potf2 -> trsm, the serial chain) runs on a second stream as soon as F1 is done, so F2
// -- the bulk of the flops -- overlaps it.
void run_potrf(hbo_ctx* c, int dtype, const TaskDesc* d_tasks, int ntasks, int max_nblk, int* d_info, InvRun* inv) {
  const PotrfPlan pl = potrf_plan(c, dtype, ntasks, max_nblk, inv ? &inv->pl : nullptr);
  PotrfState s = {c, dtype, d_tasks, ntasks, max_nblk, d_info, c->stream, pl.la ? c->stream2 : c->stream};
  if (pl.la) { hipEvent_t e = pool_event(c, s.evi++); hipEventRecord(e, s.sm); hipStreamWaitEvent(s.sp, e, 0); }   // fork
  potrf_setup(pl, s);
  c->last_chol_form = (int)s.form; c->last_inv_forms = 0;
  for (int g0 = 0, grp = 0; g0 < max_nblk; g0 += pl.q, ++grp) {
    const int g1 = std::min(g0 + pl.q, max_nblk);
    const int g2 = std::min(g1 + pl.q, max_nblk);
    if (s.form != FORM_MFMA) s.s3a.Xp = s.s3buf[grp & 1];
    if (s.form == FORM_F16X2) s.s3a.aug_scale = s.h2_aug + (grp & 1) * s.s3a.aug_stride * ntasks;
    for (int p = g0; p < g1; ++p) {
      const int gi = pl.q_inner ? g0 + (p - g0) / pl.q_inner * pl.q_inner : g0;   // first panel of p's inner group
      if (pl.q_inner && p == gi && p > g0) step_inner_update(pl, s, g0, g1, gi, p);
      if (p > gi) step_column_update(s, gi, p);
      step_panel(s, g0, g1, gi, p);
      step_hand_over(pl, s, p, inv);
    }
    if (g1 == max_nblk) break;
    step_f1(pl, s, g0, g1, g2);
    if (!pl.la) continue;
    // the main stream only learns that F1 is finished, to start F2 behind it; the panel stream continues in order
    hipEvent_t e = pool_event(c, s.evi++);
    hipEventRecord(e, s.sp); hipStreamWaitEvent(s.sm, e, 0);
    if (g2 < max_nblk) step_f2(pl, s, g0, g1, g2);
  }
  c->run.gemm_yield = nullptr;
  c->run.side.base = nullptr;
  wait_f1b(s);
  if (pl.la) { hipEvent_t e = pool_event(c, s.evi++); hipEventRecord(e, s.sp); hipStreamWaitEvent(s.sm, e, 0); }   // join
  // (the sweep's tail, on the main stream, waits for exactly what it needs of the side stream's work: sweep_advance)
  if (inv && inv->pl.early) {   // the rest of the inverse (main stream) needs the early part
    hipEvent_t e = pool_event(c, s.evi++);
    hipEventRecord(e, c->stream4);
    hipStreamWaitEvent(s.sm, e, 0);
  }
}
// The same level on the bf16 matrix cores (fp32, one matrix): both operands of each product are split exactly into three bf16
// planes (post3.hip) -- A: S21 = L21 W11 from row blocks of L and the transpose of W11, B: W21 = -W22 S21 from row blocks of
// W22 and the transpose of S21 -- then one launch per product over all groups of the level.
static bool trtri_level3(InvRun& r, int s, int grp_lo, int grp_hi, bool do_a, bool do_b, hipStream_t st) {
  hbo_ctx* c = r.c; const TaskDesc* d_tasks = r.d_tasks; const TaskDesc& h = *r.host; const int max_nblk = r.max_nblk;
  int ngrp = grp_hi - grp_lo;
  int vlast = std::min(s, max_nblk - ((grp_hi - 1) * 2 * s + s));
  if (vlast <= 0) { --ngrp; vlast = s; }
  if (ngrp <= 0) return true;
  const int nkb = 8 * s;
  // f16x2 form (run_potrf set it up: the caller knows max A_ii): L's blocks by the a-priori scale, W's and S21's by measured maxima
  // -- one word per level and operand; W11 / W22 are measured by a pass over what is about to be split, S21 by the product
  // that writes it.  The words only grow over the calls of a factorisation (other groups of the same level): still a bound.
  int li = 0;
  while ((1 << li) < s) ++li;
  unsigned int* const words = (c->run.h2_words && li < HBO_H2_LEVELS) ? c->run.h2_words + 3 * li : nullptr;
  const bool h2 = words != nullptr;
  const float sL = h2 ? post2h_scale_for(std::sqrt(c->run.chol_diag_bound)) : 1.f;
  const int64_t gstride = (int64_t)s * nkb * (h2 ? 2 : 3) * (HBO_TILE * 16);
  const size_t bytes = sizeof(unsigned short) * (size_t)gstride * ngrp;
  unsigned short* xp = static_cast<unsigned short*>(ws_get(c, WS_TRTRI3_X, bytes));
  unsigned short* yp = static_cast<unsigned short*>(ws_get(c, WS_TRTRI3_Y, bytes));
  if (!xp || !yp) return false;
  const int64_t ld = h.ld;
  const int64_t o0 = (int64_t)grp_lo * 2 * s * HBO_TILE, half = (int64_t)s * HBO_TILE;
  const float* L = static_cast<const float*>(h.A);
  const float* W = static_cast<const float*>(h.W);
  const float* S = static_cast<const float*>(h.S);
  Split3Block sb = {}; sb.ld = ld; sb.gstep = 2 * half * (ld + 1); sb.gstride = gstride; sb.nkb = nkb; sb.row_tiles = s;
  Syrk3Args g = {}; g.tasks = d_tasks; g.Xp = xp; g.Yp = yp; g.s = s; g.grp_lo = grp_lo; g.ngrp = ngrp; g.vlast = vlast;
  g.h2 = sb.h2 = h2 ? 1 : 0;
  const GridRule rule = inv_grid(r.pl.level, st == c->stream4, &c->run.side);
  const int ntiles = ((ngrp - 1) * s + vlast) * s;
  auto launch = [&](int mode) {
    g.mode = mode;
    g.yield_flag = (st == c->stream4) ? c->run.gemm_yield : nullptr;
    resident_grid(c, g, rule, ntiles, st);
    launch_syrk3(g, ntiles, 1, st);
  };
  c->last_inv_forms |= h2 ? 2 : 1;
  ProfScope ps(c, "trtri_gemm", 2, st);
  if (do_a) {
    sb.in = L + (o0 + half) * ld + o0; sb.out = xp; sb.tri = 0; sb.last_rows = vlast; sb.last_krows = (int)half;
    sb.scale = sL; sb.scale_bits = nullptr; sb.max_out = nullptr;
    launch_split3_block(sb, ngrp, false, st);                     // rows of L21
    sb.in = W + o0 * ld + o0; sb.out = yp; sb.last_rows = s; sb.last_krows = (int)half;
    sb.max_out = h2 ? words + 0 : nullptr;
    launch_split3_block(sb, ngrp, true, st);                      // W11^T (the left half of every group is complete)
    g.sx = sL; g.sx_bits = nullptr; g.sy_bits = h2 ? words + 0 : nullptr; g.max_out = h2 ? words + 1 : nullptr;
    launch(1);
  }
  if (do_b) {
    sb.in = W + (o0 + half) * ld + (o0 + half); sb.out = xp; sb.tri = 1; sb.last_rows = vlast; sb.last_krows = vlast * HBO_TILE;
    sb.scale_bits = nullptr; sb.max_out = h2 ? words + 2 : nullptr;
    launch_split3_block(sb, ngrp, false, st);                     // rows of W22 (lower triangular)
    sb.in = S + (o0 + half) * ld + o0; sb.out = yp; sb.tri = 0; sb.last_rows = s; sb.last_krows = vlast * HBO_TILE;
    sb.scale_bits = h2 ? words + 1 : nullptr; sb.max_out = nullptr;
    launch_split3_block(sb, ngrp, true, st);                      // S21^T
    g.sx_bits = h2 ? words + 2 : nullptr; g.sy_bits = h2 ? words + 1 : nullptr; g.max_out = nullptr;
    launch(2);
  }
  return true;
}

// One level of the recursive inverse restricted to the groups [grp_lo, grp_hi) (a group = 2s blocks):
//   mode A: S21 = L21 W11,  mode B: W21 = -W22 S21.
static void trtri_level(InvRun& run, int s, int grp_lo, int grp_hi, bool do_a, bool do_b, hipStream_t st) {
  hbo_ctx* c = run.c; const int dtype = run.dtype, ntasks = run.ntasks, max_nblk = run.max_nblk;
  const int ngroups = grp_hi - grp_lo;
  if (ngroups <= 0) return;
  if (s >= run.pl.lvl3_min_s && run.host && run.host->A && trtri_level3(run, s, grp_lo, grp_hi, do_a, do_b, st)) return;
  GemmArgs a = {}; a.tasks = run.d_tasks; a.p0 = s; a.grp_lo = grp_lo;
  a.small_tiles = level_small_tiles(run.pl, (int64_t)ngroups * s * s * ntasks);
  a.yield_flag = (st == c->stream4) ? c->run.gemm_yield : nullptr;
  const int tmul = a.small_tiles ? 4 : 1;
  ProfScope ps(c, "trtri_gemm", 2, st);
  // Rows of the last group's lower half that exist in the largest task: workgroups beyond them would be dispatched
  // only to exit, which is not free (56 ns each: at the top level of a batch of 64 matrices of <= 19 blocks, 13 of
  // the 16 tile rows are empty and the launch took 4.3 ms instead of 0.8).
  const int vlast = std::min(s, max_nblk - ((grp_hi - 1) * 2 * s + s));
  if (vlast <= 0 && ngroups == 1) return;
  const int xa = (ngroups - 1) * s + std::max(vlast, 0);
  a.c_hi = grp_hi - 1; a.c_lo = std::max(vlast, 0);   // TRTRI_A: last group and its launched tile rows
  int post_slot = 0;
  auto persist = [&](int64_t tiles) {
    const GridRule r = level_grid(run.pl, a.small_tiles, post_slot, st == c->stream4, &c->run.side);
    resident_grid(c, a, r, tiles, st);
    if (!r.beside && a.persistent) ++post_slot;
  };
  if (do_a && xa > 0) { a.mode = GEMM_TRTRI_A; persist((int64_t)xa * s * tmul); a.tl = tl_slot("trtri_a", s); launch_gemm(dtype, a, dim3(xa, s, ntasks), st); }
  if (do_b) {
    a.mode = GEMM_TRTRI_B;
    const int vy = ngroups == 1 ? vlast : s;
    a.kt = vy;   // valid tile rows when there is a single group (blockIdx.y counts down from them)
    persist((int64_t)ngroups * s * vy * tmul);
    a.tl = tl_slot("trtri_b", s);
    launch_gemm(dtype, a, dim3(ngroups * s, vy, ntasks), st);
  }
}

// W = L^-1 by recursive doubling over the block tree: level s merges pairs of inverted s-block diagonal pieces,
//   S21 = L21 W11 (A),  W21 = -W22 S21 (B)   for every group g = blocks [2sg, 2sg + 2s).
// A of a group only needs the block columns below 2sg + s of L, B those below the group's end, so the tree can be
// walked while the factorisation is still running: trtri_advance(cfin) launches -- level by level, which is also the
// dependency order on one stream -- every piece that has become computable now that block columns [0, cfin) are
// final and was not launched before.  run_potrf calls it on a side stream after every fourth panel (the second half
// of the factorisation is bound by the serial panel chain and leaves most CUs idle); the last call, with
// cfin = max_nblk on the main stream, launches what is left (for a 64-block matrix: the B products on the right
// spine of the tree, 1.25 of the inverse's 3.7 ms).
void trtri_advance(InvRun& r, int cfin, hipStream_t st, int max_s) {
  TrtriProgress& pg = r.pg; const int max_nblk = r.max_nblk;
  if (cfin > pg.diag) {
    ProfScope ps(r.c, "trtri_diag", 2, st);
    launch_trtri_diag(r.dtype, r.d_tasks, r.ntasks, pg.diag, cfin, st);
    pg.diag = cfin;
  }
  int li = 0;
  for (int s = 1; s < max_nblk && s <= max_s && li < 12; s *= 2, ++li) {
    // groups with a lower half: g*2s + s < max_nblk
    const int ngrp = (max_nblk - s + 2 * s - 1) / (2 * s);
    // A: left half final (cfin >= g*2s + s);  B: whole group final (cfin >= min(g*2s + 2s, max_nblk))
    int na = cfin >= s ? (cfin - s) / (2 * s) + 1 : 0;
    int nb = cfin >= max_nblk ? ngrp : cfin / (2 * s);
    na = std::min(na, ngrp); nb = std::min(nb, ngrp);
    if (na > pg.a[li]) { trtri_level(r, s, pg.a[li], na, true, false, st); pg.a[li] = na; }
    if (nb > pg.b[li]) { trtri_level(r, s, pg.b[li], nb, false, true, st); pg.b[li] = nb; }
  }
}
// ---- the one-sweep inverse -----------------------------------------------------------------------------------------------------
// With L = [[L11, 0], [L21, L22]] split at a row group R (q blocks): W = L^-1 = [[W11, 0], [-W22 L21 W11, W22]].  The product
// L21 W11 is not formed when R comes up -- it would be a skinny product with K up to N on the critical path of the sweep -- but
// accumulated: every finished group g' adds its term L[below, g'] W[g', :] to a running matrix T for ALL rows below it, a rank-q
// update of the same shape as the Cholesky's trailing update.  When R's block columns of L are final, T[R, :] is complete and
//   (a) W[R,R] = L[R,R]^-1        block-recursive inverse of the q x q diagonal group (trtri_advance capped at q / 2),
//   (b) W[R, <R] = -W[R,R] T[R, <R]                                                                  GEMM_SWEEP_B, K <= q
//   (c) T[>R, <=R] += L[>R, R] W[R, <=R]                                                              GEMM_SWEEP_T, K = q
//   (d) K^-1[<=R, <=R] += W[R, <=R]^T W[R, <=R]                                                       GEMM_SWEEP_C, K = q
// T and K^-1 share the S buffer: T lives below the front, K^-1 at and above it, and the rows R change roles between (b) and (d).
// Same flops as the recursive inverse + K^-1 = W^T W (N^3/3 each); what changes is WHEN they can run: everything but the last
// group's (a), (b), (d) sits beside the panel chain, and all of it is uniform K = 128 q work with thousands of tiles per launch.
static hipEvent_t sweep_event(hbo_ctx* c, SweepState& sw) { return event_of(c->ev_pool_sweep, (size_t)sw.nev++); }
void sweep_advance(InvRun& r, int cfin, hipStream_t st, hipEvent_t w_done) {
  hbo_ctx* c = r.c; const InvPlan& pl = r.pl; SweepState& sw = r.sw;
  const int dtype = r.dtype, ntasks = r.ntasks, max_nblk = r.max_nblk, q = pl.qs;
  // beside the panel chain (side stream, counters of this factorisation at hand): persistent and slot-limited, tiles (x tasks) from
  // a counter, polling the yield table when the chain's kernels keep one -- see trtri_level
  const GridRule rule = inv_grid(pl.swept, st == c->stream4, &c->run.side);
  // one launch: the tile size by its count of 128-tiles, then its place
  auto place = [&](GemmArgs& a, int64_t tiles128) {
    a.small_tiles = sweep_small_tiles(pl, tiles128 * ntasks);
    a.yield_flag = (st == c->stream4) ? c->run.gemm_yield : nullptr;
    resident_grid(c, a, rule, tiles128 * (a.small_tiles ? 4 : 1) * ntasks, st);
  };
  hipStream_t sd = pl.d_own_stream ? c->stream3 : st;
  while (sw.done < max_nblk) {
    const int b0 = sw.done, b1 = std::min(b0 + q, max_nblk);
    if (b1 > cfin) break;
    if (sw.ev_c && sw.st_c != st) hipStreamWaitEvent(st, sw.ev_c, 0);   // T[R, <R] is complete (and every earlier launch of that stream)
    trtri_advance(r, b1, st, q / 2);                                                                 // (a)
    GemmArgs a = {}; a.tasks = r.d_tasks; a.c_lo = b0; a.c_hi = b1;
    if (b0 > 0) {                                                                                    // (b)
      ProfScope ps(c, "sweep_b", 2, st);
      a.mode = GEMM_SWEEP_B; place(a, (int64_t)b0 * (b1 - b0)); a.tl = tl_slot("sweep_b", b1);
      launch_gemm(dtype, a, dim3(b0, b1 - b0, ntasks), st);
    }
    if (b1 == max_nblk && w_done) hipEventRecord(w_done, st);
    if (sd != st) { hipEvent_t e = sweep_event(c, sw); hipEventRecord(e, st); hipStreamWaitEvent(sd, e, 0); }   // W[R, <=R] is final
    if (b1 < max_nblk) {                                                                             // (c)
      ProfScope ps(c, "sweep_t", 2, st);
      a.mode = GEMM_SWEEP_T; place(a, (int64_t)(max_nblk - b1) * b1); a.tl = tl_slot("sweep_t", b1);
      launch_gemm(dtype, a, dim3(max_nblk - b1, b1, ntasks), st);
      sw.ev_c = sweep_event(c, sw); hipEventRecord(sw.ev_c, st); sw.st_c = st;
    }
    {                                                                                                // (d)
      ProfScope ps(c, "sweep_c", 2, sd);
      a.mode = GEMM_SWEEP_C; place(a, (int64_t)b1 * (b1 + 1) / 2);
      if (sw.ev_d && sw.st_d != sd) hipStreamWaitEvent(sd, sw.ev_d, 0);   // the previous group's update of the same K^-1 tiles
      a.tl = tl_slot("sweep_c", b1);
      launch_gemm(dtype, a, dim3(b1, 1, ntasks), sd);
      if (b1 < max_nblk) { sw.ev_d = sweep_event(c, sw); hipEventRecord(sw.ev_d, sd); sw.st_d = sd; }
    }
    sw.done = b1;
    if (b1 == max_nblk && sd != st) { hipEvent_t e = sweep_event(c, sw); hipEventRecord(e, sd); hipStreamWaitEvent(st, e, 0); }   // K^-1 is complete
  }
}
void run_trtri(InvRun& r) { trtri_advance(r, r.max_nblk, r.c->stream); }
// K^-1 = W^T W on the lower tiles.  (A two-launch form that started the W11^T W11 part beside the tail of the inverse was
// built and measured neutral in round 2 -- profiles/r02_potrf_chain.md -- and is gone.)
void run_lauum(InvRun& r) {
  hbo_ctx* c = r.c; hipStream_t s = c->stream; const int max_nblk = r.max_nblk;
  ProfScope ps(c, "lauum", 2, s);
  const GridRule rule = inv_grid(r.pl.kinv, false, &c->run.side);
  const int nt = max_nblk * (max_nblk + 1) / 2;
  // fp32, one matrix beyond the small sizes: on the bf16 matrix cores from ONE exact three-way split of W^T (post3.hip,
  // syrk3_kernel mode 3) -- 6 bytes per element of the lower triangle of W as workspace
  if (r.pl.kinv3 && r.host && r.host->W && r.host->nblk == max_nblk) {
    const int nkb = 8 * max_nblk;
    const size_t bytes = sizeof(unsigned short) * (size_t)max_nblk * nkb * 3 * (HBO_TILE * 16);
    unsigned short* xp = static_cast<unsigned short*>(ws_get(c, WS_LAUUM3, bytes));
    if (xp) {
      Syrk3Args g = {}; g.tasks = r.d_tasks; g.Xp = xp; g.nkb = nkb; g.mode = 3;
      Split3Block sw = {}; sw.in = static_cast<const float*>(r.host->W); sw.ld = r.host->ld; sw.out = xp; sw.row_tiles = sw.last_rows = max_nblk;
      sw.nkb = nkb; sw.last_krows = max_nblk * HBO_TILE; sw.lower_only = 1;
      if (c->run.h2_words) {   // the f16x2 form: max |W| by one pass, W^T as two fp16 planes, three MFMAs per product
        unsigned int* word = c->run.h2_words + HBO_H2_WORDS - 1;
        sw.h2 = 1; sw.max_out = word;
        g.h2 = 1; g.sx_bits = g.sy_bits = word;
      }
      c->last_inv_forms |= g.h2 ? 8 : 4;
      launch_split3_block(sw, 1, true, s);
      resident_grid(c, g, rule, nt, s);
      launch_syrk3(g, nt, 1, s);
      return;
    }
  }
  GemmArgs a = {}; a.tasks = r.d_tasks; a.mode = GEMM_LAUUM;
  a.small_tiles = r.pl.small_shape;
  resident_grid(c, a, rule, nt, s);
  a.tl = tl_slot("lauum", 0);
  launch_gemm(r.dtype, a, dim3(max_nblk, max_nblk, r.ntasks), s);
}
