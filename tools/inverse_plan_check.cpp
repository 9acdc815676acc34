// Stand-alone comparison of inv_plan, its launch-time helpers and potrf_plan (hyperbo_amd/csrc/sched.h) with the expressions that
// trtri_level, trtri_level3, sweep_advance, run_lauum, step_f2, obj_plan and the callers of run_potrf held inline before the inverse
// side got its plan (profiles/inverse_plan_refactor.md).  No GPU, no libhbo, host code only:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g tools/inverse_plan_check.cpp -o tools/inverse_plan_check && tools/inverse_plan_check
// and once more with  -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all  on the same line.
// The "before" functions are the old lines as they stood; streams and counters are stand-in pointers that are only compared.
// Range: dtype x tasks {1, 2, 8, 9, 64} x blocks 1..520 x every level s = 1, 2, 4, .. x want {none, W, W + K^-1} x beside the chain or
// not x host descriptor present / absent x third stream present / absent x side / main stream x side counters or none x the option
// sets below (defaults; tests/test_gpu_fuzz.py: OPTION_SETS; the four 16-bit legs off singly and together, crossed with
// trtri3_min_s x sweep_free x syrk3_free).  Exit 0 and "ran clean" when nothing differs.
#include <cstdio>
#include <vector>

#include "../hyperbo_amd/csrc/sched.h"

thread_local std::string hbo_g_err;   // (link seam: api.hip)

namespace {
long long n_cases = 0, n_bad = 0;
char where[320];
void differ(const char* what, long long a, long long b) {
  if (a == b) return;
  if (++n_bad <= 30) std::printf("DIFFERENT %s: before %lld, now %lld  (%s)\n", what, a, b, where);
}
void differ_rule(const char* what, const GridRule& a, const GridRule& b) {
  char nm[64];
  auto f = [&](const char* fld, long long x, long long y) { std::snprintf(nm, sizeof nm, "%s.%s", what, fld); differ(nm, x, y); };
  f("beside", a.beside, b.beside); f("whole", a.whole, b.whole); f("static_ok", a.static_ok, b.static_ok);
  if (a.beside) { f("free_cus", a.free_cus, b.free_cus); f("pool", a.pool != nullptr, b.pool != nullptr); }   // (read by resident_grid only then)
  if (a.whole) { f("whole_min", a.whole_min, b.whole_min); f("whole_free", a.whole_free, b.whole_free); f("whole_pool", a.whole_pool != nullptr, b.whole_pool != nullptr); }
}

void differ_site(const char* what, const GridRule& a, const GridRule& b) {
  differ(what, 0, a.beside != b.beside || a.free_cus != b.free_cus || a.whole != b.whole || a.whole_min != b.whole_min || a.whole_free != b.whole_free ||
                  a.pool || b.pool || a.whole_pool || b.whole_pool || a.static_ok || b.static_ok);
}
void differ_beyond_route(const InvPlan& a, const InvPlan& b) {
  differ("small_shape by want", a.small_shape, b.small_shape); differ("few_tiles by want", a.few_tiles, b.few_tiles);
  differ("lvl3_min_s by want", a.lvl3_min_s, b.lvl3_min_s); differ("kinv3 by want", a.kinv3, b.kinv3); differ("batch_bg by want", a.batch_bg, b.batch_bg);
  differ("sweep_big by want", a.sweep_big, b.sweep_big); differ("d_own_stream by want", a.d_own_stream, b.d_own_stream);
  differ_site("level by want", a.level, b.level); differ_site("swept by want", a.swept, b.swept); differ_site("kinv by want", a.kinv, b.kinv);
}

// ---- before: sched.hip's helpers ---------------------------------------------------------------------------------------------
int before_small_limit(const hbo_ctx* c, int dtype) { return c->opt_small_nblk >= 0 ? c->opt_small_nblk : (dtype == HBO_F64 ? 48 : 32); }
int before_batch_bg(const hbo_ctx* c, int ntasks) { return c->opt_batch_bg >= 0 ? c->opt_batch_bg : (ntasks <= 8 ? 1 : 0); }
bool before_use_sweep(const hbo_ctx* c, int dtype, int ntasks, int max_nblk) {
  if (!c->opt_sweep || !use_lookahead(c, ntasks, max_nblk) || max_nblk < 8) return false;
  if (c->opt_sweep >= 2) return true;
  if (ntasks == 1) return dtype == HBO_F64 && max_nblk > 16 && max_nblk <= 48;
  if (dtype == HBO_F32 && ntasks == 1 && max_nblk > before_small_limit(c, dtype) && (c->opt_trtri_bf16x3 || c->opt_lauum_bf16x3)) return false;
  return true;
}
int before_sweep_group(int ntasks, int max_nblk) { return (ntasks == 1 && max_nblk > 28) ? 8 : 4; }
bool use_early_trtri(const hbo_ctx* c, int ntasks, int max_nblk) { return use_lookahead(c, ntasks, max_nblk) && c->opt_overlap_trtri && max_nblk >= 4; }   // (sched.h before)
// ---- before: potrf_plan with its `bool sweep`, and what step_f2 read beside it ----------------------------------------------
struct BeforePotrf { bool la; int q, q_inner, persist_free, tgran, early_at; YieldMode yield; bool split_f1; Fp32Form form; bool h2_scales; };
BeforePotrf before_potrf_plan(const hbo_ctx* c, int dtype, int ntasks, int max_nblk, bool sweep) {
  BeforePotrf pl = {};
  pl.la = use_lookahead(c, ntasks, max_nblk);
  const bool s3 = dtype == HBO_F32 && c->opt_syrk_bf16x3;
  pl.h2_scales = dtype == HBO_F32 && c->opt_chol_f16x2 && c->run.chol_diag_bound > 0;
  pl.form = (s3 && max_nblk > 1) ? (pl.h2_scales ? FORM_F16X2 : FORM_BF16X3) : FORM_MFMA;
  const bool small_mat = max_nblk <= 96;
  const bool s3_large = s3 && !small_mat;
  const int q_small = (s3 && ntasks == 1 && max_nblk >= 56) ? 6 : ((ntasks == 1 && max_nblk > 64) ? 7 : 3);
  pl.q = c->opt_group > 0 ? c->opt_group : ((!pl.la && ntasks <= 8) ? 1 : (small_mat ? q_small : (s3_large ? 16 : (max_nblk >= 256 ? 8 : 4))));
  const int q_inner = c->opt_group_inner >= 0 ? c->opt_group_inner : ((s3_large && pl.q == 16) ? 8 : 0);
  pl.q_inner = (q_inner > 0 && q_inner < pl.q) ? q_inner : 0;
  pl.persist_free = c->opt_persist_free >= 0 ? c->opt_persist_free : 32;
  pl.split_f1 = pl.la && c->stream3 && (c->opt_split_f1 >= 2 || (c->opt_split_f1 == 1 && ntasks > 1));
  pl.tgran = 4;
  pl.early_at = -1;
  if (ntasks == 1) {
    pl.early_at = c->opt_trtri_at > 0 ? std::min(c->opt_trtri_at * max_nblk / 64, max_nblk - 1) : (max_nblk * 5 / 8) & ~3;
    if (pl.early_at < 4) pl.early_at = -1;
    pl.tgran = 1 << 30;
  }
  const bool batch_yield = ntasks > 1 && sweep && before_batch_bg(c, ntasks) >= 2;
  const bool yield = pl.la && c->opt_cu_yield && ((ntasks == 1 && (small_mat || pl.form != FORM_MFMA)) || batch_yield);
  pl.yield = !yield ? YIELD_NONE : (c->opt_cu_yield >= 2 ? YIELD_CHAIN : YIELD_POTF2);
  return pl;
}

// ---- the option sets -----------------------------------------------------------------------------------------------------------
struct Opt { int hbo_ctx::*f; int v; };
typedef std::vector<Opt> OptSet;
#define O(field, v) Opt{&hbo_ctx::opt_##field, v}
std::vector<OptSet> option_sets() {
  // tests/test_gpu_fuzz.py: OPTION_SETS, in its order (post_chunk is no option of the schedules: that entry runs the defaults)
  std::vector<OptSet> s = {
      {O(lookahead, 0)}, {O(lookahead, 2)}, {O(overlap_trtri, 0)}, {O(group, 1)}, {O(group, 2)}, {O(group, 4)}, {O(group, 8)},
      {O(persist_free, 0)}, {O(persist_free, 128)}, {O(persist_free, 64), O(small_nblk, 0)}, {O(persist_free, 200), O(small_nblk, 0)},
      {O(small_nblk, 0)}, {O(small_nblk, 4)}, {O(cu_yield, 0)}, {O(cu_yield, 1)}, {O(lookahead, 0), O(group, 3), O(small_nblk, 0)},
      {O(trtri_free, 0)}, {O(trtri_free, 120), O(small_nblk, 0)}, {O(trtri_free, 200)},
      {O(trtri_at, 12)}, {O(trtri_at, 60), O(small_nblk, 0)}, {O(trtri_at, 48), O(small_nblk, 0)}, {O(post_chunk, 128)},
      {O(sweep, 0), O(lookahead, 2)}, {O(sweep, 2)}, {O(sweep, 1), O(lookahead, 2)}, {O(sweep, 2), O(sweep_qs, 2), O(lookahead, 2)},
      {O(sweep, 2), O(sweep_qs, 8), O(small_nblk, 0)}, {O(sweep, 2), O(sweep_big, 0)}, {O(sweep, 2), O(sweep_big, 1 << 30), O(batch_bg, 1)},
      {O(sweep, 2), O(batch_bg, 2), O(lookahead, 2)}, {O(sweep, 2), O(sweep_qs, 1), O(lookahead, 2)}, {O(batch_bg, 0), O(lookahead, 2)},
      {O(lauum_persist, 0), O(small_nblk, 0)}, {O(small_nblk, 2), O(sweep, 0)}, {O(sweep, 2), O(small_nblk, 0), O(sweep_side, 0)},
      {O(sweep, 2), O(small_nblk, 4), O(sweep_qs, 2)}, {O(split_f1, 0), O(lookahead, 2)}, {O(split_f1, 2)},
      {O(split_f1, 2), O(lookahead, 2), O(group, 1)}, {O(split_f1, 2), O(sweep, 0), O(group, 2)}};
  if (s.size() != 41) { std::printf("OPTION_SETS: %zu entries, expected 41\n", s.size()); ++n_bad; }
  // the defaults and the 16-bit legs off singly and together, crossed with the three knobs no OPTION_SETS entry names
  const std::vector<OptSet> legs = {{}, {O(trtri_bf16x3, 0)}, {O(lauum_bf16x3, 0)}, {O(syrk_bf16x3, 0)}, {O(chol_f16x2, 0)},
                                    {O(trtri_bf16x3, 0), O(lauum_bf16x3, 0), O(syrk_bf16x3, 0), O(chol_f16x2, 0)}};
  for (const OptSet& leg : legs) for (int min_s : {1, 8, 64}) for (int sweep_free : {1, 24, 200}) for (int syrk3_free : {0, 32}) {
    OptSet o = leg;
    o.push_back(O(trtri3_min_s, min_s)); o.push_back(O(sweep_free, sweep_free)); o.push_back(O(syrk3_free, syrk3_free));
    s.push_back(o);
  }
  return s;
}

int dummy_word;

// one shape under one option set: everything below the options
void check_shape(hbo_ctx& c, int dtype, int ntasks, int max_nblk, const TaskDesc* host) {
  const TaskDesc none = {};
  const TaskDesc& h_task0 = host ? *host : none;   // before: hbo_ctx::trtri_host_task, zeroed for batches
  // ---- the route, as the four callers decided it, and potrf_plan under it ----
  InvPlan base = {};
  for (int want = INV_NONE; want <= INV_W_KINV; ++want) for (int beside = 0; beside < 2; ++beside) {
    ++n_cases;
    // objective (gradient): want_grad && !euc -> W + K^-1 beside; cache.hip and the EUC gradient's unused plan: W beside; hbo_spd_solve,
    // a value with extra rows and hbo_nll_samples: nothing beside the chain
    bool sweep = false, early_trtri = false; int qs = 0;
    if (beside && want == INV_W_KINV) {
      sweep = before_use_sweep(&c, dtype, ntasks, max_nblk);
      qs = !sweep ? 0 : (c.opt_sweep_qs > 0 ? c.opt_sweep_qs : before_sweep_group(ntasks, max_nblk));
      early_trtri = !sweep && use_early_trtri(&c, ntasks, max_nblk);
    } else if (beside && want == INV_W) {
      early_trtri = use_early_trtri(&c, ntasks, max_nblk);
    }
    const InvPlan pl = inv_plan(&c, dtype, ntasks, max_nblk, (InvWant)want, host != nullptr, beside != 0);
    differ("sweep", sweep, pl.sweep); differ("qs", qs, pl.qs); differ("early", early_trtri, pl.early);
    if (want == INV_NONE && !beside) base = pl;
    else {   // nothing but the route depends on want / beside
      differ_beyond_route(base, pl);
    }
    for (double bound : {0.0, 2.0}) {
      c.run.chol_diag_bound = bound;
      const BeforePotrf b = before_potrf_plan(&c, dtype, ntasks, max_nblk, sweep);
      const PotrfPlan p = potrf_plan(&c, dtype, ntasks, max_nblk, want == INV_NONE && !beside ? nullptr : &pl);
      differ("potrf.la", b.la, p.la); differ("potrf.q", b.q, p.q); differ("potrf.q_inner", b.q_inner, p.q_inner);
      differ("potrf.persist_free", b.persist_free, p.persist_free); differ("potrf.tgran", b.tgran, p.tgran); differ("potrf.early_at", b.early_at, p.early_at);
      differ("potrf.yield", b.yield, p.yield); differ("potrf.split_f1", b.split_f1, p.split_f1); differ("potrf.form", b.form, p.form);
      differ("potrf.h2_scales", b.h2_scales, p.h2_scales);
      // step_f2's two reads
      differ("f2 beside", ntasks == 1 && c.opt_syrk3_free > 0, ntasks == 1 && p.syrk3_free > 0); differ("f2 free_cus", c.opt_syrk3_free, p.syrk3_free);
      for (int m : {50, 200}) for (int small_tiles = 0; small_tiles < 2; ++small_tiles)
        differ("f2 whole", ntasks == 1 && b.persist_free > 0 && m > 96 && c.opt_lauum_persist && !small_tiles,
               ntasks == 1 && p.persist_free > 0 && m > 96 && p.bulk_whole && !small_tiles);
    }
    c.run.chol_diag_bound = 0;
  }
  const InvPlan& pl = base;
  // ---- launch time: the call on the side / main stream, with and without this factorisation's side counters ----
  for (int on_side = 0; on_side < 2; ++on_side) for (int counters = 0; counters < 2; ++counters) {
    hipStream_t st = on_side ? c.stream4 : c.stream;
    c.run.side.base = counters ? &dummy_word : nullptr;
    // trtri_level and trtri_level3, every level, one group and all of them, the call's first launch and its third
    for (int s = 1; s < max_nblk; s *= 2) for (int ngroups : {1, (max_nblk - s + 2 * s - 1) / (2 * s)}) for (int post_slot : {0, 2}) {
      ++n_cases;
      const bool use3 = dtype == HBO_F32 && c.opt_trtri_bf16x3 && ntasks == 1 && h_task0.A && s >= c.opt_trtri3_min_s && max_nblk > before_small_limit(&c, dtype);
      differ("level on the 16-bit cores", use3, s >= pl.lvl3_min_s && host && host->A);
      {
        GridRule r;
        r.beside = st == c.stream4 && c.opt_trtri_free > 0 && c.run.side.base; r.free_cus = c.opt_trtri_free; r.pool = &c.run.side;
        r.whole = c.opt_lauum_persist; r.whole_min = 4 * c.n_cus;
        if (use3) differ_rule("level3", r, inv_grid(pl.level, st == c.stream4, &c.run.side));
      }
      struct { int small_tiles; } a;
      a.small_tiles = (max_nblk <= before_small_limit(&c, dtype)) || ((int64_t)ngroups * s * s * ntasks < 600);
      const bool corun = st == c.stream4 && ntasks == 1 && c.opt_trtri_free > 0 && c.run.side.base;
      GridRule r; r.beside = corun; r.free_cus = c.opt_trtri_free; r.pool = &c.run.side; r.whole_min = 4 * c.n_cus;
      r.whole = ntasks == 1 && !a.small_tiles && c.opt_lauum_persist && post_slot < 2;
      const bool small_now = level_small_tiles(pl, (int64_t)ngroups * s * s * ntasks);
      differ("level small_tiles", a.small_tiles, small_now);
      differ_rule("level", r, level_grid(pl, small_now, post_slot, st == c.stream4, &c.run.side));
    }
    // sweep_advance: launches of few and of many tiles around sweep_big
    {
      const bool small_shape = max_nblk <= before_small_limit(&c, dtype);
      GridRule r; r.pool = &c.run.side;
      r.beside = st == c.stream4 && c.run.side.base && c.opt_trtri_free > 0 && (ntasks == 1 || before_batch_bg(&c, ntasks) >= 1);
      r.free_cus = std::min(c.opt_trtri_free, c.opt_sweep_free);
      hipStream_t sd = (c.opt_sweep_side && c.stream3 && ntasks == 1 && max_nblk > before_small_limit(&c, dtype)) ? c.stream3 : st;
      ++n_cases;
      differ_rule("sweep", r, inv_grid(pl.swept, st == c.stream4, &c.run.side));
      differ("stream of (d)", sd != st, pl.d_own_stream);
      const int64_t edge = c.opt_sweep_big / ntasks;
      for (int64_t tiles128 : {(int64_t)1, edge - 1, edge, edge + 1, (int64_t)1 << 40}) {
        if (tiles128 < 1) continue;
        differ("sweep small_tiles", small_shape && tiles128 * ntasks < c.opt_sweep_big, sweep_small_tiles(pl, tiles128 * ntasks));
      }
    }
    // run_lauum (main stream only)
    if (!on_side) {
      const TaskDesc& h = h_task0;
      GridRule r; r.whole_min = 4 * c.n_cus + 1; r.whole_free = c.opt_lauum_persist > 1 ? c.opt_lauum_persist : 16;
      const bool use3 = dtype == HBO_F32 && c.opt_lauum_bf16x3 && ntasks == 1 && h.W && h.nblk == max_nblk && max_nblk > before_small_limit(&c, dtype);
      struct { int small_tiles; } a;
      a.small_tiles = max_nblk <= before_small_limit(&c, dtype);
      if (use3) r.whole = c.opt_lauum_persist;
      else r.whole = ntasks == 1 && !a.small_tiles && c.opt_lauum_persist;
      ++n_cases;
      differ("K^-1 on the 16-bit cores", use3, pl.kinv3 && host && host->W && host->nblk == max_nblk);
      if (!use3) differ("K^-1 small_tiles", a.small_tiles, pl.small_shape);
      differ_rule("K^-1", r, inv_grid(pl.kinv, false, &c.run.side));
    }
  }
  c.run.side.base = nullptr;
}
}  // namespace

int main() {
  char word[4];   // stand-ins for streams: distinct addresses, never dereferenced
  for (const OptSet& os : option_sets()) {
    hbo_ctx c;
    c.stream = (hipStream_t)&word[0]; c.stream2 = (hipStream_t)&word[1]; c.stream4 = (hipStream_t)&word[3];
    char opts[200] = ""; size_t len = 0;
    for (const Opt& o : os) {
      c.*(o.f) = o.v;
      // (the name of the field is not at hand: its offset in hbo_ctx tells the sets apart in a report)
      len += std::snprintf(opts + len, sizeof opts - len, " +%zu=%d", (size_t)((char*)&(c.*(o.f)) - (char*)&c), o.v);
    }
    for (int dtype : {HBO_F32, HBO_F64}) for (int ntasks : {1, 2, 8, 9, 64}) for (int max_nblk = 1; max_nblk <= 520; ++max_nblk)
    for (int have_host = 0; have_host < 2; ++have_host) for (int third = 0; third < 2; ++third) {
      if (have_host && ntasks != 1) continue;   // (a host descriptor is a single task's)
      c.stream3 = third ? (hipStream_t)&word[2] : nullptr;
      TaskDesc h = {};
      h.A = h.W = h.S = &dummy_word; h.nblk = max_nblk; h.ld = max_nblk * HBO_TILE;
      std::snprintf(where, sizeof where, "dtype %d tasks %d blocks %d host %d stream3 %d options (field offset = value)%s", dtype, ntasks, max_nblk, have_host, third, opts);
      check_shape(c, dtype, ntasks, max_nblk, have_host ? &h : nullptr);
    }
  }
  std::printf("%lld cases, %lld difference(s)\n", n_cases, n_bad);
  std::printf(n_bad ? "FAILED\n" : "ran clean\n");
  return n_bad ? 1 : 0;
}
