// The L-BFGS state machine of hbo_train_lbfgs: basics/lbfgs.py (lbfgs, backtracking_linesearch, lbfgs_descent_dir_nocedal) turned
// inside out -- one call consumes the value and the raw-space gradient of the point just evaluated and leaves the point to evaluate
// next.  Plain C++, nothing of the HIP runtime: the control kernel (train.hip: lbfgs_ctl_kernel, 256 threads), the host hook
// hbo_probe_lbfgs_ctl (one thread) and tools/lbfgs_ctl_check.cpp compile this same text.
//
// A team of `nthr` threads runs every function together (thread `tid`); element i of a vector belongs to thread i % nthr.  All
// scalars are computed by every thread from the same inputs, so control flow is uniform; thread 0 stores them.
//
// Dot products: partial sum p[j], j < 256, adds a[i] * b[i] over i = j, j + 256, ... in rising i; then p[j] += p[j + s] (j < s) for
// s = 128, 64, ..., 1.  The order is fixed by P alone: one host thread and 256 device threads give the same bits.
// No fused multiply-adds, no atomics.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef HBO_LBFGS_FN
#define HBO_LBFGS_FN inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define HBO_LBFGS_BARRIER() __syncthreads()
#else
#define HBO_LBFGS_BARRIER() ((void)0)
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#else
#pragma STDC FP_CONTRACT OFF
#endif

enum { HBO_LBFGS_PARTIALS = 256 };
// the header of the state array (doubles); the vectors follow in the order of hbo_lbfgs_view
enum {
  HBO_LBFGS_S_PHASE = 0,   // what the next evaluation is: hbo_lbfgs_phase
  HBO_LBFGS_S_STATUS,      // hbo_lbfgs_status
  HBO_LBFGS_S_ITER,        // main iteration the run is in (0: the start and its line search)
  HBO_LBFGS_S_PROBES,      // probes of the current line search already evaluated
  HBO_LBFGS_S_ALPHA,       // step of the probe under evaluation
  HBO_LBFGS_S_CUR,         // value at the iterate (cur_val of the line search)
  HBO_LBFGS_S_GD,          // g . d at the iterate
  HBO_LBFGS_S_NHIST,       // (s, y) pairs held, <= memory
  HBO_LBFGS_S_HEAD,        // ring slot the next pair goes to
  HBO_LBFGS_S_EVALS,       // evaluations consumed so far
  HBO_LBFGS_S_HEADER = 16
};
enum hbo_lbfgs_phase { HBO_LBFGS_PHASE_START = 0, HBO_LBFGS_PHASE_LINE_SEARCH = 1, HBO_LBFGS_PHASE_MAIN = 2 };

struct hbo_lbfgs_opts_ctl { int memory, ls_steps, max_iters; double alpha, tol, c1, c2, grow, tau; };
struct hbo_lbfgs_eval_ctl { int kind, iter; double alpha, value; };
enum { HBO_LBFGS_CTL_START = 0, HBO_LBFGS_CTL_MAIN = 1, HBO_LBFGS_CTL_LINE_SEARCH = 2, HBO_LBFGS_CTL_IDLE = 3 };
enum { HBO_LBFGS_CTL_RUNNING = 0, HBO_LBFGS_CTL_CONVERGED_AT_START = 1, HBO_LBFGS_CTL_CONVERGED = 2, HBO_LBFGS_CTL_NO_PROGRESS = 3,
       HBO_LBFGS_CTL_INSTABILITY = 4, HBO_LBFGS_CTL_STEPS_DONE = 5 };

// the vectors of the state: iterate, point under evaluation, old_x, old_g, direction, gradient of the point under evaluation (the
// caller writes it there), then the ring of s and of y (memory x P each), then alphas and 1 / (y . s) of the two-loop recursion
struct hbo_lbfgs_view {
  double* hdr; double* x; double* xt; double* old_x; double* old_g; double* d; double* g; double* s; double* y; double* al; double* rho;
  int P, M;
};
HBO_LBFGS_FN int64_t hbo_lbfgs_state_size(int P, int memory) {
  return (int64_t)HBO_LBFGS_S_HEADER + 6 * (int64_t)P + 2 * (int64_t)memory * P + 2 * (int64_t)memory;
}
HBO_LBFGS_FN hbo_lbfgs_view hbo_lbfgs_view_of(double* state, int P, int memory) {
  hbo_lbfgs_view v;
  v.P = P; v.M = memory;
  v.hdr = state; v.x = state + HBO_LBFGS_S_HEADER; v.xt = v.x + P; v.old_x = v.xt + P; v.old_g = v.old_x + P; v.d = v.old_g + P;
  v.g = v.d + P; v.s = v.g + P; v.y = v.s + (int64_t)memory * P; v.al = v.y + (int64_t)memory * P; v.rho = v.al + memory;
  return v;
}

// scratch: HBO_LBFGS_PARTIALS doubles the team shares.  Three barriers per product: the tree's levels 128 and 64 are taken by the 64
// threads that own their results, the levels 32 .. 1 by every thread for itself (the same additions in the same order).
HBO_LBFGS_FN double hbo_lbfgs_dot(const double* a, const double* b, int P, int tid, int nthr, double* scratch) {
  HBO_LBFGS_BARRIER();   // the operands may have been written by other threads; the previous result has been read
  for (int j = tid; j < HBO_LBFGS_PARTIALS; j += nthr) {
    double acc = 0.0;
    for (int i = j; i < P; i += HBO_LBFGS_PARTIALS) acc += a[i] * b[i];
    scratch[j] = acc;
  }
  HBO_LBFGS_BARRIER();
  // p[j] += p[j + 128] (j < 128), then p[j] += p[j + 64] (j < 64): thread j reads and writes only indices congruent to j mod 64
  for (int j = tid; j < 64; j += nthr) scratch[j] = (scratch[j] + scratch[j + 128]) + (scratch[j + 64] + scratch[j + 192]);
  HBO_LBFGS_BARRIER();
  double t[32];
  for (int j = 0; j < 32; ++j) t[j] = scratch[j] + scratch[j + 32];
  for (int s = 16; s > 0; s >>= 1)
    for (int j = 0; j < s; ++j) t[j] += t[j + s];
  return t[0];
}

// the working copy of the header's scalars, the same in every thread
struct hbo_lbfgs_regs { int phase, status, iter, probes, nhist, head, evals; double alpha, cur, gd; };

// slot of pair j (0 = oldest) of the ring
HBO_LBFGS_FN int hbo_lbfgs_slot(const hbo_lbfgs_regs& r, int M, int j) { return (r.head - r.nhist + j + 2 * M) % M; }

// the point of the probe with the current alpha
HBO_LBFGS_FN void hbo_lbfgs_set_trial(const hbo_lbfgs_view& v, double alpha, int tid, int nthr) {
  for (int i = tid; i < v.P; i += nthr) v.xt[i] = v.x[i] + alpha * v.d[i];
}

// what lbfgs() does with the (new_val, step) its line search returned; `val` is the value the search started from
HBO_LBFGS_FN void hbo_lbfgs_ls_return(const hbo_lbfgs_view& v, const hbo_lbfgs_opts_ctl& o, hbo_lbfgs_regs& r, double new_val, double step,
                                      int tid, int nthr) {
  const double val = r.cur;
  // lbfgs.py: after the start `if new_val < val: move, else: stop`; in the loop `if new_val >= val: stop, else: move` (they part on NaN)
  const bool move = r.iter == 0 ? (new_val < val) : !(new_val >= val);
  if (!move) { r.status = HBO_LBFGS_CTL_NO_PROGRESS; return; }
  for (int i = tid; i < v.P; i += nthr) { const double xi = v.x[i] + step * v.d[i]; v.x[i] = xi; v.xt[i] = xi; }
  if (r.iter >= o.max_iters) { r.status = HBO_LBFGS_CTL_STEPS_DONE; return; }
  r.iter += 1;
  r.phase = HBO_LBFGS_PHASE_MAIN;
}

// backtracking_linesearch up to its first evaluation: g . d, the early return on a non-descent direction, the first probe
HBO_LBFGS_FN void hbo_lbfgs_ls_begin(const hbo_lbfgs_view& v, const hbo_lbfgs_opts_ctl& o, hbo_lbfgs_regs& r, int tid, int nthr, double* scratch) {
  r.gd = hbo_lbfgs_dot(v.g, v.d, v.P, tid, nthr, scratch);
  r.probes = 0;
  if (r.gd > 0.0) { hbo_lbfgs_ls_return(v, o, r, r.cur, 0.0, tid, nthr); return; }
  r.phase = HBO_LBFGS_PHASE_LINE_SEARCH;
  hbo_lbfgs_set_trial(v, r.alpha, tid, nthr);
}

// lbfgs_descent_dir_nocedal into v.d, in the host's order
HBO_LBFGS_FN void hbo_lbfgs_direction(const hbo_lbfgs_view& v, const hbo_lbfgs_regs& r, int tid, int nthr, double* scratch) {
  const int P = v.P, n = r.nhist;
  for (int j = 0; j < n; ++j) {
    const int64_t o = (int64_t)hbo_lbfgs_slot(r, v.M, j) * P;
    const double ys = hbo_lbfgs_dot(v.y + o, v.s + o, P, tid, nthr, scratch);
    if (tid == 0) v.rho[j] = 1.0 / ys;
  }
  for (int i = tid; i < P; i += nthr) v.d[i] = -v.g[i];   // q
  for (int j = n - 1; j >= 0; --j) {
    const int64_t o = (int64_t)hbo_lbfgs_slot(r, v.M, j) * P;
    const double sq = hbo_lbfgs_dot(v.s + o, v.d, P, tid, nthr, scratch);
    const double a = v.rho[j] * sq;
    if (tid == 0) v.al[j] = a;
    for (int i = tid; i < P; i += nthr) v.d[i] = v.d[i] - a * v.y[o + i];
  }
  const int64_t ol = (int64_t)hbo_lbfgs_slot(r, v.M, n - 1) * P;
  const double sy = hbo_lbfgs_dot(v.s + ol, v.y + ol, P, tid, nthr, scratch);
  const double yy = hbo_lbfgs_dot(v.y + ol, v.y + ol, P, tid, nthr, scratch);
  const double gamma = sy / yy;
  for (int i = tid; i < P; i += nthr) v.d[i] = gamma * v.d[i];
  for (int j = 0; j < n; ++j) {
    const int64_t o = (int64_t)hbo_lbfgs_slot(r, v.M, j) * P;
    const double yd = hbo_lbfgs_dot(v.y + o, v.d, P, tid, nthr, scratch);
    const double beta = v.rho[j] * yd;
    const double c = v.al[j] - beta;
    for (int i = tid; i < P; i += nthr) v.d[i] = v.d[i] + v.s[o + i] * c;
  }
}

// An all-zero state: the run starts at x0
HBO_LBFGS_FN void hbo_lbfgs_state_start(double* state, int P, int memory, const double* x0) {
  hbo_lbfgs_view v = hbo_lbfgs_view_of(state, P, memory);
  for (int i = 0; i < P; ++i) { v.x[i] = x0[i]; v.xt[i] = x0[i]; }
}

// One evaluation in, the next point out.  `value` and v.g (the raw-space gradient) belong to the point v.xt.  On return v.xt is the
// point to evaluate next (meaningless once the status is not RUNNING), v.x the iterate lbfgs() would return now.
HBO_LBFGS_FN void hbo_lbfgs_ctl_step(double* state, int P, const hbo_lbfgs_opts_ctl& o, double value, int tid, int nthr, double* scratch,
                                     hbo_lbfgs_eval_ctl* ev) {
  const hbo_lbfgs_view v = hbo_lbfgs_view_of(state, P, o.memory);
  hbo_lbfgs_regs r;
  r.phase = (int)v.hdr[HBO_LBFGS_S_PHASE]; r.status = (int)v.hdr[HBO_LBFGS_S_STATUS]; r.iter = (int)v.hdr[HBO_LBFGS_S_ITER];
  r.probes = (int)v.hdr[HBO_LBFGS_S_PROBES]; r.nhist = (int)v.hdr[HBO_LBFGS_S_NHIST]; r.head = (int)v.hdr[HBO_LBFGS_S_HEAD];
  r.evals = (int)v.hdr[HBO_LBFGS_S_EVALS];
  r.alpha = v.hdr[HBO_LBFGS_S_ALPHA]; r.cur = v.hdr[HBO_LBFGS_S_CUR]; r.gd = v.hdr[HBO_LBFGS_S_GD];
  HBO_LBFGS_BARRIER();   // every thread has read the header before thread 0 stores it again
  ev->value = value; ev->iter = r.iter; ev->alpha = 0.0;
  if (r.status != HBO_LBFGS_CTL_RUNNING) { ev->kind = HBO_LBFGS_CTL_IDLE; return; }
  r.evals += 1;
  if (r.phase == HBO_LBFGS_PHASE_START) {
    ev->kind = HBO_LBFGS_CTL_START;
    const double gg = hbo_lbfgs_dot(v.g, v.g, P, tid, nthr, scratch);
    if (gg <= o.tol) {
      r.status = HBO_LBFGS_CTL_CONVERGED_AT_START;
    } else {
      for (int i = tid; i < P; i += nthr) { v.old_x[i] = v.x[i]; v.old_g[i] = v.g[i]; v.d[i] = -v.g[i]; }
      r.alpha = 1.0 / sqrt(gg);
      r.cur = value;
      hbo_lbfgs_ls_begin(v, o, r, tid, nthr, scratch);
    }
  } else if (r.phase == HBO_LBFGS_PHASE_LINE_SEARCH) {
    ev->kind = HBO_LBFGS_CTL_LINE_SEARCH; ev->alpha = r.alpha;
    const double t = o.c1 * r.gd;
    const bool armijo = isfinite(value) && (r.cur + r.alpha * t >= value);
    bool accepted = false;
    r.probes += 1;
    if (armijo) {
      const double ngd = hbo_lbfgs_dot(v.g, v.d, P, tid, nthr, scratch);
      if (ngd >= o.c2 * r.gd) accepted = true;
      else r.alpha *= o.grow;
    } else {
      r.alpha *= o.tau;
    }
    if (accepted) {
      hbo_lbfgs_ls_return(v, o, r, value, r.alpha, tid, nthr);
    } else if (r.probes >= o.ls_steps) {
      // the search is exhausted: the step returned is the alpha already modified after the last probe (a point never evaluated)
      if (isfinite(value)) hbo_lbfgs_ls_return(v, o, r, value, r.alpha, tid, nthr);
      else hbo_lbfgs_ls_return(v, o, r, r.cur, 0.0, tid, nthr);
    } else {
      hbo_lbfgs_set_trial(v, r.alpha, tid, nthr);
    }
  } else {
    ev->kind = HBO_LBFGS_CTL_MAIN;
    const double gg = hbo_lbfgs_dot(v.g, v.g, P, tid, nthr, scratch);
    if (gg <= o.tol) {
      r.status = HBO_LBFGS_CTL_CONVERGED;
    } else {
      const int64_t oh = (int64_t)r.head * P;
      for (int i = tid; i < P; i += nthr) {
        v.y[oh + i] = v.g[i] - v.old_g[i];
        v.s[oh + i] = v.x[i] - v.old_x[i];
        v.old_x[i] = v.x[i]; v.old_g[i] = v.g[i];
      }
      r.head = (r.head + 1) % o.memory;
      if (r.nhist < o.memory) r.nhist += 1;
      const double magnitude = hbo_lbfgs_dot(v.y + oh, v.s + oh, P, tid, nthr, scratch);
      if (isfinite(magnitude) && magnitude >= o.tol) {
        hbo_lbfgs_direction(v, r, tid, nthr, scratch);
        r.cur = value;
        r.alpha = o.alpha;
        hbo_lbfgs_ls_begin(v, o, r, tid, nthr, scratch);
      } else {
        r.status = HBO_LBFGS_CTL_INSTABILITY;
      }
    }
  }
  HBO_LBFGS_BARRIER();
  if (tid == 0) {
    v.hdr[HBO_LBFGS_S_PHASE] = r.phase; v.hdr[HBO_LBFGS_S_STATUS] = r.status; v.hdr[HBO_LBFGS_S_ITER] = r.iter;
    v.hdr[HBO_LBFGS_S_PROBES] = r.probes; v.hdr[HBO_LBFGS_S_NHIST] = r.nhist; v.hdr[HBO_LBFGS_S_HEAD] = r.head;
    v.hdr[HBO_LBFGS_S_EVALS] = r.evals;
    v.hdr[HBO_LBFGS_S_ALPHA] = r.alpha; v.hdr[HBO_LBFGS_S_CUR] = r.cur; v.hdr[HBO_LBFGS_S_GD] = r.gd;
  }
  HBO_LBFGS_BARRIER();
}
