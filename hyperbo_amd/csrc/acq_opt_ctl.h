// The state machine of hbo_acq_maximize: a box-constrained projected L-BFGS that minimises f(x) = -(mean over the S samples of the
// acquisition) over lo <= x <= hi, turned inside out as lbfgs_ctl.h is -- one call consumes the per-sample values and gradients of the
// pending point and leaves the next point to evaluate.  Plain C++, nothing of the HIP runtime: the control kernel (acq_opt.hip:
// acq_opt_ctl_kernel, 256 threads per start), the host hook hbo_probe_acq_opt_ctl (one thread) and tools/acq_opt_ctl_check.cpp compile
// this same text.  The algorithm is written down in DESIGN.md section 6.
//
// The team conventions are those of lbfgs_ctl.h: `nthr` threads run every function together, element i of a vector belongs to thread
// i % nthr, all scalars are computed by every thread from the same inputs (uniform control flow), thread 0 stores them.  Every sum
// goes through hbo_lbfgs_dot (the 256-partial tree) or runs in index order inside one thread; a maximum is taken over 256 partials that
// every thread then reads in order.  No fused multiply-adds, no atomics: one host thread and 256 device threads give the same bits.
#pragma once
#include "lbfgs_ctl.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#else
#pragma STDC FP_CONTRACT OFF
#endif

// the header of the state array (doubles); the vectors follow in the order of hbo_acq_opt_view
enum {
  HBO_ACQ_OPT_S_PHASE = 0,   // 0: the next evaluation is the start's, 1: a line-search probe's
  HBO_ACQ_OPT_S_STATUS,      // hbo_acq_opt_status
  HBO_ACQ_OPT_S_ITER,        // accepted steps so far
  HBO_ACQ_OPT_S_PROBES,      // rejected probes of the current line search
  HBO_ACQ_OPT_S_ALPHA,       // step of the probe under evaluation
  HBO_ACQ_OPT_S_CUR,         // f at the iterate (NaN until the start has been evaluated)
  HBO_ACQ_OPT_S_NHIST,       // (s, y) pairs held, <= memory
  HBO_ACQ_OPT_S_HEAD,        // ring slot the next pair goes to
  HBO_ACQ_OPT_S_EVALS,       // evaluations consumed so far
  HBO_ACQ_OPT_S_MAGIC,       // HBO_ACQ_OPT_MAGIC once the run has been started
  HBO_ACQ_OPT_S_HEADER = 16
};
#define HBO_ACQ_OPT_MAGIC 20816.0
enum { HBO_ACQ_OPT_PHASE_START = 0, HBO_ACQ_OPT_PHASE_LINE_SEARCH = 1 };

struct hbo_acq_opt_opts_ctl { int memory, ls_steps, max_iters; double c1, tau, pgtol, ftol; };
struct hbo_acq_opt_eval_ctl { int kind, iter; double alpha, value; };
enum { HBO_ACQ_OPT_CTL_START = 0, HBO_ACQ_OPT_CTL_MAIN = 1, HBO_ACQ_OPT_CTL_LINE_SEARCH = 2, HBO_ACQ_OPT_CTL_IDLE = 3 };
enum { HBO_ACQ_OPT_CTL_RUNNING = 0, HBO_ACQ_OPT_CTL_CONVERGED = 1, HBO_ACQ_OPT_CTL_FTOL = 2, HBO_ACQ_OPT_CTL_NO_PROGRESS = 3,
       HBO_ACQ_OPT_CTL_NONFINITE_AT_START = 4, HBO_ACQ_OPT_CTL_STEPS_DONE = 5 };

// the vectors of the state: iterate, pending point, gradient of f at the iterate, gradient of f at the pending point, projected
// gradient, direction, two work vectors (x_t - x and g_t - g of the probe), then the ring of s and of y (memory x D each), then the
// alphas and 1 / (y . s) of the two-loop recursion
struct hbo_acq_opt_view {
  double* hdr; double* x; double* xt; double* g; double* gt; double* pg; double* d; double* ws; double* wy; double* s; double* y;
  double* al; double* rho;
  int D, M;
};
HBO_LBFGS_FN int64_t hbo_acq_opt_state_size(int D, int memory) {
  return (int64_t)HBO_ACQ_OPT_S_HEADER + 8 * (int64_t)D + 2 * (int64_t)memory * D + 2 * (int64_t)memory;
}
HBO_LBFGS_FN hbo_acq_opt_view hbo_acq_opt_view_of(double* state, int D, int memory) {
  hbo_acq_opt_view v;
  v.D = D; v.M = memory;
  v.hdr = state; v.x = state + HBO_ACQ_OPT_S_HEADER; v.xt = v.x + D; v.g = v.xt + D; v.gt = v.g + D; v.pg = v.gt + D; v.d = v.pg + D;
  v.ws = v.d + D; v.wy = v.ws + D; v.s = v.wy + D; v.y = v.s + (int64_t)memory * D; v.al = v.y + (int64_t)memory * D; v.rho = v.al + memory;
  return v;
}

// the largest of a[i] >= 0 (0 for an empty or all-NaN vector): partial j takes i = j, j + 256, ...; every thread reads the partials in order
HBO_LBFGS_FN double hbo_acq_opt_max(const double* a, int D, int tid, int nthr, double* scratch) {
  HBO_LBFGS_BARRIER();
  for (int j = tid; j < HBO_LBFGS_PARTIALS; j += nthr) {
    double m = 0.0;
    for (int i = j; i < D; i += HBO_LBFGS_PARTIALS) m = a[i] > m ? a[i] : m;
    scratch[j] = m;
  }
  HBO_LBFGS_BARRIER();
  double m = 0.0;
  for (int j = 0; j < HBO_LBFGS_PARTIALS; ++j) m = scratch[j] > m ? scratch[j] : m;
  return m;
}

HBO_LBFGS_FN double hbo_acq_opt_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }
HBO_LBFGS_FN double hbo_acq_opt_bound(const double* b, int i, double dflt) { return b ? b[i] : dflt; }

// sum of a[s * stride], s = 0 .. S - 1, added in that order; the loads go out HBO_ACQ_OPT_BATCH at a time (on the device every one of
// them is a trip to memory, and one at a time they cost more than the kernel that produced them)
enum { HBO_ACQ_OPT_BATCH = 16 };
HBO_LBFGS_FN double hbo_acq_opt_sum_in_order(const double* a, int64_t stride, int S) {
  double sum = 0.0;
  int s = 0;
  for (; s + HBO_ACQ_OPT_BATCH <= S; s += HBO_ACQ_OPT_BATCH) {
    double t[HBO_ACQ_OPT_BATCH];
#pragma unroll
    for (int k = 0; k < HBO_ACQ_OPT_BATCH; ++k) t[k] = a[(s + k) * stride];
#pragma unroll
    for (int k = 0; k < HBO_ACQ_OPT_BATCH; ++k) sum += t[k];
  }
  for (; s < S; ++s) sum += a[s * stride];
  return sum;
}

// f and its gradient at the pending point from the per-sample acquisition values and gradients: sums in sample order s = 0 .. S - 1,
// divided by S, negated.  vals[s * vstride], grads[s * gstride + i].  The gradient goes to v.gt; every thread returns f.
HBO_LBFGS_FN double hbo_acq_opt_reduce(const hbo_acq_opt_view& v, const double* vals, int64_t vstride, const double* grads, int64_t gstride,
                                       int S, int tid, int nthr) {
  for (int i = tid; i < v.D; i += nthr) v.gt[i] = -(hbo_acq_opt_sum_in_order(grads + i, gstride, S) / (double)S);
  return -(hbo_acq_opt_sum_in_order(vals, vstride, S) / (double)S);
}

// The same from per-sample LOG values (hbo_logei_maximize: the acquisition is the log of the mean of the samples' EI, not the mean of
// their logs): with m = max_s v_s and w_s = exp(v_s - m),  value = m + log(sum_s w_s / S),  grad = sum_s w_s g_s / sum_s w_s,  the sums
// in sample order, then negated.  m = -inf (EI is 0 under every sample): f = +inf, gradient 0 -- the caller's isfinite tests reject
// it.  A NaN value gives NaN.  S = 1: w = 1, log 1 = 0, and f and the gradient are the sample's to the bit.  exp and log are the
// library's: the device and a host thread agree to the library's ulp here, not to the bit as everywhere else in this file.
HBO_LBFGS_FN double hbo_acq_opt_reduce_lme(const hbo_acq_opt_view& v, const double* vals, int64_t vstride, const double* grads, int64_t gstride,
                                           int S, int tid, int nthr) {
  double m = -INFINITY;
  bool nan = false;
  for (int s = 0; s < S; ++s) { const double t = vals[s * vstride]; nan = nan || t != t; m = t > m ? t : m; }
  if (nan) {
    for (int i = tid; i < v.D; i += nthr) v.gt[i] = NAN;
    return NAN;
  }
  if (m == -INFINITY) {
    for (int i = tid; i < v.D; i += nthr) v.gt[i] = 0.0;
    return INFINITY;
  }
  double sw = 0.0;
  for (int s = 0; s < S; ++s) sw += exp(vals[s * vstride] - m);
  for (int i = tid; i < v.D; i += nthr) {
    double sg = 0.0;
    for (int s = 0; s < S; ++s) { const double w = exp(vals[s * vstride] - m); sg += w * grads[s * gstride + i]; }
    v.gt[i] = -(sg / sw);
  }
  const double mean = sw / (double)S;
  return -(m + log(mean));
}
enum { HBO_ACQ_OPT_REDUCE_MEAN = 0, HBO_ACQ_OPT_REDUCE_LME = 1 };

struct hbo_acq_opt_regs { int phase, status, iter, probes, nhist, head, evals; double alpha, cur; };

// the probe x_t = clip(x + alpha d, lo, hi), rounded to the model dtype
HBO_LBFGS_FN void hbo_acq_opt_set_trial(const hbo_acq_opt_view& v, double alpha, const double* lo, const double* hi, int round_f32, int tid, int nthr) {
  for (int i = tid; i < v.D; i += nthr) {
    const double step = alpha * v.d[i];
    double t = hbo_acq_opt_clip(v.x[i] + step, hbo_acq_opt_bound(lo, i, 0.0), hbo_acq_opt_bound(hi, i, 1.0));
    if (round_f32) t = (double)(float)t;
    v.xt[i] = t;
  }
}

// the projected gradient of (v.x, v.g) into v.pg; returns SciPy's measure max_i |clip(x_i - g_i, lo_i, hi_i) - x_i|  (v.ws is overwritten)
HBO_LBFGS_FN double hbo_acq_opt_project(const hbo_acq_opt_view& v, const double* lo, const double* hi, int tid, int nthr, double* scratch) {
  for (int i = tid; i < v.D; i += nthr) {
    const double l = hbo_acq_opt_bound(lo, i, 0.0), h = hbo_acq_opt_bound(hi, i, 1.0), x = v.x[i], g = v.g[i];
    const bool active = (x == l && g > 0.0) || (x == h && g < 0.0);
    v.pg[i] = active ? 0.0 : g;
    v.ws[i] = fabs(hbo_acq_opt_clip(x - g, l, h) - x);
  }
  return hbo_acq_opt_max(v.ws, v.D, tid, nthr, scratch);
}

// One evaluation in, the next point out.  vals / grads: the per-sample results at the pending point v.xt (hbo_acq_opt_reduce).  On
// return v.xt is the point to evaluate next (untouched once the status is not RUNNING) and v.x the iterate.
// REDUCE, a compile-time choice: HBO_ACQ_OPT_REDUCE_MEAN -- hbo_acq_opt_reduce, every caller but one (hbo_acq_opt_ctl_step below);
// HBO_ACQ_OPT_REDUCE_LME -- hbo_acq_opt_reduce_lme (hbo_logei_maximize).  Nothing else differs.
template <int REDUCE>
HBO_LBFGS_FN void hbo_acq_opt_ctl_step_t(double* state, int D, const hbo_acq_opt_opts_ctl& o, const double* lo, const double* hi, int round_f32,
                                       const double* vals, int64_t vstride, const double* grads, int64_t gstride, int S, int tid, int nthr,
                                       double* scratch, hbo_acq_opt_eval_ctl* ev) {
  const hbo_acq_opt_view v = hbo_acq_opt_view_of(state, D, o.memory);
  hbo_acq_opt_regs r;
  r.phase = (int)v.hdr[HBO_ACQ_OPT_S_PHASE]; r.status = (int)v.hdr[HBO_ACQ_OPT_S_STATUS]; r.iter = (int)v.hdr[HBO_ACQ_OPT_S_ITER];
  r.probes = (int)v.hdr[HBO_ACQ_OPT_S_PROBES]; r.nhist = (int)v.hdr[HBO_ACQ_OPT_S_NHIST]; r.head = (int)v.hdr[HBO_ACQ_OPT_S_HEAD];
  r.evals = (int)v.hdr[HBO_ACQ_OPT_S_EVALS]; r.alpha = v.hdr[HBO_ACQ_OPT_S_ALPHA]; r.cur = v.hdr[HBO_ACQ_OPT_S_CUR];
  HBO_LBFGS_BARRIER();   // every thread has read the header before thread 0 stores it again
  ev->iter = r.iter; ev->alpha = 0.0; ev->value = 0.0;
  if (r.status != HBO_ACQ_OPT_CTL_RUNNING) { ev->kind = HBO_ACQ_OPT_CTL_IDLE; return; }
  const double ft = REDUCE == HBO_ACQ_OPT_REDUCE_LME ? hbo_acq_opt_reduce_lme(v, vals, vstride, grads, gstride, S, tid, nthr)
                                                     : hbo_acq_opt_reduce(v, vals, vstride, grads, gstride, S, tid, nthr);
  ev->value = ft;
  r.evals += 1;
  bool accepted = false;
  if (r.phase == HBO_ACQ_OPT_PHASE_START) {
    ev->kind = HBO_ACQ_OPT_CTL_START;
    if (!isfinite(ft)) {
      r.status = HBO_ACQ_OPT_CTL_NONFINITE_AT_START;
    } else {
      r.cur = ft;
      for (int i = tid; i < D; i += nthr) v.g[i] = v.gt[i];
      HBO_LBFGS_BARRIER();
      const double conv = hbo_acq_opt_project(v, lo, hi, tid, nthr, scratch);
      if (conv <= o.pgtol) {
        r.status = HBO_ACQ_OPT_CTL_CONVERGED;
      } else {
        for (int i = tid; i < D; i += nthr) v.d[i] = -v.pg[i];
        const double nrm = sqrt(hbo_lbfgs_dot(v.pg, v.pg, D, tid, nthr, scratch));
        const double inv = 1.0 / nrm;
        r.alpha = inv < 1.0 ? inv : 1.0;
        r.probes = 0;
        r.phase = HBO_ACQ_OPT_PHASE_LINE_SEARCH;
        hbo_acq_opt_set_trial(v, r.alpha, lo, hi, round_f32, tid, nthr);
      }
    }
  } else {
    ev->alpha = r.alpha;
    // Armijo on the projected step: f_t <= f + c1 g . (x_t - x)
    for (int i = tid; i < D; i += nthr) { const double dx = v.xt[i] - v.x[i]; v.ws[i] = dx; v.wy[i] = dx != 0.0 ? 1.0 : 0.0; }
    const double gs = hbo_lbfgs_dot(v.g, v.ws, D, tid, nthr, scratch);
    const double slope = o.c1 * gs;
    accepted = isfinite(ft) && (ft <= r.cur + slope);
    if (!accepted) {
      ev->kind = HBO_ACQ_OPT_CTL_LINE_SEARCH;
      r.probes += 1;
      r.alpha *= o.tau;
      if (r.probes >= o.ls_steps) r.status = HBO_ACQ_OPT_CTL_NO_PROGRESS;
      else hbo_acq_opt_set_trial(v, r.alpha, lo, hi, round_f32, tid, nthr);
    } else if (hbo_acq_opt_max(v.wy, D, tid, nthr, scratch) == 0.0) {
      ev->kind = HBO_ACQ_OPT_CTL_LINE_SEARCH;   // accepted without moving: nothing more to gain along this direction
      r.status = HBO_ACQ_OPT_CTL_NO_PROGRESS;
    } else {
      ev->kind = HBO_ACQ_OPT_CTL_MAIN;
      const double f_old = r.cur;
      for (int i = tid; i < D; i += nthr) { v.wy[i] = v.gt[i] - v.g[i]; v.x[i] = v.xt[i]; v.g[i] = v.gt[i]; }
      r.cur = ft;
      r.iter += 1;
      ev->iter = r.iter;
      const double sy = hbo_lbfgs_dot(v.ws, v.wy, D, tid, nthr, scratch);
      const double yy = hbo_lbfgs_dot(v.wy, v.wy, D, tid, nthr, scratch);
      const double thr = 2.2e-16 * yy;
      if (sy > thr) {   // L-BFGS-B's rule; a skipped pair leaves the ring unchanged
        const int64_t oh = (int64_t)r.head * D;
        for (int i = tid; i < D; i += nthr) { v.s[oh + i] = v.ws[i]; v.y[oh + i] = v.wy[i]; }
        r.head = (r.head + 1) % o.memory;
        if (r.nhist < o.memory) r.nhist += 1;
      }
      HBO_LBFGS_BARRIER();
      const double conv = hbo_acq_opt_project(v, lo, hi, tid, nthr, scratch);
      const double af = fabs(f_old), an = fabs(ft);
      double big = af > an ? af : an;
      big = big > 1.0 ? big : 1.0;
      const double ftol_abs = o.ftol * big;
      if (conv <= o.pgtol) r.status = HBO_ACQ_OPT_CTL_CONVERGED;
      else if (f_old - ft <= ftol_abs) r.status = HBO_ACQ_OPT_CTL_FTOL;
      else if (r.iter >= o.max_iters) r.status = HBO_ACQ_OPT_CTL_STEPS_DONE;
      else {
        bool steepest = r.nhist == 0;
        if (!steepest) {
          // the two-loop recursion applied to pg (hbo_lbfgs_direction reads its gradient from view.g), zeroed on the active set
          hbo_lbfgs_view lv;
          lv.hdr = v.hdr; lv.x = v.x; lv.xt = v.xt; lv.old_x = v.ws; lv.old_g = v.wy; lv.d = v.d; lv.g = v.pg; lv.s = v.s; lv.y = v.y;
          lv.al = v.al; lv.rho = v.rho; lv.P = D; lv.M = o.memory;
          hbo_lbfgs_regs lr;
          lr.phase = 0; lr.status = 0; lr.iter = 0; lr.probes = 0; lr.evals = 0; lr.alpha = 0.0; lr.cur = 0.0; lr.gd = 0.0;
          lr.nhist = r.nhist; lr.head = r.head;
          HBO_LBFGS_BARRIER();
          hbo_lbfgs_direction(lv, lr, tid, nthr, scratch);
          for (int i = tid; i < D; i += nthr) {
            const double l = hbo_acq_opt_bound(lo, i, 0.0), h = hbo_acq_opt_bound(hi, i, 1.0), x = v.x[i], g = v.g[i];
            if ((x == l && g > 0.0) || (x == h && g < 0.0)) v.d[i] = 0.0;
          }
          const double gd = hbo_lbfgs_dot(v.g, v.d, D, tid, nthr, scratch);
          if (!(gd < 0.0)) { r.nhist = 0; r.head = 0; steepest = true; }   // not a descent direction: the history is dropped
        }
        if (steepest) {
          HBO_LBFGS_BARRIER();
          for (int i = tid; i < D; i += nthr) v.d[i] = -v.pg[i];
        }
        r.alpha = 1.0;
        r.probes = 0;
        hbo_acq_opt_set_trial(v, r.alpha, lo, hi, round_f32, tid, nthr);
      }
    }
  }
  HBO_LBFGS_BARRIER();
  if (tid == 0) {
    v.hdr[HBO_ACQ_OPT_S_PHASE] = r.phase; v.hdr[HBO_ACQ_OPT_S_STATUS] = r.status; v.hdr[HBO_ACQ_OPT_S_ITER] = r.iter;
    v.hdr[HBO_ACQ_OPT_S_PROBES] = r.probes; v.hdr[HBO_ACQ_OPT_S_NHIST] = r.nhist; v.hdr[HBO_ACQ_OPT_S_HEAD] = r.head;
    v.hdr[HBO_ACQ_OPT_S_EVALS] = r.evals; v.hdr[HBO_ACQ_OPT_S_ALPHA] = r.alpha; v.hdr[HBO_ACQ_OPT_S_CUR] = r.cur;
  }
  HBO_LBFGS_BARRIER();
}

HBO_LBFGS_FN void hbo_acq_opt_ctl_step(double* state, int D, const hbo_acq_opt_opts_ctl& o, const double* lo, const double* hi, int round_f32,
                                       const double* vals, int64_t vstride, const double* grads, int64_t gstride, int S, int tid, int nthr,
                                       double* scratch, hbo_acq_opt_eval_ctl* ev) {
  hbo_acq_opt_ctl_step_t<HBO_ACQ_OPT_REDUCE_MEAN>(state, D, o, lo, hi, round_f32, vals, vstride, grads, gstride, S, tid, nthr, scratch, ev);
}

// An all-zero state: the run starts at x0 (already a number of the model dtype, inside the box)
HBO_LBFGS_FN void hbo_acq_opt_state_start(double* state, int D, int memory, const double* x0) {
  hbo_acq_opt_view v = hbo_acq_opt_view_of(state, D, memory);
  for (int i = 0; i < D; ++i) { v.x[i] = x0[i]; v.xt[i] = x0[i]; }
  v.hdr[HBO_ACQ_OPT_S_CUR] = NAN;
  v.hdr[HBO_ACQ_OPT_S_MAGIC] = HBO_ACQ_OPT_MAGIC;
}
