// Stand-alone run of the control code of hbo_acq_maximize (hyperbo_amd/csrc/acq_opt_ctl.h, the text acq_opt_ctl_kernel and
// hbo_probe_acq_opt_ctl compile) for a build with host sanitizers.  No GPU, no libhbo:
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/acq_opt_ctl_check.cpp -o tools/acq_opt_ctl_check && tools/acq_opt_ctl_check
// Three runs on heap arrays of exactly the sizes the code is told, S = 3 samples each (the function split into three unequal parts): a
// D = 300 quadratic in [0, 1]^D whose minimiser lies on a face (more than one pass of the 256 partial sums, the ring of 10 pairs
// wraps), the 2-D Rosenbrock function in [0, 1]^2 (minimiser in the corner (1, 1)), and a function that is NaN everywhere.  Exit 0 and
// "ran clean" when every run ends where it should.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>

#include "../hyperbo_amd/csrc/acq_opt_ctl.h"

namespace {

struct Run { int evals = 0, status = 0, main_steps = 0; double f = 0; std::vector<double> x; bool monotone = true, inside = true; };

// f(x, g) is the function to MINIMISE; the control code is handed S = 3 "acquisition" samples whose mean is -f
Run drive(int D, const hbo_acq_opt_opts_ctl& o, const std::vector<double>& x0, const std::function<double(const double*, double*)>& f) {
  const int S = 3;
  const double w[S] = {1.5, -0.25, 1.75};   // sum = S
  const int64_t ns = hbo_acq_opt_state_size(D, o.memory);
  std::unique_ptr<double[]> state(new double[ns]);
  std::memset(state.get(), 0, sizeof(double) * ns);
  std::unique_ptr<double[]> scratch(new double[HBO_LBFGS_PARTIALS]);
  std::unique_ptr<double[]> vals(new double[S]), grads(new double[(size_t)S * D]), g(new double[D]);
  hbo_acq_opt_state_start(state.get(), D, o.memory, x0.data());
  const hbo_acq_opt_view v = hbo_acq_opt_view_of(state.get(), D, o.memory);
  Run r;
  double last = INFINITY;
  for (;;) {
    std::unique_ptr<double[]> point(new double[D]);
    std::memcpy(point.get(), v.xt, sizeof(double) * D);
    for (int i = 0; i < D; ++i) r.inside = r.inside && point[i] >= 0.0 && point[i] <= 1.0;
    const double value = f(point.get(), g.get());
    for (int s = 0; s < S; ++s) { vals[s] = -w[s] * value; for (int i = 0; i < D; ++i) grads[(size_t)s * D + i] = -w[s] * g[i]; }
    hbo_acq_opt_eval_ctl ev;
    hbo_acq_opt_ctl_step(state.get(), D, o, nullptr, nullptr, 0, vals.get(), 1, grads.get(), D, S, 0, 1, scratch.get(), &ev);
    r.evals += 1;
    if (ev.kind == HBO_ACQ_OPT_CTL_START || ev.kind == HBO_ACQ_OPT_CTL_MAIN) { r.monotone = r.monotone && !(ev.value > last); last = ev.value; }
    if (ev.kind == HBO_ACQ_OPT_CTL_MAIN) r.main_steps = ev.iter;
    r.status = (int)state[HBO_ACQ_OPT_S_STATUS];
    if (r.status != HBO_ACQ_OPT_CTL_RUNNING || r.evals > 100000) break;
  }
  r.f = state[HBO_ACQ_OPT_S_CUR];
  r.x.assign(v.x, v.x + D);
  return r;
}

int check(bool ok, const char* what) {
  if (!ok) std::printf("FAILED: %s\n", what);
  return ok ? 0 : 1;
}

}  // namespace

int main() {
  int bad = 0;
  hbo_acq_opt_opts_ctl o;
  o.memory = 10; o.ls_steps = 20; o.max_iters = 200; o.c1 = 1e-4; o.tau = 0.5; o.pgtol = 1e-5; o.ftol = 2.2e-9;

  {   // quadratic 0.5 sum lam_i (x_i - c_i)^2, D = 300: every third centre lies outside the box, so the minimiser is on a face
    const int D = 300;
    std::vector<double> lam(D), c(D), x0(D);
    for (int i = 0; i < D; ++i) {
      lam[i] = 1.0 + 39.0 * i / (D - 1);
      c[i] = i % 3 == 0 ? 1.25 + 0.001 * i : (i % 3 == 1 ? -0.5 : 0.3 + 0.001 * i);
      x0[i] = 0.5 + 0.4 * cos((double)i);
    }
    auto f = [&](const double* x, double* g) { double s = 0; for (int i = 0; i < D; ++i) { const double d = x[i] - c[i]; s += lam[i] * d * d; g[i] = lam[i] * d; } return 0.5 * s; };
    const Run r = drive(D, o, x0, f);
    double err = 0;
    bool exact = true;
    for (int i = 0; i < D; ++i) {
      const double want = c[i] > 1.0 ? 1.0 : (c[i] < 0.0 ? 0.0 : c[i]);
      err = std::fmax(err, std::fabs(r.x[i] - want));
      if (c[i] > 1.0 || c[i] < 0.0) exact = exact && r.x[i] == want;
    }
    std::printf("quadratic: %d evaluations, %d main steps, status %d, f %.9g, |x - x*|_inf %.3g\n", r.evals, r.main_steps, r.status, r.f, err);
    // (an FTOL stop at f ~ 465 leaves a decrease of at most 2.2e-9 f ~ 1e-6 on the table: with curvatures of 1 .. 40 that is |x - x*| ~ 1e-3)
    bad += check((r.status == HBO_ACQ_OPT_CTL_CONVERGED || r.status == HBO_ACQ_OPT_CTL_FTOL) && err < 5e-3 && exact && r.monotone && r.inside &&
                 r.main_steps > 10, "quadratic: ends on the face, bounds hit exactly, more than 10 main steps");
  }
  {   // Rosenbrock in [0, 1]^2
    auto f = [](const double* x, double* g) {
      const double a = x[0], b = x[1];
      g[0] = -2 * (1 - a) - 400 * a * (b - a * a); g[1] = 200 * (b - a * a);
      return (1 - a) * (1 - a) + 100 * (b - a * a) * (b - a * a);
    };
    const Run r = drive(2, o, {0.1, 0.9}, f);
    std::printf("rosenbrock: %d evaluations, %d main steps, status %d, f -> %.6g at (%.6f, %.6f)\n", r.evals, r.main_steps, r.status, r.f, r.x[0], r.x[1]);
    bad += check(r.status != HBO_ACQ_OPT_CTL_RUNNING && r.status != HBO_ACQ_OPT_CTL_NONFINITE_AT_START && r.f < 1e-6 && r.monotone && r.inside,
                 "rosenbrock: f < 1e-6 inside the box");
  }
  {   // NaN everywhere
    auto f = [](const double*, double* g) { g[0] = NAN; g[1] = NAN; g[2] = NAN; return (double)NAN; };
    const Run r = drive(3, o, {0.5, 0.0, 1.0}, f);
    std::printf("nan: %d evaluations, status %d\n", r.evals, r.status);
    bad += check(r.status == HBO_ACQ_OPT_CTL_NONFINITE_AT_START && r.evals == 1 && r.x[0] == 0.5 && r.x[1] == 0.0 && r.x[2] == 1.0,
                 "nan: one evaluation, non-finite at the start, x unchanged");
  }
  std::printf(bad ? "%d check(s) failed\n" : "ran clean\n", bad);
  return bad ? 1 : 0;
}
