// Stand-alone run of the L-BFGS control code (hyperbo_amd/csrc/lbfgs_ctl.h, the text lbfgs_ctl_kernel and hbo_probe_lbfgs_ctl compile)
// for a build with host sanitizers.  No GPU, no libhbo:
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/lbfgs_ctl_check.cpp -o tools/lbfgs_ctl_check && tools/lbfgs_ctl_check
// Three runs on heap arrays of exactly the sizes the code is told: a P = 300 quadratic over 25 main steps (more than one pass of the
// 256 partial sums, the ring of 10 pairs wraps), Rosenbrock from (-1.2, 1), and a function that is NaN everywhere.  Exit 0 and
// "ran clean" when every run ends as lbfgs.lbfgs would.
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>

#include "../hyperbo_amd/csrc/lbfgs_ctl.h"

namespace {

struct Run { int evals = 0, status = 0, main_steps = 0; double last_value = 0; std::vector<double> x; };

Run drive(int P, const hbo_lbfgs_opts_ctl& o, const std::vector<double>& x0, const std::function<double(const double*, double*)>& f) {
  const int64_t ns = hbo_lbfgs_state_size(P, o.memory);
  std::unique_ptr<double[]> state(new double[ns]);
  std::memset(state.get(), 0, sizeof(double) * ns);
  std::unique_ptr<double[]> scratch(new double[HBO_LBFGS_PARTIALS]);
  hbo_lbfgs_state_start(state.get(), P, o.memory, x0.data());
  const hbo_lbfgs_view v = hbo_lbfgs_view_of(state.get(), P, o.memory);
  Run r;
  for (;;) {
    std::unique_ptr<double[]> point(new double[P]);
    std::memcpy(point.get(), v.xt, sizeof(double) * P);
    const double value = f(point.get(), v.g);
    hbo_lbfgs_eval_ctl ev;
    hbo_lbfgs_ctl_step(state.get(), P, o, value, 0, 1, scratch.get(), &ev);
    r.evals += 1;
    r.last_value = value;
    if (ev.kind == HBO_LBFGS_CTL_MAIN) r.main_steps = ev.iter;
    r.status = (int)state[HBO_LBFGS_S_STATUS];
    if (r.status != HBO_LBFGS_CTL_RUNNING || r.evals > 100000) break;
  }
  r.x.assign(v.x, v.x + P);
  return r;
}

int check(bool ok, const char* what) {
  if (!ok) std::printf("FAILED: %s\n", what);
  return ok ? 0 : 1;
}

}  // namespace

int main() {
  int bad = 0;
  hbo_lbfgs_opts_ctl o;
  o.memory = 10; o.ls_steps = 50; o.max_iters = 25; o.alpha = 1.0; o.tol = 1e-30; o.c1 = 1e-4; o.c2 = 0.9; o.grow = 2.1; o.tau = 0.5;

  {   // quadratic, P = 300
    const int P = 300;
    std::vector<double> lam(P), x0(P);
    for (int i = 0; i < P; ++i) { lam[i] = 1.0 + 39.0 * i / (P - 1); x0[i] = cos((double)i) + 1.5; }
    auto f = [&](const double* x, double* g) { double s = 0; for (int i = 0; i < P; ++i) { s += lam[i] * x[i] * x[i]; g[i] = lam[i] * x[i]; } return 0.5 * s; };
    std::vector<double> g0(P);
    const double f0 = f(x0.data(), g0.data());
    const Run r = drive(P, o, x0, f);
    std::vector<double> g(P);
    const double f1 = f(r.x.data(), g.data());
    std::printf("quadratic: %d evaluations, %d main steps, status %d, f %.6g -> %.6g\n", r.evals, r.main_steps, r.status, f0, f1);
    bad += check(r.status == HBO_LBFGS_CTL_STEPS_DONE && r.main_steps == 25 && f1 < 1e-6 * f0, "quadratic: 25 main steps, then steps done");
  }
  {   // Rosenbrock
    o.tol = 1e-14;
    auto f = [](const double* x, double* g) {
      const double a = x[0], b = x[1];
      g[0] = -2 * (1 - a) - 400 * a * (b - a * a); g[1] = 200 * (b - a * a);
      return (1 - a) * (1 - a) + 100 * (b - a * a) * (b - a * a);
    };
    const Run r = drive(2, o, {-1.2, 1.0}, f);
    double g[2];
    const double f1 = f(r.x.data(), g);
    std::printf("rosenbrock: %d evaluations, %d main steps, status %d, f -> %.6g\n", r.evals, r.main_steps, r.status, f1);
    bad += check(r.status == HBO_LBFGS_CTL_STEPS_DONE && r.evals == 60 && f1 < 0.242, "rosenbrock: 60 evaluations as lbfgs.lbfgs makes");
  }
  {   // NaN everywhere
    auto f = [](const double*, double* g) { g[0] = NAN; g[1] = NAN; g[2] = NAN; return (double)NAN; };
    const Run r = drive(3, o, {0.5, -1.0, 2.0}, f);
    std::printf("nan: %d evaluations, status %d\n", r.evals, r.status);
    bad += check(r.status == HBO_LBFGS_CTL_NO_PROGRESS && r.evals == 51 && r.x[0] == 0.5 && r.x[1] == -1.0 && r.x[2] == 2.0,
                 "nan: 1 + 50 evaluations, no progress, x unchanged");
  }
  std::printf(bad ? "%d check(s) failed\n" : "ran clean\n", bad);
  return bad ? 1 : 0;
}
