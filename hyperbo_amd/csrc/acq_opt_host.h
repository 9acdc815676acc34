// What the callers of the control kernel of acq_opt_ctl.h share (acq_opt.hip: hbo_acq_maximize over the acquisition kernel;
// path_opt.hip: hbo_paths_maximize over the path kernel): the control text itself, the kernel's arguments and launch, and the
// host-side checks of options, state and box.  The definitions are in acq_opt.hip.
#pragma once
#include "api_internal.h"
#define HBO_LBFGS_FN static __host__ __device__ inline
#include "acq_opt_ctl.h"

static_assert(sizeof(hbo_acq_opt_opts) == sizeof(hbo_acq_opt_opts_ctl) && sizeof(hbo_acq_opt_eval) == sizeof(hbo_acq_opt_eval_ctl), "acq_opt_ctl.h restates hbo.h");
static_assert(HBO_ACQ_OPT_START == HBO_ACQ_OPT_CTL_START && HBO_ACQ_OPT_MAIN == HBO_ACQ_OPT_CTL_MAIN && HBO_ACQ_OPT_LINE_SEARCH == HBO_ACQ_OPT_CTL_LINE_SEARCH &&
              HBO_ACQ_OPT_IDLE == HBO_ACQ_OPT_CTL_IDLE && HBO_ACQ_OPT_RUNNING == HBO_ACQ_OPT_CTL_RUNNING && HBO_ACQ_OPT_CONVERGED == HBO_ACQ_OPT_CTL_CONVERGED &&
              HBO_ACQ_OPT_FTOL == HBO_ACQ_OPT_CTL_FTOL && HBO_ACQ_OPT_NO_PROGRESS == HBO_ACQ_OPT_CTL_NO_PROGRESS &&
              HBO_ACQ_OPT_NONFINITE_AT_START == HBO_ACQ_OPT_CTL_NONFINITE_AT_START && HBO_ACQ_OPT_STEPS_DONE == HBO_ACQ_OPT_CTL_STEPS_DONE,
              "acq_opt_ctl.h restates hbo.h");

struct AcqOptArgs {
  hbo_acq_opt_opts_ctl o;
  double* state; int64_t ns;        // [R][ns]
  const double* lo; const double* hi;   // [D] each
  void* pending;                    // [R][D] model dtype: the queries of the next evaluation launch
  const double* vals;               // [S][R] fp64 values of the pending points
  const double* grads;              // [S][R][D]
  hbo_acq_opt_eval_ctl* log;        // nullable [evals][R]
  int D, R, S;
  int reduce;                       // HBO_ACQ_OPT_REDUCE_* (acq_opt_ctl.h); 0: the mean
};

enum { ACQ_OPT_LDS_MAX = 65536 };
size_t acq_opt_lds_bytes(int64_t ns);
// one control workgroup per start (a.R of them): evaluation `slot` of the call
void launch_acq_opt_ctl(int dtype, const AcqOptArgs& a, int slot, hipStream_t st);
int acq_opt_check_opts(hbo_ctx* c, const std::string& fn, const hbo_acq_opt_opts* o);
hbo_acq_opt_opts_ctl acq_opt_ctl_opts(const hbo_acq_opt_opts* o);
int acq_opt_check_state(hbo_ctx* c, const std::string& fn, const double* h, const hbo_acq_opt_opts* o, bool* fresh);
int acq_opt_check_box(hbo_ctx* c, const std::string& fn, const double* lo, const double* hi, int D, int dtype);
bool acq_opt_in_box(const double* x, const double* lo, const double* hi, int D);
