// The steps of hbo_dataset_create and hbo_dataset_subsample (dataset.hip) that make no HIP call: where a task's parts lie in the dataset's
// one input block, the TaskHost that points there, the tasks' final order, and the host statistics of a task's targets.  A header of
// its own so that tools/api_host_check.cpp compiles this same text without a device.
#pragma once
#include "api_internal.h"

// Where a task's three parts lie in the dataset's input block: x [n][D], the column sums of y [n], the divergence rows [m + 1][n]
// (ydiv 0 for a task without them: a sub-sample of a source that has none)
struct TaskOff { size_t x, ysum, ydiv; };
static TaskOff dataset_place(BlockLayout& lay, int64_t n, int D, int m, bool has_ydiv, size_t es) {
  return {lay.take((size_t)n * D * es), lay.take((size_t)n * es), has_ydiv ? lay.take((size_t)(m + 1) * n * es) : 0};   // (a braced list: in this order)
}
// a task of n points and m columns whose inputs lie at `o` of the dataset's block, appended to the dataset
static TaskHost* dataset_add_task(hbo_dataset* ds, int64_t n, int m, const TaskOff& o, bool has_ydiv) {
  TaskHost* t = new TaskHost();
  ds->tasks.push_back(t);
  t->owns_inputs = false; task_shape(t, n, m, ds->dtype);
  t->X = (char*)ds->d_inputs + o.x; t->ysum = (char*)ds->d_inputs + o.ysum;
  if (has_ydiv) t->ydiv = (char*)ds->d_inputs + o.ydiv;
  ds->max_nblk = std::max(ds->max_nblk, t->nblk);
  return t;
}
// largest tasks first: their tiles are dispatched first.  (Stable: ties keep the caller's order.  hbo_train_adam's batches follow the
// same order, train.hip.)
static void dataset_finish(hbo_dataset* ds) {
  ds->ntasks = (int)ds->tasks.size();
  std::stable_sort(ds->tasks.begin(), ds->tasks.end(), [](TaskHost* a, TaskHost* b) { return a->n > b->n; });
}
// The host statistics of a task's targets y [n][m]: ysum, the sum over the columns (in double, then cast), and the sample statistics
// of objectives.py:57-58 -- mu_data = mean over the m aligned columns, cov_data = (1/m) sum_a yc_a yc_a^T (jnp.cov(bias=True)) --
// kept as the m rank-1 factors (y_a - mu_data) / sqrt(m), then -mu_data: the (m + 1) x n rows of ydiv.
static void task_stats(const void* y, int64_t n, int m, int dtype, void* ysum_out, void* ydiv_out) {
  const double rs = 1.0 / sqrt((double)m);
  for (int64_t i = 0; i < n; ++i) {
    double sum = 0;
    for (int a = 0; a < m; ++a) sum += host_elem(y, dtype, i * m + a);
    if (dtype == HBO_F64) ((double*)ysum_out)[i] = sum; else ((float*)ysum_out)[i] = (float)sum;
    const double mu0 = sum / m;
    for (int a = 0; a <= m; ++a) {
      const double v = a < m ? (host_elem(y, dtype, i * m + a) - mu0) * rs : -mu0;
      if (dtype == HBO_F64) ((double*)ydiv_out)[(size_t)a * n + i] = v; else ((float*)ydiv_out)[(size_t)a * n + i] = (float)v;
    }
  }
}
