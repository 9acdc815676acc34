// Stand-alone comparison of obj_plan and the gradient scatter table (hyperbo_amd/csrc/api_internal.h) with the expressions that
// objective_local held inline before it was split into plan, set-up and steps (profiles/objective_refactor.md).  No GPU, no libhbo,
// host code only:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g tools/objective_plan_check.cpp -o tools/objective_plan_check && tools/objective_plan_check
// and once more with  -fsanitize=address,undefined -fno-sanitize-recover=all  on the same line.
// Part 1: every field of the plan over objective x want_grad x sharded x dtype x T x max_nblk x aligned columns x the options
// lookahead / sweep / small_fused x LDS per block x the model grid.  Part 2: the table as the device words and as the host walk over
// the model grid (up to eight MLP layers, with and without Kumaraswamy) against the two constructions objective_local had.  The old
// device map is only built where it fits its own buffer (out_stride + 3 * 2 * HBO_MAX_MLP_LAYERS ints); the models where it does not
// are listed: they are the overflow the table closes.  Exit 0 and "ran clean" when nothing differs.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../hyperbo_amd/csrc/api_internal.h"

// ---- link seams: what the plan and the table call that lives in translation units with device code, as it is defined there
// (the schedules' policy -- use_sweep, sweep_group, small_limit -- is sched.h's own: inv_plan) ----
static bool use_early_trtri(const hbo_ctx* c, int ntasks, int max_nblk) { return use_lookahead(c, ntasks, max_nblk) && c->opt_overlap_trtri && max_nblk >= 4; }   // (before: sched.h)
thread_local std::string hbo_g_err;
int small_eval_lds(int dtype) { return dtype == HBO_F64 ? 132 * 1024 : 68 * 1024; }   // small.hip (to the KB: the plan only compares it with lds_per_block)
int grad_nacc(int kernel_id, int fdim) { return (kernel_id == HBO_KERNEL_DOT ? 3 : 2 + fdim) + 1; }   // grad.hip
extern "C" int hbo_grad_layout_of(const hbo_model* m, hbo_grad_layout* out) {   // api.hip
  int pos = 0;
  const bool dot = m->kernel_id == HBO_KERNEL_DOT;
  out->lengthscale = dot ? -1 : pos; if (!dot) pos += m->n_lengthscale;
  out->signal_variance = dot ? -1 : pos; if (!dot) pos += 1;
  out->noise_variance = pos++;
  out->constant = (m->mean_id == HBO_MEAN_CONSTANT) ? pos++ : -1;
  out->dot_prod_sigma = dot ? pos++ : -1;
  out->dot_prod_bias = dot ? pos++ : -1;
  const int fm = mean_feature_dim(m);
  out->linear_kernel = fm ? pos : -1; pos += fm;
  out->linear_bias = fm ? pos++ : -1;
  for (int l = 0; l < HBO_MAX_MLP_LAYERS; ++l) { out->mlp_kernel[l] = -1; out->mlp_bias[l] = -1; }
  if (needs_mlp(m)) {
    int fin = m->input_dim;
    for (int l = 0; l < m->n_layers; ++l) {
      out->mlp_kernel[l] = pos; pos += fin * m->features[l];
      out->mlp_bias[l] = pos; pos += m->features[l];
      fin = m->features[l];
    }
  }
  if (is_kumar(m)) pos += 2 * m->input_dim;
  out->total = pos;
  return HBO_OK;
}
extern "C" int hbo_grad_layout_kumar_of(const hbo_model* m, int32_t* a_off, int32_t* b_off) {   // api.hip
  hbo_grad_layout lay;
  hbo_grad_layout_of(m, &lay);
  *a_off = is_kumar(m) ? lay.total - 2 * m->input_dim : -1;
  *b_off = is_kumar(m) ? lay.total - m->input_dim : -1;
  return HBO_OK;
}

namespace {

long long n_cases = 0, n_bad = 0;
const char* where_model = "";   // the model of the case at hand, beside the `where` of its shape and options
void differ(const char* what, long long a, long long b, const char* where) {
  if (a == b) return;
  if (++n_bad <= 20) std::printf("DIFFERENT %s: before %lld, now %lld  (%s; %s)\n", what, a, b, where, where_model);
}

// ---- the model grid ------------------------------------------------------------------------------------------------------
const double some_values[HBO_MAX_FEATURE_DIM] = {1.0};
struct Model { hbo_model_kumar k; char name[96]; };
// the four kernels x with / without an MLP basis x the four means x Kumaraswamy on / off x lengthscales 1 / per feature x `layers`
std::vector<Model> model_grid(const std::vector<int>& layer_counts, int dtype) {
  std::vector<Model> out;
  for (int kernel = 0; kernel <= HBO_KERNEL_DOT; ++kernel) for (int basis = 0; basis < 2; ++basis) for (int mean = 0; mean <= HBO_MEAN_LINEAR_MLP; ++mean)
  for (int kumar = 0; kumar < 2; ++kumar) for (int ard = 0; ard < 2; ++ard) for (int L : layer_counts) {
    Model md; std::memset(&md.k, 0, sizeof md.k);
    hbo_model& m = md.k.base;
    m.kernel_id = kernel; m.mean_id = mean; m.dtype = dtype; m.input_dim = 5; m.kernel_uses_mlp = basis;
    const bool mlp = basis || mean == HBO_MEAN_LINEAR_MLP;
    if (!mlp && L != layer_counts[0]) continue;   // the layer count only matters with an MLP
    m.n_layers = mlp ? L : 0;
    for (int l = 0; l < m.n_layers; ++l) { m.features[l] = 3 + l; m.mlp_kernel[l] = some_values; m.mlp_bias[l] = some_values; }
    m.n_lengthscale = ard ? feature_dim(&m) : 1;
    m.input_warp = kumar ? HBO_WARP_KUMAR : HBO_WARP_NONE;
    m.lengthscale = some_values; m.linear_kernel = some_values; md.k.kumar_a = md.k.kumar_b = some_values;
    if (validate_model(nullptr, &m) != HBO_OK) continue;   // (a Kumaraswamy warp with an MLP basis: refused before any plan is made)
    std::snprintf(md.name, sizeof md.name, "kernel %d basis %d mean %d kumar %d ard %d layers %d", kernel, basis, mean, kumar, ard, m.n_layers);
    out.push_back(md);
  }
  return out;
}

// ---- part 1: the plan ----------------------------------------------------------------------------------------------------
// objective_local's own expressions as they stood in one scope, in their order; `st` / `stream2` stand in as 0 / 1
void check_plan(const hbo_ctx* c, const hbo_model* m, const hbo_dataset* ds, int objective, bool want_grad, bool sharded, const char* where) {
  hbo_grad_layout lay;
  hbo_grad_layout_of(m, &lay);
  const ObjPlan p = obj_plan(c, m, ds, lay, objective, want_grad, sharded);
  ++n_cases;
  const bool kumar = is_kumar(m);
  const int obj = objective;
  const bool euc = obj == OBJ_EUC;
  const int T = ds ? ds->ntasks : 0;
  const int red_count = 2 + (want_grad ? lay.total : 0);
  differ("red_count", red_count, p.red_count, where); differ("T", T, p.T, where); differ("sharded", sharded, p.sharded, where);
  if (T == 0) return;
  bool extras = false;
  if (obj != OBJ_NLL) for (TaskHost* t : ds->tasks) if (t->m + 1 > HBO_TILE) extras = true;
  const int dtype = ds->dtype;
  const bool small_ok = c->opt_small_fused && ds && small_eval_lds(ds->dtype) <= c->lds_per_block;
  const bool lds_only = obj == OBJ_NLL && ds->max_nblk == 1 && small_ok && !needs_mlp(m) && !(kumar && want_grad);
  const bool need_S = (want_grad || extras) && !euc;
  int64_t max_n = 0;
  for (int k = 0; k < T; ++k) max_n = std::max<int64_t>(max_n, ds->tasks[k]->n);
  const int out_stride = (m->kernel_id == HBO_KERNEL_DOT ? 0 : m->n_lengthscale) + 6 + mean_feature_dim(m);
  const size_t pack_bytes = sizeof(double) * T * (1 + (size_t)out_stride) + sizeof(int) * T;
  const bool info_fill = !(obj == OBJ_NLL && ds->max_nblk == 1 && small_ok);
  const int max_nblk = ds->max_nblk, max_npad = max_nblk * HBO_TILE;
  const bool fused_small = obj == OBJ_NLL && max_nblk == 1 && small_ok;
  differ("dtype", dtype, p.dtype, where); differ("euc", euc, p.euc, where); differ("kumar", kumar, p.kumar, where); differ("mlp", needs_mlp(m), p.mlp, where);
  differ("extras", extras, p.extras, where); differ("small_ok", small_ok, p.small_ok, where); differ("lds_only", lds_only, p.lds_only, where);
  differ("need_S", need_S, p.need_S, where); differ("max_n", max_n, p.max_n, where); differ("out_stride", out_stride, p.out_stride, where);
  differ("pack_bytes", (long long)pack_bytes, (long long)p.pack_bytes, where); differ("info fill", info_fill, !p.fused_small, where);
  differ("max_nblk", max_nblk, p.max_nblk, where); differ("max_npad", max_npad, p.max_npad, where); differ("fused_small", fused_small, p.fused_small, where);
  if (fused_small) { differ("contract", 0, p.contract, where); return; }   // the single launch: nothing below was evaluated
  int qs = 4;
  int side = 0;
  const bool la = use_lookahead(c, T, max_nblk);
  const bool sweep = want_grad && !euc && use_sweep(c, dtype, T, max_nblk);
  if (sweep) qs = c->opt_sweep_qs > 0 ? c->opt_sweep_qs : sweep_group(T, max_nblk);
  const bool early_trtri = !sweep && want_grad && use_early_trtri(c, T, max_nblk);
  if (!euc) side = (want_grad && obj == OBJ_NLL && la) ? 1 : 0;
  const bool value_inverse = extras && !euc && !want_grad;
  const int fdim = feature_dim(m);
  const int nacc = grad_nacc(m->kernel_id, fdim);
  const int64_t stride_task = (int64_t)(max_nblk * (max_nblk + 1)) * nacc;
  differ("la", la, p.la, where); differ("sweep", sweep, p.inv.sweep, where); differ("early_trtri", early_trtri, p.inv.early, where);
  if (sweep) differ("qs", qs, p.inv.qs, where);
  differ("side stream", side, p.side_reduce, where); differ("value_inverse", value_inverse, p.value_inverse, where);
  differ("fdim", fdim, p.fdim, where); differ("nacc", nacc, p.nacc, where); differ("stride_task", stride_task, p.stride_task, where);
  differ("contract", want_grad || euc, p.contract, where);
  if (want_grad || euc) {
    const size_t pb = sizeof(double) * (stride_task * T + (size_t)HBO_GRAD_PRE_ROWS * nacc * T);
    differ("partials bytes", (long long)pb, (long long)p.partials_bytes, where);
  }
}

void part_plan() {
  hbo_ctx c;
  std::vector<std::unique_ptr<TaskHost>> tasks;
  for (int dtype : {HBO_F32, HBO_F64}) {
    const std::vector<Model> models = model_grid({2}, dtype);
    for (int T : {0, 1, 2, 8, 64}) for (int max_nblk : {1, 2, 4, 5, 8, 17, 18, 48, 49}) for (int m1 : {1, 128, 129}) {
      // the dataset's shape: task 0 is the longest, the last task carries the aligned columns under test
      hbo_dataset ds;
      ds.dtype = dtype; ds.D = 5; ds.ntasks = T; ds.max_nblk = T ? max_nblk : 0;
      tasks.clear();
      for (int k = 0; k < T; ++k) {
        tasks.emplace_back(new TaskHost);
        tasks[k]->n = std::max(1, max_nblk * HBO_TILE - 3 - 7 * k); tasks[k]->m = k == T - 1 ? m1 - 1 : 1;
        ds.tasks.push_back(tasks[k].get());
      }
      for (int objective : {HBO_OBJ_NLL, HBO_OBJ_EKL, HBO_OBJ_EUC}) for (int want_grad = 0; want_grad < 2; ++want_grad) for (int sharded = 0; sharded < 2; ++sharded)
      for (int lookahead = 0; lookahead < 3; ++lookahead) for (int sweep = 0; sweep < 3; ++sweep) for (int small_fused = 0; small_fused < 2; ++small_fused)
      for (int lds : {64 * 1024, 160 * 1024}) for (int sweep_qs : {0, 2}) {
        c.opt_lookahead = lookahead; c.opt_sweep = sweep; c.opt_small_fused = small_fused; c.lds_per_block = lds; c.opt_sweep_qs = sweep_qs;
        char where[256];
        std::snprintf(where, sizeof where, "dtype %d T %d nblk %d m+1 %d obj %d grad %d sharded %d lookahead %d sweep %d small_fused %d lds %d qs %d",
                      dtype, T, max_nblk, m1, objective, want_grad, sharded, lookahead, sweep, small_fused, lds, sweep_qs);
        for (const Model& md : models) {
        where_model = md.name;
        check_plan(&c, &md.k.base, &ds, objective, want_grad != 0, sharded != 0, where);
        if (T == 0 && sharded) check_plan(&c, &md.k.base, nullptr, objective, want_grad != 0, true, where);   // a sharded call without a dataset
        }
      }
      ds.tasks.clear();
    }
  }
}

// ---- part 2: the scatter table -------------------------------------------------------------------------------------------
void part_scatter() {
  const int T = 3;
  long long listed = 0;
  for (int layers_hi : {1, 3, HBO_MAX_MLP_LAYERS}) for (const Model& md : model_grid({layers_hi}, HBO_F64)) for (int want_grad = 0; want_grad < 2; ++want_grad) {
    const hbo_model* m = &md.k.base;
    const bool kumar = is_kumar(m);
    hbo_grad_layout lay;
    hbo_grad_layout_of(m, &lay);
    const int out_stride = (m->kernel_id == HBO_KERNEL_DOT ? 0 : m->n_lengthscale) + 6 + mean_feature_dim(m);
    int32_t ka = -1, kb = -1;
    if (kumar) hbo_grad_layout_kumar_of(m, &ka, &kb);
    std::unique_ptr<GradScatter> tab(new GradScatter);   // (on the heap here so that the sanitizer sees its exact extent)
    grad_scatter_fill(*tab, m, lay, ka, kb, out_stride, want_grad != 0);
    ++n_cases;
    // the device map as objective_local built it for the sharded path
    const int n_ls = m->kernel_id == HBO_KERNEL_DOT ? 0 : m->n_lengthscale;
    const int fm = mean_feature_dim(m);
    const int seg_needed = want_grad ? (kumar ? 2 : 0) + (needs_mlp(m) ? 2 * m->n_layers : 0) : 0;
    if (seg_needed > 2 * HBO_MAX_MLP_LAYERS) {
      if (++listed <= 40) std::printf("the old device map does not fit its buffer (%d ints into room for %d): %s\n", 3 * seg_needed, 3 * 2 * HBO_MAX_MLP_LAYERS, md.name);
      differ("nseg (worst case)", seg_needed, tab->nseg, md.name);
    } else {
      std::vector<int> hmap(out_stride + 3 * 2 * HBO_MAX_MLP_LAYERS, -1);
      if (want_grad) {
        for (int d = 0; d < n_ls; ++d) hmap[d] = lay.lengthscale < 0 ? -1 : lay.lengthscale + d;
        hmap[n_ls] = lay.signal_variance; hmap[n_ls + 1] = lay.noise_variance; hmap[n_ls + 2] = lay.constant;
        hmap[n_ls + 3] = lay.dot_prod_sigma; hmap[n_ls + 4] = lay.dot_prod_bias;
        for (int d = 0; d < fm; ++d) hmap[n_ls + 5 + d] = lay.linear_kernel < 0 ? -1 : lay.linear_kernel + d;
        hmap[n_ls + 5 + fm] = lay.linear_bias;
      }
      int nseg = 0;
      if (want_grad && kumar) {
        int32_t ao = -1, bo = -1;
        hbo_grad_layout_kumar_of(m, &ao, &bo);
        int* sg = hmap.data() + out_stride;
        sg[0] = ao; sg[1] = 0; sg[2] = m->input_dim; sg[3] = bo; sg[4] = m->input_dim; sg[5] = m->input_dim; nseg = 2;
      }
      if (want_grad && needs_mlp(m)) {
        int pos = 0, fin0 = m->input_dim;
        for (int l = 0; l < m->n_layers; ++l) {
          const int wn = fin0 * m->features[l], bn = m->features[l];
          int* sg = hmap.data() + out_stride + 3 * nseg;
          sg[0] = lay.mlp_kernel[l]; sg[1] = pos; sg[2] = wn; ++nseg; pos += wn;
          sg += 3; sg[0] = lay.mlp_bias[l]; sg[1] = pos; sg[2] = bn; ++nseg; pos += bn;
          fin0 = m->features[l];
        }
      }
      differ("nseg", nseg, tab->nseg, md.name);
      differ("device words", 0, std::memcmp(hmap.data(), tab->w, sizeof(int) * hmap.size()) != 0, md.name);
    }
    for (size_t i = out_stride + 3 * tab->nseg; i < tab->bytes() / sizeof(int); ++i) differ("unused segment word", -1, tab->w[i], md.name);
    if (!want_grad) continue;
    // the host finish: results as they come back (one task failed, or none), the summed leaves, against the loop with the `add` lambda
    size_t mlp_elems = kumar ? (size_t)2 * m->input_dim : 0;
    if (needs_mlp(m)) { size_t tot = 0; int fin0 = m->input_dim; for (int l = 0; l < m->n_layers; ++l) { tot += (size_t)fin0 * m->features[l] + m->features[l]; fin0 = m->features[l]; } mlp_elems = std::max(mlp_elems, tot); }
    for (int bad_task : {-1, 1}) {
      std::unique_ptr<double[]> h_grad_buf(new double[(size_t)T * out_stride]), h_mlp(new double[std::max<size_t>(mlp_elems, 1)]);
      std::unique_ptr<int[]> h_info_buf(new int[T]);
      std::unique_ptr<double[]> before(new double[lay.total]), now(new double[lay.total]);
      const double* h_grad = h_grad_buf.get(); const int* h_info = h_info_buf.get();
      for (size_t i = 0; i < (size_t)T * out_stride; ++i) h_grad_buf[i] = 0.25 + 0.001 * (double)i;
      for (size_t i = 0; i < mlp_elems; ++i) h_mlp[i] = -3.0 - 0.01 * (double)i;
      for (int k = 0; k < T; ++k) h_info_buf[k] = k == bad_task ? 7 : INT_MAX;
      for (int i = 0; i < lay.total; ++i) before[i] = now[i] = 0;
      const bool notpd = bad_task >= 0;
      double* grad_sum = before.get();
      for (int k = 0; k < T; ++k) {
        const double* o = h_grad + (size_t)k * out_stride;
        const bool bad = h_info[k] != INT_MAX;
        auto add = [&](int off, double v) { if (off >= 0) grad_sum[off] += bad ? NAN : v; };
        for (int d = 0; d < n_ls; ++d) add(lay.lengthscale < 0 ? -1 : lay.lengthscale + d, o[d]);
        add(lay.signal_variance, o[n_ls]);
        add(lay.noise_variance, o[n_ls + 1]);
        add(lay.constant, o[n_ls + 2]);
        add(lay.dot_prod_sigma, o[n_ls + 3]);
        add(lay.dot_prod_bias, o[n_ls + 4]);
        for (int d = 0; d < fm; ++d) add(lay.linear_kernel + d, o[n_ls + 5 + d]);
        add(lay.linear_bias, o[n_ls + 5 + fm]);
      }
      if (needs_mlp(m)) {
        size_t pos = 0; int fin0 = m->input_dim;
        for (int l = 0; l < m->n_layers; ++l) {
          const size_t wn = (size_t)fin0 * m->features[l], bn = m->features[l];
          for (size_t i = 0; i < wn; ++i) grad_sum[lay.mlp_kernel[l] + i] = notpd ? NAN : h_mlp[pos + i];
          pos += wn;
          for (size_t i = 0; i < bn; ++i) grad_sum[lay.mlp_bias[l] + i] = notpd ? NAN : h_mlp[pos + i];
          pos += bn; fin0 = m->features[l];
        }
      }
      if (kumar) {
        int32_t ao = -1, bo = -1;
        hbo_grad_layout_kumar_of(m, &ao, &bo);
        for (int d = 0; d < m->input_dim; ++d) {
          grad_sum[ao + d] = notpd ? NAN : h_mlp[d];
          grad_sum[bo + d] = notpd ? NAN : h_mlp[m->input_dim + d];
        }
      }
      grad_scatter_host(*tab, T, h_grad, h_info, h_mlp.get(), notpd, now.get());
      ++n_cases;
      differ("host walk", 0, std::memcmp(before.get(), now.get(), sizeof(double) * lay.total) != 0, md.name);
    }
  }
  std::printf("scatter table: %lld model(s) whose old device map does not fit its buffer\n", listed);
}

}  // namespace

int main() {
  part_plan();
  std::printf("plan: %lld cases\n", n_cases);
  part_scatter();
  std::printf("%lld cases, %lld difference(s)\n", n_cases, n_bad);
  std::printf(n_bad ? "FAILED\n" : "ran clean\n");
  return n_bad ? 1 : 0;
}
