/* hbo_tune.h -- measurement hooks of libhbo.  NOT part of the drop-in boundary (include/hbo.h): nothing a caller of the
 * hyperbo.gp_utils surface needs.  The A/B tools under tools/ and the scheduling sweep of tests/test_gpu_fuzz.py use it to
 * vary where and when the same kernels run; no knob changes a result, and every non-default value was measured equal or worse
 * (profiles/r01_potrf_chain.md, r02_potrf_chain.md, r03_dag.md, r04_chain_and_sweep.md, r04_gemm_pipeline.md).  Names fall through to hbo_set_option.
 *
 *   overlap_trtri 0/1      inverse walks the block tree while the factorisation runs
 *   cu_yield      0..2     background GEMM workgroups pause while a panel-chain workgroup runs on their CU (1: potf2 only)
 *   persist_free  -1..200  CUs the persistent bulk update leaves with one workgroup (-1 = auto: 32)
 *   trtri_at      0..63    the overlapped inverse starts after this many 64ths of the panels (0 = auto: 5/8)
 *   trtri_free    0..200   CUs the co-running inverse products leave with one workgroup
 *   post_bf16x3 / syrk_bf16x3 / trtri_bf16x3 / lauum_bf16x3  0/1   the four parts of option bf16x3 separately
 *   trtri3_min_s  >=1      lowest level (in blocks) of the inverse that runs on the bf16 cores
 *   syrk3_free    0..200   fp32 trailing updates on the bf16 / fp16 cores: CUs the bulk update leaves with one workgroup (32)
 *   sweep         0..2     one-sweep inverse (W = L^-1 and K^-1 = W^T W row group by row group behind the panel chain): 0 never,
 *                          1 where measured faster (default: batches with look-ahead, one fp64 matrix of 17-48 blocks;
 *                          profiles/r04_chain_and_sweep.md, r04_gemm_pipeline.md), 2 wherever look-ahead is on
 *   sweep_qs      0..16    its row-group size in 128-blocks, a power of two (0 = auto: 4; 8 for one matrix above 28 blocks)
 *   sweep_free    1..200   CUs the sweep's persistent launches beside the chain leave with one workgroup (24; at most trtri_free)
 *   sweep_side    0/1      one matrix on 128-tiles: the sweep's K^-1 updates on a stream of their own (default 1: N = 6144 6.07 -> 5.71 ms)
 *   lauum_persist 0..128   one large matrix: K^-1 = W^T W and the big levels of the inverse behind the factorisation as resident grids drawing
 *                          their tiles from a counter (default 1; N = 8192 10.64 -> 10.51 ms; n > 1: K^-1 leaves n CUs free instead of 16)
 *   split_f1      0..2     the update of the next group's block columns (F1): only the next column on the panel stream, the later
 *                          ones on a third stream -- 0 never, 1 batches (default: 64 tasks 14.32 -> 14.12 ms), 2 always
 *   sweep_big     >=0      sweep launches of small / batched shapes with at least this many 128-tiles (x tasks) use 128-tiles (4000)
 *   post_f16x2    0/1      fp32 posterior product of the stationary covariances on the fp16 matrix cores from two-way splits (post3.hip: post2h_kernel;
 *                          default 1; 0 = bf16x3's exact three-way split)
 *   group_inner   -1..16   two-level panel groups: the chain's left-looking column updates stay inside inner groups of this many panels, one
 *                          update per inner boundary brings the rest of the (outer, potrf_group) group up to date; 0 = one level, -1 = auto
 *                          (8 inside groups of 16 for one fp32 matrix above 96 blocks: cfg 3's factor 18.5 -> 18.1 ms)
 *   chol_f16x2    0/1      fp32 factorisations of the stationary covariances (the objective / factor paths, which know max A_ii = signal variance +
 *                          noise + jitter): trailing updates, the inverse's bf16-core levels and K^-1 = W^T W from two-way fp16 splits
 *                          (post3.hip: syrk3_kernel<true>; default 1; 0 = the exact three-way bf16 splits, which hbo_spd_* and the
 *                          dot-product kernel always use)
 *   post_serial   0/1      streamed posterior: features + cross Gram of chunk i+1 on the SAME stream as the product of chunk i
 *                          (nothing overlaps: the stage times of hbo_profile are then each kernel's isolated time; bench.py cfg3)
 *   small_fused   0/1      batches whose tasks all have n <= 128: the single-workgroup evaluation (small.hip; default 1)
 *   poison        0/1      tests: an evaluation (objective / factor paths on the blocked pipeline) first fills what it is about to recompute --
 *                          the lower triangles of A and W, all of S, alpha, d f / d mu -- with NaN, so that a launch that skips work shows up
 *                          as NaN instead of hiding behind an earlier evaluation's identical numbers in the same pooled buffers; tests/conftest.py
 *                          turns it on for the whole GPU tier (default 0).  The per-evaluation scratch of hbo_acq_maximize (per-sample
 *                          gradients and values of the pending points) and its device log come back filled as well
 *   fault_shard   0..2     ONE-SHOT fault injection into the next hbo_objective_sharded call of this context (tests of the failure
 *                          paths): 1 = the rank's local part counts as failed -> it joins the all-reduce with NaN in every slot;
 *                          2 = and it cannot produce that buffer either -> ncclCommAbort, the peers' all-reduce fails, later sharded
 *                          calls return HBO_ERR_COMM until hbo_comm_init
 *   gram_mfma     0..4096  per context: fp32 Gram matrices of the stationary covariances with at least this many features take gram_mfma_kernel
 *                          (u = |a|^2 + |b|^2 - 2 a.b with a = (x - x_c) / l centred on a row of the tile, the dot product from exact
 *                          three-way bf16 splits on the matrix cores; tiles where that may be off by more than 1e-6 sv are computed again
 *                          in the direct form by gram_mfma_redo_kernel; default 32; 0 = always the direct form sum (a - b)^2;
 *                          profiles/r06_gram_mfma.md)
 *   batch_bg      -1..2    batches: the sweep's launches beside the chain as plain grids (0), persistent over tiles x tasks
 *                          from one counter (1), and also polling the per-CU yield table the chain's kernels then fill (2);
 *                          -1 (default): 1 up to 8 tasks, 0 above (8 tasks 2.52 -> 2.44 ms, 64 tasks 14.13 / 14.31)
 *   spd_diag_bound 0/1     TEST HOOK (tests/test_gpu_split_products.py): with 1, hbo_spd_solve takes max_i A_ii from the host matrix it was given
 *                          and holds it as the factorisation's diagonal bound for the call, so that an fp32 solve of a caller-chosen matrix
 *                          takes the f16x2 form exactly as hbo_factor does (chol_f16x2); default 0: hbo_spd_solve stays on bf16x3.
 *                          hbo_probe_factor_inverse (below) reads it the same way, over all matrices of its batch
 *
 * Read-only, through hbo_get_option:
 *   chol_form              form of the trailing updates of the context's last factorisation: 0 fp32 MFMA (and all of fp64), 1 bf16x3,
 *                          2 f16x2 (the profile's stage names are the same for all three)
 *   inv_forms              what ran on the 16-bit matrix cores since that factorisation, as bits: 1 / 2 a level of the inverse on bf16x3 /
 *                          f16x2 (syrk3_kernel modes 1 and 2), 4 / 8 K^-1 = W^T W on bf16x3 / f16x2 (mode 3); 0: all on fp32 / fp64 MFMA
 *   post_resident          (documented in hbo.h) 1: the last posterior product ran as a resident grid */
#ifndef HBO_TUNE_H_
#define HBO_TUNE_H_
#include "hbo.h"
#ifdef __cplusplus
extern "C" {
#endif
int hbo_tune(hbo_ctx* ctx, const char* name, int64_t value);
/* sustained fp64 MFMA rate of the device, measured now by ~ms milliseconds of back-to-back v_mfma_f64_16x16x4_f64 on every SIMD
 * (TFLOP/s): the roofline denominator bench.py reports beside the datasheet figure */
int hbo_mfma_peak_probe(hbo_ctx* ctx, double ms, double* tflops_out);
/* TEST HOOK: the fp32 posterior product V = W Kxq on the 16-bit matrix cores (form 0: bf16x3, 1: f16x2) on caller-chosen operands.
 * W [n, n] row-major, lower triangular (zeros above the diagonal); Kxq [n, M]; k_bound (f16x2): a bound on |Kxq|, the role the signal
 * variance plays in hbo_predict.  Both are padded as a cache pads them and go through the launches hbo_predict runs for an fp32 cache
 * (split of W, transposed split of Kxq, product), one chunk of all M candidates; use_counter = 1 hands the product a zeroed tile
 * counter as hbo_predict does (a resident grid once there are more than 4 tiles per CU).  colsq_out [ceil(n / 128), M]:
 * colsq_out[i, j] = sum over the rows r of 128-row block i of V[r, j]^2.  HBO_ERR_ARG on a bad argument, before any device call. */
int hbo_probe_post_product(hbo_ctx* ctx, int form, const float* W, int64_t n, const float* Kxq, int64_t M, double k_bound,
                           int use_counter, float* colsq_out);
/* TEST HOOK: the control code of hbo_train_lbfgs (csrc/lbfgs_ctl.h, the text its control kernel compiles) on the host, one thread,
 * for one evaluation; no context, no device.  `value` and `grad` [P] (raw space) belong to the point the state wants evaluated: x0 for
 * an all-zero state (x0 is then required), the x_next of the previous call otherwise.  x_next [P]: the point to evaluate next;
 * x_iter (nullable) [P]: the iterate lbfgs() would return now; *eval: the log entry of this evaluation; *status: hbo_lbfgs_status.
 * HBO_ERR_ARG (hbo_last_error(NULL)) on a bad argument. */
int hbo_probe_lbfgs_ctl(double* state, int32_t P, const hbo_lbfgs_opts* opts, const double* x0, double value, const double* grad,
                        double* x_next, double* x_iter, hbo_lbfgs_eval* eval, int32_t* status);
/* TEST HOOK: hbo_acq_grad_samples (same arguments, same launch, same results) that also returns val64_out [S, M]: the acquisition
 * values before they are rounded to the model dtype -- what the control kernel of hbo_acq_maximize reads.  For an fp64 model
 * val64_out equals acq_out to the bit. */
int hbo_probe_acq_grad_samples64(hbo_ctx* ctx, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq, int64_t M,
                                 int acq_id, const double* params, const double* add_noise, double scale, void* acq_out, double* grad_out,
                                 double* val64_out);
/* TEST HOOK: hbo_acq_grad_samples_blocked (same checks, same launches, same results) that also returns val64_out [S, M], the fp64
 * values the control kernel of hbo_acq_maximize_blocked reads.  force_blocked != 0 sends a call whose caches all have n <= 128 through
 * the blocked kernels of csrc/acq_blocked.hip too (without it such a call is hbo_acq_grad_samples' one launch); chunk_queries > 0
 * overrides the number of queries per pass (0: the entry point's own choice; < 0: HBO_ERR_ARG).  Neither changes a bit of a row that
 * the blocked kernels computed: every sum runs in an order fixed by the cache's n and input_dim alone, without atomics. */
int hbo_probe_acq_grad_samples_blocked64(hbo_ctx* ctx, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq,
                                         int64_t M, int acq_id, const double* params, const double* add_noise, double scale, void* acq_out,
                                         double* grad_out, int32_t force_blocked, int64_t chunk_queries, double* val64_out);
/* TEST HOOK: hbo_acq_grad_samples_mlp (same checks, same launches, same results) with the three extras of the hook above, same meaning:
 * val64_out [S, M], the fp64 values the control kernel of hbo_acq_maximize_mlp reads; force_blocked != 0, the five launches of the
 * blocked route (forward pass, then the four) for caches of n <= 128 too; chunk_queries > 0, the queries per pass (< 0: HBO_ERR_ARG).
 * Neither changes a bit of a row that the blocked kernels computed.  Refusals: those of hbo_acq_grad_samples_mlp. */
int hbo_probe_acq_grad_samples_mlp64(hbo_ctx* ctx, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq,
                                     int64_t M, int acq_id, const double* params, const double* add_noise, double scale, void* acq_out,
                                     double* grad_out, int32_t force_blocked, int64_t chunk_queries, double* val64_out);
/* TEST HOOK: hbo_mes_grad_samples (same checks, same launches, same results) with the three extras of the hook above: val64_out [S, M],
 * the fp64 values the control kernel of hbo_mes_maximize reads; force_blocked, the blocked kernels for caches of n <= 128 too;
 * chunk_queries.  Neither changes a bit of a row that the blocked kernels computed: every sum runs in a fixed order, without atomics. */
int hbo_probe_mes_grad_samples64(hbo_ctx* ctx, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq, int64_t M,
                                 const double* ystar, int32_t K, const double* add_noise, double scale, void* acq_out, double* grad_out,
                                 int32_t force_blocked, int64_t chunk_queries, double* val64_out);
/* TEST HOOK: hbo_logei_grad_samples (same checks, same launches, same results) with the same three extras: val64_out [S, M], the fp64
 * values the control kernel of hbo_logei_maximize reads; force_blocked; chunk_queries. */
int hbo_probe_logei_grad_samples64(hbo_ctx* ctx, const hbo_model* models, int32_t S, hbo_cache* const* caches, const void* xq, int64_t M,
                                   const double* targets, const double* add_noise, double scale, void* acq_out, double* grad_out,
                                   int32_t force_blocked, int64_t chunk_queries, double* val64_out);
/* TEST HOOK: the control code of hbo_acq_maximize (csrc/acq_opt_ctl.h, the text its control kernel compiles) on the host, one thread,
 * for one evaluation of one start; no context, no device.  D: input_dim; dtype: the model dtype the pending point is rounded to.
 * lo, hi [D] (both null: 0 and 1).  vals [S] and grads [S, D]: the per-sample acquisition values (fp64) and gradients at the point the
 * state wants evaluated: x0 [D] (doubles) for an all-zero state (x0 is then required), the x_next of the previous call otherwise.
 * x_next [D]: the point to evaluate next; x_iter (nullable) [D]: the iterate; *eval: the log record; *status: hbo_acq_opt_status.
 * HBO_ERR_ARG (hbo_last_error(NULL)) on a bad argument. */
int hbo_probe_acq_opt_ctl(double* state, int32_t D, int dtype, const hbo_acq_opt_opts* opts, const double* lo, const double* hi,
                          const double* x0, const double* vals, const double* grads, int32_t S, double* x_next, double* x_iter,
                          hbo_acq_opt_eval* eval, int32_t* status);
/* TEST HOOK (tests/test_gpu_gram.py): the Gram launch in the two forms hbo_gram does not take, on host arrays, with every element of
 * the device output preset to `sentinel` (rounded to the model dtype) so that what the kernels do not write shows.  models [n_models]:
 * no MLP basis, no linear_mlp mean, no input warp, one family.  x: the rows of the T tasks one after the other, [sum ns, input_dim];
 * ns [T], 1 <= ns[k] <= 4096, T <= 64.  The WHOLE padded buffers come back in `out` (capacity out_cap elements), task after task in the
 * caller's order, task k as rows_out[k] rows of ld_out[k] elements.
 *   form 1  the posterior's padded cross Gram (cache.hip: produce_chunk): T = 1, n_models = 1, K(x, x2) with x2 [n2, input_dim];
 *           symmetric = 0, padded = 1, extents rounded to 128 and the leading dimension of a posterior chunk, grid (n2pad / 128, nblk);
 *           direct_form as the streamed posterior sets it (1: the fp32 VALU kernel whatever gram_mfma says).  n2 must fit one chunk.
 *   form 2  the batched symmetric task form of the objectives and hbo_factor: a dataset of the T tasks, its workspaces and descriptors
 *           from the set-up of an NLL evaluation, grid (max_nblk, max_nblk, T); n_models = 1: one model for the batch (model_stride 0),
 *           n_models = T: models[k] for task k (model_stride 1).  x2 = NULL, n2 = 0, direct_form = 0.  A comes back without its
 *           augmented tile row: rows_out[k] = npad.
 * gram_mfma is the context's.  HBO_ERR_ARG (hbo_last_error) on a bad argument, before any device call except an out_cap that turns
 * out too small; no product path calls this. */
int hbo_probe_gram(hbo_ctx* ctx, int form, const hbo_model* models, int32_t n_models, const void* x, const int64_t* ns, int32_t T,
                   const void* x2, int64_t n2, int direct_form, double sentinel, void* out, int64_t out_cap, int64_t* rows_out,
                   int64_t* ld_out);
/* What hbo_probe_factor_inverse planned (csrc/sched.h: PotrfPlan, InvPlan), so that a test can tell which route it reached.
 * Factorisation: la look-ahead, q / q_inner panels per trailing update / per inner group (0: one level), early_at / tgran when the
 * early inverse gets its work (after panel early_at, -1: never; after every tgran-th panel), split_f1, yield (0 none, 1 potf2, 2 the
 * chain's wide kernels too).  Inverse: sweep and its row group qs (0: no sweep), early (block-recursive inverse started beside the
 * chain), small_shape (64-tiles throughout), batch_bg (0 plain grids, 1 persistent, 2 and polling the yield table), d_own_stream (the
 * sweep's K^-1 updates on the third stream). */
typedef struct hbo_probe_plan {
  int32_t la, q, q_inner, early_at, tgran, split_f1, yield;
  int32_t sweep, qs, early, small_shape, batch_bg, d_own_stream;
} hbo_probe_plan;
/* TEST HOOK (tests/test_gpu_inverse.py): the factor and inverse steps of an NLL evaluation with gradient on caller-chosen SPD matrices
 * instead of a Gram.  T tasks (1 <= T <= 64), task k of ns[k] points (1 <= ns[k] <= 4096); a: the tasks' matrices [ns[k], ns[k]]
 * row-major one after the other (only the lower triangles are read), b (nullable): their right-hand sides [ns[k], m] one after the
 * other, 1 <= m <= 8 (m = 0 without b).  The batch is built as hbo_probe_gram form 2 builds it (dataset, workspaces, descriptors),
 * poisoned first where the option says so, then the steps run as the objective runs them: the InvRun of
 * inv_plan(T, max_nblk, W and K^-1, beside_chain), run_potrf with it, the rest of the sweep or of the recursive inverse, W^T z for
 * the m columns behind W on the stream the objective uses, K^-1 = W^T W unless the plan sweeps.  The hook decides nothing itself;
 * beside_chain = 0 is the plan of hbo_spd_solve.  With option spd_diag_bound the largest max_i A_ii of the batch is the
 * factorisation's diagonal bound (fp32: the f16x2 form), as for hbo_spd_solve.
 * Outputs, each nullable, dense, task after task in the caller's order:
 *   chol_out [n, n]  L; zeros above the diagonal (written by the export)
 *   w_out    [n, n]  W = L^-1 as it stands in the task's W buffer, the part above the diagonal included (zeros: an invariant the
 *                    products rely on)
 *   kinv_out [n, n]  K^-1 as it stands in S: valid on and below the 128-tile diagonal (whole diagonal tiles); tiles above it are
 *                    scratch (the sweep's running matrix lived there)
 *   z_out    [n, m]  L^-1 b (the augmented rows after the factorisation), x_out [n, m] = A^-1 b = W^T z; both need b
 *   info_out [T]     0 for a task that factorised, else the 1-based row of its first non-positive pivot
 *   plan_out         what was planned (filled before the factorisation is queued: also there when a task turns out not PD)
 * HBO_ERR_ARG on a bad argument, before any device call and with no output touched; HBO_NOT_PD when a task did not factorise: the
 * outputs of those tasks (and only those) are NaN.  No product path calls this. */
int hbo_probe_factor_inverse(hbo_ctx* ctx, int dtype, int32_t T, const int64_t* ns, const void* a, const void* b, int32_t m,
                             int beside_chain, void* chol_out, void* w_out, void* kinv_out, void* x_out, void* z_out, int32_t* info_out,
                             hbo_probe_plan* plan_out);
/* TEST HOOK (tests/test_gpu_kumar_leaves.py): the element-wise kernels of the Kumaraswamy input warp (csrc/kumar.hip) on caller-chosen
 * rows.  model: an hbo_model_kumar (input_warp = HBO_WARP_KUMAR); x [n, input_dim] in the model dtype, 1 <= n <= 2^20.  Two launches, the
 * shipped ones: the forward pass in its gradient form -- w_out [n, input_dim] (model dtype) = w(x), dwda_out / dwdb_out [n, input_dim]
 * (fp64) = dw/da, dw/db at the warped a, b -- and the query-side chain rule on a cotangent of ones: dwdx_out [n, input_dim] (fp64) = dw/dx.
 * HBO_ERR_ARG on a null pointer, a model without the warp or n out of range, before any device call; no product path calls this. */
int hbo_probe_kumar_warp(hbo_ctx* ctx, const hbo_model* model, const void* x, int64_t n, void* w_out, double* dwda_out, double* dwdb_out,
                         double* dwdx_out);
/* TEST HOOK (tests/test_gpu_grad_contract.py): the blocked gradient contraction sum_ij G_ij dK_ij / dtheta (csrc/grad.hip) on a
 * caller-chosen G.  T tasks (1 <= T <= 64), task k of ns[k] points (1 <= ns[k] <= 4096), one model (no input warp; a linear_mlp mean only
 * with an MLP kernel, an MLP kernel not with a linear mean); obj: 0 NLL, 1 EKL, 2 EUC.  All arrays hold the tasks one after the other in
 * the caller's order, in the model dtype unless said:
 *   x       [n, fdim]  the kernel's features: the inputs, or for an MLP kernel the MLP OUTPUT F itself (fdim = the last layer's width;
 *                      the weights of the model are validated but never read: no MLP pass runs)
 *   s       [n, n]     dense symmetric, where K^-1 stands (G = lh s - c sum_b v_b v_b^T); ignored for EUC (G = K1 - sum_b v_b v_b^T), may be
 *                      NULL then
 *   vecs    [nvec, n]  the outer-product vectors; nvec = 1 for NLL, 1..9 otherwise
 *   coef_lh, coef_c [T] doubles, the task's lh and c (what fill_desc derives from the objective otherwise)
 *   dmu     [n] doubles, nullable (zeros): d f / d mu_i, what the mean leaves are summed from
 * The batch is built as hbo_probe_gram form 2 builds it, with the workspaces, descriptors and buffer sizes of an evaluation with gradient
 * (obj_setup, obj_plan), poisoned first where the option says so.  The operands are then written where the inverse and the extra-rows
 * step leave them: s into S on and below the 128-tile diagonal (whole diagonal tiles), the vectors where outer_vecs finds them, dmu.
 * Rows and columns beyond n, and the tiles of S above the tile diagonal, hold `sentinel` (rounded to the model dtype; the tests pass NaN).
 * (EKL with nvec = 1: a task of one target column, whose second vector is zeros over its n elements.)  Then the shipped launches, and only
 * those, in objective.hip's order: launch_grad_contract; launch_grad_finalize with `pre` behind the partials as obj_plan places it (the
 * two-step column sum switches on by the shipped rule); for an MLP kernel launch_grad_feat, and launch_scale_dF for EUC, on a zeroed dF.
 * The hook decides nothing itself.  Outputs, each nullable, doubles, task after task in the caller's order:
 *   grad_out       [T, out_stride]  the finalised block, out_stride = (dot product: 0, else n_lengthscale) + 6 + the mean's feature count:
 *                                   [lengthscale] [signal_variance] [noise_variance] [constant] [dot_prod_sigma] [dot_prod_bias]
 *                                   [linear_kernel] [linear_bias]
 *   partials_out   per task [nblk (nblk + 1), nacc], nblk = ceil(n / 128): the raw slots of the 64 x 128 half tiles, slot
 *                  (ti (ti + 1) / 2 + tj) 2 + h for rows 128 ti + 64 h ..., columns 128 tj ...; nacc = 4 (dot product) or fdim + 3:
 *                  [sum G k] [tr G] [dot: sum G | else fdim of sum G dk/du (ds_d)^2] [sum G0 G, the Frobenius slot (EKL, EUC)]
 *   fro_out        [T]  EUC: |C0 - K1|_F as grad_finalize_kernel leaves it in fnorm[0]
 *   dF_out         [n, fdim]  MLP kernel: d f / d F (EUC: rescaled by 1 / |C0 - K1|_F)
 *   prereduced_out 1 when grad_prereduce_kernel ran (read off `pre`, which is preset to NaN as the partials and the gradient block are)
 * HBO_ERR_ARG on a bad argument, before any device call and with no output touched; no product path calls this. */
int hbo_probe_grad_contract(hbo_ctx* ctx, const hbo_model* model, int obj, int32_t T, const int64_t* ns, const void* x, const void* s,
                            const void* vecs, int32_t nvec, const double* coef_lh, const double* coef_c, const double* dmu, double sentinel,
                            double* grad_out, double* partials_out, double* fro_out, double* dF_out, int32_t* prereduced_out);
/* What hbo_probe_posterior ran (csrc/api_internal.h: PostPlan, after the workspaces were acquired), so that a test can tell which route
 * it reached.  form: the product's form, 0 fp32 MFMA (and all of fp64: GEMM_POST), 1 bf16x3, 2 f16x2; kchunk / nch: the split-K
 * product's 128-blocks per K chunk (0: not split) and the chunks of the longest row tile; nchunks / nbuf: query chunks and alternating
 * workspaces; resident_chunks: chunks whose product ran as a resident grid drawing its tiles from a counter; direct_form: what the
 * streamed producer's cross Gram would be told (1 exactly when nbuf = 2). */
typedef struct hbo_probe_post_plan {
  int32_t form, kchunk, nch, nchunks, nbuf, resident_chunks, direct_form;
} hbo_probe_post_plan;
/* TEST HOOK (tests/test_gpu_posterior.py): the streamed posterior of hbo_predict / hbo_acq (no full_cov) on caller-chosen operands.  All
 * arrays are host arrays in `dtype` (HBO_F32 / HBO_F64), row-major: W [n, n] lower triangular with zeros above the diagonal (checked),
 * where a cache holds L^-1; alpha [n], where it holds K^-1 (y - mu); Kxq [n, M], the cross Gram; kdiag [M], k(x_q, x_q); mu0 [M], the prior
 * mean.  1 <= n <= 4096, 1 <= M <= 2^17.  k_bound > 0: a stationary covariance with that signal variance, |Kxq| <= k_bound (fp32: the
 * f16x2 product is allowed and scales Kxq by it); k_bound = 0: an unbounded covariance, treated as the dot product (fp32: bf16x3 at most).
 * The hook builds a cache-shaped object with the helpers hbo_factor uses (shape, workspaces, descriptor; W and alpha uploaded padded
 * with zeros) and runs the posterior's own code over it: the plan from the context's options (post_chunk, post_bf16x3, post_f16x2,
 * lauum_persist) and the CU count, the workspaces, the split of W, per chunk the product (GEMM_POST plain, resident or split along K with
 * post_colsq_split_kernel; post3_kernel / post2h_kernel), post_mupart_kernel and post_epilogue_kernel, the two alternating workspaces and
 * the events between the two streams.  ONE step is swapped: where the producer would compute the features, the prior mean and variance
 * and the padded cross Gram of queries [q0, q0 + mc), it copies those columns of Kxq, kdiag and mu0 into the chunk's slices, on the
 * producer stream, the padding zero as the padded Gram leaves it; the transposed split of Kxq for the 16-bit forms stays.  The hook
 * decides nothing itself.
 * Outputs: mu_out, var_out [M]; colsq_out, mupart_out [ceil(n / 128), M] (nullable): per 128-row block i the column sums of V^2 and of
 * Kxq[i-block] * alpha as the epilogue read them -- single-chunk calls only (M <= post_chunk), HBO_ERR_ARG otherwise; plan_out
 * (nullable): what ran.  HBO_ERR_ARG on a bad argument, before any device call and with no output touched; no product path calls this. */
int hbo_probe_posterior(hbo_ctx* ctx, int dtype, const void* W, int64_t n, const void* alpha, const void* Kxq, const void* kdiag,
                        const void* mu0, int64_t M, double k_bound, void* mu_out, void* var_out, void* colsq_out, void* mupart_out,
                        hbo_probe_post_plan* plan_out);
#ifdef __cplusplus
}
#endif
#endif /* HBO_TUNE_H_ */
