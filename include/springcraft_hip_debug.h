/*
 * springcraft_hip_debug.h -- tuning / diagnostic entry points of libspringcraft_hip.so.
 *
 * NOT part of the drop-in boundary (that is springcraft_hip.h): nothing in the product path calls these; they exist for
 * the scripts under tools/ and may change between rounds.  They are exported from the same library so that the kernels
 * they exercise are exactly the ones the product launches.
 */
#ifndef SPRINGCRAFT_HIP_DEBUG_H
#define SPRINGCRAFT_HIP_DEBUG_H

#include "springcraft_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Times `iters` launches of one grouped-GEMM shape on buffers it allocates itself and checks the result against a host
 * product (max abs error).  mode 0: C = A B (A m x k, B k x n, column-major); 1: lower triangle of C += A B^T (the
 * SYR2K shape, B stored n x k); 2: C = A^T B (A stored k x m).  tile 10..13: the k_gemm2 tilings (automatic,
 * 128x128, 128x64, 64x64).  Returns an SC_* code.  tools/gemm2_bench.py */
int sc_dbg_gemm_bench(sc_ctx* ctx, int m, int n, int k, int mode, int tile, int split_k, int iters, int beta_one,
                      double* ms_out, double* max_err_out);

/* ONE launch of one GEMM record on host data (a, b laid out as in sc_dbg_gemm_bench for `mode`; c: m x n column-major,
 * in / out; with split_k > 1 the K slices are summed into c on the host and beta must be 0; lower_grid as the launcher
 * takes it).  alpha == 0 with beta != 0 is SC_ERR_INVALID_ARG: the kernel does not take such a record.  The GPU unit
 * tests of the launch paths compare the result with NumPy.  tests/test_gemm_gpu.py */
int sc_dbg_gemm_host(sc_ctx* ctx, const double* a, const double* b, double* c, int m, int n, int k, int mode, int tile,
                     int split_k, double alpha, double beta, int lower_grid);

/* One record of a grouped GEMM launch as the host describes it: the kernel's record (GemmDesc, csrc/gemm_f64.h) with
 * element offsets in place of pointers -- a, b, c into an arena of doubles, a_kidx, b_kidx, c_jidx into an arena of ints
 * (-1: no list).  Every other field is handed to the kernel unchanged.  144 bytes, no padding. */
typedef struct sc_dbg_gemm_record {
  long long a, b, c;
  long long a_kidx, b_kidx, c_jidx;
  long long sa_i, sa_k, sb_k, sb_j, ldc, split_stride;
  double alpha, beta;
  int m, n, k;
  int lower_only, row_off, col_off;
  int a_tri;
  int reserved;
} sc_dbg_gemm_record;

/* ONE grouped launch (launch_gemm_f64) of `count` records on host data: triangular operands, gather lists, several
 * records of different sizes, sub-matrix views, record lists longer than one grid.  arena (arena_len doubles, in / out)
 * is copied whole to the device and whole back; idx (idx_len ints) holds the index lists.  count, max_m, max_n, split_k,
 * gather, tri, layout (0 = A m-contiguous / B k-contiguous, 1 = both k-contiguous, 2 = A m-contiguous / B n-contiguous)
 * and lower_grid as the launcher takes them; tile 10..13 as sc_dbg_gemm_host (gather launches: 12 = 128 x 64, 13 =
 * 64 x 64, else by size).  With split_k > 1 the K slices stay where the kernel wrote them (c + s * split_stride).
 * SC_ERR_INVALID_ARG, and no launch, when a record could make the kernel touch an address outside its arena (offsets,
 * strides, list entries), when its unit strides do not match the layout, when it carries a_tri or lists the launch does
 * not read, or for alpha == 0 with beta != 0.  The device copy of the arena lies between two guard areas; a launch that
 * changed them is SC_ERR_HIP.  tests/test_gemm_records_gpu.py */
int sc_dbg_gemm_records_host(sc_ctx* ctx, double* arena, long long arena_len, const int* idx, long long idx_len,
                             const sc_dbg_gemm_record* recs, int count, int max_m, int max_n, int split_k, int gather,
                             int tri, int layout, int lower_grid, int tile);

/* `count` products of ONE shape on host data through k_gemm3, the role-split persistent kernel of the short-K updates
 * (csrc/gemm3.hip), whatever their size: a count x (m x k) column-major; b count x (k x n) column-major (layout 0,
 * kGemmAmBk) or count x (n x k) column-major (layout 2, kGemmAmBn); c count x (m x n) column-major, in / out; C = beta C
 * + A B with beta 0 or 1; lower: only entries on / below the diagonal are written (m == n).  Returns
 * SC_ERR_INVALID_ARG for a shape the kernel does not take.  tests/test_gemm_gpu.py */
int sc_dbg_gemm3_host(sc_ctx* ctx, const double* a, const double* b, double* c, int count, int m, int n, int k, int layout,
                      int lower, double beta);

/* x = sym(a) v through k_symm3 (csrc/symm3.hip), the band reduction's symmetric product as one role-split launch:
 * `count` matrices a (m x m, column-major; read where (row | 1) >= col), v and x count x (m x 64) column-major, `split`
 * K slices (summed on the host).  m a multiple of 16.  tests/test_gemm_gpu.py */
int sc_dbg_symm3_host(sc_ctx* ctx, const double* a, const double* v, double* x, int count, int m, int split);
/* Library built with -DSYMM3_STAMPS (else returns 1): out4 = shader cycles the first loader wave of every k_symm3 workgroup
 * spent {waiting for its LDS-DMA group to land, at the step barriers, in its loop}, and the steps it waited in; reset by
 * the call.  tools/r06_symm3_stamps.sh */
int sc_dbg_symm3_stamps(unsigned long long* out4);
/* `count` random matrices of order m (even, >= 256), X = A V through k_symm3 with `split` K slices, `iters` timed launches:
 * average milliseconds per launch.  tools/symm3_bench.py */
int sc_dbg_symm3_bench(sc_ctx* ctx, int count, int m, int split, int iters, double* ms_out);

/* `count` matrices of one shape on freshly allocated buffers, C += A B (lower != 0: the lower triangle, m == n), timed
 * through k_gemm3 (kernel 3; order 0 / 1: its flat / per-XCD super-tile order) or through k_gemm2 (kernel 2) with the same
 * records: ms_out = milliseconds per launch.  tools/gemm3_shapes.py */
int sc_dbg_gemm3_bench(sc_ctx* ctx, int count, int m, int n, int k, int layout, int lower, int kernel, int order, int iters,
                       double* ms_out);

/* s_memtime segment sums of k_gemm2 (library built with -DGEMM_STAMPS; returns 1 otherwise): out4[0..2] =
 * shader cycles summed over waves in the prologue, the K loop and the C epilogue, out4[3] = waves counted; `reset`
 * zeroes the sums after the read.  tools/gemm_stamps.py */
int sc_dbg_gemm_stamps(unsigned long long* out4, int reset);

/* Per-workgroup timeline of k_gemm2 (same diagnostic build): up to `max_records` records of 6 values
 * {hw id (XCC_ID << 32 | HW_ID), t_start, t_loop, t_epilogue, t_end, blockIdx linear} of the workgroups launched since
 * the last reset; returns the number of records written through *count.  tools/gemm_trace.py */
int sc_dbg_gemm_trace(unsigned long long* out, int max_records, int* count, int reset);

/* The stages of a solve on host data (csrc/eigh_debug.hip), on the drivers' own plan and reduction step (csrc/eigh_plan.h).
 *
 * The reduction stage of a full-spectrum solve on host data, with its factors: `batch` matrices a (batch x n x n, NumPy
 * layout, lower triangle read) go through the scaling pass and the tridiagonalisation the product would choose for (ctx, n,
 * batch) -- the plan of sc_dev_eigh_f64 (csrc/eigh_policy.h:two_stage_for), with sc_ctx_set_two_stage, sc_dbg_set_chase,
 * sc_dbg_set_panel_coop[_fail] and sc_dbg_set_resident honoured -- and the product's back-transformation is applied to
 * Z = I.  No kernel of its own.
 *   d_out, e_out   batch x n each: the tridiagonal T (e[n - 1] = 0)
 *   scale_out      null, or batch: the power of two s the matrix was multiplied by, so that  s A = Q T Q^T
 *   band_out       null, or batch x (128 x n), two-stage path only: the band B after stage 1, B(i, j) at [(i - j) + 128 j]
 *                  for 0 <= i - j <= 64 (the rows beyond 64 are zero); untouched on the one-stage path
 *   q_out          null (no back-transformation), or batch x n x n: the orthogonal factor `which`, its COLUMNS as the rows
 *                  of the NumPy array (the layout of the eigenvectors of sc_eigh_f64: q_out[k] = Q e_k):
 *                  which 0: Q = Q1 Q2 (bt2_prepare + bt2_batched, then backtransform_batched; one-stage: its only factor),
 *                        1: Q1, the stage-1 reflectors alone (backtransform_batched, off = 64),  s A = Q1 B Q1^T,
 *                        2: Q2, the stage-2 reflectors alone (k_bt2_apply),  B = Q2 T Q2^T;
 *                  1 and 2 on the one-stage path are SC_ERR_INVALID_ARG
 *   two_stage_out  null, or the path taken (1 two-stage, 0 one-stage)
 * SC_ERR_INVALID_ARG for n < 256 on a context whose two-stage path is forced on.  The call synchronises.
 * tests/test_stage_ratios_gpu.py, tools/check_two_stage.py */
int sc_dbg_reduce_host(sc_ctx* ctx, const double* a, int n, int batch, int which, double* d_out, double* e_out,
                       double* scale_out, double* band_out, double* q_out, int* two_stage_out);

/* stedc_batched, the tridiagonal divide & conquer of the full-spectrum solve, on `batch` tridiagonal matrices from the
 * host: d, e batch x n each (e[n - 1] is not read; the layout sc_dbg_reduce_host returns).  w_out batch x n ascending;
 * z_out batch x n x n, row k of the NumPy array = the eigenvector of w[k].  The call synchronises; a QL failure is
 * SC_ERR_NOCONV.  tests/test_stage_ratios_gpu.py */
int sc_dbg_stedc_host(sc_ctx* ctx, const double* d, const double* e, int n, int batch, double* w_out, double* z_out);
/* Rows of the largest leaf the D&C solves by QL at order n (kLeafMax of stedc_plan.h, the same at every order). */
int sc_dbg_stedc_leaf_max(int n);

/* The partial-spectrum stage (csrc/stein.hip) on `batch` tridiagonal matrices from the host, through the product's host
 * functions: window_count_batched (window only), stein_batched, window_compact_batched (window only).  No kernel of its
 * own, and no unscale_values_batched: the eigenvalues are those of the T that was given.
 *   d, e           batch x n each (e[n - 1] is not read; the layout sc_dbg_reduce_host returns)
 *   f              null (1.0), or batch: the power-of-two factor k_window_count multiplies the bounds by (TL.hscale + 2)
 *   own            null, or batch: the own order of every matrix as a ragged window solve passes it (window only)
 *   window == 0    eigenpairs il .. il + m - 1 (0-based) of every matrix; vl, vu are not read
 *   window != 0    the window (vl, vu] into slots of K = m eigenpairs; il is not read
 *   vectors == 0   values only (stein_batched's d_x = nullptr return); z_out is not written
 *   w_out          batch x m; z_out batch x m x n, row k = the eigenvector of w[k] (the layout of sc_eigh_f64)
 *   win_out        null, or batch x 4 ints: the WinCount records {il, count, start, 0} (window only)
 *   count_out      null, or batch: the window's true counts (window only)
 * SC_ERR_INVALID_ARG, and no launch, for a null required pointer, n outside 1..46000, batch < 1, a range outside
 * 0 <= il, il + m <= n, m >= 1, a capacity outside 1..n, !(vl < vu), or own[b] outside K..n.  The call synchronises and
 * returns the deferred status.  tests/test_partial_ratios_gpu.py */
int sc_dbg_partial_tridiag_host(sc_ctx* ctx, const double* d, const double* e, const double* f, const int* own, int n,
                                int batch, int window, int il, int m, double vl, double vu, int vectors, double* w_out,
                                double* z_out, int* win_out, long long* count_out);

/* Per-wave s_memtime segment sums of k_bt2_apply (library built with -DBT2_STAMPS; returns 1 otherwise):
 * out[64 workgroups][8 waves][16 sums + diamond count].  tools/bt2_stamps.py */
int sc_dbg_bt2_stamps(unsigned long long* out);

/* Shader clock while the most recent k_bt2_apply launch ran (library built with -DBT2_CLOCK; returns 1
 * otherwise): out2 = {shader cycles (s_memtime), 100 MHz ticks (s_memrealtime)} over the life of wave 0 of workgroup 0.
 * tools/bt2_clock.py */
int sc_dbg_bt2_clock(unsigned long long* out2);

/* s_memtime in front of every MFMA of one diamond of k_bt2_apply (library built with -DBT2_TRACE; returns 1 otherwise):
 * out[8 waves][2 halves][81].  tools/bt2_trace.py */
int sc_dbg_bt2_trace(unsigned long long* out);

/* s_memtime sums of k_bulge_step over all tasks since the last call (library built with -DBULGE_STAMPS; returns 1
 * otherwise): out6 = {cycles from task start until the off-diagonal block E is in LDS, until E is stored [both: tasks
 * with k > 0], until the diagonal block D is in LDS, until the end; tasks; tasks with k > 0}.  tools/bulge_stamps.py */
int sc_dbg_bulge_stamps(unsigned long long* out6);
/* The same for the pair form of the persistent chase (k_bulge_pair; library built with -DPAIR_STAMPS, else returns 1):
 * 48 entries.  [0..15] thread 0 (team A): [0..6] = cycles between the barriers of a common step (wait + [0], block reads +
 * [1], E right update + reflector, column sums + D image, E left update + D products, w, D update), [8] = steps, [9] =
 * common steps, [12] = block reads alone; [16..31] thread 256 (team B), same layout, [23] its look at the predecessor pair, [30] steps in which it polled, [26] slot reads, [27] store drain,
 * [29] D update + stores; [32..47] unused (zero). */
int sc_dbg_pair_stamps(unsigned long long* out48);
/* The same for the persistent chase with one sweep per workgroup (k_bulge_chase; library built with -DCHASE_STAMPS, else
 * returns 1): out16[1..11] = cycles of all waves between eleven points of a task, summed over all tasks since the last call
 * (the segments are listed at the macro in sb2st.hip), [15] = waves x tasks.  tools/chase_stamps.py */
int sc_dbg_chase_stamps(unsigned long long* out16);

/* Persistent bulge chase of this context: mode -1 = SPRINGCRAFT_BULGE_PERSISTENT or the size rule (default), 0 never,
 * 1 by size, 2 always (3: always and in the pair form k_bulge_pair, 4: always with one sweep per workgroup,
 * k_bulge_chase, a matrix on one XCD; 5: as 4 with the workgroups of a matrix on all XCDs -- fewer matrices than XCDs only;
 * 2 picks the form by size like the default).  give_up_after > 0: test hook, every workgroup of the chase raises the
 * time-out flag after that many tasks, which forces the take-over on the device (k_chase_finish; counted in
 * "chase_resumed", not in "chase_timeouts").  tests/test_two_stage_gpu.py */
int sc_dbg_set_chase(sc_ctx* ctx, int mode, int give_up_after);

/* Cooperative panel QR of this context (k_panel_coop: several workgroups of one launch own 256 rows of a panel each;
 * stage 1 of the two-stage tridiagonalisation, few matrices): min_rows = panels of at least that many rows take it
 * (>= 128; the default rule: 300 rows with fewer than four matrices, else above the single-workgroup kernels' 6144),
 * 0 = never, -1 = the default rule
 * (SPRINGCRAFT_QR_COOP / SPRINGCRAFT_QR_COOP_MIN).  Counters "panel_coop_launches" / "panel_coop_timeouts".
 * tests/test_two_stage_gpu.py */
int sc_dbg_set_panel_coop(sc_ctx* ctx, int min_rows);
/* Test hook of the cooperative panel kernel's take-over: from panel `panel` on (-1: never) the abort flags of all
 * matrices are raised before the launch, as after a wait that ran into its bound; k_panel_serial then factors that panel
 * and every later one, counted in "panel_coop_timeouts". */
int sc_dbg_set_panel_coop_fail(sc_ctx* ctx, int panel);

/* One-launch tridiagonalisation of ONE matrix whose rows stay in LDS (k_sytrd_resident, tridiag.hip; one-stage path,
 * the trailing matrix of order <= 2048): mode 0 = never, 1 / -1 = the default rule (SPRINGCRAFT_RESIDENT).  hook: tests,
 * 1 = the roll call of its workgroups fails (nothing stored yet: k_sytrd_takeover reduces the matrix), 2 + c = the
 * exchange of step c fails (the take-over restores the matrix from its other triangle and starts again); 0 = none.
 * workgroups: 0 = by size, else a power of two (SPRINGCRAFT_RESIDENT_WGS).  Every call with mode != 0 re-arms a context
 * that had given the kernel up (after a lost wait, or three failed roll calls).  Counters "resident_launches" /
 * "resident_takeovers" / "resident_rollcall_failures" / "resident_lost_waits".  tests/test_resident_gpu.py */
int sc_dbg_set_resident(sc_ctx* ctx, int mode, int hook, int workgroups);
/* Library built with -DRES_STAMPS (else returns 1): cycles workgroup 0 of k_sytrd_resident spent in the segments of a
 * step -- [0] publish + poll of the records, [1] w~.v and the next column, [2] its norm, the next reflector and its
 * stores, [3] the pass over the own rows, [5] the sums of y --, [7] = steps; summed since the last call.
 * tools/resident_check.py --stamps */
int sc_dbg_resident_stamps(unsigned long long* out8);

#ifdef __cplusplus
}
#endif
#endif
