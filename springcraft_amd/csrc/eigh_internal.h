// Internal interfaces between the stages of the batched symmetric eigensolver
//   tridiag.hip (K5)  ->  stedc.hip (K6)  ->  backtransform.hip (K7),  driven by eigh.hip.
#pragma once

#include "common.h"
#include "gemm_f64.h"
#include "stedc_plan.h"
#include "sy2sb_plan.h"

// Per-matrix workspace slab of the tridiagonalisation (offsets in doubles from the slab base).
struct TriLayout {
  int n, nb;
  long long slab;    // slab stride between consecutive matrices of the batch
  long long vw;      // [V|W] panel, n x 2nb, column-major ld n
  long long wv;      // [W|V] panel, n x 2nb
  long long xraw;    // updated column a (n)
  long long ypart;   // SYMV partial products, nt x n
  long long dpart;   // partial dots V^T v / W^T v, nt x 2nb
  long long npart;   // partial squared norms (<= n/256 + 1)
  long long wvpart;  // partial w~^T v
  long long d, e, tau;  // tridiagonal + reflector scalars (n each)
  long long hscale;     // [0] = 1/(alpha - beta) of the current column (written by k_symv_tiles);
                        // [1] = bit pattern of max |a_ij|, [2] = power-of-two factor the matrix was scaled by
  long long rctl;       // k_sytrd_resident: control words (16 ints), directly followed by
  long long rrec;       // its exchange records, 3 buffers x (n rounded up to 64) x 16 bytes
};
// bytes from rctl that a solve sets to 0xFF before k_sytrd_resident (control words "undecided", records "empty")
inline size_t tri_resident_bytes(int n) { return sizeof(double) * (8 + (size_t)6 * ((n + 63) / 64 * 64)); }

// d_a: (batch) n x n column-major, lower triangle valid after the mirror pass; on exit column c holds
// v_c (explicit leading 1) in rows c+1.., and ws holds d, e, tau.
// NumPy (row-major) lower triangle -> column-major lower triangle, in place
int mirror_lower_batched(sc_ctx* ctx, double* d_a, long long stride_a, int n, int batch);
// mirror + scaling of badly scaled matrices (largest |entry| outside [1e-100, 1e100]) by a power of two; the factor
// stays in the tri slab and unscale_values_batched divides the computed eigenvalues by it.  Call before
// tridiag_batched / sytrd_2stage_batched (neither mirrors by itself).
int prepare_matrix_batched(sc_ctx* ctx, double* d_a, long long stride_a, int n, int batch, double* d_tri_ws,
                           const TriLayout& L);
int unscale_values_batched(sc_ctx* ctx, double* d_w, long long stride_w, int m, int batch, const double* d_tri_ws,
                           const TriLayout& L);

int tridiag_batched(sc_ctx* ctx, double* d_a, long long stride_a, int n, int batch, double* d_ws,
                    const TriLayout& L, const GemmDesc* d_syr2k_descs, float* ms_symv, float* ms_syr2k);
// whether tridiag_batched hands the (trailing) matrix of a one-matrix solve to k_sytrd_resident on this context (ctx may
// be null: the environment's answer)
bool resident_enabled(const sc_ctx* ctx);

// ---- divide & conquer (stedc.hip) --------------------------------------------------------------------
// The plan (stedc_plan.h) owns every decision: the merge tree of an order (DcNode, built once per solve inside
// stedc_batched), the launch shapes and LDS bytes of the kernels of a merge level, which ping-pong buffer a level reads
// and writes, and the layout of what the D&C keeps in sc_ctx::dc_aux (the uploaded tree, the profiling word, the sorted
// copies of merges too wide for LDS) -- stedc_batched reserves and fills that buffer itself.  The caller owns the rest
// and sizes it from the two functions below: per matrix a slab of dc_slab_doubles(n) doubles laid out by DcLayout, two
// (batch, n, n) work matrices beside the output, and 2 * dc_max_nodes(n) * batch merge records.
using sc_host::DcNode;

struct DcLayout {
  int n;
  long long slab;    // per-matrix stride (doubles) of the D&C slab
  long long dd, ee;  // scaled copies of d, e (n each)
  long long w0, w1;  // eigenvalue ping-pong (n each)
  long long z;       // rank-one vector (n)
  long long dl, zz;  // non-deflated poles / weights, compacted per node at [lo, lo+K)
  long long ddef;    // deflated eigenvalues per node at [lo, lo+ndef)
  long long lam;     // new roots per node (n)
  long long tauv;    // secular root offsets (n)
  long long zhat;    // Gu-Eisenstat weights (n)
  long long rot_c, rot_s;  // rotation list (n each)
  long long scale;   // [0] = norm used for scaling
  // integer arrays live in the same slab, offsets in doubles (each int array padded to n doubles)
  long long src;     // int[n]: source column of non-deflated k (at lo+k); of deflated e (at lo+K+e)
  long long org;     // int[n]: origin pole of each root
  long long dest;    // int[n]: destination column of non-deflated k (at lo+k) / deflated (at lo+K+e)
  long long rot_a, rot_b;  // int[n] each: rotated column pairs
  long long ktop_src, ktop_k;  // int[n] each: columns that are non-zero in the node's TOP half: source column / pole index
  long long kbot_src, kbot_k;  // same for the BOTTOM half
  long long cnt;     // int[2 * max_nodes]: per node K and number of rotations
};

// Eigen-decomposition of `batch` symmetric tridiagonal matrices (d, e in the TriLayout slab).
// On exit: d_w (batch, n) ascending eigenvalues; eigenvectors (columns) in d_q_out (batch, n, n).
// d_q_tmp / d_u: two more (batch, n, n) work matrices.
int stedc_batched(sc_ctx* ctx, int n, int batch, const double* d_tri_ws, const TriLayout& TL,
                  double* d_dc_ws, const DcLayout& DL, double* d_w, long long stride_w,
                  double* d_q_out, double* d_q_tmp, double* d_u, long long stride_q,
                  GemmDesc* d_merge_descs /* 2 * dc_max_nodes(n) * batch */);
size_t dc_slab_doubles(int n, DcLayout* out);
int dc_max_nodes(int n);   // leaves and merges of the tree of order n

// Eigenvalues only: Sturm-sequence bisection (one thread per eigenvalue).
int sturm_bisect_batched(sc_ctx* ctx, int n, int batch, const double* d_tri_ws, const TriLayout& TL,
                         double* d_w, long long stride_w);

// ---- back-transformation -----------------------------------------------------------------------------
// Z <- Q_H Z with the reflectors stored in d_a (see tridiag_batched) and tau in the tri slab.
// off: row distance of a reflector's unit entry from the diagonal (1: one-stage; 64: stage 1 of the two-stage path).
struct BtLayout {
  int n, nbt, splits;
  long long slab;
  long long vc;     // (unused)
  long long gram;   // per block: split-K slabs of V^T V, splits_g x nbt x nbt
  long long t;      // per block: nbt x nbt triangular factor
  long long g12;    // per block: summed Gram block V1^T V2 (128 x 128)
  long long tx;     // per block: (V1^T V2) T2
  long long w1;     // split-K slabs of V^T Z: splits x nbt x n
  long long w2;     // T * sum(w1): nbt x n
  int splits_g;
};
size_t bt_slab_doubles(int n, BtLayout* out);
int bt_desc_count(int n, int batch);
// d_a is modified (cleaned in place); d_vt: (batch, n, n) scratch that receives V T.
int backtransform_batched(sc_ctx* ctx, double* d_a, long long stride_a, int n, int batch,
                          const double* d_tri_ws, const TriLayout& TL, double* d_bt_ws,
                          const BtLayout& BL, double* d_z, long long stride_z, int ncols, double* d_vt,
                          GemmDesc* d_descs /* bt_desc_count(n, batch) records */, int off = 1, int phase = 0);

// ---- two-stage tridiagonalisation (twostage.hip, sy2sb.hip, sb2st.hip, bt2.hip) -------------------------------
// The slab of a matrix (SbLayout, sb_slab_doubles) and the count of stage 1's GEMM records (stage1_record_count): sy2sb_plan.h
using sc_host::sb_slab_doubles, sc_host::stage1_record_count;
int sb_band_width();
// d_a: column-major lower triangle valid.  On exit d, e (and the stage-1 tau) are in the tri slab, the stage-1
// reflectors in A (unit entry of column c at row c + sb_band_width()), the stage-2 reflectors in the sb slab.
int sytrd_2stage_batched(sc_ctx* ctx, double* d_a, long long stride_a, int n, int batch, double* d_tri_ws,
                         const TriLayout& TL, double* d_sb_ws, const SbLayout& SL, int* d_dia_off /* n/64 + 2 ints */,
                         GemmDesc* d_descs /* stage1_record_count */, float* ms_stage1, float* ms_stage2,
                         double* d_band_copy = nullptr);
// Z <- Q2 Z (stage-2 reflectors): bt2_prepare (T factors; independent of Z, may run on another stream), then bt2_batched
int bt2_prepare(sc_ctx* ctx, int n, int batch, double* d_sb_ws, const SbLayout& SL, hipStream_t st);
int bt2_batched(sc_ctx* ctx, int n, int batch, double* d_sb_ws, const SbLayout& SL, const int* d_dia_off, double* d_z,
                long long stride_z, int ncols, float* ms_fused = nullptr);

// ---- partial spectrum (stein.hip) -----------------------------------------------------------------------
// Eigenvalue window (vl, vu] of one matrix, counted on the device: il = #(lambda <= vl), count = #(lambda <= vu) - il;
// its slot of K eigenpairs holds eigenpairs start .. start + K - 1, start = min(il, n - K)
struct WinCount {
  int il, count, start, pad;
};
size_t stein_workspace_doubles(int n, int m);
// d_win: null (eigenpairs il..iu of every matrix), or the counts of window_count_batched (matrix b: eigenpairs
// d_win[b].start .. d_win[b].start + iu - il)
int stein_batched(sc_ctx* ctx, int n, int batch, const double* d_tri_ws, const TriLayout& TL, int il, int iu,
                  double* d_w, long long stride_w, double* d_x, long long stride_x, double* d_ws,
                  GemmDesc* d_descs /* 2 * batch */, const WinCount* d_win = nullptr);
// d_win[b] (and d_count[b] = count unless null) for every matrix of the tridiagonalised batch; 1 <= K <= n.
// d_own: null, or per matrix the number of leading eigenvalues that are its own (1 <= K <= own <= n): the rest never count
int window_count_batched(sc_ctx* ctx, int batch, const double* d_tri_ws, const TriLayout& TL, double vl, double vu, int K,
                         WinCount* d_win, long long* d_count, const RaggedRec* d_own = nullptr);
// The window's rows of every slot of d_w (batch, K) / d_v (null or (batch, K, n)) to the front, NaN / zero rows behind;
// d_w_copy (batch K) and d_v_copy (batch K n) are scratch
int window_compact_batched(sc_ctx* ctx, int n, int batch, int K, const WinCount* d_win, double* d_w, double* d_v,
                           double* d_w_copy, double* d_v_copy);

// ---- mode consumers (batch_consumers.hip, dist_fluct.hip, mode_response.hip) ----------------------------------------------------------
// d_s (batch, nsel) <- the weight of every (structure, listed row): 1 / lambda for a selected row, exactly 0.0 for one
// that is not (behind a window's count, a ragged slot's pad rows, under the pinv threshold), NaN for a listed row outside
// 0..nvec-1.  nsel = batch_modes_nsel(sel, nvec) > 0.  One launch of k_mode_weights; every consumer reads its rows through it.
int launch_mode_weights(sc_ctx* ctx, const double* d_w, int64_t nvec, int64_t batch, const sc_mode_selection& sel,
                        int64_t nsel, const int64_t* d_counts, double* d_s, const RaggedView* rv);
// Listed rows per chunk of the consumers that sum across rows and add their chunks in a fixed order (msf, tensors,
// mode_response.hip's combine): a function of the number of listed rows alone, so that a structure's bits are the same
// in any batch.
int msf_chunk(int64_t nsel);
#ifdef __HIPCC__
// Tile t of the lower triangle of a square of tiles, rows first: t = ta (ta + 1) / 2 + tc with tc <= ta (dist_fluct.hip,
// mode_prs.hip: every unordered pair of tiles has one workgroup).  The float root is a first guess, the loops make it exact.
__device__ __forceinline__ void tri_tile_decode(int t, int& ta, int& tc) {
  ta = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
  while ((ta + 1) * (ta + 2) / 2 <= t) ++ta;
  while (ta * (ta + 1) / 2 > t) --ta;
  tc = t - ta * (ta + 1) / 2;
}
#endif
