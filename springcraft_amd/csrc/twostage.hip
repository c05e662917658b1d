// Two-stage tridiagonalisation for large matrices (replaces the one-stage panel algorithm of tridiag.hip, whose
// matrix-vector products are bound by HBM bandwidth: 4/3 n^3 bytes per matrix).
//
//   stage 1  sy2sb   dense -> band of half-width kB = 64.  Per 64-column panel: Householder QR of the block below
//                    the band (k_panel_qr, one launch per column, the panel streamed through LDS), then the
//                    two-sided update  A22 <- Q^T A22 Q = A22 - V W^T - W V^T  in which all O(n^2 b) work is f64-MFMA
//                    GEMM: X = A22 V (two triangular-operand GEMMs on the lower-stored A22), V^T [X|V] (Gram, split-K),
//                    W = [X|V] [T; -S/2] and the SYR2K  [V|W] [W|V]^T.
//   stage 2  sb2st   band -> tridiagonal by Householder bulge chasing (Lang's algorithm: sweep s annihilates column s
//                    below the first sub-diagonal and chases the bulge down the band, one reflector of length <= 64
//                    per block).  Task (s, k) only conflicts with (s+1, k-1) and later, so launch t runs every task
//                    with 2 s + k = t, one workgroup each (k_bulge_step): 2 n + n/64 launches, no spin-waits.
//   back-transformation  Z <- Q1 Q2 Z.  Q2: the reflectors of 64 consecutive sweeps at the same chase position form
//                    a "diamond" (127 x 64 parallelogram) = one compact-WY block I - V T V^T; diamonds (S, k) are
//                    applied in wavefronts 3 (Smax - S) + k = const as two grouped GEMMs per wavefront (bt2).
//                    Q1: the stage-1 reflectors through the block back-transformation of backtransform.hip.
//
// Role in the reference: part of np.linalg.eigh (LAPACK dsyevd) at nma.py:61; LAPACK itself uses the one-stage dsytrd.
//
// Files: this one holds the driver of stages 1 and 2; sy2sb.hip stage 1, sb2st.hip stage 2, bt2.hip the Q2
// back-transformation (bt2); twostage_internal.h what they share; twostage_policy.h every choice between kernel forms;
// sy2sb_plan.h the slab layout and what stage 1 launches with (records, LDS, carves).
#include <algorithm>
#include <vector>

#include "twostage_internal.h"

// ================================================================================================================
// Stage 1 + 2 driver.  d_a: lower triangle valid (after mirror_lower_batched).  On exit: tri slab holds d, e and the
// stage-1 tau; A holds the stage-1 reflectors (cleaned for the back-transformation); the sb slab holds the diamonds.
int sytrd_2stage_batched(sc_ctx* ctx, double* d_a, long long stride_a, int n, int batch, double* d_tri_ws,
                         const TriLayout& TL, double* d_sb_ws, const SbLayout& SL, int* d_dia_off,
                         GemmDesc* d_descs, float* ms_stage1, float* ms_stage2, double* d_band_copy) {
  hipStream_t st = ctx->stream;
  ScopedEvents<3> ev;
  const bool prof = ctx->profiling && ms_stage1 && ms_stage2;
  if (prof) {
    for (auto& e : ev) SC_HIP(ctx, hipEventCreate(&e));
    SC_HIP(ctx, hipEventRecord(ev[0], st));
  }

  // ---- descriptors of stage 1 (sy2sb_plan.h); the panels' roles: 0 single, 1 first of a pair, 2 second of a pair
  const sc_host::TwoStageEnv& E = sc_host::two_stage_env();
  const std::vector<int> role = sc_host::panel_roles(E, n);
  const std::vector<GemmDesc> hs = sc_host::stage1_records(n, batch, role, sc_host::symm3_for(E, n), d_a, stride_a, d_sb_ws, SL);
  if (!hs.empty()) SC_TRY(sc_stage_upload(ctx, d_descs, hs.data(), hs.size() * sizeof(GemmDesc)));
  const std::vector<int> doff = dia_offsets(n);
  SC_TRY(sc_stage_upload(ctx, d_dia_off, doff.data(), doff.size() * sizeof(int)));

  SbTimers timers(ctx, st);
  SC_TRY(sb_stage1(ctx, d_a, stride_a, n, batch, d_tri_ws, TL, d_sb_ws, SL, d_descs, role, prof, timers));
  if (prof) SC_HIP(ctx, hipEventRecord(ev[1], st));
  SC_TRY(sb_stage2(ctx, d_a, stride_a, n, batch, d_tri_ws, TL, d_sb_ws, SL, d_band_copy, timers));
  if (prof) {
    SC_HIP(ctx, hipEventRecord(ev[2], st));
    SC_HIP(ctx, hipEventSynchronize(ev[2]));
    SC_HIP(ctx, hipEventElapsedTime(ms_stage1, ev[0], ev[1]));
    SC_HIP(ctx, hipEventElapsedTime(ms_stage2, ev[1], ev[2]));
  }
  timers.finish();
  return SC_OK;
}

int sb_band_width() { return kB; }
