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
// Files: this one holds the slab layout and the driver of stages 1 and 2; sy2sb.hip stage 1, sb2st.hip stage 2, bt2.hip the
// Q2 back-transformation (bt2); twostage_internal.h what they share; twostage_policy.h every choice between kernel forms.
#include <algorithm>
#include <vector>

#include "twostage_internal.h"

// ================================================================================================================
// Layout
size_t sb_slab_doubles(int n, int batch, SbLayout* out) {
  SbLayout L{};
  L.n = n;
  long long off = 0;
  auto take = [&](long long cnt) { long long o = off; off += (cnt + 31) / 32 * 32; return o; };
  const int nchunk = (n + kQrRows - 1) / kQrRows + 1;
  L.vw = take((long long)n * 4 * kB);
  L.wv = take((long long)n * 4 * kB);
  L.xv = take((long long)n * 3 * kB);
  L.symm_split = sc_host::symm_split_for(sc_host::two_stage_env(), n, batch);
  L.xsplit = L.symm_split > 1 ? take((long long)2 * L.symm_split * n * kB) : 0;
  L.qrpart = take((long long)2 * nchunk * kB);
  L.qrpiv = take(2 * (kB + 8));
  L.qrpart8 = take((long long)nchunk * kIb * kB);
  L.small = take((long long)kSmallSplit * kB * 3 * kB);
  L.cmat = take(3 * kB * kB);
  L.small2 = take((long long)kSmallSplit * 2 * kB * kB);
  L.p2 = take(2 * kB * kB);
  L.ab = take((long long)kLdab * n);
  // diamonds
  const int nsweep = std::max(n - 2, 0);
  L.ngroups = (nsweep + kG - 1) / kG;
  long long ndia = 0;
  for (int S = 0; S < L.ngroups; ++S) {
    const int len = (n - 1 - S * kG + kB - 1) / kB;
    ndia += len;
  }
  L.ndia = ndia;
  L.vd = take(ndia * kDiaSize);
  L.frag = take(ndia * kFragDoubles);
  L.tau2 = take(ndia * kG);
  L.slab = off;
  if (out) *out = L;
  return (size_t)off;
}

int sb_desc_count(int n, int batch) {
  const int npanels = n / kB + 1;
  return npanels * kDescKinds * batch;
}

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

  // ---- descriptors of stage 1 (sy2sb.hip); the panels' roles: 0 single, 1 first of a pair, 2 second of a pair
  const std::vector<int> role = sc_host::panel_roles(sc_host::two_stage_env(), n);
  const std::vector<GemmDesc> hs = sb_stage1_records(n, batch, role, d_a, stride_a, d_sb_ws, SL);
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
