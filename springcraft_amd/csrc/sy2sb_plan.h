// The plan of the band reduction (sy2sb.hip): the per-matrix slab, the geometry of a panel, the GEMM records of a solve and
// where each sits, the dynamic-LDS layout of every stage-1 kernel, k_panel_coop's carve of sc_ctx::dc_aux and the parts of
// a batch that is split over streams.  Same form as stedc_plan.h and twostage_policy.h (which says WHICH kernel form runs):
// no HIP, header-only, closed-form functions of integers; tests/host_sanitize/test_sy2sb_plan.cpp compiles exactly this
// code with g++ -fsanitize=address,undefined.  The host takes every LDS byte count from here and so do the kernels' carves.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "gemm_policy.h"       // GemmDesc
#include "twostage_policy.h"   // kBand, panel_count, symm_split_for, SC_POLICY_HD, kLdsPerWorkgroup

#ifndef SC_QR_IB
#define SC_QR_IB 8
#endif

// Per-matrix workspace slab of the two-stage path (offsets in doubles from the slab base).
struct SbLayout {
  int n;
  long long slab;
  long long vw, wv;   // [V|W], [W|V] panels of TWO consecutive panels, n x 256 (the trailing update takes them together)
  long long xv;       // [X1|X2|V], n x 192
  long long qrpart, qrpiv;   // panel-QR partial Gram rows / pivot row (two copies each)
  long long qrpart8;         // blocked panel QR: per-chunk partial products of an inner block, nchunk x 8 x 64
  long long xsplit;   // K slices of X1 and X2 when the SYMM runs split-K: 2 x symm_split x (n x 64)
  int symm_split;     // 1: no split
  long long small;    // split-K slices of V^T [X1|X2|V]
  long long cmat;     // [T; T; -S/2], 192 x 64
  long long small2;   // split-K slices of [W1|V1]^T V2 (second panel of a pair), 128 x 64 each
  long long p2;       // their sum
  long long ab;       // band storage 128 x n
  int ngroups;        // sweep groups (64 sweeps each)
  long long ndia;     // diamonds
  long long vd;       // diamonds: V row-major (128 rows x 64 sweeps)
  long long frag;     // diamonds: MFMA fragments of V^T and -(V T), 160 x 64 doubles each (k_dia_tfactor2 -> k_bt2_apply)
  long long tau2;     // ndia x 64
};

namespace sc_host {

constexpr int kSweepGroup = 64;                    // sweeps per diamond
constexpr int kDiaDoubles = 128 * kSweepGroup;     // a diamond: leading dimension 128 (kBand + kSweepGroup - 1 = 127 rows used)
constexpr int kDiaFragDoubles = 4 * 40 * 64;       // its 160 MFMA fragments (order and use: bt2.hip), 80 KB
constexpr int kBandRows = 2 * kBand;               // rows of the band storage: AB(i, j) = ab[(i - j) + j * kBandRows]
constexpr int kQrRows = 128;                       // rows of the panel one k_panel_qr workgroup owns
constexpr int kQrIb = SC_QR_IB;                    // inner block of the blocked panel QR
constexpr int kSmallSplit = 8;                     // split-K of the V^T [X1|X2|V] product

// The slab of an order-n matrix whose SYMM runs in symm_split K slices (which need room); returns its doubles
inline size_t sb_slab_layout(int n, int symm_split, SbLayout* out) {
  SbLayout L{};
  L.n = n;
  L.symm_split = symm_split;
  long long off = 0;
  auto take = [&](long long cnt) { long long o = off; off += (cnt + 31) / 32 * 32; return o; };
  const int nchunk = (n + kQrRows - 1) / kQrRows + 1;
  L.vw = take((long long)n * 4 * kBand);
  L.wv = take((long long)n * 4 * kBand);
  L.xv = take((long long)n * 3 * kBand);
  L.xsplit = L.symm_split > 1 ? take((long long)2 * L.symm_split * n * kBand) : 0;
  L.qrpart = take((long long)2 * nchunk * kBand);
  L.qrpiv = take(2 * (kBand + 8));
  L.qrpart8 = take((long long)nchunk * kQrIb * kBand);
  L.small = take((long long)kSmallSplit * kBand * 3 * kBand);
  L.cmat = take(3 * kBand * kBand);
  L.small2 = take((long long)kSmallSplit * 2 * kBand * kBand);
  L.p2 = take(2 * kBand * kBand);
  L.ab = take((long long)kBandRows * n);
  L.ngroups = (std::max(n - 2, 0) + kSweepGroup - 1) / kSweepGroup;
  for (int S = 0; S < L.ngroups; ++S) L.ndia += (n - 1 - S * kSweepGroup + kBand - 1) / kBand;   // diamonds of sweep group S
  L.vd = take(L.ndia * kDiaDoubles);
  L.frag = take(L.ndia * kDiaFragDoubles);
  L.tau2 = take(L.ndia * kSweepGroup);
  L.slab = off;
  if (out) *out = L;
  return (size_t)off;
}
// batch: matrices of the solve (few matrices: more slices)
inline size_t sb_slab_doubles(int n, int batch, SbLayout* out) {
  return sb_slab_layout(n, symm_split_for(two_stage_env(), n, batch), out);
}

// ---- panels and their GEMM records --------------------------------------------------------------------------------
// Panel p factors the columns j0 .. j0 + 63 below the band: rows r0 .. n - 1, m of them, nr reflectors (64 unless the
// panel is the short last one), in nchunks chunks of kQrRows rows (the grid of the chunked launches).
struct PanelGeom { int j0, r0, m, nr, nchunks; };
inline PanelGeom panel_geom(int n, int p) {
  const int r0 = (p + 1) * kBand, m = n - r0;
  return {p * kBand, r0, m, std::min(kBand, m - 1), (m + kQrRows - 1) / kQrRows};
}

// The records of one panel and matrix (V: the panel's reflectors, L: the lower-stored trailing matrix A22).
enum SbRec : int {
  kRecX1,      // X1 = L V
  kRecX2,      // X2 = strict(L)^T V
  kRecGram,    // V^T [X1 | X2 | V], split-K slices
  kRecW,       // W = [X1 | X2 | V] C into its column block of [V|W..]
  kRecNegW,    // -W into its column block of [W|V..]
  kRecTrail,   // trailing update, lower triangle: A22 += [V|W] (-[W|V])^T; second of a pair: both panels' blocks, K = 256
  kRecFirst,   // first of a pair: only the next panel's 64 columns get this panel's update now
  kRecP2,      // second of a pair: P2 = (-[W1|V1])^T V2, split-K slices
  kRecCorr,    // ... and the correction X1 += [V1|W1] P2
  kRecKinds
};
// Records the solve reserves: those of n / 64 + 1 panels, never fewer than the panels there are -- panel_count(n) is
// (n - 2) / 64 for n >= 2, at most n / 64.  (The surplus is kept: the workspace totals are pinned by the tests.)
inline int stage1_record_count(int n, int batch) { return (n / kBand + 1) * kRecKinds * batch; }
// Where the record of (panel, kind, matrix) sits: the records of one launch (a kind, matrices lo .. hi - 1) are contiguous
inline size_t stage1_record_index(int p, int kind, int batch, int b) { return ((size_t)p * kRecKinds + kind) * batch + b; }

// Every record of a solve, on device addresses (d_a: the matrices, d_sb_ws: their slabs); role: panel_roles.
inline std::vector<GemmDesc> stage1_records(int n, int batch, const std::vector<int>& role, bool use_symm3, double* d_a,
                                            long long stride_a, double* d_sb_ws, const SbLayout& SL) {
  constexpr int kB = kBand;
  std::vector<GemmDesc> h(role.size() * kRecKinds * batch);
  for (int p = 0; p < (int)role.size(); ++p) {
    const int r0 = panel_geom(n, p).r0, m = panel_geom(n, p).m;
    const bool second = role[(size_t)p] == 2;
    const long long vw_w = second ? 3 * kB : kB, wv_w = second ? 2 * kB : 0;   // columns W goes to
    for (int b = 0; b < batch; ++b) {
      double* sb = d_sb_ws + (size_t)b * SL.slab;
      double* a22 = d_a + (size_t)b * stride_a + (size_t)r0 * n + r0;
      double* x1 = sb + SL.xv + r0;                          // [X1 | X2 | V], ld n
      double* v = sb + SL.xv + (size_t)2 * kB * n + r0;
      auto rec = [&](int kind) -> GemmDesc& { return h[stage1_record_index(p, kind, batch, b)]; };
      // C (m x nn, ld ldc) = beta C + A B over K = kk with A(i, k) = a[i sa_i + k sa_k], B(k, j) = bb[k sb_k + j sb_j]
      auto put = [&](int kind, const double* a, long long sa_i, long long sa_k, const double* bb, long long sb_k, long long sb_j,
                     double* c, long long ldc, int mm, int nn, int kk, double beta) -> GemmDesc& {
        GemmDesc& g = rec(kind);
        g.a = a; g.sa_i = sa_i; g.sa_k = sa_k;
        g.b = bb; g.sb_k = sb_k; g.sb_j = sb_j;
        g.c = c; g.ldc = ldc;
        g.m = mm; g.n = nn; g.k = kk; g.alpha = 1.0; g.beta = beta;
        return g;
      };
      GemmDesc& X1 = put(kRecX1, a22, 1, n, v, 1, n, x1, n, m, kB, m, 0.0);
      X1.a_tri = 1;
      if (SL.symm_split > 1) {   // K slices into their own buffers, summed into X1 / X2 by k_sum_xslices
        X1.c = sb + SL.xsplit + r0;
        X1.split_stride = (long long)n * kB;
      }
      GemmDesc& X2 = rec(kRecX2) = X1;
      X2.sa_i = n; X2.sa_k = 1; X2.a_tri = 2;
      X2.c = SL.symm_split > 1 ? sb + SL.xsplit + (size_t)SL.symm_split * n * kB + r0 : x1 + (size_t)kB * n;
      put(kRecGram, v, n, 1, x1, 1, n, sb + SL.small, kB, kB, 3 * kB, m, 0.0).split_stride = (long long)kB * 3 * kB;
      const GemmDesc& W = put(kRecW, x1, 1, n, sb + SL.cmat, 1, 3 * kB, sb + SL.vw + (size_t)vw_w * n + r0, n, m, kB, 3 * kB, 0.0);
      // (the [W|V] panel holds -[W|V], so that every product that subtracts -- the trailing updates, the correction of X
      // in a pair -- has alpha = 1: the role-split kernel k_gemm3 keeps C itself in its accumulators and folds no sign;
      // negation is exact, the results are bit for bit those of alpha = -1 on [W|V])
      GemmDesc& NW = rec(kRecNegW) = W;
      NW.c = sb + SL.wv + (size_t)wv_w * n + r0;
      NW.alpha = -1.0;
      GemmDesc& R = put(kRecTrail, sb + SL.vw + r0, 1, n, sb + SL.wv + r0, n, 1, a22, n, m, m, second ? 4 * kB : 2 * kB, 1.0);
      // (with k_symm3 in use the trailing updates also keep the first super-diagonal entry of every even row: symm3.hip)
      R.lower_only = use_symm3 ? 2 : 1;
      GemmDesc& D = rec(kRecFirst) = R;
      D.n = kB; D.k = 2 * kB;
      // second of a pair (rows r0 .. of the first panel's blocks); P2 comes out negated (a = -[W1|V1])
      put(kRecP2, sb + SL.wv + r0, n, 1, v, 1, n, sb + SL.small2, 2 * kB, 2 * kB, kB, m, 0.0).split_stride = (long long)2 * kB * kB;
      put(kRecCorr, sb + SL.vw + r0, 1, n, sb + SL.p2, 1, 2 * kB, x1, n, m, kB, 2 * kB, 1.0);
    }
  }
  return h;
}

// ---- dynamic LDS of the stage-1 kernels: offsets in doubles from the base; a launch asks for 8 * total bytes -------------
// No launch may ask for more than the device's LDS per workgroup; only k_panel_coop also raises its attribute.
struct LdsPanelQr { int P, wv, vv, red, total; };      // k_panel_qr holding ncl columns: kQrIb + 1 (blocked) or 64
SC_POLICY_HD constexpr LdsPanelQr lds_panel_qr(int ncl) {
  const int wv = ncl * (kQrRows + 1), vv = wv + kBand, red = vv + kQrRows;
  return {0, wv, vv, red, red + 4 * kBand};
}
// k_pqr_blk_a / _b hold columns c0 .. 63 of the chunk; mid: _a kQrRows doubles without a user (kept: the launches' bytes stay), _b Ms
struct LdsBlk { int P, mid, red, total; };
SC_POLICY_HD constexpr LdsBlk lds_pqr_blk_a(int c0) {
  const int vv = (kBand - c0) * (kQrRows + 1), red = vv + kQrRows;
  return {0, vv, red, red + 8 * kBand};
}
SC_POLICY_HD constexpr LdsBlk lds_pqr_blk_b(int c0) {
  const int Ms = (kBand - c0) * (kQrRows + 1), red = Ms + kQrIb * kBand;
  return {0, Ms, red, red + 4 * kBand};
}
struct LdsPanelWg { int red, piv, tauL, Ms, part, total; };   // k_panel_wg<.., NT>
SC_POLICY_HD constexpr LdsPanelWg lds_panel_wg(int nt) {
  const int waves = nt / 64, piv = 2 * waves * 8, tauL = piv + 16, Ms = tauL + 8, part = Ms + 8 * kBand;
  return {0, piv, tauL, Ms, part, part + waves * kBand * 8};
}
struct LdsPanelCoop { int Pl, Vl, Ms, red, piv, tauA, tot4, dead, total; };
SC_POLICY_HD constexpr LdsPanelCoop lds_panel_coop() {
  const int Vl = kBand * (kCoopRows + 1), Ms = Vl + kCoopRows * 8, red = Ms + 8 * kBand, piv = red + 64, tauA = piv + 16,
            tot4 = tauA + kBand, dead = tot4 + 128;
  return {0, Vl, Ms, red, piv, tauA, tot4, dead, dead + 2};
}
struct LdsSbSmall { int G, M1, T, U, total; };          // k_sb_small: four 64 x 65 matrices
SC_POLICY_HD constexpr LdsSbSmall lds_sb_small() {
  const int sq = kBand * (kBand + 1);
  return {0, sq, 2 * sq, 3 * sq, 4 * sq};
}
constexpr size_t lds_bytes(int total_doubles) { return sizeof(double) * (size_t)total_doubles; }
static_assert(lds_bytes(lds_panel_qr(kQrIb + 1).total) <= 64 * 1024 && lds_bytes(lds_panel_wg(512).total) <= 64 * 1024, "");
// (the others are above 64 KB at their largest -- 68.0, 69.5, 70.5, 70.2 and 130 KB -- and are launched without an attribute)
static_assert(lds_bytes(lds_panel_qr(kBand).total) <= kLdsPerWorkgroup && lds_bytes(lds_pqr_blk_a(0).total) <= kLdsPerWorkgroup &&
              lds_bytes(lds_pqr_blk_b(0).total) <= kLdsPerWorkgroup && lds_bytes(lds_panel_wg(1024).total) <= kLdsPerWorkgroup &&
              lds_bytes(lds_sb_small().total) <= kLdsPerWorkgroup && lds_bytes(lds_panel_coop().total) <= kLdsPerWorkgroup, "");

// ---- k_panel_coop's records in sc_ctx::dc_aux (byte offsets) -------------------------------------------------------------
constexpr int kCoopVals = 8 * kBand;   // values of one block exchange (M and the Gram matrix)
// 16-byte records of one matrix with G workgroups: column records [2][G][16] | block partials [G][512] | block totals [512]
SC_POLICY_HD constexpr size_t coop_recs_per_matrix(int G) { return (size_t)2 * G * 16 + (size_t)G * kCoopVals + kCoopVals; }
struct CoopAux {
  size_t ctl;    // one control record of 8 ints per matrix
  size_t recs;   // coop_recs_per_matrix(gmax) records per matrix (the tallest panel's count, whatever G a launch has)
  size_t total;  // zeroed per solve: sequence numbers are unique within a solve only
};
inline CoopAux coop_aux_carve(int batch, int gmax) {
  const size_t recs = policy_align_up((size_t)batch * 8 * sizeof(int), 256);
  return {0, recs, recs + (size_t)batch * coop_recs_per_matrix(gmax) * 16};
}

// ---- parts of a batch on separate streams: part q of `parts` holds the matrices [lo, hi) ---------------------------------
struct PartBounds { int lo, hi; };
inline PartBounds part_bounds(int batch, int parts, int q) {
  return {(int)((long long)batch * q / parts), (int)((long long)batch * (q + 1) / parts)};
}

}  // namespace sc_host
