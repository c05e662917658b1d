// Generalized correlation of atom pairs from the linear mutual information (Lange & Grubmueller 2006) for a batch, over
// the selected modes and without a covariance in memory.
//
// w (batch, nvec), v (batch, nvec, m) rows = modes, m = 3 N (ANM only), and per (structure, listed row) the weight s of
// k_mode_weights (batch_consumers.hip): 1 / lambda for a selected row, exactly 0.0 for any other.
//
//   C_ac  = sum_r s[b, r] v_r[a] v_r[c]^T                  the 3 x 3 block (a, c) of the covariance
//   P_a C_aa P_a^T = L_a L_a^T (Cholesky, diagonal pivoting),  W_a = L_a^-1 P_a       3 x 3, W_a C_aa W_a^T = I
//   M     = W_a C_ac W_c^T,  S = M M^T
//   delta = det(I - S) clamped to [0, 1]
//   out[b, a, c] = sqrt(1 - cbrt(delta))                    information: -1/2 ln(delta), in nats
//
// which is 1/2 [ln det C_aa + ln det C_cc - ln det C_(ac)] of the 6 x 6 block of the two atoms and r = sqrt(1 - exp(-2 I /
// 3)).  Both are invariant under any invertible linear map per atom (it changes L_a and cancels in M M^T up to an orthogonal
// factor), so there is no temperature and no per-atom scale: a mass-weighted solve gives the Cartesian result.
//
// Three steps on the stream.  (1) The diagonal blocks C_aa are the anisotropic tensors of the same selection and weights:
// batch_aniso_device (batch_consumers.hip) writes them, six doubles per atom, into the modes workspace behind its own
// weights and partial sums.  (2) k_lmi_whiten, one lane per atom, writes the nine entries of W_a behind them (the permutation
// moves the zeros of L_a^-1, so six numbers do not describe W_a).  A pivot that is not finite or is <= 2^-40 times the block's
// own diagonal entry (a definition: fewer than three selected modes, an atom at rest in the selection) makes all nine NaN.
// (3) k_mode_lmi runs on the pair-block core of pair_block_tile.h, which describes the data flow, with the tile ownership
// of k_mode_prs (mode_prs.hip): 64 x 64 atom tiles with tile_a >= tile_c, the weight folded into the a side, the nine
// entries of one C_ac in one lane, no per-atom scale.  Selection happens at the fetch, so 0 * NaN from a window's padding
// never reaches a result, and a NaN weight is staged as NaN on the a side of all atoms of its structure alone.
// The tensors are summed in chunks of kLmiTensorChunk listed rows, a constant, where the tensor consumer itself cuts by the
// number of listed rows: rows without weight behind a structure's own (a ragged slot's pad rows) then fill chunks of
// exact zeros and move no boundary, and a member of a ragged batch has the bits of its uniform solve.
//
// The epilogue, per pair of the lane (8 of them: 4 atoms a, 2 atoms c), in one fixed order: T = W_a C (27 multiply-adds),
// M = T W_c^T (27), the six entries of S (18), I - S, the determinant by the first row's cofactors (14), the clamp written so that NaN stays NaN, then the cube root and square root or the logarithm.  The value
// is stored to [a, c] and [c, a] from one register (a diagonal tile from its a >= c lanes only), so the result equals its
// transpose bit for bit; [a, a] is 1.0 / +inf by definition, NaN where W_a is.  No atomics, no partial sums across
// workgroups: a structure's bits depend on its own w, v and the selection only.
// Ragged batches: N, W (at 9 atom_off) and the result (at sq_off) are the structure's own, m is the slot order.
//
// Per (pair, row): 18 flops on the matrix pipe, as k_mode_prs; per pair once: about 180 flops and two or three
// transcendental calls on the vector pipe.
#include <algorithm>
#include <cmath>

#include "eigh_internal.h"
#include "pair_block_tile.h"

namespace {

using namespace pair_tile;

constexpr double kPivotFloor = 0x1p-40;       // a pivot <= this times its diagonal entry: the block cannot be whitened

struct LmiArgs : ListedRows {   // (scale: null)
  const double* wh;         // (batch, N, 9) whitening factors; ragged: packed at 9 atom_off
  int information;
};

__device__ __forceinline__ double pick3(int i, double x0, double x1, double x2) { return i == 0 ? x0 : (i == 1 ? x1 : x2); }

// t[b, a, :] = xx yy zz xy xz yz of C_aa  ->  wh[b, a, :] = the nine entries, row-major, of W_a = L^-1 P, P C_aa P^T = L L^T
// the Cholesky factorisation with diagonal pivoting (the largest remaining diagonal entry next, the lower index on a tie), or
// nine NaN.  Without pivoting the elimination's growth, sqrt(yy / d1), multiplies the rounding noise that is the third pivot
// of a rank-two block, and the rule below would let such a block pass; with it the growth is bounded.
__global__ __launch_bounds__(256) void k_lmi_whiten(const double* __restrict__ t, double* __restrict__ wh, int N,
                                                    const RaggedRec* __restrict__ rag, int b0) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  const size_t b = (size_t)b0 + blockIdx.y;
  if (rag) N = rag[b].n_atoms;
  if (a >= N) return;
  const size_t at = (rag ? (size_t)rag[b].atom_off : b * N) + a;
  const double* p = t + at * 6;
  const double xx = p[0], yy = p[1], zz = p[2], xy = p[3], xz = p[4], yz = p[5];
  // entry (i, j) of the symmetric block
  auto entry = [&](int i, int j) {
    return pick3(i, pick3(j, xx, xy, xz), pick3(j, xy, yy, yz), pick3(j, xz, yz, zz));
  };
  int p0 = yy > xx ? 1 : 0;
  if (zz > pick3(p0, xx, yy, zz)) p0 = 2;
  int q1 = p0 == 0 ? 1 : 0, q2 = p0 == 2 ? 1 : 2;
  const double b00 = entry(p0, p0);
  const double l00 = sqrt(b00);
  double l10 = entry(q1, p0) / l00, l20 = entry(q2, p0) / l00;
  double s11 = entry(q1, q1) - l10 * l10, s22 = entry(q2, q2) - l20 * l20;
  const double s12 = entry(q2, q1) - l20 * l10;
  if (s22 > s11) {
    const int qi = q1; q1 = q2; q2 = qi;
    double x = l10; l10 = l20; l20 = x;
    x = s11; s11 = s22; s22 = x;
  }
  const double d1 = s11;
  const double l11 = sqrt(d1);
  const double l21 = s12 / l11;
  const double d2 = s22 - l21 * l21;
  const double l22 = sqrt(d2);
  // (a NaN pivot fails every comparison, an infinite one the second)
  const bool ok = b00 > kPivotFloor * b00 && b00 < HUGE_VAL && d1 > kPivotFloor * entry(q1, q1) && d1 < HUGE_VAL &&
                  d2 > kPivotFloor * entry(q2, q2) && d2 < HUGE_VAL;
  const double w00 = 1.0 / l00, w11 = 1.0 / l11, w22 = 1.0 / l22;
  const double w10 = -(l10 * w00) * w11;
  const double w21 = -(l21 * w11) * w22;
  const double w20 = -(l20 * w00 + l21 * w10) * w22;
  const double nan = __builtin_nan("");
  double* o = wh + at * 9;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int j = c == p0 ? 0 : (c == q1 ? 1 : 2);   // column c of W_a is column j of L^-1
    o[c] = ok ? pick3(j, w00, 0.0, 0.0) : nan;
    o[3 + c] = ok ? pick3(j, w10, w11, 0.0) : nan;
    o[6 + c] = ok ? pick3(j, w20, w21, w22) : nan;
  }
}

// the value of one pair from its covariance block c[d][e] and the two whitening factors, in one fixed operation order
__device__ __forceinline__ double lmi_pair(const double (&c)[3][3], const double (&wa)[9], const double (&wc)[9],
                                           int information) {
  double t[3][3], mm[3][3];
#pragma unroll
  for (int d = 0; d < 3; ++d)   // T = W_a C
#pragma unroll
    for (int e = 0; e < 3; ++e) t[d][e] = wa[3 * d] * c[0][e] + wa[3 * d + 1] * c[1][e] + wa[3 * d + 2] * c[2][e];
#pragma unroll
  for (int d = 0; d < 3; ++d)   // M = T W_c^T
#pragma unroll
    for (int e = 0; e < 3; ++e) mm[d][e] = t[d][0] * wc[3 * e] + t[d][1] * wc[3 * e + 1] + t[d][2] * wc[3 * e + 2];
  // A = I - M M^T
  const double a00 = 1.0 - (mm[0][0] * mm[0][0] + mm[0][1] * mm[0][1] + mm[0][2] * mm[0][2]);
  const double a11 = 1.0 - (mm[1][0] * mm[1][0] + mm[1][1] * mm[1][1] + mm[1][2] * mm[1][2]);
  const double a22 = 1.0 - (mm[2][0] * mm[2][0] + mm[2][1] * mm[2][1] + mm[2][2] * mm[2][2]);
  const double a01 = -(mm[0][0] * mm[1][0] + mm[0][1] * mm[1][1] + mm[0][2] * mm[1][2]);
  const double a02 = -(mm[0][0] * mm[2][0] + mm[0][1] * mm[2][1] + mm[0][2] * mm[2][2]);
  const double a12 = -(mm[1][0] * mm[2][0] + mm[1][1] * mm[2][1] + mm[1][2] * mm[2][2]);
  double delta = a00 * (a11 * a22 - a12 * a12) - a01 * (a01 * a22 - a12 * a02) + a02 * (a01 * a12 - a11 * a02);
  delta = delta < 0.0 ? 0.0 : (delta > 1.0 ? 1.0 : delta);   // (not fmin / fmax: NaN stays NaN)
  return information ? -0.5 * log(delta) : sqrt(1.0 - cbrt(delta));
}

// grid (tiles with tile_a >= tile_c, structures of the slab)
__global__ __launch_bounds__(512) void k_mode_lmi(const LmiArgs A) {
  __shared__ double lds[kLdsDoubles];
  int ta, tc;
  tri_tile_decode(blockIdx.x, ta, tc);
  const int b = A.b0 + blockIdx.y;
  const int N = A.rag ? A.rag[b].n_atoms : A.m / 3;
  const int a0 = ta * kTile, c0 = tc * kTile;   // c0 <= a0
  if (a0 >= N) return;                          // (the whole workgroup: a ragged structure smaller than the grid)
  const size_t atom_off = A.rag ? (size_t)A.rag[b].atom_off : (size_t)b * N;
  double* ob = A.out + (A.rag ? (size_t)A.rag[b].sq_off : (size_t)b * N * N);
  const double* whb = A.wh + atom_off * 9;

  const Lanes L = lanes(lds, threadIdx.x);
  d4 acc[2][3][3];
  mode_blocks<false>(A, lds, L, b, N, atom_off, a0, c0, acc);

  // the epilogue: the lane's pairs.  An atom behind the structure's own takes the factors of its last atom and stores nothing
  const bool diag = ta == tc;
  const double defined = A.information ? HUGE_VAL : 1.0;
  double wc[9];
  for_pairs(
      L, acc,
      [&](int cl) {
        const double* p = whb + (size_t)min(c0 + cl, N - 1) * 9;
#pragma unroll
        for (int i = 0; i < 9; ++i) wc[i] = p[i];
      },
      [&](int al, int cl, const double (&cb)[3][3]) {
        const int a = a0 + al, c = c0 + cl;
        double wa[9];
        const double* p = whb + (size_t)min(a, N - 1) * 9;
#pragma unroll
        for (int i = 0; i < 9; ++i) wa[i] = p[i];
        double val = lmi_pair(cb, wa, wc, A.information);
        if (a >= N || c >= N || (diag && a < c)) return;
        if (a == c) {
          val = wa[0] != wa[0] ? wa[0] : defined;   // (k_lmi_whiten writes nine NaN or none)
        }
        ob[(size_t)a * N + c] = val;
        if (a != c) ob[(size_t)c * N + a] = val;
      });
}

}  // namespace

// what = 8 beside the weights and the tensors' partial sums: the tensors, six doubles per atom of the batch, and the
// factors, nine (ragged: packed over all atoms)
static size_t lmi_tensor_bytes(int64_t m, int64_t batch, const RaggedView* rv) {
  const size_t atoms = rv ? (size_t)rv->total_atoms : (size_t)batch * (size_t)(m / 3);
  return align_up(atoms * 6 * 8, 256);
}
size_t modes_lmi_whiten_bytes(int64_t m, int64_t batch, const RaggedView* rv) {
  const size_t atoms = rv ? (size_t)rv->total_atoms : (size_t)batch * (size_t)(m / 3);
  return lmi_tensor_bytes(m, batch, rv) + align_up(atoms * 9 * 8, 256);
}

// dim 3 only (the callers check): d_out (batch, m / 3, m / 3), ragged (sum n_atoms^2) packed
int batch_lmi_device(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                     const sc_mode_selection& sel, const int64_t* d_counts, int information, double* d_out,
                     const RaggedView* rv) {
  hipStream_t st = ctx->stream;
  const int64_t nsel = batch_modes_nsel(sel, nvec);
  const int64_t N = rv ? rv->max_atoms : m / 3;   // (bounds the grids)
  // the whole workspace: batch_aniso_device's layout (weights, partial sums in chunks of kLmiTensorChunk rows) is its head
  const size_t total = batch_modes_workspace_bytes(m, nvec, batch, 3, nsel, 8, 0, rv);
  SC_TRY(sc_reserve_modes(ctx, total));
  double* d_s = reinterpret_cast<double*>(ctx->modes_ws);
  double* d_t = reinterpret_cast<double*>((char*)ctx->modes_ws + (total - 1024 - modes_lmi_whiten_bytes(m, batch, rv)));
  double* d_wh = reinterpret_cast<double*>((char*)d_t + lmi_tensor_bytes(m, batch, rv));
  // weights (at the head of the workspace) and diagonal blocks; an empty selection gives zero blocks, which fail the pivot rule
  SC_TRY(batch_aniso_device(ctx, d_w, d_v, m, nvec, batch, sel, d_counts, 0, d_t, rv, kLmiTensorChunk));
  LmiArgs A{};
  A.v = d_v; A.s = d_s; A.wh = d_wh; A.out = d_out;
  fill_listed_rows(A, sel, nsel, nvec, m, rv);
  A.information = information ? 1 : 0;
  const unsigned tiles = tri_tiles(N);
  const unsigned strips = (unsigned)((N + 255) / 256);
  for (int64_t b0 = 0; b0 < batch; b0 += kMaxSlab) {
    const unsigned nb = (unsigned)std::min(kMaxSlab, batch - b0);
    A.b0 = (int)b0;
    hipLaunchKernelGGL(k_lmi_whiten, dim3(strips, nb), dim3(256), 0, st, d_t, d_wh, (int)N, A.rag, (int)b0);
    hipLaunchKernelGGL(k_mode_lmi, dim3(tiles, nb), dim3(512), 0, st, A);
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}
