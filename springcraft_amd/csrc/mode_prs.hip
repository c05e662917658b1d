// Perturbation-response scanning (nma.py:476-524) for a batch, over the selected modes and without a covariance in memory.
//
// w (batch, nvec), v (batch, nvec, m) rows = modes, m = 3 N (ANM only), and per (structure, listed row) the weight s of
// k_mode_weights (batch_consumers.hip): 1 / lambda for a selected row, exactly 0.0 for any other.
//
//   u_r[a]     = scale[b, a] * V[b, r, 3 a .. 3 a + 2]              scale: NULL = 1 (mass-weighted solve: 1 / sqrt(mass))
//   C_ac[d, e] = sum_r  s[b, r] * u_r[a][d] * u_r[c][e]             the 3 x 3 block (a, c) of the covariance
//   P[b, a, c] = sum_{d, e} C_ac[d, e]^2                            norm: P[b, a, c] / P[b, a, a]
//
// the reference's two reduceat of cov**2.  The one-model path (consumers.hip) writes V / w and the (3N, 3N) covariance to
// scratch and reduces them afterwards; here a block C_ac lives in nine accumulator slots of one lane and is squared there.
//
// k_mode_prs runs on the pair-block core of pair_block_tile.h, which describes the data flow: 64 x 64 atom tiles of one
// structure, 512 lanes, the listed rows walked in order on the f64 matrix pipe, selection and the NaN rule at the fetch.
// Its own part is the epilogue: the sum of squares of a block in one fixed (d, e) order, in the lane that holds it.
//
// Only tiles with tile_a >= tile_c exist; they store P[a, c] and P[c, a] from the same register (a diagonal tile from its
// a >= c lanes only: the weight is folded into the a side, so the (c, a) lane may round differently), and the unnormalised
// matrix equals its transpose bit for bit.  No atomics, no partial sums across workgroups: a structure's bits depend on
// its own w, v, scale and the selection only.  norm: the diagonal is copied to the workspace, then row a is divided by
// it in a second small launch; an empty selection gives zeros, and 0 / 0 = NaN under norm as in NumPy.
// Ragged batches: N, the scale (at atom_off) and the result (at sq_off) are the structure's own, m is the slot order; pad
// rows carry no weight, pad columns are never read.
#include <algorithm>
#include <cmath>

#include "eigh_internal.h"
#include "pair_block_tile.h"

namespace {

using namespace pair_tile;

using PrsArgs = ListedRows;

// grid (tiles with tile_a >= tile_c, structures of the slab)
__global__ __launch_bounds__(512) void k_mode_prs(const PrsArgs A) {
  __shared__ double lds[kLdsDoubles];
  int ta, tc;
  tri_tile_decode(blockIdx.x, ta, tc);
  const int b = A.b0 + blockIdx.y;
  const int N = A.rag ? A.rag[b].n_atoms : A.m / 3;
  const int a0 = ta * kTile, c0 = tc * kTile;   // c0 <= a0
  if (a0 >= N) return;                          // (the whole workgroup: a ragged structure smaller than the grid)
  const size_t atom_off = A.rag ? (size_t)A.rag[b].atom_off : (size_t)b * N;
  double* ob = A.out + (A.rag ? (size_t)A.rag[b].sq_off : (size_t)b * N * N);

  const Lanes L = lanes(lds, threadIdx.x);
  d4 acc[2][3][3];
  mode_blocks<true>(A, lds, L, b, N, atom_off, a0, c0, acc);

  const bool diag = ta == tc;
  for_pairs(L, acc, [](int) {}, [&](int al, int cl, const double (&blk)[3][3]) {
    const int a = a0 + al, c = c0 + cl;
    double p = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
      for (int e = 0; e < 3; ++e) p = fma(blk[d][e], blk[d][e], p);
    if (a >= N || c >= N || (diag && a < c)) return;
    ob[(size_t)a * N + c] = p;
    if (a != c) ob[(size_t)c * N + a] = p;
  });
}

// diag[structure of the slab, a] <- P[a, a]; ragged: packed at atom_off
__global__ __launch_bounds__(256) void k_prs_diag(const double* __restrict__ out, int N, double* __restrict__ diag,
                                                  const RaggedRec* __restrict__ rag, int b0) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  const size_t b = (size_t)b0 + blockIdx.y;
  if (rag) {
    const RaggedRec r = rag[b];
    if (a < r.n_atoms) diag[r.atom_off + a] = out[r.sq_off + (size_t)a * r.n_atoms + a];
    return;
  }
  if (a < N) diag[(size_t)blockIdx.y * N + a] = out[(b * N + a) * N + a];
}

// row a of every structure of the slab divided by its original diagonal entry (nma.py:520-522)
__global__ __launch_bounds__(256) void k_prs_norm(double* __restrict__ out, const double* __restrict__ diag, int N,
                                                  const RaggedRec* __restrict__ rag, int b0) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int a = blockIdx.y;
  const size_t b = (size_t)b0 + blockIdx.z;
  if (rag) N = rag[b].n_atoms;
  if (a >= N || c >= N) return;
  const double* db = rag ? diag + rag[b].atom_off : diag + (size_t)blockIdx.z * N;
  double* ob = rag ? out + rag[b].sq_off : out + b * N * N;
  ob[(size_t)a * N + c] = ob[(size_t)a * N + c] / db[a];
}

}  // namespace

// what = 7 beside the weights: one diagonal per structure of a slab (ragged: packed over all atoms)
size_t modes_prs_diag_bytes(int64_t m, int64_t batch, const RaggedView* rv) {
  const size_t diag = rv ? (size_t)rv->total_atoms : (size_t)std::min(kMaxSlab, batch) * (size_t)(m / 3);
  return align_up(diag * 8, 256);
}

// dim 3 only (the callers check): d_out (batch, m / 3, m / 3), ragged (sum n_atoms^2) packed
int batch_prs_device(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                     const sc_mode_selection& sel, const int64_t* d_counts, const double* d_atom_scale, int norm,
                     double* d_out, const RaggedView* rv) {
  hipStream_t st = ctx->stream;
  const int64_t nsel = batch_modes_nsel(sel, nvec);
  const int64_t N = rv ? rv->max_atoms : m / 3;   // (bounds the grids)
  SC_TRY(sc_reserve_modes(ctx, batch_modes_workspace_bytes(m, nvec, batch, 3, nsel, 7, 0, rv)));
  double* d_s = reinterpret_cast<double*>(ctx->modes_ws);
  double* d_diag = reinterpret_cast<double*>((char*)ctx->modes_ws + align_up((size_t)batch * std::max<int64_t>(nsel, 1) * 8, 256));
  if (nsel == 0) {
    SC_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(double) * (rv ? (size_t)rv->total_sq : (size_t)batch * N * N), st));
  } else {
    SC_TRY(launch_mode_weights(ctx, d_w, nvec, batch, sel, nsel, d_counts, d_s, rv));
  }
  PrsArgs A{};
  A.v = d_v; A.s = d_s; A.scale = d_atom_scale; A.out = d_out;
  fill_listed_rows(A, sel, nsel, nvec, m, rv);
  const unsigned tiles = tri_tiles(N);
  const unsigned strips = (unsigned)((N + 255) / 256);
  for (int64_t b0 = 0; b0 < batch; b0 += kMaxSlab) {
    const unsigned nb = (unsigned)std::min(kMaxSlab, batch - b0);
    A.b0 = (int)b0;
    if (nsel > 0) hipLaunchKernelGGL(k_mode_prs, dim3(tiles, nb), dim3(512), 0, st, A);
    if (norm) {
      hipLaunchKernelGGL(k_prs_diag, dim3(strips, nb), dim3(256), 0, st, d_out, (int)N, d_diag, A.rag, (int)b0);
      hipLaunchKernelGGL(k_prs_norm, dim3(strips, (unsigned)N, nb), dim3(256), 0, st, d_out, d_diag, (int)N, A.rag, (int)b0);
    }
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}
