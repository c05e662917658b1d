// Fluctuations of the inter-atom distances over the selected modes, on the tensors the batched solvers leave in HBM.
//
// No reference counterpart (ProDy: calcDistFlucts / calcMechStiff; Bio3D derives it from the covariance).  w (batch, nvec),
// v (batch, nvec, m) rows = modes, m = 3 N (ANM only), coord (batch, N, 3), and per (structure, listed row) the weight s
// of k_mode_weights (batch_consumers.hip): 1 / lambda for a selected row, exactly 0.0 for any other.
//
//   F[b, a, c] = sum_r  s[b, r] * ( n_ac . (u_r[c] - u_r[a]) )^2        n_ac = (x_c - x_a) / |x_c - x_a|
//   u_r[a]     = scale[b, a] * V[b, r, 3 a .. 3 a + 2]                   scale: NULL = 1 (mass-weighted solve: 1 / sqrt(mass))
//
// the projection of the relative displacement of two atoms on the line between them: the harmonic constant of that
// distance's potential of mean force is k_B T / F.  n differs per pair, so the sum is no bilinear product of the rows; the
// expanded form n^T U_a n + n^T U_c n - 2 n^T C_ac n needs all nine component planes of the covariance and subtracts nearly
// equal numbers for neighbours.  The direct sum has only terms of one sign and is exactly symmetric, and it is what runs
// here, on the f64 vector unit: 3 subtractions, a 3-term dot product and two more operations per (pair, row), 8 in all.
//
// One workgroup of 256 lanes owns a 64 x 64 tile of atom pairs of one structure; lane (ty, tx) keeps the 4 x 4 pairs
// a = a0 + 4 ty + i, c = c0 + tx + 16 j: their unit vectors (48 doubles) and sums (16) stay in registers.  The workgroup
// walks the listed rows in order, kRows at a time: 192 lanes fetch the 3 x 64 consecutive doubles of the tile's two atom
// sets from each row (8-byte pieces: rows are only 8-byte aligned for odd N) while the previous group is summed, and put
// them, times scale, into LDS component-major, where the a side is read as broadcasts and the c side lane by lane.
// Only tiles with tile_a >= tile_c exist; they store F[a, c] and F[c, a] from the same sum.  The diagonal tile computes
// both orientations: every operand changes its sign exactly, so the bits agree; F[a, a] is stored as 0.0.  Two distinct
// atoms at one position: 0 / 0 = NaN for that pair.
//
// No atomics, no partial sums: a pair's sum is one fixed sequence over the listed rows, the same in any batch and at any
// position.  A row without weight is never read (nor is a listed row outside 0..nvec-1, whose NaN weight alone makes the
// structure's pairs NaN; a failed structure's weights are 1 / NaN).  Ragged batches: N, the coordinates (at atom_off), the
// result (at sq_off) are the structure's own, m is the slot order; pad rows carry no weight, pad columns are never read.
#include <algorithm>
#include <cmath>

#include "eigh_internal.h"
#include "pair_block_tile.h"   // (the listed rows and the grid of the pair consumers; the kernel is not on its MFMA core)

namespace {

constexpr int kTile = pair_tile::kTile;   // atoms per side of a tile
constexpr int kRows = 8;                  // listed rows staged in LDS at a time (24 KiB)
constexpr int kSide = 3 * kTile;          // doubles of one atom set of one row
using pair_tile::kMaxSlab;

struct DistFluctArgs : pair_tile::ListedRows {
  const double* coord;      // (batch, N, 3); ragged: packed
};

// the kRows x 2 values lane `tid` < kSide fetches of the group of listed rows from kk0 on: column tid of the a side and of
// the c side of every row that carries a weight
__device__ __forceinline__ void fetch_rows(const DistFluctArgs& A, const double* __restrict__ vb,
                                           const double* __restrict__ sb, int kk0, int ga, int gc, bool ok_a, bool ok_c,
                                           double (&pre)[2 * kRows]) {
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int kk = kk0 + r;
    const double sv = kk < A.nsel ? sb[kk] : 0.0;   // (uniform over the workgroup)
    pre[2 * r] = 0.0;
    pre[2 * r + 1] = 0.0;
    if (sv != 0.0 && sv == sv) {
      const int row = min(max(A.rows ? A.rows[kk] : A.row0 + kk, 0), A.nvec - 1);
      const double* p = vb + (size_t)row * A.m;
      if (ok_a) pre[2 * r] = p[ga];
      if (ok_c) pre[2 * r + 1] = p[gc];
    }
  }
}

// grid (tiles with tile_a >= tile_c, structures of the slab)
__global__ __launch_bounds__(256) void k_dist_fluct(const DistFluctArgs A) {
  __shared__ double lds[kRows * 2 * kSide];
  const int tid = threadIdx.x;
  const int t = blockIdx.x;
  int ta, tc;
  tri_tile_decode(t, ta, tc);
  const int b = A.b0 + blockIdx.y;
  const int N = A.rag ? A.rag[b].n_atoms : A.m / 3;
  const int a0 = ta * kTile, c0 = tc * kTile;   // c0 <= a0
  if (a0 >= N) return;                          // (the whole workgroup: a ragged structure smaller than the grid)
  const size_t atom_off = A.rag ? (size_t)A.rag[b].atom_off : (size_t)b * N;
  const double* xb = A.coord + 3 * atom_off;
  double* ob = A.out + (A.rag ? (size_t)A.rag[b].sq_off : (size_t)b * N * N);
  const double* vb = A.v + (size_t)b * A.nvec * A.m;
  const double* sb = A.s + (size_t)b * A.nsel;

  // the lane's 4 x 4 pairs: unit vectors from a to c.  An atom behind N takes the last one's place; its pairs are not stored
  const int ty = tid >> 4, tx = tid & 15;
  double n[4][4][3], acc[4][4];
  {
    double xa[4][3], xc[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int a = min(a0 + 4 * ty + i, N - 1), c = min(c0 + tx + 16 * i, N - 1);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        xa[i][k] = xb[3 * (size_t)a + k];
        xc[i][k] = xb[3 * (size_t)c + k];
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double dx = xc[j][0] - xa[i][0], dy = xc[j][1] - xa[i][1], dz = xc[j][2] - xa[i][2];
        const double len = sqrt(fma(dz, dz, fma(dy, dy, dx * dx)));
        n[i][j][0] = dx / len;
        n[i][j][1] = dy / len;
        n[i][j][2] = dz / len;
        acc[i][j] = 0.0;
      }
  }

  // the loader lanes: column `tid` of a tile side is component `comp` of its atom `atom`
  const int atom = tid / 3, comp = tid - 3 * atom;
  const bool loader = tid < kSide;
  const bool ok_a = loader && a0 + atom < N, ok_c = loader && c0 + atom < N;
  const double sc_a = (A.scale && ok_a) ? A.scale[atom_off + a0 + atom] : 1.0;
  const double sc_c = (A.scale && ok_c) ? A.scale[atom_off + c0 + atom] : 1.0;
  const int ga = 3 * a0 + tid, gc = 3 * c0 + tid;
  const int slot = comp * kTile + atom;

  double pre[2 * kRows];
  fetch_rows(A, vb, sb, 0, ga, gc, ok_a, ok_c, pre);
  for (int kk0 = 0; kk0 < A.nsel; kk0 += kRows) {
    __syncthreads();   // the previous group has been summed
    if (loader) {
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        lds[(2 * r) * kSide + slot] = pre[2 * r] * sc_a;
        lds[(2 * r + 1) * kSide + slot] = pre[2 * r + 1] * sc_c;
      }
    }
    __syncthreads();
    if (kk0 + kRows < A.nsel) fetch_rows(A, vb, sb, kk0 + kRows, ga, gc, ok_a, ok_c, pre);
#pragma unroll 1
    for (int r = 0; r < kRows; ++r) {
      const int kk = kk0 + r;
      const double sv = kk < A.nsel ? sb[kk] : 0.0;
      if (sv == 0.0) continue;   // (uniform) a row without weight adds nothing, whatever it holds
      const double* la = lds + (2 * r) * kSide + 4 * ty;
      const double* lc = lds + (2 * r + 1) * kSide + tx;
      double ua[4][3], uc[4][3];
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          ua[i][k] = la[k * kTile + i];
          uc[i][k] = lc[k * kTile + 16 * i];
        }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double dx = uc[j][0] - ua[i][0], dy = uc[j][1] - ua[i][1], dz = uc[j][2] - ua[i][2];
          const double p = fma(n[i][j][2], dz, fma(n[i][j][1], dy, n[i][j][0] * dx));
          acc[i][j] = fma(sv * p, p, acc[i][j]);
        }
    }
  }

  const bool diag = ta == tc;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int a = a0 + 4 * ty + i;
    if (a >= N) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + tx + 16 * j;
      if (c >= N) continue;
      if (diag) {
        ob[(size_t)a * N + c] = a == c ? 0.0 : acc[i][j];
      } else {
        ob[(size_t)a * N + c] = acc[i][j];
        ob[(size_t)c * N + a] = acc[i][j];
      }
    }
  }
}

}  // namespace

// dim 3 only (the callers check): d_out (batch, m / 3, m / 3), ragged (sum n_atoms^2) packed
int batch_distfluct_device(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                           const sc_mode_selection& sel, const int64_t* d_counts, const double* d_coord,
                           const double* d_atom_scale, double* d_out, const RaggedView* rv) {
  hipStream_t st = ctx->stream;
  const int64_t nsel = batch_modes_nsel(sel, nvec);
  const int64_t N = rv ? rv->max_atoms : m / 3;   // (bounds the grid)
  if (nsel == 0) {
    SC_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(double) * (rv ? (size_t)rv->total_sq : (size_t)batch * N * N), st));
    return SC_OK;
  }
  SC_TRY(sc_reserve_modes(ctx, batch_modes_workspace_bytes(m, nvec, batch, 3, nsel, 4, 0, rv)));
  double* d_s = reinterpret_cast<double*>(ctx->modes_ws);
  SC_TRY(launch_mode_weights(ctx, d_w, nvec, batch, sel, nsel, d_counts, d_s, rv));
  DistFluctArgs A{};
  A.v = d_v; A.s = d_s; A.coord = d_coord; A.scale = d_atom_scale; A.out = d_out;
  pair_tile::fill_listed_rows(A, sel, nsel, nvec, m, rv);
  const unsigned tiles = pair_tile::tri_tiles(N);
  for (int64_t b0 = 0; b0 < batch; b0 += kMaxSlab) {
    A.b0 = (int)b0;
    hipLaunchKernelGGL(k_dist_fluct, dim3(tiles, (unsigned)std::min(kMaxSlab, batch - b0)), dim3(256), 0, st, A);
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}
