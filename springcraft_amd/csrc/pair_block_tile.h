// The 64 x 64 pair-block core of the f64 matrix pipe: every 3 x 3 block  B_ac[d, e] = sum_k X[k][a][d] * Y[k][c][e]  of a
// 64 x 64 tile of pairs (a, c), the nine entries of one block in one lane.  Its kernels: k_mode_prs (mode_prs.hip) and
// k_mode_lmi (mode_lmi.hip), where k runs over the listed rows of a structure's modes and (a, c) are atoms.  Each keeps its
// own epilogue on the blocks; the tile, the LDS layout, the lane mapping and the MFMA step are here.  k_rmsd_product
// (rmsd_matrix.hip), where k runs over the atoms and (a, c) are frames, has the same core in a copy of its own: on these
// functions the compiler numbers its registers differently and it takes 1.3 % longer (profiles/pair_block_tile.txt).
//
// One workgroup of 512 lanes owns the tile and walks k in ascending order, kRows at a time; 2 x 192 loader lanes fetch the
// 3 x 64 doubles of the tile's two sides of each k while the previous group is multiplied, and put them into LDS
// component-major, [k][side][component][index].  With that layout a 16 x 16 x 4 MFMA is "component d of 16 indices a
// times component e of 16 indices c, summed over 4 k": lane l gives A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l &
// 15] and holds D[i = 4 reg + (l >> 4)][j = l & 15].  Wavefront w owns the 16 indices 16 (w & 3) .. of the a side and two
// blocks of 16 of the c side, 32 (w >> 2) ..: 2 x 9 accumulators (144 registers: four blocks would not leave room for the
// operands), and the nine entries of one B_ac sit in the same lane and register slot of nine of them, so an epilogue needs
// no LDS round trip and no shuffle.
//
// The mode kernels (mode_blocks): B_ac = sum_r s[b, r] u_r[a] u_r[c]^T, the covariance block of two atoms over the listed
// rows, u_r[a] = scale[b, a] (null: 1) times V[b, r, 3 a .. 3 a + 2] (8-byte pieces: rows are only 8-byte aligned for odd
// N); the a side is staged times weight and scale, the c side times scale.  An MFMA cannot skip a row, so selection
// happens at the fetch: a row whose weight is 0.0, a listed row outside 0..nvec-1, the tail that rounds a group up to
// kRows rows and a column behind the structure's own 3 N are staged as 0.0 and never loaded -- 0 * NaN from a window
// solve's padding cannot reach a result.  A NaN weight (a listed row that was not solved; every row of a failed structure,
// 1 / NaN) is staged as NaN on the a side of all its atoms: NaN * 0 is NaN, so that structure's result is NaN, and no
// other's.  The weight is folded into the a side alone, so the blocks (a, c) and (c, a) may round differently: a kernel
// that wants a symmetric result has only tiles with tile_a >= tile_c, stores both places from one register, and takes a
// diagonal tile's a >= c lanes only.
//
// Per (pair, k): 9 multiply-adds = 18 flops on the matrix pipe; a tile reads 2 x 192 doubles of a k for its 4096 pairs,
// 0.75 bytes per (pair, k) from memory and the same again into LDS.
#pragma once
#include <algorithm>

#include "eigh_internal.h"
#include "ensemble_policy.h"
#include "host_logic.h"

namespace pair_tile {

constexpr int kTile = 64;                     // indices per side of a tile: 4 blocks of 16
constexpr int kRows = 8;                      // k staged in LDS at a time: two MFMA steps of 4
constexpr int kSide = 3 * kTile;              // doubles of one side of one k
// one staged k: the a side, the c side and 16 doubles more, so that the four k one MFMA operand load touches start in
// alternating halves of the LDS banks (2 kSide doubles are a multiple of the 256-byte bank row)
constexpr int kRowStride = 2 * kSide + 16;
constexpr int kLdsDoubles = kRows * kRowStride;
constexpr int64_t kMaxSlab = 32768;           // grid.y carries the structures of a slab
static_assert(kTile == sc_host::kRmsdTile && kRows == sc_host::kRmsdRows, "the host pads the RMSD operands to this tile");
static_assert(kTile == 64 && kRows % 4 == 0, "the lane mapping is written for 64 x 64 tiles and MFMA steps of 4");

// "the listed rows of a batch member" and the place of its pair matrix: what a pair consumer's kernel reads its rows
// through and writes to (also dist_fluct.hip)
struct ListedRows {
  const double* v;          // (batch, nvec, m)
  const double* s;          // (batch, nsel) weights of k_mode_weights
  const int* rows;          // null: listed row kk is row row0 + kk
  const double* scale;      // null, or (batch, N); ragged: packed
  const RaggedRec* rag;     // null: uniform batch
  double* out;              // (batch, N, N); ragged: packed at sq_off
  int row0, nsel, nvec, m, b0;
};
// everything of A that follows from the selection and the shapes; v, s, scale, out and, per slab, b0 are the launcher's
inline void fill_listed_rows(ListedRows& A, const sc_mode_selection& sel, int64_t nsel, int64_t nvec, int64_t m,
                             const RaggedView* rv) {
  A.rows = sel.kind == SC_SEL_ROWS ? sel.d_rows : nullptr;
  A.row0 = sel.kind == SC_SEL_FROM_ROW ? (int)sel.row0 : 0;
  A.rag = rv ? rv->d_rec : nullptr;
  A.nsel = (int)nsel; A.nvec = (int)nvec; A.m = (int)m;
}
// workgroups of one structure of at most N atoms: the tiles with tile_a >= tile_c (tri_tile_decode)
inline unsigned tri_tiles(int64_t N) { return (unsigned)sc_host::tri_tile_count(N, kTile); }

#ifdef __HIPCC__
typedef double d4 __attribute__((ext_vector_type(4)));

// the MFMA lanes: wavefront w, lane (fr, fk) supplies index 16 ab + fr of the a side and index 16 (cb0 + j) + fr of the c
// side, both of k = fk of a step, read from la / lc
struct Lanes {
  int fr, fk, ab, cb0;
  const double* la;
  const double* lc;
};
__device__ __forceinline__ Lanes lanes(const double* lds, int tid) {
  Lanes L;
  const int w = tid >> 6;
  L.fr = tid & 15; L.fk = (tid >> 4) & 3;
  L.ab = w & 3; L.cb0 = 2 * (w >> 2);
  L.la = lds + L.fk * kRowStride + 16 * L.ab + L.fr;
  L.lc = lds + L.fk * kRowStride + kSide + 16 * L.cb0 + L.fr;
  return L;
}

__device__ __forceinline__ void zero(d4 (&acc)[2][3][3]) {
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
      for (int e = 0; e < 3; ++e) acc[j][d][e] = d4{0.0, 0.0, 0.0, 0.0};
}

// the four staged k from 4 k4 on: 3 + 6 operand loads, 18 MFMAs
__device__ __forceinline__ void mfma_step(const Lanes& L, int k4, d4 (&acc)[2][3][3]) {
  double af[3], bf[2][3];
#pragma unroll
  for (int d = 0; d < 3; ++d) af[d] = L.la[4 * k4 * kRowStride + d * kTile];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int e = 0; e < 3; ++e) bf[j][e] = L.lc[4 * k4 * kRowStride + e * kTile + 16 * j];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
      for (int e = 0; e < 3; ++e)
        acc[j][d][e] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[d], bf[j][e], acc[j][d][e], 0, 0, 0);
}

// The lane's eight pairs, the c side outer: at_c(c) once per index c = 16 (cb0 + j) + fr of the c side, then
// at_pair(a, c, block) for its four a = 16 ab + 4 r + fk, both local to the tile, block[d][e] the pair's B_ac.
template <class AtC, class AtPair>
__device__ __forceinline__ void for_pairs(const Lanes& L, const d4 (&acc)[2][3][3], AtC&& at_c, AtPair&& at_pair) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = 16 * (L.cb0 + j) + L.fr;
    at_c(c);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double block[3][3];
#pragma unroll
      for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int e = 0; e < 3; ++e) block[d][e] = acc[j][d][e][r];
      at_pair(16 * L.ab + 4 * r + L.fk, c, block);
    }
  }
}

// the kRows values a loader lane fetches of the group of listed rows from kk0 on: its column `g` of every row that carries
// a weight (ok: the column is the structure's own); on the a side a NaN weight takes the place of the row, which is not read
__device__ __forceinline__ void fetch_rows(const ListedRows& A, const double* __restrict__ vb,
                                           const double* __restrict__ sb, int kk0, int g, bool ok, bool a_side,
                                           double (&pre)[kRows]) {
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int kk = kk0 + r;
    const double sv = kk < A.nsel ? sb[kk] : 0.0;   // (uniform over the workgroup)
    pre[r] = (sv != sv && a_side) ? sv : 0.0;
    if (sv != 0.0 && sv == sv && ok) {
      const int row = min(max(A.rows ? A.rows[kk] : A.row0 + kk, 0), A.nvec - 1);
      pre[r] = vb[(size_t)row * A.m + g];
    }
  }
}

// acc <- the covariance blocks of the tile of atoms (a0 .., c0 ..) of structure b (N atoms, its scale at atom_off) over the
// listed rows; the whole workgroup calls it.  kScaled = false: A.scale is null and no factor is staged
template <bool kScaled>
__device__ __forceinline__ void mode_blocks(const ListedRows& A, double* lds, const Lanes& L, int b, int N,
                                            size_t atom_off, int a0, int c0, d4 (&acc)[2][3][3]) {
  const int tid = threadIdx.x;
  const double* vb = A.v + (size_t)b * A.nvec * A.m;
  const double* sb = A.s + (size_t)b * A.nsel;
  // the loader lanes: lanes 0..191 take the a side, 192..383 the c side; column `col` of a side is component `comp` of its
  // atom `atom`
  const bool loader = tid < 2 * kSide, a_side = tid < kSide;
  const int col = a_side ? tid : tid - kSide;
  const int atom = col / 3, comp = col - 3 * atom;
  const int s0 = a_side ? a0 : c0;
  const bool ok = loader && s0 + atom < N;
  const double sc = (kScaled && A.scale && ok) ? A.scale[atom_off + s0 + atom] : 1.0;
  const int g = 3 * s0 + col;
  const int slot = (a_side ? 0 : kSide) + comp * kTile + atom;

  zero(acc);
  double pre[kRows];
  fetch_rows(A, vb, sb, 0, g, ok, a_side, pre);
  for (int kk0 = 0; kk0 < A.nsel; kk0 += kRows) {
    __syncthreads();   // the previous group has been multiplied
    if (loader) {
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        const int kk = kk0 + r;
        const double sv = (a_side && kk < A.nsel) ? sb[kk] : 1.0;   // (the weight is folded into the a side alone)
        lds[r * kRowStride + slot] = kScaled ? pre[r] * (sv * sc) : pre[r] * sv;
      }
    }
    __syncthreads();
    if (kk0 + kRows < A.nsel) fetch_rows(A, vb, sb, kk0 + kRows, g, ok, a_side, pre);
#pragma unroll
    for (int k4 = 0; k4 < kRows / 4; ++k4) {
      if (kk0 + 4 * k4 >= A.nsel) break;   // (uniform) a step of nothing but the tail
      mfma_step(L, k4, acc);
    }
  }
}
#endif  // __HIPCC__

}  // namespace pair_tile
