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
// Data flow as in dist_fluct.hip: one workgroup, here of 512 lanes, owns a 64 x 64 tile of atom pairs of one structure and
// walks the listed rows in order, kRows at a time; 2 x 192 lanes fetch the 3 x 64 consecutive doubles of the tile's two
// atom sets from each row (8-byte pieces: rows are only 8-byte aligned for odd N) while the previous group is multiplied,
// and put them into LDS component-major, [row][side][component][atom]: the a side times weight and scale, the c side
// times scale.  The arithmetic runs on the f64 matrix pipe.  With that layout a 16 x 16 x 4 MFMA is "component d of 16
// atoms a times component e of 16 atoms c, summed over 4 rows": lane l gives A[i = l & 15][k = l >> 4] and B[k = l >> 4]
// [j = l & 15] and holds D[i = 4 reg + (l >> 4)][j = l & 15].  Wavefront w owns the 16 atoms a0 + 16 (w & 3) .. and two
// blocks of 16 atoms c, 32 (w >> 2) ..: 2 x 9 accumulators (144 registers: four blocks would not leave room for the
// operands), and the nine entries of one C_ac sit in the same lane and register slot of nine of them.  The sum of squares
// is taken there, in one fixed (d, e) order, with no LDS round trip and no shuffle.
//
// An MFMA cannot skip a row, so selection happens at the fetch: a row whose weight is 0.0, a listed row outside
// 0..nvec-1, the tail that rounds a group up to kRows rows and a column behind the structure's own 3 N are staged as 0.0
// and never loaded -- 0 * NaN from a window solve's padding cannot reach a result.  A NaN weight (a listed row that was not
// solved; every row of a failed structure, 1 / NaN) is staged as NaN on the a side of all its atoms: NaN * 0 is NaN, so
// that structure's result is NaN, and no other's.
//
// Only tiles with tile_a >= tile_c exist; they store P[a, c] and P[c, a] from the same register (a diagonal tile from its
// a >= c lanes only: the weight is folded into the a side, so the (c, a) lane may round differently), and the unnormalised
// matrix equals its transpose bit for bit.  No atomics, no partial sums across workgroups: a structure's bits depend on
// its own w, v, scale and the selection only.  norm: the diagonal is copied to the workspace, then row a is divided by
// it in a second small launch; an empty selection gives zeros, and 0 / 0 = NaN under norm as in NumPy.
// Ragged batches: N, the scale (at atom_off) and the result (at sq_off) are the structure's own, m is the slot order; pad
// rows carry no weight, pad columns are never read.
//
// Per (pair, row): 9 multiply-adds = 18 flops on the matrix pipe; a tile reads 2 x 192 doubles of a row for its 4096
// pairs, 0.75 bytes per (pair, row) from memory and the same again into LDS.
#include <algorithm>
#include <cmath>

#include "eigh_internal.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 64;                     // atoms per side of a tile: 4 blocks of 16
constexpr int kRows = 8;                      // listed rows staged in LDS at a time: two MFMA steps of 4
constexpr int kSide = 3 * kTile;              // doubles of one atom set of one row
// one staged row: the a side, the c side and 16 doubles more, so that the four rows one MFMA operand load touches start
// in alternating halves of the LDS banks (2 kSide doubles are a multiple of the 256-byte bank row)
constexpr int kRowStride = 2 * kSide + 16;
constexpr int64_t kMaxSlab = 32768;           // grid.y carries the structures of a slab

struct PrsArgs {
  const double* v;          // (batch, nvec, m)
  const double* s;          // (batch, nsel) weights
  const int* rows;          // null: listed row kk is row row0 + kk
  const double* scale;      // null, or (batch, N); ragged: packed
  const RaggedRec* rag;     // null: uniform batch
  double* out;              // (batch, N, N); ragged: packed at sq_off
  int row0, nsel, nvec, m, b0;
};

// the kRows values a loader lane fetches of the group of listed rows from kk0 on: its column `g` of every row that carries
// a weight (ok: the column is the structure's own); on the a side a NaN weight takes the place of the row, which is not read
__device__ __forceinline__ void fetch_rows(const PrsArgs& A, const double* __restrict__ vb, const double* __restrict__ sb,
                                           int kk0, int g, bool ok, bool a_side, double (&pre)[kRows]) {
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

// grid (tiles with tile_a >= tile_c, structures of the slab)
__global__ __launch_bounds__(512) void k_mode_prs(const PrsArgs A) {
  __shared__ double lds[kRows * kRowStride];
  const int tid = threadIdx.x;
  int ta, tc;
  tri_tile_decode(blockIdx.x, ta, tc);
  const int b = A.b0 + blockIdx.y;
  const int N = A.rag ? A.rag[b].n_atoms : A.m / 3;
  const int a0 = ta * kTile, c0 = tc * kTile;   // c0 <= a0
  if (a0 >= N) return;                          // (the whole workgroup: a ragged structure smaller than the grid)
  const size_t atom_off = A.rag ? (size_t)A.rag[b].atom_off : (size_t)b * N;
  double* ob = A.out + (A.rag ? (size_t)A.rag[b].sq_off : (size_t)b * N * N);
  const double* vb = A.v + (size_t)b * A.nvec * A.m;
  const double* sb = A.s + (size_t)b * A.nsel;

  // the loader lanes: lanes 0..191 take the a side, 192..383 the c side; column `col` of a side is component `comp` of its
  // atom `atom`
  const bool loader = tid < 2 * kSide, a_side = tid < kSide;
  const int col = a_side ? tid : tid - kSide;
  const int atom = col / 3, comp = col - 3 * atom;
  const int s0 = a_side ? a0 : c0;
  const bool ok = loader && s0 + atom < N;
  const double sc = (A.scale && ok) ? A.scale[atom_off + s0 + atom] : 1.0;
  const int g = 3 * s0 + col;
  const int slot = (a_side ? 0 : kSide) + comp * kTile + atom;

  // the MFMA lanes: wavefront w, lane (fr, fk) supplies atom 16 ab + fr of the a side and atom 16 (cb0 + j) + fr of the c
  // side, both of row fk of a step
  const int w = tid >> 6, fr = tid & 15, fk = (tid >> 4) & 3;
  const int ab = w & 3, cb0 = 2 * (w >> 2);
  const double* la = lds + fk * kRowStride + 16 * ab + fr;
  const double* lc = lds + fk * kRowStride + kSide + 16 * cb0 + fr;
  d4 acc[2][3][3];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
      for (int e = 0; e < 3; ++e) acc[j][d][e] = d4{0.0, 0.0, 0.0, 0.0};

  double pre[kRows];
  fetch_rows(A, vb, sb, 0, g, ok, a_side, pre);
  for (int kk0 = 0; kk0 < A.nsel; kk0 += kRows) {
    __syncthreads();   // the previous group has been multiplied
    if (loader) {
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        const int kk = kk0 + r;
        const double sv = (a_side && kk < A.nsel) ? sb[kk] : 1.0;   // (the weight is folded into the a side alone)
        lds[r * kRowStride + slot] = pre[r] * (sv * sc);
      }
    }
    __syncthreads();
    if (kk0 + kRows < A.nsel) fetch_rows(A, vb, sb, kk0 + kRows, g, ok, a_side, pre);
#pragma unroll
    for (int k4 = 0; k4 < kRows / 4; ++k4) {
      if (kk0 + 4 * k4 >= A.nsel) break;   // (uniform) a step of nothing but the tail
      double af[3], bf[2][3];
#pragma unroll
      for (int d = 0; d < 3; ++d) af[d] = la[4 * k4 * kRowStride + d * kTile];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 3; ++e) bf[j][e] = lc[4 * k4 * kRowStride + e * kTile + 16 * j];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
          for (int e = 0; e < 3; ++e)
            acc[j][d][e] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[d], bf[j][e], acc[j][d][e], 0, 0, 0);
    }
  }

  const bool diag = ta == tc;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = c0 + 16 * (cb0 + j) + fr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = a0 + 16 * ab + 4 * r + fk;
      double p = 0.0;
#pragma unroll
      for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int e = 0; e < 3; ++e) p = fma(acc[j][d][e][r], acc[j][d][e][r], p);
      if (a >= N || c >= N || (diag && a < c)) continue;
      ob[(size_t)a * N + c] = p;
      if (a != c) ob[(size_t)c * N + a] = p;
    }
  }
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
  const RaggedRec* rag = rv ? rv->d_rec : nullptr;
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
  A.rows = sel.kind == SC_SEL_ROWS ? sel.d_rows : nullptr;
  A.row0 = sel.kind == SC_SEL_FROM_ROW ? (int)sel.row0 : 0;
  A.rag = rag;
  A.nsel = (int)nsel; A.nvec = (int)nvec; A.m = (int)m;
  const int64_t T = (N + kTile - 1) / kTile;
  const unsigned tiles = (unsigned)(T * (T + 1) / 2);
  const unsigned strips = (unsigned)((N + 255) / 256);
  for (int64_t b0 = 0; b0 < batch; b0 += kMaxSlab) {
    const unsigned nb = (unsigned)std::min(kMaxSlab, batch - b0);
    A.b0 = (int)b0;
    if (nsel > 0) hipLaunchKernelGGL(k_mode_prs, dim3(tiles, nb), dim3(512), 0, st, A);
    if (norm) {
      hipLaunchKernelGGL(k_prs_diag, dim3(strips, nb), dim3(256), 0, st, d_out, (int)N, d_diag, rag, (int)b0);
      hipLaunchKernelGGL(k_prs_norm, dim3(strips, (unsigned)N, nb), dim3(256), 0, st, d_out, d_diag, (int)N, rag, (int)b0);
    }
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}
