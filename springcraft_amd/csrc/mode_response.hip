// Displacement fields built from the modes, on the tensors the solvers leave in HBM: the linear response to a force and
// the linear combination of modes underneath it.
//
// Reference: nma.py:422-473 linear_response = covariance @ force, for one model and through the (3N, 3N) pseudo-inverse.
// Here no covariance is formed.  v (batch, nvec, m) rows = modes, m = dim N; s_a an optional per-atom scale (1 / sqrt(mass)
// behind a mass-weighted solve); wt the weights of k_mode_weights, 1 / lambda for a selected row and exactly 0.0 for any
// other.  Two streaming passes over the listed rows of v, per group of four forces:
//
//   project   c[b, j, r] = <v_r, g_j> wt[b, r],   g_j[dim a + d] = s_a f_j[dim a + d]
//   combine   X[b, j, dim a + d] = s_a sum_r c[b, j, r] v[b, r, dim a + d]
//
// With s = 1 and the pinv rule that is pinv(H) f; the combine pass alone, on coefficients the caller chose, is what ProDy
// calls deformAtoms / traverseMode / sampleModes, and the inverse of the overlaps of mode_overlap.hip.
//
// k_modes_project sums ALONG a row, with the lane-to-atom map and the fixed butterfly of k_modes_overlap: one wavefront per
// two rows, lane l owns the atoms 128 i + 2 l and 128 i + 2 l + 1 and adds them in ascending order, the 64 lane sums are
// added at distance 32, 16, ..., 1.  The order is a function of (N, dim) alone and every force has its own chain.  A row
// whose weight is exactly 0.0 -- outside the selection, behind a window's count, a ragged slot's pad row -- is not read and
// its coefficient is 0.0 (selected, not multiplied); a listed row that was not solved has weight NaN, is not read either,
// and gets NaN.  No atomics, no LDS.
//
// k_modes_combine_partial sums ACROSS rows, as k_bmsf_partial does: grid (column tiles of 512, row chunks, structures of the
// slab), lanes along the coordinate axis, up to four sums per owned column (one per force of the group), the chunk's
// listed rows in ascending order with fma.  The chunk length is msf_chunk's, from the number of listed rows alone, and
// k_modes_combine_reduce adds the chunks in ascending order and applies s_a: a structure's bits do not depend on the batch
// size, its position, its neighbours or q.  Ragged: only a structure's own columns are read and written, force and result
// packed at dim * atom_off with vector j at stride dim * sum n, the layout of mode_overlap.hip's displacement.
//
// Both passes are bandwidth-bound: each reads the listed rows once per group of four forces, nsel m 8 bytes per structure.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "eigh_internal.h"

namespace {

constexpr int kWaveRows = 2;                         // rows a wavefront carries side by side
constexpr int kBlockRows = 4 * kWaveRows;            // 256 threads
constexpr int kQGroup = 4;                           // forces per pass
constexpr int64_t kMaxSlab = 32768;                  // a grid axis carries the structures of a slab

struct ProjectArgs {
  const double* v;            // (batch, nvec, m)
  const double* wt;           // (batch, nsel) weights of the listed rows
  const double* force;        // vector j of structure b at force + b * force_b + j * force_j (ragged: + dim * atom_off)
  const double* scale;        // null, or (batch, N); ragged: packed at atom_off
  const int* rows;            // null: listed row kk is row row0 + kk of v; else row rows[kk]
  const RaggedRec* rag;       // null: uniform batch
  double* coef;               // (batch, kQGroup, nsel): coefficient of force j0 + j at slot j
  long long force_b, force_j;
  int m, nvec, nsel, row0, j0, b0;
};

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// the 2 DIM doubles of a lane's two atoms: columns c0 .. c0 + DIM - 1 and c1 .. c1 + DIM - 1 (VEC: c1 = c0 + DIM, c0 even)
template <int DIM, bool VEC>
__device__ __forceinline__ void load_atoms(const double* __restrict__ p, int c0, int c1, double (&x)[2 * DIM]) {
  if (VEC) {
    const double2* p2 = reinterpret_cast<const double2*>(p + c0);
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      const double2 t = p2[c];
      x[2 * c] = t.x; x[2 * c + 1] = t.y;
    }
  } else {
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      x[c] = p[c0 + c];
      x[DIM + c] = p[c1 + c];
    }
  }
}

// acc + <x, y> over the DIM components of one atom, in component order
template <int DIM>
__device__ __forceinline__ double dot_atom(const double* x, const double* y, double acc) {
#pragma unroll
  for (int c = 0; c < DIM; ++c) acc = fma(x[c], y[c], acc);
  return acc;
}

// grid (groups of kBlockRows listed rows, structures of the slab); a wavefront per kWaveRows listed rows.
template <int DIM, bool VEC, int NQ, bool SCALE>
__global__ __launch_bounds__(256) void k_modes_project(const ProjectArgs A) {
  const int lane = threadIdx.x & 63;
  const int kk0 = ((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * kWaveRows;
  if (kk0 >= A.nsel) return;   // (the whole wavefront)
  const int b = A.b0 + blockIdx.y;
  const int N = A.rag ? A.rag[b].n_atoms : A.m / DIM;
  const double* wb = A.wt + (size_t)b * A.nsel;
  // (everything about the rows is uniform over the wavefront)
  int row[kWaveRows];
  double s[kWaveRows];
  bool ok[kWaveRows];
#pragma unroll
  for (int u = 0; u < kWaveRows; ++u) {
    const int kk = kk0 + u;
    const bool listed = kk < A.nsel;
    row[u] = listed ? (A.rows ? A.rows[kk] : A.row0 + kk) : -1;
    s[u] = listed ? wb[kk] : 0.0;
    // weight 0.0: not selected; a row outside 0..nvec-1 carries NaN (k_mode_weights) and is not read either
    ok[u] = listed && s[u] != 0.0 && row[u] >= 0 && row[u] < A.nvec;
  }
  double dot[kWaveRows][NQ];
#pragma unroll
  for (int u = 0; u < kWaveRows; ++u)
#pragma unroll
    for (int j = 0; j < NQ; ++j) dot[u][j] = 0.0;

  if (ok[0] || ok[1]) {
    // a row that is not read: its place in the pair is taken by the other row, its sums are dropped
    const double* vb = A.v + (size_t)b * A.nvec * A.m;
    const double* vr[kWaveRows] = {vb + (size_t)(ok[0] ? row[0] : row[1]) * A.m,
                                   vb + (size_t)(ok[1] ? row[1] : row[0]) * A.m};
    const double* fb = A.force + (A.rag ? (long long)DIM * A.rag[b].atom_off : (long long)b * A.force_b);
    const double* fj[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) fj[j] = fb + (long long)(A.j0 + j) * A.force_j;
    const double* sc = SCALE ? A.scale + (A.rag ? (size_t)A.rag[b].atom_off : (size_t)b * N) : nullptr;

    for (int a0 = 2 * lane; a0 < N; a0 += 128) {
      const bool two = VEC || a0 + 1 < N;   // (VEC: N is even)
      const int a1 = two ? a0 + 1 : a0;
      const int c0 = a0 * DIM;
      const int c1 = a1 * DIM;
      double x[kWaveRows][2 * DIM], g[NQ][2 * DIM];
#pragma unroll
      for (int u = 0; u < kWaveRows; ++u) load_atoms<DIM, VEC>(vr[u], c0, c1, x[u]);
#pragma unroll
      for (int j = 0; j < NQ; ++j) load_atoms<DIM, VEC>(fj[j], c0, c1, g[j]);
      if (SCALE) {
        const double s0 = sc[a0], s1 = sc[a1];
#pragma unroll
        for (int j = 0; j < NQ; ++j)
#pragma unroll
          for (int c = 0; c < DIM; ++c) {
            g[j][c] *= s0;
            g[j][DIM + c] *= s1;
          }
      }
#pragma unroll
      for (int u = 0; u < kWaveRows; ++u)
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
          const double t0 = dot_atom<DIM>(x[u], g[j], dot[u][j]), t1 = dot_atom<DIM>(x[u] + DIM, g[j] + DIM, t0);
          dot[u][j] = two ? t1 : t0;
        }
    }
    // every lane takes part, also one without atoms (a row shorter than a wavefront): its sums are 0
#pragma unroll
    for (int u = 0; u < kWaveRows; ++u)
#pragma unroll
      for (int j = 0; j < NQ; ++j) dot[u][j] = wave_sum(dot[u][j]);
  }
  if (lane != 0) return;
#pragma unroll
  for (int u = 0; u < kWaveRows; ++u) {
    const int kk = kk0 + u;
    if (kk >= A.nsel) continue;
#pragma unroll
    for (int j = 0; j < NQ; ++j)
      A.coef[((size_t)b * kQGroup + j) * A.nsel + kk] = ok[u] ? dot[u][j] * s[u] : (s[u] == 0.0 ? 0.0 : NAN);
  }
}

using ProjectKernel = void (*)(const ProjectArgs);

template <int DIM, bool VEC, bool SCALE>
ProjectKernel project_kernel(int nq) {
  switch (nq) {
    case 1: return k_modes_project<DIM, VEC, 1, SCALE>;
    case 2: return k_modes_project<DIM, VEC, 2, SCALE>;
    case 3: return k_modes_project<DIM, VEC, 3, SCALE>;
    default: return k_modes_project<DIM, VEC, 4, SCALE>;
  }
}

template <int DIM>
ProjectKernel project_kernel(bool vec, bool scale, int nq) {
  return vec ? (scale ? project_kernel<DIM, true, true>(nq) : project_kernel<DIM, true, false>(nq))
             : (scale ? project_kernel<DIM, false, true>(nq) : project_kernel<DIM, false, false>(nq));
}

// ---- combine -----------------------------------------------------------------------------------------------------
struct CombineArgs {
  const double* v;            // (batch, nvec, m)
  const double* coef;         // coefficient of (structure b, vector j0 + j, listed row kk) at coef + b * coef_b + j * coef_j + kk
  const double* wt;           // null: every listed row counts; else (batch, nsel): a row with weight 0.0 is selected out
  const int* rows;            // null: listed row kk is row row0 + kk of v; else row rows[kk]
  const long long* counts;    // null, or (batch) rows that exist behind a window solve
  const RaggedRec* rag;       // null: uniform batch
  double* part;               // (structures of the slab, chunks, nq, m)
  long long coef_b, coef_j;
  int m, nvec, nsel, row0, chunk, b0, first_row;
};

// rows of structure b that exist: all nvec, the window's min(counts[b], nvec), a ragged slot's own - first_row
__device__ __forceinline__ int rows_limit(const long long* __restrict__ counts, int b, int nvec,
                                          const RaggedRec* __restrict__ rag, int first_row) {
  int lim = nvec;
  if (counts) {
    const long long c = counts[b];
    lim = c < 0 ? 0 : (c < nvec ? (int)c : nvec);
  }
  if (rag) lim = max(min(lim, rag[b].own - first_row), 0);
  return lim;
}

// U listed rows from kk on: all coefficients, weights and row pointers first, then all loads, then the sums in row order
template <bool VEC, bool LIST, bool WT, int NQ, int U>
__device__ __forceinline__ void combine_rows(const CombineArgs& A, const double* __restrict__ vb,
                                             const double* __restrict__ cb, const double* __restrict__ wb, int kk, int j0,
                                             int j1c, double (&acc)[NQ][2]) {
  double c[U][NQ], x0[U], x1[U];
  bool use[U];
  const double* p[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int j = 0; j < NQ; ++j) c[u][j] = cb[(long long)j * A.coef_j + kk + u];
    use[u] = WT ? wb[kk + u] != 0.0 : true;
    const int r = LIST ? A.rows[kk + u] : A.row0 + kk + u;
    p[u] = vb + (size_t)min(max(r, 0), A.nvec - 1) * A.m;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (VEC) {
      const double2 x = *reinterpret_cast<const double2*>(p[u] + j0);
      x0[u] = x.x; x1[u] = x.y;
    } else {
      x0[u] = p[u][j0]; x1[u] = p[u][j1c];
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const double t0 = fma(c[u][j], x0[u], acc[j][0]), t1 = fma(c[u][j], x1[u], acc[j][1]);
      acc[j][0] = use[u] ? t0 : acc[j][0];
      acc[j][1] = use[u] ? t1 : acc[j][1];
    }
}

// part[bz, c, j, col] = sum over the listed rows kk of chunk c, in order, of coef[b, j0 + j, kk] V[b, row(kk), col].
// Column ownership as k_bmsf_partial: VEC (m even, v 16-byte aligned) columns (2t, 2t + 1) of the tile as one 16-byte
// piece, otherwise columns t and t + 256 as 8-byte pieces.
template <bool VEC, bool LIST, bool WT, int NQ>
__global__ __launch_bounds__(256) void k_modes_combine_partial(const CombineArgs A) {
  const int b = A.b0 + blockIdx.z;
  const int c = blockIdx.y;
  // ragged: the structure's own columns; a tile wholly behind them returns here, before its first load, and the lanes
  // of the tile that straddles them mask their tail (VEC: the 16-byte load may take one pad column, which is dropped)
  const int mo = A.rag ? A.rag[b].own : A.m;
  if ((int)blockIdx.x * 512 >= mo) return;
  const int k0 = c * A.chunk;
  int k1 = min(k0 + A.chunk, A.nsel);
  // without a list the rows ascend: those behind the window's count (and a slot's pad rows) are not read, and neither
  // are their coefficients
  if (!LIST) k1 = min(k1, rows_limit(A.counts, b, A.nvec, A.rag, A.first_row) - A.row0);
  const int j0 = VEC ? (blockIdx.x * 256 + threadIdx.x) * 2 : blockIdx.x * 512 + threadIdx.x;
  const int j1 = VEC ? j0 + 1 : j0 + 256;
  if (j0 >= mo) return;
  const bool has1 = j1 < mo;
  const int j1c = has1 ? j1 : j0;
  const double* vb = A.v + (size_t)b * A.nvec * A.m;
  const double* cb = A.coef + (long long)b * A.coef_b;
  const double* wb = WT ? A.wt + (size_t)b * A.nsel : nullptr;
  double acc[NQ][2];
#pragma unroll
  for (int j = 0; j < NQ; ++j) acc[j][0] = acc[j][1] = 0.0;
  int kk = k0;
  for (; kk + 4 <= k1; kk += 4) combine_rows<VEC, LIST, WT, NQ, 4>(A, vb, cb, wb, kk, j0, j1c, acc);
  for (; kk < k1; ++kk) combine_rows<VEC, LIST, WT, NQ, 1>(A, vb, cb, wb, kk, j0, j1c, acc);
  double* pp = A.part + ((size_t)blockIdx.z * gridDim.y + c) * NQ * A.m;
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    pp[(size_t)j * A.m + j0] = acc[j][0];
    if (has1) pp[(size_t)j * A.m + j1] = acc[j][1];
  }
}

// out[b, j0 + j, col] = s_a times the sum over the chunks in ascending order, a = col / dim.  grid (column tiles of 256,
// vectors of the group, structures of the slab); vector j of structure b at out + b * out_b + j * out_j (ragged: + dim *
// atom_off), the scale as in ProjectArgs.
__global__ __launch_bounds__(256) void k_modes_combine_reduce(const double* __restrict__ part, int nchunk, int nq, int m,
                                                              int dim, int b0, int j0, const double* __restrict__ scale,
                                                              double* __restrict__ out, long long out_b, long long out_j,
                                                              const RaggedRec* __restrict__ rag) {
  const int b = b0 + blockIdx.z;
  const int j = blockIdx.y;
  const int mo = rag ? rag[b].own : m;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= mo) return;
  const double* pb = part + ((size_t)blockIdx.z * nchunk * nq + j) * m + col;
  double acc = 0.0;
  for (int c = 0; c < nchunk; ++c) acc += pb[(size_t)c * nq * m];
  if (scale) acc *= scale[(rag ? (size_t)rag[b].atom_off : (size_t)b * (m / dim)) + col / dim];
  out[(rag ? (long long)dim * rag[b].atom_off : (long long)b * out_b) + (long long)(j0 + j) * out_j + col] = acc;
}

using CombineKernel = void (*)(const CombineArgs);

template <bool VEC, bool LIST, bool WT>
CombineKernel combine_kernel(int nq) {
  switch (nq) {
    case 1: return k_modes_combine_partial<VEC, LIST, WT, 1>;
    case 2: return k_modes_combine_partial<VEC, LIST, WT, 2>;
    case 3: return k_modes_combine_partial<VEC, LIST, WT, 3>;
    default: return k_modes_combine_partial<VEC, LIST, WT, 4>;
  }
}

CombineKernel combine_kernel(bool vec, bool list, bool wt, int nq) {
  if (vec) {
    if (list) return wt ? combine_kernel<true, true, true>(nq) : combine_kernel<true, true, false>(nq);
    return wt ? combine_kernel<true, false, true>(nq) : combine_kernel<true, false, false>(nq);
  }
  if (list) return wt ? combine_kernel<false, true, true>(nq) : combine_kernel<false, true, false>(nq);
  return wt ? combine_kernel<false, false, true>(nq) : combine_kernel<false, false, false>(nq);
}

int nchunks(int64_t nsel) { return (int)((nsel + msf_chunk(nsel) - 1) / msf_chunk(nsel)); }

// four partial sums per column and chunk where the msf keeps one
int64_t combine_slab(int64_t m, int64_t nsel, int64_t batch, size_t budget) {
  const size_t per = (size_t)nchunks(nsel) * kQGroup * m * 8;
  const int64_t slab = std::min<int64_t>(kMaxSlab, (int64_t)std::max<size_t>(1, budget / std::max<size_t>(per, 1)));
  return std::min(slab, std::max<int64_t>(batch, 1));
}

// where vector j of structure b lies in a (batch, q, m) tensor / a ragged (q, dim * sum n) packed buffer
struct VecLayout {
  long long b, j;
};
VecLayout vec_layout(int64_t m, int64_t q, int dim, const RaggedView* rv) {
  return rv ? VecLayout{0, (long long)dim * rv->total_atoms} : VecLayout{(long long)q * m, (long long)m};
}

// One group of nq <= 4 vectors: partial sums and their reduction, slab by slab.  A.coef / coef_b / coef_j, A.wt, A.rows,
// A.row0, A.nsel are set; d_out is the whole result, of which vectors j0 .. j0 + nq - 1 are written.
int launch_combine_group(sc_ctx* ctx, CombineArgs A, int64_t batch, int dim, int nq, int j0, int64_t q, size_t budget,
                         const double* d_scale, double* d_part, double* d_out, const RaggedView* rv) {
  const int nchunk = nchunks(A.nsel);
  const int64_t slab = combine_slab(A.m, A.nsel, batch, budget);
  const bool vec = A.m % 2 == 0 && reinterpret_cast<uintptr_t>(A.v) % 16 == 0;
  const int64_t mo = rv ? (int64_t)dim * rv->max_atoms : A.m;   // (bounds the grid of the reduce)
  const VecLayout lo = vec_layout(A.m, q, dim, rv);
  const CombineKernel kern = combine_kernel(vec, A.rows != nullptr, A.wt != nullptr, nq);
  A.part = d_part;
  for (int64_t b0 = 0; b0 < batch; b0 += slab) {
    const unsigned nb = (unsigned)std::min(slab, batch - b0);
    A.b0 = (int)b0;
    hipLaunchKernelGGL(kern, dim3((unsigned)((A.m + 511) / 512), (unsigned)nchunk, nb), dim3(256), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_modes_combine_reduce, dim3((unsigned)((mo + 255) / 256), (unsigned)nq, nb), dim3(256), 0,
                       ctx->stream, d_part, nchunk, nq, A.m, dim, (int)b0, j0, d_scale, d_out, lo.b, lo.j, A.rag);
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

size_t out_elems(int64_t m, int64_t batch, int dim, int64_t q, const RaggedView* rv) {
  return (size_t)q * (rv ? (size_t)dim * rv->total_atoms : (size_t)batch * m);
}

}  // namespace

// what = 5: coefficients of one group of forces (batch, 4, nsel) | partial sums of one slab; what = 6: the partial sums
size_t modes_response_workspace_bytes(int64_t m, int64_t batch, int64_t nsel, int what, size_t budget) {
  if (budget == 0) budget = modes_budget_default();
  const int64_t ns = std::max<int64_t>(nsel, 1);
  size_t bytes = align_up((size_t)combine_slab(m, ns, batch, budget) * nchunks(ns) * kQGroup * m * 8, 256);
  if (what == 5) bytes += align_up((size_t)batch * kQGroup * ns * 8, 256);
  return bytes;
}

int modes_response_device(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                          int dim, const sc_mode_selection& sel, const int64_t* d_counts, const double* d_force, int64_t q,
                          const double* d_atom_scale, size_t budget, double* d_out, const RaggedView* rv) {
  if (q == 0) return SC_OK;
  if (budget == 0) budget = modes_budget_default();
  const int64_t nsel = batch_modes_nsel(sel, nvec);
  if (nsel == 0) {
    SC_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(double) * out_elems(m, batch, dim, q, rv), ctx->stream));
    return SC_OK;
  }
  SC_TRY(sc_reserve_modes(ctx, batch_modes_workspace_bytes(m, nvec, batch, dim, nsel, 5, budget, rv)));
  char* base = (char*)ctx->modes_ws;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base + off; off += align_up(bytes, 256); return reinterpret_cast<double*>(p); };
  double* d_s = take((size_t)batch * nsel * 8);
  double* d_coef = take((size_t)batch * kQGroup * nsel * 8);
  double* d_part = take(0);
  SC_TRY(launch_mode_weights(ctx, d_w, nvec, batch, sel, nsel, d_counts, d_s, rv));

  const VecLayout lo = vec_layout(m, q, dim, rv);
  ProjectArgs P{};
  P.v = d_v; P.wt = d_s; P.force = d_force; P.scale = d_atom_scale; P.coef = d_coef;
  P.rows = sel.kind == SC_SEL_ROWS ? sel.d_rows : nullptr;
  P.row0 = sel.kind == SC_SEL_FROM_ROW ? (int)sel.row0 : 0;
  P.rag = rv ? rv->d_rec : nullptr;
  P.force_b = lo.b; P.force_j = lo.j;
  P.m = (int)m; P.nvec = (int)nvec; P.nsel = (int)nsel;
  CombineArgs A{};
  A.v = d_v; A.coef = d_coef; A.wt = d_s; A.rows = P.rows; A.row0 = P.row0;
  A.counts = reinterpret_cast<const long long*>(d_counts);
  A.rag = P.rag;
  A.coef_b = (long long)kQGroup * nsel; A.coef_j = nsel;
  A.m = (int)m; A.nvec = (int)nvec; A.nsel = (int)nsel; A.chunk = msf_chunk(nsel);
  A.first_row = rv ? rv->first_row : 0;

  const bool pvec = !rv && m % 2 == 0 && reinterpret_cast<uintptr_t>(d_v) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(d_force) % 16 == 0;
  const unsigned gx = (unsigned)((nsel + kBlockRows - 1) / kBlockRows);
  for (int64_t j0 = 0; j0 < q; j0 += kQGroup) {
    const int nq = (int)std::min<int64_t>(kQGroup, q - j0);
    const ProjectKernel kern = dim == 3 ? project_kernel<3>(pvec, d_atom_scale != nullptr, nq)
                                        : project_kernel<1>(pvec, d_atom_scale != nullptr, nq);
    P.j0 = (int)j0;
    for (int64_t b0 = 0; b0 < batch; b0 += kMaxSlab) {
      P.b0 = (int)b0;
      hipLaunchKernelGGL(kern, dim3(gx, (unsigned)std::min(kMaxSlab, batch - b0)), dim3(256), 0, ctx->stream, P);
    }
    SC_TRY(launch_combine_group(ctx, A, batch, dim, nq, (int)j0, q, budget, d_atom_scale, d_part, d_out, rv));
  }
  return SC_OK;
}

int modes_combine_device(sc_ctx* ctx, const double* d_v, int64_t m, int64_t nvec, int64_t batch, int dim,
                         const int* d_rows, int64_t nsel, const double* d_coef, int64_t q, const int64_t* d_counts,
                         const double* d_atom_scale, size_t budget, double* d_out, const RaggedView* rv) {
  if (q == 0) return SC_OK;
  if (budget == 0) budget = modes_budget_default();
  if (nsel == 0) {
    SC_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(double) * out_elems(m, batch, dim, q, rv), ctx->stream));
    return SC_OK;
  }
  SC_TRY(sc_reserve_modes(ctx, batch_modes_workspace_bytes(m, nvec, batch, dim, nsel, 6, budget, rv)));
  CombineArgs A{};
  A.v = d_v; A.rows = d_rows;
  A.counts = reinterpret_cast<const long long*>(d_counts);
  A.rag = rv ? rv->d_rec : nullptr;
  A.coef_b = (long long)q * nsel; A.coef_j = nsel;
  A.m = (int)m; A.nvec = (int)nvec; A.nsel = (int)nsel; A.chunk = msf_chunk(nsel);
  A.first_row = rv ? rv->first_row : 0;
  for (int64_t j0 = 0; j0 < q; j0 += kQGroup) {
    const int nq = (int)std::min<int64_t>(kQGroup, q - j0);
    A.coef = d_coef + j0 * nsel;
    SC_TRY(launch_combine_group(ctx, A, batch, dim, nq, (int)j0, q, budget, d_atom_scale,
                                reinterpret_cast<double*>(ctx->modes_ws), d_out, rv));
  }
  return SC_OK;
}
