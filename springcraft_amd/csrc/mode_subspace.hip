// Pairwise comparison of the mode subspaces of a batch: RMSIP, covariance overlap and the raw table of mode overlaps.
// No reference counterpart (Bio3D: rmsip / covsoverlap; ProDy: calcSubspaceOverlap / calcCovOverlap / calcOverlap).
//
// Two operand sets (w, v, counts, selection), v (batch, nvec, m) rows = modes, and per (structure, listed row) a weight
// p >= 0, exactly 0.0 for a row that is not selected.  For structures a of the first and b of the second set
//
//   G_ab[i, j] = <v[a, row_a(i), :], v[b, row_b(j), :]>
//   S[a, b]    = sum_i sum_j p[a, i] p[b, j] G_ab[i, j]^2
//   kind 0 (RMSIP):               p = 1,            t = sum_i p,      out = sqrt(S / sqrt(t_a t_b))
//   kind 1 (covariance overlap):  p = 1 / sqrt(w),  t = sum_i 1 / w,  out = 1 - sqrt(max(0, t_a + t_b - 2 S) / (t_a + t_b))   (Hess 2002)
//
// Over all modes of 64 structures of m = 6000 the G_ab are 2080 x 288 MB, so S is reduced where G is accumulated.
// k_mode_subspace is mode_prs.hip transposed: the MFMA's K dimension runs along m, the output tile is (listed rows of a) x
// (listed rows of b).  One workgroup of 256 lanes owns one pair (a, b) and one T x T tile (T = 32 or 64) and walks m in
// chunks of 32 columns: every 32 lanes fetch 32 consecutive doubles of one listed row (8-byte pieces: rows are only
// 8-byte aligned for odd m) while the previous chunk is multiplied, and stage them in LDS times sqrt(p), [side][row][34]:
// the stores of 16 lanes are 16 consecutive doubles, and the 32 lanes of an operand load -- rows r .. r + 15 at columns k,
// k + 1 -- take the doubles 34 r + k, all distinct modulo 32.  Wavefront w owns the NB x NB blocks of 16 x 16 at block row
// NB (w >> 1), block column NB (w & 1); lane l gives A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15] and holds
// D[i = 4 reg + (l >> 4)][j = l & 15] (v_mfma_f64_16x16x4).
//
// An MFMA cannot skip a row, so selection happens at the fetch: a row whose weight is 0.0, a listed row outside
// 0..nvec-1, a row beyond the list and the tail of m are staged as 0.0 and never loaded.  A NaN weight (a listed row that
// was not solved; every row of a failed structure) is staged as NaN on that structure's side alone: NaN * 0 is NaN, so
// every pair with that structure is NaN and no other.
//
// S: the accumulators are squared and summed in the lane, the 256 sums added through LDS in one fixed tree, and one
// partial per (pair, tile) stored; k_subspace_finish adds a pair's partials in tile order and writes out[a, b] -- and, for
// a self-comparison, where only the pairs a >= b are launched, out[b, a] from the same value: the result equals its
// transpose bit for bit.  No atomics, no split along m: an entry's bits depend on the two structures' own (w, v,
// selection), the side each is on and the tile, not on the batch sizes, their positions or their neighbours.  The tile is
// chosen from the number of listed rows alone.  G: the same kernel stores its accumulators instead (weights 1).
//
// Per (pair, row pair, column): one multiply-add on the matrix pipe; a T x T tile reads 2 T doubles per column, 16 / T
// bytes per multiply-add: 0.25 at T = 64.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "eigh_internal.h"
#include "scratch_arena.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kChunk = 32;            // columns of m staged at a time: eight MFMA steps of 4
constexpr int kStride = kChunk + 2;   // doubles of one staged row (the banks: see above)
constexpr int64_t kMaxSlab = 32768;   // grid.y carries the pairs of a slab

struct SubSide {
  const double* v;   // (batch, nvec, m)
  const double* q;   // (batch, nsel): sqrt(p)
  const int* rows;   // null: listed row kk is row row0 + kk
  int row0, nsel, nvec, batch;
};

struct SubArgs {
  SubSide a, b;
  const int* pairs;   // pair mode 2: (n_pairs, 2)
  double* part;       // S: (pairs of the slab, tiles)
  double* gram;       // G: (n_pairs, a.nsel, b.nsel)
  int m, pair_mode, p0, tiles_j;
};

// pair p -> structures (sa, sb).  0: the triangle sa >= sb of one set, rows first; 1: the rectangle, row-major; 2: the list
__device__ __forceinline__ void pair_decode(int pair_mode, const int* __restrict__ pairs, int batch_b, int p, int& sa,
                                            int& sb) {
  if (pair_mode == 0) {
    tri_tile_decode(p, sa, sb);
  } else if (pair_mode == 1) {
    sa = p / batch_b;
    sb = p - sa * batch_b;
  } else {
    sa = pairs[2 * p];
    sb = pairs[2 * p + 1];
  }
}

// the L listed rows kk0 + rg + 8 u of structure s a loader lane fetches from: where each starts (null: not read) and its sqrt(p)
template <int L>
__device__ __forceinline__ void loader_rows(const SubSide& S, int s, int kk0, int rg, int m, const double* (&ptr)[L],
                                            double (&q)[L]) {
#pragma unroll
  for (int u = 0; u < L; ++u) {
    const int kk = kk0 + rg + 8 * u;
    const double qv = kk < S.nsel ? S.q[(size_t)s * S.nsel + kk] : 0.0;
    q[u] = qv;
    ptr[u] = nullptr;
    if (qv != 0.0 && qv == qv) {
      const int row = min(max(S.rows ? S.rows[kk] : S.row0 + kk, 0), S.nvec - 1);
      ptr[u] = S.v + ((size_t)s * S.nvec + row) * m;
    }
  }
}

// grid (tiles of (listed rows of a) x (listed rows of b), pairs of the slab)
template <int NB, bool GRAM>
__global__ __launch_bounds__(256) void k_mode_subspace(const SubArgs A) {
  constexpr int T = 32 * NB;   // rows per side of a tile
  constexpr int L = T / 8;     // rows per side a loader lane fetches from
  __shared__ double lds[2 * T * kStride];
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const int p = A.p0 + blockIdx.y;
  int sa, sb;
  pair_decode(A.pair_mode, A.pairs, A.b.batch, p, sa, sb);
  const int ti = blockIdx.x / A.tiles_j, tj = blockIdx.x - ti * A.tiles_j;
  const int i0 = ti * T, j0 = tj * T;
  const int m = A.m;

  // the MFMA lanes
  const int w = tid >> 6, fr = tid & 15, fk = (tid >> 4) & 3;
  const int rb = 16 * NB * (w >> 1), cb = 16 * NB * (w & 1);
  if (GRAM && (sa < 0 || sa >= A.a.batch || sb < 0 || sb >= A.b.batch)) {   // (the whole workgroup) a pair that names no structure
#pragma unroll
    for (int x = 0; x < NB; ++x)
#pragma unroll
      for (int y = 0; y < NB; ++y)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + rb + 16 * x + 4 * r + fk, j = j0 + cb + 16 * y + fr;
          if (i < A.a.nsel && j < A.b.nsel) A.gram[((size_t)p * A.a.nsel + i) * A.b.nsel + j] = NAN;
        }
    return;
  }

  // the loader lanes: 32 lanes along the columns of a chunk, eight groups of them across the rows of both sides
  const int c = tid & 31, rg = tid >> 5;
  const double *pa[L], *pb[L];
  double qa[L], qb[L];
  loader_rows<L>(A.a, sa, i0, rg, m, pa, qa);
  loader_rows<L>(A.b, sb, j0, rg, m, pb, qb);
  double* sta = lds + rg * kStride + c;
  double* stb = lds + (T + rg) * kStride + c;
  const double* la = lds + (rb + fr) * kStride + fk;
  const double* lb = lds + (T + cb + fr) * kStride + fk;

  d4 acc[NB][NB];
#pragma unroll
  for (int x = 0; x < NB; ++x)
#pragma unroll
    for (int y = 0; y < NB; ++y) acc[x][y] = d4{0.0, 0.0, 0.0, 0.0};

  double prea[L], preb[L];
  auto fetch = [&](int c0) {
    const bool ok = c0 + c < m;
#pragma unroll
    for (int u = 0; u < L; ++u) {
      prea[u] = (pa[u] && ok) ? pa[u][c0 + c] : 0.0;
      preb[u] = (pb[u] && ok) ? pb[u][c0 + c] : 0.0;
    }
  };
  fetch(0);
  for (int c0 = 0; c0 < m; c0 += kChunk) {
    __syncthreads();   // the previous chunk has been multiplied
    const bool ok = c0 + c < m;
#pragma unroll
    for (int u = 0; u < L; ++u) {
      // a row that is not read is its weight, 0.0 or NaN; the tail of m is 0.0
      sta[8 * u * kStride] = !pa[u] ? qa[u] : (ok ? prea[u] * qa[u] : 0.0);
      stb[8 * u * kStride] = !pb[u] ? qb[u] : (ok ? preb[u] * qb[u] : 0.0);
    }
    __syncthreads();
    if (c0 + kChunk < m) fetch(c0 + kChunk);
#pragma unroll
    for (int ks = 0; ks < kChunk / 4; ++ks) {
      if (c0 + 4 * ks >= m) break;   // (uniform) a step of nothing but the tail
      double af[NB], bf[NB];
#pragma unroll
      for (int x = 0; x < NB; ++x) af[x] = la[16 * x * kStride + 4 * ks];
#pragma unroll
      for (int y = 0; y < NB; ++y) bf[y] = lb[16 * y * kStride + 4 * ks];
#pragma unroll
      for (int x = 0; x < NB; ++x)
#pragma unroll
        for (int y = 0; y < NB; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[x], bf[y], acc[x][y], 0, 0, 0);
    }
  }

  if (GRAM) {
#pragma unroll
    for (int x = 0; x < NB; ++x)
#pragma unroll
      for (int y = 0; y < NB; ++y)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + rb + 16 * x + 4 * r + fk, j = j0 + cb + 16 * y + fr;
          if (i < A.a.nsel && j < A.b.nsel) A.gram[((size_t)p * A.a.nsel + i) * A.b.nsel + j] = acc[x][y][r];
        }
    return;
  }
  // rows and columns beyond the lists were staged as zeros and add exactly nothing
  double ss = 0.0;
#pragma unroll
  for (int x = 0; x < NB; ++x)
#pragma unroll
    for (int y = 0; y < NB; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r) ss = fma(acc[x][y][r], acc[x][y][r], ss);
  red[tid] = ss;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) A.part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

// s (batch, nsel): in, k_mode_weights' 1 / w of a selected row, 0.0 or NaN; out, sqrt(p).  kind 1: p = sqrt(1 / w) (a
// selected row with w < 0: NaN) and t[b] = sum of 1 / w = sum of p^2, the trace of the covariance; else p = 1 for a
// selected row and t[b] = sum of p.  The sum is taken in one fixed order given by nsel.
__global__ __launch_bounds__(256) void k_subspace_weights(double* __restrict__ s, int nsel, int kind, double* __restrict__ t) {
  __shared__ double red[256];
  const int b = blockIdx.x;
  double* sb = s + (size_t)b * nsel;
  double acc = 0.0;
  for (int kk = threadIdx.x; kk < nsel; kk += 256) {
    const double sv = sb[kk];
    double tv, qv;
    if (kind == 1) {
      tv = sv;
      qv = sqrt(sqrt(sv));
    } else {
      tv = qv = (sv != 0.0 && sv == sv) ? 1.0 : sv;
    }
    sb[kk] = qv;
    acc += tv;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) t[b] = red[0];
}

// one lane per pair of the slab: its tile partials added in tile order, then the public quantity
__global__ __launch_bounds__(256) void k_subspace_finish(const double* __restrict__ part, int tiles, int pair_mode, int p0,
                                                         int count, int batch_b, const double* __restrict__ ta,
                                                         const double* __restrict__ tb, int kind, double* __restrict__ out,
                                                         double* __restrict__ s_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  int sa, sb;
  pair_decode(pair_mode, nullptr, batch_b, p0 + i, sa, sb);
  double S = 0.0;
  for (int t = 0; t < tiles; ++t) S += part[(size_t)i * tiles + t];
  const double Ta = ta[sa], Tb = tb[sb];
  double val;
  if (kind == 1) {
    double d = Ta + Tb - 2.0 * S;
    d = d < 0.0 ? 0.0 : d;   // (a NaN stays)
    val = 1.0 - sqrt(d / (Ta + Tb));
  } else {
    val = sqrt(S / sqrt(Ta * Tb));
  }
  out[(size_t)sa * batch_b + sb] = val;
  if (s_out) s_out[(size_t)sa * batch_b + sb] = S;
  if (pair_mode == 0 && sa != sb) {
    out[(size_t)sb * batch_b + sa] = val;
    if (s_out) s_out[(size_t)sb * batch_b + sa] = S;
  }
}

// rows per side of a tile, from the numbers of listed rows alone (profiles/subspace.txt); SPRINGCRAFT_SUBSPACE_TILE = 32 or
// 64 overrides it for measurements (read once)
int subspace_tile(int64_t nsel_a, int64_t nsel_b) {
  static const int forced = [] {
    const char* e = getenv("SPRINGCRAFT_SUBSPACE_TILE");
    const int x = e ? atoi(e) : 0;
    return (x == 32 || x == 64) ? x : 0;
  }();
  if (forced) return forced;
  return std::max(nsel_a, nsel_b) <= 32 ? 32 : 64;
}

struct SubLayout {
  double *q_a = nullptr, *q_b = nullptr, *t_a = nullptr, *t_b = nullptr, *part = nullptr;
};

// weights and t of each set (one set for a self-comparison) and the tile partials of a slab of pairs
void sub_layout(sc_host::Arena& ar, const SubspaceSet& a, int64_t nsel_a, const SubspaceSet* b, int64_t nsel_b,
                int64_t slab, int64_t tiles, bool gram, SubLayout& out) {
  out.q_a = ar.take<double>((size_t)a.batch * std::max<int64_t>(nsel_a, 1));
  out.t_a = ar.take<double>((size_t)a.batch);
  out.q_b = out.q_a;
  out.t_b = out.t_a;
  if (b) {
    out.q_b = ar.take<double>((size_t)b->batch * std::max<int64_t>(nsel_b, 1));
    out.t_b = ar.take<double>((size_t)b->batch);
  }
  if (!gram) out.part = ar.take<double>((size_t)slab * tiles);
}

}  // namespace

int modes_subspace_device(sc_ctx* ctx, const SubspaceSet& a, const SubspaceSet* b, int64_t m, int kind,
                          const int32_t* d_pairs, int64_t n_pairs, double* d_out, double* d_s, double* d_t_a,
                          double* d_t_b) {
  hipStream_t st = ctx->stream;
  const bool gram = kind == 2;
  const SubspaceSet& bb = b ? *b : a;
  const int64_t nsel_a = batch_modes_nsel(*a.sel, a.nvec), nsel_b = batch_modes_nsel(*bb.sel, bb.nvec);
  const int pair_mode = gram ? 2 : (b ? 1 : 0);
  const int64_t pairs = gram ? n_pairs : (b ? a.batch * bb.batch : a.batch * (a.batch + 1) / 2);
  const int T = subspace_tile(nsel_a, nsel_b);
  const int64_t tiles_i = (nsel_a + T - 1) / T, tiles_j = (nsel_b + T - 1) / T, tiles = tiles_i * tiles_j;
  if (pairs > INT32_MAX || tiles > INT32_MAX)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%lld pairs of %lld tiles", (long long)pairs, (long long)tiles);
  // the partials of a slab take at most the consumers' budget; the slab does not enter any sum
  const int64_t slab = std::max<int64_t>(
      1, std::min<int64_t>(std::min<int64_t>(kMaxSlab, std::max<int64_t>(pairs, 1)),
                           (int64_t)(modes_budget_default() / (size_t)std::max<int64_t>(8 * tiles, 8))));
  sc_host::Arena measure;
  SubLayout lay;
  sub_layout(measure, a, nsel_a, b, nsel_b, slab, tiles, gram, lay);
  SC_TRY(sc_reserve_modes(ctx, measure.bytes()));
  sc_host::Arena carve(ctx->modes_ws, ctx->modes_ws_bytes);
  sub_layout(carve, a, nsel_a, b, nsel_b, slab, tiles, gram, lay);
  if (carve.overrun()) return sc_set_error(ctx, SC_ERR_NOMEM, "workspace layout overran its measure");

  const int wkind = kind == 1 ? 1 : 0;
  if (nsel_a > 0) SC_TRY(launch_mode_weights(ctx, a.d_w, a.nvec, a.batch, *a.sel, nsel_a, a.d_counts, lay.q_a, nullptr));
  hipLaunchKernelGGL(k_subspace_weights, dim3((unsigned)a.batch), dim3(256), 0, st, lay.q_a, (int)nsel_a, wkind, lay.t_a);
  if (b) {
    if (nsel_b > 0) SC_TRY(launch_mode_weights(ctx, bb.d_w, bb.nvec, bb.batch, *bb.sel, nsel_b, bb.d_counts, lay.q_b, nullptr));
    hipLaunchKernelGGL(k_subspace_weights, dim3((unsigned)bb.batch), dim3(256), 0, st, lay.q_b, (int)nsel_b, wkind, lay.t_b);
  }
  SC_HIP(ctx, hipGetLastError());
  if (d_t_a) SC_HIP(ctx, hipMemcpyAsync(d_t_a, lay.t_a, (size_t)a.batch * 8, hipMemcpyDeviceToDevice, st));
  if (d_t_b) SC_HIP(ctx, hipMemcpyAsync(d_t_b, lay.t_b, (size_t)bb.batch * 8, hipMemcpyDeviceToDevice, st));
  if (pairs == 0 || (gram && tiles == 0)) return SC_OK;

  SubArgs A{};
  auto side = [&](const SubspaceSet& s, const double* q, int64_t nsel) {
    SubSide o{};
    o.v = s.d_v; o.q = q;
    o.rows = s.sel->kind == SC_SEL_ROWS ? s.sel->d_rows : nullptr;
    o.row0 = s.sel->kind == SC_SEL_FROM_ROW ? (int)s.sel->row0 : 0;
    o.nsel = (int)nsel; o.nvec = (int)s.nvec; o.batch = (int)s.batch;
    return o;
  };
  A.a = side(a, lay.q_a, nsel_a);
  A.b = side(bb, lay.q_b, nsel_b);
  A.pairs = d_pairs; A.part = lay.part; A.gram = gram ? d_out : nullptr;
  A.m = (int)m; A.pair_mode = pair_mode; A.tiles_j = (int)std::max<int64_t>(tiles_j, 1);
  for (int64_t p0 = 0; p0 < pairs; p0 += slab) {
    const unsigned np = (unsigned)std::min(slab, pairs - p0);
    A.p0 = (int)p0;
    if (tiles > 0) {
      auto kern = gram ? (T == 32 ? k_mode_subspace<1, true> : k_mode_subspace<2, true>)
                       : (T == 32 ? k_mode_subspace<1, false> : k_mode_subspace<2, false>);
      hipLaunchKernelGGL(kern, dim3((unsigned)tiles, np), dim3(256), 0, st, A);
    }
    if (!gram)
      hipLaunchKernelGGL(k_subspace_finish, dim3((np + 255) / 256), dim3(256), 0, st, lay.part, (int)tiles, pair_mode,
                         (int)p0, (int)np, (int)bb.batch, lay.t_a, lay.t_b, wkind, d_out, d_s);
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}
