// Overlaps of the modes with displacement vectors, and the modes' collectivities, on the tensors the solvers leave in HBM.
//
// No reference counterpart (ProDy: calcOverlap / calcCollectivity, Bio3D: overlap).  v (batch, nvec, m) rows = modes,
// m = dim N; a displacement d_j has the length and the coordinates of a row (mass-weighted solve: the caller passes
// sqrt(mass) d).  For every row r of every structure b, in ONE pass over v:
//
//   O[b, j, r] = <v_r, d_j> / (|v_r| |d_j|)                      signed; a zero row or a zero d_j gives 0 / 0 = NaN
//   kappa[b, r] = exp(-sum_a p_a ln p_a) / N,  p_a = s_a / S,  s_a = sum_{c < dim} v_r[dim a + c]^2,  S = sum_a s_a
//               = exp(ln S - (sum_a s_a ln s_a) / S) / N         the one-pass form; a term with s_a = 0 is exactly 0
//
// The other batch consumers (batch_consumers.hip) sum over rows and write per atom; this one sums ALONG a row and writes
// per row.  One wavefront takes two rows at a time; lane l owns the atoms 128 i + 2 l and 128 i + 2 l + 1 (i = 0, 1, ...)
// of both, so the three components of an atom meet in one lane, and adds its atoms in ascending order; the 64 lane sums
// are added by a fixed butterfly (lanes at distance 32, 16, ..., 1).  That order is a function of (N, dim) alone -- N =
// m / dim, in a ragged batch the structure's own atom count -- and every quantity (S, sum s ln s, each <v, d_j>, each
// |d_j|^2) has its own chain, so a row's results do not depend, bit for bit, on the batch size, the structure's position,
// its neighbours, the row it shares a wavefront with, q, or the vectors that accompany d_j.  No atomics, no LDS, no
// workspace: |d_j|^2 is summed by every wavefront from the values it loads anyway (in the same order, hence to the same
// bits).  The displacement vectors are read q / 4 times per two rows and come from L1 / L2 (48 kB per vector at m = 6000;
// the workgroups of one structure are neighbours in the grid).
//
// VEC (m even, v and d 16-byte aligned, uniform batch): a lane's two atoms are 2 dim consecutive doubles at an even
// column, loaded as dim 16-byte pieces.  Otherwise (m = 3 N is odd for odd N: rows are only 8-byte aligned; ragged: the
// packed displacement starts anywhere) the same atoms come as 2 dim 8-byte pieces, and the last atom of an odd N has no
// partner: its lane reads it twice and drops the second sum.  The lane-to-atom map, and so the bits, are the same.
//
// q is taken in groups of four vectors (template NQ: the sums stay in registers); the collectivity comes from the first
// group only, and a vector's chain is the same in every group.  Rows without a meaning -- behind a window's count, a
// ragged slot's pad rows, beyond a listed row's range -- are NaN in both outputs and their v is never read.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace {

constexpr int kWaveRows = 2;                         // rows a wavefront carries side by side
constexpr int kBlockRows = 4 * kWaveRows;            // 256 threads
constexpr int kQGroup = 4;                           // displacement vectors per pass
constexpr int64_t kMaxSlab = 32768;                  // grid.y carries the structures of a slab

struct OverlapArgs {
  const double* v;            // (batch, nvec, m)
  const double* disp;         // vector j of structure b at disp + b * disp_b + j * disp_j (ragged: + dim * atom_off)
  const int* rows;            // null: output row kk is row kk of v; else row rows[kk] (one model's mode list)
  const long long* counts;    // null, or (batch) rows that exist behind a window solve
  const RaggedRec* rag;       // null: uniform batch
  double* overlap;            // (batch, q, nout)
  double* coll;               // (batch, nout)
  long long disp_b, disp_j;
  int m, nvec, nout, q, j0, b0, first_row;
};

// x ln x with the limit 0 at x = 0 (selected, not multiplied: ln 0 = -inf never reaches the sum); NaN stays NaN
__device__ __forceinline__ double xlogx(double x) { return x == 0.0 ? 0.0 : x * log(x); }

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

// grid (groups of kBlockRows output rows, structures of the slab); a wavefront per kWaveRows rows.
template <int DIM, bool VEC, int NQ, bool COLL>
__global__ __launch_bounds__(256) void k_modes_overlap(const OverlapArgs A) {
  constexpr int NQ1 = NQ > 0 ? NQ : 1;
  const int lane = threadIdx.x & 63;
  const int kk0 = ((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * kWaveRows;
  if (kk0 >= A.nout) return;   // (the whole wavefront)
  const int b = A.b0 + blockIdx.y;
  const int N = A.rag ? A.rag[b].n_atoms : A.m / DIM;
  // rows of v that exist: all nvec, the window's min(counts[b], nvec), a ragged slot's own - first_row
  int lim = A.nvec;
  if (A.counts) {
    const long long c = A.counts[b];
    lim = c < 0 ? 0 : (c < A.nvec ? (int)c : A.nvec);
  }
  if (A.rag) lim = max(min(lim, A.rag[b].own - A.first_row), 0);
  // (everything about the rows is uniform over the wavefront)
  int row[kWaveRows];
  bool ok[kWaveRows];
#pragma unroll
  for (int u = 0; u < kWaveRows; ++u) {
    const int kk = kk0 + u;
    row[u] = kk < A.nout ? (A.rows ? A.rows[kk] : kk) : -1;
    ok[u] = row[u] >= 0 && row[u] < lim;
  }
  double S[kWaveRows], E[kWaveRows], dot[kWaveRows][NQ1], dd[NQ1];
#pragma unroll
  for (int u = 0; u < kWaveRows; ++u) {
    S[u] = 0.0; E[u] = 0.0;
#pragma unroll
    for (int j = 0; j < NQ1; ++j) dot[u][j] = 0.0;
  }
#pragma unroll
  for (int j = 0; j < NQ1; ++j) dd[j] = 0.0;

  if (ok[0] || ok[1]) {
    // a row without a meaning is not read: its place in the pair is taken by the other row, its sums are dropped
    const double* vb = A.v + (size_t)b * A.nvec * A.m;
    const double* vr[kWaveRows] = {vb + (size_t)(ok[0] ? row[0] : row[1]) * A.m,
                                   vb + (size_t)(ok[1] ? row[1] : row[0]) * A.m};
    const double* dj[NQ1];
    const double* db =
        NQ > 0 ? A.disp + (A.rag ? (long long)DIM * A.rag[b].atom_off : (long long)b * A.disp_b) : nullptr;
#pragma unroll
    for (int j = 0; j < NQ1; ++j) dj[j] = NQ > 0 ? db + (long long)(A.j0 + j) * A.disp_j : nullptr;

    for (int a0 = 2 * lane; a0 < N; a0 += 128) {
      const bool two = VEC || a0 + 1 < N;   // (VEC: N is even)
      const int c0 = a0 * DIM;
      const int c1 = two ? c0 + DIM : c0;
      double x[kWaveRows][2 * DIM], d[NQ1][2 * DIM];
#pragma unroll
      for (int u = 0; u < kWaveRows; ++u) load_atoms<DIM, VEC>(vr[u], c0, c1, x[u]);
      if (NQ > 0) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) load_atoms<DIM, VEC>(dj[j], c0, c1, d[j]);
      }
#pragma unroll
      for (int u = 0; u < kWaveRows; ++u) {
        const double s0 = dot_atom<DIM>(x[u], x[u], 0.0), s1 = dot_atom<DIM>(x[u] + DIM, x[u] + DIM, 0.0);
        const double S0 = S[u] + s0, S1 = S0 + s1;
        S[u] = two ? S1 : S0;
        if (COLL) {
          const double E0 = E[u] + xlogx(s0), E1 = E0 + xlogx(s1);
          E[u] = two ? E1 : E0;
        }
        if (NQ > 0) {
#pragma unroll
          for (int j = 0; j < NQ; ++j) {
            const double t0 = dot_atom<DIM>(x[u], d[j], dot[u][j]), t1 = dot_atom<DIM>(x[u] + DIM, d[j] + DIM, t0);
            dot[u][j] = two ? t1 : t0;
          }
        }
      }
      if (NQ > 0) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
          const double t0 = dot_atom<DIM>(d[j], d[j], dd[j]), t1 = dot_atom<DIM>(d[j] + DIM, d[j] + DIM, t0);
          dd[j] = two ? t1 : t0;
        }
      }
    }
    // every lane takes part, also one without atoms (a row shorter than a wavefront): its sums are 0
#pragma unroll
    for (int u = 0; u < kWaveRows; ++u) {
      S[u] = wave_sum(S[u]);
      if (COLL) E[u] = wave_sum(E[u]);
      if (NQ > 0) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) dot[u][j] = wave_sum(dot[u][j]);
      }
    }
    if (NQ > 0) {
#pragma unroll
      for (int j = 0; j < NQ; ++j) dd[j] = wave_sum(dd[j]);
    }
  }
  if (lane != 0) return;
#pragma unroll
  for (int u = 0; u < kWaveRows; ++u) {
    const int kk = kk0 + u;
    if (kk >= A.nout) continue;
    if (COLL) A.coll[(size_t)b * A.nout + kk] = ok[u] ? exp(log(S[u]) - E[u] / S[u]) / (double)N : NAN;
    if (NQ > 0) {
      const double nv = sqrt(S[u]);
#pragma unroll
      for (int j = 0; j < NQ; ++j)
        A.overlap[((size_t)b * A.q + A.j0 + j) * A.nout + kk] = ok[u] ? dot[u][j] / (nv * sqrt(dd[j])) : NAN;
    }
  }
}

using OverlapKernel = void (*)(const OverlapArgs);

template <int DIM, bool VEC>
OverlapKernel overlap_kernel(int nq, bool coll) {
  switch (nq) {
    case 0: return k_modes_overlap<DIM, VEC, 0, true>;
    case 1: return coll ? k_modes_overlap<DIM, VEC, 1, true> : k_modes_overlap<DIM, VEC, 1, false>;
    case 2: return coll ? k_modes_overlap<DIM, VEC, 2, true> : k_modes_overlap<DIM, VEC, 2, false>;
    case 3: return coll ? k_modes_overlap<DIM, VEC, 3, true> : k_modes_overlap<DIM, VEC, 3, false>;
    default: return coll ? k_modes_overlap<DIM, VEC, 4, true> : k_modes_overlap<DIM, VEC, 4, false>;
  }
}

}  // namespace

int modes_overlap_device(sc_ctx* ctx, const double* d_v, int64_t m, int64_t nvec, int64_t batch, int dim,
                         const int* d_rows, int64_t nout, const double* d_disp, int64_t q, const int64_t* d_counts,
                         double* d_overlap, double* d_coll, const RaggedView* rv) {
  if (nout == 0 || (q == 0 && !d_coll)) return SC_OK;
  OverlapArgs A{};
  A.v = d_v; A.disp = d_disp; A.rows = d_rows;
  A.counts = reinterpret_cast<const long long*>(d_counts);
  A.rag = rv ? rv->d_rec : nullptr;
  A.overlap = d_overlap; A.coll = d_coll;
  A.disp_b = rv ? 0 : (long long)q * m;
  A.disp_j = rv ? (long long)dim * rv->total_atoms : (long long)m;
  A.m = (int)m; A.nvec = (int)nvec; A.nout = (int)nout; A.q = (int)q;
  A.first_row = rv ? rv->first_row : 0;
  const bool vec = !rv && m % 2 == 0 && reinterpret_cast<uintptr_t>(d_v) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(d_disp) % 16 == 0;
  const unsigned gx = (unsigned)((nout + kBlockRows - 1) / kBlockRows);
  for (int64_t b0 = 0; b0 < batch; b0 += kMaxSlab) {
    const unsigned nb = (unsigned)std::min(kMaxSlab, batch - b0);
    A.b0 = (int)b0;
    for (int64_t j0 = 0; j0 == 0 || j0 < q; j0 += kQGroup) {
      const int nq = (int)std::min<int64_t>(kQGroup, q - j0);
      const bool coll = j0 == 0 && d_coll != nullptr;   // the collectivity: from the first group only
      A.j0 = (int)j0;
      const OverlapKernel kern = dim == 3 ? (vec ? overlap_kernel<3, true>(nq, coll) : overlap_kernel<3, false>(nq, coll))
                                          : (vec ? overlap_kernel<1, true>(nq, coll) : overlap_kernel<1, false>(nq, coll));
      hipLaunchKernelGGL(kern, dim3(gx, nb), dim3(256), 0, ctx->stream, A);
    }
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}
