// Mode-subset consumers for a BATCH of structures, on the tensors the batched solvers leave in HBM.
//
// The reference derives these from nma.eigen for one model (nma.py:108-184 msf, :233-359 dcc).  Here the inputs are the
// batch solver's own w (batch, nvec), v (batch, nvec, m) rows = modes and, behind a window solve, counts (batch): at the
// benchmarked shape v is 18 GB that nobody wants to move or copy.  One model's device-resident eigenpairs (sc_modes_*,
// api_modes.hip) come through here as a batch of one with a row list.
//
// One idea carries every selection: k_mode_weights turns (w, selection, counts) into a weight per (structure, listed
// row), 1 / lambda for a selected row and exactly 0.0 for any other, and then
//
//   msf[b, a]    = sum_r  s[b, r] * sum_d V[b, r, dim a + d]^2
//   dcc[b, a, c] = sum_r  s[b, r] * sum_d V[b, r, dim a + d] V[b, r, dim c + d]
//   U[b, a, d, e] = sum_r  s[b, r] * V[b, r, 3 a + d] V[b, r, 3 a + e]        (ANM: the anisotropic fluctuation tensors)
//
// A row without weight is never multiplied in (the kernels select, they do not multiply by zero), so the NaN / zero
// padding behind a window's rows cannot reach a result.  No atomics: every sum is a fixed sequence.
//
// Ragged batches (sc_batch_plan): every kernel takes an optional table of RaggedRec, one per structure.  Without it the
// batch is uniform and nothing differs from the above.  With it m is the common slot order, structure b owns the first
// rag[b].own rows and columns of its slot -- pad rows never carry a weight, pad columns are never packed or summed -- and
// the results go to packed buffers at rag[b].atom_off (msf, diagonals; six values per atom for the tensors) and
// rag[b].sq_off (dcc).
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "common.h"
#include "gemm_f64.h"

namespace {

// bytes the msf partial sums / the packed dcc operands may take at a time (SPRINGCRAFT_MODES_BUDGET_BYTES, read once)
constexpr size_t kModesBudgetBytes = (size_t)1 << 30;
// grid.z carries the structures of a slab
constexpr int64_t kMaxSlab = 32768;

// rows of structure b that may carry a weight: all nvec, or the window's min(counts[b], nvec); in a ragged batch no more
// than the own - first_row rows that are the structure's modes (first_row: global index of row 0)
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

// s[b, kk] for the kk-th listed row: rows[kk], or row0 + kk without a list.  One workgroup per structure.
// pinv: the rule of numpy.linalg.pinv(hermitian=True): rows with |w| <= rcond * max|w| (of this structure) get 0.
__global__ __launch_bounds__(256) void k_mode_weights(const double* __restrict__ w, int nvec, int pinv, int row0,
                                                      const int* __restrict__ rows, int nsel, double rcond,
                                                      const long long* __restrict__ counts, double* __restrict__ s,
                                                      const RaggedRec* __restrict__ rag, int first_row) {
  __shared__ double red[256];
  const int b = blockIdx.x;
  const double* wb = w + (size_t)b * nvec;
  const int lim = rows_limit(counts, b, nvec, rag, first_row);   // (bounds the weights AND the pinv maximum)
  double thr = -1.0;   // |w| <= thr never holds: nothing is dropped
  if (pinv) {
    double mx = 0.0;   // (fmax skips NaN: a failed structure keeps thr = 0 and 1 / NaN below)
    for (int i = threadIdx.x; i < lim; i += 256) mx = fmax(mx, fabs(wb[i]));
    red[threadIdx.x] = mx;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (threadIdx.x < h) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + h]);
      __syncthreads();
    }
    thr = rcond * red[0];
  }
  for (int kk = threadIdx.x; kk < nsel; kk += 256) {
    const int row = rows ? rows[kk] : row0 + kk;
    double sv;
    if (row < 0 || row >= nvec) {
      sv = NAN;        // a listed row that was not solved: never read (the readers clamp), and loud in the result
    } else if (row >= lim) {
      sv = 0.0;
    } else {
      const double wk = wb[row];
      sv = fabs(wk) <= thr ? 0.0 : 1.0 / wk;   // (NaN compares false: a failed structure's results are NaN)
    }
    s[(size_t)b * nsel + kk] = sv;
  }
}

__device__ __forceinline__ int listed_row(const int* __restrict__ rows, int row0, int kk, int nvec) {
  const int r = rows ? rows[kk] : row0 + kk;
  return min(max(r, 0), nvec - 1);
}

// ---- msf ---------------------------------------------------------------------------------------------------------
// part[bz, c, j] = sum over the listed rows kk of chunk c, in order, of s[b, kk] V[b, row(kk), j]^2.
// grid (column tiles of 512, chunks, structures of the slab); lanes along the coordinate axis.  VEC: m is even and v is
// 16-byte aligned, so every row is, and a lane loads columns (2t, 2t + 1) as one 16-byte piece; otherwise (m = 3 N is
// odd for odd N: rows are only 8-byte aligned) a lane loads columns t and t + 256 of the tile as 8-byte pieces.
// The chunk length depends on the number of listed rows alone (msf_chunk), so a structure's partial sums -- and the
// result -- are the same bits in any batch.
// U listed rows from kk on: all row numbers and weights first, then all loads, then the sums in row order
template <bool VEC, bool LIST, int U>
__device__ __forceinline__ void msf_rows(const double* __restrict__ vb, const double* __restrict__ sb,
                                         const int* __restrict__ rows, int row0, int kk, int nvec, int m, int j0, int j1c,
                                         double& acc0, double& acc1) {
  double sv[U], x0[U], x1[U];
  const double* p[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    sv[u] = sb[kk + u];
    p[u] = vb + (size_t)listed_row(LIST ? rows : nullptr, row0, kk + u, nvec) * m;
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
  for (int u = 0; u < U; ++u) {
    const double t0 = fma(x0[u] * x0[u], sv[u], acc0), t1 = fma(x1[u] * x1[u], sv[u], acc1);
    acc0 = sv[u] != 0.0 ? t0 : acc0;
    acc1 = sv[u] != 0.0 ? t1 : acc1;
  }
}

template <bool VEC, bool LIST>
__global__ __launch_bounds__(256) void k_bmsf_partial(const double* __restrict__ v, const double* __restrict__ s,
                                                      const int* __restrict__ rows, int row0, int nsel, int nvec, int m,
                                                      int chunk, const long long* __restrict__ counts, int b0,
                                                      double* __restrict__ part, const RaggedRec* __restrict__ rag,
                                                      int first_row) {
  const int b = b0 + blockIdx.z;
  const int c = blockIdx.y;
  // ragged: the structure's own columns; a tile wholly behind them returns here, before its first load, and the lanes
  // of the tile that straddles them mask their tail (VEC: the 16-byte load may take one pad column, which is dropped)
  const int mo = rag ? rag[b].own : m;
  if ((int)blockIdx.x * 512 >= mo) return;
  const int k0 = c * chunk;
  int k1 = min(k0 + chunk, nsel);
  // without a list the rows ascend: those behind the window's count (and a slot's pad rows) are not even read
  if (!LIST) k1 = min(k1, rows_limit(counts, b, nvec, rag, first_row) - row0);
  const int j0 = VEC ? (blockIdx.x * 256 + threadIdx.x) * 2 : blockIdx.x * 512 + threadIdx.x;
  const int j1 = VEC ? j0 + 1 : j0 + 256;
  if (j0 >= mo) return;
  const bool has1 = j1 < mo;
  const int j1c = has1 ? j1 : j0;
  const double* vb = v + (size_t)b * nvec * m;
  const double* sb = s + (size_t)b * nsel;
  double acc0 = 0.0, acc1 = 0.0;
  int kk = k0;
  for (; kk + 4 <= k1; kk += 4) msf_rows<VEC, LIST, 4>(vb, sb, rows, row0, kk, nvec, m, j0, j1c, acc0, acc1);
  for (; kk < k1; ++kk) msf_rows<VEC, LIST, 1>(vb, sb, rows, row0, kk, nvec, m, j0, j1c, acc0, acc1);
  double* pp = part + ((size_t)blockIdx.z * gridDim.y + c) * m;
  pp[j0] = acc0;
  if (has1) pp[j1] = acc1;
}

// out[b, a] = sum over chunks, then over the dim components, in that fixed order
// (ragged: over the structure's n_atoms, to its packed atom offset)
__global__ __launch_bounds__(256) void k_bmsf_reduce(const double* __restrict__ part, int nchunk, int m, int dim, int b0,
                                                     double* __restrict__ out, const RaggedRec* __restrict__ rag) {
  const int b = b0 + blockIdx.y;
  const int N = rag ? rag[b].n_atoms : m / dim;
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= N) return;
  const double* pb = part + (size_t)blockIdx.y * nchunk * m;
  double acc = 0.0;
  for (int c = 0; c < nchunk; ++c)
    for (int d = 0; d < dim; ++d) acc += pb[(size_t)c * m + a * dim + d];
  out[(rag ? (size_t)rag[b].atom_off : (size_t)b * N) + a] = acc;
}

// ---- anisotropic fluctuation tensors (ANM, dim 3) ----------------------------------------------------------------
// The 3 x 3 diagonal blocks of the covariance over the selected modes, what crystallography records as ANISOU: six
// values per atom in that record's order, e = xx yy zz xy xz yz; xx + yy + zz is the msf of the same selection.
//   part[bz, c, e, a] = sum over the listed rows kk of chunk c, in order, of s[b, kk] V[b, row(kk), 3a + d] V[.., 3a + d']
// grid (atom tiles of 256, chunks, structures of the slab); one lane per ATOM: it loads the atom's three consecutive
// doubles of every listed row (rows are only 8-byte aligned for odd N, so three 8-byte pieces; a wavefront takes 1536
// contiguous bytes of the row) and keeps the six sums.  The same rows are read exactly once, as k_bmsf_partial reads
// them, and the chunks are msf_chunk's: a structure's bits are the same in any batch.  The partial sums are stored
// component-major (`na` atoms per component: m / 3) so that lanes store, and k_baniso_reduce loads, side by side.
// U listed rows from kk on: all row numbers and weights first, then all loads, then the sums in row order
template <bool LIST, int U>
__device__ __forceinline__ void aniso_rows(const double* __restrict__ vb, const double* __restrict__ sb,
                                           const int* __restrict__ rows, int row0, int kk, int nvec, int m, int j0,
                                           double (&acc)[6]) {
  double sv[U], x[U], y[U], z[U];
  const double* p[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    sv[u] = sb[kk + u];
    p[u] = vb + (size_t)listed_row(LIST ? rows : nullptr, row0, kk + u, nvec) * m + j0;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    x[u] = p[u][0]; y[u] = p[u][1]; z[u] = p[u][2];
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const double sx = sv[u] * x[u], sy = sv[u] * y[u], sz = sv[u] * z[u];
    const double t[6] = {fma(sx, x[u], acc[0]), fma(sy, y[u], acc[1]), fma(sz, z[u], acc[2]),
                         fma(sx, y[u], acc[3]), fma(sx, z[u], acc[4]), fma(sy, z[u], acc[5])};
#pragma unroll
    for (int e = 0; e < 6; ++e) acc[e] = sv[u] != 0.0 ? t[e] : acc[e];
  }
}

template <bool LIST>
__global__ __launch_bounds__(256) void k_baniso_partial(const double* __restrict__ v, const double* __restrict__ s,
                                                        const int* __restrict__ rows, int row0, int nsel, int nvec, int m,
                                                        int chunk, const long long* __restrict__ counts, int b0,
                                                        double* __restrict__ part, const RaggedRec* __restrict__ rag,
                                                        int first_row) {
  const int b = b0 + blockIdx.z;
  const int c = blockIdx.y;
  const int na = m / 3;
  // ragged: the structure's own atoms; a tile wholly behind them returns before its first load
  const int N = rag ? rag[b].n_atoms : na;
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= N) return;
  const int k0 = c * chunk;
  int k1 = min(k0 + chunk, nsel);
  // without a list the rows ascend: those behind the window's count (and a slot's pad rows) are not even read
  if (!LIST) k1 = min(k1, rows_limit(counts, b, nvec, rag, first_row) - row0);
  const double* vb = v + (size_t)b * nvec * m;
  const double* sb = s + (size_t)b * nsel;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int kk = k0;
  for (; kk + 4 <= k1; kk += 4) aniso_rows<LIST, 4>(vb, sb, rows, row0, kk, nvec, m, 3 * a, acc);
  for (; kk < k1; ++kk) aniso_rows<LIST, 1>(vb, sb, rows, row0, kk, nvec, m, 3 * a, acc);
  double* pp = part + ((size_t)blockIdx.z * gridDim.y + c) * 6 * na + a;
#pragma unroll
  for (int e = 0; e < 6; ++e) pp[(size_t)e * na] = acc[e];
}

// out[b, a, e] = sum over the chunks in their order (ragged: the structure's n_atoms, at 6 times its packed atom offset)
__global__ __launch_bounds__(256) void k_baniso_reduce(const double* __restrict__ part, int nchunk, int na, int b0,
                                                       double* __restrict__ out, const RaggedRec* __restrict__ rag) {
  const int b = b0 + blockIdx.y;
  const int N = rag ? rag[b].n_atoms : na;
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= N) return;
  const double* pb = part + (size_t)blockIdx.y * nchunk * 6 * na + a;
  double* o = out + ((rag ? (size_t)rag[b].atom_off : (size_t)b * N) + a) * 6;
#pragma unroll
  for (int e = 0; e < 6; ++e) {
    double acc = 0.0;
    for (int c = 0; c < nchunk; ++c) acc += pb[((size_t)c * 6 + e) * na];
    o[e] = acc;
  }
}

// ---- dcc ---------------------------------------------------------------------------------------------------------
// Listed rows k0 .. k0 + kc - 1 of every structure of the slab, component-major, so that the contraction over (row,
// component) is one GEMM per structure:
//   P[bz][(d * kc + k) * N + a] = V[b, row(k0 + k), dim a + d]        S = the same times s[b, k0 + k]
// A row without weight is not read: zeros in both operands.  Ragged: N = n_atoms of the structure and only its first
// dim * N columns are packed (the slot of `stride` elements is sized for the slot order).
__global__ __launch_bounds__(256) void k_bdcc_pack(const double* __restrict__ v, const double* __restrict__ s,
                                                   const int* __restrict__ rows, int row0, int nsel, int nvec, int m,
                                                   int dim, int k0, int kc, int b0, size_t stride,
                                                   double* __restrict__ p, double* __restrict__ sp,
                                                   const RaggedRec* __restrict__ rag) {
  const int k = blockIdx.y, kk = k0 + k;
  const int b = b0 + blockIdx.z;
  const double sv = s[(size_t)b * nsel + kk];
  const double* vr = v + ((size_t)b * nvec + listed_row(rows, row0, kk, nvec)) * m;
  const int N = rag ? rag[b].n_atoms : m / dim;
  const int mo = N * dim;
  double* pb = p + (size_t)blockIdx.z * stride;
  double* sb = sp + (size_t)blockIdx.z * stride;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < mo; j += gridDim.x * 256) {
    const int a = j / dim, d = j - a * dim;
    const size_t o = ((size_t)d * kc + k) * N + a;
    if (sv != 0.0) {   // (uniform over the workgroup)
      const double x = vr[j];
      pb[o] = x;
      sb[o] = x * sv;
    } else {
      pb[o] = 0.0;
      sb[o] = 0.0;
    }
  }
}

// one GEMM record per structure of the slab: out[b] (N, N) (+)= S^T-by-P over K = kc * dim (layout kGemmAmBn).
// out: the first structure of the slab (uniform) / the packed buffer (ragged: M = N = ldc = the structure's n_atoms, C at
// its square offset)
__global__ void k_bdcc_descs(GemmDesc* __restrict__ desc, int count, const double* __restrict__ sp,
                             const double* __restrict__ p, size_t stride, double* __restrict__ out, int N, int K,
                             double beta, const RaggedRec* __restrict__ rag, int b0) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= count) return;
  GemmDesc D{};
  if (rag) N = rag[b0 + i].n_atoms;
  D.a = sp + (size_t)i * stride; D.sa_i = 1; D.sa_k = N;
  D.b = p + (size_t)i * stride; D.sb_k = N; D.sb_j = 1;
  D.c = rag ? out + rag[b0 + i].sq_off : out + (size_t)i * N * N;
  D.ldc = N; D.m = N; D.n = N; D.k = K;
  D.alpha = 1.0; D.beta = beta;
  desc[i] = D;
}

// (c, diag: the first structure of the launch; ragged: the packed buffers, b0 the first structure of the launch)
__global__ __launch_bounds__(256) void k_bcopy_diag(const double* __restrict__ c, int N, double* __restrict__ diag,
                                                    const RaggedRec* __restrict__ rag, int b0) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  const size_t b = blockIdx.y;
  if (rag) {
    const RaggedRec r = rag[b0 + b];
    if (a < r.n_atoms) diag[r.atom_off + a] = c[r.sq_off + (size_t)a * r.n_atoms + a];
    return;
  }
  if (a < N) diag[b * N + a] = c[(b * N + a) * N + a];
}

// in place; the reference divides by outer(sqrt(diag), sqrt(diag)) (nma.py:352-354)
__global__ __launch_bounds__(256) void k_bdcc_norm(double* __restrict__ c, const double* __restrict__ diag, int N,
                                                   const RaggedRec* __restrict__ rag, int b0) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  const int r = blockIdx.y;
  const size_t b = blockIdx.z;
  if (rag) N = rag[b0 + b].n_atoms;
  if (a >= N || r >= N) return;
  const double* db = rag ? diag + rag[b0 + b].atom_off : diag + b * N;
  double* cb = rag ? c + rag[b0 + b].sq_off : c + b * N * N;
  cb[(size_t)r * N + a] = cb[(size_t)r * N + a] / (sqrt(db[a]) * sqrt(db[r]));
}

}  // namespace

// listed rows per chunk: from the number of listed rows alone.  20 rows -> 5 chunks of 4 (64 structures of m = 6000:
// 3840 workgroups), 6000 rows -> 48 chunks of 125 (36864 workgroups, partial sums 1.6 % of the bytes read).
// (declared in eigh_internal.h: mode_response.hip cuts its rows the same way)
int msf_chunk(int64_t nsel) { return (int)std::min<int64_t>(128, std::max<int64_t>(4, (nsel + 47) / 48)); }

namespace {

struct DccPlan {
  int64_t kc;      // listed rows per GEMM
  int64_t slab;    // structures per GEMM launch
  size_t stride;   // elements of one structure's P (and S) slot
};

// from (m, rows, budget) only -- never from the batch size or a structure's position
DccPlan dcc_plan(int64_t m, int64_t nsel, int64_t batch, size_t budget) {
  DccPlan pl{};
  const size_t row_bytes = 2 * (size_t)m * 8;            // one listed row in P and in S
  const size_t full = row_bytes * (size_t)nsel;
  if (full <= budget) {
    pl.kc = nsel;
    pl.slab = std::min<int64_t>(kMaxSlab, (int64_t)std::max<size_t>(1, budget / std::max<size_t>(full, 1)));
  } else {
    pl.kc = (int64_t)std::max<size_t>(1, budget / row_bytes);
    pl.slab = 1;
  }
  pl.kc = std::min<int64_t>(std::max<int64_t>(pl.kc, 1), 65535);   // (grid.y of k_bdcc_pack)
  pl.slab = std::min(pl.slab, std::max<int64_t>(batch, 1));
  pl.stride = align_up((size_t)pl.kc * m, 32);
  return pl;
}

int64_t msf_slab(int64_t m, int64_t nsel, int64_t batch, size_t budget) {
  const size_t per = (size_t)((nsel + msf_chunk(nsel) - 1) / msf_chunk(nsel)) * m * 8;
  const int64_t slab = std::min<int64_t>(kMaxSlab, (int64_t)std::max<size_t>(1, budget / std::max<size_t>(per, 1)));
  return std::min(slab, std::max<int64_t>(batch, 1));
}

// six partial sums per atom and chunk where the msf keeps three
int64_t aniso_slab(int64_t m, int64_t nsel, int64_t batch, size_t budget, int chunk) {
  const size_t per = (size_t)((nsel + chunk - 1) / chunk) * 6 * (m / 3) * 8;
  const int64_t slab = std::min<int64_t>(kMaxSlab, (int64_t)std::max<size_t>(1, budget / std::max<size_t>(per, 1)));
  return std::min(slab, std::max<int64_t>(batch, 1));
}

}  // namespace

// (declared in eigh_internal.h: dist_fluct.hip takes its weights from here too)
int launch_mode_weights(sc_ctx* ctx, const double* d_w, int64_t nvec, int64_t batch, const sc_mode_selection& sel,
                        int64_t nsel, const int64_t* d_counts, double* d_s, const RaggedView* rv) {
  hipLaunchKernelGGL(k_mode_weights, dim3((unsigned)batch), dim3(256), 0, ctx->stream, d_w, (int)nvec,
                     sel.kind == SC_SEL_PINV ? 1 : 0, sel.kind == SC_SEL_FROM_ROW ? (int)sel.row0 : 0,
                     sel.kind == SC_SEL_ROWS ? sel.d_rows : nullptr, (int)nsel, sel.rcond,
                     reinterpret_cast<const long long*>(d_counts), d_s, rv ? rv->d_rec : nullptr,
                     rv ? rv->first_row : 0);
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

size_t modes_budget_default() {
  static const size_t v = [] {
    const char* e = getenv("SPRINGCRAFT_MODES_BUDGET_BYTES");
    const long long x = e ? atoll(e) : 0;
    return x > 0 ? (size_t)x : kModesBudgetBytes;
  }();
  return v;
}

int64_t batch_modes_nsel(const sc_mode_selection& sel, int64_t nvec) {
  switch (sel.kind) {
    case SC_SEL_FROM_ROW: return std::max<int64_t>(0, nvec - sel.row0);
    case SC_SEL_ROWS: return sel.n_rows;
    default: return nvec;
  }
}

// weights (batch, n_sel) | msf, tensors: partial sums of one slab | dcc: P and S of one slab, diagonals (batch, N), records |
// distance fluctuations: nothing more | response, combine (mode_response.hip): coefficients and partial sums, partial sums
// | scanning (mode_prs.hip): one diagonal per structure of a slab | generalized correlation (mode_lmi.hip): the tensors'
// partial sums of one slab, tensors (batch, N, 6), whitening factors (batch, N, 9)
// (ragged: m is the slot order, the diagonals are packed over all atoms)
size_t batch_modes_workspace_bytes(int64_t m, int64_t nvec, int64_t batch, int dim, int64_t nsel, int what,
                                   size_t budget, const RaggedView* rv) {
  (void)nvec;
  if (budget == 0) budget = modes_budget_default();
  size_t bytes = align_up((size_t)batch * std::max<int64_t>(nsel, 1) * 8, 256);
  if (what == 0) {
    const int chunk = msf_chunk(nsel);
    bytes += align_up((size_t)msf_slab(m, nsel, batch, budget) * ((nsel + chunk - 1) / chunk) * m * 8, 256);
  } else if (what == 2) {
    const int chunk = msf_chunk(nsel);
    bytes += align_up((size_t)aniso_slab(m, nsel, batch, budget, chunk) * ((nsel + chunk - 1) / chunk) * 6 * (m / 3) * 8, 256);
  } else if (what == 4) {
    // distance fluctuations (dist_fluct.hip): the weights alone, a pair's sum never leaves its lane
  } else if (what == 7) {
    bytes += modes_prs_diag_bytes(m, batch, rv);
  } else if (what == 8) {
    // generalized correlation (mode_lmi.hip): the tensors' partial sums in chunks of kLmiTensorChunk rows, then the
    // tensors and the factors
    const int chunk = kLmiTensorChunk;
    bytes += align_up((size_t)aniso_slab(m, nsel, batch, budget, chunk) * ((nsel + chunk - 1) / chunk) * 6 * (m / 3) * 8, 256);
    bytes += modes_lmi_whiten_bytes(m, batch, rv);
  } else if (what == 5) {
    bytes += modes_response_workspace_bytes(m, batch, nsel, 5, budget);
  } else if (what == 6) {
    bytes = modes_response_workspace_bytes(m, batch, nsel, 6, budget);   // (no weights: the caller's coefficients)
  } else {
    const DccPlan pl = dcc_plan(m, nsel, batch, budget);
    const size_t diag = (size_t)(rv ? rv->total_atoms : batch * (m / dim));
    bytes += 2 * align_up((size_t)pl.slab * pl.stride * 8, 256) + align_up(diag * 8, 256) +
             align_up((size_t)pl.slab * sizeof(GemmDesc), 256);
  }
  return bytes + 1024;
}

int batch_msf_device(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch, int dim,
                     const sc_mode_selection& sel, const int64_t* d_counts, size_t budget, double* d_out,
                     const RaggedView* rv) {
  if (budget == 0) budget = modes_budget_default();
  hipStream_t st = ctx->stream;
  const int64_t nsel = batch_modes_nsel(sel, nvec);
  const int64_t N = rv ? rv->max_atoms : m / dim;   // (bounds the grid of the reduce)
  const RaggedRec* rag = rv ? rv->d_rec : nullptr;
  const int first_row = rv ? rv->first_row : 0;
  if (nsel == 0) {
    SC_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(double) * (size_t)(rv ? rv->total_atoms : batch * N), st));
    return SC_OK;
  }
  SC_TRY(sc_reserve_modes(ctx, batch_modes_workspace_bytes(m, nvec, batch, dim, nsel, 0, budget, rv)));
  char* base = (char*)ctx->modes_ws;
  double* d_s = reinterpret_cast<double*>(base);
  double* d_part = reinterpret_cast<double*>(base + align_up((size_t)batch * nsel * 8, 256));
  SC_TRY(launch_mode_weights(ctx, d_w, nvec, batch, sel, nsel, d_counts, d_s, rv));
  const int chunk = msf_chunk(nsel);
  const int nchunk = (int)((nsel + chunk - 1) / chunk);
  const int64_t slab = msf_slab(m, nsel, batch, budget);
  const bool vec = m % 2 == 0 && reinterpret_cast<uintptr_t>(d_v) % 16 == 0;
  const int* rows = sel.kind == SC_SEL_ROWS ? sel.d_rows : nullptr;
  const int row0 = sel.kind == SC_SEL_FROM_ROW ? (int)sel.row0 : 0;
  const long long* cnt = reinterpret_cast<const long long*>(d_counts);
  for (int64_t b0 = 0; b0 < batch; b0 += slab) {
    const unsigned nb = (unsigned)std::min(slab, batch - b0);
    const dim3 grid((unsigned)((m + 511) / 512), (unsigned)nchunk, nb);
    auto kern = vec ? (rows ? k_bmsf_partial<true, true> : k_bmsf_partial<true, false>)
                    : (rows ? k_bmsf_partial<false, true> : k_bmsf_partial<false, false>);
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, d_v, d_s, rows, row0, (int)nsel, (int)nvec, (int)m, chunk, cnt,
                       (int)b0, d_part, rag, first_row);
    hipLaunchKernelGGL(k_bmsf_reduce, dim3((unsigned)((N + 255) / 256), nb), dim3(256), 0, st, d_part, nchunk, (int)m,
                       dim, (int)b0, d_out, rag);
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

// dim 3 only (the callers check): d_out (batch, m / 3, 6), ragged (sum n_atoms, 6) packed
int batch_aniso_device(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                       const sc_mode_selection& sel, const int64_t* d_counts, size_t budget, double* d_out,
                       const RaggedView* rv, int chunk_rows) {
  if (budget == 0) budget = modes_budget_default();
  hipStream_t st = ctx->stream;
  const int64_t nsel = batch_modes_nsel(sel, nvec);
  const int64_t na = m / 3;
  const int64_t N = rv ? rv->max_atoms : na;   // (bounds the grids)
  const RaggedRec* rag = rv ? rv->d_rec : nullptr;
  const int first_row = rv ? rv->first_row : 0;
  if (nsel == 0) {
    SC_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(double) * 6 * (size_t)(rv ? rv->total_atoms : batch * N), st));
    return SC_OK;
  }
  // (chunk_rows: mode_lmi.hip's call, which has reserved its own workspace, what = 8, with this one's layout at its head)
  if (!chunk_rows) SC_TRY(sc_reserve_modes(ctx, batch_modes_workspace_bytes(m, nvec, batch, 3, nsel, 2, budget, rv)));
  char* base = (char*)ctx->modes_ws;
  double* d_s = reinterpret_cast<double*>(base);
  double* d_part = reinterpret_cast<double*>(base + align_up((size_t)batch * nsel * 8, 256));
  SC_TRY(launch_mode_weights(ctx, d_w, nvec, batch, sel, nsel, d_counts, d_s, rv));
  const int chunk = chunk_rows ? chunk_rows : msf_chunk(nsel);
  const int nchunk = (int)((nsel + chunk - 1) / chunk);
  const int64_t slab = aniso_slab(m, nsel, batch, budget, chunk);
  const int* rows = sel.kind == SC_SEL_ROWS ? sel.d_rows : nullptr;
  const int row0 = sel.kind == SC_SEL_FROM_ROW ? (int)sel.row0 : 0;
  const long long* cnt = reinterpret_cast<const long long*>(d_counts);
  const unsigned tiles = (unsigned)((N + 255) / 256);
  for (int64_t b0 = 0; b0 < batch; b0 += slab) {
    const unsigned nb = (unsigned)std::min(slab, batch - b0);
    hipLaunchKernelGGL(rows ? k_baniso_partial<true> : k_baniso_partial<false>, dim3(tiles, (unsigned)nchunk, nb),
                       dim3(256), 0, st, d_v, d_s, rows, row0, (int)nsel, (int)nvec, (int)m, chunk, cnt, (int)b0, d_part,
                       rag, first_row);
    hipLaunchKernelGGL(k_baniso_reduce, dim3(tiles, nb), dim3(256), 0, st, d_part, nchunk, (int)na, (int)b0, d_out, rag);
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

int batch_dcc_device(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch, int dim,
                     const sc_mode_selection& sel, const int64_t* d_counts, int norm, size_t budget, double* d_out,
                     const RaggedView* rv) {
  if (budget == 0) budget = modes_budget_default();
  hipStream_t st = ctx->stream;
  const int64_t nsel = batch_modes_nsel(sel, nvec);
  const int N = rv ? rv->max_atoms : (int)(m / dim);   // (ragged: bounds the grids; every kernel reads the structure's own)
  const RaggedRec* rag = rv ? rv->d_rec : nullptr;
  SC_TRY(sc_reserve_modes(ctx, batch_modes_workspace_bytes(m, nvec, batch, dim, nsel, 1, budget, rv)));
  const DccPlan pl = dcc_plan(m, nsel, batch, budget);
  char* base = (char*)ctx->modes_ws;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* q = base + off; off += align_up(bytes, 256); return q; };
  double* d_s = reinterpret_cast<double*>(take((size_t)batch * std::max<int64_t>(nsel, 1) * 8));
  double* d_p = reinterpret_cast<double*>(take((size_t)pl.slab * pl.stride * 8));
  double* d_sp = reinterpret_cast<double*>(take((size_t)pl.slab * pl.stride * 8));
  double* d_diag = reinterpret_cast<double*>(take((size_t)(rv ? rv->total_atoms : batch * (int64_t)N) * 8));
  GemmDesc* d_desc = reinterpret_cast<GemmDesc*>(take((size_t)pl.slab * sizeof(GemmDesc)));
  if (nsel == 0) {
    SC_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(double) * (rv ? (size_t)rv->total_sq : (size_t)batch * N * N), st));
  } else {
    SC_TRY(launch_mode_weights(ctx, d_w, nvec, batch, sel, nsel, d_counts, d_s, rv));
    const int* rows = sel.kind == SC_SEL_ROWS ? sel.d_rows : nullptr;
    const int row0 = sel.kind == SC_SEL_FROM_ROW ? (int)sel.row0 : 0;
    // one block tile for every launch of this call, the short last slab included: a structure rounds the same way in
    // whichever slab it lands
    const int pin = gemm_f64_tile(ctx, (int)pl.slab, N, N, kGemmAmBn);
    for (int64_t b0 = 0; b0 < batch; b0 += pl.slab) {
      const int nb = (int)std::min(pl.slab, batch - b0);
      for (int64_t k0 = 0; k0 < nsel; k0 += pl.kc) {
        const int kc = (int)std::min(pl.kc, nsel - k0);
        hipLaunchKernelGGL(k_bdcc_pack, dim3((unsigned)std::min<int64_t>((m + 255) / 256, 64), (unsigned)kc, (unsigned)nb),
                           dim3(256), 0, st, d_v, d_s, rows, row0, (int)nsel, (int)nvec, (int)m, dim, (int)k0, kc,
                           (int)b0, pl.stride, d_p, d_sp, rag);
        hipLaunchKernelGGL(k_bdcc_descs, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, st, d_desc, nb, d_sp, d_p,
                           pl.stride, rag ? d_out : d_out + (size_t)b0 * N * N, N, kc * dim, k0 == 0 ? 0.0 : 1.0, rag,
                           (int)b0);
        SC_HIP(ctx, hipGetLastError());
        SC_TRY(launch_gemm_f64(ctx, d_desc, {.count = nb, .max_m = N, .max_n = N, .layout = kGemmAmBn, .pin_tile = pin}));
      }
    }
  }
  if (norm) {
    for (int64_t b0 = 0; b0 < batch; b0 += kMaxSlab) {
      const unsigned nb = (unsigned)std::min(kMaxSlab, batch - b0);
      double* c = rag ? d_out : d_out + (size_t)b0 * N * N;
      double* dg = rag ? d_diag : d_diag + (size_t)b0 * N;
      hipLaunchKernelGGL(k_bcopy_diag, dim3((unsigned)((N + 255) / 256), nb), dim3(256), 0, st, c, N, dg, rag, (int)b0);
      hipLaunchKernelGGL(k_bdcc_norm, dim3((unsigned)((N + 255) / 256), (unsigned)N, nb), dim3(256), 0, st, c, dg, N, rag,
                         (int)b0);
    }
    SC_HIP(ctx, hipGetLastError());
  }
  return SC_OK;
}
