// Stage 1 of the two-stage tridiagonalisation (sy2sb): dense -> band of half-width kB.  The six forms of the panel QR
// (k_panel_qr with k_pqr_blk_a / _b, k_panel_wg, k_panel_coop with its take-over k_panel_serial), the small kernels
// between the GEMMs of the two-sided update (k_sum_xslices, k_sum_p2, k_sb_small) and the host side: launch_panel_qr and
// run_panel (one panel of a part of the batch) and sb_stage1.
//
// Overview of the algorithm: twostage.hip; which form a panel gets: twostage_policy.h; the GEMM records of a solve, the LDS
// layouts the kernels carve and the launches size, k_panel_coop's records: sy2sb_plan.h.
#include <algorithm>
#include <vector>

#include "twostage_internal.h"

namespace {

using sc_host::lds_bytes;
constexpr int kEarly = (kIb + 2) / 2;   // column loads per thread that cover a launch of an inner block (kIb + 1 columns)

// ================================================================================================================
// Stage 1: panel QR.  Panel = A[r0 : n, j0 : j0 + kB] (m x kB, column-major, ld n).  Launch j (0 .. nr):
//   (a) j >= 1: finish reflector j-1 from the partial results of launch j-1 (tail Gram row, pivot row) and apply it
//       to columns j .. kB-1; column j-1 becomes (R entries above, beta at the pivot, v below); v also goes, with its
//       explicit 1 and zeros above, into the three panel buffers [V|W], [W|V], [X1|X2|V];
//   (b) j < nr: tail Gram row of column j:  g[c] = sum_{r > j} P[r, j] P[r, c]  (per 128-row chunk; chunk 0 also saves
//       the pivot row P[j, j..]) for launch j+1.
// Grid (chunks, batch), 256 threads; the chunk's columns j-1 .. kB-1 live in LDS for the duration of the launch.
__global__ __launch_bounds__(256) void k_panel_qr(double* __restrict__ a_all, long long stride_a,
                                                  double* __restrict__ tri_all, TriLayout TL,
                                                  double* __restrict__ sb_all, SbLayout SL, int j0, int j, int nr,
                                                  int c_end) {
  // c_end: columns j .. c_end-1 are updated (kB: the whole rest of the panel; blocked panels: the rest of the
  // 8-column inner block, the other columns get the inner block's reflectors at once from k_pqr_blk_a / _b)
  constexpr int LD = kQrRows + 1;
  extern __shared__ __attribute__((aligned(16))) double sm[];
  // only the columns this launch touches, c_lo .. c_end-1, are held (the image is indexed relative to c_lo): with the
  // blocked panels that is at most 9 columns = 9 KB instead of 66 KB, i.e. 8 workgroups per CU instead of 2
  const int c_lo = j > 0 ? j - 1 : 0;
  const int ncl = c_end - c_lo;
  const sc_host::LdsPanelQr lds = sc_host::lds_panel_qr(ncl);
  double* P = sm + lds.P;              // [ncl][LD]   column c at P[(c - c_lo) * LD + r]
  double* wv = sm + lds.wv;            // [kB]  w_c of the reflector being applied
  double* vv = sm + lds.vv;            // [kQrRows]  v_r
  double* red = sm + lds.red;          // [4][kB]
  __shared__ double s_scale, s_beta, s_tau;

  const int n = TL.n;
  const int r0 = j0 + kB, m = n - r0;
  double* A = a_all + (size_t)blockIdx.y * stride_a;
  double* tri = tri_all + (size_t)blockIdx.y * TL.slab;
  double* sb = sb_all + (size_t)blockIdx.y * SL.slab;
  const int chunk = blockIdx.x, nchunks = gridDim.x;
  const int row_base = chunk * kQrRows;   // local (panel) row of this chunk's first row
  const int tid = threadIdx.x;
  const int prev = j - 1;
  // launch j reads what launch j-1 left and writes for launch j+1 while other workgroups may still be reading:
  // two copies, alternating
  const int nchunk_cap = (n + kQrRows - 1) / kQrRows + 1;
  const double* part_in = sb + SL.qrpart + (size_t)((j + 1) & 1) * nchunk_cap * kB;
  double* part_out = sb + SL.qrpart + (size_t)(j & 1) * nchunk_cap * kB;
  const double* piv_in = sb + SL.qrpiv + (size_t)((j + 1) & 1) * (kB + 8);
  double* piv_out = sb + SL.qrpiv + (size_t)(j & 1) * (kB + 8);

  // (1a) chunk -> registers, requested BEFORE the partial results of the previous launch are read and reduced (two
  // dependent memory round trips become one; a launch of a blocked panel holds at most 9 columns = one pass)
  const int ld_r = tid & (kQrRows - 1), ld_half = tid >> 7;
  const int ld_rl = row_base + ld_r;
  const double* ld_src = A + (size_t)j0 * n + r0 + std::min(ld_rl, m - 1);
  const bool early = ncl <= 2 * kEarly;
  double t_early[kEarly];
  if (early) {
#pragma unroll
    for (int u = 0; u < kEarly; ++u) t_early[u] = ld_src[(size_t)std::min(c_lo + ld_half + 2 * u, kB - 1) * n];
  }

  // (a0) reflector scalars and w
  if (j >= 1) {
    {
      // tail Gram row of column prev: sum of the chunks' partial rows, four threads per column, loads four deep
      const int cq = tid & 63, qq = tid >> 6;
      double g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0;
      int ch = qq;
      for (; ch + 12 < nchunks; ch += 16) {
        g0 += part_in[(size_t)ch * kB + cq];
        g1 += part_in[(size_t)(ch + 4) * kB + cq];
        g2 += part_in[(size_t)(ch + 8) * kB + cq];
        g3 += part_in[(size_t)(ch + 12) * kB + cq];
      }
      for (; ch < nchunks; ch += 4) g0 += part_in[(size_t)ch * kB + cq];
      red[qq * kB + cq] = (g0 + g1) + (g2 + g3);
    }
    __syncthreads();
    if (tid < kB) red[tid] = (red[tid] + red[kB + tid]) + (red[2 * kB + tid] + red[3 * kB + tid]);
    __syncthreads();
    if (tid == 0) {
      const double alpha = piv_in[prev];
      const HH h = householder(alpha, red[prev]);
      s_scale = h.scale; s_beta = h.beta; s_tau = h.tau;
      if (chunk == 0) tri[TL.tau + j0 + prev] = h.tau;
    }
    __syncthreads();
    if (tid < kB && tid >= j) {
      const double prow = piv_in[tid];
      wv[tid] = s_tau * (prow + s_scale * red[tid]);
    }
  }

  // (1) chunk -> LDS: lanes along the rows (contiguous in memory)
  // (loads are unconditional, with clamped indices, and issued eight at a time: a load that is merged with a zero
  //  under a predicate makes hipcc wait for it before issuing the next one)
  if (early) {
#pragma unroll
    for (int u = 0; u < kEarly; ++u) {
      const int c = c_lo + ld_half + 2 * u;
      if (c < c_end) P[(c - c_lo) * LD + ld_r] = ld_rl < m ? t_early[u] : 0.0;
    }
  } else {
    const int r = ld_r, half = ld_half, rl = ld_rl;
    const double* src = ld_src;
    for (int c = c_lo + half; c < c_end; c += 16) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = src[(size_t)std::min(c + 2 * u, kB - 1) * n];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (c + 2 * u < c_end) P[((c + 2 * u) - c_lo) * LD + r] = rl < m ? t[u] : 0.0;
    }
  }
  __syncthreads();

  const int c = tid & 63, q = tid >> 6;   // column / row quarter (32 rows) of this thread in the compute phases
  if (j >= 1) {
    // (a1) v
    if (tid < kQrRows) {
      const int rl = row_base + tid;
      double v = 0.0;
      if (rl < m) v = rl > prev ? s_scale * P[(prev - c_lo) * LD + tid] : (rl == prev ? 1.0 : 0.0);
      vv[tid] = v;
    }
    __syncthreads();
    // (a2) P[:, c] -= v w_c
    if (c >= j && c < c_end) {
      const double w = wv[c];
#pragma unroll 8
      for (int r = q * 32; r < q * 32 + 32; ++r) P[(c - c_lo) * LD + r] -= vv[r] * w;
    }
    // column prev: v below the pivot, beta at it (rows above keep their R entries); and the panel buffers
    if (tid < kQrRows) {
      const int rl = row_base + tid;
      if (rl < m) {
        const double v = vv[tid];
        if (rl > prev) P[(prev - c_lo) * LD + tid] = v;
        else if (rl == prev) P[(prev - c_lo) * LD + tid] = s_beta;
        const size_t row = (size_t)r0 + rl;
        sb[SL.vw + (size_t)prev * n + row] = v;
        sb[SL.wv + (size_t)(kB + prev) * n + row] = -v;   // (the [W|V] panel holds -[W|V]: see the trailing update's record)
        sb[SL.xv + (size_t)(2 * kB + prev) * n + row] = v;
      }
    }
    __syncthreads();
  }

  if (j < nr) {
    // (b) tail Gram row of column j over this chunk: rows with local index > j
    double acc = 0.0;
    if (c >= j && c < c_end) {
#pragma unroll 8
      for (int r = q * 32; r < q * 32 + 32; ++r) {
        const int rl = row_base + r;
        if (rl > j && rl < m) acc += P[(j - c_lo) * LD + r] * P[(c - c_lo) * LD + r];
      }
    }
    red[q * kB + c] = acc;
    __syncthreads();
    if (tid < kB) {
      part_out[(size_t)chunk * kB + tid] = (red[tid] + red[kB + tid]) + (red[2 * kB + tid] + red[3 * kB + tid]);
      if (chunk == 0 && tid >= j && tid < c_end) piv_out[tid] = P[(tid - c_lo) * LD + j];   // pivot row (alpha at [j])
    }
  } else {
    // last launch of the panel: columns without a reflector (short last panel) are zero in the V buffers
    for (int cc = nr; cc < kB; ++cc)
      for (int r = tid; r < kQrRows; r += 256) {
        const int rl = row_base + r;
        if (rl < m) {
          const size_t row = (size_t)r0 + rl;
          sb[SL.vw + (size_t)cc * n + row] = 0.0;
          sb[SL.wv + (size_t)(kB + cc) * n + row] = 0.0;
          sb[SL.xv + (size_t)(2 * kB + cc) * n + row] = 0.0;
        }
      }
  }

  // (2) LDS -> chunk
  if (j >= 1) {
    const int r = tid & (kQrRows - 1), half = tid >> 7;
    const int rl = row_base + r;
    if (rl < m)
      for (int cc = c_lo + half; cc < c_end; cc += 2) A[(size_t)(j0 + cc) * n + r0 + rl] = P[(cc - c_lo) * LD + r];
  }
}

// ---- blocked panels: the 8 reflectors of an inner block [c0, c0+8) applied to the columns to their right at once ----
// k_pqr_blk_a: finishes reflector c0+7 (the inner block's last) and forms, per 128-row chunk, the partial products
//   M[i][c] = v_{c0+i} . P[:, c]  for c = c0 .. kB-1  (the first 8 columns are the Gram matrix of the block's reflectors).
// k_pqr_blk_b: sums them, builds the 8 x 8 T factor, W = T^T M, updates P[:, c] -= V W for c >= c0+8 and leaves the
//   tail Gram row / pivot row of column c0+8 for the next inner block's first column launch.

// explicit form of the inner block's reflectors in the LDS copy of chunk 0 (memory keeps R above the pivots)
__device__ __forceinline__ void blk_explicit_v(double* P, int LD, int c0, int ncols, int row_base) {
  if (row_base != 0) return;   // pivot rows are local rows c0 .. c0+7 of the first chunk
  for (int idx = threadIdx.x; idx < ncols * kB; idx += 256) {
    const int i = idx / kB, r = idx % kB;   // rows 0..63 suffice (pivots < 64)
    const int piv = c0 + i;
    if (r < piv) P[i * LD + r] = 0.0;          // (the LDS image starts at column c0)
    else if (r == piv) P[i * LD + r] = 1.0;
  }
}

__global__ __launch_bounds__(256) void k_pqr_blk_a(double* __restrict__ a_all, long long stride_a,
                                                   double* __restrict__ tri_all, TriLayout TL,
                                                   double* __restrict__ sb_all, SbLayout SL, int j0, int c0) {
  constexpr int LD = kQrRows + 1;
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const sc_host::LdsBlk lds = sc_host::lds_pqr_blk_a(c0);
  double* P = sm + lds.P;              // [kB - c0][LD]: columns c0 .. kB-1, indexed relative to c0
  // (lds.mid: kQrRows doubles nobody uses any more; kept, the launch's byte count and with it the occupancy stay)
  double* red = sm + lds.red;          // [4][2][kB]
  __shared__ double s_scale, s_beta;
  const int n = TL.n;
  const int r0 = j0 + kB, m = n - r0;
  double* A = a_all + (size_t)blockIdx.y * stride_a;
  double* tri = tri_all + (size_t)blockIdx.y * TL.slab;
  double* sb = sb_all + (size_t)blockIdx.y * SL.slab;
  const int chunk = blockIdx.x, nchunks = gridDim.x;
  const int row_base = chunk * kQrRows;
  const int tid = threadIdx.x;
  const int prev = c0 + kIb - 1;
  const int nchunk_cap = (n + kQrRows - 1) / kQrRows + 1;
  const double* part_in = sb + SL.qrpart + (size_t)(prev & 1) * nchunk_cap * kB;
  const double* piv_in = sb + SL.qrpiv + (size_t)(prev & 1) * (kB + 8);

  // scalars of reflector prev
  {
    double g = 0.0;
    for (int ch = tid; ch < nchunks; ch += 256) g += part_in[(size_t)ch * kB + prev];
    g = wave_sum(g);
    if ((tid & 63) == 0) red[tid >> 6] = g;
    __syncthreads();
    if (tid == 0) {
      const HH h = householder(piv_in[prev], (red[0] + red[1]) + (red[2] + red[3]));
      s_scale = h.scale; s_beta = h.beta;
      if (chunk == 0) tri[TL.tau + j0 + prev] = h.tau;
    }
  }
  // chunk (columns c0 .. kB-1) -> LDS
  {
    const int r = tid & (kQrRows - 1), half = tid >> 7;
    const int rl = row_base + r;
    const double* src = A + (size_t)j0 * n + r0 + std::min(rl, m - 1);
    for (int c = c0 + half; c < kB; c += 16) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = src[(size_t)std::min(c + 2 * u, kB - 1) * n];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (c + 2 * u < kB) P[((c + 2 * u) - c0) * LD + r] = rl < m ? t[u] : 0.0;
    }
  }
  __syncthreads();
  // v of reflector prev: to memory (v below the pivot, beta at it), to the panel buffers, explicit form in LDS
  if (tid < kQrRows) {
    const int rl = row_base + tid;
    double v = 0.0;
    if (rl < m) v = rl > prev ? s_scale * P[(prev - c0) * LD + tid] : (rl == prev ? 1.0 : 0.0);
    if (rl < m) {
      if (rl > prev) A[(size_t)(j0 + prev) * n + r0 + rl] = v;
      else if (rl == prev) A[(size_t)(j0 + prev) * n + r0 + rl] = s_beta;
      const size_t row = (size_t)r0 + rl;
      sb[SL.vw + (size_t)prev * n + row] = v;
      sb[SL.wv + (size_t)(kB + prev) * n + row] = -v;   // (the [W|V] panel holds -[W|V]: see the trailing update's record)
      sb[SL.xv + (size_t)(2 * kB + prev) * n + row] = v;
    }
    P[(prev - c0) * LD + tid] = v;
  }
  __syncthreads();
  blk_explicit_v(P, LD, c0, kIb - 1, row_base);
  __syncthreads();
  // M partial: thread (c, q): 8 dot products over its 32 rows
  const int c = tid & 63, q = tid >> 6;
  double acc[kIb];
#pragma unroll
  for (int i = 0; i < kIb; ++i) acc[i] = 0.0;
  if (c >= c0) {
#pragma unroll 4
    for (int r = q * 32; r < q * 32 + 32; ++r) {
      const double x = P[(c - c0) * LD + r];
#pragma unroll
      for (int i = 0; i < kIb; ++i) acc[i] += P[((c0 + i) - c0) * LD + r] * x;
    }
  }
  double* p8 = sb + SL.qrpart8 + (size_t)chunk * kIb * kB;
#pragma unroll
  for (int pass = 0; pass < kIb / 2; ++pass) {
    red[(q * 2 + 0) * kB + c] = acc[2 * pass];
    red[(q * 2 + 1) * kB + c] = acc[2 * pass + 1];
    __syncthreads();
    if (tid < 2 * kB) {
      const int h = tid >> 6, cc = tid & 63;
      p8[(size_t)(2 * pass + h) * kB + cc] =
          (red[(0 * 2 + h) * kB + cc] + red[(1 * 2 + h) * kB + cc]) + (red[(2 * 2 + h) * kB + cc] + red[(3 * 2 + h) * kB + cc]);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_pqr_blk_b(double* __restrict__ a_all, long long stride_a,
                                                   const double* __restrict__ tri_all, TriLayout TL,
                                                   double* __restrict__ sb_all, SbLayout SL, int j0, int c0) {
  constexpr int LD = kQrRows + 1;
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const sc_host::LdsBlk lds = sc_host::lds_pqr_blk_b(c0);
  double* P = sm + lds.P;              // [kB - c0][LD]: columns c0 .. kB-1, indexed relative to c0
  double* Ms = sm + lds.mid;           // [kIb][kB]  M, later W
  double* red = sm + lds.red;          // [4][kB]
  __shared__ double T[kIb][kIb];
  const int n = TL.n;
  const int r0 = j0 + kB, m = n - r0;
  double* A = a_all + (size_t)blockIdx.y * stride_a;
  const double* tri = tri_all + (size_t)blockIdx.y * TL.slab;
  double* sb = sb_all + (size_t)blockIdx.y * SL.slab;
  const int chunk = blockIdx.x, nchunks = gridDim.x;
  const int row_base = chunk * kQrRows;
  const int tid = threadIdx.x;
  const int jn = c0 + kIb;             // first column to the right = next pivot column
  const int nchunk_cap = (n + kQrRows - 1) / kQrRows + 1;
  double* part_out = sb + SL.qrpart + (size_t)(jn & 1) * nchunk_cap * kB;
  double* piv_out = sb + SL.qrpiv + (size_t)(jn & 1) * (kB + 8);

  // chunk (columns c0 .. kB-1) -> LDS (issued first: the loads fly while the partial products are summed)
  {
    const int r = tid & (kQrRows - 1), half = tid >> 7;
    const int rl = row_base + r;
    const double* src = A + (size_t)j0 * n + r0 + std::min(rl, m - 1);
    for (int c = c0 + half; c < kB; c += 16) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = src[(size_t)std::min(c + 2 * u, kB - 1) * n];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (c + 2 * u < kB) P[((c + 2 * u) - c0) * LD + r] = rl < m ? t[u] : 0.0;
    }
  }
  // M = sum of the chunks' partial products
  for (int idx = tid; idx < kIb * kB; idx += 256) {
    const double* p8 = sb + SL.qrpart8 + idx;
    double g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0;
    int ch = 0;
    for (; ch + 3 < nchunks; ch += 4) {
      g0 += p8[(size_t)ch * kIb * kB];
      g1 += p8[(size_t)(ch + 1) * kIb * kB];
      g2 += p8[(size_t)(ch + 2) * kIb * kB];
      g3 += p8[(size_t)(ch + 3) * kIb * kB];
    }
    for (; ch < nchunks; ++ch) g0 += p8[(size_t)ch * kIb * kB];
    Ms[idx] = (g0 + g1) + (g2 + g3);
  }
  __syncthreads();
  // T (larft, forward columnwise) of the inner block: G[l][q] = Ms[l][c0 + q]
  if (tid == 0) {
    for (int qq = 0; qq < kIb; ++qq) {
      const double tau = tri[TL.tau + j0 + c0 + qq];
      for (int a = 0; a < qq; ++a) {
        double s2 = 0.0;
        for (int l = a; l < qq; ++l) s2 += T[a][l] * Ms[l * kB + c0 + qq];
        T[a][qq] = -tau * s2;
      }
      T[qq][qq] = tau;
      for (int a = qq + 1; a < kIb; ++a) T[a][qq] = 0.0;
    }
  }
  __syncthreads();
  // W = T^T M (in place, column by column: each thread owns column c)
  if (tid < kB && tid >= jn) {
    double mcol[kIb], wcol[kIb];
#pragma unroll
    for (int l = 0; l < kIb; ++l) mcol[l] = Ms[l * kB + tid];
#pragma unroll
    for (int i = 0; i < kIb; ++i) {
      double s2 = 0.0;
#pragma unroll
      for (int l = 0; l <= i; ++l) s2 += T[l][i] * mcol[l];
      wcol[i] = s2;
    }
#pragma unroll
    for (int i = 0; i < kIb; ++i) Ms[i * kB + tid] = wcol[i];
  }
  __syncthreads();
  blk_explicit_v(P, LD, c0, kIb, row_base);
  __syncthreads();
  // P[:, c] -= V W[:, c]
  const int c = tid & 63, q = tid >> 6;
  if (c >= jn) {
    double wcol[kIb];
#pragma unroll
    for (int i = 0; i < kIb; ++i) wcol[i] = Ms[i * kB + c];
#pragma unroll 4
    for (int r = q * 32; r < q * 32 + 32; ++r) {
      double s2 = 0.0;
#pragma unroll
      for (int i = 0; i < kIb; ++i) s2 += P[((c0 + i) - c0) * LD + r] * wcol[i];
      P[(c - c0) * LD + r] -= s2;
    }
  }
  __syncthreads();
  // tail Gram row and pivot row of column jn over the next inner block
  {
    double acc = 0.0;
    if (c >= jn && c < jn + kIb) {
#pragma unroll 8
      for (int r = q * 32; r < q * 32 + 32; ++r) {
        const int rl = row_base + r;
        if (rl > jn && rl < m) acc += P[(jn - c0) * LD + r] * P[(c - c0) * LD + r];
      }
    }
    red[q * kB + c] = acc;
    __syncthreads();
    if (tid < kB) {
      part_out[(size_t)chunk * kB + tid] = (red[tid] + red[kB + tid]) + (red[2 * kB + tid] + red[3 * kB + tid]);
      if (chunk == 0 && tid >= jn && tid < jn + kIb) piv_out[tid] = P[(tid - c0) * LD + jn];
    }
  }
  // LDS -> chunk (columns to the right of the inner block)
  {
    const int r = tid & (kQrRows - 1), half = tid >> 7;
    const int rl = row_base + r;
    if (rl < m)
      for (int cc = jn + half; cc < kB; cc += 2) A[(size_t)(j0 + cc) * n + r0 + rl] = P[(cc - c0) * LD + r];
  }
}

// ---- the whole panel QR in ONE workgroup per matrix (panels of at most 1024 RU rows) -----------------------------------
// The launches above exist because a column's reflector needs sums over all rows, i.e. over all 128-row chunks: 80
// dependent launches per panel, 10 - 22 us each, the longest item of a latency-bound solve (C4: 4700 launches per
// step).  Here 1024 threads own the rows of the panel (thread t: rows t, t + 1024, ...), the 8 columns of an inner block
// live in registers, and every sum over the rows is a wave reduction + 16 partials in LDS + two workgroup barriers
// (~1 us instead of a launch).  Same arithmetic as the launches above (tail Gram row + pivot row per column, the inner
// block's reflectors applied to the rest of the panel as one block update), other reduction trees.
// One workgroup streams its panel at the rate of one CU: the path is for batches (the matrices run side by side) and
// panels of at most 4096 rows; larger panels and single large matrices keep the chunked launches.
// Sums of eight values over the 64 lanes with 10 exchanges instead of 48: three halving steps (a lane keeps half of its
// values and receives the partner's sums of those), then three plain steps.  The exchanges inside a row of 16 lanes (eight of the ten) are DPP
// moves on the vector ALU; the two across rows go through the LDS crossbar, which all 16 waves of the workgroup share.  Lane l < 8 returns the total of v[wave_reduce8_index(l)].
template <int CTRL>
__device__ __forceinline__ double dpp_quad(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, 0xf, 0xf, true);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo));
}
__device__ __forceinline__ int wave_reduce8_index(int lane) { return 4 * (lane & 1) + 2 * ((lane >> 1) & 1) + ((lane >> 2) & 1); }
__device__ __forceinline__ double wave_reduce8(const double (&v)[8]) {
  const int lane = threadIdx.x & 63;
  double k4[4], k2[2];
  const bool b0 = (lane & 1) != 0, b1 = (lane & 2) != 0, b2 = (lane & 4) != 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double send = b0 ? v[k] : v[k + 4];
    k4[k] = (b0 ? v[k + 4] : v[k]) + dpp_quad<0xB1>(send);      // quad_perm [1, 0, 3, 2]: lane ^ 1
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double send = b1 ? k4[k] : k4[k + 2];
    k2[k] = (b1 ? k4[k + 2] : k4[k]) + dpp_quad<0x4E>(send);    // quad_perm [2, 3, 0, 1]: lane ^ 2
  }
  const double send = b2 ? k2[0] : k2[1];
  const double from_lo = dpp_quad<0x114>(send), from_hi = dpp_quad<0x104>(send);   // row_shr:4 (lane - 4), row_shl:4 (lane + 4)
  double r = (b2 ? k2[1] : k2[0]) + (b2 ? from_lo : from_hi);                      // lane ^ 4
  r += dpp_quad<0x128>(r);                                                         // row_ror:8 = lane ^ 8 inside a row of 16
  r += __shfl_xor(r, 16);
  r += __shfl_xor(r, 32);
  return r;
}

template <int RU, int CU, int NT = 1024>
__global__ __launch_bounds__(NT) void k_panel_wg(double* __restrict__ a_all, long long stride_a,
                                                   double* __restrict__ tri_all, TriLayout TL,
                                                   double* __restrict__ sb_all, SbLayout SL, int j0) {
  constexpr int kWgThreads = NT, kWgWaves = NT / 64;   // NT threads per panel
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr sc_host::LdsPanelWg lds = sc_host::lds_panel_wg(NT);
  double* red = sm + lds.red;                     // [2][kWgWaves][8] wave partials of the per-column sums (by column parity)
  double* piv = sm + lds.piv;                     // [2][8]          pivot row of the inner block
  double* tauL = sm + lds.tauL;                   // [8]
  double* Ms = sm + lds.Ms;                       // [8][kB]         M = V^T P, then W = T^T M (column index = panel column)
  double* part = sm + lds.part;                   // [kWgWaves][kB][8] wave partials of M
  const int n = TL.n;
  const int r0 = j0 + kB, m = n - r0;
  double* A = a_all + (size_t)blockIdx.x * stride_a;
  double* tri = tri_all + (size_t)blockIdx.x * TL.slab;
  double* sb = sb_all + (size_t)blockIdx.x * SL.slab;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  double* P = A + (size_t)j0 * n + r0;            // P(r, c) = P[c * n + r]
  int rl[RU], rc[RU];                             // my rows, and the same clamped into the panel for the loads
  bool ok[RU];
#pragma unroll
  for (int u = 0; u < RU; ++u) { rl[u] = tid + kWgThreads * u; ok[u] = rl[u] < m; rc[u] = std::min(rl[u], m - 1); }
  // accesses = a column's (uniform, scalar) base + the row's 32-bit byte offset, re-materialised at the access so that
  // the compiler does not hoist RU x 64 per-column vector addresses out of the loops (they would not fit the registers)
  typedef char __attribute__((address_space(1)))* gbp;
  typedef double __attribute__((address_space(1)))* gdp;
  typedef const double __attribute__((address_space(1)))* gdp_c;
  auto off = [&](int row) -> unsigned {
    unsigned e = 8u * (unsigned)row;
    asm volatile("" : "+v"(e));
    return e;
  };
  auto ld = [&](const double* colbase, int row) -> double { return *(gdp_c)((gbp)colbase + off(row)); };
  auto st = [&](double* colbase, int row, double val) { *(gdp)((gbp)colbase + off(row)) = val; };

  for (int c0 = 0; c0 < kB; c0 += 8) {
    // ---- the inner block's columns -> registers
    double x[RU][8];
#pragma unroll
    for (int u = 0; u < RU; ++u)
#pragma unroll
      for (int i = 0; i < 8; ++i) x[u][i] = ld(P + (size_t)(c0 + i) * n, rc[u]);
#pragma unroll
    for (int u = 0; u < RU; ++u)
#pragma unroll
      for (int i = 0; i < 8; ++i) x[u][i] = ok[u] ? x[u][i] : 0.0;
    // ---- its 8 reflectors
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const int j = c0 + jj;                      // pivot = local row j, owned by thread j (u = 0)
      const int pb = jj & 1;
      double g[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        double acc = 0.0;
        if (c >= jj) {
#pragma unroll
          for (int u = 0; u < RU; ++u) acc += rl[u] > j ? x[u][jj] * x[u][c] : 0.0;
        }
        g[c] = acc;
      }
      const double gs = wave_reduce8(g);
      if (lane < 8) red[(pb * kWgWaves + wv) * 8 + wave_reduce8_index(lane)] = gs;
      if (tid == j) {
#pragma unroll
        for (int c = jj; c < 8; ++c) piv[pb * 8 + c] = x[0][c];
      }
      __syncthreads();   // (ONE barrier per column: the partials and the pivot row are double-buffered by its parity)
      // totals: lane c < 8 of every wave sums the 16 partials of value c (same order in every wave), the others take them
      // from that lane through a scalar register
      double tot = 0.0;
      if (lane < 8) {
#pragma unroll
        for (int w2 = 0; w2 < kWgWaves; ++w2) tot += red[(pb * kWgWaves + w2) * 8 + lane];
      }
      double fin[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const unsigned long long tb = (unsigned long long)__double_as_longlong(tot);
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)tb, c);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(tb >> 32), c);
        fin[c] = __longlong_as_double((long long)(((unsigned long long)hi << 32) | (unsigned long long)lo));
      }
      const HH h = householder(piv[pb * 8 + jj], fin[jj]);
      if (tid == 0) { tri[TL.tau + j0 + j] = h.tau; tauL[jj] = h.tau; }
      double v[RU];
#pragma unroll
      for (int u = 0; u < RU; ++u) v[u] = rl[u] > j ? h.scale * x[u][jj] : (rl[u] == j ? 1.0 : 0.0);
#pragma unroll
      for (int c = jj + 1; c < 8; ++c) {
        const double wc = h.tau * (piv[pb * 8 + c] + h.scale * fin[c]);
#pragma unroll
        for (int u = 0; u < RU; ++u) x[u][c] -= v[u] * wc;
      }
      // column j is final: R entries of this inner block above the pivot, beta at it, v below; V in its explicit form
      // stays in the registers and goes to the three panel buffers
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        if (ok[u]) {
          if (rl[u] >= c0) st(P + (size_t)j * n, rl[u], rl[u] > j ? v[u] : (rl[u] == j ? h.beta : x[u][jj]));
          st(sb + SL.vw + (size_t)j * n + r0, rl[u], v[u]);
          st(sb + SL.wv + (size_t)(kB + j) * n + r0, rl[u], -v[u]);   // (-[W|V])
          st(sb + SL.xv + (size_t)(2 * kB + j) * n + r0, rl[u], v[u]);
        }
        x[u][jj] = ok[u] ? v[u] : 0.0;
      }
    }
    const int jn = c0 + 8;                        // first column to the right of the inner block
    if (jn >= kB) break;
    // ---- M[i][c] = v_i . P[:, c]: first the block's own columns (the Gram matrix of its reflectors), then the columns
    // to the right, CU at a time so that their loads are in flight together; wave partials -> LDS, summed below
#pragma unroll
    for (int ci = 0; ci < 8; ++ci) {
      double pr[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        double acc = 0.0;
#pragma unroll
        for (int u = 0; u < RU; ++u) acc += x[u][i] * x[u][ci];
        pr[i] = acc;
      }
      const double ps = wave_reduce8(pr);
      if (lane < 8) part[((size_t)wv * kB + c0 + ci) * 8 + wave_reduce8_index(lane)] = ps;
    }
    for (int cb = jn; cb < kB; cb += CU) {
      double a[CU][RU];
#pragma unroll
      for (int k = 0; k < CU; ++k)
#pragma unroll
        for (int u = 0; u < RU; ++u) a[k][u] = ld(P + (size_t)std::min(cb + k, kB - 1) * n, rc[u]);
#pragma unroll
      for (int k = 0; k < CU; ++k) {
        double pr[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          double acc = 0.0;
#pragma unroll
          for (int u = 0; u < RU; ++u) acc += ok[u] ? x[u][i] * a[k][u] : 0.0;
          pr[i] = acc;
        }
        const double ps = wave_reduce8(pr);
        if (lane < 8 && cb + k < kB) part[((size_t)wv * kB + cb + k) * 8 + wave_reduce8_index(lane)] = ps;
      }
    }
    __syncthreads();
    for (int idx = tid; idx < 8 * (kB - c0); idx += kWgThreads) {
      const int i = idx & 7, c = c0 + (idx >> 3);
      double acc = 0.0;
#pragma unroll
      for (int w2 = 0; w2 < kWgWaves; ++w2) acc += part[((size_t)w2 * kB + c) * 8 + i];
      Ms[i * kB + c] = acc;
    }
    __syncthreads();
    // W = T^T M for the columns to the right without forming T: (D + striu(G))^T W = M with D = diag(1 / tau) and
    // G[l][i] = Ms[l][c0 + i] the Gram matrix of the block's reflectors, i.e. W[i] = tau_i (M[i] - sum_{l < i} G[l][i] W[l])
    // (rows of tau = 0 reflectors come out zero, as in larft's T); one thread per column, in place
    if (tid >= jn && tid < kB) {
      double wcol[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        double acc = Ms[i * kB + tid];
#pragma unroll
        for (int l = 0; l < i; ++l) acc -= Ms[l * kB + c0 + i] * wcol[l];
        wcol[i] = tauL[i] * acc;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) Ms[i * kB + tid] = wcol[i];
    }
    __syncthreads();
    // P[:, c] -= V W[:, c]
    for (int cb = jn; cb < kB; cb += CU) {
      double a[CU][RU];
#pragma unroll
      for (int k = 0; k < CU; ++k)
#pragma unroll
        for (int u = 0; u < RU; ++u) a[k][u] = ld(P + (size_t)std::min(cb + k, kB - 1) * n, rc[u]);
#pragma unroll
      for (int k = 0; k < CU; ++k) {
        const int c = std::min(cb + k, kB - 1);
        double wcol[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) wcol[i] = Ms[i * kB + c];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
          double s2 = 0.0;
#pragma unroll
          for (int i = 0; i < 8; ++i) s2 += x[u][i] * wcol[i];
          if (ok[u] && rl[u] >= c0 && cb + k < kB) st(P + (size_t)c * n, rl[u], a[k][u] - s2);
        }
      }
    }
    __syncthreads();   // (the next inner block reads what this thread has just written to the same rows; the barrier
                       // separates the reuse of the LDS buffers)
  }
}

// ---- tall panels of a FEW matrices: the panel QR by several workgroups of one launch -------------------------------
// A panel of more than 4096 rows of one matrix (C5: up to 24 000; a single N = 2000 structure: 5 936) went through the
// chunked launches above: 80 dependent launches of ~8-10 us per panel, 0.77 ms per panel whatever its height (C5: 288 ms
// of a 1.45 s solve, a single n = 6000 solve: 52 of 190 ms).  One workgroup cannot take such a panel -- it would stream
// it at the rate of one CU.  Here G = ceil(m / 256) workgroups own 256 rows each, FOR THE WHOLE PANEL: the rows sit in
// LDS (64 columns x 256 rows = 131 KB), loaded once and never re-read from memory, the 8 columns of the inner block in
// registers as in k_panel_wg, and every sum over the rows of the panel is an exchange of 16-byte RECORDS
// {value, sequence number} between the workgroups: written and read as ONE access (global_store / global_load_dwordx4
// with sc1: agent scope, coherent across the XCDs without any fence or cache write-back -- the value and the tag that
// says it is this step's arrive together).  Same arithmetic as k_panel_wg (tail Gram row + pivot row per column, the
// inner block's reflectors applied to the columns on its right as one block update), other reduction trees:
//   * per column: wave partials -> LDS -> the workgroup's 8 sums (+ workgroup 0: the pivot row) as 16 records; every
//     workgroup polls the records of all G workgroups (the four waves a quarter each), sums them in the same order;
//   * per inner block: M = V^T P for the columns on the right (up to 8 x 56 values + the block's 8 x 8 Gram matrix) by
//     threads that own a COLUMN and a quarter of the rows (no cross-lane reduction: the column stride of 257 doubles
//     makes both the row-parallel and the column-parallel LDS access conflict-free); the sum over the workgroups in two
//     hops (value i is summed by workgroup i mod G, which publishes the total), because all-to-all would be G x 8 KB
//     of records per workgroup.
// All G workgroups must be resident together (each waits for all others): G <= 128 and the launch rule keeps
// matrices x G well below the number of CUs; a wait that runs into its bound (never expected: seconds) raises a flag that
// every workgroup sees in its polls, the kernel ends, the host returns an error and the context does not use the kernel
// again.  Sequence numbers are unique within a solve ((panel + 1) * 128 + step) and the records are zeroed per solve.
constexpr int kCoopRows = sc_host::kCoopRows;
constexpr int kCoopLd = kCoopRows + 1;
constexpr int kCoopVals = sc_host::kCoopVals;     // values of one block exchange (M and the Gram matrix)
constexpr size_t kCoopLdsBytes = lds_bytes(sc_host::lds_panel_coop().total);
using sc_host::coop_recs_per_matrix;              // 16-byte records of one matrix (their layout: sy2sb_plan.h)

__device__ __forceinline__ void st16_agent(void* p, double v, int tag) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const v4i r = {(int)(unsigned)b, (int)(unsigned)(b >> 32), tag, 0};
  asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(r) : "memory");
}
__device__ __forceinline__ double rec_value(v4i r) {
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)r.y << 32) | (unsigned)r.x));
}
// one record, polled until it carries `want` (false: the abort flag is up or the bound was reached)
__device__ __forceinline__ bool poll_rec(const v4i* p, int want, int* ctl, double* out) {
  long spins = 0;
  while (true) {
    v4i r;
    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(r) : "v"(p) : "memory");
    if (r.z == want) { *out = rec_value(r); return true; }
    ++spins;
    if ((spins & 63) == 0 && __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return false;
    if (spins > (1L << 22)) {
      // (what was waited for, for the host's message: kind 2 = a block record, the tag wanted, the tag seen, the record)
      if (atomicCAS(ctl, 0, 1) == 0) { ctl[1] = 2; ctl[2] = want; ctl[3] = r.z; ctl[4] = (int)(p - (const v4i*)nullptr); ctl[5] = blockIdx.x; }
      return false;
    }
  }
}
// The 16 column records of the workgroups g = w, w + 4, ... (wave w): lane = (g / 4 mod 4) * 16 + value, R rounds of 16
// workgroups; all loads of a poll in flight together.  Returns this wave's share of the 16 sums in lanes 0-15 (every lane
// l holds the sum of value l & 15).
template <int R>
__device__ __forceinline__ bool poll_cols(const v4i* base, int G, int w, int lane, int want, int* ctl, double* out) {
  const int v = lane & 15, q = lane >> 4;
  const v4i* ptr[R];
  bool need[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int g = w + 4 * (q + 4 * r);
    need[r] = g < G;
    ptr[r] = base + (size_t)(need[r] ? g : 0) * 16 + v;
  }
  v4i rec[R];
  long spins = 0;
  while (true) {
#pragma unroll
    for (int r = 0; r < R; ++r) asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(rec[r]) : "v"(ptr[r]) : "memory");
    if constexpr (R == 1) asm volatile("s_waitcnt vmcnt(0)" : "+v"(rec[0])::"memory");
    if constexpr (R == 2) asm volatile("s_waitcnt vmcnt(0)" : "+v"(rec[0]), "+v"(rec[1])::"memory");
    if constexpr (R == 3) asm volatile("s_waitcnt vmcnt(0)" : "+v"(rec[0]), "+v"(rec[1]), "+v"(rec[2])::"memory");
    if constexpr (R == 4) asm volatile("s_waitcnt vmcnt(0)" : "+v"(rec[0]), "+v"(rec[1]), "+v"(rec[2]), "+v"(rec[3])::"memory");
    if constexpr (R == 6)
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(rec[0]), "+v"(rec[1]), "+v"(rec[2]), "+v"(rec[3]), "+v"(rec[4]), "+v"(rec[5])::"memory");
    if constexpr (R == 8)
      asm volatile("s_waitcnt vmcnt(0)"
                   : "+v"(rec[0]), "+v"(rec[1]), "+v"(rec[2]), "+v"(rec[3]), "+v"(rec[4]), "+v"(rec[5]), "+v"(rec[6]), "+v"(rec[7])::"memory");
    bool fresh = true;
#pragma unroll
    for (int r = 0; r < R; ++r) fresh = fresh && (!need[r] || rec[r].z == want);
    if (__all(fresh)) break;
    ++spins;
    if ((spins & 63) == 0 && __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return false;
    if (spins > (1L << 22)) {
      if (lane == 0 && atomicCAS(ctl, 0, 1) == 0) { ctl[1] = 1; ctl[2] = want; ctl[3] = rec[0].z; ctl[4] = w; ctl[5] = blockIdx.x; }
      return false;
    }
  }
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) s += need[r] ? rec_value(rec[r]) : 0.0;
  s += __shfl_xor(s, 16);
  s += __shfl_xor(s, 32);
  *out = s;
  return true;
}

__global__ __launch_bounds__(kCoopRows) void k_panel_coop(double* __restrict__ a_all, long long stride_a,
                                                          double* __restrict__ tri_all, TriLayout TL,
                                                          double* __restrict__ sb_all, SbLayout SL, int j0, int G,
                                                          v4i* __restrict__ recs_all, int* __restrict__ ctl, int seq_base) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr sc_host::LdsPanelCoop lds = sc_host::lds_panel_coop();
  static_assert(lds.Vl == kB * kCoopLd, "rows of the panel image");
  double* Pl = sm + lds.Pl;                 // [kB][kCoopLd]  the workgroup's rows of the panel
  double* Vl = sm + lds.Vl;                 // [256][8]       the inner block's reflectors by row; then partial sums
  double* Ms = sm + lds.Ms;                 // [8][kB]        M, then W = T^T M
  double* red = sm + lds.red;               // [2][4][8]
  double* piv = sm + lds.piv;               // [2][8]
  double* tauA = sm + lds.tauA;             // [kB]           tau of every column (stored at the end)
  double* tot4 = sm + lds.tot4;             // [2][4][16]
  int* s_dead = reinterpret_cast<int*>(sm + lds.dead);
  const int n = TL.n;
  const int r0 = j0 + kB, m = n - r0;
  const int g = blockIdx.x, mat = blockIdx.y;
  double* A = a_all + (size_t)mat * stride_a;
  double* tri = tri_all + (size_t)mat * TL.slab;
  double* sb = sb_all + (size_t)mat * SL.slab;
  // (round 6: one control record of 8 ints per matrix -- [0] the abort flag its workgroups poll, [1..5] what was waited
  // for --, so that a matrix whose wait timed out does not stop the matrices beside it half-way through their stores)
  ctl += 8 * (int)blockIdx.y;
  if (__hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;   // given up in an earlier panel: k_panel_serial
  v4i* colrec = recs_all + (size_t)mat * coop_recs_per_matrix(G);
  v4i* mrec = colrec + (size_t)2 * G * 16;
  v4i* trec = mrec + (size_t)G * kCoopVals;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  double* P = A + (size_t)j0 * n + r0;
  const int row = g * kCoopRows + tid;      // my row of the panel
  const bool ok = row < m;
  const int rc = min(row, m - 1);
  const int R = (G + 15) / 16;
  typedef char __attribute__((address_space(1)))* gbp;
  typedef double __attribute__((address_space(1)))* gdp;
  typedef const double __attribute__((address_space(1)))* gdp_c;
  auto off = [&](int rr) -> unsigned {
    unsigned e = 8u * (unsigned)rr;
    asm volatile("" : "+v"(e));
    return e;
  };
  auto st = [&](double* colbase, int rr, double val) { *(gdp)((gbp)colbase + off(rr)) = val; };
  if (tid == 0) *s_dead = 0;
  for (int c = 0; c < kB; ++c) {
    const double v = *(gdp_c)((gbp)(P + (size_t)c * n) + off(rc));
    Pl[c * kCoopLd + tid] = ok ? v : 0.0;
  }
  lds_barrier();

  for (int c0 = 0; c0 < kB; c0 += 8) {
    double x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = Pl[(c0 + i) * kCoopLd + tid];
    // ---- the inner block's 8 reflectors
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const int j = c0 + jj;
      const int pb = jj & 1;
      double gr[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) gr[c] = (c >= jj && row > j) ? x[jj] * x[c] : 0.0;
      const double gs = wave_reduce8(gr);
      if (lane < 8) red[(pb * 4 + wv) * 8 + wave_reduce8_index(lane)] = gs;
      if (row == j) {
#pragma unroll
        for (int c = 0; c < 8; ++c) piv[pb * 8 + c] = x[c];
      }
      lds_barrier();
      if (wv == 0 && lane < 16) {
        double val;
        if (lane < 8) val = (red[(pb * 4 + 0) * 8 + lane] + red[(pb * 4 + 1) * 8 + lane]) + (red[(pb * 4 + 2) * 8 + lane] + red[(pb * 4 + 3) * 8 + lane]);
        else val = g == 0 ? piv[pb * 8 + lane - 8] : 0.0;
        st16_agent(colrec + ((size_t)pb * G + g) * 16 + lane, val, seq_base + 1 + j);
      }
      {
        const v4i* base = colrec + (size_t)pb * G * 16;
        double s = 0.0;
        bool good;
        switch (R) {
          case 1: good = poll_cols<1>(base, G, wv, lane, seq_base + 1 + j, ctl, &s); break;
          case 2: good = poll_cols<2>(base, G, wv, lane, seq_base + 1 + j, ctl, &s); break;
          case 3: good = poll_cols<3>(base, G, wv, lane, seq_base + 1 + j, ctl, &s); break;
          case 4: good = poll_cols<4>(base, G, wv, lane, seq_base + 1 + j, ctl, &s); break;
          case 5: case 6: good = poll_cols<6>(base, G, wv, lane, seq_base + 1 + j, ctl, &s); break;
          default: good = poll_cols<8>(base, G, wv, lane, seq_base + 1 + j, ctl, &s); break;
        }
        if (lane < 16) tot4[(pb * 4 + wv) * 16 + lane] = s;
        if (!good && lane == 0) *s_dead = 1;
      }
      lds_barrier();
      if (*s_dead) return;
      // the 16 totals: lane l < 16 of every wave adds the four waves' shares of value l, the others take them from that
      // lane through scalar registers
      double fin[8], pv[8];
      {
        const int l16 = lane & 15;
        const double t = (tot4[(pb * 4 + 0) * 16 + l16] + tot4[(pb * 4 + 1) * 16 + l16]) +
                         (tot4[(pb * 4 + 2) * 16 + l16] + tot4[(pb * 4 + 3) * 16 + l16]);
        const unsigned long long tb = (unsigned long long)__double_as_longlong(t);
#pragma unroll
        for (int c = 0; c < 16; ++c) {
          const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)tb, c);
          const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(tb >> 32), c);
          const double val = __longlong_as_double((long long)(((unsigned long long)hi << 32) | (unsigned long long)lo));
          if (c < 8) fin[c] = val; else pv[c - 8] = val;
        }
      }
      const HH h = householder(pv[jj], fin[jj]);
      if (tid == 0) tauA[j] = h.tau;
      const double v = row > j ? h.scale * x[jj] : (row == j ? 1.0 : 0.0);
#pragma unroll
      for (int c = jj + 1; c < 8; ++c) {
        const double wc = h.tau * (pv[c] + h.scale * fin[c]);
        x[c] -= v * wc;
      }
      // column j is final.  It stays in LDS in the form the matrix takes it (R entries above the pivot, beta at it, v below);
      // NOTHING is stored to memory inside the loop: a poll waits for vmcnt(0), i.e. for every store of the wave in flight
      Pl[j * kCoopLd + tid] = row > j ? v : (row == j ? h.beta : x[jj]);
      x[jj] = ok ? v : 0.0;
    }
    const int jn = c0 + 8;
    if (jn >= kB) break;
    const int ncols = kB - c0;               // the block's own columns (their Gram matrix) + the columns on the right
    const int nvals = 8 * ncols;
    const int blk = c0 >> 3;
    // ---- V by row (for the broadcast reads below; the block's own columns -- their Gram matrix -- are read from here too)
#pragma unroll
    for (int i = 0; i < 8; ++i) Vl[tid * 8 + i] = x[i];
    lds_barrier();
    // ---- M[i][c] = v_i . P[:, c] over this workgroup's rows: thread = (column, quarter of the rows)
    {
      const int c = tid & 63, q = tid >> 6;
      double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (c < ncols) {
        const double* vr = Vl + q * 64 * 8;
        const double* pc = c < 8 ? vr + c : Pl + (c0 + c) * kCoopLd + q * 64;
        const int stp = c < 8 ? 8 : 1;
#pragma unroll 4
        for (int rr = 0; rr < 64; ++rr) {
          const double pval = pc[rr * stp];
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[i] += vr[rr * 8 + i] * pval;
        }
      }
      lds_barrier();                        // (the partial sums take the place of V by row)
      if (c < ncols) {
#pragma unroll
        for (int i = 0; i < 8; ++i) Vl[(q * 64 + c) * 8 + i] = acc[i];
      }
    }
    lds_barrier();
    for (int idx = tid; idx < nvals; idx += kCoopRows) {
      const double t = (Vl[idx] + Vl[64 * 8 + idx]) + (Vl[2 * 64 * 8 + idx] + Vl[3 * 64 * 8 + idx]);
      st16_agent(mrec + (size_t)g * kCoopVals + idx, t, seq_base + 65 + blk);
    }
    lds_barrier();
    // ---- hop 1: value idx is summed by workgroup idx mod G
    bool good = true;
    const int nown = g < nvals ? (nvals - g + G - 1) / G : 0;
    for (int pi = tid; pi < nown * G; pi += kCoopRows) {
      const int k = pi / G, gg = pi - k * G;
      double val = 0.0;
      good = poll_rec(mrec + (size_t)gg * kCoopVals + (g + k * G), seq_base + 65 + blk, ctl, &val) && good;
      Vl[pi] = val;
    }
    if (!good) *s_dead = 1;
    lds_barrier();
    if (*s_dead) return;
    for (int k = tid; k < nown; k += kCoopRows) {
      double acc = 0.0;
      for (int gg = 0; gg < G; ++gg) acc += Vl[k * G + gg];
      st16_agent(trec + (g + k * G), acc, seq_base + 73 + blk);
    }
    // ---- hop 2: the totals
    for (int idx = tid; idx < nvals; idx += kCoopRows) {
      double val = 0.0;
      good = poll_rec(trec + idx, seq_base + 73 + blk, ctl, &val) && good;
      Ms[(idx & 7) * kB + c0 + (idx >> 3)] = val;
    }
    if (!good) *s_dead = 1;
    lds_barrier();
    if (*s_dead) return;
    // W = T^T M for the columns on the right (as in k_panel_wg): one thread per column, in place
    if (tid >= jn && tid < kB) {
      double wcol[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        double acc = Ms[i * kB + tid];
#pragma unroll
        for (int l = 0; l < i; ++l) acc -= Ms[l * kB + c0 + i] * wcol[l];
        wcol[i] = tauA[c0 + i] * acc;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) Ms[i * kB + tid] = wcol[i];
    }
    lds_barrier();
    // P[:, c] -= V W[:, c] on my row
    for (int c = jn; c < kB; ++c) {
      double s2 = 0.0;
#pragma unroll
      for (int i = 0; i < 8; ++i) s2 += x[i] * Ms[i * kB + c];
      Pl[c * kCoopLd + tid] -= s2;
    }
    // (the next block reads its own row of Pl; Ms is still being read here by slower waves when a fast one is through
    // the next block's first barriers and writes it again: one barrier)
    lds_barrier();
  }
  // ---- the panel -> memory: the matrix' columns, and V in its explicit form into the three panel buffers
  lds_barrier();
  if (g == 0 && tid < kB) tri[TL.tau + j0 + tid] = tauA[tid];
  if (ok) {
    for (int c = 0; c < kB; ++c) {
      const double val = Pl[c * kCoopLd + tid];
      const double v = row > c ? val : (row == c ? 1.0 : 0.0);
      st(P + (size_t)c * n, row, val);
      st(sb + SL.vw + (size_t)c * n + r0, row, v);
      st(sb + SL.wv + (size_t)(kB + c) * n + r0, row, -v);   // (-[W|V])
      st(sb + SL.xv + (size_t)(2 * kB + c) * n + r0, row, v);
    }
  }
}

// The take-over of k_panel_coop, enqueued behind every one of its launches (round 6; until then a time-out failed the
// solve).  Workgroup b looks at matrix b's control record and returns unless its abort flag is up -- always, in practice.
// Otherwise the panel is intact in memory (k_panel_coop stores nothing before its last exchange has succeeded) and is
// factored here by this ONE workgroup, from memory, column by column: norm and pivot, reflector, the columns on the right
// eight at a time (w = tau (v^T P), P -= v w) -- slow (the panel is streamed 64 / 8 + 1 times per column group) and only
// there so that a solve whose cooperative launch could not get its workgroups resident together (another stream or
// process holds CUs with a persistent kernel of its own) still ends with LAPACK's numbers.  The flag stays up for the
// rest of the solve; the event is counted in stats[5] and the context keeps to the chunked launches afterwards.
__global__ __launch_bounds__(1024) void k_panel_serial(double* __restrict__ a_all, long long stride_a,
                                                       double* __restrict__ tri_all, TriLayout TL,
                                                       double* __restrict__ sb_all, SbLayout SL, int j0,
                                                       const int* __restrict__ ctl, unsigned long long* __restrict__ stats) {
  __shared__ double red[16 * 9];
  __shared__ double s_w[8];
  __shared__ double s_tau, s_beta, s_scale;
  const int mat = blockIdx.x;
  if (ctl[8 * mat] == 0) return;
  const int n = TL.n;
  const int r0 = j0 + kB, m = n - r0;
  double* A = a_all + (size_t)mat * stride_a;
  double* tri = tri_all + (size_t)mat * TL.slab;
  double* sb = sb_all + (size_t)mat * SL.slab;
  double* P = A + (size_t)j0 * n + r0;      // P(r, c) at P[c * n + r], r = 0 .. m - 1, c = 0 .. kB - 1
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) atomicAdd(stats + 5, 1ull);
  // sum of up to 8 values per thread over the workgroup: wave sums, then 16 partials per value
  auto block_sum8 = [&](double (&a)[8], int cnt) {
    for (int i = 0; i < cnt; ++i) {
      const double t = wave_sum(a[i]);
      if (lane == 0) red[wv * 9 + i] = t;
    }
    __syncthreads();
    for (int i = 0; i < cnt; ++i) {
      double t = 0.0;
      for (int w = 0; w < 16; ++w) t += red[w * 9 + i];
      a[i] = t;
    }
    __syncthreads();
  };
  for (int j = 0; j < kB; ++j) {
    double* pj = P + (size_t)j * n;
    {
      double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int r = j + 1 + tid; r < m; r += 1024) a[0] += pj[r] * pj[r];
      block_sum8(a, 1);
      if (tid == 0) {
        const HH h = householder(pj[j], a[0]);
        s_tau = h.tau; s_beta = h.beta; s_scale = h.scale;
        tri[TL.tau + j0 + j] = h.tau;
      }
      __syncthreads();
    }
    const double tau = s_tau, scale = s_scale;
    for (int c0 = j + 1; c0 < kB; c0 += 8) {
      const int cnt = min(8, kB - c0);
      double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int r = j + 1 + tid; r < m; r += 1024) {
        const double x = pj[r];
        for (int i = 0; i < cnt; ++i) a[i] += x * P[(size_t)(c0 + i) * n + r];
      }
      block_sum8(a, cnt);
      if (tid < cnt) s_w[tid] = tau * (P[(size_t)(c0 + tid) * n + j] + scale * a[tid]);
      __syncthreads();
      for (int r = j + tid; r < m; r += 1024) {
        const double v = r > j ? scale * pj[r] : 1.0;
        for (int i = 0; i < cnt; ++i) P[(size_t)(c0 + i) * n + r] -= v * s_w[i];
      }
      __syncthreads();
    }
    // column j in the form the matrix takes it: R above the pivot (untouched), beta at it, v below
    for (int r = j + tid; r < m; r += 1024) pj[r] = r > j ? scale * pj[r] : s_beta;
    __syncthreads();
  }
  // V in its explicit form into the three panel buffers (as k_panel_coop's last loop)
  for (int c = 0; c < kB; ++c)
    for (int r = tid; r < m; r += 1024) {
      const double val = P[(size_t)c * n + r];
      const double v = r > c ? val : (r == c ? 1.0 : 0.0);
      sb[SL.vw + (size_t)c * n + r0 + r] = v;
      sb[SL.wv + (size_t)(kB + c) * n + r0 + r] = -v;
      sb[SL.xv + (size_t)(2 * kB + c) * n + r0 + r] = v;
    }
}

// X1 / X2 = sum of their K slices (split-K SYMM, few matrices): blockIdx.y = column of [X1 | X2], rows r0 .. n - 1
__global__ __launch_bounds__(256) void k_sum_xslices(double* __restrict__ sb_all, SbLayout SL, int r0) {
  const int n = SL.n, p = SL.symm_split;
  double* sb = sb_all + (size_t)blockIdx.z * SL.slab;
  const int which = blockIdx.y / kB, c = blockIdx.y % kB;
  const int r = r0 + blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const double* src = sb + SL.xsplit + (size_t)which * p * n * kB + (size_t)c * n + r;
  double s = 0.0;
  for (int q = 0; q < p; ++q) s += src[(size_t)q * n * kB];
  sb[SL.xv + (size_t)(which * kB + c) * n + r] = s;
}

// second panel of a pair: P2 = [W1|V1]^T V2 (128 x 64) from its split-K slices
__global__ __launch_bounds__(256) void k_sum_p2(double* __restrict__ sb_all, SbLayout SL) {
  double* sb = sb_all + (size_t)blockIdx.y * SL.slab;
  const int i = blockIdx.x * 256 + threadIdx.x;   // 0 .. 2 kB kB - 1
  double acc = 0.0;
#pragma unroll
  for (int sl = 0; sl < kSmallSplit; ++sl) acc += sb[SL.small2 + (size_t)sl * 2 * kB * kB + i];
  sb[SL.p2 + i] = acc;
}

// One workgroup per matrix: T (larft, forward columnwise) from tau and G = V^T V;  S = T^T (V^T X) T;
// C = [T; T; -S/2]  (3 kB x kB, column-major), the right-hand factor of  W = [X1 | X2 | V] C.
__global__ __launch_bounds__(1024) void k_sb_small(const double* __restrict__ tri_all, TriLayout TL,
                                                   double* __restrict__ sb_all, SbLayout SL, int j0) {
  // One workgroup per matrix, on the critical path of every panel (QR -> SYMM -> Gram -> this -> W -> trailing update):
  // 1024 threads and a T factor by halving (16 x 16 diagonal blocks by substitution, then T12 = -T11 G12 T22 twice)
  // instead of 256 threads and larft's 64 dependent columns: 150-240 us -> see DESIGN section 7.
  constexpr int LD = kB + 1;
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr sc_host::LdsSbSmall lds = sc_host::lds_sb_small();
  double* G = sm + lds.G;         // [kB][LD]  G[i * LD + j]
  double* M1 = sm + lds.M1;
  double* T = sm + lds.T;
  double* U = sm + lds.U;
  const double* tri = tri_all + (size_t)blockIdx.x * TL.slab;
  double* sb = sb_all + (size_t)blockIdx.x * SL.slab;
  const int tid = threadIdx.x, nthr = blockDim.x;
  // the split-K product is (kB x 3 kB), column-major ld kB: columns [X1 | X2 | V]
  const double* prod = sb + SL.small;
  const size_t slice = (size_t)kB * 3 * kB;
  for (int idx = tid; idx < kB * kB; idx += nthr) {
    const int i = idx & 63, jj = idx >> 6;
    double g = 0.0, x = 0.0;
#pragma unroll
    for (int s = 0; s < kSmallSplit; ++s) {
      const double* ps = prod + s * slice;
      x += ps[i + (size_t)jj * kB] + ps[i + (size_t)(kB + jj) * kB];
      g += ps[i + (size_t)(2 * kB + jj) * kB];
    }
    G[i * LD + jj] = g;
    M1[i * LD + jj] = x;
    T[i * LD + jj] = 0.0;
  }
  __syncthreads();
  // ---- T = the compact-WY factor of the panel's reflectors: (D + striu(G)) T = I row by row, i.e.
  // T[i][c] = tau_i (delta_ic - sum_{l > i} G[i][l] T[l][c])  (larft's T; rows of tau = 0 reflectors come out zero).
  // Diagonal 16 x 16 blocks: one thread per column, rows bottom-up, the column in registers.
  if (tid < kB) {
    const int bb = tid >> 4, c = tid & 15, o = bb * 16;
    double x[16];
#pragma unroll
    for (int i = 15; i >= 0; --i) {
      double acc = (i == c) ? 1.0 : 0.0;
#pragma unroll
      for (int l = i + 1; l < 16; ++l) acc -= G[(o + i) * LD + o + l] * x[l];
      x[i] = i <= c ? tri[TL.tau + j0 + o + i] * acc : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) T[(o + i) * LD + o + c] = x[i];
  }
  __syncthreads();
  // off-diagonal blocks by halving: T12 = -T11 (G12 T22), block sizes 16 then 32 (U serves as the scratch for G12 T22)
#pragma unroll
  for (int bs = 16; bs <= 32; bs *= 2) {
    const int npair = kB / (2 * bs);                 // 2 pairs of 16-blocks, then 1 pair of 32-blocks
    for (int idx = tid; idx < npair * bs * bs; idx += nthr) {
      const int pr = idx / (bs * bs), e = idx % (bs * bs), i = e / bs, jj = e % bs;
      const int o1 = pr * 2 * bs, o2 = o1 + bs;
      double acc = 0.0;
      for (int l = 0; l <= jj; ++l) acc += G[(o1 + i) * LD + o2 + l] * T[(o2 + l) * LD + o2 + jj];   // T22 upper triangular
      U[(o1 + i) * LD + o2 + jj] = acc;
    }
    __syncthreads();
    for (int idx = tid; idx < npair * bs * bs; idx += nthr) {
      const int pr = idx / (bs * bs), e = idx % (bs * bs), i = e / bs, jj = e % bs;
      const int o1 = pr * 2 * bs, o2 = o1 + bs;
      double acc = 0.0;
      for (int l = i; l < bs; ++l) acc += T[(o1 + i) * LD + o1 + l] * U[(o1 + l) * LD + o2 + jj];    // T11 upper triangular
      T[(o1 + i) * LD + o2 + jj] = -acc;
    }
    __syncthreads();
  }
  // U = M1 T ; S = T^T U
  for (int idx = tid; idx < kB * kB; idx += nthr) {
    const int i = idx >> 6, jj = idx & 63;
    double s = 0.0;
    for (int l = 0; l <= jj; ++l) s += M1[i * LD + l] * T[l * LD + jj];
    U[i * LD + jj] = s;
  }
  __syncthreads();
  double* cm = sb + SL.cmat;   // ld 3 kB
  for (int idx = tid; idx < kB * kB; idx += nthr) {
    const int i = idx & 63, jj = idx >> 6;
    double s = 0.0;
    for (int l = 0; l <= i; ++l) s += T[l * LD + i] * U[l * LD + jj];
    const double t = T[i * LD + jj];
    cm[i + (size_t)jj * 3 * kB] = t;
    cm[kB + i + (size_t)jj * 3 * kB] = t;
    cm[2 * kB + i + (size_t)jj * 3 * kB] = -0.5 * s;
  }
}

}  // namespace

// ================================================================================================================
// Host side of stage 1.  Which kernel form a panel gets: twostage_policy.h; the records, their places and every LDS size:
// sy2sb_plan.h.

// What a panel needs of its solve.
struct PanelRun {
  sc_ctx* ctx;
  hipStream_t st;   // the solve's own stream
  double* d_a; long long stride_a; int n, batch;
  double* d_tri_ws; const TriLayout& TL;
  double* d_sb_ws; const SbLayout& SL;
  const GemmDesc* d_descs;
  const std::vector<int>& role;
  sc_host::CoopPlan coop;
  v4i* coop_recs;   // null: no k_panel_coop in this solve
  int* coop_ctl;
  bool use_symm3;
  int symm3_nb_min;
  SbTimers& t;
};

// The QR of panel p of the matrices [lo, lo + nb) on `ps`, in the form the policy names.
static int launch_panel_qr(const PanelRun& R, int p, int lo, int nb, hipStream_t ps) {
  using sc_host::PanelQr;
  sc_ctx* ctx = R.ctx;
  const TriLayout& TL = R.TL;
  const long long stride_a = R.stride_a;
  const sc_host::PanelGeom g = sc_host::panel_geom(R.n, p);
  const int j0 = g.j0, nr = g.nr;
  double* a_h = R.d_a + (size_t)lo * stride_a;
  double* tri_h = R.d_tri_ws + (size_t)lo * TL.slab;
  double* sb_h = R.d_sb_ws + (size_t)lo * R.SL.slab;
  const dim3 qgrid((unsigned)g.nchunks, (unsigned)nb);
  SbLayout SQ = R.SL;   // where the panel QR leaves V: the second panel of a pair uses the second half of [V|W..], [W|V..]
  if (R.role[(size_t)p] == 2) { SQ.vw += (long long)2 * kB * R.n; SQ.wv += (long long)2 * kB * R.n; }
  const sc_host::PanelQrForm F =
      sc_host::panel_qr_form(sc_host::two_stage_env(), R.coop, R.coop_recs != nullptr, g.m, nb, ps == R.st);
  // k_panel_wg<ru, cu, nt>: one workgroup per matrix
  auto wg = [&](void (*kernel)(double*, long long, double*, TriLayout, double*, SbLayout, int), int nt) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)nb), dim3((unsigned)nt), lds_bytes(sc_host::lds_panel_wg(nt).total), ps, a_h,
                       stride_a, tri_h, TL, sb_h, SQ, j0);
  };
  switch (F.kind) {
    case PanelQr::Coop: {
      const int coop_g = F.coop_g;
      // (test hook, sc_dbg_set_panel_coop_fail: from this panel on the matrices' abort flags are up, as after a time-out)
      if (p == ctx->coop_fail_panel) SC_HIP(ctx, hipMemsetAsync(R.coop_ctl + 8 * lo, 1, sizeof(int) * 8 * nb, ps));
      hipLaunchKernelGGL(k_panel_coop, dim3((unsigned)coop_g, (unsigned)nb), dim3(kCoopRows), kCoopLdsBytes, ps, a_h, stride_a,
                         tri_h, TL, sb_h, SQ, j0, coop_g, R.coop_recs + (size_t)lo * coop_recs_per_matrix(coop_g),
                         R.coop_ctl + 8 * lo, (p + 1) * 128);
      // the take-over: returns at once unless a wait of the launch above (or of an earlier panel) timed out
      hipLaunchKernelGGL(k_panel_serial, dim3((unsigned)nb), dim3(1024), 0, ps, a_h, stride_a, tri_h, TL, sb_h, SQ, j0,
                         (const int*)(R.coop_ctl + 8 * lo), ctx->d_status);
      ++ctx->cnt_coop_launches;
      break;
    }
    case PanelQr::Wg1024:
      ++ctx->cnt_panel_form[std::max(1, std::min(F.ru, 4)) - 1];
      if (F.ru == 1) wg(k_panel_wg<1, 8>, 1024);
      else if (F.ru == 2) wg(k_panel_wg<2, 8>, 1024);
      else if (F.ru == 3) wg(k_panel_wg<3, 4>, 1024);
      else wg(k_panel_wg<4, 2>, 1024);
      break;
    case PanelQr::Wg512:
      ++ctx->cnt_panel_form[F.ru == 10 ? 4 : 5];
      if (F.ru == 10) wg(k_panel_wg<10, 1, 512>, 512);
      else wg(k_panel_wg<12, 1, 512>, 512);
      break;
    case PanelQr::Blocked: {
      // blocked panel: inner blocks of 8 columns, their reflectors applied to the rest of the panel at once
      const size_t lds_qr_blk = lds_bytes(sc_host::lds_panel_qr(kIb + 1).total);
      ++ctx->cnt_panel_form[6];
      hipLaunchKernelGGL(k_panel_qr, qgrid, dim3(256), lds_qr_blk, ps, a_h, stride_a, tri_h, TL, sb_h, SQ, j0, 0, nr, kIb);
      for (int c0 = 0; c0 < kB; c0 += kIb) {
        for (int j = c0 + 1; j < c0 + kIb; ++j)
          hipLaunchKernelGGL(k_panel_qr, qgrid, dim3(256), lds_qr_blk, ps, a_h, stride_a, tri_h, TL, sb_h, SQ, j0, j, nr,
                             c0 + kIb);
        // (their LDS image holds columns c0 .. kB-1 only)
        hipLaunchKernelGGL(k_pqr_blk_a, qgrid, dim3(256), lds_bytes(sc_host::lds_pqr_blk_a(c0).total), ps, a_h, stride_a, tri_h,
                           TL, sb_h, SQ, j0, c0);
        if (c0 + kIb < kB)
          hipLaunchKernelGGL(k_pqr_blk_b, qgrid, dim3(256), lds_bytes(sc_host::lds_pqr_blk_b(c0).total), ps, a_h, stride_a,
                             tri_h, TL, sb_h, SQ, j0, c0);
      }
      break;
    }
    case PanelQr::Unblocked: {
      const size_t lds_qr = lds_bytes(sc_host::lds_panel_qr(kB).total);
      ++ctx->cnt_panel_form[7];
      for (int j = 0; j <= nr; ++j)
        hipLaunchKernelGGL(k_panel_qr, qgrid, dim3(256), lds_qr, ps, a_h, stride_a, tri_h, TL, sb_h, SQ, j0, j, nr, kB);
      break;
    }
  }
  return SC_OK;
}

// One panel of the matrices [lo, hi) on `ps`: QR of the panel, X = A22 V, the small products, W, the trailing update
// its role asks for (single: SYR2K; first of a pair: the next panel's columns only; second: the joint update).
static int run_panel(const PanelRun& R, int p, int lo, int hi, hipStream_t ps, bool timed) {
  using sc_host::SbRec, sc_host::kRecX1, sc_host::kRecX2, sc_host::kRecGram, sc_host::kRecW, sc_host::kRecNegW, sc_host::kRecTrail,
      sc_host::kRecFirst, sc_host::kRecP2, sc_host::kRecCorr;
  sc_ctx* ctx = R.ctx;
  const SbLayout& SL = R.SL;
  const int n = R.n, batch = R.batch, nb = hi - lo;
  const int rl = R.role[(size_t)p];
  const sc_host::PanelGeom g = sc_host::panel_geom(n, p);
  const int j0 = g.j0, r0 = g.r0, m = g.m;
  double* tri_h = R.d_tri_ws + (size_t)lo * R.TL.slab;
  double* sb_h = R.d_sb_ws + (size_t)lo * SL.slab;
  StreamScope scope(ctx, ps);   // launch_gemm_f64 launches on the context's stream
  if (timed) R.t.qr.start();
  SC_TRY(launch_panel_qr(R, p, lo, nb, ps));
  if (timed) R.t.qr.stop();
  if (rl != 0) ++ctx->cnt_panel_role[rl - 1];
  // the records of this launch: one kind of panel p, matrices lo .. hi - 1
  auto rec = [&](SbRec kind) { return R.d_descs + sc_host::stage1_record_index(p, kind, batch, lo); };
  if (timed) R.t.symm.start();
  // X = A22 V: one launch of k_symm3 (X into X1; X2 was zeroed for the whole solve) while the panel has enough tiles
  // for it, else X1 = L V and X2 = strict(L)^T V by two triangular-operand launches of k_gemm2
  if (R.use_symm3 && symm3_would_take(ctx, R.symm3_nb_min, m, SL.symm_split, /*aligned16=*/true) &&
      launch_symm3(ctx, rec(kRecX1), nb, m, SL.symm_split, /*aligned16=*/true, /*any_size=*/true) == SC_OK) {
    if (SL.symm_split > 1)
      hipLaunchKernelGGL(k_sum_xslices, dim3((unsigned)((m + 255) / 256), kB, (unsigned)nb), dim3(256), 0, ps, sb_h, SL, r0);
  } else {
    ++ctx->cnt_symm_tri;
    SC_TRY(launch_gemm_f64(ctx, rec(kRecX1), {.count = nb, .max_m = m, .max_n = kB, .layout = kGemmAmBk, .split_k = SL.symm_split, .tri = true}));
    SC_TRY(launch_gemm_f64(ctx, rec(kRecX2), {.count = nb, .max_m = m, .max_n = kB, .layout = kGemmAkBk, .split_k = SL.symm_split, .tri = true}));
    if (SL.symm_split > 1)
      hipLaunchKernelGGL(k_sum_xslices, dim3((unsigned)((m + 255) / 256), 2 * kB, (unsigned)nb), dim3(256), 0, ps, sb_h, SL, r0);
  }
  if (rl == 2) {   // the trailing matrix has not seen the first panel's update yet: X1 -= [V1|W1] ([W1|V1]^T V2)
    SC_TRY(launch_gemm_f64(ctx, rec(kRecP2), {.count = nb, .max_m = 2 * kB, .max_n = kB, .layout = kGemmAkBk, .split_k = kSmallSplit}));
    hipLaunchKernelGGL(k_sum_p2, dim3((unsigned)(2 * kB * kB / 256), (unsigned)nb), dim3(256), 0, ps, sb_h, SL);
    SC_TRY(launch_gemm_f64(ctx, rec(kRecCorr), {.count = nb, .max_m = m, .max_n = kB, .layout = kGemmAmBk}));
  }
  if (timed) R.t.symm.stop();
  SC_TRY(launch_gemm_f64(ctx, rec(kRecGram), {.count = nb, .max_m = kB, .max_n = 3 * kB, .layout = kGemmAkBk, .split_k = kSmallSplit}));
  hipLaunchKernelGGL(k_sb_small, dim3((unsigned)nb), dim3(1024), lds_bytes(sc_host::lds_sb_small().total), ps, tri_h, R.TL, sb_h, SL, j0);
  static_assert(kRecNegW == kRecW + 1, "W and -W of a whole batch are one launch of 2 * batch records");
  if (nb == batch) {
    SC_TRY(launch_gemm_f64(ctx, rec(kRecW), {.count = 2 * batch, .max_m = m, .max_n = kB, .layout = kGemmAmBk}));
  } else {
    SC_TRY(launch_gemm_f64(ctx, rec(kRecW), {.count = nb, .max_m = m, .max_n = kB, .layout = kGemmAmBk}));
    SC_TRY(launch_gemm_f64(ctx, rec(kRecNegW), {.count = nb, .max_m = m, .max_n = kB, .layout = kGemmAmBk}));
  }
  if (timed) R.t.syr2k.start();
  if (rl == 1)
    SC_TRY(launch_gemm_f64(ctx, rec(kRecFirst), {.count = nb, .max_m = m, .max_n = kB, .layout = kGemmAmBn}));
  else
    // (records of one launch share (m, m, K); operands start at even rows of buffers with even leading dimension n)
    if (launch_gemm3_uniform(ctx, rec(kRecTrail),
                             {.count = nb, .m = m, .n = m, .k = rl == 2 ? 4 * kB : 2 * kB, .layout = kGemmAmBn, .lower = R.use_symm3 ? 2 : 1,
                              .alpha = 1.0, .beta = 1.0, .aligned16 = (n & 1) == 0 && (r0 & 1) == 0}) != SC_OK) {
      ++ctx->cnt_gemm3_declined;
      SC_TRY(launch_gemm_f64(ctx, rec(kRecTrail), {.count = nb, .max_m = m, .max_n = m, .layout = kGemmAmBn, .lower_grid = true}));
    }
  if (timed) R.t.syr2k.stop();
  return SC_OK;
}

// Stage 1 on ctx->stream, the GEMM records of the solve uploaded: dense -> band.
int sb_stage1(sc_ctx* ctx, double* d_a, long long stride_a, int n, int batch, double* d_tri_ws, const TriLayout& TL,
              double* d_sb_ws, const SbLayout& SL, const GemmDesc* d_descs, const std::vector<int>& role, bool prof,
              SbTimers& timers) {
  const sc_host::TwoStageEnv& E = sc_host::two_stage_env();
  hipStream_t st = ctx->stream;
  const int npanels = (int)role.size();

  // tau of columns without a reflector must read 0
  for (int b = 0; b < batch; ++b)
    SC_HIP(ctx, hipMemsetAsync(d_tri_ws + (size_t)b * TL.slab + TL.tau, 0, sizeof(double) * n, st));

  const int s1_parts = sc_host::stage1_parts(E, batch, prof);
  ctx->last_stage1_parts = s1_parts;
  ctx->last_symm_slices = SL.symm_split;
  const sc_host::CoopPlan coop = sc_host::coop_plan(E, n, batch, ctx->num_cus, prof, ctx->coop_min_rows, ctx->coop_ok);
  v4i* coop_recs = nullptr;
  int* coop_ctl = nullptr;
  if (coop.ask) {
    if (ctx->coop_attr < 0)
      ctx->coop_attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_panel_coop),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCoopLdsBytes) == hipSuccess;
    if (ctx->coop_attr == 1 && coop.nb_max >= 1) {
      const sc_host::CoopAux aux = sc_host::coop_aux_carve(batch, coop.gmax);
      SC_TRY(sc_reserve_dc_aux(ctx, aux.total));
      coop_ctl = reinterpret_cast<int*>(reinterpret_cast<char*>(ctx->dc_aux) + aux.ctl);
      coop_recs = reinterpret_cast<v4i*>(reinterpret_cast<char*>(ctx->dc_aux) + aux.recs);
      SC_HIP(ctx, hipMemsetAsync(ctx->dc_aux, 0, aux.total, st));
    }
  }
  // k_symm3 writes X into the X1 block of [X1 | X2 | V]; the X2 block reads zero for the whole solve (the panels at the
  // end of the reduction that fall back to the two triangular-operand launches rewrite their rows of it themselves)
  const bool use_symm3 = sc_host::symm3_for(E, n);
  if (use_symm3)
    for (int b = 0; b < batch; ++b)
      SC_HIP(ctx, hipMemsetAsync(d_sb_ws + (size_t)b * SL.slab + SL.xv + (size_t)kB * n, 0, sizeof(double) * (size_t)kB * n, st));
  // (whether a panel takes k_symm3 is decided for the SMALLEST part of a batch that is split over streams, and then holds
  // for every part: sc_host::stage1_parts)
  const PanelRun R{ctx, st, d_a, stride_a, n, batch, d_tri_ws, TL, d_sb_ws, SL, d_descs, role, coop, coop_recs, coop_ctl,
                   use_symm3, std::max(1, batch / s1_parts), timers};
  if (s1_parts > 1) {
    struct SideBySide {   // (k_gemm3 leaves CUs to the other parts' kernels while this is set: gemm3_would_take)
      sc_ctx* c;
      explicit SideBySide(sc_ctx* c_) : c(c_) { c->gemm3_side_by_side = true; }
      ~SideBySide() { c->gemm3_side_by_side = false; }
    } side_by_side(ctx);
    SideFork parts(ctx, st);
    SC_TRY(parts.fork(s1_parts));
    int rc_parts = SC_OK;
    for (int p = 0; p < npanels && rc_parts == SC_OK; ++p)
      for (int q = 0; q < s1_parts && rc_parts == SC_OK; ++q) {
        const sc_host::PartBounds pb = sc_host::part_bounds(batch, s1_parts, q);
        rc_parts = run_panel(R, p, pb.lo, pb.hi, parts.stream(q), q == 0);
      }
    SC_TRY(parts.join());   // (also after an error: before anything returns)
    SC_TRY(rc_parts);
  } else {
    for (int p = 0; p < npanels; ++p) SC_TRY(run_panel(R, p, 0, batch, st, true));
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}
