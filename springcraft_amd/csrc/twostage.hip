// Two-stage tridiagonalisation for large matrices (replaces the one-stage panel algorithm of tridiag.hip, whose
// matrix-vector products are bound by HBM bandwidth: 4/3 n^3 bytes per matrix).
//
//   stage 1  sy2sb   dense -> band of half-width kB = 64.  Per 64-column panel: Householder QR of the block below
//                    the band (k_panel_qr, one launch per column, the panel streamed through LDS), then the
//                    two-sided update  A22 <- Q^T A22 Q = A22 - V W^T - W V^T  in which all O(n^2 b) work is f64-MFMA
//                    GEMM: X = A22 V (two triangular-operand GEMMs on the lower-stored A22), V^T [X|V] (Gram, split-K),
//                    W = [X|V] [T; -S/2] and the SYR2K  [V|W] [W|V]^T.
//   stage 2  sb2st   band -> tridiagonal by Householder bulge chasing (Lang's algorithm: sweep s annihilates column s
//                    below the first sub-diagonal and chases the bulge down the band, one reflector of length <= 64
//                    per block).  Task (s, k) only conflicts with (s+1, k-1) and later, so launch t runs every task
//                    with 2 s + k = t, one workgroup each (k_bulge_step): 2 n + n/64 launches, no spin-waits.
//   back-transformation  Z <- Q1 Q2 Z.  Q2: the reflectors of 64 consecutive sweeps at the same chase position form
//                    a "diamond" (127 x 64 parallelogram) = one compact-WY block I - V T V^T; diamonds (S, k) are
//                    applied in wavefronts 3 (Smax - S) + k = const as two grouped GEMMs per wavefront (bt2).
//                    Q1: the stage-1 reflectors through the block back-transformation of backtransform.hip.
//
// Role in the reference: part of np.linalg.eigh (LAPACK dsyevd) at nma.py:61; LAPACK itself uses the one-stage dsytrd.
//
// Files: this one holds stages 1 and 2, their driver and the slab layout; bt2.hip the Q2 back-transformation (bt2);
// twostage_internal.h what the two share; twostage_policy.h every choice between kernel forms.
#include <algorithm>
#include <vector>

#include "twostage_internal.h"

namespace {

constexpr int kLdab = 2 * kB;     // rows of the band storage: AB(i, j) = ab[(i - j) + j * kLdab]
constexpr int kQrRows = 128;      // rows of the panel one k_panel_qr workgroup owns
constexpr int kSmallSplit = 8;    // split-K of the V^T [X1|X2|V] product
constexpr int kDescKinds = 9;     // GEMM records per panel and matrix (stage 1)
#ifndef SC_QR_IB
#define SC_QR_IB 8
#endif
constexpr int kIb = SC_QR_IB;     // inner block of the blocked panel QR (columns whose reflectors are applied to the rest at once)
constexpr int kEarly = (kIb + 2) / 2;   // column loads per thread that cover a launch of an inner block (kIb + 1 columns)

typedef int v4i __attribute__((ext_vector_type(4)));   // a 16-byte record (early hand-off of the chase, the cooperative panel)

struct HH {
  double beta, tau, scale;
};

// LAPACK dlarfg scalars: x = (alpha, tail), xn2 = ||tail||^2;  H x = beta e1,  v = (1, scale * tail)
__device__ __forceinline__ HH householder(double alpha, double xn2) {
  HH h;
  // No reflection either when the column (pivot included) is below 1e-140: its squares are in the underflow range, where
  // a norm is not a norm any more (LAPACK's dlarfg rescales there) and the reflector would come out non-orthogonal.  The
  // input is scaled to [1e-100, 1e100] (matrix_scale_factor), so such a column is < 1e-40 of the matrix: the caller
  // stores zeros for its tail, a backward error far below rounding.  Seen with exactly rank-deficient input such as
  // ones(n, n), whose trailing matrices shrink by a factor eps per column.
  if (xn2 == 0.0 || alpha * alpha + xn2 < 1e-280) {
    h.beta = alpha; h.tau = 0.0; h.scale = 0.0;
    return h;
  }
  h.beta = -copysign(sqrt(alpha * alpha + xn2), alpha);
  h.tau = (h.beta - alpha) / h.beta;
  h.scale = 1.0 / (alpha - h.beta);
  return h;
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the vector-memory counter, i.e. waits for
// the acknowledgement of every global store in flight (about 2 us under load) -- wasted when no thread of the workgroup
// reads global data that another one wrote in the same kernel.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// ---- XCDs of the device, counted by a probe launch (once per context): every workgroup ORs the bit of the XCC_ID it
// runs on into a mask.  8 x CUs workgroups of one wave: the dispatcher deals consecutive workgroups round-robin over
// the XCDs, so every XCD that exists is seen.  (num_cus / 32 holds for MI350 / MI355 and their partitions only.)
__global__ void k_xcd_probe(unsigned* mask) {
  unsigned id;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
  if (threadIdx.x == 0) atomicOr(mask, 1u << (id & 15u));
}
int probe_xcd_count(sc_ctx* ctx, hipStream_t st) {
  SC_TRY(sc_reserve_dc_aux(ctx, 256));
  unsigned* d_mask = reinterpret_cast<unsigned*>(ctx->dc_aux);
  SC_HIP(ctx, hipMemsetAsync(d_mask, 0, sizeof(unsigned), st));
  const int cus = ctx->num_cus > 0 ? ctx->num_cus : 256;
  hipLaunchKernelGGL(k_xcd_probe, dim3((unsigned)(8 * cus)), dim3(64), 0, st, d_mask);
  SC_HIP(ctx, hipGetLastError());
  unsigned h_mask = 0;
  SC_HIP(ctx, hipMemcpyAsync(&h_mask, d_mask, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  SC_HIP(ctx, hipStreamSynchronize(st));
  int count = 0, top = 0;
  for (int b = 0; b < 16; ++b)
    if (h_mask >> b & 1u) { ++count; top = b + 1; }
  // the kernels bind matrix b to XCD b mod nxcd by XCC_ID value: ids must be 0 .. count - 1 (they are on every part seen)
  ctx->nxcd = (count >= 1 && count == top) ? std::min(count, 8) : 1;
  return SC_OK;
}

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
  double* P = sm;                      // [ncl][LD]   column c at P[(c - c_lo) * LD + r]
  double* wv = sm + ncl * LD;          // [kB]  w_c of the reflector being applied
  double* vv = wv + kB;                // [kQrRows]  v_r
  double* red = vv + kQrRows;          // [4][kB]
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
  double* P = sm;                      // [kB - c0][LD]: columns c0 .. kB-1, indexed relative to c0
  double* vv = sm + (kB - c0) * LD;    // [kQrRows]
  double* red = vv + kQrRows;          // [4][2][kB]
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
  double* P = sm;                      // [kB - c0][LD]: columns c0 .. kB-1, indexed relative to c0
  double* Ms = sm + (kB - c0) * LD;    // [kIb][kB]  M, later W
  double* red = Ms + kIb * kB;         // [4][kB]
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
constexpr int kWgThreads = 1024, kWgWaves = kWgThreads / 64;

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
  constexpr int kWgThreads = NT, kWgWaves = NT / 64;   // (shadow the file-level constants: NT threads per panel)
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* red = sm;                               // [2][kWgWaves][8] wave partials of the per-column sums (by column parity)
  double* piv = red + 2 * kWgWaves * 8;           // [2][8]          pivot row of the inner block
  double* tauL = piv + 16;                        // [8]
  double* Ms = tauL + 8;                          // [8][kB]         M = V^T P, then W = T^T M (column index = panel column)
  double* part = Ms + 8 * kB;                         // [kWgWaves][kB][8] wave partials of M
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
constexpr int kCoopVals = 8 * kB;                 // values of one block exchange (M and the Gram matrix)
constexpr size_t kCoopLdsBytes = sizeof(double) * ((size_t)kB * kCoopLd + kCoopRows * 8 + 8 * kB + 64 + 16 + kB + 128 + 2);
// workspace of one matrix (16-byte records): column records [2][G][16] | block partials [G][512] | block totals [512]
__host__ __device__ inline size_t coop_recs_per_matrix(int G) { return (size_t)2 * G * 16 + (size_t)G * kCoopVals + kCoopVals; }

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
  double* Pl = sm;                          // [kB][kCoopLd]  the workgroup's rows of the panel
  double* Vl = Pl + kB * kCoopLd;           // [256][8]       the inner block's reflectors by row; then partial sums
  double* Ms = Vl + kCoopRows * 8;          // [8][kB]        M, then W = T^T M
  double* red = Ms + 8 * kB;                // [2][4][8]
  double* piv = red + 64;                   // [2][8]
  double* tauA = piv + 16;                  // [kB]           tau of every column (stored at the end)
  double* tot4 = tauA + kB;                 // [2][4][16]
  int* s_dead = reinterpret_cast<int*>(tot4 + 128);
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
  double* G = sm;                 // [kB][LD]  G[i * LD + j]
  double* M1 = G + kB * LD;
  double* T = M1 + kB * LD;
  double* U = T + kB * LD;
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

// ================================================================================================================
// Band storage and stage 2
__global__ __launch_bounds__(256) void k_band_extract(const double* __restrict__ a_all, long long stride_a,
                                                      double* __restrict__ sb_all, SbLayout SL) {
  const int n = SL.n;
  const double* A = a_all + (size_t)blockIdx.y * stride_a;
  double* ab = sb_all + (size_t)blockIdx.y * SL.slab + SL.ab;
  const size_t total = (size_t)kLdab * n;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int d = (int)(idx % kLdab), jj = (int)(idx / kLdab);
    ab[idx] = (d <= kB && jj + d < n) ? A[(size_t)jj * n + jj + d] : 0.0;
  }
}

__global__ __launch_bounds__(256) void k_band_to_tri(const double* __restrict__ sb_all, SbLayout SL,
                                                     double* __restrict__ tri_all, TriLayout TL) {
  const int n = SL.n;
  const double* ab = sb_all + (size_t)blockIdx.y * SL.slab + SL.ab;
  double* tri = tri_all + (size_t)blockIdx.y * TL.slab;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    tri[TL.d + i] = ab[(size_t)i * kLdab];
    tri[TL.e + i] = i < n - 1 ? ab[(size_t)i * kLdab + 1] : 0.0;
  }
}

// After the band has been copied out: make the stage-1 reflectors a plain sub-matrix view of A for the block
// back-transformation (unit entry at row c + kB, zeros between the diagonal block and the unit entry).
__global__ __launch_bounds__(256) void k_sb_clean(double* __restrict__ a_all, long long stride_a, int n) {
  double* A = a_all + (size_t)blockIdx.y * stride_a;
  const int c = blockIdx.x;   // column
  for (int r = c + 1 + threadIdx.x; r <= std::min(c + kB, n - 1); r += 256) A[(size_t)c * n + r] = r == c + kB ? 1.0 : 0.0;
}

// Number of chase positions of sweep s: blocks of kB rows from row s+1 to n-1
using sc_host::chase_len;

// Diagnostic build (-DBULGE_STAMPS): shader cycles of wave 0 between five points of every task, summed over all tasks
// since the last read (sc_dbg_bulge_stamps, tools/bulge_stamps.py); no stamp executes in the normal build.
#ifdef BULGE_STAMPS
__device__ unsigned long long g_bulge_stamps[8];
#define BULGE_STAMP(var) unsigned long long var; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory");
#else
#define BULGE_STAMP(var)
#endif

typedef const double __attribute__((address_space(1)))* gdptr_c;
__device__ __forceinline__ double ld_l2(gdptr_c p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One task (sweep s, chase position k) of the bulge chase by one workgroup of 256 threads, blocks from and to the band
// storage: the body of k_bulge_step (one launch per wavefront of tasks) and of k_chase_finish (the take-over after a
// persistent chase that gave up).
struct BulgeTaskLds {
  double E[kB * (kB + 1)];
  double vp[kB], vn[kB], u[kB], red[4 * kB];
  double s_tau, s_beta;
};
__device__ __forceinline__ void bulge_task(double* __restrict__ sb, const SbLayout& SL, int s, int k, BulgeTaskLds& W) {
  constexpr int LD = kB + 1;
  double* const E = W.E;
  double* const D = E;   // the diagonal block is processed after E has gone back to memory: same buffer
  double* const vp = W.vp;
  double* const vn = W.vn;
  double* const u = W.u;
  double* const red = W.red;
  double& s_tau = W.s_tau;
  double& s_beta = W.s_beta;
  const int n = SL.n;
  double* ab = sb + SL.ab;
  const int S = s / kG, cc = s - S * kG;
  // diamonds of group S start at sum_{S' < S} chase_len(n, 64 S') = S K0 - S (S - 1) / 2  (K0 = chase_len(n, 0))
  const size_t dia = (size_t)S * chase_len(n, 0) - (size_t)S * (S - 1) / 2 + k;
  // diamonds are stored row-major (sweep index contiguous): element (row r, sweep c) at [c + r * kG]
  double* vd = sb + SL.vd + dia * kDiaSize + (size_t)cc * kG + cc;   // this reflector's first entry (row cc, column cc)
  const int tid = threadIdx.x;
  const int i = tid & 63, q = tid >> 6;

  const int r0 = s + 1 + k * kB;             // first row of the reflector being generated
  const int L = std::min(kB, n - r0);        // its length (>= 1)
  BULGE_STAMP(t0)

  // the diagonal block D = AB(r0 .. r0+L-1, r0 .. r0+L-1) (lower stored) is not touched before its own update:
  // fetch it right away (unconditional loads with clamped indices, masked when they go to LDS)
  // (one wave-uniform base per block + 32-bit element offsets instead of a 64-bit address per access)
  gdptr colbase = wave_uniform(ab + (size_t)r0 * kLdab);                    // AB(r0, r0)
  double d16[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int jc = std::min(q * 16 + u, L - 1);
    const int ic = std::min(std::max(i, jc), L - 1);
    d16[u] = colbase[(unsigned)((ic - jc) + jc * kLdab)];
  }

  if (k > 0) {
    gdptr ebase = wave_uniform(ab + (size_t)(r0 - kB) * kLdab);             // AB(r0 - kB, r0 - kB)
    const double* vdp = sb + SL.vd + (dia - 1) * kDiaSize + (size_t)cc * kG + cc;
    const double tau_p = sb[SL.tau2 + (dia - 1) * kG + cc];
    if (tid < kB) vp[tid] = vdp[(size_t)tid * kG];
    // E(i, j) = AB(r0 + i, c0 + j), rows i < L: thread (i, q) keeps row i, columns 16 q .. 16 q + 15 in registers for the
    // row-wise steps; only the column sums of the second reflector go through an LDS image.
    double t16[16];
    {
      const int ic = std::min(i, L - 1);
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int jj = q * 16 + u;
        t16[u] = ebase[(unsigned)((kB + ic - jj) + jj * kLdab)];
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) t16[u] = i < L ? t16[u] : 0.0;
    }
    lds_barrier();   // vp
#ifdef BULGE_STAMPS
    { BULGE_STAMP(t1) if (tid == 0) atomicAdd(&g_bulge_stamps[0], t1 - t0); }
#endif
    // u = tau_p E vp: partial sums over this wave's 16 columns, every thread adds the four partials of its own row
    {
      double a = 0.0;
#pragma unroll
      for (int u = 0; u < 16; ++u) a += t16[u] * vp[q * 16 + u];
      red[q * kB + i] = a;
    }
    lds_barrier();
    {
      const double ui = tau_p * ((red[i] + red[kB + i]) + (red[2 * kB + i] + red[3 * kB + i]));
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        t16[u] -= ui * vp[q * 16 + u];
        E[i * LD + q * 16 + u] = t16[u];
      }
    }
    // new reflector from the first column of E, which wave 0 holds in t16[0]
    if (q == 0) {
      const double x = t16[0];
      const double t2 = wave_sum((i >= 1 && i < L) ? x * x : 0.0);
      const HH h = householder(__shfl(x, 0), t2);
      vn[i] = i == 0 ? 1.0 : (i < L ? x * h.scale : 0.0);
      if (i == 0) { s_tau = h.tau; s_beta = h.beta; }
    }
    lds_barrier();
    // z_j = sum_i E[i, j] v_i  (j >= 1);  thread (j = i, rows q*16..)
    {
      double a = 0.0;
#pragma unroll
      for (int ii = q * 16; ii < q * 16 + 16; ++ii) a += E[ii * LD + i] * vn[ii];
      red[q * kB + i] = a;
    }
    lds_barrier();
    if (tid < kB) u[tid] = s_tau * ((red[tid] + red[kB + tid]) + (red[2 * kB + tid] + red[3 * kB + tid]));
    lds_barrier();
    // E <- H E (from the registers), first column = beta e1; write back.  Nobody reads the LDS image of E any more (the
    // column sums were two barriers ago), so the diagonal block may take over its buffer without another barrier.
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int jj = q * 16 + c;
      double e = t16[c] - vn[i] * u[jj];
      if (jj == 0) e = i == 0 ? s_beta : 0.0;
      if (i < L) ebase[(unsigned)((kB + i - jj) + jj * kLdab)] = e;
    }
#ifdef BULGE_STAMPS
    { BULGE_STAMP(t2) if (tid == 0) { atomicAdd(&g_bulge_stamps[1], t2 - t0); atomicAdd(&g_bulge_stamps[5], 1ull); } }
#endif
  } else {
    // sweep start: x = AB(s+1 .. s+L, s)
    if (tid < 64) {
      const double xr = ab[(size_t)(1 + std::min(tid, L - 1)) + (size_t)s * kLdab];
      const double x = tid < L ? xr : 0.0;
      const double t2 = wave_sum(tid >= 1 ? x * x : 0.0);
      const double alpha = __shfl(x, 0);
      const HH h = householder(alpha, t2);
      vn[tid] = tid == 0 ? 1.0 : x * h.scale;
      if (tid == 0) { s_tau = h.tau; s_beta = h.beta; }
      if (tid < L) ab[(size_t)(1 + tid) + (size_t)s * kLdab] = tid == 0 ? h.beta : 0.0;
    }
    lds_barrier();
  }

  // two-sided update of the diagonal block D = AB(r0 .. r0+L-1, r0 .. r0+L-1) (lower stored)
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int jj = q * 16 + u;
    if (i >= jj) {
      const double x = (i < L) ? d16[u] : 0.0;
      D[i * LD + jj] = x;
      D[jj * LD + i] = x;
    }
  }
  lds_barrier();
  BULGE_STAMP(t3)
  {
    double a = 0.0;
#pragma unroll
    for (int jj = q * 16; jj < q * 16 + 16; ++jj) a += D[i * LD + jj] * vn[jj];
    red[q * kB + i] = a;
  }
  lds_barrier();
  if (tid < 64) {
    const double p = s_tau * ((red[tid] + red[kB + tid]) + (red[2 * kB + tid] + red[3 * kB + tid]));
    const double dot = wave_sum(p * vn[tid]);
    const double alpha2 = -0.5 * s_tau * dot;
    u[tid] = p + alpha2 * vn[tid];   // w
  }
  lds_barrier();
  for (int jj = q * 16; jj < q * 16 + 16; ++jj)
    if (i >= jj && i < L)
      colbase[(unsigned)((i - jj) + jj * kLdab)] = D[i * LD + jj] - vn[i] * u[jj] - u[i] * vn[jj];

  // the reflector goes into its diamond
  if (tid < L) vd[(size_t)tid * kG] = vn[tid];
  if (tid == 0) sb[SL.tau2 + dia * kG + cc] = s_tau;
#ifdef BULGE_STAMPS
  {
    BULGE_STAMP(t4)
    if (tid == 0) {
      atomicAdd(&g_bulge_stamps[2], t3 - t0);
      atomicAdd(&g_bulge_stamps[3], t4 - t0);
      atomicAdd(&g_bulge_stamps[4], 1ull);
    }
  }
#endif
}

// Launch t of the bulge chase: workgroup x handles task (s, k) with k = (t & 1) + 2x, s = (t - k) / 2.
__global__ __launch_bounds__(256, 4) void k_bulge_step(double* __restrict__ sb_all, SbLayout SL,
                                                    int t, const int* __restrict__ done = nullptr) {
  __shared__ BulgeTaskLds W;
  const int n = SL.n;
  const int k = (t & 1) + 2 * (int)blockIdx.x;
  const int s = (t - k) / 2;
  if (s < 0 || s > n - 3 || k >= chase_len(n, s)) return;
  // resuming a persistent chase that gave up (k_bulge_chase): done[b][s] tasks of sweep s are finished already
  if (done && k < done[(size_t)blockIdx.y * n + s]) return;
  bulge_task(sb_all + (size_t)blockIdx.y * SL.slab, SL, s, k, W);
}

// Take-over after a persistent chase (k_bulge_chase / k_bulge_pair), enqueued behind every one of them so that the host
// never has to look at the chase's outcome inside a solve (round 6: the solve only enqueues).  A chase that completed
// -- always, in practice -- costs this launch a look at the control block.  Otherwise (the stop flag is up: a wait ran
// into its bound or the test hook fired; or an XCD that owns matrices received no workgroup) workgroup b finishes matrix
// b alone, task after task in the order sweep, position from the published counts -- a valid order of the chase's
// dependences whatever the state the workgroups left behind, and slow: it is the last line of defence, counted in
// stats[] (read at the next synchronising call: sc_collect_events), after which the context keeps to the per-wavefront
// launches.  stats (unsigned long long, sc_ctx::d_status): [2] chases that needed it, [3] of those: stop flag raised by a
// time-out (not by the test hook), [4] sweeps finished by the persistent kernels (all chases), [6] incomplete without a flag.
__global__ __launch_bounds__(256) void k_chase_finish(double* __restrict__ sb_all, SbLayout SL, int batch, int nxcd,
                                                      int* __restrict__ progress, const int* __restrict__ ctl,
                                                      unsigned long long* __restrict__ stats) {
  __shared__ BulgeTaskLds W;
  const int n = SL.n;
  const int b = blockIdx.x;
  long long sweeps = 0;
  for (int x = 0; x < 8; ++x) sweeps += ctl[16 + x];
  const bool complete = ctl[0] == 0 && sweeps == (long long)batch * (n - 2);
  if (b == 0 && threadIdx.x == 0) {
    atomicAdd(stats + 4, (unsigned long long)sweeps);
    if (!complete) {
      atomicAdd(stats + 2, 1ull);
      if (ctl[0] && ctl[1] == 0) atomicAdd(stats + 3, 1ull);
      if (!ctl[0]) atomicAdd(stats + 6, 1ull);
    }
  }
  if (complete) return;
  int* prog = progress + (size_t)b * n;
  double* sb = sb_all + (size_t)b * SL.slab;
  for (int s = 0; s <= n - 3; ++s) {
    const int len = chase_len(n, s);
    for (int k = prog[s]; k < len; ++k) {
      bulge_task(sb, SL, s, k, W);
      __syncthreads();   // (the task's stores are visible to this workgroup's next task: same CU, same L1 / L2 path)
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------
// Persistent form of the bulge chase: ONE launch, no launch per wavefront.  A workgroup CLAIMS the next unclaimed sweep
// of a matrix (an atomic counter per matrix) and walks it down the band, task after task; task (s, k) starts when sweep
// s - 1 has published k + 2 finished tasks (progress[b][s - 1], one counter per sweep), which is the only dependence
// the chase has.  The previous reflector of the sweep stays in LDS (no round trip through the diamond storage), a sweep
// never waits for a launch boundary, and the matrices drift apart freely, so no round of workgroups is left half empty.
//
// Forward progress by construction: sweeps are claimed in order by workgroups that are running, so the owner of sweep
// s - 1 is always running or finished when somebody waits for it -- whatever the number of resident workgroups and
// however the dispatcher spreads them over the XCDs.  (Round 2 gave workgroup r of W the sweeps r, r + W, ... statically;
// a role that was not resident orphaned its sweeps and the successor spun into its bound.)  No cooperative launch and no
// placement census is needed any more.
//
// Coherence without L2 write-backs: all workgroups of a matrix sit on ONE XCD (matrix b on XCD b mod 8; a workgroup
// reads the XCD it runs on from XCC_ID and only ever touches that XCD's matrices, their claim counters and progress
// counters), i.e. behind one L2.  A task's stores are drained (vmcnt(0)) and fenced by a workgroup barrier before thread
// 0 publishes the counter; consumers read the counter and the band through agent-scope relaxed atomic loads, which
// bypass the CU's L1 and are served by that L2 (26 us per hand-off with release / acquire at agent scope, 3 us this way:
// tools/probe_handoff.hip).  A workgroup starts on its "home" matrix (ticket mod matrices of the XCD) and moves on to
// the XCD's other matrices when that one has no unclaimed sweep left, so every matrix of an XCD is finished as long as
// ONE workgroup lands there.  Every spin is bounded as a last line of defence: a time-out raises a flag that ends all
// workgroups between tasks; the host counts it (sc_ctx_get_counter "chase_timeouts"), finishes the chase with the
// per-wavefront launches from the published counters and does not use the persistent form on that context again.
//
// ctl (ints): [0] time-out flag, [1] workgroup-local tasks after which the test hook raised it, [2..9] tickets drawn
// per XCD, [10..12] (matrix, sweep, task) of the wait that timed out, [16..23] sweeps finished per XCD (kChaseCtlInts
// ints: sc_ctx::d_chase_ctl).

// Early hand-off (round 4).  Task (s, k) reads three things from sweep s - 1: the blocks task (s - 1, k) has left --
// all its rows but the last --, and from task (s - 1, k + 1) its last row: the entry beta (what remains of the column that
// task annihilated) in the off-diagonal block and the row of the diagonal block.  The right update of the off-diagonal
// block and the new reflector only need beta, which task (s - 1, k + 1) knows as soon as it has generated ITS reflector --
// two thirds of a task before its stores have drained.  So a task publishes (beta, position) in a 16-byte record right
// there, its successor in the next sweep starts when task (s - 1, k) is complete and that record is in, loads its blocks
// and runs the first half of its work, and only then waits for (s - 1, k + 1) to be complete, fetches the last row of its
// diagonal block, and stores.  Nothing is stored before that second wait, so the order of the writes to the band is the
// one of the plain dependence.  The dependent chain of a latency-bound chase -- one task per link -- shortens by the
// loads and the first half of the arithmetic (profiles/r04_bulge_sweep.txt).
// Records: a ring of kEarlyRing per sweep, slot k mod kEarlyRing holds {beta of task k, k + 1}; written and read as ONE
// 16-byte access.  A reader that finds a later tag knows that its task (s - 1, k + 1) is long complete and takes the
// entry from the band instead.
constexpr int kEarlyRing = sc_host::kEarlyRing;
__device__ __forceinline__ void st16(void* p, v4i v) { asm volatile("global_store_dwordx4 %0, %1, off" ::"v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ void st16_sc1(void* p, v4i v) { asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory"); }
// a band entry as the chase's workgroups hand it on.  SPREAD = 0: all workgroups of a matrix sit behind ONE L2, a plain
// store (drained before the counter moves) is what the consumer's sc1 load finds there.  SPREAD = 1 (round 6: one large
// matrix chased from every XCD): a write-through store at agent scope, which a consumer on another XCD reads from memory
// with its sc1 load -- the pair MI355X_MICROARCH.md lists as valid without any fence (k_panel_coop's records use it too)
template <int SPREAD>
__device__ __forceinline__ void st_band(gdptr p, double v) {
  if (SPREAD) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}
__device__ __forceinline__ v4i ld16_l2(const void* p) {
  v4i r;
  asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(r) : "v"(p) : "memory");
  return r;
}

// Diagnostic build (-DCHASE_STAMPS): shader cycles of every wave of k_bulge_chase between ten points of a task, summed over
// all tasks of all workgroups (sc_dbg_chase_stamps, tools/chase_stamps.py): [1] wait for the predecessor sweep (poll +
// barrier), [2] loads of both blocks + first products up to the first barrier, [3] right update of E + the new reflector,
// [4] column sums + u, [5] second wait (early hand-off), [6] E stores issued + D into LDS, [7] D products, [8] w, [9] D update
// + stores issued, [10] store drain + barrier, [11] publish; [15] = waves x tasks.  Tasks at k = 0 have no E block: their
// segments [2] .. [4] are the reflector of the column alone.
#ifdef CHASE_STAMPS
__device__ unsigned long long g_chase_stamps[16];
#define CHASE_STAMP_DECL unsigned long long cs_prev = 0, cs_n = 0, cs_sum[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define CHASE_STAMP(i)                                                                 \
  {                                                                                    \
    unsigned long long t_;                                                             \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");        \
    if ((i) != 0) cs_sum[i] += t_ - cs_prev;                                           \
    cs_prev = t_;                                                                      \
  }
#define CHASE_STAMP_WRITE                                                                          \
  if ((threadIdx.x & 63) == 0) {                                                                   \
    for (int i_ = 1; i_ < 12; ++i_) atomicAdd(&g_chase_stamps[i_], cs_sum[i_]);                    \
    atomicAdd(&g_chase_stamps[15], cs_n);                                                          \
  }
#else
#define CHASE_STAMP_DECL
#define CHASE_STAMP(i)
#define CHASE_STAMP_WRITE
#endif
// SPREAD = 1 (round 6): the workgroups of ONE matrix on all XCDs -- the launch passes nxcd = 1, so every workgroup
// counts as "XCD 0" and serves every matrix; band stores and the early records are written through at agent scope
// (st_band).  For a few large matrices (config C5: one n = 24000 matrix has ~188 tasks per wavefront, three times the
// workgroups one XCD holds): until round 5 those took one launch per wavefront (48 000 launches of 8.7 us).
template <int SPREAD>
__global__ __launch_bounds__(256, 2) void k_bulge_chase(double* __restrict__ sb_all, SbLayout SL, int batch, int W, int nxcd,
                                                     int* __restrict__ progress, int* __restrict__ next_sweep,
                                                     int* __restrict__ ctl, int give_up_after, v4i* __restrict__ early) {
  constexpr int LD = kB + 1;
  __shared__ double E[kB * LD];
  double* D = E;
  __shared__ double vbuf[2][kB], u[kB], red[4 * kB];
  __shared__ double s_tau, s_beta, s_beta_in;
  __shared__ int s_go, s_claim, s_mode;

  const int n = SL.n;
  const int tid = threadIdx.x;
  const int i = tid & 63, q = tid >> 6;
  __shared__ int s_xcd, s_slot;
  if (tid == 0) {
    unsigned id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
    s_xcd = (int)(id & 7u) % nxcd;
    s_slot = atomicAdd(ctl + 2 + s_xcd, 1);
  }
  __syncthreads();
  const int xcd = s_xcd, slot = s_slot;
  const int mpx = xcd < batch ? (batch - xcd + nxcd - 1) / nxcd : 0;   // matrices of this XCD: xcd, xcd + nxcd, ...
  if (mpx == 0 || slot >= mpx * W) return;                      // no more than W workgroups per matrix
  const int K0 = chase_len(n, 0);
  int tasks_left = give_up_after;

  CHASE_STAMP_DECL
  int cur = slot % mpx, exhausted = 0;
  while (exhausted < mpx) {
    const int b = xcd + nxcd * cur;
    int* prog = progress + (size_t)b * n;
    // ---- claim the next sweep of matrix b (the counter is only ever touched from this XCD)
    if (tid == 0) s_claim = atomicAdd(next_sweep + b, 1);
    __syncthreads();
    const int s = __builtin_amdgcn_readfirstlane(s_claim);
    __syncthreads();
    if (s > n - 3) {
      ++exhausted;
      cur = cur + 1 < mpx ? cur + 1 : 0;
      continue;
    }
    exhausted = 0;
    double* sb = sb_all + (size_t)b * SL.slab;
    double* ab = sb + SL.ab;
    {
      const int len = chase_len(n, s);
      const int S = s / kG, cc = s - S * kG;
      const size_t dia0 = (size_t)S * K0 - (size_t)S * (S - 1) / 2;
      const int len_prev = s > 0 ? chase_len(n, s - 1) : 0;
      double tau_p = 0.0;
      for (int k = 0; k < len; ++k) {
        double* vp = vbuf[(k + 1) & 1];   // reflector of task k - 1 of this sweep
        double* vn = vbuf[k & 1];
        // ---- wait for sweep s - 1.  With a task (s - 1, k + 1) to wait for (early hand-off, see above): task (s - 1, k)
        // complete AND either (s - 1, k + 1) complete too (mode 2: everything is in the band) or its record in (mode 1:
        // beta from the record, the last row of the diagonal block after the second wait).  Else (mode 0): all of sweep
        // s - 1 that touches these rows is complete.
        const bool early_task = early != nullptr && s > 0 && k + 1 < len_prev;
        CHASE_STAMP(0)
        if (tid == 0) {
          // (the stop flag and the predecessor's progress are requested TOGETHER: one L2 round trip, ~0.7 us, per task on
          // the sweep-to-sweep critical path instead of two; while waiting, the flag is looked at every 16th poll only)
          const int need = s > 0 ? min(k + (early_task ? 1 : 2), len_prev) : 0;
          const int stop0 = __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          int have = s > 0 ? __hip_atomic_load(prog + s - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
          int go = stop0 ? 0 : 1;
          int mode = 0;
          double beta_in = 0.0;
          const v4i* rec = early_task ? early + ((size_t)b * n + s - 1) * kEarlyRing + ((k + 1) & (kEarlyRing - 1)) : nullptr;
          long spins = 0;
          while (go) {
            if (have >= need) {
              if (!early_task) break;
              if (have >= k + 2) { mode = 2; break; }
              const v4i r = ld16_l2(rec);
              if (r.z == k + 2) {
                mode = 1;
                beta_in = __longlong_as_double((long long)(((unsigned long long)(unsigned)r.y << 32) | (unsigned)r.x));
                break;
              }
            }
            // (2^21 polls of ~1 us: seconds, orders of magnitude above any wait for a running workgroup)
            ++spins;
            if (spins > (1L << 21) ||
                ((spins & 15) == 0 && __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
              if (!__hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                ctl[10] = b; ctl[11] = s; ctl[12] = k;
              }
              __hip_atomic_store(ctl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              go = 0;
              break;
            }
            __builtin_amdgcn_s_sleep(1);
            have = __hip_atomic_load(prog + s - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          s_go = go;
          s_mode = mode;
          s_beta_in = beta_in;
        }
        __syncthreads();
        if (!s_go) return;
        CHASE_STAMP(1)
        const int mode = s_mode;   // 1: the last row of both blocks is not in the band yet
        // second wait of a task that started on the record (mode 1): task (s - 1, k + 1) complete, then the last row of
        // the diagonal block.  Nothing of this task has been stored before.
#define CHASE_SECOND_WAIT()                                                                                       \
        if (mode == 1) {                                                                                          \
          if (tid == 0) {                                                                                         \
            int go = 1;                                                                                           \
            long spins = 0;                                                                                       \
            while (__hip_atomic_load(prog + s - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < k + 2) {         \
              ++spins;                                                                                            \
              if (spins > (1L << 21) ||                                                                           \
                  ((spins & 15) == 0 && __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {    \
                if (!__hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {                        \
                  ctl[10] = b; ctl[11] = s; ctl[12] = k;                                                          \
                }                                                                                                 \
                __hip_atomic_store(ctl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                           \
                go = 0;                                                                                           \
                break;                                                                                            \
              }                                                                                                   \
              __builtin_amdgcn_s_sleep(1);                                                                        \
            }                                                                                                     \
            s_go = go;                                                                                            \
          }                                                                                                       \
          __syncthreads();                                                                                        \
          if (!s_go) return;                                                                                      \
        }

        const int r0 = s + 1 + k * kB;
        const int L = min(kB, n - r0);
        const size_t dia = dia0 + k;
        double* vd = sb + SL.vd + dia * kDiaSize + (size_t)cc * kG + cc;
        // (one wave-uniform base per block + 32-bit element offsets: a 64-bit pointer per access costs the kernel a
        // workgroup per CU in registers)
        gdptr colbase_k = wave_uniform(ab + (size_t)r0 * kLdab);                 // AB(r0, r0)
        double d16[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) {
          const int jc = min(q * 16 + c, L - 1);
          const int ic = min(max(i, jc), L - 1);
          d16[c] = ld_l2(colbase_k + (unsigned)((ic - jc) + jc * kLdab));
        }
        if (k > 0) {
          gdptr ebase_k = wave_uniform(ab + (size_t)(r0 - kB) * kLdab);          // AB(r0 - kB, r0 - kB)
          double t16[16];
          {
            const int ic = min(i, L - 1);
#pragma unroll
            for (int c = 0; c < 16; ++c) {
              const int jj = q * 16 + c;
              t16[c] = ld_l2(ebase_k + (unsigned)((kB + ic - jj) + jj * kLdab));
            }
#pragma unroll
            for (int c = 0; c < 16; ++c) t16[c] = i < L ? t16[c] : 0.0;
            if (mode == 1 && i == kB - 1) {   // the last row: zeros and the predecessor's beta (the band still holds the old entry)
              const double bin = s_beta_in;
#pragma unroll
              for (int c = 0; c < 16; ++c) t16[c] = q * 16 + c == kB - 1 ? bin : 0.0;
            }
          }
          {
            double a = 0.0;
#pragma unroll
            for (int c = 0; c < 16; ++c) a += t16[c] * vp[q * 16 + c];
            red[q * kB + i] = a;
          }
          lds_barrier();
          CHASE_STAMP(2)
          {
            const double ui = tau_p * ((red[i] + red[kB + i]) + (red[2 * kB + i] + red[3 * kB + i]));
#pragma unroll
            for (int c = 0; c < 16; ++c) {
              t16[c] -= ui * vp[q * 16 + c];
              E[i * LD + q * 16 + c] = t16[c];
            }
          }
          if (q == 0) {
            const double x = t16[0];
            const double t2 = wave_sum((i >= 1 && i < L) ? x * x : 0.0);
            const HH h = householder(__shfl(x, 0), t2);
            vn[i] = i == 0 ? 1.0 : (i < L ? x * h.scale : 0.0);
            if (i == 0) {
              s_tau = h.tau; s_beta = h.beta;
              if (early) {   // the record of this task: all its successor in sweep s + 1 needs to start on
                const unsigned long long bb = (unsigned long long)__double_as_longlong(h.beta);
                if (SPREAD) st16_sc1(early + ((size_t)b * n + s) * kEarlyRing + (k & (kEarlyRing - 1)), v4i{(int)(unsigned)bb, (int)(unsigned)(bb >> 32), k + 1, 0});
                else st16(early + ((size_t)b * n + s) * kEarlyRing + (k & (kEarlyRing - 1)), v4i{(int)(unsigned)bb, (int)(unsigned)(bb >> 32), k + 1, 0});
              }
            }
          }
          lds_barrier();
          CHASE_STAMP(3)
          {
            double a = 0.0;
#pragma unroll
            for (int ii = q * 16; ii < q * 16 + 16; ++ii) a += E[ii * LD + i] * vn[ii];
            red[q * kB + i] = a;
          }
          lds_barrier();
          if (tid < kB) u[tid] = s_tau * ((red[tid] + red[kB + tid]) + (red[2 * kB + tid] + red[3 * kB + tid]));
          lds_barrier();
          CHASE_STAMP(4)
          CHASE_SECOND_WAIT()
          CHASE_STAMP(5)
#pragma unroll
          for (int c = 0; c < 16; ++c) {
            const int jj = q * 16 + c;
            double e = t16[c] - vn[i] * u[jj];
            if (jj == 0) e = i == 0 ? s_beta : 0.0;
            if (i < L) st_band<SPREAD>(ebase_k + (unsigned)((kB + i - jj) + jj * kLdab), e);
          }
        } else {
          gdptr col_s = wave_uniform(ab + (size_t)s * kLdab);
          if (tid < 64) {
            const double xr = ld_l2(col_s + (unsigned)(1 + min(tid, L - 1)));
            double x = tid < L ? xr : 0.0;
            if (mode == 1 && tid == kB - 1) x = s_beta_in;   // (its last entry is task (s - 1, 1)'s beta)
            const double t2 = wave_sum(tid >= 1 ? x * x : 0.0);
            const HH h = householder(__shfl(x, 0), t2);
            vn[tid] = tid == 0 ? 1.0 : x * h.scale;
            if (tid == 0) { s_tau = h.tau; s_beta = h.beta; }
          }
          lds_barrier();
          CHASE_STAMP(4)
          CHASE_SECOND_WAIT()
          CHASE_STAMP(5)
          if (tid < L) st_band<SPREAD>(col_s + (unsigned)(1 + tid), tid == 0 ? s_beta : 0.0);
        }
#undef CHASE_SECOND_WAIT
        // ---- diagonal block (after the second wait its last row is in the band)
        if (mode == 1 && i == kB - 1) {
#pragma unroll
          for (int c = 0; c < 16; ++c) {
            const int jc = q * 16 + c;
            d16[c] = ld_l2(colbase_k + (unsigned)((kB - 1 - jc) + jc * kLdab));
          }
        }
#pragma unroll
        for (int c = 0; c < 16; ++c) {
          const int jj = q * 16 + c;
          if (i >= jj) {
            const double x = (i < L) ? d16[c] : 0.0;
            D[i * LD + jj] = x;
            D[jj * LD + i] = x;
          }
        }
        lds_barrier();
        CHASE_STAMP(6)
        {
          double a = 0.0;
#pragma unroll
          for (int jj = q * 16; jj < q * 16 + 16; ++jj) a += D[i * LD + jj] * vn[jj];
          red[q * kB + i] = a;
        }
        lds_barrier();
        CHASE_STAMP(7)
        const double tau_now = s_tau;
        if (tid < 64) {
          const double pp = tau_now * ((red[tid] + red[kB + tid]) + (red[2 * kB + tid] + red[3 * kB + tid]));
          const double dot = wave_sum(pp * vn[tid]);
          u[tid] = pp - 0.5 * tau_now * dot * vn[tid];
        }
        lds_barrier();
        CHASE_STAMP(8)
        for (int jj = q * 16; jj < q * 16 + 16; ++jj)
          if (i >= jj && i < L)
            st_band<SPREAD>(colbase_k + (unsigned)((i - jj) + jj * kLdab), D[i * LD + jj] - vn[i] * u[jj] - u[i] * vn[jj]);
        if (tid < L) vd[(size_t)tid * kG] = vn[tid];
        if (tid == 0) sb[SL.tau2 + dia * kG + cc] = tau_now;
        tau_p = tau_now;
        // ---- publish: this task's stores are in the L2 before the counter moves
        CHASE_STAMP(9)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        CHASE_STAMP(10)
        if (tid == 0) {
          __hip_atomic_store(prog + s, k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (k + 1 == len) atomicAdd(ctl + 16 + xcd, 1);
          // test hook (sc_dbg_set_chase): raise the time-out flag after that many tasks of this workgroup
          if (give_up_after > 0 && --tasks_left == 0) {
            ctl[1] = give_up_after;
            __hip_atomic_store(ctl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
        CHASE_STAMP(11)
#ifdef CHASE_STAMPS
        ++cs_n;
#endif
      }
    }
  }
  CHASE_STAMP_WRITE
}

// ----------------------------------------------------------------------------------------------------------------
// Pair form of the persistent chase (round 4): ONE workgroup walks TWO consecutive sweeps down the band.
//
// Why: every byte a task stores leaves the XCD's L2 (the L2 writes through), so the chase moves 96 KB of HBM traffic
// per task whatever the cache does -- 1.75 TB per 64 x n = 6000 step, the floor of both older forms -- and every
// hand-off between sweeps goes through memory.  Sweep s + 1 touches, two tasks later, the very blocks sweep s has just
// left (shifted by one row and one column).  Here team A (threads 0..255) runs the tasks of sweep sA = 2 p and leaves
// its blocks in LDS; team B (threads 256..511) runs sweep sB = sA + 1 two positions behind and takes its blocks from
// there: per PAIR of tasks one block set is read from memory (A) and one is written (B) -- half the traffic -- and the
// A -> B hand-off costs a workgroup barrier instead of store drain + publish + poll + L2 loads.
//
// LDS: a ring of three position slots (E 64 x 65 + D packed lower, 49 920 B each): at step m, A works on position m
// (slot m % 3), B on position m - 2, position m - 1 waits.  B's block at position k is A's block shifted by (1, 1):
//   E'(i, j) = E_k(i + 1, j + 1),  E'(i, 63) = D_k(i + 1, 0),  E'(63, 63) = E_{k+1}(0, 0),  E'(63, j < 63) = 0
//   D'(i, j) = D_k(i + 1, j + 1),  D'(63, j) = E_{k+1}(0, j + 1),  D'(63, 63) = D_{k+1}(0, 0)
// so every element A leaves behind is consumed by exactly one task of B -- except the entries A has just annihilated
// (E_k(1.., 0)), which no block of sweep sB covers, and the corner D_0(0, 0) of A's first block, which has no task of B
// above it: A stores those to the band itself.  tools/models/bulge_pair_model.py is the NumPy model of this data flow
// (tests/test_bulge_pair_model.py runs it on the CPU).  The column sums a task needs (z = E^T v and the strictly-lower
// half of p = D v) read an LDS image of the block: for A that is its slot, for B the slot it has just emptied.
//
// Both teams keep ONE barrier schedule -- eight workgroup barriers per step, [0] .. [7] -- and differ in where blocks come
// from (A: memory through the L2, B: LDS) and go to (A: LDS, B: memory).  A step is either the common one (both teams on
// full 64-row blocks, neither at a sweep start: pair_step_full<TEAM>, one instruction stream per team without masks,
// clamps or case distinctions) or the general one (pair_step_general: every case, out of line so that its registers are
// not charged to the common step).  B's store drain and its publish sit behind the NEXT step's barrier [1], where team
// A waits for its E loads anyway; A's D loads are issued behind that barrier and land during steps (2)-(4).
//
// Dependences across workgroups are those of k_bulge_chase: pairs are CLAIMED in order (so the owner of sweep sA - 1 is
// running or done), A's task k starts when progress[sA - 1] >= k + 2, B publishes progress[sB] after its stores have
// drained; all workgroups of a matrix sit on one XCD.  When a wait runs into its bound or the stop flag is up, the
// workgroup writes its live slots back to the band and publishes both sweeps' counts, so the per-wavefront launches can
// finish the chase from the counters exactly as after k_bulge_chase.
constexpr int kSlotE = kB * (kB + 1);          // E block, row stride 65 (conflict-free column access)
// D block, lower triangle packed by rows: (i, j) at i (i + 1) / 2 + j (2080 doubles).  The region is a little larger
// (2176 doubles: sized in round 6 for a form of the kernel that has been removed; kept, so that the
// LDS layout and the launch stay what they were).
constexpr int kSlotD = 17 * 128;
constexpr int kSlot = kSlotE + kSlotD;
constexpr int kTeamLds = 2 * kB + kB + 4 * kB + 8;   // vbuf[2][64], u[64], red[256], tau, beta (+ pad)
constexpr size_t kPairLdsBytes = sizeof(double) * (3 * kSlot + 2 * kTeamLds);

// Diagnostic build (-DPAIR_STAMPS): shader cycles of thread 0 between the barriers of every step, summed over all steps
// of all workgroups since the last read (sc_dbg_pair_stamps, tools/pair_stamps.py); nothing of it in the normal build.
// (round 6: the sums are kept in LDS -- one writer per entry: thread 0 [0..15], thread 256 [16..31]; [32..47] are
// unused -- and added to the global table when the thread leaves the kernel: a global atomic per stamp
// more than doubled the stage's time)
#ifdef PAIR_STAMPS
__device__ unsigned long long g_pair_stamps[48];
__shared__ unsigned long long s_pair_stamps[48];
#define PAIR_STAMP(var) unsigned long long var; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory");
#define PAIR_ACC(slot, a, b) if (tid == 0) s_pair_stamps[slot] += (b) - (a);
#define PAIR_ACC_B(slot, a, b) if (tid == 256) s_pair_stamps[16 + (slot)] += (b) - (a);
#define PAIR_FLUSH(first)                                                                         \
  for (int i_ = 0; i_ < 16; ++i_)                                                                 \
    if (s_pair_stamps[(first) + i_]) atomicAdd(&g_pair_stamps[(first) + i_], s_pair_stamps[(first) + i_]);
#else
#define PAIR_STAMP(var)
#define PAIR_ACC(slot, a, b)
#define PAIR_ACC_B(slot, a, b)
#define PAIR_FLUSH(first)
#endif

// The common step of k_bulge_pair: both teams at work on full 64-row blocks, neither at a sweep start.  Same barriers
// and the same arithmetic as the general form inside the kernel, without its masks, clamps and case distinctions -- the
// step is bound by instruction issue, not by flops -- and one instruction stream per team: A (TEAM 0) loads its blocks
// from the band and leaves them in its LDS slot, B (TEAM 1) takes the shifted blocks from the slots and stores to the band.
typedef double __attribute__((address_space(3)))* ldptr;   // LDS: ds_read / ds_write, never flat
struct PairStepArgs {
  double* ab;        // band of this matrix
  double* vd;        // its diamonds
  double* tau2;
  ldptr slots;       // LDS: ring of three position slots
  ldptr vbuf, u, red, sc;   // LDS: this team's vectors
  int* prog;
  int s, k;          // this team's sweep and position
  size_t dia;
  int cc;
  int tid;
};

template <int TEAM>
__device__ __forceinline__ void pair_step_full(const PairStepArgs& P, double& tau_p, int& pend_k) {
  const int tid = P.tid, tt = tid & 255, i = tid & 63;
  const int q = (tid >> 6) & 3;
  const int k = P.k, s = P.s;
  const int r0 = s + 1 + k * kB;
  ldptr vp = P.vbuf + ((k + 1) & 1) * kB;
  ldptr vn = P.vbuf + (k & 1) * kB;
  ldptr Eimg = P.slots + (k % 3) * kSlot;   // A: its slot; B: the slot it consumes, then its scratch image
  ldptr Dimg = Eimg + kSlotE;
  ldptr red = P.red;
  ldptr u = P.u;
  gdptr colbase_k = wave_uniform(P.ab + (size_t)r0 * kLdab);
  gdptr ebase_k = wave_uniform(P.ab + (size_t)(r0 - kB) * kLdab);
  const unsigned o_e = (unsigned)(kB + i + q * 16 * (kLdab - 1));   // E(i, 16 q + c) at ebase[o_e + c (kLdab - 1)]
  const unsigned o_d = (unsigned)(i + q * 16 * (kLdab - 1));        // D(i, 16 q + c) at colbase[o_d + c (kLdab - 1)]
  double d16[16], t16[16], vr[16];
  PAIR_STAMP(f0)
  if (TEAM == 0) {
#pragma unroll
    for (int c = 0; c < 16; ++c) t16[c] = ld_l2(ebase_k + (o_e + (unsigned)(c * (kLdab - 1))));
  } else {
    const ldptr En = P.slots + ((k + 1) % 3) * kSlot;
    const int i1 = min(i + 1, kB - 1);
    const ldptr rowD = i < kB - 1 ? Dimg + i1 * (i1 + 1) / 2 : En;
    const ldptr rowE = Eimg + i1 * (kB + 1) + 1;
#pragma unroll
    for (int c = 0; c < 16; ++c) d16[c] = rowD[q * 16 + c + 1];
#pragma unroll
    for (int c = 0; c < 16; ++c) t16[c] = i < kB - 1 ? rowE[q * 16 + c] : 0.0;
    if (q == 3) {
      const double dcol = Dimg[i1 * (i1 + 1) / 2];
      t16[15] = i < kB - 1 ? dcol : En[0];
      if (i == kB - 1) d16[15] = En[kSlotE];
    }
    PAIR_STAMP(g1)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the previous step's stores are in the L2
    PAIR_STAMP(g2)
    PAIR_ACC_B(10, f0, g1) PAIR_ACC_B(11, g1, g2)
  }
#pragma unroll
  for (int c = 0; c < 16; ++c) vr[c] = vp[q * 16 + c];
  PAIR_STAMP(fa)
  lds_barrier();                                                                  // [1]
  PAIR_STAMP(f1)
  PAIR_ACC(12, f0, fa)
  if (TEAM == 1) {
    if (tt == 0 && pend_k >= 0) __hip_atomic_store(P.prog + s, pend_k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    pend_k = k;
  } else {
    // D is not touched before step (5): its loads are issued here, behind the barrier, so that the other team does not
    // wait for their issue (under load the memory pipeline takes a block's 16 load instructions per wave slowly: issuing
    // them costs as much as waiting for the data) and land behind steps (2)-(4).  Entries above the diagonal: whatever
    // lies in front of the column, masked in step (5).
#pragma unroll
    for (int c = 0; c < 16; ++c) d16[c] = ld_l2(colbase_k + (o_d + (unsigned)(c * (kLdab - 1))));
  }
  {
    double a = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) a += t16[c] * vr[c];
    red[q * kB + i] = a;
  }
  lds_barrier();                                                                  // [2]
  {
    const double ui = tau_p * ((red[i] + red[kB + i]) + (red[2 * kB + i] + red[3 * kB + i]));
    ldptr erow = Eimg + i * (kB + 1) + q * 16;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      t16[c] -= ui * vr[c];
      erow[c] = t16[c];
    }
    if (q == 0) {
      const double x = t16[0];
      const double t2 = wave_sum(i >= 1 ? x * x : 0.0);
      const HH h = householder(__shfl(x, 0), t2);
      vn[i] = i == 0 ? 1.0 : x * h.scale;
      if (i == 0) { P.sc[0] = h.tau; P.sc[1] = h.beta; }
    }
  }
  lds_barrier();                                                                  // [3]
  PAIR_STAMP(f3)
#pragma unroll
  for (int c = 0; c < 16; ++c) vr[c] = vn[q * 16 + c];
  {
    double a = 0.0;
    const ldptr ecol = Eimg + q * 16 * (kB + 1) + i;
#pragma unroll
    for (int c = 0; c < 16; ++c) a += ecol[c * (kB + 1)] * vr[c];
    red[q * kB + i] = a;
  }
  lds_barrier();                                                                  // [4]
  if (tt < kB) u[tt] = P.sc[0] * ((red[tt] + red[kB + tt]) + (red[2 * kB + tt] + red[3 * kB + tt]));
  {
    ldptr rowp = Dimg + i * (i + 1) / 2 + q * 16;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      d16[c] = q * 16 + c <= i ? d16[c] : 0.0;
      if (q * 16 + c <= i) rowp[c] = d16[c];
    }
  }
  lds_barrier();                                                                  // [5]
  PAIR_STAMP(f5)
  {
    const double vi = vn[i];
#pragma unroll
    for (int c = 0; c < 16; ++c) t16[c] -= vi * u[q * 16 + c];
    if (q == 0) t16[0] = i == 0 ? P.sc[1] : 0.0;
    if (TEAM == 0) {
      ldptr erow = Eimg + i * (kB + 1) + q * 16;
#pragma unroll
      for (int c = 0; c < 16; ++c) erow[c] = t16[c];
      if (q == 0 && i >= 1) ebase_k[(unsigned)(kB + i)] = 0.0;   // the annihilated entries, see the kernel's header
    } else {
#pragma unroll
      for (int c = 0; c < 16; ++c) ebase_k[o_e + (unsigned)(c * (kLdab - 1))] = t16[c];
    }
    double a = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int ii = q * 16 + c;
      const double dcolv = Dimg[ii * (ii + 1) / 2 + min(i, ii)];
      a += (d16[c] + (ii > i ? dcolv : 0.0)) * vr[c];     // row half + column half share vn[16 q + c]
    }
    red[q * kB + i] = a;
  }
  lds_barrier();                                                                  // [6]
  PAIR_STAMP(f6)
  const double tau_f = P.sc[0];
  if (tt < kB) {
    const double pp = tau_f * ((red[tt] + red[kB + tt]) + (red[2 * kB + tt] + red[3 * kB + tt]));
    const double dot = wave_sum(pp * vn[tt]);
    u[tt] = pp - 0.5 * tau_f * dot * vn[tt];
  }
  lds_barrier();                                                                  // [7]
  PAIR_STAMP(f7)
  {
    const double vi = vn[i], wi = u[i];
    if (TEAM == 0) {
      ldptr rowp = Dimg + i * (i + 1) / 2 + q * 16;
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (q * 16 + c <= i) rowp[c] = d16[c] - vi * u[q * 16 + c] - wi * vr[c];
    } else {
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (q * 16 + c <= i) colbase_k[o_d + (unsigned)(c * (kLdab - 1))] = d16[c] - vi * u[q * 16 + c] - wi * vr[c];
    }
    double* vd = P.vd + P.dia * kDiaSize + (size_t)P.cc * kG + P.cc;
    if (tt < kB) vd[(size_t)tt * kG] = vn[tt];
    if (tt == 0) P.tau2[P.dia * kG + P.cc] = tau_f;
    tau_p = tau_f;
  }
#ifdef PAIR_STAMPS
  {
    PAIR_STAMP(f8)
    PAIR_ACC(1, f0, f1) PAIR_ACC(2, f1, f3) PAIR_ACC(3, f3, f5) PAIR_ACC(4, f5, f6) PAIR_ACC(5, f6, f7) PAIR_ACC(6, f7, f8)
    PAIR_ACC_B(1, f0, f1) PAIR_ACC_B(2, f1, f3) PAIR_ACC_B(3, f3, f5) PAIR_ACC_B(4, f5, f6) PAIR_ACC_B(5, f6, f7)
    PAIR_ACC_B(13, f7, f8)
  }
#endif
}

// The general step of k_bulge_pair (sweep starts, partial last blocks, steps in which only one team has a position): the
// same barriers as pair_step_full, with every mask and case distinction.  Not inlined: it runs in a few steps per pair
// only, and its registers would otherwise be charged to the common step.
struct PairGenArgs {
  double* ab;
  double* vd;
  double* tau2;
  ldptr slots;
  ldptr vbuf, u, red, sc;
  int* prog;
  int* sweeps_done;
  int n, s, k, my_len, team, to_lds;
  size_t dia0;
  int cc, tid;
};
struct PairCarry {
  double tau_p;
  int pend_k;
};

__device__ __noinline__ PairCarry pair_step_general(const PairGenArgs P, double tau_p, int pend_k) {
  double* const ab = P.ab;
  const ldptr slots = P.slots, vbuf = P.vbuf, u = P.u, red = P.red, sc = P.sc;
  int* const prog = P.prog;
  const int n = P.n, s = P.s, k = P.k, my_len = P.my_len, team = P.team, cc = P.cc, tid = P.tid;
  const bool to_lds = P.to_lds != 0;
  const size_t dia0 = P.dia0;
  const int tt = tid & 255, i = tid & 63, q = (tid >> 6) & 3;
  const bool active = k >= 0 && k < my_len;
  const bool first = k == 0;
  const bool eph = active && !first;            // this team has an off-diagonal block in this step
  const int kk = active ? k : 0;
  const int r0 = s + 1 + kk * kB;
  const int L = active ? min(kB, n - r0) : 0;
  ldptr vp = vbuf + ((kk + 1) & 1) * kB;   // reflector of this sweep's previous task
  ldptr vn = vbuf + (kk & 1) * kB;
  ldptr Eimg = slots + (kk % 3) * kSlot;   // A: its slot; B: the slot it consumes, then its scratch image
  ldptr Dimg = Eimg + kSlotE;
  const size_t dia = dia0 + kk;
  gdptr colbase_k = wave_uniform(ab + (size_t)r0 * kLdab);                        // AB(r0, r0)
  gdptr ebase_k = wave_uniform(ab + (size_t)(r0 - (first ? 0 : kB)) * kLdab);    // AB(r0 - kB, r0 - kB)

  // ---- (1) the blocks into registers: thread (i, q) holds row i, columns 16 q .. 16 q + 15
  double d16[16], t16[16];
  double xcol = 0.0;   // sweep start (k == 0, first wave of the team): x = AB(s + 1 + i, s)
#pragma unroll
  for (int c = 0; c < 16; ++c) { d16[c] = 0.0; t16[c] = 0.0; }
  if (active && team == 0) {
    // (E first: it is needed at once; D is not touched before step (5), its loads land behind steps (2)-(4))
    if (!first) {
      const int ic = min(i, L - 1);
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const int jj = q * 16 + c;
        t16[c] = ld_l2(ebase_k + (unsigned)((kB + ic - jj) + jj * kLdab));
      }
    } else if (q == 0) {
      gdptr col_s = wave_uniform(ab + (size_t)s * kLdab);
      xcol = ld_l2(col_s + (unsigned)(1 + min(i, L - 1)));
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int jc = min(q * 16 + c, L - 1);
      const int ic = min(max(i, jc), L - 1);
      d16[c] = ld_l2(colbase_k + (unsigned)((ic - jc) + jc * kLdab));
    }
  } else if (active) {
    // B's block = A's, shifted by (1, 1) (see the header); row 63 comes from row 0 of A's next position.  Whatever is
    // read from a slot that does not exist (A's last position: then L <= 63) is masked out below
    const ldptr En = slots + ((kk + 1) % 3) * kSlot;
    const int i1 = min(i + 1, kB - 1);
    const ldptr rowD = i < kB - 1 ? Dimg + i1 * (i1 + 1) / 2 : En;   // D'(i, jj) = rowD[jj + 1]
    const ldptr rowE = Eimg + i1 * (kB + 1) + 1;                     // E'(i, jj) = rowE[jj]  (i, jj < 63)
#pragma unroll
    for (int c = 0; c < 16; ++c) d16[c] = rowD[q * 16 + c + 1];
    if (!first) {
#pragma unroll
      for (int c = 0; c < 16; ++c) t16[c] = i < kB - 1 ? rowE[q * 16 + c] : 0.0;
    }
    if (q == 3) {   // column 63: E'(i, 63) = D_k(i + 1, 0); corner (63, 63): D_{k+1}(0, 0) and E_{k+1}(0, 0)
      const double dcol = Dimg[i1 * (i1 + 1) / 2];
      if (!first) t16[15] = i < kB - 1 ? dcol : En[0];
      if (i == kB - 1) d16[15] = En[kSlotE];
    }
    if (first && q == 0) xcol = i < kB - 1 ? Dimg[i1 * (i1 + 1) / 2] : En[0];
  }
#pragma unroll
  for (int c = 0; c < 16; ++c) t16[c] = i < L ? t16[c] : 0.0;
  xcol = i < L ? xcol : 0.0;
  // B (and a lone A): the stores of the previous step are in the L2 -- a wait that overlaps A's for its loads
  // (A's own few stores -- zeros, corner, reflector -- are older than its next loads, whose data it waits for: in
  // order; once A has run out of positions it drains like B)
  if (!to_lds || !active) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  lds_barrier();                                                                    // [1] B's slot reads are done
  if (tt == 0 && pend_k >= 0) {   // publish the previous step's task
    __hip_atomic_store(prog + s, pend_k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (pend_k + 1 == my_len) atomicAdd(P.sweeps_done, 1);
  }
  pend_k = -1;

  // ---- (2) u = tau_p E vp: partial sums over this wave's 16 columns
  if (eph) {
    double a = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) a += t16[c] * vp[q * 16 + c];
    red[q * kB + i] = a;
  }
  lds_barrier();                                                                    // [2]
  // ---- (3) E <- E (I - tau_p vp vp^T) in registers + its LDS image; new reflector; image of D (packed lower)
  if (eph) {
    const double ui = tau_p * ((red[i] + red[kB + i]) + (red[2 * kB + i] + red[3 * kB + i]));
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      t16[c] -= ui * vp[q * 16 + c];
      Eimg[i * (kB + 1) + q * 16 + c] = t16[c];
    }
    if (q == 0) xcol = t16[0];
  }
  if (active && q == 0) {
    const double t2 = wave_sum((i >= 1 && i < L) ? xcol * xcol : 0.0);
    const HH h = householder(__shfl(xcol, 0), t2);
    vn[i] = i == 0 ? 1.0 : (i < L ? xcol * h.scale : 0.0);
    if (i == 0) { sc[0] = h.tau; sc[1] = h.beta; }
    if (first && i < L) {   // the annihilated column: AB(s + 1 .., s) = (beta, 0, ..)
      gdptr col_s = wave_uniform(ab + (size_t)s * kLdab);
      col_s[(unsigned)(1 + i)] = i == 0 ? h.beta : 0.0;
    }
  }
  lds_barrier();                                                                    // [3]
    // ---- (4) z_j = sum_i E[i, j] vn_i: thread (j = i, rows 16 q ..)
  if (eph) {
    double a = 0.0;
#pragma unroll
    for (int ii = q * 16; ii < q * 16 + 16; ++ii) a += Eimg[ii * (kB + 1) + i] * vn[ii];
    red[q * kB + i] = a;
  }
  lds_barrier();                                                                    // [4]
  if (eph && tt < kB) u[tt] = sc[0] * ((red[tt] + red[kB + tt]) + (red[2 * kB + tt] + red[3 * kB + tt]));
  // image of D (packed lower) for the column half of p = D vn; A's D loads have had steps (2)-(4) to land
#pragma unroll
  for (int c = 0; c < 16; ++c) d16[c] = (i < L && q * 16 + c <= i) ? d16[c] : 0.0;
  if (active) {
    ldptr rowp = Dimg + i * (i + 1) / 2 + q * 16;
#pragma unroll
    for (int c = 0; c < 16; ++c)
      if (q * 16 + c <= i) rowp[c] = d16[c];
  }
  lds_barrier();                                                                    // [5]
    // ---- (6) E <- H E, first column = beta e1: to LDS (A) or to the band (B); then p = D vn, row half from the
  // registers, strictly-lower (column) half from the packed image
  if (eph) {
    const double vi = vn[i], beta = sc[1];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int jj = q * 16 + c;
      double e = t16[c] - vi * u[jj];
      if (jj == 0) e = i == 0 ? beta : 0.0;
      if (to_lds) {
        Eimg[i * (kB + 1) + jj] = i < L ? e : 0.0;
        // the annihilated entries (first column below its first row) lie outside every block of sweep sB: B's shifted
        // blocks never write them back, so A zeroes them in the band itself
        if (jj == 0 && i >= 1 && i < L) ebase_k[(unsigned)(kB + i)] = 0.0;
      } else if (i < L) {
        ebase_k[(unsigned)((kB + i - jj) + jj * kLdab)] = e;
      }
    }
  }
  if (active) {
    double a = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) a += d16[c] * vn[q * 16 + c];          // (entries above the diagonal are zero)
#pragma unroll
    for (int ii = q * 16; ii < q * 16 + 16; ++ii) {
      const double dv = Dimg[ii * (ii + 1) / 2 + min(i, ii)];
      a += ii > i ? dv * vn[ii] : 0.0;
    }
    red[q * kB + i] = a;
  }
  lds_barrier();                                                                    // [6]
    const double tau_now = sc[0];
  if (active && tt < kB) {
    const double pp = tau_now * ((red[tt] + red[kB + tt]) + (red[2 * kB + tt] + red[3 * kB + tt]));
    const double dot = wave_sum(pp * vn[tt]);
    u[tt] = pp - 0.5 * tau_now * dot * vn[tt];
  }
  lds_barrier();                                                                    // [7]
    // ---- (8) D <- D - vn w^T - w vn^T: to LDS (A) or to the band (B); the reflector goes into its diamond
  if (active) {
    const double vi = vn[i], wi = u[i];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int jj = q * 16 + c;
      if (jj <= i) {
        const double val = d16[c] - vi * u[jj] - wi * vn[jj];
        if (to_lds) {
          Dimg[i * (i + 1) / 2 + jj] = i < L ? val : 0.0;
          // row 0 of a block is consumed by B's task one position up -- which does not exist for A's first block:
          // its corner AB(sA + 1, sA + 1) is final already and goes to the band here
          if (first && i == 0) colbase_k[0] = val;
        } else if (i < L) {
          colbase_k[(unsigned)((i - jj) + jj * kLdab)] = val;
        }
      }
    }
    double* vd = P.vd + dia * kDiaSize + (size_t)cc * kG + cc;
    if (tt < L) vd[(size_t)tt * kG] = vn[tt];
    if (tt == 0) P.tau2[dia * kG + cc] = tau_now;
    tau_p = tau_now;
    if (!to_lds) pend_k = k;   // published once the stores have drained: behind the next step's loads
  }
  return PairCarry{tau_p, pend_k};
}

// (the few fields of the band workspace's layout the kernel needs, instead of all of SbLayout in scalar registers)
struct PairLayout {
  int n;
  long long slab, ab, vd, tau2;
};

// whether step m of a pair is the common one (both teams on full blocks, neither at a sweep start)
__device__ __forceinline__ bool pair_common_step(bool hasB, int m, int lenA, int sA, int n) {
  return hasB && m >= 3 && m < lenA && sA + 1 + (m + 1) * kB <= n;
}

__global__ __launch_bounds__(512, 1) void k_bulge_pair(double* __restrict__ sb_all, PairLayout SL, int batch, int W, int nxcd,
                                                       int* __restrict__ progress, int* __restrict__ next_pair,
                                                       int* __restrict__ ctl, int give_up_after) {
  extern __shared__ __attribute__((aligned(16))) double pair_lds[];
  __shared__ int s_go, s_claim, s_xcd, s_slot;

  const int n = SL.n;
  const int tid = threadIdx.x;
  // (the team is uniform over a wave: told to the compiler, so that the position, the step's case and the branches on
  // them are scalar)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int team = wave >> 2;
  const int tt = tid & 255;
  double* const slots = pair_lds;
  double* const tl = pair_lds + 3 * kSlot + team * kTeamLds;
  double* const vbuf = tl;
  double* const u = tl + 2 * kB;
  double* const red = tl + 3 * kB;
  double* const sc = tl + 7 * kB;   // [0] tau, [1] beta of the reflector being generated

  if (tid == 0) {
    unsigned id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
    s_xcd = (int)(id & 7u) % nxcd;
    s_slot = atomicAdd(ctl + 2 + s_xcd, 1);
  }
#ifdef PAIR_STAMPS
  if (tid < 48) s_pair_stamps[tid] = 0;
#endif
  __syncthreads();
  const int xcd = s_xcd, slot = s_slot;
  const int mpx = xcd < batch ? (batch - xcd + nxcd - 1) / nxcd : 0;   // matrices of this XCD: xcd, xcd + nxcd, ...
  if (mpx == 0 || slot >= mpx * W) return;
  const int K0 = chase_len(n, 0);
  int steps_left = give_up_after;

  int cur = slot % mpx, exhausted = 0;
  while (exhausted < mpx) {
    const int b = xcd + nxcd * cur;
    int* prog = progress + (size_t)b * n;
    if (tid == 0) s_claim = atomicAdd(next_pair + b, 1);
    __syncthreads();
    const int sA = 2 * __builtin_amdgcn_readfirstlane(s_claim);
    __syncthreads();
    if (sA > n - 3) {
      ++exhausted;
      cur = cur + 1 < mpx ? cur + 1 : 0;
      continue;
    }
    exhausted = 0;
    double* sb = sb_all + (size_t)b * SL.slab;
    double* ab = sb + SL.ab;
    const bool hasB = sA + 1 <= n - 3;
    const int lenA = chase_len(n, sA), lenB = hasB ? chase_len(n, sA + 1) : 0;
    const int s = sA + team;                 // this team's sweep
    const int my_len = team ? lenB : lenA;
    const int S = s / kG, cc = s - S * kG;
    const size_t dia0 = (size_t)S * K0 - (size_t)S * (S - 1) / 2;
    const int len_prev = sA > 0 ? chase_len(n, sA - 1) : 0;
    const bool to_lds = team == 0 && hasB;   // A's results stay in LDS (a lone last sweep writes to memory itself)
    double tau_p = 0.0;

    const int nsteps = hasB ? lenA + 2 : lenA;
    // ---- the look at the predecessor pair (A's dependence; B's are inside the workgroup), by thread 256: the first wave of
    // team B opens a step with LDS reads only.  Followers run at the dependence's limit -- pair p + 1 starts when its
    // workgroup has finished pair p - 3, a few steps behind pair p, and both advance at the same rate -- so the look is
    // needed in 0.6 of all steps and costs 2 300 cycles of a 16 900-cycle step, all other waves waiting at [0]
    // (profiles/r06_pair_stamps.txt; requesting the values a step ahead did not pay: profiles/r06_pair_ab.txt).
    int have_c = 0;      // thread 256: last value seen of the predecessor's counter (it only grows)
    int pend_k = -1;     // task of this team whose stores are on their way: published behind the next step's loads
    for (int m = 0; m < nsteps; ++m) {
      PAIR_STAMP(ts0)
      if (tid == 256) {
        const int need = (sA > 0 && m < lenA) ? min(m + 2, len_prev) : 0;
        int go = 1;
        if (have_c < need || (m & 7) == 0) {
#ifdef PAIR_STAMPS
          s_pair_stamps[16 + 14] += 1ull;
#endif
          const int want = need;
          const int stop0 = __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          int have = sA > 0 ? __hip_atomic_load(prog + sA - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
          if (stop0) go = 0;
          long spins = 0;
          while (go && have < want) {
            // (2^21 polls of ~1 us: seconds, orders of magnitude above any wait for a running workgroup)
            ++spins;
            if (spins > (1L << 21) ||
                ((spins & 15) == 0 && __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
              if (!__hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                ctl[10] = b; ctl[11] = sA; ctl[12] = m;
              }
              __hip_atomic_store(ctl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              go = 0;
              break;
            }
            __builtin_amdgcn_s_sleep(1);
            have = __hip_atomic_load(prog + sA - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          have_c = have;
        }
        s_go = go;
      }
      PAIR_STAMP(tsp)
      lds_barrier();   // [0] (also: A's last slot writes of the previous step are ordered before B's reads below)
      if (!s_go) {
        // ---- give up between steps.  First the pending publish (its stores drained), then: A has finished positions
        // < min(m, lenA), B positions < m - 2; what A left for B (positions m - 2 and m - 1) goes back to the band, and
        // both counts are published
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tt == 0 && pend_k >= 0) __hip_atomic_store(prog + s, pend_k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (hasB) {
          for (int pos = max(m - 2, 0); pos < min(m, lenA); ++pos) {
            const double* Es = slots + (pos % 3) * kSlot;
            const double* Ds = Es + kSlotE;
            const int r0p = sA + 1 + pos * kB;
            const int Lp = min(kB, n - r0p);
            // (row 0 of the older slot has been consumed and rewritten in the band by B's task one position up)
            const int i_lo = (pos == m - 2 && pos >= 1) ? 1 : 0;
            if (pos > 0)
              for (int e = tid; e < kB * kB; e += 512) {
                const int ii = e & 63, jj = e >> 6;
                if (ii >= i_lo && ii < Lp) ab[(size_t)(r0p - kB + jj) * kLdab + (kB + ii - jj)] = Es[ii * (kB + 1) + jj];
              }
            for (int e = tid; e < kB * kB; e += 512) {
              const int ii = e & 63, jj = e >> 6;
              if (ii >= jj && ii >= i_lo && ii < Lp) ab[(size_t)(r0p + jj) * kLdab + (ii - jj)] = Ds[ii * (ii + 1) / 2 + jj];
            }
          }
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __syncthreads();
          if (tid == 0) {
            __hip_atomic_store(prog + sA, min(m, lenA), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(prog + sA + 1, min(max(m - 2, 0), lenB), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
        if (tid == 0) { PAIR_FLUSH(0) }
        if (tid == 256) { PAIR_FLUSH(16) }
        return;
      }

      PAIR_STAMP(ts1)
      const int k = team ? m - 2 : m;
      // ---- the common step: both teams at work on full 64-row blocks, neither at a sweep start (pair_step_full)
      if (pair_common_step(hasB, m, lenA, sA, n)) {
        PairStepArgs pa{ab, sb + SL.vd, sb + SL.tau2, (ldptr)slots, (ldptr)vbuf, (ldptr)u, (ldptr)red, (ldptr)sc, prog, s, k,
                        dia0 + k, cc, tid};
        if (team == 0) pair_step_full<0>(pa, tau_p, pend_k);
        else pair_step_full<1>(pa, tau_p, pend_k);
#ifdef PAIR_STAMPS
        if (tid == 0) { s_pair_stamps[9] += 1ull; s_pair_stamps[0] += ts1 - ts0; }
        if (tid == 256) { s_pair_stamps[16] += ts1 - ts0; s_pair_stamps[16 + 7] += tsp - ts0; }
#endif
      } else {
        PairGenArgs ga{ab, sb + SL.vd, sb + SL.tau2, (ldptr)slots, (ldptr)vbuf, (ldptr)u, (ldptr)red, (ldptr)sc, prog,
                       ctl + 16 + xcd, n, s, k, my_len, team, to_lds ? 1 : 0, dia0, cc, tid};
        const PairCarry pc = pair_step_general(ga, tau_p, pend_k);
        tau_p = pc.tau_p;
        pend_k = pc.pend_k;
      }
      // (no barrier here: the next step's [0] orders this step's slot writes before their readers, and nothing else of
      // the next step touches LDS before it)
#ifdef PAIR_STAMPS
      if (tid == 0) s_pair_stamps[8] += 1ull;
#endif
      if (tid == 0) {
        if (to_lds && m + 1 == lenA) atomicAdd(ctl + 16 + xcd, 1);   // (A's last task; its count is published below)
        // test hook (sc_dbg_set_chase): raise the time-out flag after that many steps of this workgroup
        if (give_up_after > 0 && --steps_left == 0) {
          ctl[1] = give_up_after;
          __hip_atomic_store(ctl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    // ---- end of the pair: the last task's stores, then its count; sweep sA lived in LDS until B had consumed it -- its
    // count only matters to a take-over and is complete now
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tt == 0 && pend_k >= 0) {
      __hip_atomic_store(prog + s, pend_k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (pend_k + 1 == my_len) atomicAdd(ctl + 16 + xcd, 1);
    }
    if (tid == 0 && hasB) __hip_atomic_store(prog + sA, lenA, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid == 0) { PAIR_FLUSH(0) }
  if (tid == 256) { PAIR_FLUSH(16) }
}

}  // namespace

// ================================================================================================================
// Layout
size_t sb_slab_doubles(int n, int batch, SbLayout* out) {
  SbLayout L{};
  L.n = n;
  long long off = 0;
  auto take = [&](long long cnt) { long long o = off; off += (cnt + 31) / 32 * 32; return o; };
  const int nchunk = (n + kQrRows - 1) / kQrRows + 1;
  L.vw = take((long long)n * 4 * kB);
  L.wv = take((long long)n * 4 * kB);
  L.xv = take((long long)n * 3 * kB);
  L.symm_split = sc_host::symm_split_for(sc_host::two_stage_env(), n, batch);
  L.xsplit = L.symm_split > 1 ? take((long long)2 * L.symm_split * n * kB) : 0;
  L.qrpart = take((long long)2 * nchunk * kB);
  L.qrpiv = take(2 * (kB + 8));
  L.qrpart8 = take((long long)nchunk * kIb * kB);
  L.small = take((long long)kSmallSplit * kB * 3 * kB);
  L.cmat = take(3 * kB * kB);
  L.small2 = take((long long)kSmallSplit * 2 * kB * kB);
  L.p2 = take(2 * kB * kB);
  L.ab = take((long long)kLdab * n);
  // diamonds
  const int nsweep = std::max(n - 2, 0);
  L.ngroups = (nsweep + kG - 1) / kG;
  long long ndia = 0;
  for (int S = 0; S < L.ngroups; ++S) {
    const int len = (n - 1 - S * kG + kB - 1) / kB;
    ndia += len;
  }
  L.ndia = ndia;
  L.vd = take(ndia * kDiaSize);
  L.frag = take(ndia * kFragDoubles);
  L.tau2 = take(ndia * kG);
  L.slab = off;
  if (out) *out = L;
  return (size_t)off;
}

int sb_desc_count(int n, int batch) {
  const int npanels = n / kB + 1;
  return npanels * kDescKinds * batch;
}

// ================================================================================================================
// Host side of stages 1 and 2.  Which kernel form a panel / a chase gets: twostage_policy.h.

// kernel-group timers of a profiled solve (the driver owns them: they are resolved when both stages have been enqueued)
struct SbTimers {
  PhaseTimer qr, symm, syr2k, bulge;
  SbTimers(sc_ctx* ctx, hipStream_t st) : qr(ctx, "panel_qr", st), symm(ctx, "symm", st), syr2k(ctx, "syr2k", st), bulge(ctx, "bulge", st) {}
  void finish() { qr.finish(); symm.finish(); syr2k.finish(); bulge.finish(); }
};

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

// One panel of the matrices [lo, hi) on `ps`: QR of the panel, X = A22 V, the small products, W, the trailing update
// its role asks for (single: SYR2K; first of a pair: the next panel's columns only; second: the joint update).
static int run_panel(const PanelRun& R, int p, int lo, int hi, hipStream_t ps, bool timed) {
  using sc_host::PanelQr;
  const sc_host::TwoStageEnv& E = sc_host::two_stage_env();
  sc_ctx* ctx = R.ctx;
  const TriLayout& TL = R.TL;
  const SbLayout& SL = R.SL;
  const int n = R.n, batch = R.batch;
  const long long stride_a = R.stride_a;
  struct StreamScope {   // launch_gemm_f64 launches on the context's stream
    sc_ctx* c; hipStream_t old;
    StreamScope(sc_ctx* c_, hipStream_t s) : c(c_), old(c_->stream) { c->stream = s; }
    ~StreamScope() { c->stream = old; }
  } scope(ctx, ps);
  const int nb = hi - lo;
  const int rl = R.role[(size_t)p];
  double* a_h = R.d_a + (size_t)lo * stride_a;
  double* tri_h = R.d_tri_ws + (size_t)lo * TL.slab;
  double* sb_h = R.d_sb_ws + (size_t)lo * SL.slab;
  const int j0 = p * kB, r0 = j0 + kB, m = n - r0;
  const int nr = std::min(kB, m - 1);
  const int nchunks = (m + kQrRows - 1) / kQrRows;
  const dim3 qgrid((unsigned)nchunks, (unsigned)nb);
  SbLayout SQ = SL;     // where the panel QR leaves V: the second panel of a pair uses the second half of [V|W..], [W|V..]
  if (rl == 2) { SQ.vw += (long long)2 * kB * n; SQ.wv += (long long)2 * kB * n; }
  if (timed) R.t.qr.start();
  const sc_host::PanelQrForm F = sc_host::panel_qr_form(E, R.coop, R.coop_recs != nullptr, m, nb, ps == R.st);
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
    case PanelQr::Wg1024: {
      const size_t lds_wg = sizeof(double) * (size_t)(2 * kWgWaves * 8 + 16 + 8 + 8 * kB + kWgWaves * kB * 8);
      const dim3 g1((unsigned)nb), b1((unsigned)kWgThreads);
      if (F.ru == 1) hipLaunchKernelGGL((k_panel_wg<1, 8>), g1, b1, lds_wg, ps, a_h, stride_a, tri_h, TL, sb_h, SQ, j0);
      else if (F.ru == 2) hipLaunchKernelGGL((k_panel_wg<2, 8>), g1, b1, lds_wg, ps, a_h, stride_a, tri_h, TL, sb_h, SQ, j0);
      else if (F.ru == 3) hipLaunchKernelGGL((k_panel_wg<3, 4>), g1, b1, lds_wg, ps, a_h, stride_a, tri_h, TL, sb_h, SQ, j0);
      else hipLaunchKernelGGL((k_panel_wg<4, 2>), g1, b1, lds_wg, ps, a_h, stride_a, tri_h, TL, sb_h, SQ, j0);
      break;
    }
    case PanelQr::Wg512: {
      constexpr int kW = 512 / 64;
      const size_t lds_wg = sizeof(double) * (size_t)(2 * kW * 8 + 16 + 8 + 8 * kB + kW * kB * 8);
      const dim3 g1((unsigned)nb), b1(512u);
      if (F.ru == 10) hipLaunchKernelGGL((k_panel_wg<10, 1, 512>), g1, b1, lds_wg, ps, a_h, stride_a, tri_h, TL, sb_h, SQ, j0);
      else hipLaunchKernelGGL((k_panel_wg<12, 1, 512>), g1, b1, lds_wg, ps, a_h, stride_a, tri_h, TL, sb_h, SQ, j0);
      break;
    }
    case PanelQr::Blocked: {
      // blocked panel: inner blocks of 8 columns, their reflectors applied to the rest of the panel at once
      const size_t lds_qr_blk = sizeof(double) * ((size_t)(kIb + 1) * (kQrRows + 1) + kB + kQrRows + 4 * kB);
      const size_t lds_blk_a = sizeof(double) * ((size_t)kB * (kQrRows + 1) + kQrRows + 8 * kB);
      const size_t lds_blk_b = sizeof(double) * ((size_t)kB * (kQrRows + 1) + kIb * kB + 4 * kB);
      hipLaunchKernelGGL(k_panel_qr, qgrid, dim3(256), lds_qr_blk, ps, a_h, stride_a, tri_h, TL, sb_h, SQ, j0, 0, nr, kIb);
      for (int c0 = 0; c0 < kB; c0 += kIb) {
        for (int j = c0 + 1; j < c0 + kIb; ++j)
          hipLaunchKernelGGL(k_panel_qr, qgrid, dim3(256), lds_qr_blk, ps, a_h, stride_a, tri_h, TL, sb_h, SQ, j0, j, nr,
                             c0 + kIb);
        // (their LDS image holds columns c0 .. kB-1 only)
        const size_t cut = sizeof(double) * (size_t)c0 * (kQrRows + 1);
        hipLaunchKernelGGL(k_pqr_blk_a, qgrid, dim3(256), lds_blk_a - cut, ps, a_h, stride_a, tri_h, TL, sb_h, SQ, j0, c0);
        if (c0 + kIb < kB)
          hipLaunchKernelGGL(k_pqr_blk_b, qgrid, dim3(256), lds_blk_b - cut, ps, a_h, stride_a, tri_h, TL, sb_h, SQ, j0, c0);
      }
      break;
    }
    case PanelQr::Unblocked: {
      const size_t lds_qr = sizeof(double) * ((size_t)kB * (kQrRows + 1) + kB + kQrRows + 4 * kB);
      for (int j = 0; j <= nr; ++j)
        hipLaunchKernelGGL(k_panel_qr, qgrid, dim3(256), lds_qr, ps, a_h, stride_a, tri_h, TL, sb_h, SQ, j0, j, nr, kB);
      break;
    }
  }
  if (timed) R.t.qr.stop();
  const GemmDesc* g = R.d_descs + (size_t)p * kDescKinds * batch;   // [kind][batch]
  if (timed) R.t.symm.start();
  // X = A22 V: one launch of k_symm3 (X into X1; X2 was zeroed for the whole solve) while the panel has enough tiles
  // for it, else X1 = L V and X2 = strict(L)^T V by two triangular-operand launches of k_gemm2
  if (R.use_symm3 && symm3_would_take(ctx, R.symm3_nb_min, m, SL.symm_split, /*aligned16=*/true) &&
      launch_symm3(ctx, g + lo, nb, m, SL.symm_split, /*aligned16=*/true, /*any_size=*/true) == SC_OK) {
    if (SL.symm_split > 1)
      hipLaunchKernelGGL(k_sum_xslices, dim3((unsigned)((m + 255) / 256), kB, (unsigned)nb), dim3(256), 0, ps, sb_h, SL, r0);
  } else {
    SC_TRY(launch_gemm_f64(ctx, g + lo, nb, m, kB, kGemmTile, SL.symm_split, false, true, kGemmAmBk));           // X1 = L V
    SC_TRY(launch_gemm_f64(ctx, g + batch + lo, nb, m, kB, kGemmTile, SL.symm_split, false, true, kGemmAkBk));   // X2 = strict(L)^T V
    if (SL.symm_split > 1)
      hipLaunchKernelGGL(k_sum_xslices, dim3((unsigned)((m + 255) / 256), 2 * kB, (unsigned)nb), dim3(256), 0, ps, sb_h, SL, r0);
  }
  if (rl == 2) {   // the trailing matrix has not seen the first panel's update yet: X1 -= [V1|W1] ([W1|V1]^T V2)
    SC_TRY(launch_gemm_f64(ctx, g + 7 * batch + lo, nb, 2 * kB, kB, kGemmTile, kSmallSplit, false, false, kGemmAkBk));
    hipLaunchKernelGGL(k_sum_p2, dim3((unsigned)(2 * kB * kB / 256), (unsigned)nb), dim3(256), 0, ps, sb_h, SL);
    SC_TRY(launch_gemm_f64(ctx, g + 8 * batch + lo, nb, m, kB, kGemmTile, 1, false, false, kGemmAmBk));
  }
  if (timed) R.t.symm.stop();
  SC_TRY(launch_gemm_f64(ctx, g + 2 * batch + lo, nb, kB, 3 * kB, kGemmTile, kSmallSplit, false, false, kGemmAkBk));
  const size_t lds_small = sizeof(double) * 4 * kB * (kB + 1);
  hipLaunchKernelGGL(k_sb_small, dim3((unsigned)nb), dim3(1024), lds_small, ps, tri_h, TL, sb_h, SL, j0);
  if (nb == batch) {
    SC_TRY(launch_gemm_f64(ctx, g + 3 * batch, 2 * batch, m, kB, kGemmTile, 1, false, false, kGemmAmBk));
  } else {
    SC_TRY(launch_gemm_f64(ctx, g + 3 * batch + lo, nb, m, kB, kGemmTile, 1, false, false, kGemmAmBk));
    SC_TRY(launch_gemm_f64(ctx, g + 4 * batch + lo, nb, m, kB, kGemmTile, 1, false, false, kGemmAmBk));
  }
  if (timed) R.t.syr2k.start();
  if (rl == 1)
    SC_TRY(launch_gemm_f64(ctx, g + 6 * batch + lo, nb, m, kB, kGemmTile, 1, false, false, kGemmAmBn));
  else
    // (records of one launch share (m, m, K); operands start at even rows of buffers with even leading dimension n)
    if (launch_gemm3_uniform(ctx, g + 5 * batch + lo, nb, m, m, rl == 2 ? 4 * kB : 2 * kB, kGemmAmBn, /*lower=*/R.use_symm3 ? 2 : 1, 1.0, 1.0,
                             /*aligned16=*/(n & 1) == 0 && (r0 & 1) == 0) != SC_OK)
      SC_TRY(launch_gemm_f64(ctx, g + 5 * batch + lo, nb, m, m, kGemmTile, 1, false, false, kGemmAmBn, /*lower_grid=*/true));
  if (timed) R.t.syr2k.stop();
  return SC_OK;
}

// Stage 1 on ctx->stream, the GEMM records of the solve uploaded: dense -> band.
static int sb_stage1(sc_ctx* ctx, double* d_a, long long stride_a, int n, int batch, double* d_tri_ws, const TriLayout& TL,
                     double* d_sb_ws, const SbLayout& SL, const GemmDesc* d_descs, const std::vector<int>& role, bool prof,
                     SbTimers& timers) {
  const sc_host::TwoStageEnv& E = sc_host::two_stage_env();
  hipStream_t st = ctx->stream;
  const int npanels = (int)role.size();

  // tau of columns without a reflector must read 0
  for (int b = 0; b < batch; ++b)
    SC_HIP(ctx, hipMemsetAsync(d_tri_ws + (size_t)b * TL.slab + TL.tau, 0, sizeof(double) * n, st));

  const int s1_parts = sc_host::stage1_parts(E, batch, prof);
  const sc_host::CoopPlan coop = sc_host::coop_plan(E, n, batch, ctx->num_cus, prof, ctx->coop_min_rows, ctx->coop_ok);
  v4i* coop_recs = nullptr;
  int* coop_ctl = nullptr;
  if (coop.ask) {
    if (ctx->coop_attr < 0)
      ctx->coop_attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_panel_coop),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCoopLdsBytes) == hipSuccess;
    if (ctx->coop_attr == 1 && coop.nb_max >= 1) {
      const size_t rec_bytes = (size_t)batch * coop_recs_per_matrix(coop.gmax) * sizeof(v4i);
      const size_t ctl_bytes = align_up((size_t)batch * 8 * sizeof(int), 256);   // one control record per matrix
      SC_TRY(sc_reserve_dc_aux(ctx, ctl_bytes + rec_bytes));
      coop_ctl = reinterpret_cast<int*>(ctx->dc_aux);
      coop_recs = reinterpret_cast<v4i*>(reinterpret_cast<char*>(ctx->dc_aux) + ctl_bytes);
      // (sequence numbers are unique within a solve only)
      SC_HIP(ctx, hipMemsetAsync(ctx->dc_aux, 0, ctl_bytes + rec_bytes, st));
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
    SC_TRY(sc_aux_stream(ctx));
    SC_TRY(sc_side_streams(ctx, s1_parts - 1));
    SC_HIP(ctx, hipEventRecord(ctx->aux_fork, st));
    for (int q = 1; q < s1_parts; ++q) SC_HIP(ctx, hipStreamWaitEvent(ctx->side_streams[q - 1], ctx->aux_fork, 0));
    int rc_parts = SC_OK;
    for (int p = 0; p < npanels && rc_parts == SC_OK; ++p)
      for (int q = 0; q < s1_parts && rc_parts == SC_OK; ++q) {
        const int lo = (int)((long long)batch * q / s1_parts), hi = (int)((long long)batch * (q + 1) / s1_parts);
        rc_parts = run_panel(R, p, lo, hi, q == 0 ? st : ctx->side_streams[q - 1], q == 0);
      }
    // (also after an error: the side streams are joined before anything returns, so that what they still have queued
    // is ordered before whatever the caller enqueues next on the main stream)
    for (int q = 1; q < s1_parts; ++q) {
      SC_HIP(ctx, hipEventRecord(ctx->side_joins[q - 1], ctx->side_streams[q - 1]));
      SC_HIP(ctx, hipStreamWaitEvent(st, ctx->side_joins[q - 1], 0));
    }
    SC_TRY(rc_parts);
  } else {
    for (int p = 0; p < npanels; ++p) SC_TRY(run_panel(R, p, 0, batch, st, true));
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

// The persistent chase of the whole batch as ONE launch (+ k_chase_finish, the take-over) in the form sc_host::chase_form_for
// chose.  Returns whether it went out; if not, the caller chases by the per-wavefront launches.
static int launch_chase(sc_ctx* ctx, sc_host::ChaseForm form, int n, int batch, double* d_sb_ws, const SbLayout& SL,
                        SbTimers& timers, bool* chased) {
  using sc_host::ChaseForm;
  hipStream_t st = ctx->stream;
  const bool pair = form == ChaseForm::Pair;
  int per_cu = 0;
  const hipError_t oe =
      pair ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_bulge_pair, 512, kPairLdsBytes)
           : (form == ChaseForm::Spread ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_bulge_chase<1>, 256, 0)
                                        : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_bulge_chase<0>, 256, 0));
  if (oe != hipSuccess) per_cu = 0;
  const sc_host::ChaseLaunch L =
      sc_host::chase_launch(sc_host::two_stage_env(), form, n, batch, ctx->nxcd, ctx->num_cus, per_cu);
  if (L.W < 1) return SC_OK;
  // progress counters (batch x n) | claim counters (batch) | early hand-off records in dc_aux; the control block is the
  // context's own (dc_aux is reused by the D&C of this solve before sc_collect_events reads the block)
  SC_TRY(sc_reserve_dc_aux(ctx, L.prog_bytes + L.next_bytes + L.early_bytes));
  int* d_prog = reinterpret_cast<int*>(ctx->dc_aux);
  int* d_next = reinterpret_cast<int*>(reinterpret_cast<char*>(ctx->dc_aux) + L.prog_bytes);
  int* d_ctl = ctx->d_chase_ctl;
  v4i* d_early = L.early_bytes ? reinterpret_cast<v4i*>(reinterpret_cast<char*>(ctx->dc_aux) + L.prog_bytes + L.next_bytes)
                               : nullptr;
  SC_HIP(ctx, hipMemsetAsync(ctx->dc_aux, 0, L.prog_bytes + L.next_bytes + L.early_bytes, st));
  SC_HIP(ctx, hipMemsetAsync(d_ctl, 0, kChaseCtlInts * sizeof(int), st));
  timers.bulge.start();
  if (pair)
    hipLaunchKernelGGL(k_bulge_pair, dim3((unsigned)L.grid), dim3(512), kPairLdsBytes, st, d_sb_ws,
                       PairLayout{SL.n, SL.slab, SL.ab, SL.vd, SL.tau2}, batch, L.W, L.nxcd, d_prog, d_next, d_ctl,
                       ctx->chase_give_up);
  else if (form == ChaseForm::Spread)
    hipLaunchKernelGGL(k_bulge_chase<1>, dim3((unsigned)L.grid), dim3(256), 0, st, d_sb_ws, SL, batch, L.W, L.nxcd, d_prog,
                       d_next, d_ctl, ctx->chase_give_up, d_early);
  else
    hipLaunchKernelGGL(k_bulge_chase<0>, dim3((unsigned)L.grid), dim3(256), 0, st, d_sb_ws, SL, batch, L.W, L.nxcd, d_prog,
                       d_next, d_ctl, ctx->chase_give_up, d_early);
  const hipError_t le = hipGetLastError();
  timers.bulge.stop();
  if (le != hipSuccess) {
    // a refused pair launch (e.g. the 157 KB of dynamic LDS on a device that does not grant them): this solve is
    // finished by the per-wavefront launches, later solves of the context leave the pair form alone
    if (pair) {
      ctx->pair_attr = 0;
      ++ctx->cnt_pair_fallbacks;
    }
    return SC_OK;
  }
  // (round 6: no look at the outcome from the host -- the take-over is a launch of its own that returns at once
  // when the chase completed, and the control block's counts reach the context's counters at the next
  // synchronising call: sc_collect_events)
  hipLaunchKernelGGL(k_chase_finish, dim3((unsigned)batch), dim3(256), 0, st, d_sb_ws, SL, batch, L.nxcd, d_prog,
                     (const int*)d_ctl, ctx->d_status);
  SC_HIP(ctx, hipGetLastError());
  ++ctx->cnt_chase_launches;
  if (pair) ++ctx->cnt_pair_launches;
  ctx->last_chase_ctl = d_ctl;
  ctx->chase_ctl_xcds = L.nxcd;
  *chased = true;
  return SC_OK;
}

// The chase as one launch per wavefront of tasks (k_bulge_step), parts of the batch on separate streams.
static int chase_stepwise(sc_ctx* ctx, int n, int batch, double* d_sb_ws, const SbLayout& SL) {
  const sc_host::TwoStageEnv& E = sc_host::two_stage_env();
  hipStream_t st = ctx->stream;
  const int t_max = 2 * (n - 3) + chase_len(n, n - 3) - 1;
  const int gx = chase_len(n, 0) / 2 + 1;
  const int nparts = sc_host::bulge_stream_parts(E, batch);
  if (nparts > 1) {
    SC_TRY(sc_aux_stream(ctx));            // (its fork event)
    SC_TRY(sc_side_streams(ctx, nparts - 1));
    SC_HIP(ctx, hipEventRecord(ctx->aux_fork, st));
    for (int p = 1; p < nparts; ++p) SC_HIP(ctx, hipStreamWaitEvent(ctx->side_streams[p - 1], ctx->aux_fork, 0));
    const int burst = sc_host::bulge_burst(E);
    for (int t0 = 0; t0 <= t_max; t0 += burst)
      for (int p = 0; p < nparts; ++p) {
        const int lo = (int)((long long)batch * p / nparts), hi = (int)((long long)batch * (p + 1) / nparts);
        for (int t = t0; t <= std::min(t_max, t0 + burst - 1); ++t)
          hipLaunchKernelGGL(k_bulge_step, dim3((unsigned)gx, (unsigned)(hi - lo)), dim3(256), 0,
                             p == 0 ? st : ctx->side_streams[p - 1], d_sb_ws + (size_t)lo * SL.slab, SL, t);
      }
    for (int p = 1; p < nparts; ++p) {
      SC_HIP(ctx, hipEventRecord(ctx->side_joins[p - 1], ctx->side_streams[p - 1]));
      SC_HIP(ctx, hipStreamWaitEvent(st, ctx->side_joins[p - 1], 0));
    }
  } else {
    for (int t = 0; t <= t_max; ++t)
      hipLaunchKernelGGL(k_bulge_step, dim3((unsigned)gx, (unsigned)batch), dim3(256), 0, st, d_sb_ws, SL, t);
  }
  return SC_OK;
}

// Stage 2 on ctx->stream: band -> tridiagonal; d, e into the tri slab.
static int sb_stage2(sc_ctx* ctx, double* d_a, long long stride_a, int n, int batch, double* d_tri_ws, const TriLayout& TL,
                     double* d_sb_ws, const SbLayout& SL, double* d_band_copy, SbTimers& timers) {
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_band_extract, dim3(256, (unsigned)batch), dim3(256), 0, st, d_a, stride_a, d_sb_ws, SL);
  if (d_band_copy)   // debugging aid: the band as stage 1 left it (first matrix)
    SC_HIP(ctx, hipMemcpyAsync(d_band_copy, d_sb_ws + SL.ab, sizeof(double) * kLdab * n, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k_sb_clean, dim3((unsigned)n, (unsigned)batch), dim3(256), 0, st, d_a, stride_a, n);
  for (int b = 0; b < batch; ++b) {
    double* sb = d_sb_ws + (size_t)b * SL.slab;
    SC_HIP(ctx, hipMemsetAsync(sb + SL.vd, 0, sizeof(double) * (size_t)SL.ndia * kDiaSize, st));
    SC_HIP(ctx, hipMemsetAsync(sb + SL.tau2, 0, sizeof(double) * (size_t)SL.ndia * kG, st));
  }
  if (n >= 3) {
    if (ctx->pair_attr < 0)   // per device, hence per context: the caller made ctx->device current
      ctx->pair_attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bulge_pair),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPairLdsBytes) == hipSuccess;
    if (ctx->nxcd <= 0) SC_TRY(probe_xcd_count(ctx, st));
    const sc_host::ChaseForm form =
        sc_host::chase_form_for(sc_host::two_stage_env(), n, batch, ctx->nxcd, ctx->num_cus, ctx->pair_attr == 1,
                                ctx->chase_mode, ctx->chase_form, ctx->chase_ok);
    bool chased = false;
    if (form != sc_host::ChaseForm::Stepwise) SC_TRY(launch_chase(ctx, form, n, batch, d_sb_ws, SL, timers, &chased));
    if (!chased) {
      ++ctx->cnt_stepwise_chases;
      timers.bulge.start();
      SC_TRY(chase_stepwise(ctx, n, batch, d_sb_ws, SL));
      timers.bulge.stop();
    }
  }
  hipLaunchKernelGGL(k_band_to_tri, dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, st, d_sb_ws, SL,
                     d_tri_ws, TL);
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

// ================================================================================================================
// Stage 1 + 2 driver.  d_a: lower triangle valid (after mirror_lower_batched).  On exit: tri slab holds d, e and the
// stage-1 tau; A holds the stage-1 reflectors (cleaned for the back-transformation); the sb slab holds the diamonds.
int sytrd_2stage_batched(sc_ctx* ctx, double* d_a, long long stride_a, int n, int batch, double* d_tri_ws,
                         const TriLayout& TL, double* d_sb_ws, const SbLayout& SL, int* d_dia_off,
                         GemmDesc* d_descs, float* ms_stage1, float* ms_stage2, double* d_band_copy) {
  hipStream_t st = ctx->stream;
  ScopedEvents<3> ev;
  const bool prof = ctx->profiling && ms_stage1 && ms_stage2;
  if (prof) {
    for (auto& e : ev) SC_HIP(ctx, hipEventCreate(&e));
    SC_HIP(ctx, hipEventRecord(ev[0], st));
  }

  // ---- descriptors of stage 1: per panel kDescKinds kinds x batch (the panels' roles: sc_host::panel_roles)
  const sc_host::TwoStageEnv& E = sc_host::two_stage_env();
  const std::vector<int> role = sc_host::panel_roles(E, n);   // 0 single, 1 first of a pair, 2 second of a pair
  const int npanels = (int)role.size();
  std::vector<GemmDesc> h((size_t)npanels * kDescKinds * batch);
  for (int p = 0; p < npanels; ++p) {
    const int j0 = p * kB, r0 = j0 + kB, m = n - r0;
    const int rl = role[(size_t)p];
    const long long vw_w = rl == 2 ? 3 * kB : kB, wv_w = rl == 2 ? 2 * kB : 0;   // columns W goes to
    for (int b = 0; b < batch; ++b) {
      double* A = d_a + (size_t)b * stride_a;
      double* sb = d_sb_ws + (size_t)b * SL.slab;
      double* a22 = A + (size_t)r0 * n + r0;
      GemmDesc* g = &h[((size_t)p * batch + b) * kDescKinds];
      // X1 = L V
      GemmDesc X1{};
      X1.a = a22; X1.sa_i = 1; X1.sa_k = n; X1.a_tri = 1;
      X1.b = sb + SL.xv + (size_t)2 * kB * n + r0; X1.sb_k = 1; X1.sb_j = n;
      X1.c = sb + SL.xv + r0; X1.ldc = n;
      X1.m = m; X1.n = kB; X1.k = m; X1.alpha = 1.0; X1.beta = 0.0;
      if (SL.symm_split > 1) {   // K slices into their own buffers, summed into X1 / X2 by k_sum_xslices
        X1.c = sb + SL.xsplit + r0;
        X1.split_stride = (long long)n * kB;
      }
      g[0] = X1;
      // X2 = strict(L)^T V
      GemmDesc X2 = X1;
      X2.sa_i = n; X2.sa_k = 1; X2.a_tri = 2;
      X2.c = sb + SL.xv + (size_t)kB * n + r0;
      if (SL.symm_split > 1) X2.c = sb + SL.xsplit + (size_t)SL.symm_split * n * kB + r0;
      g[1] = X2;
      // V^T [X1 | X2 | V], split-K slices
      GemmDesc P{};
      P.a = sb + SL.xv + (size_t)2 * kB * n + r0; P.sa_i = n; P.sa_k = 1;
      P.b = sb + SL.xv + r0; P.sb_k = 1; P.sb_j = n;
      P.c = sb + SL.small; P.ldc = kB;
      P.m = kB; P.n = 3 * kB; P.k = m; P.alpha = 1.0; P.beta = 0.0;
      P.split_stride = (long long)kB * 3 * kB;
      g[2] = P;
      // W = [X1 | X2 | V] C  -> its column block of [V|W..] and of [W|V..]
      GemmDesc W{};
      W.a = sb + SL.xv + r0; W.sa_i = 1; W.sa_k = n;
      W.b = sb + SL.cmat; W.sb_k = 1; W.sb_j = 3 * kB;
      W.c = sb + SL.vw + (size_t)vw_w * n + r0; W.ldc = n;
      W.m = m; W.n = kB; W.k = 3 * kB; W.alpha = 1.0; W.beta = 0.0;
      g[3] = W;
      // (the [W|V] panel holds -[W|V], so that every product that subtracts -- the trailing updates, the correction of X
      // in a pair -- has alpha = 1: the role-split kernel k_gemm3 keeps C itself in its accumulators and folds no sign;
      // negation is exact, the results are bit for bit those of alpha = -1 on [W|V])
      W.c = sb + SL.wv + (size_t)wv_w * n + r0;
      W.alpha = -1.0;
      g[4] = W;
      // trailing update, lower triangle: A22 -= [V|W] [W|V]^T (single panel) or the four-block form (second of a pair)
      GemmDesc R{};
      R.a = sb + SL.vw + r0; R.sa_i = 1; R.sa_k = n;
      R.b = sb + SL.wv + r0; R.sb_k = n; R.sb_j = 1;
      R.c = a22; R.ldc = n;
      R.m = m; R.n = m; R.k = rl == 2 ? 4 * kB : 2 * kB; R.alpha = 1.0; R.beta = 1.0;   // b = -[W|V]
      // (with k_symm3 in use the trailing updates also keep the first super-diagonal entry of every even row: symm3.hip)
      R.lower_only = sc_host::symm3_for(E, n) ? 2 : 1;
      g[5] = R;
      // first of a pair: only the next panel's 64 columns (and the band block above them) get this panel's update now
      GemmDesc D = R;
      D.n = kB; D.k = 2 * kB;
      g[6] = D;
      // second of a pair (rows r0 .. of the first panel's blocks): P2 = [W1|V1]^T V2, X1 -= [V1|W1] P2
      GemmDesc Q{};
      Q.a = sb + SL.wv + r0; Q.sa_i = n; Q.sa_k = 1;
      Q.b = sb + SL.xv + (size_t)2 * kB * n + r0; Q.sb_k = 1; Q.sb_j = n;
      Q.c = sb + SL.small2; Q.ldc = 2 * kB;
      Q.m = 2 * kB; Q.n = kB; Q.k = m; Q.alpha = 1.0; Q.beta = 0.0;
      Q.split_stride = (long long)2 * kB * kB;
      g[7] = Q;
      GemmDesc Cr{};
      Cr.a = sb + SL.vw + r0; Cr.sa_i = 1; Cr.sa_k = n;
      Cr.b = sb + SL.p2; Cr.sb_k = 1; Cr.sb_j = 2 * kB;
      Cr.c = sb + SL.xv + r0; Cr.ldc = n;
      Cr.m = m; Cr.n = kB; Cr.k = 2 * kB; Cr.alpha = 1.0; Cr.beta = 1.0;   // P2 comes out negated (a = -[W1|V1])
      g[8] = Cr;
    }
  }
  // regroup so that each launch's records are contiguous: [panel][kind][batch]
  std::vector<GemmDesc> hs(h.size());
  for (int p = 0; p < npanels; ++p)
    for (int b = 0; b < batch; ++b) {
      const GemmDesc* g = &h[((size_t)p * batch + b) * kDescKinds];
      GemmDesc* o = &hs[(size_t)p * kDescKinds * batch];
      for (int kd = 0; kd < kDescKinds; ++kd) o[(size_t)kd * batch + b] = g[kd];
    }
  if (!hs.empty()) SC_TRY(sc_stage_upload(ctx, d_descs, hs.data(), hs.size() * sizeof(GemmDesc)));
  const std::vector<int> doff = dia_offsets(n);
  SC_TRY(sc_stage_upload(ctx, d_dia_off, doff.data(), doff.size() * sizeof(int)));

  SbTimers timers(ctx, st);
  SC_TRY(sb_stage1(ctx, d_a, stride_a, n, batch, d_tri_ws, TL, d_sb_ws, SL, d_descs, role, prof, timers));
  if (prof) SC_HIP(ctx, hipEventRecord(ev[1], st));
  SC_TRY(sb_stage2(ctx, d_a, stride_a, n, batch, d_tri_ws, TL, d_sb_ws, SL, d_band_copy, timers));
  if (prof) {
    SC_HIP(ctx, hipEventRecord(ev[2], st));
    SC_HIP(ctx, hipEventSynchronize(ev[2]));
    SC_HIP(ctx, hipEventElapsedTime(ms_stage1, ev[0], ev[1]));
    SC_HIP(ctx, hipEventElapsedTime(ms_stage2, ev[1], ev[2]));
  }
  timers.finish();
  return SC_OK;
}

int sb_band_width() { return kB; }

// ---- diagnostic build only (-DCHASE_STAMPS): the segment sums of k_bulge_chase; reset after the read
extern "C" int sc_dbg_chase_stamps(unsigned long long* out16) {
#ifdef CHASE_STAMPS
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_chase_stamps), sizeof(unsigned long long) * 16) != hipSuccess) return 5;
  static const unsigned long long zeros[16] = {0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_chase_stamps), zeros, sizeof(zeros)) == hipSuccess ? 0 : 5;
#else
  (void)out16;
  return 1;
#endif
}

// ---- diagnostic build only: {sum t(E in LDS), sum t(E stored) [tasks with k > 0], sum t(D in LDS), sum t(end), tasks,
// tasks with k > 0}, cycles since the task's start; reset after the read
extern "C" int sc_dbg_pair_stamps(unsigned long long* out16) {
#ifdef PAIR_STAMPS
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_pair_stamps), 384) != hipSuccess) return 5;   // (48 entries)
  const unsigned long long z[48] = {0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_pair_stamps), z, 384) == hipSuccess ? 0 : 5;
#else
  (void)out16;
  return 1;
#endif
}

extern "C" int sc_dbg_bulge_stamps(unsigned long long* out6) {
#ifdef BULGE_STAMPS
  if (hipMemcpyFromSymbol(out6, HIP_SYMBOL(g_bulge_stamps), 48) != hipSuccess) return 5;
  unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_bulge_stamps), z, 64) == hipSuccess ? 0 : 5;
#else
  (void)out6;
  return 1;
#endif
}

// ---- debugging entry point (not part of the public C ABI): band after stage 1 (128 x n, AB(i,j) at [(i-j) + 128 j])
// and the tridiagonal after stage 2 of ONE host matrix (NumPy layout, lower triangle read).
extern "C" int sc_dbg_two_stage(sc_ctx* ctx, const double* a, int n, double* band_out, double* d_out, double* e_out) {
  if (!ctx || !a || n < 4 * kB) return SC_ERR_INVALID_ARG;
  SC_HIP(ctx, hipSetDevice(ctx->device));
  TriLayout TL{};
  TL.n = n; TL.nb = kB;
  TL.d = 0; TL.e = n; TL.tau = 2 * (long long)n; TL.slab = 3 * (long long)n + 64;
  SbLayout SL;
  const size_t sbd = sb_slab_doubles(n, 1, &SL);
  double *d_a = nullptr, *d_tri = nullptr, *d_sb = nullptr, *d_band = nullptr;
  int* d_off = nullptr;
  GemmDesc* d_desc = nullptr;
  SC_HIP(ctx, hipMalloc(&d_a, sizeof(double) * (size_t)n * n));
  SC_HIP(ctx, hipMalloc(&d_tri, sizeof(double) * TL.slab));
  SC_HIP(ctx, hipMalloc(&d_sb, sizeof(double) * sbd));
  SC_HIP(ctx, hipMalloc(&d_band, sizeof(double) * kLdab * n));
  SC_HIP(ctx, hipMalloc(&d_off, sizeof(int) * (n / 64 + 8)));
  SC_HIP(ctx, hipMalloc(&d_desc, sizeof(GemmDesc) * sb_desc_count(n, 1)));
  SC_HIP(ctx, hipMemcpyAsync(d_a, a, sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice, ctx->stream));
  int rc = mirror_lower_batched(ctx, d_a, (long long)n * n, n, 1);
  if (rc == SC_OK)
    rc = sytrd_2stage_batched(ctx, d_a, (long long)n * n, n, 1, d_tri, TL, d_sb, SL, d_off, d_desc, nullptr, nullptr,
                              d_band);
  if (rc == SC_OK) {
    (void)hipMemcpy(band_out, d_band, sizeof(double) * kLdab * n, hipMemcpyDeviceToHost);
    (void)hipMemcpy(d_out, d_tri + TL.d, sizeof(double) * n, hipMemcpyDeviceToHost);
    (void)hipMemcpy(e_out, d_tri + TL.e, sizeof(double) * n, hipMemcpyDeviceToHost);
  }
  (void)hipFree(d_a); (void)hipFree(d_tri); (void)hipFree(d_sb); (void)hipFree(d_band); (void)hipFree(d_off);
  (void)hipFree(d_desc);
  return rc;
}
