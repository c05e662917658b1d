// What the files of the two-stage solver share -- twostage.hip (slab layout, driver), sy2sb.hip (stage 1), sb2st.hip
// (stage 2), bt2.hip (the Q2 back-transformation): whatever more than one of them needs; everything else is in its file.
#pragma once

#include <algorithm>
#include <vector>

#include "eigh_internal.h"
#include "twostage_policy.h"

// (internal linkage: every file gets its own copy of the constants and of the device helpers, which are always inlined)
namespace {

constexpr int kB = sc_host::kBand;  // band half-width = panel width = reflector length of stage 2
constexpr int kG = sc_host::kSweepGroup;   // sweeps per diamond
constexpr int kDiaLd = 128;       // leading dimension of a diamond (kB + kG - 1 = 127 rows used)
constexpr int kDiaSize = kDiaLd * kG;

// sizes of the fragment storage of a diamond (the slab layout needs them; their order and use: bt2.hip)
constexpr int kMiniFrags = 40;                     // fragments per mini: 20 of V^T, 20 of -(V T)
constexpr int kDiaFrags = 4 * kMiniFrags;          // 160 per diamond
constexpr int kFragDoubles = kDiaFrags * 64;       // 10240 doubles = 80 KB
static_assert(kDiaSize == sc_host::kDiaDoubles && kFragDoubles == sc_host::kDiaFragDoubles, "the slab is sized in sy2sb_plan.h");

constexpr int kLdab = sc_host::kBandRows;       // rows of the band storage: AB(i, j) = ab[(i - j) + j * kLdab]
constexpr int kQrRows = sc_host::kQrRows;       // rows of the panel one k_panel_qr workgroup owns
constexpr int kSmallSplit = sc_host::kSmallSplit;   // split-K of the V^T [X1|X2|V] product
constexpr int kIb = sc_host::kQrIb;             // inner block of the blocked panel QR (columns whose reflectors are applied to the rest at once)

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

typedef double __attribute__((address_space(1)))* gdptr;          // global memory: global_load / global_store, never flat
// a pointer every lane of the wave holds the same value of, told so to the compiler (scalar registers, and memory
// instructions of the form scalar base + 32-bit lane offset instead of a 64-bit address per access)
__device__ __forceinline__ gdptr wave_uniform(double* p) {
  const unsigned long long b = (unsigned long long)(size_t)p;
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
  return (gdptr)(size_t)(((unsigned long long)hi << 32) | (unsigned long long)lo);
}

}  // namespace

// Diamond offsets per sweep group (shared by all matrices of the batch): host copy, (ngroups + 1) ints.
inline std::vector<int> dia_offsets(int n) {
  const int nsweep = std::max(n - 2, 0);
  const int ng = (nsweep + kG - 1) / kG;
  std::vector<int> off((size_t)ng + 1, 0);
  for (int S = 0; S < ng; ++S) off[(size_t)S + 1] = off[(size_t)S] + (n - 1 - S * kG + kB - 1) / kB;
  return off;
}

// kernel-group timers of a profiled solve (the driver owns them: they are resolved when both stages have been enqueued)
struct SbTimers {
  PhaseTimer qr, symm, syr2k, bulge;
  SbTimers(sc_ctx* ctx, hipStream_t st) : qr(ctx, "panel_qr", st), symm(ctx, "symm", st), syr2k(ctx, "syr2k", st), bulge(ctx, "bulge", st) {}
  void finish() { qr.finish(); symm.finish(); syr2k.finish(); bulge.finish(); }
};

// Stage 1 on ctx->stream, the GEMM records of the solve (sc_host::stage1_records) uploaded: dense -> band (sy2sb.hip).
int sb_stage1(sc_ctx* ctx, double* d_a, long long stride_a, int n, int batch, double* d_tri_ws, const TriLayout& TL,
              double* d_sb_ws, const SbLayout& SL, const GemmDesc* d_descs, const std::vector<int>& role, bool prof,
              SbTimers& timers);
// Stage 2 on ctx->stream: band -> tridiagonal; d, e into the tri slab (sb2st.hip).
int sb_stage2(sc_ctx* ctx, double* d_a, long long stride_a, int n, int batch, double* d_tri_ws, const TriLayout& TL,
              double* d_sb_ws, const SbLayout& SL, double* d_band_copy, SbTimers& timers);
