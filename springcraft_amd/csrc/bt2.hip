// The Q2 back-transformation of the two-stage solver (bt2): Z <- Q2 Z with the reflectors of the bulge chase, grouped
// into diamonds.  k_dia_tfactor2 (T factors and MFMA fragments), k_bt2_apply (one launch over all diamonds), k_bt2_wave
// (one launch per wavefront of diamonds), their host side and the readers of the diagnostic builds' stamps.
// Overview of the algorithm: twostage.hip; which form a solve gets: twostage_policy.h.
#include <type_traits>

#include "twostage_internal.h"

namespace {

// ================================================================================================================
// Z <- Q2 Z (k_dia_tfactor2 + k_bt2_apply; tools/models/bt2_model.py is their NumPy specification).
//
// The f64 matrix pipe issues one 16x16x4 MFMA per 64 cycles (profiles/r02_probe_clock.txt).  The columns of Z are
// independent, so ONE launch lets every workgroup take 16 NW columns through ALL diamonds in order (sweep groups last to
// first, chase positions first to last) with no synchronisation between workgroups:
//   * the 128-row window of Z lives in the accumulators as Z itself (rows x columns), split over the waves by COLUMNS:
//     a wave owns 16 columns x 128 rows = 8 accumulator tiles.  An accumulator register of this MFMA has exactly the lane
//     layout of a B operand (k = lane >> 4 <-> tile row 4 r + k, j = lane & 15), so  W = V^T Z  takes its B operands
//     straight from the window registers and  Z -= (V T) W  takes them straight from the W accumulators: no LDS
//     round trip for Z or W; going from one chase position to the next the window slides by 64 rows (64 finished rows
//     are stored, 64 new ones loaded): Z is read and written once per sweep group;
//   * a diamond (64 sweeps at one chase position) is applied as FOUR compact-WY blocks of 16 sweeps ("minis", sweep tile
//     st = 3, 2, 1, 0: Q = Q_0 Q_1 Q_2 Q_3, the last acts first).  The reflectors of a mini span rows 16 st .. 16 st + 78
//     = 5 row tiles for V^T Z and for (V T) W alike: 4 x (20 + 20) = 160 MFMAs per diamond and 16 columns, 1.25 x the
//     algorithmic flops.  (Round 2 applied all 64 sweeps as one block: 80 + 104 MFMAs = 1.44 x, because V T of a
//     64-sweep block is a trapezoid rather than a parallelogram.)
//   * the A operands (V^T and -(V T)) are the same for every wave and every column chunk: k_dia_tfactor2 writes them
//     once per diamond as ready-made MFMA fragments (512 B = one wave-wide ds_read_b64 each) in exactly the order the
//     products consume them, 160 per diamond = 80 KB;
//   * a workgroup streams the fragments into a ring of three half-diamond buffers (40 KB each) with LDS-DMA
//     (global_load_lds_dwordx4, no staging registers), two halves ahead of the MFMAs; one barrier per half.
#ifndef BT2_DBG
#define BT2_DBG 0
#endif
// Diagnostic build (-DBT2_STAMPS): per wave, the shader cycles between eight points of the diamond loop are summed and left
// in g_bt2_stamps (read with sc_dbg_bt2_stamps, tools/bt2_stamps.py); no stamp executes in the normal build.
#ifdef BT2_STAMPS
__device__ unsigned long long g_bt2_stamps[64 * 8 * 17];
#define BT2_STAMP_DECL unsigned long long st_sum[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, st_prev = 0, st_n = 0;
#define BT2_STAMP(i)                                                              \
  {                                                                               \
    __builtin_amdgcn_sched_barrier(0);                                            \
    unsigned long long t_;                                                        \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");   \
    if ((i) != 0 || st_n != 0) st_sum[i] += t_ - st_prev;                         \
    st_prev = t_;                                                                 \
    if ((i) == 15) ++st_n;                                                        \
    __builtin_amdgcn_sched_barrier(0);                                            \
  }
#define BT2_STAMP_WRITE                                                           \
  if (blockIdx.x < 64 && lane == 0) {                                             \
    for (int i = 0; i < 16; ++i) g_bt2_stamps[(blockIdx.x * 8 + (w & 7)) * 17 + i] = st_sum[i]; \
    g_bt2_stamps[(blockIdx.x * 8 + (w & 7)) * 17 + 16] = st_n;                    \
  }
#else
#define BT2_STAMP_DECL
#define BT2_STAMP(i)
#define BT2_STAMP_WRITE
#endif
// Diagnostic build (-DBT2_CLOCK): the shader clock while k_bt2_apply runs -- wave 0 of workgroup 0 reads
// s_memtime (shader cycles) and s_memrealtime (100 MHz) at its start and end (sc_dbg_bt2_clock, tools/bt2_clock.py).
#ifdef BT2_CLOCK
__device__ unsigned long long g_bt2_clk[2];
#define BT2_CLOCK_BEGIN                                                                                      \
  unsigned long long ck0_ = 0, rt0_ = 0;                                                                     \
  if (blockIdx.x == 0 && threadIdx.x < 64)                                                                   \
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(ck0_), "=s"(rt0_)::"memory");
#define BT2_CLOCK_END                                                                                        \
  if (blockIdx.x == 0 && threadIdx.x < 64) {                                                                 \
    unsigned long long ck1_, rt1_;                                                                           \
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(ck1_), "=s"(rt1_)::"memory"); \
    if (threadIdx.x == 0) { g_bt2_clk[0] = ck1_ - ck0_; g_bt2_clk[1] = rt1_ - rt0_; }                        \
  }
#else
#define BT2_CLOCK_BEGIN
#define BT2_CLOCK_END
#endif
// Diagnostic build (-DBT2_TRACE): s_memtime in front of every MFMA of ONE diamond (workgroup 0, sweep group
// ngroups / 2, fourth chase position), every wave: g_bt2_trace[wave][half][step] (sc_dbg_bt2_trace, tools/bt2_trace.py).
#ifdef BT2_TRACE
__device__ unsigned long long g_bt2_trace[8 * 2 * 81];
#define BT2_TRACE_POINT(H, f)                                                                       \
  if (trace_on) {                                                                                   \
    unsigned long long t_;                                                                          \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                      \
    if (lane == 0) g_bt2_trace[((w & 7) * 2 + (H)) * 81 + (f)] = t_;                                \
  }
#else
#define BT2_TRACE_POINT(H, f)
#endif
typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int kMini = 16;                          // sweeps per compact-WY block
constexpr int kHalfFrags = 2 * kMiniFrags;         // a half-diamond (two minis) is the unit of the LDS ring
constexpr int kHalfDoubles = kHalfFrags * 64;      // 5120 doubles = 40 KB
// Fragment index inside a diamond = issue index: minis in the order st = 3, 2, 1, 0; inside a mini first the 20 steps
// of W = V_st^T Z (j = 4 (rt - st) + r: Z tile rt register r is the B operand), then the 20 of Z -= (V_st T_st) W
// (j = 5 r + (rt - st): W register r is the B operand, the five row tiles take turns).
__host__ __device__ constexpr int mf_p1(int st, int rt, int r) { return (3 - st) * kMiniFrags + 4 * (rt - st) + r; }
__host__ __device__ constexpr int mf_p2(int st, int rt, int r) { return (3 - st) * kMiniFrags + 20 + 5 * r + (rt - st); }
static_assert(mf_p2(0, 4, 3) == kDiaFrags - 1 && mf_p1(3, 3, 0) == 0, "fragment order");
// Where lane l's value of fragment f lives inside a diamond's block: the two fragments of an even / odd pair of steps
// side by side, so that a lane fetches both with ONE 16-byte LDS read (ds_read_b128 runs at the full LDS rate, 8-byte
// reads at half of it -- and the fragment reads are most of the kernel's LDS traffic).
__host__ __device__ constexpr int frag_off(int f, int l) { return ((f >> 1) * 64 + l) * 2 + (f & 1); }

typedef const double __attribute__((address_space(1)))* zptr_c;   // global_load / global_store, never flat
typedef double __attribute__((address_space(1)))* zptr;
typedef const void __attribute__((address_space(1)))* gvoid_c;
typedef void __attribute__((address_space(3)))* lvoid;

// acc += A B over k-steps [k4_lo, k4_hi): lane (fr, fk) supplies A[i = fr][k = 4 k4 + fk] = a(fr, k) and
// B[k][j = fr] = b(k, fr); acc[r] is D[i = 4 r + fk][j = fr].
template <class FA, class FB>
__device__ __forceinline__ d4 mma_range(d4 acc, int k4_lo, int k4_hi, int fr, int fk, FA a, FB b) {
  for (int k4 = k4_lo; k4 < k4_hi; ++k4) {
    const int k = 4 * k4 + fk;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a(fr, k), b(k, fr), acc, 0, 0, 0);
  }
  return acc;
}

// Per diamond and mini: T = (diag(1 / tau) + striu(V^T V))^-1 of the mini's 16 reflectors (the dlarft recurrence is the
// back substitution for this inverse; reflectors with tau = 0 are decoupled), then the fragments of V^T and -(V T)^T.
// Gram blocks and (V T)^T on the matrix cores; (V T)^T is computed transposed because an accumulator register of the
// transposed tile IS the fragment (same lane, same order), so it is stored with one coalesced 512-byte write.
__global__ __launch_bounds__(256) void k_dia_tfactor2(double* __restrict__ sb_all, SbLayout SL, int dia0) {
  constexpr int LD = kG + 1;
  __shared__ double Vc[kG * LD];          // Vc[c * LD + i] = V[c + i, c]
  __shared__ double Us[4][kMini * 17];    // per mini: U[a * 17 + b], a <= b
  __shared__ double Ts[4][kMini * 17];    // per mini: T[a * 17 + b]
  __shared__ double tau_s[kG];
  double* sb = sb_all + (size_t)blockIdx.y * SL.slab;
  const size_t dia = (size_t)dia0 + blockIdx.x;
  const double* vd = sb + SL.vd + dia * kDiaSize;
  const double* tau = sb + SL.tau2 + dia * kG;
  double* frag = sb + SL.frag + dia * kFragDoubles;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  {
    const int c = tid & 63, q = tid >> 6;   // lanes along the sweeps (contiguous in memory)
    for (int i = q; i < kB; i += 4) Vc[c * LD + i] = vd[(size_t)(c + i) * kG + c];
    if (tid < kG) tau_s[tid] = tau[tid];
  }
  __syncthreads();
  auto V = [&](int row, int c) -> double {
    const int i = row - c;
    return (unsigned)i < (unsigned)kB ? Vc[c * LD + i] : 0.0;
  };
  // ---- U of mini st = w: strictly upper part of its Gram block (rows 16 st .. 16 st + 78), 1 / tau on the diagonal
  {
    const int st = w;
    const d4 g = mma_range(d4{0, 0, 0, 0}, 4 * st, 4 * st + 20, fr, fk,
                           [&](int i, int k) { return V(k, 16 * st + i); }, [&](int k, int j) { return V(k, 16 * st + j); });
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = 4 * r + fk, b = fr;
      const double ta = tau_s[16 * st + a], tb = tau_s[16 * st + b];
      double u = 0.0;
      if (a < b) u = (ta != 0.0 && tb != 0.0) ? g[r] : 0.0;
      else if (a == b) u = ta != 0.0 ? 1.0 / ta : 1.0;
      Us[st][a * 17 + b] = u;
    }
  }
  __syncthreads();
  // ---- lane (st, j) of the first wave solves U_st x = e_j by back substitution
  if (w == 0) {
    const int st = lane >> 4, j = lane & 15;
    const double* Ub = Us[st];
    double x[16];
#pragma unroll
    for (int i = 15; i >= 0; --i) {
      double s = i == j ? 1.0 : 0.0;
#pragma unroll
      for (int l = i + 1; l < 16; ++l) s -= Ub[i * 17 + l] * x[l];
      x[i] = i <= j ? s / Ub[i * 17 + i] : 0.0;
    }
    if (tau_s[16 * st + j] == 0.0) x[j] = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) Ts[st][i * 17 + j] = x[i];
  }
  __syncthreads();
  // ---- fragments of V^T: lane l holds V[16 rt + 4 r + (l >> 4)][16 st + (l & 15)]
  for (int idx = tid; idx < 4 * 20 * 64; idx += 256) {
    const int l = idx & 63, f = idx >> 6;
    const int st = f / 20, j = f % 20, rt = st + j / 4, r = j % 4;
    frag[frag_off(mf_p1(st, rt, r), l)] = V(16 * rt + 4 * r + (l >> 4), 16 * st + (l & 15));
  }
  // ---- fragments of -(V T): tile (st, rt) transposed,  D'[sweep i][row j] = sum_l T_st[l][i] V[16 rt + j][16 st + l]
  for (int q = w; q < 20; q += 4) {
    const int st = q / 5, rt = st + q % 5;
    const d4 d = mma_range(d4{0, 0, 0, 0}, 0, 4, fr, fk, [&](int i, int k) { return Ts[st][k * 17 + i]; },
                           [&](int k, int j) { return V(16 * rt + j, 16 * st + k); });
#pragma unroll
    for (int r = 0; r < 4; ++r) frag[frag_off(mf_p2(st, rt, r), lane)] = -d[r];
  }
}

template <int NW>
__global__ __launch_bounds__(64 * NW, 2) void k_bt2_apply(const double* __restrict__ sb_all, SbLayout SL,
                                                          const int* __restrict__ dia_off, double* __restrict__ z_all,
                                                          long long stride_z, int ncols, int batch, int xcd_map) {
  // ablation builds only (tools/ablate_bt2.sh; results are wrong by construction): 1 no fragment DMA, 2 no Z traffic,
  // 4 one MFMA in ten, 8 no workgroup barriers in the diamond loop, 16 no fragment reads from LDS, 32 finished rows not
  // stored, 64 entering rows not loaded / scattered, 128 finished rows transposed but not stored, 256 entering rows
  // loaded but not scattered
  constexpr int dbg = BT2_DBG;
  extern __shared__ __attribute__((aligned(16))) double lds[];   // ring of 3 half-diamond buffers | transposition tiles
  const int n = SL.n;
  constexpr int kCols = 16 * NW;
  int mat, chunk;
  if (xcd_map) {   // all column chunks of a matrix on one XCD: they stream the same fragments through one L2
    const int nchunk = (ncols + kCols - 1) / kCols;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    mat = xcd + 8 * (slot / nchunk);
    chunk = slot % nchunk;
    if (mat >= batch) return;
  } else {
    mat = blockIdx.y;
    chunk = blockIdx.x;
  }
  // (workgroup-uniform, and told so: the fragment addresses below are then scalar arithmetic)
  const unsigned long long sb_bits = (unsigned long long)(size_t)(sb_all + (size_t)mat * SL.slab);
  const double* sb = (const double*)(size_t)(
      ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(sb_bits >> 32)) << 32) |
      (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)sb_bits));
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int col = chunk * kCols + 16 * w + fr;          // this lane's column in the accumulator layout
  const bool col_ok = col < ncols;

  // ---- Z <-> accumulator tiles.  In the accumulator layout a lane owns (row 4 r + fk, column fr): a global access in
  // that shape is 16 columns x 32 bytes per instruction, which the memory path serves at ~3 TB/s (measured: the Z
  // traffic alone then takes longer than all MFMAs).  So global memory is touched in the row-contiguous shape - lane l
  // moves 16 bytes: rows 2 (l & 7), + 1 of column (l >> 3) [and of column (l >> 3) + 8 in a second instruction], i.e.
  // 8 full 128-byte column segments per instruction - and each 16 x 16 tile is transposed through a wave-private LDS
  // tile [column][18] on its way to / from the accumulator layout (LDS executes a wave's accesses in order: no waits).
  constexpr int kStg = 16 * 18;
  double* stg = lds + 3 * kHalfDoubles + w * kStg;
  const int gc = lane >> 3, gr = (lane & 7) * 2;
  const int col_a = chunk * kCols + 16 * w + gc, col_b = col_a + 8;
  double* z_mat = z_all + (size_t)mat * stride_z;
  // addresses = one wave-uniform base (scalar registers; the row of an access is added there) + a 32-bit element
  // offset per lane: no 64-bit vector arithmetic per access
  const int base_col = std::max(0, std::min(chunk * kCols + 16 * w, ncols - 16));
  const gdptr zw = wave_uniform(z_mat + (size_t)base_col * n);
  // (BYTE offsets: a 32-bit offset the compiler has to scale by 8 may exceed 32 bits for all it knows, and it falls back
  // to 64-bit vector adds)
  typedef char __attribute__((address_space(1)))* gbptr;
  // the base of row `row` as an opaque scalar value (otherwise the compiler re-associates base + row + lane offset into
  // a hoisted 64-bit per-lane pointer + row, one 64-bit vector add per access again)
  // (and the lane offset re-materialised in the block of the access: hoisted out of the loop it arrives there as a 64-bit
  // value the instruction selector cannot see the zero extension of, and the scalar-base form is not chosen)
  auto lane_off = [&](unsigned e) -> unsigned {
    asm volatile("" : "+v"(e));
    return e;
  };
  auto row_base = [&](int row) -> gbptr {
    unsigned long long b = (unsigned long long)(size_t)(zw + row);
    asm volatile("" : "+s"(b));
    return (gbptr)(size_t)b;
  };
  const unsigned ea = 8u * (unsigned)(((col_a < ncols ? col_a : ncols - 1) - base_col) * n + gr);
  const unsigned eb = 8u * (unsigned)(((col_b < ncols ? col_b : ncols - 1) - base_col) * n + gr);
  typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));
  typedef const d2u __attribute__((address_space(1)))* z2ptr_c;
  typedef d2u __attribute__((address_space(1)))* z2ptr;
  struct Raw { d2u a, b; };   // one tile as it comes from / goes to memory
  // raw load, branch-free and without a use of the values (they are consumed much later; a select or a branch here makes
  // hipcc wait for every load on the spot).  A tile that sticks out of the matrix is loaded from rows n - 16 .. n - 1
  // instead and shifted back when it is scattered.
  auto load_raw = [&](Raw& t, int row0) {
    const int rs = row0 < n - 16 ? row0 : n - 16;
    const gbptr zr = row_base(rs);
    t.a = *(z2ptr_c)(zr + lane_off(ea));
    t.b = *(z2ptr_c)(zr + lane_off(eb));
  };
  // raw tile -> accumulator layout, rows beyond the matrix and columns beyond ncols masked to zero
  auto scatter_tile = [&](d4& t, const Raw& raw, int row0) {
    *(d2u*)(stg + gc * 18 + gr) = raw.a;
    *(d2u*)(stg + (gc + 8) * 18 + gr) = raw.b;
    asm volatile("" ::: "memory");   // compiler ordering only: the tile is read back through another type
    const int shift = row0 < n - 16 ? 0 : row0 - (n - 16);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 4 * r + fk + shift;
      // (a select, not a multiplication by a 0 / 1 mask: f64 VALU work queues behind the MFMAs in flight)
      const double x = stg[fr * 18 + (i < 16 ? i : 15)];
      t[r] = (col_ok && row0 + 4 * r + fk < n) ? x : 0.0;
    }
    asm volatile("" ::: "memory");
  };
  // accumulator layout -> memory in two stages, so that the LDS round trip can sit in the shadow of MFMAs:
  // stage 1 (tile_to_rows): through the staging tile into two row-contiguous register pairs; stage 2 (store_rows).
  auto tile_to_rows = [&](const d4& t, Raw& out) {
#pragma unroll
    for (int r = 0; r < 4; ++r) stg[fr * 18 + 4 * r + fk] = t[r];
    asm volatile("" ::: "memory");
    out.a = *(const d2u*)(stg + gc * 18 + gr);
    out.b = *(const d2u*)(stg + (gc + 8) * 18 + gr);
    asm volatile("" ::: "memory");
  };
  auto store_rows = [&](const Raw& v, int row0) {
    const gbptr zr = row_base(row0);
    if (row0 + 16 <= n) {
      if (col_a < ncols) *(z2ptr)(zr + lane_off(ea)) = v.a;
      if (col_b < ncols) *(z2ptr)(zr + lane_off(eb)) = v.b;
    } else {
      if (col_a < ncols) {
        if (row0 + gr < n) *(gdptr)(zr + ea) = v.a[0];
        if (row0 + gr + 1 < n) *(gdptr)(zr + ea + 8) = v.a[1];
      }
      if (col_b < ncols) {
        if (row0 + gr < n) *(gdptr)(zr + eb) = v.b[0];
        if (row0 + gr + 1 < n) *(gdptr)(zr + eb + 8) = v.b[1];
      }
    }
  };
  auto store_tile = [&](const d4& t, int row0) {
    Raw v;
    tile_to_rows(t, v);
    store_rows(v, row0);
  };
  // the same in pieces of a few instructions (one piece per MFMA in the diamond loop): one column half per piece, the
  // tile that sticks out of the matrix handled by lane predicates instead of a second code path
  // (all 16 NW columns of the workgroup inside the matrix: with the tile inside too, the store needs no lane predicate
  // -- one scalar branch per piece instead of a dozen exec-mask branches)
  const bool full_cols = chunk * kCols + kCols <= ncols;
  auto store_half = [&](unsigned ec, bool col_in, const d2u& v, int row0) {
    const gbptr zr = row_base(row0);
    if (full_cols && row0 + 16 <= n) {
      *(z2ptr)(zr + lane_off(ec)) = v;
    } else if (col_in) {
      if (row0 + gr + 1 < n) *(z2ptr)(zr + lane_off(ec)) = v;
      else if (row0 + gr < n) *(gdptr)(zr + lane_off(ec)) = v[0];
    }
  };
  auto store_rows_a = [&](const Raw& v, int row0) { store_half(ea, col_a < ncols, v.a, row0); };
  auto store_rows_b = [&](const Raw& v, int row0) { store_half(eb, col_b < ncols, v.b, row0); };
  // scatter_tile in two pieces: raw tile -> transposition tile -> four values per lane (scatter_in); masks and the move
  // into the accumulator layout a few MFMAs later, when the LDS reads have come back (scatter_out)
  // (round 5: a tile inside the matrix, all columns of the workgroup inside too, takes ONE scalar branch and no vector
  // compare / select / index arithmetic at all -- every VALU instruction between two MFMAs costs matrix-pipe time: eight
  // v_xor per 32 MFMAs cost k_gemm3's K loop 6 %)
  auto scatter_in = [&](const Raw& raw, double (&tmp)[4], int row0) {
    *(d2u*)(stg + gc * 18 + gr) = raw.a;
    *(d2u*)(stg + (gc + 8) * 18 + gr) = raw.b;
    asm volatile("" ::: "memory");
    if (row0 < n - 16) {
#pragma unroll
      for (int r = 0; r < 4; ++r) tmp[r] = stg[fr * 18 + 4 * r + fk];
    } else {
      const int shift = row0 - (n - 16);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * r + fk + shift;
        tmp[r] = stg[fr * 18 + (i < 16 ? i : 15)];
      }
    }
    asm volatile("" ::: "memory");
  };
  auto scatter_out = [&](d4& t, const double (&tmp)[4], int row0) {
    double x[4];
    if (full_cols && row0 + 16 <= n) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        x[r] = tmp[r];
        asm volatile("" : "+v"(x[r]));
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        x[r] = (col_ok && row0 + 4 * r + fk < n) ? tmp[r] : 0.0;
        // (pinned here: the values are only used by the next diamond, and the compiler would otherwise sink the selects
        // to the end of this one, where nothing overlaps them)
        asm volatile("" : "+v"(x[r]));
      }
    }
    t = d4{x[0], x[1], x[2], x[3]};
  };
  // LDS-DMA: instruction q moves bytes [1024 q, 1024 q + 1024) of a half-diamond; wave w issues q = kDmaPer w + j.
  // Issued from inline asm: hipcc then keeps no scoreboard entry for them (with the builtin it guards later LDS reads
  // and register reuse with vmcnt(0), i.e. waits for the DMA it has just issued); their completion is counted by hand:
  // every wait for them below is an explicit vmcnt.
  // M0 (the LDS destination base) is written ONCE per five instructions: a write to M0 waits until the LDS-DMA
  // instructions in flight have landed (measured: with M0 saved / set / restored around every instruction the five
  // issued one memory latency apart, ~2600 cycles per half in which the wave issued nothing else).  The instruction's
  // immediate offset moves both the global and the LDS address, so five consecutive kilobytes share one M0 and one
  // scalar base, both pointing at the middle one.  Nothing else in this kernel uses M0 (saved / restored around the
  // whole loop).
  const unsigned lds_base = (unsigned)(size_t)(lvoid)lds;
  constexpr int kDmaInstr = kHalfDoubles * 8 / 1024;          // 40 per half
  constexpr int kDmaPer = kDmaInstr / NW;                     // per wave: 5 (8 waves) or 10 (4 waves)
  static_assert(kDmaPer * NW == kDmaInstr && kDmaPer % 5 == 0, "DMA instructions are shared in fives");
  const int wu = __builtin_amdgcn_readfirstlane(w);
  const unsigned voff = (unsigned)lane * 16u;
  // 8 waves = two per SIMD: waves 4 .. 7 run one half-diamond behind waves 0 .. 3 (see the diamond loop)
#ifndef BT2_LAGSEL
#define BT2_LAGSEL 0   // experiments: 1 = odd waves trail instead of waves 4 .. 7, 2 = nobody trails
#endif
#ifndef BT2_BURST
#define BT2_BURST 0    // experiment: 1 = the heavy pieces of a first half in one burst in front of its first MFMA
#endif
#define PF(x) (BT2_BURST ? 0 : (x))
#ifndef BT2_DMA_H0
#define BT2_DMA_H0 1   // experiment: 0 = every wave issues its share of the DMA in both halves
#endif
  constexpr bool kPhased = NW == 8 && BT2_LAGSEL != 2;
  const int lag = (kPhased && (BT2_LAGSEL == 1 ? (wu & 1) != 0 : wu >= 4)) ? 1 : 0;
  // DMA instructions a wave issues in a first / second half: with the phase offset exactly one wave group is in a first
  // half during any time slot, and it issues ALL 40 (the first half is the piece-heavy one anyway; the partner's second
  // half stays as bare as possible)
  constexpr bool kDmaAllH0 = kPhased && BT2_LAGSEL == 0 && BT2_DMA_H0;
  constexpr int kDmaH0 = kDmaAllH0 ? 2 * kDmaPer : kDmaPer, kDmaH1 = kDmaAllH0 ? 0 : kDmaPer;
  const int dma_w = kDmaAllH0 ? (wu & 3) : wu;
  constexpr int kFin0 = kDmaH0 == 5 ? 10 : 16;
  // M0 and the scalar base for instructions 5 g .. 5 g + 4 of this wave, half at `src`, ring slot `slot`
  auto dma_begin = [&](const double* src, int slot, int g, int widx, int per) -> unsigned long long {
    const int qc = widx * per + 5 * g + 2;
    const unsigned long long ga = (unsigned long long)(size_t)src + (unsigned long long)qc * 1024ull;
    // (the builtin returns int: widen through unsigned, or a low half with bit 31 set would smear into the high half)
    const unsigned ga_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)ga);
    const unsigned ga_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(ga >> 32));
    const unsigned lq = __builtin_amdgcn_readfirstlane(lds_base + (unsigned)(slot * kHalfDoubles) * 8u + (unsigned)qc * 1024u);
    // (s_nop 4: the scalar base below comes out of v_readfirstlane, and an SGPR written by a VALU instruction needs five
    // wait states before a global_* instruction reads it as its base -- hipcc pads nothing around an asm statement;
    // found in round 5 on k_gemm3, where a base reloaded from a spill lane right in front of the DMA read as zero)
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 4" : : "s"(lq) : "memory");
    return ((unsigned long long)ga_hi << 32) | (unsigned long long)ga_lo;
  };
  auto dma_go = [&](unsigned long long sbase, int i) {   // i = 0 .. 4 (a constant after unrolling)
    switch (i) {
      case 0: asm volatile("global_load_lds_dwordx4 %0, %1 offset:-2048" : : "v"(voff), "s"(sbase) : "memory"); break;
      case 1: asm volatile("global_load_lds_dwordx4 %0, %1 offset:-1024" : : "v"(voff), "s"(sbase) : "memory"); break;
      case 2: asm volatile("global_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(sbase) : "memory"); break;
      case 3: asm volatile("global_load_lds_dwordx4 %0, %1 offset:1024" : : "v"(voff), "s"(sbase) : "memory"); break;
      default: asm volatile("global_load_lds_dwordx4 %0, %1 offset:2048" : : "v"(voff), "s"(sbase) : "memory"); break;
    }
  };
  auto dma_half = [&](const double* src, int slot) {     // all of this wave's instructions at once (group prologue)
    unsigned long long sbase = 0;
#pragma unroll
    for (int j = 0; j < kDmaPer; ++j) {
      if (j % 5 == 0) sbase = dma_begin(src, slot, j / 5, wu, kDmaPer);
      dma_go(sbase, j % 5);
    }
  };
  auto wait_vm0 = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
  auto barrier = [&]() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  // Window registers: three arrays of four tiles (64 rows each).  The window of diamond k is arrays ph | ph + 1 (mod 3),
  // ph = k mod 3; the third array first holds the 64 rows finished at the last slide (stored behind the MFMAs of this
  // diamond's first half) and is then refilled with the 64 rows that enter the window at the next slide (scattered in
  // behind the MFMAs of the second half): sliding is a renaming, no register moves and nothing left outside the shadow
  // of the MFMA runs.  The diamond body is instantiated once per phase so that every tile index is a constant.
  d4 zz[12];
  int fin_row = 0;
  bool have_fin = false;

  BT2_STAMP_DECL
  BT2_CLOCK_BEGIN
  int S_cur = 0;   // (read by the -DBT2_TRACE build only)
  (void)S_cur;
  auto diamond = [&](auto PH, const double* fgrp, int k, int nh, bool more, int& slot, int win) {
    constexpr int ph = decltype(PH)::value;
#ifdef BT2_TRACE
    const bool trace_on = blockIdx.x == 0 && S_cur == SL.ngroups / 2 && k == 3;
#endif
#define ZT(rt) zz[4 * ((ph + (rt) / 4) % 3) + (rt) % 4]
    Raw zn[2], fin_rows;
#pragma unroll
    for (int H = 0; H < 2; ++H) {
      const int q = 2 * k + H;                               // half index inside the group
      typedef double d2l __attribute__((ext_vector_type(2)));
      const d2l* ldsP = (const d2l*)(lds + slot * kHalfDoubles) + lane;   // pair p of this half: ldsP[64 p]
      // the half fetched during this time slot is the one the leading wave group runs NEXT (slot index = q + lag):
      // ring position (q + lag + 1) mod 3, the one the trailing group left at the last barrier
      int slot_pre = slot + 1 + lag;
      slot_pre = slot_pre >= 3 ? slot_pre - 3 : slot_pre;
      // (past the end of the group the last half is fetched again, into a slot nobody reads: no branch in the loop)
      const double* src_pre = fgrp + (size_t)(q + lag + 1 < nh ? q + lag + 1 : nh - 1) * kHalfDoubles;
      BT2_STAMP(7 * H)
      if (!(dbg & 8)) barrier();   // half q complete in LDS (every wave waited for its own part); half q - 1 finished
      BT2_STAMP(7 * H + 1)
      // ---- 80 MFMAs: minis st = 3 - 2 H and 2 - 2 H, everything else in their shadow: the DMA of half q + 2; in the
      // first half the store of the rows finished at the last slide (through the transposition tile, then to memory);
      // the loads of the 64 rows that enter the window at the slide and their way through the transposition tile into
      // the spare array (issued and consumed in EVERY iteration - after the last diamond of a group they are not needed,
      // the clamped addresses are still valid: hipcc's wait-count bookkeeping is not path sensitive, and loads that
      // are only issued / consumed under `more` stay "maybe pending" around the loop, which costs a vmcnt(0) wherever
      // their registers are reused).
      // One MFMA at a time: what else the half has to do is cut into pieces of a few instructions each, and at most one
      // piece sits in front of every MFMA, so that it issues while the previous MFMA occupies the matrix pipe (64
      // cycles).  (Measured with the in-kernel stamps: with the same work bunched between groups of 4 or 8 MFMAs a wave
      // spends as long issuing its ~600 other instructions per half as the pipe needs for its 80 MFMAs, and the second
      // wave of the SIMD cannot fill the holes because it runs the same pattern.)
      d4 wa = d4{0, 0, 0, 0};
#ifndef BT2_KAHEAD
#define BT2_KAHEAD 8
#endif
      constexpr int kAhead = BT2_KAHEAD;                      // fragments in flight between LDS and the MFMA that uses them
      double fq[kAhead];
      double sc[4];                                           // a new tile between the transposition tile and its select
      unsigned long long dma_base = 0;                        // scalar base of the DMA instructions being issued
#pragma unroll
      for (int j = 0; j < kAhead / 2; ++j) {
        const d2l t = ldsP[j * 64];
        fq[2 * j] = t[0];
        fq[2 * j + 1] = t[1];
      }
#pragma unroll
      for (int f = 0; f < ((dbg & 4) ? 8 : kHalfFrags); ++f) {
        // ---- this step's piece
        // Two waves share a SIMD (w and w + 4) and the trailing one runs one half behind (lag): the pieces are placed
        // so that the partner of a wave in a piece-heavy stretch is in a stretch of (nearly) bare MFMAs and can keep
        // the matrix pipe fed -- the heavy pieces (DMA issue, the stores of the finished rows) sit in the first 40
        // steps of the FIRST half, which run beside the partner's second half, whose first 40 steps carry three light
        // pieces; the second 40 steps of both halves carry a few light ones each.
        if (H == 0) {
#if BT2_BURST
          if (f == 0 && !(dbg & 1)) {
#pragma unroll
            for (int j = 0; j < kDmaH0; ++j) {
              if (j % 5 == 0) dma_base = dma_begin(src_pre, slot_pre, j / 5, dma_w, kDmaH0);
              dma_go(dma_base, j % 5);
            }
          }
#else
          if (f < kDmaH0 && !(dbg & 1)) {
            if (f % 5 == 0) dma_base = dma_begin(src_pre, slot_pre, f / 5, dma_w, kDmaH0);
            dma_go(dma_base, f % 5);
          }
#endif
        } else {
          if (f >= 46 && f < 46 + kDmaH1 && !(dbg & 1)) {
            if ((f - 46) % 5 == 0) dma_base = dma_begin(src_pre, slot_pre, (f - 46) / 5, dma_w, kDmaH1);
            dma_go(dma_base, (f - 46) % 5);
          }
        }
        if (!(dbg & 2)) {
          if (H == 0) {
            // rows entering at the slide, tiles 0 and 1: requested right after the half's DMA instructions (the compiler
            // does not see those: its vmcnt for the first use of a row then covers them, being older, and nothing younger)
            if (f == PF(kDmaH0 + 1) && !(dbg & 64)) load_raw(zn[0], win + 128);
            if (f == PF(kDmaH0 + 3) && !(dbg & 64)) load_raw(zn[1], win + 128 + 16);
            // rows finished at the last slide: tile i through the transposition tile at step 10 + 8 i (8 waves; 14 + 8 i
            // with the 10 DMA steps of the 4-wave variant), column halves a / b stored 4 and 6 steps later
            if (have_fin && !(dbg & 32)) {
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                if (f == PF(kFin0 + 8 * i)) tile_to_rows(ZT(8 + i), fin_rows);
                if (dbg & 128) {   // (ablation: the transposition without the stores)
                  if (f == PF(kFin0 + 4 + 8 * i)) asm volatile("" : : "v"(fin_rows.a), "v"(fin_rows.b));
                } else {
                  if (f == PF(kFin0 + 4 + 8 * i)) store_rows_a(fin_rows, fin_row + 16 * i);
                  if (f == PF(kFin0 + 6 + 8 * i)) store_rows_b(fin_rows, fin_row + 16 * i);
                }
              }
            }
            // tiles 0, 1 of the new rows into the spare array (free since step kFin0 + 24), then the requests for
            // tiles 2, 3 into the same two raw registers: the youngest four loads of the half, the only ones its closing
            // vmcnt(4) leaves in flight
            if (f == 52 && (dbg & 256)) asm volatile("" : : "v"(zn[0].a), "v"(zn[0].b));
            if (f == 52 && !(dbg & 64) && !(dbg & 256)) scatter_in(zn[0], sc, win + 128);
            if (f == 58 && !(dbg & 64) && !(dbg & 256)) scatter_out(ZT(8), sc, win + 128);
            if (f == 60 && (dbg & 256)) asm volatile("" : : "v"(zn[1].a), "v"(zn[1].b));
            if (f == 60 && !(dbg & 64) && !(dbg & 256)) scatter_in(zn[1], sc, win + 128 + 16);
            if (f == 66 && !(dbg & 64) && !(dbg & 256)) scatter_out(ZT(9), sc, win + 128 + 16);
            if (f == 68 && !(dbg & 64)) load_raw(zn[0], win + 128 + 32);
            if (f == 70 && !(dbg & 64)) load_raw(zn[1], win + 128 + 48);
          } else {
            // tiles 2, 3 (requested ~40 steps ago) before this half's DMA instructions are issued: the compiler's
            // vmcnt(0) for them must not cover the DMA
            if (f == 28 && (dbg & 256)) asm volatile("" : : "v"(zn[0].a), "v"(zn[0].b));
            if (f == 28 && !(dbg & 64) && !(dbg & 256)) scatter_in(zn[0], sc, win + 128 + 32);
            if (f == 34 && !(dbg & 64) && !(dbg & 256)) scatter_out(ZT(10), sc, win + 128 + 32);
            if (f == 36 && (dbg & 256)) asm volatile("" : : "v"(zn[1].a), "v"(zn[1].b));
            if (f == 36 && !(dbg & 64) && !(dbg & 256)) scatter_in(zn[1], sc, win + 128 + 48);
            if (f == 42 && !(dbg & 64) && !(dbg & 256)) scatter_out(ZT(11), sc, win + 128 + 48);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
#ifdef BT2_STAMPS
#ifdef BT2_STAMPS_FINE   // the first half's four inner stamps after steps 2, 5, 8, 11 (or 13, 16, 19, 22 with =2) instead
        if (H == 0 && f >= 3 + 11 * (BT2_STAMPS_FINE - 1) && f <= 12 + 11 * (BT2_STAMPS_FINE - 1) &&
            (f - 11 * (BT2_STAMPS_FINE - 1)) % 3 == 0) BT2_STAMP(1 + (f - 11 * (BT2_STAMPS_FINE - 1)) / 3)
        if (H == 1 && (f == 16 || f == 32 || f == 48 || f == 64)) BT2_STAMP(7 * H + 1 + f / 16)
#else
        if (f == 16 || f == 32 || f == 48 || f == 64) BT2_STAMP(7 * H + 1 + f / 16)
#endif
#endif
        BT2_TRACE_POINT(H, f)
        // ---- the MFMA
        {
          const int st = 3 - 2 * H - f / kMiniFrags, p = f % kMiniFrags;
          const double a = fq[f % kAhead];
          if (p < 20) {            // W += V^T Z: one accumulator (a dependent chain of this MFMA issues at the full
            const int rt = st + p / 4, r = p % 4;   // rate of one per 64 cycles: tools/probe_mini_chain.hip)
            if (p == 0) wa = d4{0, 0, 0, 0};
            wa = __builtin_amdgcn_mfma_f64_16x16x4f64(a, ZT(rt)[r], wa, 0, 0, 0);
          } else {                 // Z -= (V T) W: the five row tiles take turns
            const int jj = p - 20, r = jj / 5, rt = st + jj % 5;
            ZT(rt) = __builtin_amdgcn_mfma_f64_16x16x4f64(a, wa[r], ZT(rt), 0, 0, 0);
          }
        }
        // ---- the fragments kAhead steps ahead take the registers the last two MFMAs have read (one 16-byte LDS read)
        if ((f & 1) && f + kAhead - 1 < kHalfFrags && !(dbg & 16)) {
          const d2l t = ldsP[((f + kAhead - 1) / 2) * 64];
          fq[(f - 1) % kAhead] = t[0];
          fq[f % kAhead] = t[1];
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      BT2_TRACE_POINT(H, 80)
      BT2_STAMP(7 * H + 6)
      // this wave's part of the half fetched during this slot must have landed before the barrier that opens the next
      // slot (and the stores of the finished rows with it); after a first half the four youngest loads (new rows, tiles
      // 2 and 3) stay in flight
      if (H == 0 && !(dbg & 2) && !(dbg & 64)) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else wait_vm0();
      slot = slot == 2 ? 0 : slot + 1;
    }
    // ---- slide by 64 rows = the next phase.  After the last diamond of a group the whole window goes back to memory.
    BT2_STAMP(14)
    if (more) {
      fin_row = win;
      have_fin = true;
    } else {
      if (!(dbg & 2)) {
#pragma unroll
        for (int t = 0; t < 8; ++t) store_tile(ZT(t), win + 16 * t);
      }
      have_fin = false;
    }
    BT2_STAMP(15)
    // nothing of this diamond may sink into the next one: behind its LDS-DMA issue the compiler would wait vmcnt(0) for it
    __builtin_amdgcn_sched_barrier(0);
#undef ZT
  };
  unsigned m0_keep;
  asm volatile("s_mov_b32 %0, m0" : "=s"(m0_keep));
  for (int S = SL.ngroups - 1; S >= 0; --S) {
    S_cur = S;
    const int d0 = dia_off[S], nk = dia_off[S + 1] - d0;
    const int nh = 2 * nk;                                    // halves of this group, streamed back to back
    int win = S * kG + 1;
    const double* fgrp = sb + SL.frag + (size_t)d0 * kFragDoubles;
    {
      Raw raw[8];
#pragma unroll
      for (int rt = 0; rt < 8; ++rt) load_raw(raw[rt], win + 16 * rt);
#pragma unroll
      for (int rt = 0; rt < 8; ++rt) scatter_tile(zz[rt], raw[rt], win + 16 * rt);
    }
    barrier();                       // every wave has left the previous group: the whole ring is free
    if (!(dbg & 1)) {
      dma_half(fgrp, 0);
    }
    wait_vm0();
    __builtin_amdgcn_sched_barrier(0);
    if (lag) {
      // time slot 0 of the trailing wave group: the leading group runs half 0; only this group's share of half 1's DMA
      if (!(dbg & 8)) barrier();
      if (!(dbg & 1) && !kDmaAllH0) {
        dma_half(fgrp + (size_t)(1 < nh ? 1 : 0) * kHalfDoubles, 1);
      }
      wait_vm0();
      __builtin_amdgcn_sched_barrier(0);
    }
    int slot = 0;                    // ring slot of the half about to run
    int ph = 0;
    for (int k = 0; k < nk; ++k, win += 64) {
      const bool more = k + 1 < nk;
      if (ph == 0) diamond(std::integral_constant<int, 0>{}, fgrp, k, nh, more, slot, win);
      else if (ph == 1) diamond(std::integral_constant<int, 1>{}, fgrp, k, nh, more, slot, win);
      else diamond(std::integral_constant<int, 2>{}, fgrp, k, nh, more, slot, win);
      ph = ph == 2 ? 0 : ph + 1;
    }
    // time slot nh of the leading group (the trailing one runs its last half): one barrier, so that both count the same
    if (kPhased && !lag && !(dbg & 8)) barrier();
  }
  asm volatile("s_mov_b32 m0, %0" : : "s"(m0_keep));
  BT2_STAMP_WRITE
  BT2_CLOCK_END
}

// ---- few columns (partial spectrum): one launch per WAVEFRONT of diamonds ------------------------------------------
// k_bt2_apply gives a workgroup 16 NW columns and lets it walk all diamonds in order: with the ~100 columns of a
// partial-spectrum solve that is two workgroups on the whole chip, each applying ~n^2 / 8192 diamonds one after the other
// (config C5, n = 24000: 70 000 diamonds, 470 ms).  Diamond (S, k) touches rows 64 S + 1 + 64 k .. + 126 and must follow
// (S, k - 1) and (S + 1, k .. k + 2): all diamonds with the same t = 3 (Smax - S) + k are independent.  Launch t runs
// them side by side, one workgroup per (diamond, 64 columns): window from memory, the same 160 MFMAs with the
// fragments read straight from L2, window back to memory.  n / 64 + 3 n / 64 launches instead of n^2 / 8192 serial steps.
__global__ __launch_bounds__(256) void k_bt2_wave(const double* __restrict__ sb_all, SbLayout SL,
                                                  const int* __restrict__ dia_off, double* __restrict__ z_all,
                                                  long long stride_z, int ncols, int t) {
  __shared__ double stg_all[4][16 * 18];
  const int n = SL.n;
  const int S = SL.ngroups - 1 - (int)blockIdx.x;
  const int k = t - 3 * (int)blockIdx.x;
  if (S < 0 || k < 0) return;
  const int d0 = dia_off[S], nk = dia_off[S + 1] - d0;
  if (k >= nk) return;
  const double* sb = sb_all + (size_t)blockIdx.z * SL.slab;
  const double* frag = sb + SL.frag + (size_t)(d0 + k) * kFragDoubles;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int col = ((int)blockIdx.y * 4 + w) * 16 + fr;
  const bool col_ok = col < ncols;
  const int win = S * kG + 1 + kB * k;
  double* stg = stg_all[w];
  const int gc = lane >> 3, gr = (lane & 7) * 2;
  const int col_a = ((int)blockIdx.y * 4 + w) * 16 + gc, col_b = col_a + 8;
  double* z_mat = z_all + (size_t)blockIdx.z * stride_z;
  double* za = z_mat + (size_t)(col_a < ncols ? col_a : ncols - 1) * n + gr;
  double* zb = z_mat + (size_t)(col_b < ncols ? col_b : ncols - 1) * n + gr;
  d4 zt[8];
  // window -> accumulator layout through the wave's transposition tile (same maps as k_bt2_apply)
#pragma unroll
  for (int rt = 0; rt < 8; ++rt) {
    const int row0 = win + 16 * rt;
    const int rs = row0 < n - 16 ? row0 : n - 16;
    const int shift = row0 < n - 16 ? 0 : row0 - (n - 16);
    double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
    if (rs >= 0) { a0 = za[rs]; a1 = za[rs + 1]; b0 = zb[rs]; b1 = zb[rs + 1]; }
    stg[gc * 18 + gr] = a0; stg[gc * 18 + gr + 1] = a1;
    stg[(gc + 8) * 18 + gr] = b0; stg[(gc + 8) * 18 + gr + 1] = b1;
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 4 * r + fk + shift;
      const double x = stg[fr * 18 + (i < 16 ? i : 15)];
      zt[rt][r] = (col_ok && row0 + 4 * r + fk < n) ? x : 0.0;
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  // the 160 MFMAs, fragments eight ahead
  constexpr int kAhead = 8;
  double fq[kAhead];
#pragma unroll
  for (int j = 0; j < kAhead; ++j) fq[j] = frag[frag_off(j, lane)];
  d4 wa = d4{0, 0, 0, 0};
#pragma unroll
  for (int f = 0; f < kDiaFrags; ++f) {
    const int st = 3 - f / kMiniFrags, p = f % kMiniFrags;
    const double a = fq[f % kAhead];
    if (p < 20) {
      const int rt = st + p / 4, r = p % 4;
      if (p == 0) wa = d4{0, 0, 0, 0};
      wa = __builtin_amdgcn_mfma_f64_16x16x4f64(a, zt[rt][r], wa, 0, 0, 0);
    } else {
      const int jj = p - 20, r = jj / 5, rt = st + jj % 5;
      zt[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, wa[r], zt[rt], 0, 0, 0);
    }
    if (f + kAhead < kDiaFrags) fq[f % kAhead] = frag[frag_off(f + kAhead, lane)];
  }
  // window back to memory
#pragma unroll
  for (int rt = 0; rt < 8; ++rt) {
    const int row0 = win + 16 * rt;
#pragma unroll
    for (int r = 0; r < 4; ++r) stg[fr * 18 + 4 * r + fk] = zt[rt][r];
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const double a0 = stg[gc * 18 + gr], a1 = stg[gc * 18 + gr + 1];
    const double b0 = stg[(gc + 8) * 18 + gr], b1 = stg[(gc + 8) * 18 + gr + 1];
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (col_a < ncols) {
      if (row0 + gr < n) za[row0] = a0;
      if (row0 + gr + 1 < n) za[row0 + 1] = a1;
    }
    if (col_b < ncols) {
      if (row0 + gr < n) zb[row0] = b0;
      if (row0 + gr + 1 < n) zb[row0 + 1] = b1;
    }
  }
}

}  // namespace

// ================================================================================================================
// T factors and V T of all diamonds, on `st` (they only depend on the bulge chase, not on Z).
int bt2_prepare(sc_ctx* ctx, int n, int batch, double* d_sb_ws, const SbLayout& SL, hipStream_t st) {
  if (n < 3 || SL.ndia == 0) return SC_OK;
  for (auto& ph : ctx->phases)
    if (ph.first == "dia_tfactor") ph.second = 0.0;
  for (long long d0 = 0; d0 < SL.ndia; d0 += 32768) {
    const unsigned cnt = (unsigned)std::min<long long>(32768, SL.ndia - d0);
    hipLaunchKernelGGL(k_dia_tfactor2, dim3(cnt, (unsigned)batch), dim3(256), 0, st, d_sb_ws, SL, (int)d0);
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

// Z <- Q2 Z (after bt2_prepare).  d_z: (batch) ncols columns of length n (ld n).
int bt2_batched(sc_ctx* ctx, int n, int batch, double* d_sb_ws, const SbLayout& SL, const int* d_dia_off, double* d_z,
                long long stride_z, int ncols, float* ms_fused) {
  hipStream_t st = ctx->stream;
  if (n < 3 || SL.ndia == 0 || ncols <= 0) return SC_OK;
  ScopedEvents<2> ev;
  const bool prof = ctx->profiling && ms_fused;
  if (prof) {
    for (auto& e : ev) SC_HIP(ctx, hipEventCreate(&e));
    SC_HIP(ctx, hipEventRecord(ev[0], st));
  }
  const sc_host::Bt2Plan P = sc_host::bt2_plan(sc_host::two_stage_env(), n, batch, ncols, ctx->num_cus);
  ++ctx->cnt_bt2_form[P.wave ? 0 : (P.nw == 8 ? 2 : 1)];
  if (P.wave) {
    int nk0 = 0;
    {
      const std::vector<int> doff = dia_offsets(n);
      for (size_t S = 0; S + 1 < doff.size(); ++S) nk0 = std::max(nk0, doff[S + 1] - doff[S]);
    }
    const int t_last = 3 * (SL.ngroups - 1) + nk0 - 1;
    for (int t = 0; t <= t_last; ++t) {
      const int gx = std::min(t / 3, SL.ngroups - 1) + 1;
      hipLaunchKernelGGL(k_bt2_wave, dim3((unsigned)gx, (unsigned)((ncols + 63) / 64), (unsigned)batch), dim3(256), 0, st,
                         d_sb_ws, SL, d_dia_off, d_z, stride_z, ncols, t);
    }
  } else {
    // ring of three half-diamond fragment buffers + one 16 x 18 transposition tile per wave
    constexpr size_t lds = sizeof(double) * (3 * kHalfDoubles + 8 * 16 * 18);
    // (per device, with the answer checked -- ADVICE round 5: a process-wide flag left a context on a second GPU with a
    // refused 138 KB launch)
    if (!sc_raise_dyn_lds(reinterpret_cast<const void*>(&k_bt2_apply<8>), (int)lds) ||
        !sc_raise_dyn_lds(reinterpret_cast<const void*>(&k_bt2_apply<4>), (int)lds))
      return sc_set_error(ctx, SC_ERR_HIP, "k_bt2_apply: the device refuses %zu bytes of dynamic LDS", lds);
    const dim3 grid(P.grid_x, P.grid_y);
    if (P.xcd) ++ctx->cnt_bt2_xcd;
    if (P.nw == 8)
      hipLaunchKernelGGL(k_bt2_apply<8>, grid, dim3(512), lds, st, d_sb_ws, SL, d_dia_off, d_z, stride_z, ncols, batch,
                         P.xcd ? 1 : 0);
    else
      hipLaunchKernelGGL(k_bt2_apply<4>, grid, dim3(256), lds, st, d_sb_ws, SL, d_dia_off, d_z, stride_z, ncols, batch,
                         P.xcd ? 1 : 0);
  }
  SC_HIP(ctx, hipGetLastError());
  if (prof) {
    SC_HIP(ctx, hipEventRecord(ev[1], st));
    SC_HIP(ctx, hipEventSynchronize(ev[1]));
    SC_HIP(ctx, hipEventElapsedTime(ms_fused, ev[0], ev[1]));
  }
  return SC_OK;
}

// ---- diagnostic build only (-DBT2_TRACE): time stamps in front of every MFMA of one diamond, [wave][half][81]
extern "C" int sc_dbg_bt2_trace(unsigned long long* out) {
#ifdef BT2_TRACE
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bt2_trace), sizeof(unsigned long long) * 8 * 2 * 81) == hipSuccess ? 0 : 5;
#else
  (void)out;
  return 1;
#endif
}

extern "C" int sc_dbg_bt2_clock(unsigned long long* out2) {
#ifdef BT2_CLOCK
  return hipMemcpyFromSymbol(out2, HIP_SYMBOL(g_bt2_clk), sizeof(unsigned long long) * 2) == hipSuccess ? 0 : 5;
#else
  (void)out2;
  return 1;
#endif
}

// ---- diagnostic build only: per-wave segment sums of k_bt2_apply (first 64 workgroups x 8 waves x (8 sums + count))
extern "C" int sc_dbg_bt2_stamps(unsigned long long* out) {
#ifdef BT2_STAMPS
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bt2_stamps), sizeof(unsigned long long) * 64 * 8 * 17) == hipSuccess ? 0 : 5;
#else
  (void)out;
  return 1;
#endif
}
