// Correlation networks: the weighted residue graph of a coupling map, the shortest communication path between every pair
// of residues and how many of those paths every residue carries.  No reference counterpart (Bio3D: cna on dccm / lmi;
// Sethi et al. 2009; WISP; the shortest paths and betweenness of a graph library).
//
// Every kernel works on the packed pair layout: member b is an (n_b, n_b) row-major block at element offset off_b, and one
// launch serves a uniform and a ragged batch through the members' records (n_b, off_b, atom_off_b).  Members are grid axis
// y, the other axis is sized by the largest member, and a workgroup outside its member exits.  All positions are relative
// to the member, so a member's bits depend on its own input alone: not on the batch, its place in it or its neighbours.
//
// k_net_weights, one pass: W[a, c] = -log(min(|c_ac|, 1)) where |c_ac| >= min_correlation and, with coordinates, |x_a - x_c|^2
// <= cutoff^2; +inf elsewhere; 0 on the diagonal.  A NaN in a member's map or coordinates sets the member's flag.
//
// Shortest paths: blocked Floyd-Warshall in the (min, +) semiring on float64 with 64 x 64 tiles, D[i, j] = min(D[i, j],
// D[i, k] + D[k, j]), and the next hop S[i, j] (int32) of the stored path beside it.  k_net_init: D = W with a zero
// diagonal, S[i, j] = j for a finite edge, S[i, i] = i, -1 elsewhere; a NaN or negative weight sets the flag.  Round r of
// ceil(n_max / 64), three launches:
//   1  the pivot tile (r, r) closed on itself in LDS;
//   2  the tiles of the pivot's row and column against the closed pivot, 64 dependent steps each in LDS;
//   3  every other tile (i, j), independent: the K = 64 min-plus product of tile (i, r) and tile (r, j).
// An entry changes on strict improvement only, k ascending, and takes S[i, j] <- S[i, k].  In step k of phases 1 and 2 row
// k and column k of the tile do not change (the pivot's diagonal is exactly 0 and no sum of non-negative weights is below
// its addend), so one barrier per step orders the tile's reads and writes.  Pad rows and columns of a partial tile are
// +inf / -1 in LDS and are never stored.  inf + inf = inf: no NaN arises.  Both candidates of D[i, j] and D[j, i] are the
// same two addends in the same k order, so a symmetric input gives D equal to its transpose bit for bit.  No atomics, no
// partial results across workgroups.  k_net_finish turns a flagged member into NaN / -1 and touches nothing else.
//
// Phase 3 is the hot path: 2 n^3 float64 additions and comparisons per member over all rounds.  A workgroup of 256 lanes
// holds tile (i, r) transposed, At[k][i], tile (r, j) as B[k][j] and the int32 next hops of tile (i, r) transposed in LDS:
// 32 + 32 + 16 KB, two workgroups per CU.  A lane owns rows {2 ty, 2 ty + 1, 32 + 2 ty, 33 + 2 ty} and the same columns of
// tx: a 4 x 4 block of D and S in registers.  Per k it reads 2 x 16 bytes of At, 2 x 16 bytes of B and 2 x 8 bytes of St:
// the 16 lanes of a tx run read 256 consecutive bytes of B, the lanes of one ty the same address.  The transposing store
// puts element (k, i) at column i ^ 2 (k & 15), which keeps the pairs together and spreads a store's 16 lanes over the banks.
//
// k_net_usage, one workgroup per (member, target t): column t of S and n counters in LDS (2 x 4 n bytes, n <= 8192); lanes
// stride over the sources a and walk a -> S[a, t] -> ... -> t, adding 1 to the counter of every interior node (integer LDS
// adds: the sum has no order).  A walk leaves after n hops or at a next hop outside 0 .. n - 1 and sets the member's flag.
// The workgroup writes row t of an int32 workspace; k_net_usage_sum adds the rows in ascending t into int64.  One stored
// path per pair: on ties this is not Brandes' fractional betweenness.
#include <cmath>

#include "network_internal.h"

// (the contact test's squared distance is the three products and two sums as written)
#pragma clang fp contract(off)

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef int i2 __attribute__((ext_vector_type(2)));

constexpr int kT = sc_host::kNetTile;
constexpr int kTT = kT * kT;
static_assert(kT == 64, "the lane mappings below are written for 64 x 64 tiles and 256 lanes");

struct Rec { long long n, off, atom_off; };
__device__ __forceinline__ Rec load_rec(const long long* __restrict__ rec, int b) {
  const long long* r = rec + (long long)sc_host::kNetRecInts * b;
  return Rec{r[0], r[1], r[2]};
}
__device__ __forceinline__ double pos_inf() { return __builtin_huge_val(); }

// ---- streaming passes: grid (ceil(n_max^2 / 256), count) ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_net_weights(const long long* __restrict__ rec, long long n_max,
                                                     const double* __restrict__ corr, const double* __restrict__ coord,
                                                     double cutoff_sq, double min_corr, double* __restrict__ W,
                                                     int* __restrict__ flags) {
  const int b = blockIdx.y;
  const Rec R = load_rec(rec, b);
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (R.n > n_max || idx >= R.n * R.n) return;
  const long long a = idx / R.n, c = idx - a * R.n;
  const double v = corr[R.off + idx];
  bool bad = v != v;
  const double ac = fabs(v);
  bool edge = ac >= min_corr;
  if (coord) {
    const double* xa = coord + 3 * (R.atom_off + a);
    const double* xc = coord + 3 * (R.atom_off + c);
    const double d0 = xa[0] - xc[0], d1 = xa[1] - xc[1], d2 = xa[2] - xc[2];
    const double dist_sq = (d0 * d0 + d1 * d1) + d2 * d2;
    bad = bad || dist_sq != dist_sq;
    edge = edge && dist_sq <= cutoff_sq;
  }
  double w = edge ? (ac >= 1.0 ? 0.0 : -log(ac)) : pos_inf();
  if (a == c) w = 0.0;
  W[R.off + idx] = w;
  if (bad) flags[b] = 1;   // (every writer writes the same value)
}

__global__ __launch_bounds__(256) void k_net_init(const long long* __restrict__ rec, long long n_max, const double* W,
                                                  double* D, int* __restrict__ S, int* __restrict__ flags) {
  const int b = blockIdx.y;
  const Rec R = load_rec(rec, b);
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (R.n > n_max || idx >= R.n * R.n) return;
  const long long a = idx / R.n, c = idx - a * R.n;
  const double w = W[R.off + idx];
  if (!(w >= 0.0)) flags[b] = 1;   // NaN or negative
  const bool diag = a == c;
  D[R.off + idx] = diag ? 0.0 : w;
  S[R.off + idx] = diag ? (int)a : (w < pos_inf() ? (int)c : -1);
}

__global__ __launch_bounds__(256) void k_net_finish(const long long* __restrict__ rec, long long n_max, double* __restrict__ D,
                                                    int* __restrict__ S, const int* __restrict__ flags) {
  const int b = blockIdx.y;
  if (!flags[b]) return;
  const Rec R = load_rec(rec, b);
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (R.n > n_max || idx >= R.n * R.n) return;
  D[R.off + idx] = __builtin_nan("");
  S[R.off + idx] = -1;
}

// ---- phases 1 and 2 -----------------------------------------------------------------------------------------------------------
// tile (ti, tj) of a member -> LDS, row-major; outside the member +inf / -1
__device__ __forceinline__ void load_tile(const double* D, const int* S, long long n, int ti, int tj, double* X, int* XS) {
  for (int e = threadIdx.x; e < kTT; e += 256) {
    const long long gi = (long long)ti * kT + (e >> 6), gj = (long long)tj * kT + (e & 63);
    const bool in = gi < n && gj < n;
    X[e] = in ? D[gi * n + gj] : pos_inf();
    XS[e] = in ? S[gi * n + gj] : -1;
  }
}

// kPhase 1: grid (1, count), the pivot tile.  kPhase 2: grid (2 T_max, count): x < T_max is tile (round, x) of the pivot's
// row, else tile (x - T_max, round) of its column.
template <int kPhase>
__global__ __launch_bounds__(256) void k_fw_dependent(const long long* __restrict__ rec, long long n_max, int round, double* D,
                                                      int* S) {
  __shared__ double X[kTT];
  __shared__ int XS[kTT];
  __shared__ double P[kPhase == 2 ? kTT : 1];
  __shared__ int PS[kPhase == 2 ? kTT : 1];
  const Rec R = load_rec(rec, blockIdx.y);
  const int tiles = (int)((R.n + kT - 1) / kT);
  if (R.n > n_max || round >= tiles) return;
  int ti = round, tj = round;
  bool row = false;
  if (kPhase == 2) {
    const int t_max = gridDim.x / 2;
    row = (int)blockIdx.x < t_max;
    const int t = row ? blockIdx.x : blockIdx.x - t_max;
    if (t == round || t >= tiles) return;
    ti = row ? round : t;
    tj = row ? t : round;
    load_tile(D + R.off, S + R.off, R.n, round, round, P, PS);
  }
  load_tile(D + R.off, S + R.off, R.n, ti, tj, X, XS);
  // candidate of entry (i, j) in step k: A[i][k] + B[k][j], next hop SA[i][k]
  const double* A = (kPhase == 2 && row) ? P : X;
  const int* SA = (kPhase == 2 && row) ? PS : XS;
  const double* B = (kPhase == 2 && !row) ? P : X;
  const int i0 = 4 * (threadIdx.x >> 4), j0 = 4 * (threadIdx.x & 15);
  for (int k = 0; k < kT; ++k) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double a = A[(i0 + r) * kT + k];
      const int sa = SA[(i0 + r) * kT + k];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int e = (i0 + r) * kT + j0 + c;
        const double cand = a + B[k * kT + j0 + c];
        if (cand < X[e]) {
          X[e] = cand;
          XS[e] = sa;
        }
      }
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kTT; e += 256) {
    const long long gi = (long long)ti * kT + (e >> 6), gj = (long long)tj * kT + (e & 63);
    if (gi < R.n && gj < R.n) {
      D[R.off + gi * R.n + gj] = X[e];
      S[R.off + gi * R.n + gj] = XS[e];
    }
  }
}

// ---- phase 3: grid (T_max^2, count) -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fw_independent(const long long* __restrict__ rec, long long n_max, int round, double* D,
                                                        int* S) {
  __shared__ __attribute__((aligned(16))) double At[kTT];   // [k][i ^ swizzle(k)] = D[tile i rows][pivot columns]
  __shared__ __attribute__((aligned(16))) double B[kTT];    // [k][j] = D[pivot rows][tile j columns]
  __shared__ __attribute__((aligned(16))) int St[kTT];      // next hops of At's entries, same places
  const Rec R = load_rec(rec, blockIdx.y);
  const int tiles = (int)((R.n + kT - 1) / kT);
  const int t_max = (int)((n_max + kT - 1) / kT);
  const int ti = blockIdx.x / t_max, tj = blockIdx.x - ti * t_max;
  if (R.n > n_max || round >= tiles || ti >= tiles || tj >= tiles || ti == round || tj == round) return;
  const long long n = R.n;
  double* Dm = D + R.off;
  int* Sm = S + R.off;
  const int tid = threadIdx.x;
  for (int e = tid; e < kTT; e += 256) {
    const int hi = e >> 6, lo = e & 63;
    {   // (i, k) = (hi, lo): consecutive lanes read consecutive k
      const long long gi = (long long)ti * kT + hi, gk = (long long)round * kT + lo;
      const bool in = gi < n && gk < n;
      const int at = lo * kT + (hi ^ ((lo & 15) << 1));
      At[at] = in ? Dm[gi * n + gk] : pos_inf();
      St[at] = in ? Sm[gi * n + gk] : -1;
    }
    {   // (k, j) = (hi, lo)
      const long long gk = (long long)round * kT + hi, gj = (long long)tj * kT + lo;
      B[e] = (gk < n && gj < n) ? Dm[gk * n + gj] : pos_inf();
    }
  }
  const int tx = tid & 15, ty = tid >> 4;
  int li[4], lj[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    li[r] = 32 * (r >> 1) + 2 * ty + (r & 1);
    lj[r] = 32 * (r >> 1) + 2 * tx + (r & 1);
  }
  double d[4][4];
  int s[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long long gi = (long long)ti * kT + li[r], gj = (long long)tj * kT + lj[c];
      const bool in = gi < n && gj < n;
      d[r][c] = in ? Dm[gi * n + gj] : pos_inf();
      s[r][c] = in ? Sm[gi * n + gj] : -1;
    }
  __syncthreads();
  for (int k0 = 0; k0 < kT; k0 += 16) {
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const int k = k0 + kk, col = (2 * ty) ^ (kk << 1);
      const d2 a01 = *reinterpret_cast<const d2*>(&At[k * kT + col]);
      const d2 a23 = *reinterpret_cast<const d2*>(&At[k * kT + 32 + col]);
      const i2 s01 = *reinterpret_cast<const i2*>(&St[k * kT + col]);
      const i2 s23 = *reinterpret_cast<const i2*>(&St[k * kT + 32 + col]);
      const d2 b01 = *reinterpret_cast<const d2*>(&B[k * kT + 2 * tx]);
      const d2 b23 = *reinterpret_cast<const d2*>(&B[k * kT + 32 + 2 * tx]);
      const double a[4] = {a01.x, a01.y, a23.x, a23.y};
      const double bb[4] = {b01.x, b01.y, b23.x, b23.y};
      const int sa[4] = {s01.x, s01.y, s23.x, s23.y};
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double cand = a[r] + bb[c];
          const bool better = cand < d[r][c];
          d[r][c] = better ? cand : d[r][c];
          s[r][c] = better ? sa[r] : s[r][c];
        }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long long gi = (long long)ti * kT + li[r], gj = (long long)tj * kT + lj[c];
      if (gi < n && gj < n) {
        Dm[gi * n + gj] = d[r][c];
        Sm[gi * n + gj] = s[r][c];
      }
    }
}

// ---- path usage ----------------------------------------------------------------------------------------------------------------------
// grid (n_max, count), dynamic LDS 2 x 4 n_max bytes
__global__ __launch_bounds__(256) void k_net_usage(const long long* __restrict__ rec, long long n_max, const int* __restrict__ S,
                                                   int* __restrict__ through, int* __restrict__ flags) {
  extern __shared__ int usage_lds[];
  const int b = blockIdx.y;
  const Rec R = load_rec(rec, b);
  const long long t = blockIdx.x;
  if (R.n > n_max || t >= R.n) return;
  const int n = (int)R.n;
  int* hop = usage_lds;         // column t of S
  int* cnt = usage_lds + n_max;
  for (int a = threadIdx.x; a < n; a += 256) {
    hop[a] = S[R.off + (long long)a * n + t];
    cnt[a] = 0;
  }
  __syncthreads();
  bool bad = false;
  for (int a = threadIdx.x; a < n; a += 256) {
    if (a == t) continue;
    int v = hop[a];
    if (v == -1) continue;   // t is not reachable from a
    for (int hops = 0; v != t; ++hops) {
      if ((unsigned)v >= (unsigned)n || hops >= n) {
        bad = true;
        break;
      }
      atomicAdd(&cnt[v], 1);
      v = hop[v];
    }
  }
  __syncthreads();
  for (int v = threadIdx.x; v < n; v += 256) through[R.off + t * n + v] = cnt[v];
  if (bad) flags[b] = 1;
}

// grid (ceil(n_max / 256), count): usage[v] = sum over t ascending; -1 for a flagged member
__global__ __launch_bounds__(256) void k_net_usage_sum(const long long* __restrict__ rec, long long n_max,
                                                       const int* __restrict__ through, const int* __restrict__ flags,
                                                       long long* __restrict__ usage) {
  const int b = blockIdx.y;
  const Rec R = load_rec(rec, b);
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (R.n > n_max || v >= R.n) return;
  long long sum = 0;
  for (long long t = 0; t < R.n; ++t) sum += through[R.off + t * R.n + v];
  usage[R.atom_off + v] = flags[b] ? -1 : sum;
}

dim3 stream_grid(int64_t count, int64_t n_max) {
  return dim3((unsigned)((n_max * n_max + 255) / 256), (unsigned)count);
}

}  // namespace

int launch_net_weights(sc_ctx* ctx, const int64_t* d_rec, int64_t count, int64_t n_max, const double* d_corr,
                       const double* d_coord, double cutoff_sq, double min_correlation, double* d_w, int32_t* d_flags) {
  hipStream_t st = ctx->stream;
  SC_HIP(ctx, hipMemsetAsync(d_flags, 0, sizeof(int32_t) * (size_t)count, st));
  hipLaunchKernelGGL(k_net_weights, stream_grid(count, n_max), dim3(256), 0, st, (const long long*)d_rec, (long long)n_max,
                     d_corr, d_coord, cutoff_sq, min_correlation, d_w, d_flags);
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

int launch_net_paths(sc_ctx* ctx, const int64_t* d_rec, int64_t count, int64_t n_max, const double* d_w, double* d_d,
                     int32_t* d_s, int32_t* d_flags) {
  hipStream_t st = ctx->stream;
  const long long* rec = (const long long*)d_rec;
  const long long nm = n_max;
  const unsigned tiles = (unsigned)sc_host::net_tiles(n_max), members = (unsigned)count;
  hipLaunchKernelGGL(k_net_init, stream_grid(count, n_max), dim3(256), 0, st, rec, nm, d_w, d_d, d_s, d_flags);
  for (int round = 0; round < (int)tiles; ++round) {
    hipLaunchKernelGGL(k_fw_dependent<1>, dim3(1, members), dim3(256), 0, st, rec, nm, round, d_d, d_s);
    if (tiles > 1) {
      hipLaunchKernelGGL(k_fw_dependent<2>, dim3(2 * tiles, members), dim3(256), 0, st, rec, nm, round, d_d, d_s);
      hipLaunchKernelGGL(k_fw_independent, dim3(tiles * tiles, members), dim3(256), 0, st, rec, nm, round, d_d, d_s);
    }
  }
  hipLaunchKernelGGL(k_net_finish, stream_grid(count, n_max), dim3(256), 0, st, rec, nm, d_d, d_s, (const int*)d_flags);
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

int launch_net_usage(sc_ctx* ctx, const int64_t* d_rec, int64_t count, int64_t n_max, const int32_t* d_s, int32_t* d_through,
                     int64_t* d_usage, int32_t* d_flags) {
  hipStream_t st = ctx->stream;
  const long long* rec = (const long long*)d_rec;
  hipLaunchKernelGGL(k_net_usage, dim3((unsigned)n_max, (unsigned)count), dim3(256), sc_host::net_usage_lds_bytes(n_max), st, rec,
                     (long long)n_max, d_s, d_through, d_flags);
  hipLaunchKernelGGL(k_net_usage_sum, dim3((unsigned)((n_max + 255) / 256), (unsigned)count), dim3(256), 0, st, rec,
                     (long long)n_max, (const int*)d_through, (const int*)d_flags, (long long*)d_usage);
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}
