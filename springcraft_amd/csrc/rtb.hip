// Rotation-translation blocks (RTB): the Hessian of an elastic network projected onto the rigid-body motions of blocks
// of atoms, H_b = P^T H P, straight from the ordered pair list, and the expansion of block modes back to atoms, v = P u.
// Neither forms the (3N, 3N) Hessian: the projection reads k pairs and writes (nr, nr), nr = sum of the blocks' degrees of
// freedom (<= 6 each); the expansion streams (nvec, 3N) out once.
//
// Projector: d_P (N, 3, 6) row-major, atom a's three rows of its block's <= 6 columns (unused columns are 0.0);
// d_block_of_atom (N) int32; d_offset (n_blocks + 1) int64, block b owns rows / columns offset[b] .. offset[b + 1] - 1.
//
// Projection.  With d = r_j - r_i, g = gamma_p / |d|^2, t_a = s_a P[a]^T d (s = inv_sqrt_mass, 1 if null) every directed
// pair p = (i, j), I = block(i), J = block(j), contributes
//     -g t_i t_j^T  to H_b[I, J]      (sc_hessian_from_pairs_f64: block (i, j) = -gamma(i, j) d d^T / |d|^2)
//     +g t_j t_j^T  to H_b[J, J]      (its diagonal block of atom j is minus the sum of column j's blocks)
// The caller hands in the pairs' order sorted by (J, I) (stable, so the order inside a segment is the pair list's), the
// starts of the (J, I) segments and, per block J, the start of its first segment.  One wavefront owns one segment
// (k_rtb_blocks<false>) or one block's diagonal (k_rtb_blocks<true>): lane l takes the segment's pairs l, l + 64, ... in
// ascending order into 36 private sums, a fixed xor butterfly adds the lanes, and lane e < 36 stores entry e of the 6 x 6
// block once.  No atomics: a result's bits depend on the inputs alone.  The diagonal pass runs after the segment pass and
// adds to the (J, J) block that pass (or the memset) left.
#include "common.h"

namespace {

struct Vec6 {
  double c[6];
};

// t = scale * P[a]^T d: the atom's three rows of 6 doubles as nine 16-byte loads (a row is 48 bytes, an atom 144)
__device__ __forceinline__ Vec6 project_atom(const double* __restrict__ P, long long a, double dx, double dy, double dz,
                                             double scale) {
  const double2* row = reinterpret_cast<const double2*>(P + a * 18);
  Vec6 t;
#pragma unroll
  for (int h = 0; h < 3; ++h) {
    const double2 x = row[h], y = row[3 + h], z = row[6 + h];
    t.c[2 * h] = scale * ((x.x * dx + y.x * dy) + z.x * dz);
    t.c[2 * h + 1] = scale * ((x.y * dx + y.y * dy) + z.y * dz);
  }
  return t;
}

template <bool DIAG>
__global__ __launch_bounds__(256) void k_rtb_blocks(const double* __restrict__ coord, long long n_atoms,
                                                    const long long* __restrict__ pairs, long long k,
                                                    const double* __restrict__ gamma, const double* __restrict__ ism,
                                                    const double* __restrict__ P, const int* __restrict__ boa,
                                                    const long long* __restrict__ offset, long long n_blocks,
                                                    long long nr, const long long* __restrict__ order,
                                                    const long long* __restrict__ start, long long n_work,
                                                    double* __restrict__ hb) {
  const int lane = threadIdx.x & 63;
  const long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= n_work) return;
  long long lo = start[s], hi = start[s + 1];
  if (lo < 0) lo = 0;
  if (hi > k) hi = k;
  if (lo >= hi) return;   // (a block no pair ends in: the memset's zeros stay)

  double acc[36];
#pragma unroll
  for (int e = 0; e < 36; ++e) acc[e] = 0.0;

  for (long long t = lo + lane; t < hi; t += 64) {
    const long long p = order[t];
    if (p < 0 || p >= k) continue;
    const long long i = pairs[2 * p], j = pairs[2 * p + 1];
    if (i < 0 || i >= n_atoms || j < 0 || j >= n_atoms) continue;
    const double dx = coord[3 * j + 0] - coord[3 * i + 0];
    const double dy = coord[3 * j + 1] - coord[3 * i + 1];
    const double dz = coord[3 * j + 2] - coord[3 * i + 2];
    const double g = gamma[p] / ((dx * dx + dy * dy) + dz * dz);
    const Vec6 tj = project_atom(P, j, dx, dy, dz, ism ? ism[j] : 1.0);
    Vec6 ti;
    if (DIAG) {
#pragma unroll
      for (int a = 0; a < 6; ++a) ti.c[a] = g * tj.c[a];
    } else {
      ti = project_atom(P, i, dx, dy, dz, ism ? -g * ism[i] : -g);
    }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < 6; ++b) acc[a * 6 + b] += ti.c[a] * tj.c[b];
  }

  // every lane ends with the same bits: at each level the two partners add the same two numbers
  double mine = 0.0;
#pragma unroll
  for (int e = 0; e < 36; ++e) {
    double v = acc[e];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if (lane == e) mine = v;
  }
  if (lane >= 36) return;

  // the segment's blocks, from its first pair (every pair of a segment has the same)
  const long long p0 = order[lo];
  if (p0 < 0 || p0 >= k) return;
  const long long i0 = pairs[2 * p0], j0 = pairs[2 * p0 + 1];
  if (i0 < 0 || i0 >= n_atoms || j0 < 0 || j0 >= n_atoms) return;
  const long long J = DIAG ? s : boa[j0];
  const long long I = DIAG ? s : boa[i0];
  if (I < 0 || I >= n_blocks || J < 0 || J >= n_blocks) return;
  const long long ro = offset[I], co = offset[J];
  const int a = lane / 6, b = lane % 6;
  if (a >= offset[I + 1] - ro || b >= offset[J + 1] - co) return;
  if (ro < 0 || co < 0 || ro + a >= nr || co + b >= nr) return;
  double* dst = hb + (size_t)(ro + a) * (size_t)nr + (size_t)(co + b);
  if (DIAG) *dst += mine; else *dst = mine;
}

// V[r, 3 a + al] = sum_c P[a, al, c] U[r, offset[block(a)] + c]: a thread owns one column of V, keeps its row of P in
// registers and walks kExpandRows rows of U; consecutive threads store consecutive doubles.
constexpr int kExpandRows = 8;

__global__ __launch_bounds__(256) void k_rtb_expand(const double* __restrict__ U, long long nvec, long long nr,
                                                    const double* __restrict__ P, const int* __restrict__ boa,
                                                    const long long* __restrict__ offset, long long n3,
                                                    double* __restrict__ V) {
  const long long col = (long long)blockIdx.x * 256 + threadIdx.x;
  if (col >= n3) return;
  const long long a = col / 3;
  const long long blk = boa[a];
  long long off = 0;
  int dof = 0;
  if (blk >= 0) {   // (block_of_atom is the caller's, like every index array of the device entries)
    off = offset[blk];
    const long long d = offset[blk + 1] - off;
    dof = d < 0 ? 0 : (d > 6 ? 6 : (int)d);
    if (off < 0 || off + dof > nr) dof = 0;
  }
  const double2* row = reinterpret_cast<const double2*>(P + col * 6);
  const double2 p01 = row[0], p23 = row[1], p45 = row[2];
  const double p[6] = {p01.x, p01.y, p23.x, p23.y, p45.x, p45.y};
  const long long r0 = (long long)blockIdx.y * kExpandRows;
  const long long r1 = r0 + kExpandRows < nvec ? r0 + kExpandRows : nvec;
  for (long long r = r0; r < r1; ++r) {
    const double* u = U + r * nr + off;
    double sum = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c)
      if (c < dof) sum += p[c] * u[c];
    V[r * n3 + col] = sum;
  }
}

}  // namespace

int launch_rtb_hessian(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, const int64_t* d_pairs, int64_t k,
                       const double* d_gamma, const double* d_ism, const double* d_P, const int32_t* d_boa,
                       const int64_t* d_offset, int64_t n_blocks, int64_t nr, const int64_t* d_order,
                       const int64_t* d_seg_start, int64_t n_seg, const int64_t* d_blk_start, double* d_hb) {
  SC_HIP(ctx, hipMemsetAsync(d_hb, 0, sizeof(double) * (size_t)nr * (size_t)nr, ctx->stream));
  if (k > 0 && n_seg > 0) {
    hipLaunchKernelGGL((k_rtb_blocks<false>), dim3((unsigned)((n_seg + 3) / 4)), dim3(256), 0, ctx->stream, d_coord,
                       (long long)n_atoms, (const long long*)d_pairs, (long long)k, d_gamma, d_ism, d_P, d_boa,
                       (const long long*)d_offset, (long long)n_blocks, (long long)nr, (const long long*)d_order,
                       (const long long*)d_seg_start, (long long)n_seg, d_hb);
    hipLaunchKernelGGL((k_rtb_blocks<true>), dim3((unsigned)((n_blocks + 3) / 4)), dim3(256), 0, ctx->stream, d_coord,
                       (long long)n_atoms, (const long long*)d_pairs, (long long)k, d_gamma, d_ism, d_P, d_boa,
                       (const long long*)d_offset, (long long)n_blocks, (long long)nr, (const long long*)d_order,
                       (const long long*)d_blk_start, (long long)n_blocks, d_hb);
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

int launch_rtb_expand(sc_ctx* ctx, const double* d_u, int64_t nvec, int64_t nr, const double* d_P, const int32_t* d_boa,
                      const int64_t* d_offset, int64_t n_atoms, double* d_v) {
  const long long n3 = 3 * (long long)n_atoms;
  const dim3 grid((unsigned)((n3 + 255) / 256), (unsigned)((nvec + kExpandRows - 1) / kExpandRows));
  hipLaunchKernelGGL(k_rtb_expand, grid, dim3(256), 0, ctx->stream, d_u, (long long)nvec, (long long)nr, d_P, d_boa,
                     (const long long*)d_offset, n3, d_v);
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}
