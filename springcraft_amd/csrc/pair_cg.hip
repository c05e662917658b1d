// Conjugate gradients on the pair-list operator for q right-hand sides at once: the kernels of one iteration.
// No reference counterpart.  The matrix T H T is the one of k_pairs_panel (pair_panel.hip), applied by the same walk
// (pair_walk.h); what CG adds is a per-column inner product fused into that walk and per-column coefficients that stay on
// the device.  Compiled with -ffp-contract=off (build.py): every operation is the one written.
//
// Layout.  Panels X, R, P, Q have m = dim N rows and q columns with leading dimension ld >= q, columns are the vectors
// (pair_panel.hip).  The state is seven rows of ld 8-byte words, row r of column c at state[r ld + c]:
//     0 rho = <r, r>   1 stop = (tol |f|)^2   2 alpha   3 beta        (double)
//     4 status: 0 running, 1 converged, 2 broken down   5 iters      (int64)
//     6 pq = <p, (T H T) p> of the last iteration                    (double)
// The workspace holds one partial sum per (workgroup of four atoms, column): work[b q + c], b < ceil(N / 4).
//
// One iteration, five kernels on one stream, no atomics, no host synchronisation:
//   k_cg_apply_dot   Q <- (T H T) P by the walk of k_pairs_panel -- one wavefront per (atom, 64 columns), four consecutive
//                    atoms per workgroup, the bits of panel_step(P, Q, 1, 0, 0) -- and the lane's p[i] . q[i] of its atom; the
//                    four wavefronts' terms are added in wavefront order through LDS (2 KiB: lane = column, consecutive
//                    doubles, no bank conflict) and stored to work[blockIdx.x][col]
//   k_cg_reduce<PQ>  pq_c = sum of the partials, alpha_c = rho_c / pq_c; pq_c not finite and positive: status 2; a column with
//                    status != 0 gets alpha_c = 0
//   k_cg_update      X += alpha P, R -= alpha Q for running columns and the partials of <r, r>, the same (four atoms, 64
//                    columns) per workgroup as above: a streaming pass with dim rows per lane, all loads of a lane
//                    independent (about 30 VGPRs, eight wavefronts per SIMD)
//   k_cg_reduce<RR>  rho_new = sum, beta = rho_new / rho, rho <- rho_new, iters += 1, status 1 when rho_new <= stop
//   k_cg_direction   P <- R + beta P for running columns
// The reduction of a column: sixteen wavefronts of one workgroup, lane = column, wavefront w adds the partials b = w, w + 16,
// ... in ascending order, and the sixteen sums are added in wavefront order through LDS.  The order depends on N alone.
//
// Promises.  Lanes beyond q write nothing: columns q .. ld - 1 of the panels and of the state keep their bits.  A column's
// bits in X, R, P, rho and iters depend on its own right-hand side and the network only, not on q, ld, its position or the
// other columns.  A column with status != 0 is frozen: no kernel writes its X, R, P, rho or iters, however many iterations
// follow (its Q is still overwritten).  An atom without pairs contributes exactly 0 to Q and to the dots.
#include "pair_walk.h"

namespace {

enum { CG_RHO = 0, CG_STOP = 1, CG_ALPHA = 2, CG_BETA = 3, CG_STATUS = 4, CG_ITERS = 5, CG_PQ = 6 };
enum { RED_INIT = 0, RED_PQ = 1, RED_RR = 2 };
constexpr int RED_WAVES = 16;

// the four wavefronts' values of a column, added in wavefront order; the result in the lanes of wavefront 0
__device__ __forceinline__ bool combine4(double v, int wave, int lane, double* lds, double& sum) {
  lds[wave * 64 + lane] = v;
  __syncthreads();
  if (wave != 0) return false;
  sum = ((lds[lane] + lds[64 + lane]) + lds[128 + lane]) + lds[192 + lane];
  return true;
}

template <int DIM>
__global__ __launch_bounds__(256) void k_cg_apply_dot(const double* __restrict__ coord, long long n_atoms,
                                                      const long long* __restrict__ pairs, long long k,
                                                      const double* __restrict__ gamma,
                                                      const long long* __restrict__ row_start,
                                                      const double* __restrict__ scale, const double* __restrict__ p,
                                                      double* __restrict__ qq, long long ld, long long q,
                                                      double* __restrict__ work) {
  __shared__ double lds[256];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long i = (long long)blockIdx.x * 4 + wave;
  const long long col = (long long)blockIdx.y * 64 + lane;
  const bool live = col < q;
  double dot = 0.0;   // (a wavefront beyond the last atom adds exactly 0)
  if (i < n_atoms) {
    const double ti = scale ? scale[i] : 1.0;
    const double* __restrict__ pc = p + (live ? col : (long long)blockIdx.y * 64);
    double xi[DIM], ui[DIM], s[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      xi[c] = pc[(DIM * i + c) * ld];
      ui[c] = ti * xi[c];
      s[c] = 0.0;
    }
    pair_walk<DIM>(coord, n_atoms, pairs, k, gamma, row_start, scale, pc, ld, i, lane, ui, s);
    double v[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) v[c] = 1.0 * (ti * s[c]) + 0.0 * xi[c];   // k_pairs_panel's store with alpha 1, beta 0
    if (live) {
#pragma unroll
      for (int c = 0; c < DIM; ++c) qq[(DIM * i + c) * ld + col] = v[c];
    }
    dot = xi[0] * v[0];
    if (DIM == 3) dot = (dot + xi[1] * v[1]) + xi[2] * v[2];
  }
  double sum;
  if (combine4(dot, wave, lane, lds, sum) && live) work[(long long)blockIdx.x * q + col] = sum;
}

// X = 0, P = R and the partials of <r, r>: the start of a solve
template <int DIM>
__global__ __launch_bounds__(256) void k_cg_start(long long n_atoms, double* __restrict__ x, const double* __restrict__ r,
                                                  double* __restrict__ p, long long ld, long long q,
                                                  double* __restrict__ work) {
  __shared__ double lds[256];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long i = (long long)blockIdx.x * 4 + wave;
  const long long col = (long long)blockIdx.y * 64 + lane;
  const bool live = col < q;
  double rr = 0.0;
  if (i < n_atoms && live) {
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      const long long at = (DIM * i + c) * ld + col;
      const double rv = r[at];
      x[at] = 0.0;
      p[at] = rv;
      rr = c == 0 ? rv * rv : rr + rv * rv;
    }
  }
  double sum;
  if (combine4(rr, wave, lane, lds, sum) && live) work[(long long)blockIdx.x * q + col] = sum;
}

template <int DIM>
__global__ __launch_bounds__(256) void k_cg_update(long long n_atoms, double* __restrict__ x, double* __restrict__ r,
                                                   const double* __restrict__ p, const double* __restrict__ qq,
                                                   long long ld, long long q, const double* __restrict__ state,
                                                   double* __restrict__ work) {
  __shared__ double lds[256];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long i = (long long)blockIdx.x * 4 + wave;
  const long long col = (long long)blockIdx.y * 64 + lane;
  const bool live = col < q;
  double rr = 0.0;   // (a stopped column's partials are 0 and never read)
  if (i < n_atoms && live && ((const long long*)state)[CG_STATUS * ld + col] == 0) {
    const double alpha = state[CG_ALPHA * ld + col];
    double xv[DIM], rv[DIM], pv[DIM], qv[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      const long long at = (DIM * i + c) * ld + col;
      xv[c] = x[at];
      rv[c] = r[at];
      pv[c] = p[at];
      qv[c] = qq[at];
    }
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      const long long at = (DIM * i + c) * ld + col;
      const double rn = rv[c] - alpha * qv[c];
      x[at] = xv[c] + alpha * pv[c];
      r[at] = rn;
      rr = c == 0 ? rn * rn : rr + rn * rn;
    }
  }
  double sum;
  if (combine4(rr, wave, lane, lds, sum) && live) work[(long long)blockIdx.x * q + col] = sum;
}

__global__ __launch_bounds__(256) void k_cg_direction(long long m, const double* __restrict__ r, double* __restrict__ p,
                                                      long long ld, long long q, const double* __restrict__ state) {
  const int lane = threadIdx.x & 63;
  const long long col = (long long)blockIdx.y * 64 + lane;
  if (col >= q || ((const long long*)state)[CG_STATUS * ld + col] != 0) return;
  const double beta = state[CG_BETA * ld + col];
  // a wavefront takes four consecutive rows: four independent loads of r and of p per lane
  const long long row0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
  double rv[4], pv[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (row0 + c < m) {
      rv[c] = r[(row0 + c) * ld + col];
      pv[c] = p[(row0 + c) * ld + col];
    }
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (row0 + c < m) p[(row0 + c) * ld + col] = rv[c] + beta * pv[c];
}

// One workgroup of sixteen wavefronts per 64 columns, lane = column.
template <int MODE>
__global__ __launch_bounds__(64 * RED_WAVES) void k_cg_reduce(const double* __restrict__ work, long long n_blocks,
                                                              long long ld, long long q, double tol,
                                                              double* __restrict__ state) {
  __shared__ double lds[64 * RED_WAVES];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long col = (long long)blockIdx.x * 64 + lane;
  const bool live = col < q;
  double acc = 0.0;
  if (live) {
    const double* __restrict__ w = work + col;
#pragma unroll 8
    for (long long b = wave; b < n_blocks; b += RED_WAVES) acc += w[b * q];
  }
  lds[wave * 64 + lane] = acc;
  __syncthreads();
  if (wave != 0 || !live) return;
  double sum = lds[lane];
#pragma unroll
  for (int w = 1; w < RED_WAVES; ++w) sum += lds[w * 64 + lane];

  long long* __restrict__ status = (long long*)state + CG_STATUS * ld + col;
  long long* __restrict__ iters = (long long*)state + CG_ITERS * ld + col;
  double* __restrict__ rho = state + CG_RHO * ld + col;
  if (MODE == RED_INIT) {
    *rho = sum;
    state[CG_STOP * ld + col] = (tol * tol) * sum;
    state[CG_ALPHA * ld + col] = 0.0;
    state[CG_BETA * ld + col] = 0.0;
    state[CG_PQ * ld + col] = 0.0;
    *status = sum == 0.0 ? 1 : (sum > 0.0 && sum <= 1.7976931348623157e308 ? 0 : 2);   // (a non-finite |f|: broken down)
    *iters = 0;
  } else if (MODE == RED_PQ) {
    double alpha = 0.0;
    if (*status == 0) {
      state[CG_PQ * ld + col] = sum;
      if (sum > 0.0 && sum <= 1.7976931348623157e308) alpha = *rho / sum;
      else *status = 2;
    }
    state[CG_ALPHA * ld + col] = alpha;
  } else {
    if (*status != 0) return;
    state[CG_BETA * ld + col] = sum / *rho;
    *rho = sum;
    *iters += 1;
    if (sum <= state[CG_STOP * ld + col]) *status = 1;
  }
}

template <int MODE>
void reduce(sc_ctx* ctx, const double* work, int64_t n_blocks, int64_t ld, int64_t q, double tol, double* state) {
  hipLaunchKernelGGL(k_cg_reduce<MODE>, dim3((unsigned)((q + 63) / 64)), dim3(64 * RED_WAVES), 0, ctx->stream, work,
                     (long long)n_blocks, (long long)ld, (long long)q, tol, state);
}

}  // namespace

size_t pairs_cg_workspace_bytes(int64_t n_atoms, int64_t q) { return (size_t)((n_atoms + 3) / 4) * (size_t)q * sizeof(double); }

int launch_pairs_cg_init(sc_ctx* ctx, int64_t n_atoms, int dim, double* d_x, const double* d_r, double* d_p, int64_t ld,
                         int64_t q, double tol, double* d_state, double* d_work) {
  if (q == 0) return SC_OK;
  const int64_t nb = (n_atoms + 3) / 4;
  const dim3 grid((unsigned)nb, (unsigned)((q + 63) / 64));
  if (dim == 3)
    hipLaunchKernelGGL(k_cg_start<3>, grid, dim3(256), 0, ctx->stream, (long long)n_atoms, d_x, d_r, d_p, (long long)ld,
                       (long long)q, d_work);
  else
    hipLaunchKernelGGL(k_cg_start<1>, grid, dim3(256), 0, ctx->stream, (long long)n_atoms, d_x, d_r, d_p, (long long)ld,
                       (long long)q, d_work);
  reduce<RED_INIT>(ctx, d_work, nb, ld, q, tol, d_state);
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

int launch_pairs_cg_step(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs, int64_t k,
                         const double* d_gamma, const int64_t* d_row_start, const double* d_atom_scale, double* d_x,
                         double* d_r, double* d_p, double* d_q, int64_t ld, int64_t q, double* d_state, double* d_work,
                         int64_t iterations) {
  if (q == 0) return SC_OK;
  const int64_t nb = (n_atoms + 3) / 4, m = dim * n_atoms;
  const dim3 grid((unsigned)nb, (unsigned)((q + 63) / 64));
  const dim3 rows((unsigned)((m + 15) / 16), (unsigned)((q + 63) / 64));
  for (int64_t it = 0; it < iterations; ++it) {
    if (dim == 3) {
      hipLaunchKernelGGL(k_cg_apply_dot<3>, grid, dim3(256), 0, ctx->stream, d_coord, (long long)n_atoms,
                         (const long long*)d_pairs, (long long)k, d_gamma, (const long long*)d_row_start, d_atom_scale,
                         d_p, d_q, (long long)ld, (long long)q, d_work);
      reduce<RED_PQ>(ctx, d_work, nb, ld, q, 0.0, d_state);
      hipLaunchKernelGGL(k_cg_update<3>, grid, dim3(256), 0, ctx->stream, (long long)n_atoms, d_x, d_r, d_p, d_q,
                         (long long)ld, (long long)q, d_state, d_work);
    } else {
      hipLaunchKernelGGL(k_cg_apply_dot<1>, grid, dim3(256), 0, ctx->stream, d_coord, (long long)n_atoms,
                         (const long long*)d_pairs, (long long)k, d_gamma, (const long long*)d_row_start, d_atom_scale,
                         d_p, d_q, (long long)ld, (long long)q, d_work);
      reduce<RED_PQ>(ctx, d_work, nb, ld, q, 0.0, d_state);
      hipLaunchKernelGGL(k_cg_update<1>, grid, dim3(256), 0, ctx->stream, (long long)n_atoms, d_x, d_r, d_p, d_q,
                         (long long)ld, (long long)q, d_state, d_work);
    }
    reduce<RED_RR>(ctx, d_work, nb, ld, q, 0.0, d_state);
    hipLaunchKernelGGL(k_cg_direction, rows, dim3(256), 0, ctx->stream, (long long)m, d_r, d_p, (long long)ld,
                       (long long)q, d_state);
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}
