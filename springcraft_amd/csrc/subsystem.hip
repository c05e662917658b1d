// Vibrational subsystem analysis (Hinsen 2000; Zheng & Brooks 2005; Ming & Wall 2005): the atoms are split into a system (s)
// and an environment (e), and the modes of the system with the environment relaxed adiabatically are the eigenpairs of
//     H_eff = H_ss - H_se H_ee^-1 H_es,
// the Schur complement of H_ee; the environment follows as x_e = -H_ee^-1 H_es x_s.  No reference counterpart (ProDy:
// reduceModel; Bio3D: nma's subsystem option).
//
// There is one path.  It takes B members with one system size and environments of different size, inputs packed back to back,
// in slots of one order: env_order atoms per environment slot, me = dim env_order.  A single structure is a batch of one with
// env_order = n_e: no pad atoms, and the leading dimensions are the blocks' own.
//
// Assembly.  The three blocks come straight from the ordered pair list; the (dim N, dim N) matrix is never formed.  The member
// is blockIdx.y.  One thread per directed pair (i, j) writes the off-diagonal block -gamma d d^T / |d|^2 (dim 3) or -gamma
// (dim 1) once: into H_ss, H_ee or, for i in the environment and j in the system, H_es; the mirror pair (j, i) of that one
// writes nothing.  One thread per atom sums its diagonal block over its run of the list in list order.  With symmetric
// constants both directions of a pair compute the same bits, so H_ss and H_ee equal their transposes bit for bit; there are
// no atomics and two calls agree bit for bit.  inv_sqrt_mass of the SYSTEM atoms scales the rows and columns of H_ss and the
// columns of H_es; the environment carries no mass (the adiabatic approximation).  The launcher zeroes all three buffers
// first.  A member with fewer than env_order environment atoms gets the slot diag(H_ee(b), I) and zero pad rows of H_es: the
// atom kernel also owns the pad diagonal, thread n_atoms + t of a member writes the 1.0 of pad atom n_e + t.
//
// Reduction.  potrf(H_ee) = L L^T; Y^T = H_se L^-T by block substitution on the (ms, me) column-major view of H_es' buffer;
// H_eff = H_ss - Y^T Y on the lower_grid SYRK form of launch_gemm_f64, then mirrored: one batched factorisation, one batched
// substitution, one grouped product and one mirror for all members.  L and Y stay in their buffers for the follow motion
// x_e = -L^-T (Y x_s), per slot: one product and one backward substitution.  The factor of a padded slot is diag(L_b, I), Y's
// pad rows are 0 and H_eff gains exact zeros.
//
// A member's bits depend on the member and on the slot order alone, not on the batch or its place in it: its pairs and atoms
// are summed by the same expressions in the same order wherever it stands, and the GEMM tile of the products is pinned to
// the shape of one member.
#include "gemm_f64.h"
#include "potrf_internal.h"

namespace {

using sc_host::SubMember;

template <int DIM>
__global__ __launch_bounds__(256) void k_sub_offdiag(const SubMember* __restrict__ members, const double* __restrict__ coord_all,
                                                     const long long* __restrict__ pairs_all,
                                                     const double* __restrict__ gamma_all, const int* __restrict__ group_all,
                                                     const int* __restrict__ pos_all, long long n_s, long long env_order,
                                                     const double* __restrict__ ism_all, double* __restrict__ hss_all,
                                                     double* __restrict__ hes_all, double* __restrict__ hee_all) {
  const long long b = blockIdx.y;
  const SubMember M = members[b];
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n_atoms = M.n_atoms, k = M.n_pairs, n_e = M.n_e;
  if (p >= k || n_e < 0 || n_e > env_order) return;
  const long long ms = DIM * n_s, me = DIM * env_order;
  const double* coord = coord_all + 3 * M.atom0;
  const long long* pairs = pairs_all + 2 * M.pair0;
  const double* gamma = gamma_all + M.pair0;
  const int* group = group_all + M.atom0;
  const int* pos = pos_all + M.atom0;
  const double* ism = ism_all ? ism_all + b * n_s : nullptr;
  const long long i = pairs[2 * p], j = pairs[2 * p + 1];
  if (i < 0 || i >= n_atoms || j < 0 || j >= n_atoms || i == j) return;
  const int gi = group[i], gj = group[j];
  if (gi == 0 && gj == 1) return;   // (the block of H_se: its mirror pair writes H_es)
  const long long pi = pos[i], pj = pos[j];
  const long long ni = gi == 0 ? n_s : n_e, nj = gj == 0 ? n_s : n_e;
  if (gi < 0 || gi > 1 || gj < 0 || gj > 1 || pi < 0 || pi >= ni || pj < 0 || pj >= nj) return;
  const double si = (gi == 0 && ism) ? ism[pi] : 1.0, sj = (gj == 0 && ism) ? ism[pj] : 1.0;
  double* dst = gi == 0 ? hss_all + b * ms * ms : (gj == 0 ? hes_all + b * me * ms : hee_all + b * me * me);
  const long long ldd = gj == 0 ? ms : me;
  dst += DIM * pi * ldd + DIM * pj;
  if (DIM == 1) {
    dst[0] = -gamma[p] * (si * sj);
    return;
  }
  const double d[3] = {coord[3 * j + 0] - coord[3 * i + 0], coord[3 * j + 1] - coord[3 * i + 1],
                       coord[3 * j + 2] - coord[3 * i + 2]};
  const double g = -(gamma[p] / ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])) * (si * sj);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[a * ldd + c] = g * (d[a] * d[c]);
}

template <int DIM>
__global__ __launch_bounds__(256) void k_sub_diag(const SubMember* __restrict__ members, const double* __restrict__ coord_all,
                                                  const long long* __restrict__ pairs_all, const double* __restrict__ gamma_all,
                                                  const long long* __restrict__ row_start_all,
                                                  const int* __restrict__ group_all, const int* __restrict__ pos_all,
                                                  long long n_s, long long env_order, const double* __restrict__ ism_all,
                                                  double* __restrict__ hss_all, double* __restrict__ hee_all) {
  const long long b = blockIdx.y;
  const SubMember M = members[b];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n_atoms = M.n_atoms, k = M.n_pairs, n_e = M.n_e;
  if (n_e < 0 || n_e > env_order) return;
  const long long ms = DIM * n_s, me = DIM * env_order;
  double* hee = hee_all + b * me * me;
  if (i >= n_atoms) {   // a pad atom of the slot: the identity on the pad diagonal
    const long long t = n_e + (i - n_atoms);
    if (t >= env_order) return;
#pragma unroll
    for (int a = 0; a < DIM; ++a) hee[(DIM * t + a) * me + DIM * t + a] = 1.0;
    return;
  }
  const double* coord = coord_all + 3 * M.atom0;
  const long long* pairs = pairs_all + 2 * M.pair0;
  const double* gamma = gamma_all + M.pair0;
  const long long* row_start = row_start_all + M.atom0 + b;
  const int* group = group_all + M.atom0;
  const int* pos = pos_all + M.atom0;
  const double* ism = ism_all ? ism_all + b * n_s : nullptr;
  const int gi = group[i];
  const long long pi = pos[i], ni = gi == 0 ? n_s : n_e;
  if (gi < 0 || gi > 1 || pi < 0 || pi >= ni) return;
  long long lo = row_start[i], hi = row_start[i + 1];
  if (lo < 0) lo = 0;
  if (hi > k) hi = k;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // xx xy xz yy yz zz (dim 1: acc[0])
  for (long long p = lo; p < hi; ++p) {
    const long long j = pairs[2 * p + 1];
    if (pairs[2 * p] != i || j < 0 || j >= n_atoms || j == i) continue;
    if (DIM == 1) {
      acc[0] += gamma[p];
      continue;
    }
    const double dx = coord[3 * j + 0] - coord[3 * i + 0], dy = coord[3 * j + 1] - coord[3 * i + 1],
                 dz = coord[3 * j + 2] - coord[3 * i + 2];
    const double g = gamma[p] / ((dx * dx + dy * dy) + dz * dz);
    acc[0] += g * (dx * dx); acc[1] += g * (dx * dy); acc[2] += g * (dx * dz);
    acc[3] += g * (dy * dy); acc[4] += g * (dy * dz); acc[5] += g * (dz * dz);
  }
  const double s = (gi == 0 && ism) ? ism[pi] * ism[pi] : 1.0;
  const long long ldd = gi == 0 ? ms : me;
  double* dst = (gi == 0 ? hss_all + b * ms * ms : hee) + DIM * pi * ldd + DIM * pi;
  if (DIM == 1) {
    dst[0] = acc[0] * s;
    return;
  }
  dst[0] = acc[0] * s; dst[1] = acc[1] * s; dst[2] = acc[2] * s;
  dst[ldd] = acc[1] * s; dst[ldd + 1] = acc[3] * s; dst[ldd + 2] = acc[4] * s;
  dst[2 * ldd] = acc[2] * s; dst[2 * ldd + 1] = acc[4] * s; dst[2 * ldd + 2] = acc[5] * s;
}

// matrix blockIdx.y, column-major (n, n): the strict upper triangle <- the strict lower one
__global__ __launch_bounds__(256) void k_sub_mirror(double* __restrict__ mats, long long n) {
  double* mat = mats + (long long)blockIdx.y * n * n;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long row = i % n, col = i / n;
  if (col >= n || row <= col) return;
  mat[row * n + col] = mat[col * n + row];
}

}  // namespace

int launch_subsystem_assembly(sc_ctx* ctx, const sc_host::BatchBlocksBufs& B, const sc_host::SubMember* h_members,
                              int64_t batch, int64_t max_pairs, const double* d_coord, int dim, const int64_t* d_pairs,
                              const double* d_gamma, const int64_t* d_row_start, const int32_t* d_group,
                              const int32_t* d_pos, int64_t n_s, int64_t env_order, const double* d_ism, double* d_hss,
                              double* d_hes, double* d_hee) {
  hipStream_t st = ctx->stream;
  const size_t ms = (size_t)dim * (size_t)n_s, me = (size_t)dim * (size_t)env_order, nb = (size_t)batch;
  const SubMember* d_members = reinterpret_cast<const SubMember*>(B.members);
  SC_TRY(sc_stage_upload(ctx, B.members, h_members, nb * sizeof(SubMember)));
  SC_HIP(ctx, hipMemsetAsync(d_hss, 0, sizeof(double) * nb * ms * ms, st));
  if (me > 0) {
    SC_HIP(ctx, hipMemsetAsync(d_hes, 0, sizeof(double) * nb * me * ms, st));
    SC_HIP(ctx, hipMemsetAsync(d_hee, 0, sizeof(double) * nb * me * me, st));
  }
  const int64_t atom_threads = sc_host::sub_batch_atom_threads(n_s, env_order);
  const dim3 gp((unsigned)((max_pairs + 255) / 256), (unsigned)batch), ga((unsigned)((atom_threads + 255) / 256), (unsigned)batch);
  if (dim == 3) {
    if (max_pairs > 0)
      hipLaunchKernelGGL(k_sub_offdiag<3>, gp, dim3(256), 0, st, d_members, d_coord, (const long long*)d_pairs, d_gamma,
                         d_group, d_pos, (long long)n_s, (long long)env_order, d_ism, d_hss, d_hes, d_hee);
    hipLaunchKernelGGL(k_sub_diag<3>, ga, dim3(256), 0, st, d_members, d_coord, (const long long*)d_pairs, d_gamma,
                       (const long long*)d_row_start, d_group, d_pos, (long long)n_s, (long long)env_order, d_ism, d_hss, d_hee);
  } else {
    if (max_pairs > 0)
      hipLaunchKernelGGL(k_sub_offdiag<1>, gp, dim3(256), 0, st, d_members, d_coord, (const long long*)d_pairs, d_gamma,
                         d_group, d_pos, (long long)n_s, (long long)env_order, d_ism, d_hss, d_hes, d_hee);
    hipLaunchKernelGGL(k_sub_diag<1>, ga, dim3(256), 0, st, d_members, d_coord, (const long long*)d_pairs, d_gamma,
                       (const long long*)d_row_start, d_group, d_pos, (long long)n_s, (long long)env_order, d_ism, d_hss, d_hee);
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

int launch_subsystem_reduction(sc_ctx* ctx, const sc_host::BatchReduceBufs& B, double* d_hss, double* d_hes, double* d_hee,
                               int64_t ms, int64_t me, int64_t batch, int outer, long long* d_info) {
  hipStream_t st = ctx->stream;
  PhaseTimer t_f(ctx, "subsystem_potrf", st), t_s(ctx, "subsystem_trsm", st), t_p(ctx, "subsystem_syrk", st);
  t_f.start();
  SC_TRY(launch_potrf(ctx, B.potrf, d_hee, me, me, me * me, batch, outer, d_info));
  t_f.stop();
  // slot b of the (me, ms) row-major buffer is H_se (ms, me) column-major: Y^T = H_se L^-T in place
  t_s.start();
  SC_TRY(launch_trsm(ctx, B.trsm, 0, kTrsmRight, d_hee, me, me, me * me, batch, d_hes, ms, ms, me * ms));
  t_s.stop();
  t_p.start();
  std::vector<GemmDesc> h((size_t)batch);   // H_eff(i, j) = H_ss(i, j) - sum_k Yt(i, k) Yt(j, k), i >= j, per member
  for (int64_t b = 0; b < batch; ++b) {
    GemmDesc G{};
    G.a = G.b = d_hes + b * me * ms;
    G.sa_i = 1; G.sa_k = ms;
    G.sb_j = 1; G.sb_k = ms;
    G.c = d_hss + b * ms * ms; G.ldc = ms;
    G.m = G.n = (int)ms; G.k = (int)me;
    G.alpha = -1.0; G.beta = 1.0;
    G.lower_only = 1;
    h[(size_t)b] = G;
  }
  GemmDesc* d_desc = reinterpret_cast<GemmDesc*>(B.descs);
  SC_TRY(sc_stage_upload(ctx, d_desc, h.data(), h.size() * sizeof(GemmDesc)));
  // the block tile of ONE member's product, whatever the batch: a member's bits do not depend on the batch
  SC_TRY(launch_gemm_f64(ctx, d_desc, {.count = (int)batch, .max_m = (int)ms, .max_n = (int)ms, .layout = kGemmAmBn,
                                      .lower_grid = true, .pin_tile = gemm_f64_tile(ctx, 1, (int)ms, (int)ms, kGemmAmBn)}));
  hipLaunchKernelGGL(k_sub_mirror, dim3((unsigned)(((long long)ms * ms + 255) / 256), (unsigned)batch), dim3(256), 0, st, d_hss,
                     (long long)ms);
  t_p.stop();
  SC_HIP(ctx, hipGetLastError());
  t_f.finish(); t_s.finish(); t_p.finish();
  return SC_OK;
}

int launch_subsystem_follow(sc_ctx* ctx, const sc_host::FollowBufs& B, const double* d_l, const double* d_y, int64_t ms,
                            int64_t me, const double* d_xs, int64_t q, double* d_xe) {
  GemmDesc G{};   // xe(e, j) = -sum_s Yt(s, e) xs(s, j)
  G.a = d_y; G.sa_i = ms; G.sa_k = 1;
  G.b = d_xs; G.sb_k = 1; G.sb_j = ms;
  G.c = d_xe; G.ldc = me;
  G.m = (int)me; G.n = (int)q; G.k = (int)ms;
  G.alpha = -1.0; G.beta = 0.0;
  GemmDesc* d_desc = reinterpret_cast<GemmDesc*>(B.desc);
  SC_TRY(sc_stage_upload(ctx, d_desc, &G, sizeof(G)));
  SC_TRY(launch_gemm_f64(ctx, d_desc, {.count = 1, .max_m = (int)me, .max_n = (int)q, .layout = kGemmAkBk}));
  return launch_trsm(ctx, B.trsm, 0, kTrsmBackward, d_l, me, me, 0, 1, d_xe, q, me, 0);
}
