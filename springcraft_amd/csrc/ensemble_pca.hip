// Principal components of a conformational ensemble (quasi-harmonic / essential-dynamics modes) from M fitted frames of N
// atoms.  No reference counterpart (Bio3D: pca.xyz; ProDy: PCA).
//
//   Xc[f, 3 a + c] = (x_f[a, c] - mean[a, c]) sqrt(mass_a)                     k_pca_centre, one workgroup per frame
//   total = sum Xc^2 / (M - 1)                                                  the frames' sums of squares, in order
//   M - 1 < 3 N:  G = Xc Xc^T / (M - 1), order M         else  C = Xc^T Xc / (M - 1), order 3 N      launch_gemm_f64
//   the n_modes largest eigenpairs (mu, u)                                      eigh_range_batched_async / eigh_batched_async
//   Gram route: raw_j = Xc^T u_j (one GEMM); covariance route: raw_j = u_j
//   v_j = raw_j / |raw_j|, rows by descending mu; var_j = mu_j, w_j = 1 / mu_j   k_pca_finish, one workgroup per row
//
// On the Gram route |Xc^T u_j| = sqrt((M - 1) mu_j) in exact arithmetic; the rows are divided by their computed norm instead,
// which is a unit vector to rounding also where mu_j carries the eigensolver's absolute error.  The product's K slices (a
// short result with a long K axis) are added in ascending order; the covariance route without slices computes the lower
// triangle only and mirrors it.  Every sum has a fixed order: two calls agree bit for bit.
#include "block_sum.h"
#include "ensemble_internal.h"
#include "gemm_f64.h"

namespace {

__global__ __launch_bounds__(256) void k_pca_centre(const double* __restrict__ frames, long long n3,
                                                    const double* __restrict__ mean, const double* __restrict__ sqrt_mass,
                                                    double* __restrict__ xc, double* __restrict__ frame_ss) {
  __shared__ double red[4];
  const long long f = blockIdx.x;
  double s[1] = {0.0};
  for (long long i = threadIdx.x; i < n3; i += 256) {
    const double v = (frames[f * n3 + i] - mean[i]) * (sqrt_mass ? sqrt_mass[i / 3] : 1.0);
    xc[f * n3 + i] = v;
    s[0] += v * v;
  }
  block_sum<1>(s, red);
  if (threadIdx.x == 0) frame_ss[f] = s[0];
}

// out[0] = scale * sum of x[0 .. n - 1]; one workgroup
__global__ __launch_bounds__(1024) void k_sum_ordered(const double* __restrict__ x, long long n, double scale,
                                                      double* __restrict__ out) {
  __shared__ double red[16];
  double s[1] = {0.0};
  for (long long i = threadIdx.x; i < n; i += 1024) s[0] += x[i];
  block_sum<1>(s, red);
  if (threadIdx.x == 0) out[0] = scale * s[0];
}

__global__ __launch_bounds__(256) void k_slice_sum(const double* __restrict__ slices, int split, long long elems,
                                                   double* __restrict__ mat) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= elems) return;
  double s = slices[i];
  for (int q = 1; q < split; ++q) s += slices[(long long)q * elems + i];
  mat[i] = s;
}

// column-major (n, n): the strict upper triangle <- the strict lower one
__global__ __launch_bounds__(256) void k_mirror_lower(double* __restrict__ mat, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long row = i % n, col = i / n;
  if (col >= n || row <= col) return;
  mat[row * n + col] = mat[col * n + row];
}

// output row j <- source row k - 1 - j over its norm; var[j] = mu of that row, w[j] = 1 / mu
__global__ __launch_bounds__(256) void k_pca_finish(const double* __restrict__ src, long long ld, long long n3, long long k,
                                                    const double* __restrict__ evals, double* __restrict__ v,
                                                    double* __restrict__ var, double* __restrict__ w) {
  __shared__ double red[4];
  const long long j = blockIdx.x, r = k - 1 - j;
  const double* row = src + r * ld;
  double s[1] = {0.0};
  for (long long i = threadIdx.x; i < n3; i += 256) s[0] += row[i] * row[i];
  block_sum<1>(s, red);
  const double inv = 1.0 / sqrt(s[0]);
  for (long long i = threadIdx.x; i < n3; i += 256) v[j * n3 + i] = row[i] * inv;
  if (threadIdx.x == 0) {
    var[j] = evals[r];
    w[j] = 1.0 / evals[r];
  }
}

}  // namespace

size_t ensemble_pca_desc_bytes() { return sizeof(GemmDesc); }

int launch_ensemble_pca(sc_ctx* ctx, const sc_host::PcaPlan& P, const sc_host::PcaBufs& B, const double* d_frames,
                        int64_t n_frames, int64_t n_atoms, const double* d_mean, const double* d_sqrt_mass, int64_t n_modes,
                        double* d_w, double* d_var, double* d_v, double* d_total) {
  hipStream_t st = ctx->stream;
  const long long M = n_frames, n3 = 3 * (long long)n_atoms, ord = P.order, k = n_modes;
  const double inv = 1.0 / (double)(M - 1);
  PhaseTimer t_prod(ctx, "pca_product", st), t_eig(ctx, "pca_eigh", st), t_exp(ctx, "pca_expand", st);

  t_prod.start();
  hipLaunchKernelGGL(k_pca_centre, dim3((unsigned)M), dim3(256), 0, st, d_frames, n3, d_mean, d_sqrt_mass, B.xc, B.frame_ss);
  hipLaunchKernelGGL(k_sum_ordered, dim3(1), dim3(1024), 0, st, B.frame_ss, M, inv, d_total);

  GemmDesc h[2] = {};
  GemmDesc& G = h[0];
  G.c = P.split_k > 1 ? B.slices : B.mat;
  G.m = G.n = (int)ord;
  G.k = (int)P.k_len;
  G.ldc = ord;
  G.alpha = inv;
  G.beta = 0.0;
  G.split_stride = ord * ord;
  G.a = G.b = B.xc;
  if (P.route == sc_host::kPcaGram) {   // G[i, j] = sum_c Xc[i, c] Xc[j, c]
    G.sa_i = n3; G.sa_k = 1;
    G.sb_k = 1; G.sb_j = n3;
  } else {                              // C[i, j] = sum_f Xc[f, i] Xc[f, j]
    G.sa_i = 1; G.sa_k = n3;
    G.sb_k = n3; G.sb_j = 1;
    G.lower_only = P.lower_grid ? 1 : 0;
  }
  GemmDesc& E = h[1];                   // raw (k, 3 N) row-major = column-major (3 N, k): raw[j, i] = sum_f Xc[f, i] U[j, f]
  E.a = B.xc; E.sa_i = 1; E.sa_k = n3;
  E.b = B.evecs; E.sb_k = 1; E.sb_j = ord;
  E.c = B.raw; E.ldc = n3;
  E.m = (int)n3; E.n = (int)k; E.k = (int)M;
  E.alpha = 1.0; E.beta = 0.0;
  GemmDesc* d_desc = reinterpret_cast<GemmDesc*>(B.descs);
  SC_TRY(sc_stage_upload(ctx, d_desc, h, sizeof(h)));
  SC_TRY(launch_gemm_f64(ctx, d_desc, {.count = 1, .max_m = (int)ord, .max_n = (int)ord,
                                      .layout = P.route == sc_host::kPcaGram ? kGemmAkBk : kGemmAmBn,
                                      .split_k = P.split_k, .lower_grid = P.lower_grid}));
  if (P.split_k > 1)
    hipLaunchKernelGGL(k_slice_sum, dim3((unsigned)((ord * ord + 255) / 256)), dim3(256), 0, st, B.slices, P.split_k,
                       ord * ord, B.mat);
  if (P.lower_grid)
    hipLaunchKernelGGL(k_mirror_lower, dim3((unsigned)((ord * ord + 255) / 256)), dim3(256), 0, st, B.mat, ord);
  t_prod.stop();
  SC_HIP(ctx, hipGetLastError());

  t_eig.start();
  if (P.full) SC_TRY(eigh_batched_async(ctx, B.mat, ord, 1, B.evals, B.evecs));
  else SC_TRY(eigh_range_batched_async(ctx, B.mat, ord, 1, ord - k, ord - 1, B.evals, B.evecs));
  t_eig.stop();

  t_exp.start();
  const bool gram = P.route == sc_host::kPcaGram;
  if (gram) SC_TRY(launch_gemm_f64(ctx, d_desc + 1, {.count = 1, .max_m = (int)n3, .max_n = (int)k, .layout = kGemmAmBk}));
  hipLaunchKernelGGL(k_pca_finish, dim3((unsigned)k), dim3(256), 0, st, gram ? B.raw : B.evecs, gram ? n3 : ord, n3, k,
                     B.evals, d_v, d_var, d_w);
  t_exp.stop();
  SC_HIP(ctx, hipGetLastError());
  SC_TRY(sc_stage_end(ctx));
  t_prod.finish(); t_eig.finish(); t_exp.finish();
  return SC_OK;
}
