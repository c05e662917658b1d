// Perturbation response scanning on device-resident eigenpairs.
//
// The reference evaluates it with NumPy on the (eig_values, eig_vectors) pair that nma.eigen returns, solving the
// eigenproblem again (nma.py:476-524).  Here the eigenpairs stay in HBM (struct sc_modes, api_modes.hip): two kernels and one
// MFMA GEMM, and only the (N, N) result crosses PCIe.
//
//   prs[a, b] = sum_{d, e} C[3a + d, 3b + e]^2,  C = pinv(H)                      (optionally / prs[a, a])
//
// V is stored as the solver leaves it: (n, n) row-major, row k = mode k.  The other consumers of one model (msf, dcc,
// anisotropic tensors, overlaps) are the batch kernels with a batch of one: batch_consumers.hip, mode_overlap.hip.
#include "common.h"
#include "gemm_f64.h"

namespace {

// in place: m[a, b] /= m[a, a] needs the original diagonal -> copy it first
__global__ void k_copy_diag(const double* __restrict__ c, int N, double* __restrict__ diag) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a < N) diag[a] = c[(size_t)a * N + a];
}

// ---- prs ------------------------------------------------------------------------------------------------------
// scale the eigenvector rows by 1/w for |w| > rcond * max|w|, else 0 (numpy.linalg.pinv(hermitian=True) rule)
__global__ __launch_bounds__(256) void k_pinv_rows(const double* __restrict__ v, const double* __restrict__ w, int n,
                                                   double rcond, double* __restrict__ vs) {
  __shared__ double red[256];
  double m = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) m = fmax(m, fabs(w[i]));
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  const int k = blockIdx.x;
  const double wk = w[k];
  const double sc = fabs(wk) > rcond * red[0] ? 1.0 / wk : 0.0;
  for (int j = threadIdx.x; j < n; j += 256) vs[(size_t)k * n + j] = v[(size_t)k * n + j] * sc;
}

// out[a, b] = sum of the squared entries of the 3x3 block (a, b) of the covariance; row-major (N, N)
__global__ __launch_bounds__(256) void k_prs_blocks(const double* __restrict__ cov, int N, double* __restrict__ out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  const int a = blockIdx.y;
  if (b >= N) return;
  const size_t n = (size_t)3 * N;
  double acc = 0.0;
  // same association as np.add.reduceat over rows, then over columns (nma.py:515-517)
  double colsum[3];
  for (int e = 0; e < 3; ++e) {
    double s = 0.0;
    for (int d = 0; d < 3; ++d) {
      const double x = cov[(size_t)(3 * a + d) * n + 3 * b + e];
      s += x * x;
    }
    colsum[e] = s;
  }
  acc = (colsum[0] + colsum[1]) + colsum[2];
  out[(size_t)a * N + b] = acc;
}

__global__ __launch_bounds__(256) void k_prs_norm(double* __restrict__ m, const double* __restrict__ diag, int N) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  const int a = blockIdx.y;
  if (b >= N) return;
  m[(size_t)a * N + b] = m[(size_t)a * N + b] / diag[a];
}

int run_gemm(sc_ctx* ctx, const GemmDesc& D, GemmDesc* d_desc) {
  SC_HIP(ctx, hipMemcpyAsync(d_desc, &D, sizeof(D), hipMemcpyHostToDevice, ctx->stream));
  // A(i, k) with unit row stride, B(k, j) with unit column stride
  return launch_gemm_f64(ctx, d_desc, {.count = 1, .max_m = D.m, .max_n = D.n, .layout = kGemmAmBn});
}

}  // namespace

// bytes of modes_prs_device's scratch
size_t prs_scratch_bytes(int64_t n) {
  const size_t N = (size_t)(n / 3);
  return 2 * align_up((size_t)n * n * 8, 256) + align_up(N * N * 8, 256) + align_up(N * 8, 256) + 1024;
}

// ANM only (n = 3N).  scratch (prs_scratch_bytes): VS (n^2) | COV (n^2) | diag (N) | desc
int modes_prs_device(sc_ctx* ctx, const double* d_v, const double* d_w, int64_t n64, double rcond, int norm,
                     char* scratch, double* d_out) {
  const int n = (int)n64, N = n / 3;
  hipStream_t st = ctx->stream;
  const size_t mat = align_up((size_t)n * n * 8, 256);
  double* d_vs = reinterpret_cast<double*>(scratch);
  double* d_cov = reinterpret_cast<double*>(scratch + mat);
  double* d_diag = reinterpret_cast<double*>(scratch + 2 * mat);
  GemmDesc* d_desc = reinterpret_cast<GemmDesc*>(scratch + 2 * mat + align_up((size_t)N * 8, 256));
  hipLaunchKernelGGL(k_pinv_rows, dim3(n), dim3(256), 0, st, d_v, d_w, n, rcond, d_vs);
  SC_HIP(ctx, hipGetLastError());
  // cov[i, j] = sum_k VS[k, i] V[k, j]
  GemmDesc D{};
  D.a = d_vs; D.sa_i = 1; D.sa_k = n;
  D.b = d_v; D.sb_k = n; D.sb_j = 1;
  D.c = d_cov; D.ldc = n; D.m = n; D.n = n; D.k = n;
  D.alpha = 1.0; D.beta = 0.0;
  SC_TRY(run_gemm(ctx, D, d_desc));
  hipLaunchKernelGGL(k_prs_blocks, dim3((N + 255) / 256, N), dim3(256), 0, st, d_cov, N, d_out);
  if (norm) {
    hipLaunchKernelGGL(k_copy_diag, dim3((N + 255) / 256), dim3(256), 0, st, d_out, N, d_diag);
    hipLaunchKernelGGL(k_prs_norm, dim3((N + 255) / 256, N), dim3(256), 0, st, d_out, d_diag, N);
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}
