// Least-squares superposition of M frames of N atoms on one target frame, and the mean frame of an ensemble.  No reference
// counterpart (its callers superimpose with biotite).
//
// Superposition.  With weights w_a >= 0 (1 if null), W = sum w, the weighted centroids c of the frame x and c_t of the target
// t, and S = sum_a w_a (x_a - c)(t_a - c_t)^T, the optimal PROPER rotation is Horn's (1987): the unit quaternion q that
// maximises q^T N q for the symmetric 4 x 4 matrix N built from S, i.e. the eigenvector of N's largest eigenvalue, found by
// cyclic Jacobi in float64.  A quaternion always gives det R = +1: a mirror image gets the best rotation, never a
// reflection.  A degenerate frame (N = 1, 2, collinear, planar) makes the largest eigenvalue multiple; every eigenvector
// of it is a minimiser and Jacobi returns one of them, orthonormal to rounding.  The fitted frame is R (x - c) + c_t; the
// RMSD is sqrt(sum w |R (x - c) + c_t - t|^2 / W), summed from the residuals themselves.
//
// One workgroup per frame.  k_superpose<true> keeps the frame in LDS: one coalesced read, three passes over LDS (centroid,
// S, fit), one coalesced write.  k_superpose<false> streams a frame of any size: the same three passes read global memory.
// Every sum is a per-thread sum over the atoms tid, tid + T, ... in ascending order followed by block_sum: a frame's bits
// depend on that frame, the target and the weights alone.  A non-finite coordinate makes the centroid non-finite and with
// it every output of that frame NaN; no other frame reads it.
//
// Mean frame.  mean[c] = sum_f p_f x_f[c] / P over the frames (p = 1 if null) and msd[a] = sum_f p_f |x_f[a] - mean[a]|^2 /
// P, each as a two-level sum: chunks of kMeanChunk frames per coordinate, then the chunks, both ascending.
#include "block_sum.h"
#include "common.h"
#include "ensemble_policy.h"

namespace {

constexpr int kJacobiSweeps = 30;

// R (row-major 3 x 3) from S (row-major, S[3 i + j] = sum w x_i t_j of the centred coordinates): R x ~ t
__device__ void horn_rotation(const double* S, double* R) {
  const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
  double A[4][4], V[4][4];
  A[0][0] = (Sxx + Syy) + Szz;
  A[1][1] = (Sxx - Syy) - Szz;
  A[2][2] = (Syy - Sxx) - Szz;
  A[3][3] = (Szz - Sxx) - Syy;
  A[0][1] = A[1][0] = Syz - Szy;
  A[0][2] = A[2][0] = Szx - Sxz;
  A[0][3] = A[3][0] = Sxy - Syx;
  A[1][2] = A[2][1] = Sxy + Syx;
  A[1][3] = A[3][1] = Szx + Sxz;
  A[2][3] = A[3][2] = Syz + Szy;
  double scale2 = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      V[i][j] = i == j ? 1.0 : 0.0;
      scale2 += A[i][j] * A[i][j];
    }
  // an off-diagonal entry below eps / 256 of the matrix norm is set to zero instead of rotated away
  const double thr = sqrt(scale2) * 0x1p-60;
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (fabs(apq) <= thr) {
          A[p][q] = A[q][p] = 0.0;
          continue;
        }
        rotated = true;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k != p && k != q) {
            const double akp = A[k][p], akq = A[k][q];
            A[k][p] = A[p][k] = c * akp - s * akq;
            A[k][q] = A[q][k] = s * akp + c * akq;
          }
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
        A[p][p] -= t * apq;
        A[q][q] += t * apq;
        A[p][q] = A[q][p] = 0.0;
      }
    if (!rotated) break;
  }
  // the column of the largest eigenvalue, the first one among equals
  double best = A[0][0], q0 = V[0][0], q1 = V[1][0], q2 = V[2][0], q3 = V[3][0];
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (A[j][j] > best) {
      best = A[j][j];
      q0 = V[0][j]; q1 = V[1][j]; q2 = V[2][j]; q3 = V[3][j];
    }
  const double inv = 1.0 / sqrt((q0 * q0 + q1 * q1) + (q2 * q2 + q3 * q3));
  q0 *= inv; q1 *= inv; q2 *= inv; q3 *= inv;
  const double aa = q0 * q0, bb = q1 * q1, cc = q2 * q2, dd = q3 * q3;
  R[0] = (aa + bb) - (cc + dd);
  R[1] = 2.0 * (q1 * q2 - q0 * q3);
  R[2] = 2.0 * (q1 * q3 + q0 * q2);
  R[3] = 2.0 * (q1 * q2 + q0 * q3);
  R[4] = (aa + cc) - (bb + dd);
  R[5] = 2.0 * (q2 * q3 - q0 * q1);
  R[6] = 2.0 * (q1 * q3 - q0 * q2);
  R[7] = 2.0 * (q2 * q3 + q0 * q1);
  R[8] = (aa + dd) - (bb + cc);
  // a non-finite S leaves the whole rotation NaN, whatever Jacobi made of it
  bool finite = true;
#pragma unroll
  for (int e = 0; e < 9; ++e) finite = finite && fabs(S[e]) <= 1.7976931348623157e308;
  if (!finite)
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = __builtin_nan("");
}

// tc[0..2] = weighted centroid of the target, tc[3] = W; one workgroup
__global__ __launch_bounds__(1024) void k_target_centre(const double* __restrict__ target, long long n,
                                                        const double* __restrict__ weights, double* __restrict__ tc) {
  __shared__ double red[16 * 4];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long a = threadIdx.x; a < n; a += blockDim.x) {
    const double w = weights ? weights[a] : 1.0;
    s[0] += w * target[3 * a + 0];
    s[1] += w * target[3 * a + 1];
    s[2] += w * target[3 * a + 2];
    s[3] += w;
  }
  block_sum<4>(s, red);
  if (threadIdx.x == 0) {
    tc[0] = s[0] / s[3];
    tc[1] = s[1] / s[3];
    tc[2] = s[2] / s[3];
    tc[3] = s[3];
  }
}

template <bool LDS>
__global__ __launch_bounds__(LDS ? 256 : 1024) void k_superpose(const double* frames, long long n,
                                                                const double* __restrict__ target,
                                                                const double* __restrict__ weights,
                                                                const double* __restrict__ tc, double* out,
                                                                double* __restrict__ rot, double* __restrict__ trans,
                                                                double* __restrict__ rmsd) {
  extern __shared__ double xs[];          // LDS form: the frame
  __shared__ double red[16 * 9];
  __shared__ double rsh[16];              // R, then c
  const long long f = blockIdx.x;
  const double* x = frames + f * 3 * n;   // (out may be frames: not __restrict__, and read before written per atom)
  double* y = out + f * 3 * n;
  const int tid = threadIdx.x, nt = blockDim.x;
  const double* xr = LDS ? xs : x;
  if (LDS) {
    for (long long i = tid; i < 3 * n; i += nt) xs[i] = x[i];
    __syncthreads();
  }
  const double W = tc[3], t0 = tc[0], t1 = tc[1], t2 = tc[2];

  // ---- weighted centroid
  double s[3] = {0.0, 0.0, 0.0};
  for (long long a = tid; a < n; a += nt) {
    const double w = weights ? weights[a] : 1.0;
    s[0] += w * xr[3 * a + 0];
    s[1] += w * xr[3 * a + 1];
    s[2] += w * xr[3 * a + 2];
  }
  block_sum<3>(s, red);
  const double c0 = s[0] / W, c1 = s[1] / W, c2 = s[2] / W;

  // ---- cross-covariance with the centred target
  double m[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) m[e] = 0.0;
  for (long long a = tid; a < n; a += nt) {
    const double w = weights ? weights[a] : 1.0;
    const double d[3] = {w * (xr[3 * a + 0] - c0), w * (xr[3 * a + 1] - c1), w * (xr[3 * a + 2] - c2)};
    const double u[3] = {target[3 * a + 0] - t0, target[3 * a + 1] - t1, target[3 * a + 2] - t2};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) m[3 * i + j] += d[i] * u[j];
  }
  block_sum<9>(m, red);
  if (tid == 0) {
    double R[9];
    horn_rotation(m, R);
#pragma unroll
    for (int e = 0; e < 9; ++e) rsh[e] = R[e];
  }
  __syncthreads();
  double R[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) R[e] = rsh[e];

  // ---- the fitted frame and its residuals
  double e2[1] = {0.0};
  for (long long a = tid; a < n; a += nt) {
    const double w = weights ? weights[a] : 1.0;
    const double d0 = xr[3 * a + 0] - c0, d1 = xr[3 * a + 1] - c1, d2 = xr[3 * a + 2] - c2;
    const double f0 = ((R[0] * d0 + R[1] * d1) + R[2] * d2) + t0;
    const double f1 = ((R[3] * d0 + R[4] * d1) + R[5] * d2) + t1;
    const double f2 = ((R[6] * d0 + R[7] * d1) + R[8] * d2) + t2;
    const double r0 = f0 - target[3 * a + 0], r1 = f1 - target[3 * a + 1], r2 = f2 - target[3 * a + 2];
    e2[0] += w * ((r0 * r0 + r1 * r1) + r2 * r2);
    if (LDS) {
      xs[3 * a + 0] = f0; xs[3 * a + 1] = f1; xs[3 * a + 2] = f2;
    } else {
      y[3 * a + 0] = f0; y[3 * a + 1] = f1; y[3 * a + 2] = f2;
    }
  }
  block_sum<1>(e2, red);   // (its barriers also order the LDS frame's writes before the copy below)
  if (LDS)
    for (long long i = tid; i < 3 * n; i += nt) y[i] = xs[i];
  if (tid == 0) {
    if (rmsd) rmsd[f] = sqrt(e2[0] / W);
    if (rot)
#pragma unroll
      for (int e = 0; e < 9; ++e) rot[9 * f + e] = R[e];
    if (trans) {   // fitted = R x + trans
      trans[3 * f + 0] = t0 - ((R[0] * c0 + R[1] * c1) + R[2] * c2);
      trans[3 * f + 1] = t1 - ((R[3] * c0 + R[4] * c1) + R[5] * c2);
      trans[3 * f + 2] = t2 - ((R[6] * c0 + R[7] * c1) + R[8] * c2);
    }
  }
}

// partial[ch, col] = sum over the frames f of chunk ch, ascending, of p_f g(x_f[col]); g = identity (mean null) or the
// squared deviation from mean[col]
__global__ __launch_bounds__(256) void k_mean_partial(const double* __restrict__ frames, long long n_frames, long long n3,
                                                      const double* __restrict__ fw, const double* __restrict__ mean,
                                                      double* __restrict__ partial) {
  const long long col = (long long)blockIdx.x * 256 + threadIdx.x;
  if (col >= n3) return;
  const long long f0 = (long long)blockIdx.y * sc_host::kMeanChunk;
  const long long f1 = f0 + sc_host::kMeanChunk < n_frames ? f0 + sc_host::kMeanChunk : n_frames;
  const double mu = mean ? mean[col] : 0.0;
  double s = 0.0;
  for (long long f = f0; f < f1; ++f) {
    const double p = fw ? fw[f] : 1.0;
    const double v = frames[f * n3 + col];
    s += mean ? p * ((v - mu) * (v - mu)) : p * v;
  }
  partial[(long long)blockIdx.y * n3 + col] = s;
}

// the sum of the frame weights, the same bits in every thread that asks
__device__ __forceinline__ double weight_sum(const double* __restrict__ fw, long long n_frames) {
  if (!fw) return (double)n_frames;
  double s = 0.0;
  for (long long f = 0; f < n_frames; ++f) s += fw[f];
  return s;
}

// per_atom = false: out[col] = sum_ch partial[ch, col] / P; true: out[a] = sum_ch (the three columns of atom a) / P
__global__ __launch_bounds__(256) void k_mean_final(const double* __restrict__ partial, long long chunks, long long n3,
                                                    const double* __restrict__ fw, long long n_frames, bool per_atom,
                                                    double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (per_atom ? n3 / 3 : n3)) return;
  double s = 0.0;
  for (long long ch = 0; ch < chunks; ++ch) {
    const double* p = partial + ch * n3;
    s += per_atom ? (p[3 * i + 0] + p[3 * i + 1]) + p[3 * i + 2] : p[i];
  }
  out[i] = s / weight_sum(fw, n_frames);
}

}  // namespace

int launch_superpose(sc_ctx* ctx, int form, const double* d_frames, int64_t n_frames, int64_t n_atoms,
                     const double* d_target, const double* d_weights, double* d_tc, double* d_out, double* d_rot,
                     double* d_trans, double* d_rmsd) {
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_target_centre, dim3(1), dim3(1024), 0, st, d_target, (long long)n_atoms, d_weights, d_tc);
  if (form == sc_host::kSuperposeFormLds)
    hipLaunchKernelGGL(k_superpose<true>, dim3((unsigned)n_frames), dim3(256), sizeof(double) * 3 * (size_t)n_atoms, st,
                       d_frames, (long long)n_atoms, d_target, d_weights, d_tc, d_out, d_rot, d_trans, d_rmsd);
  else
    hipLaunchKernelGGL(k_superpose<false>, dim3((unsigned)n_frames), dim3(1024), 0, st, d_frames, (long long)n_atoms,
                       d_target, d_weights, d_tc, d_out, d_rot, d_trans, d_rmsd);
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

int launch_ensemble_mean(sc_ctx* ctx, const double* d_frames, int64_t n_frames, int64_t n_atoms, const double* d_fw,
                         double* d_partial, double* d_mean, double* d_msd) {
  hipStream_t st = ctx->stream;
  const long long n3 = 3 * (long long)n_atoms, chunks = sc_host::mean_chunks(n_frames);
  const dim3 grid((unsigned)((n3 + 255) / 256), (unsigned)chunks);
  hipLaunchKernelGGL(k_mean_partial, grid, dim3(256), 0, st, d_frames, (long long)n_frames, n3, d_fw,
                     (const double*)nullptr, d_partial);
  hipLaunchKernelGGL(k_mean_final, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, st, d_partial, chunks, n3, d_fw,
                     (long long)n_frames, false, d_mean);
  if (d_msd) {
    hipLaunchKernelGGL(k_mean_partial, grid, dim3(256), 0, st, d_frames, (long long)n_frames, n3, d_fw,
                       (const double*)d_mean, d_partial);
    hipLaunchKernelGGL(k_mean_final, dim3((unsigned)((n_atoms + 255) / 256)), dim3(256), 0, st, d_partial, chunks, n3, d_fw,
                       (long long)n_frames, true, d_msd);
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}
