// The Hessian / Kirchhoff matrix of an elastic network as an operator on the ordered pair list: products, per-atom
// deformation energies and per-spring strain without the (dim N, dim N) matrix.  No reference counterpart (Hinsen's
// deformation energy, Bio3D: deformation.nma; the strain is the derivative of an eigenvalue by ln gamma).
//
// Pair p = (i, j) of the directed list (sorted by i then j, both directions), gamma_p, d_p = x_j - x_i, n_p = d_p / |d_p|,
// t_a the atom scale (1 / sqrt(mass), null: 1).  For a row x (dim N), u[a] = t_a x[dim a .. dim a + dim - 1]:
//
//   dim 3:  e_p = n_p . (u[i] - u[j])            dim 1:  e_p = u[i] - u[j]
//   Y[i]  = t_i sum_{p = (i, .)} gamma_p e_p n_p  (dim 1: without n_p)      = ((T H T) x)[i]
//   E[i]  = 1/2 sum_{p = (i, .)} gamma_p e_p^2                              sum_i E[i] = x^T (T H T) x
//   S[p]  = gamma_p e_p^2                                                   sum_p S[p] = 2 x^T (T H T) x
//
// H is the matrix launch_hessian_from_pairs / launch_kirchhoff_from_pairs fill (block (i, j) = -gamma d d^T / |d|^2, the
// diagonal minus the sum of a row's blocks) for symmetric constants, gamma(i, j) = gamma(j, i); the caller checks that.
//
// k_pairs_apply: one wavefront owns an atom, its lanes the atom's pairs row_start[i] .. row_start[i + 1] - 1 in chunks
// of 64.  A lane keeps its pair's j, gamma, n_p and t_j in registers across the loop over the q rows (the geometry is
// computed once per call, not once per row); per row it forms its term, a fixed xor butterfly adds the 64 lanes, and
// lanes 0 .. dim write Y and E.  A later chunk adds to what the wavefront's same lane stored for the chunk before, so an
// atom's sum is ((chunk 0) + chunk 1) + ..., a sequence its own pair range fixes: no atomics, and a row's bits do not
// depend on q, on the row's position or on the other rows.  An atom without pairs stores exactly 0.0.  The file is
// compiled with -ffp-contract=off (build.py), so every operation below is the one written.
//
// k_pairs_strain: one thread per listed pair, geometry in registers, a stride loop over the rows.
#include "common.h"

namespace {

// the sum over the wavefront; every lane ends with the same bits (at each level the two partners add the same two numbers)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

template <int DIM>
__global__ __launch_bounds__(256) void k_pairs_apply(const double* __restrict__ coord, long long n_atoms,
                                                     const long long* __restrict__ pairs, long long k,
                                                     const double* __restrict__ gamma,
                                                     const long long* __restrict__ row_start,
                                                     const double* __restrict__ scale, const double* __restrict__ x,
                                                     long long q, double* __restrict__ y, double* __restrict__ energy) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_atoms) return;
  const long long m = DIM * n_atoms;
  long long lo = 0, hi = 0;
  if (k > 0) {
    lo = row_start[i];
    hi = row_start[i + 1];
    if (lo < 0) lo = 0;
    if (hi > k) hi = k;
  }
  if (lo >= hi) {   // no pairs: exact zeros
    for (long long r = lane; r < q; r += 64) {
      if (y) {
#pragma unroll
        for (int c = 0; c < DIM; ++c) y[r * m + DIM * i + c] = 0.0;
      }
      if (energy) energy[r * n_atoms + i] = 0.0;
    }
    return;
  }

  const double ti = scale ? scale[i] : 1.0;
  double xi[3] = {0.0, 0.0, 0.0};
  if (DIM == 3) {
    xi[0] = coord[3 * i + 0];
    xi[1] = coord[3 * i + 1];
    xi[2] = coord[3 * i + 2];
  }

  for (long long c0 = lo; c0 < hi; c0 += 64) {
    // this lane's pair of the chunk: j, gamma, n_p, t_j (skipped: no lane pair, or an entry outside 0 .. N - 1)
    const long long p = c0 + lane;
    bool valid = p < hi;
    long long j = 0;
    double g = 0.0, tj = 1.0, n[3] = {0.0, 0.0, 0.0};
    if (valid) {
      const long long pi = pairs[2 * p];
      j = pairs[2 * p + 1];
      valid = pi == i && j >= 0 && j < n_atoms;
      if (!valid) j = 0;
    }
    if (valid) {
      g = gamma[p];
      if (scale) tj = scale[j];
      if (DIM == 3) {
        const double dx = coord[3 * j + 0] - xi[0];
        const double dy = coord[3 * j + 1] - xi[1];
        const double dz = coord[3 * j + 2] - xi[2];
        const double len = sqrt((dx * dx + dy * dy) + dz * dz);
        n[0] = dx / len;   // (two atoms at one position: 0 / 0 = NaN, as the Hessian entry)
        n[1] = dy / len;
        n[2] = dz / len;
      }
    }
    const bool first = c0 == lo;

    for (long long r = 0; r < q; ++r) {
      const double* __restrict__ xr = x + r * m;
      double s[3] = {0.0, 0.0, 0.0}, se = 0.0;
      if (valid) {
        if (DIM == 3) {
          const double ex = ti * xr[3 * i + 0] - tj * xr[3 * j + 0];
          const double ey = ti * xr[3 * i + 1] - tj * xr[3 * j + 1];
          const double ez = ti * xr[3 * i + 2] - tj * xr[3 * j + 2];
          const double e = (n[0] * ex + n[1] * ey) + n[2] * ez;
          const double ge = g * e;
          s[0] = ge * n[0];
          s[1] = ge * n[1];
          s[2] = ge * n[2];
          se = ge * e;
        } else {
          const double e = ti * xr[i] - tj * xr[j];
          s[0] = g * e;
          se = s[0] * e;
        }
      }
      double mine = 0.0;
      if (y) {
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
          const double v = wave_sum(s[c]);
          if (lane == c) mine = ti * v;
        }
      }
      if (energy) {
        const double v = wave_sum(se);
        if (lane == DIM) mine = 0.5 * v;
      }
      double* dst = nullptr;
      if (lane < DIM) {
        if (y) dst = y + r * m + DIM * i + lane;
      } else if (lane == DIM) {
        if (energy) dst = energy + r * n_atoms + i;
      }
      if (dst) *dst = first ? mine : *dst + mine;
    }
  }
}

// grid (listed pairs / 256, row lanes): S[r, s] = gamma_p e_p^2 for p = pair_idx[s]
template <int DIM>
__global__ __launch_bounds__(256) void k_pairs_strain(const double* __restrict__ coord, long long n_atoms,
                                                      const long long* __restrict__ pairs, long long k,
                                                      const double* __restrict__ gamma, const double* __restrict__ scale,
                                                      const long long* __restrict__ pair_idx, long long ks,
                                                      const double* __restrict__ x, long long q,
                                                      double* __restrict__ out) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= ks) return;
  const long long m = DIM * n_atoms;
  const long long p = pair_idx[s];
  const bool listed = p >= 0 && p < k;   // (an index outside the list: NaN, and nothing of the list is read)
  long long i = 0, j = 0;
  bool valid = false;
  double g = 0.0, ti = 1.0, tj = 1.0, n[3] = {0.0, 0.0, 0.0};
  if (listed) {
    i = pairs[2 * p];
    j = pairs[2 * p + 1];
    valid = i >= 0 && i < n_atoms && j >= 0 && j < n_atoms;
  }
  if (valid) {
    g = gamma[p];
    if (scale) {
      ti = scale[i];
      tj = scale[j];
    }
    if (DIM == 3) {
      const double dx = coord[3 * j + 0] - coord[3 * i + 0];
      const double dy = coord[3 * j + 1] - coord[3 * i + 1];
      const double dz = coord[3 * j + 2] - coord[3 * i + 2];
      const double len = sqrt((dx * dx + dy * dy) + dz * dz);
      n[0] = dx / len;
      n[1] = dy / len;
      n[2] = dz / len;
    }
  }
  for (long long r = blockIdx.y; r < q; r += gridDim.y) {
    double v = listed ? 0.0 : __builtin_nan("");   // (a listed pair with an atom outside 0 .. N - 1 is skipped: 0.0)
    if (valid) {
      const double* __restrict__ xr = x + r * m;
      double e;
      if (DIM == 3) {
        const double ex = ti * xr[3 * i + 0] - tj * xr[3 * j + 0];
        const double ey = ti * xr[3 * i + 1] - tj * xr[3 * j + 1];
        const double ez = ti * xr[3 * i + 2] - tj * xr[3 * j + 2];
        e = (n[0] * ex + n[1] * ey) + n[2] * ez;
      } else {
        e = ti * xr[i] - tj * xr[j];
      }
      v = (g * e) * e;
    }
    out[r * ks + s] = v;
  }
}

constexpr long long kStrainRowLanes = 64;   // grid.y of k_pairs_strain: rows r, r + 64, ... per thread

}  // namespace

int launch_pairs_apply(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs, int64_t k,
                       const double* d_gamma, const int64_t* d_row_start, const double* d_atom_scale, const double* d_x,
                       int64_t q, double* d_y, double* d_energy) {
  if (q == 0) return SC_OK;
  const dim3 grid((unsigned)((n_atoms + 3) / 4));
  if (dim == 3)
    hipLaunchKernelGGL(k_pairs_apply<3>, grid, dim3(256), 0, ctx->stream, d_coord, (long long)n_atoms,
                       (const long long*)d_pairs, (long long)k, d_gamma, (const long long*)d_row_start, d_atom_scale,
                       d_x, (long long)q, d_y, d_energy);
  else
    hipLaunchKernelGGL(k_pairs_apply<1>, grid, dim3(256), 0, ctx->stream, d_coord, (long long)n_atoms,
                       (const long long*)d_pairs, (long long)k, d_gamma, (const long long*)d_row_start, d_atom_scale,
                       d_x, (long long)q, d_y, d_energy);
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

int launch_pairs_strain(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs, int64_t k,
                        const double* d_gamma, const double* d_atom_scale, const int64_t* d_pair_idx, int64_t ks,
                        const double* d_x, int64_t q, double* d_out) {
  if (q == 0 || ks == 0) return SC_OK;
  const dim3 grid((unsigned)((ks + 255) / 256), (unsigned)(q < kStrainRowLanes ? q : kStrainRowLanes));
  if (dim == 3)
    hipLaunchKernelGGL(k_pairs_strain<3>, grid, dim3(256), 0, ctx->stream, d_coord, (long long)n_atoms,
                       (const long long*)d_pairs, (long long)k, d_gamma, d_atom_scale, (const long long*)d_pair_idx,
                       (long long)ks, d_x, (long long)q, d_out);
  else
    hipLaunchKernelGGL(k_pairs_strain<1>, grid, dim3(256), 0, ctx->stream, d_coord, (long long)n_atoms,
                       (const long long*)d_pairs, (long long)k, d_gamma, d_atom_scale, (const long long*)d_pair_idx,
                       (long long)ks, d_x, (long long)q, d_out);
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}
