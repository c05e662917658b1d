// The walk over one atom's pairs on a column panel, shared by k_pairs_panel (pair_panel.hip) and k_cg_apply_dot
// (pair_cg.hip): both instantiate this one function, so the sums s[] of a column have the same bits in both.  The files that
// include it are compiled with -ffp-contract=off (build.py).
//
// One wavefront owns (atom i, a chunk of 64 columns), lane = column.  It walks the atom's pairs row_start[i] ..
// row_start[i + 1] - 1 in list order, 64 at a time: every lane loads ONE pair of the 64 (j, gamma, t_j) and computes its
// n_p -- the square root and the three divisions cost a pair one lane-instruction instead of one per column -- and the
// wavefront then takes the 64 pairs one after the other, each broadcast from its lane into scalar registers (v_readlane, a
// uniform lane index).  Per pair and component a lane gathers X[dim j + c, r]: the wavefront reads 64 consecutive doubles,
// one fully used 512-byte row segment.  A lane adds its own dim sums in registers, sequentially in pair order.  No LDS, no
// atomics, no sum across lanes.  Rows of the list whose first atom is not i or whose second lies outside 0 .. N - 1 are
// skipped.
#ifndef SPRINGCRAFT_PAIR_WALK_H
#define SPRINGCRAFT_PAIR_WALK_H
#include "common.h"

namespace {

__device__ __forceinline__ double lane_value(double v, int l) {   // v of lane l (uniform) in every lane
  const long long bits = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)bits, l);
  const int hi = __builtin_amdgcn_readlane((int)(bits >> 32), l);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// s[c] += sum over the pairs (i, j) of gamma_p e_p n_p[c] (dim 1: gamma_p e_p) for the column xc points at (element (row,
// this lane's column) at xc[row * ld]), with ui[c] = t_i x[dim i + c].  Every lane of the wavefront must call it (the
// broadcasts are convergent); i < n_atoms.
template <int DIM>
__device__ __forceinline__ void pair_walk(const double* __restrict__ coord, long long n_atoms,
                                          const long long* __restrict__ pairs, long long k,
                                          const double* __restrict__ gamma, const long long* __restrict__ row_start,
                                          const double* __restrict__ scale, const double* __restrict__ xc, long long ld,
                                          long long i, int lane, const double (&ui)[DIM], double (&s)[DIM]) {
  long long lo = 0, hi = 0;
  if (k > 0) {
    lo = row_start[i];
    hi = row_start[i + 1];
    if (lo < 0) lo = 0;
    if (hi > k) hi = k;
  }
  double ci[3] = {0.0, 0.0, 0.0};
  if (DIM == 3 && lo < hi) {
    ci[0] = coord[3 * i + 0];
    ci[1] = coord[3 * i + 1];
    ci[2] = coord[3 * i + 2];
  }

  for (long long c0 = lo; c0 < hi; c0 += 64) {
    // this lane's pair of the 64: j, gamma, t_j, n_p (skipped: an entry whose first atom is not i or whose second lies
    // outside 0 .. N - 1)
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
        const double dx = coord[3 * j + 0] - ci[0];
        const double dy = coord[3 * j + 1] - ci[1];
        const double dz = coord[3 * j + 2] - ci[2];
        const double len = sqrt((dx * dx + dy * dy) + dz * dz);
        n[0] = dx / len;   // (two atoms at one position: 0 / 0 = NaN, as the Hessian entry)
        n[1] = dy / len;
        n[2] = dz / len;
      }
    }
    const unsigned long long listed = __ballot(valid);
    const int count = (int)(hi - c0 < 64 ? hi - c0 : 64);

    // the pair of lane l (uniform; every lane of the wavefront is active here) from scalar registers; j < 2^32 (the entry
    // refuses more atoms)
    auto add_pair = [&](int l) {
      const long long jl = (long long)(unsigned int)__builtin_amdgcn_readlane((int)j, l);
      const double gl = lane_value(g, l);
      const double tl = lane_value(tj, l);
      if (DIM == 3) {
        const double n0 = lane_value(n[0], l), n1 = lane_value(n[1], l), n2 = lane_value(n[2], l);
        const double ex = ui[0] - tl * xc[(3 * jl + 0) * ld];
        const double ey = ui[1] - tl * xc[(3 * jl + 1) * ld];
        const double ez = ui[2] - tl * xc[(3 * jl + 2) * ld];
        const double e = (n0 * ex + n1 * ey) + n2 * ez;
        const double ge = gl * e;
        s[0] += ge * n0;
        s[1] += ge * n1;
        s[2] += ge * n2;
      } else {
        const double e = ui[0] - tl * xc[jl * ld];
        s[0] += gl * e;
      }
    };
    // All loops add the listed pairs in list order.  The first, for a chunk without a skipped row (every chunk of a
    // checked list), takes four pairs per step without a branch between them, so that their gathers are in flight
    // together (unrolled by hand: the compiler does not unroll a loop of convergent operations with a remainder).
    if (listed == (count == 64 ? ~0ull : (1ull << count) - 1)) {
      int l = 0;
      for (; l + 4 <= count; l += 4) {
        add_pair(l);
        add_pair(l + 1);
        add_pair(l + 2);
        add_pair(l + 3);
      }
      for (; l < count; ++l) add_pair(l);
    } else {
      for (unsigned long long rest = listed; rest; rest &= rest - 1) add_pair(__builtin_ctzll(rest));
    }
  }
}

}  // namespace
#endif
