// One fused Chebyshev step of the pair-list operator on a column panel: Z <- alpha (T H T) X + beta X + gamma_c Z.
// No reference counterpart.  The matrix T H T is the one of k_pairs_apply (pair_operator.hip, whose header has the pair
// list, d_p, n_p, t_a and the formulas); what differs is the arrangement, made for an iteration that applies H hundreds of
// times to a block of 30 .. 200 vectors.
//
// Layout.  A panel has m = dim N rows and q columns with leading dimension ld >= q: element (row dim a + c, column r) at
// X[(dim a + c) ld + r].  Columns are the vectors.
//
// k_pairs_panel: one wavefront owns (atom i, a chunk of 64 columns), lane = column.  It walks the atom's pairs
// row_start[i] .. row_start[i + 1] - 1 in list order, 64 at a time: every lane loads ONE pair of the 64 (j, gamma, t_j) and
// computes its n_p -- the square root and the three divisions cost a pair one lane-instruction instead of one per column
// -- and the wavefront then takes the 64 pairs one after the other, each broadcast from its lane into scalar registers
// (v_readlane, a uniform lane index).  Per pair and component a lane gathers X[dim j + c, r]: the wavefront reads 64
// consecutive doubles, one fully used 512-byte row segment.  A lane adds its own dim sums in registers, sequentially in
// pair order, and stores alpha (t_i sum) + beta X[i] (+ gamma_c Z[i]).  No LDS, no atomics, no workspace, and no sum
// across lanes: a column's bits depend on the atom's pair range alone, not on q, ld, the column's position or the other
// columns (the file is compiled with -ffp-contract=off, build.py, so every operation is the one written, and a pair's
// geometry is the same number whichever lane computed it).
//
// Workgroup: 256 threads = four wavefronts that take four consecutive ATOMS of one column chunk, not one atom's four
// chunks.  (1) Neighbours in the list are neighbours in space: consecutive atoms share most of their partners j, so
// the four wavefronts gather the same rows of X and the second to fourth find them in the CU's vector L1.  Four chunks of
// one atom share only the pair data, 40 bytes per pair against 1536 per pair and chunk of X.  (2) The solver's panels
// have 30 .. 200 columns, one to four chunks: four chunks per workgroup would leave one to three wavefronts of every
// workgroup without work, four atoms keep all of them busy at every q.  The kernel uses some 40 VGPRs, so eight
// wavefronts per SIMD hide the latency of the gathers.
//
// Edge rules.  An atom without pairs: the H term is exactly 0.0, the result beta X + gamma_c Z.  Rows of the list whose
// first atom is not i or whose second lies outside 0 .. N - 1 are skipped, as in k_pairs_apply.  Z is read only when
// gamma_c != 0 (with gamma_c = 0 it is overwritten, whatever it held); lanes beyond q load pair data like the others,
// read no column beyond q and write nothing, so the columns q .. ld - 1 of Z keep their bits.
#include "pair_walk.h"   // the walk itself, shared with k_cg_apply_dot (pair_cg.hip)

namespace {

template <int DIM>
__global__ __launch_bounds__(256) void k_pairs_panel(const double* __restrict__ coord, long long n_atoms,
                                                     const long long* __restrict__ pairs, long long k,
                                                     const double* __restrict__ gamma,
                                                     const long long* __restrict__ row_start,
                                                     const double* __restrict__ scale, const double* __restrict__ x,
                                                     double* __restrict__ z, long long ld, long long q, double alpha,
                                                     double beta, double gamma_c) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (i >= n_atoms) return;
  const long long col = (long long)blockIdx.y * 64 + lane;
  const bool live = col < q;
  const double ti = scale ? scale[i] : 1.0;
  // a lane beyond q reads the chunk's first column in place of its own (the same addresses, no further traffic) and stores
  // nothing: the walk then has no divergent branch
  const double* __restrict__ xc = x + (live ? col : (long long)blockIdx.y * 64);
  double xi[DIM], ui[DIM], s[DIM];
#pragma unroll
  for (int c = 0; c < DIM; ++c) {
    xi[c] = xc[(DIM * i + c) * ld];
    ui[c] = ti * xi[c];
    s[c] = 0.0;
  }
  pair_walk<DIM>(coord, n_atoms, pairs, k, gamma, row_start, scale, xc, ld, i, lane, ui, s);

  if (!live) return;
  double* __restrict__ zc = z + col;
#pragma unroll
  for (int c = 0; c < DIM; ++c) {
    const long long at = (DIM * i + c) * ld;
    double v = alpha * (ti * s[c]) + beta * xi[c];
    if (gamma_c != 0.0) v += gamma_c * zc[at];
    zc[at] = v;
  }
}

}  // namespace

int launch_pairs_panel(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs, int64_t k,
                       const double* d_gamma, const int64_t* d_row_start, const double* d_atom_scale, const double* d_x,
                       double* d_z, int64_t ld, int64_t q, double alpha, double beta, double gamma_c) {
  if (q == 0) return SC_OK;
  const dim3 grid((unsigned)((n_atoms + 3) / 4), (unsigned)((q + 63) / 64));
  if (dim == 3)
    hipLaunchKernelGGL(k_pairs_panel<3>, grid, dim3(256), 0, ctx->stream, d_coord, (long long)n_atoms,
                       (const long long*)d_pairs, (long long)k, d_gamma, (const long long*)d_row_start, d_atom_scale,
                       d_x, d_z, (long long)ld, (long long)q, alpha, beta, gamma_c);
  else
    hipLaunchKernelGGL(k_pairs_panel<1>, grid, dim3(256), 0, ctx->stream, d_coord, (long long)n_atoms,
                       (const long long*)d_pairs, (long long)k, d_gamma, (const long long*)d_row_start, d_atom_scale,
                       d_x, d_z, (long long)ld, (long long)q, alpha, beta, gamma_c);
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}
