// The least-squares RMSD of every pair of frames of one ensemble, or of every frame of one with every frame of another,
// without a rotation formed or a frame written.  No reference counterpart (Bio3D: rmsd(xyz, fit = TRUE); ProDy, MDTraj and
// MDAnalysis have their own pairwise RMSD matrices).
//
// Atom weights w_a >= 0 (1 if null), W = sum w.  Per frame f: c_f = sum w x_f / W, y_f = x_f - c_f, G_f = sum_a w_a
// |y_f[a]|^2.  Per pair: S = sum_a w_a y_f[a] y_g[a]^T, lambda the largest eigenvalue of Horn's 4 x 4 matrix N(S) (the
// one horn_rotation of superpose.hip builds; it belongs to a proper rotation, also for a mirror image),
//     msd(f, g) = max(0, (G_f + G_g) - 2 lambda) / W,     rmsd = sqrt(msd).
// Without the fit y_f = x_f - o, o the weighted centroid of the first frame of the first ensemble (0 where that is not
// finite), and lambda = tr S: a common origin keeps the cancellation at the scale of the structure, not of its position.
//
// k_rmsd_prepare, one workgroup per frame: the centroid and G_f, every sum a per-thread sum over the atoms tid, tid + T, ...
// in ascending order followed by block_sum as in superpose.hip, and the transposed copy Y[a][d][f] = sqrt(w_a) y_f[a][d]
// of shape (N_pad, 3, M_pad): M_pad a multiple of the tile side, N_pad of the staged atom group, every pad entry written
// as exactly 0.0 by the workgroups of the pad frames and by every frame's workgroup behind its last atom.  A non-finite
// coordinate makes G_f NaN (0 * NaN of a zero-weight atom included).
//
// k_rmsd_product is the core of pair_block_tile.h with frames and atoms in swapped roles, in a copy of its own (on the
// shared functions it took 1.3 % longer at 10^4 x 2000: profiles/pair_block_tile.txt).  One workgroup of 512 lanes owns a 64 x 64 tile of
// frame pairs and walks the atoms in ascending order, kRows at a time: 2 x 192 lanes fetch the 64 consecutive doubles of
// the three components of the tile's two frame sets of each atom while the previous group is multiplied, into LDS as
// [atom][side][component][frame].  A 16 x 16 x 4 MFMA is "component d of 16 frames f times component e of 16 frames g,
// summed over 4 atoms": lane l gives A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] and holds D[i = 4 reg + (l >>
// 4)][j = l & 15].  Wavefront w owns the 16 frames f0 + 16 (w & 3) .. and two blocks of 16 frames g, 32 (w >> 2) ..: 2 x 9
// accumulators, and the nine entries of one S_fg sit in the same lane and register slot of nine of them.  The epilogue
// builds N(S) there and runs an eigenvalue-only cyclic Jacobi (threshold and sweep limit of horn_rotation, no vectors).
//
// Self-comparison: only tiles with tile_f >= tile_g exist; they store (f, g) and (g, f) from the same register, a diagonal
// tile from its f > g lanes, and its f = g lanes store the diagonal: exactly 0.0, NaN for a non-finite frame.  The matrix
// equals its transpose bit for bit.  A pair one of whose frames has a NaN G is NaN, and no other entry is: S_fg holds no
// other frame's numbers.  No atomics, no partial sums across workgroups, and an output element's arithmetic does not
// depend on its lane: an entry's bits depend on its two frames, the weights and the fit alone.
//
// Per (pair, atom): 9 multiply-adds = 18 flops on the matrix pipe; a tile reads 2 x 192 doubles of an atom for its 4096
// pairs, 0.75 bytes per (pair, atom) from memory and the same again into LDS.  Per pair: one Jacobi in one lane.
//
// Neighbour bits (launch_frame_neighbours).  The same kernel with a second epilogue, for a self-comparison: instead of the
// value a pair's bit, value <= cutoff, goes into the (n, ceil(n / 64)) bit matrix adj that neighbour-count clustering runs
// on (cluster.hip), and the (n, n) matrix is never stored: 1 bit per ordered pair instead of 64.  pair_value is the one
// value function of both epilogues, so a bit is the comparison of exactly the double the matrix would hold.  A 64 x 64
// tile is one 64-bit word of 64 rows, word tile_g of the rows f0 .. f0 + 63.  Per (j, r) a wavefront's __ballot is 4 rows
// (fk) x 16 columns (fr): bits 16 fk .. 16 fk + 15 are the columns 16 (gb0 + j) .. + 15 of row 16 fb + 4 r + fk, and the
// lane fr = 0 of every 16-lane group stores them as quarter gb0 + j of that row's word, one uint16_t of a 64-word tile in
// the staging LDS; the wavefronts w and w ^ 4 supply the two halves of a word.  Then 64 lanes store the rows' words and,
// off the diagonal, 64 more the transposed words (bit i' of column i from row i' of the tile): word tile_f of the rows g0
// .. g0 + 63.  A diagonal tile computes f > g only and ORs the tile with its transpose and the diagonal before its one
// store.  The semantics are k_cluster_pack's: a valid frame (G not NaN) is its own neighbour, an invalid frame's row and
// column are zero, the bits of the columns >= n of the last word are zero.  Every word of adj is written exactly once, by
// one workgroup: no memset, no atomics, adj equals its transpose bit for bit.  k_neighbour_finish, one wavefront per row:
// the row's popcount, label -1, the validity words from G and the status of a clustering run.
#include <cmath>
#include <cstdint>

#include "block_sum.h"
#include "eigh_internal.h"
#include "cluster_policy.h"
#include "ensemble_internal.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kTile = sc_host::kRmsdTile;     // frames per side of a tile: 4 blocks of 16
constexpr int kRows = sc_host::kRmsdRows;     // atoms staged in LDS at a time: two MFMA steps of 4
constexpr int kSide = 3 * kTile;              // doubles of one frame set of one atom
// one staged atom: the f side, the g side and 16 doubles more, so that the four atoms one MFMA operand load touches start
// in alternating halves of the LDS banks (2 kSide doubles are a multiple of the 256-byte bank row)
constexpr int kRowStride = 2 * kSide + 16;
constexpr int kJacobiSweeps = 30;             // horn_rotation's
static_assert(kTile == 64 && kRows % 4 == 0, "the lane mapping below is written for 64 x 64 tiles and MFMA steps of 4");
// (pair_block_tile.h asserts that its tile is this one)

__device__ __forceinline__ bool is_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// grid (M_pad): frame f of `frames` (n_frames, n, 3); origin: null (fit: the frame's own centroid) or the frame whose
// weighted centroid is the common origin
__global__ __launch_bounds__(256) void k_rmsd_prepare(const double* __restrict__ frames, long long n_frames, long long n,
                                                      long long n_pad, long long m_pad,
                                                      const double* __restrict__ weights,
                                                      const double* __restrict__ origin, double* __restrict__ Y,
                                                      double* __restrict__ G, double* __restrict__ wsum) {
  __shared__ double red[4 * 4];
  const long long f = blockIdx.x;
  const int tid = threadIdx.x, nt = blockDim.x;
  if (f >= n_frames) {   // (the whole workgroup) a pad frame
    for (long long i = tid; i < 3 * n_pad; i += nt) Y[i * m_pad + f] = 0.0;
    if (tid == 0) G[f] = 0.0;
    return;
  }
  const double* x = frames + f * 3 * n;
  const double* cx = origin ? origin : x;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long a = tid; a < n; a += nt) {
    const double w = weights ? weights[a] : 1.0;
    s[0] += w * cx[3 * a + 0];
    s[1] += w * cx[3 * a + 1];
    s[2] += w * cx[3 * a + 2];
    s[3] += w;
  }
  block_sum<4>(s, red);
  double c0 = s[0] / s[3], c1 = s[1] / s[3], c2 = s[2] / s[3];
  if (origin && !(is_finite(c0) && is_finite(c1) && is_finite(c2))) c0 = c1 = c2 = 0.0;

  double g[1] = {0.0};
  for (long long a = tid; a < n; a += nt) {
    const double w = weights ? weights[a] : 1.0;
    const double d0 = x[3 * a + 0] - c0, d1 = x[3 * a + 1] - c1, d2 = x[3 * a + 2] - c2;
    g[0] += w * ((d0 * d0 + d1 * d1) + d2 * d2);
    const double sw = sqrt(w);
    Y[(3 * a + 0) * m_pad + f] = sw * d0;
    Y[(3 * a + 1) * m_pad + f] = sw * d1;
    Y[(3 * a + 2) * m_pad + f] = sw * d2;
  }
  for (long long i = 3 * n + tid; i < 3 * n_pad; i += nt) Y[i * m_pad + f] = 0.0;
  block_sum<1>(g, red);
  if (tid == 0) {
    G[f] = is_finite(g[0]) ? g[0] : __builtin_nan("");
    if (f == 0 && wsum) wsum[0] = s[3];
  }
}

// The largest eigenvalue of Horn's N(S), S row-major: horn_rotation's matrix, threshold and rotations, without the vectors.
__device__ __forceinline__ double horn_lambda(const double (&S)[9]) {
  const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
  double A[4][4];
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
    for (int j = 0; j < 4; ++j) scale2 += A[i][j] * A[i][j];
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
        for (int k = 0; k < 4; ++k)
          if (k != p && k != q) {
            const double akp = A[k][p], akq = A[k][q];
            A[k][p] = A[p][k] = c * akp - s * akq;
            A[k][q] = A[q][k] = s * akp + c * akq;
          }
        A[p][p] -= t * apq;
        A[q][q] += t * apq;
        A[p][q] = A[q][p] = 0.0;
      }
    if (!rotated) break;
  }
  double best = A[0][0];
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (A[j][j] > best) best = A[j][j];
  return best;
}

// The value of one pair from its nine sums (slot r of the accumulators S), the two frames' G and W: NaN when a frame is not
// finite, exactly 0 for a frame with itself (`same`), else max(0, (Gf + Gg) - 2 lambda) / W or its root.  Both epilogues of
// k_rmsd_product call this and nothing else.
__device__ __forceinline__ double pair_value(const d4 (&S)[3][3], int r, double Gf, double Gg, double W, bool same, int fit,
                                             int squared) {
  const bool bad = Gf != Gf || Gg != Gg;
  double v;
  if (bad) {
    v = __builtin_nan("");
  } else if (same) {
    v = 0.0;
  } else {
    double lambda;
    if (fit) {
      double s[9];
#pragma unroll
      for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int e = 0; e < 3; ++e) s[3 * d + e] = S[d][e][r];
      lambda = horn_lambda(s);
    } else {
      lambda = (S[0][0][r] + S[1][1][r]) + S[2][2][r];
    }
    v = fmax(0.0, (Gf + Gg) - 2.0 * lambda) / W;
    if (!squared) v = sqrt(v);
  }
  return v;
}

struct RmsdArgs {
  static constexpr bool kBits = false;
  const double* ya;   // (N_pad, 3, m_pad_a): the f side
  const double* yb;   // (N_pad, 3, m_pad_b): the g side; a self-comparison: ya
  const double* ga;   // (m_pad_a)
  const double* gb;   // (m_pad_b)
  const double* wsum;
  double* out;        // (n_a, n_b)
  long long m_pad_a, m_pad_b;
  int n_a, n_b, groups;   // groups: N_pad / kRows
  int tiles_b;            // 0: self-comparison, the triangle of tiles; else tiles along g
  int fit, squared;
};
// the bit epilogue's: a self-comparison (tiles_b = 0, n_b = n_a, out unused)
struct NeighbourArgs : RmsdArgs {
  static constexpr bool kBits = true;
  unsigned long long* adj;   // (n_a, words)
  long long words;
  double cutoff;
};

typedef unsigned long long u64;
// the bit tile in the staging buffer: written as uint16_t quarters, read as words
typedef uint16_t __attribute__((may_alias)) tile_u16;
typedef u64 __attribute__((may_alias)) tile_u64;

// grid (tiles).  Args: RmsdArgs, the (n_a, n_b) matrix; NeighbourArgs, the neighbour bits of a self-comparison.
template <class Args>
__global__ __launch_bounds__(512) void k_rmsd_product(const Args A) {
  __shared__ double lds[kRows * kRowStride];
  const int tid = threadIdx.x;
  const bool self = A.tiles_b == 0;
  int tf, tg;
  if (self) {
    tri_tile_decode(blockIdx.x, tf, tg);
  } else {
    tf = blockIdx.x / A.tiles_b;
    tg = blockIdx.x - tf * A.tiles_b;
  }
  const int f0 = tf * kTile, g0 = tg * kTile;   // self: g0 <= f0

  // the loader lanes: lanes 0..191 take the f side, 192..383 the g side; column `col` of a side is component `comp` of its
  // frame `frame`, consecutive lanes consecutive frames
  const bool loader = tid < 2 * kSide, f_side = tid < kSide;
  const int col = f_side ? tid : tid - kSide;
  const int comp = col / kTile, frame = col - kTile * comp;
  const long long ld = f_side ? A.m_pad_a : A.m_pad_b;
  // (a, comp, frame) of the side's copy is at 3 a ld + src: inside it for a < N_pad, the tile lies within M_pad
  const double* src = (f_side ? A.ya : A.yb) + comp * ld + (f_side ? f0 : g0) + frame;
  const int slot = (f_side ? 0 : kSide) + col;

  // the MFMA lanes: wavefront w, lane (fr, fk) supplies frame 16 fb + fr of the f side and frame 16 (gb0 + j) + fr of the g
  // side, both of atom fk of a step
  const int w = tid >> 6, fr = tid & 15, fk = (tid >> 4) & 3;
  const int fb = w & 3, gb0 = 2 * (w >> 2);
  const double* la = lds + fk * kRowStride + 16 * fb + fr;
  const double* lc = lds + fk * kRowStride + kSide + 16 * gb0 + fr;
  d4 acc[2][3][3];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
      for (int e = 0; e < 3; ++e) acc[j][d][e] = d4{0.0, 0.0, 0.0, 0.0};

  double pre[kRows];
  if (loader)
#pragma unroll
    for (int r = 0; r < kRows; ++r) pre[r] = src[3 * (long long)r * ld];
  for (int grp = 0; grp < A.groups; ++grp) {
    __syncthreads();   // the previous group has been multiplied
    if (loader)
#pragma unroll
      for (int r = 0; r < kRows; ++r) lds[r * kRowStride + slot] = pre[r];
    __syncthreads();
    if (loader && grp + 1 < A.groups)
#pragma unroll
      for (int r = 0; r < kRows; ++r) pre[r] = src[3 * ((long long)(grp + 1) * kRows + r) * ld];
#pragma unroll
    for (int k4 = 0; k4 < kRows / 4; ++k4) {
      double af[3], bf[2][3];
#pragma unroll
      for (int d = 0; d < 3; ++d) af[d] = la[4 * k4 * kRowStride + d * kTile];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 3; ++e) bf[j][e] = lc[4 * k4 * kRowStride + e * kTile + 16 * j];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
          for (int e = 0; e < 3; ++e)
            acc[j][d][e] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[d], bf[j][e], acc[j][d][e], 0, 0, 0);
    }
  }

  const bool diag = self && tf == tg;
  const double W = A.wsum[0];
  if constexpr (!Args::kBits) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int g = g0 + 16 * (gb0 + j) + fr;
      const double Gg = g < A.n_b ? A.gb[g] : 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = f0 + 16 * fb + 4 * r + fk;
        if (f >= A.n_a || g >= A.n_b || (diag && f < g)) continue;
        const double v = pair_value(acc[j], r, A.ga[f], Gg, W, diag && f == g, A.fit, A.squared);
        A.out[(size_t)f * A.n_b + g] = v;
        if (self && f != g) A.out[(size_t)g * A.n_b + f] = v;
      }
    }
  } else {
    const int n = A.n_a;
    __syncthreads();   // every wavefront has read the last staged group: the buffer is free
    tile_u16* tile16 = reinterpret_cast<tile_u16*>(lds);
    const tile_u64* tile = reinterpret_cast<const tile_u64*>(lds);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int g = g0 + 16 * (gb0 + j) + fr;
      const double Gg = g < n ? A.gb[g] : 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * fb + 4 * r + fk, f = f0 + row;
        bool in = false;
        // (a NaN value, an invalid frame's, is not <= cutoff; the diagonal is set below)
        if (f < n && g < n && !(diag && f <= g)) in = pair_value(acc[j], r, A.ga[f], Gg, W, false, A.fit, A.squared) <= A.cutoff;
        const u64 m = __ballot(in);
        if (fr == 0) tile16[4 * row + gb0 + j] = (uint16_t)(m >> (16 * fk));
      }
    }
    __syncthreads();
    if (tid < 128) {
      const int i = tid & 63;
      const bool across = tid >= 64;   // the transposed words: off the diagonal only
      if (!(across && diag)) {
        u64 word = 0, column = 0;
        if (!across) word = tile[i];
        if (across || diag)
          for (int k = 0; k < 64; ++k) column |= ((tile[k] >> i) & 1ull) << k;
        const int row = (across ? g0 : f0) + i;
        if (row < n) {
          if (diag) {
            const double G = A.ga[row];
            word |= column | (G == G ? 1ull << i : 0ull);
          } else if (across) {
            word = column;
          }
          A.adj[(size_t)row * A.words + (across ? tf : tg)] = word;
        }
      }
    }
  }
}

// grid (ceil(n / 4)), 256 threads: one wavefront per row of adj.  count[i] <- the row's popcount; labels[i] <- -1; the
// wavefront of row 64 w: word w of valid (and alive) <- the frames whose G is not NaN.  Workgroup 0 also: ctl <- 0, status
// <- (valid frames, 0, 0, 0).  alive, labels, ctl and status may be null (status and ctl together).
__global__ __launch_bounds__(256) void k_neighbour_finish(const u64* __restrict__ adj, const double* __restrict__ G, long long n,
                                                          long long words, int* __restrict__ count, u64* __restrict__ valid,
                                                          u64* __restrict__ alive, int* __restrict__ labels,
                                                          int* __restrict__ ctl, int* __restrict__ status) {
  __shared__ int red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long i = (long long)blockIdx.x * 4 + wave;
  if (i < n) {
    int c = 0;
    for (long long w = lane; w < words; w += 64) c += __popcll(adj[i * words + w]);
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
    if (lane == 0) {
      count[i] = c;
      if (labels) labels[i] = -1;
    }
    if ((i & 63) == 0) {
      bool ok = false;
      if (i + lane < n) {
        const double g = G[i + lane];
        ok = g == g;
      }
      const u64 m = __ballot(ok);
      if (lane == 0) {
        valid[i >> 6] = m;
        if (alive) alive[i >> 6] = m;
      }
    }
  }
  if (blockIdx.x == 0 && status) {   // (the whole workgroup)
    int ok = 0;
    for (long long j = threadIdx.x; j < n; j += 256) {
      const double g = G[j];
      ok += g == g;
    }
    for (int off = 32; off >= 1; off >>= 1) ok += __shfl_xor(ok, off);
    if (lane == 0) red[wave] = ok;
    __syncthreads();
    if (threadIdx.x < sc_host::kClusterCtlInts) ctl[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
      status[0] = ((red[0] + red[1]) + red[2]) + red[3];
      status[1] = status[2] = status[3] = 0;
    }
  }
}

}  // namespace

int launch_rmsd_matrix(sc_ctx* ctx, const sc_host::RmsdBufs& B, const double* d_a, int64_t n_a, const double* d_b,
                       int64_t n_b, int64_t n_atoms, const double* d_weights, bool fit, bool squared, double* d_out) {
  hipStream_t st = ctx->stream;
  const long long n_pad = sc_host::rmsd_pad_atoms(n_atoms);
  const long long ma = sc_host::rmsd_pad_frames(n_a), mb = d_b ? sc_host::rmsd_pad_frames(n_b) : 0;
  const double* origin = fit ? nullptr : d_a;
  hipLaunchKernelGGL(k_rmsd_prepare, dim3((unsigned)ma), dim3(256), 0, st, d_a, (long long)n_a, (long long)n_atoms, n_pad,
                     ma, d_weights, origin, B.ya, B.ga, B.wsum);
  if (d_b)
    hipLaunchKernelGGL(k_rmsd_prepare, dim3((unsigned)mb), dim3(256), 0, st, d_b, (long long)n_b, (long long)n_atoms,
                       n_pad, mb, d_weights, origin, B.yb, B.gb, (double*)nullptr);
  RmsdArgs A{};
  A.ya = B.ya; A.ga = B.ga;
  A.yb = d_b ? B.yb : B.ya; A.gb = d_b ? B.gb : B.ga;
  A.wsum = B.wsum; A.out = d_out;
  A.m_pad_a = ma; A.m_pad_b = d_b ? mb : ma;
  A.n_a = (int)n_a; A.n_b = (int)n_b;
  A.groups = (int)(n_pad / kRows);
  A.tiles_b = d_b ? (int)(mb / kTile) : 0;
  A.fit = fit; A.squared = squared;
  const unsigned tiles = (unsigned)sc_host::rmsd_tiles(n_a, d_b ? n_b : 0);
  hipLaunchKernelGGL(k_rmsd_product<RmsdArgs>, dim3(tiles), dim3(512), 0, st, A);
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

int launch_frame_neighbours(sc_ctx* ctx, const sc_host::RmsdBufs& B, const double* d_frames, int64_t n, int64_t n_atoms,
                            const double* d_weights, bool fit, bool squared, double cutoff, uint64_t* d_adj,
                            int32_t* d_count, uint64_t* d_valid, uint64_t* d_alive, int32_t* d_labels, int32_t* d_ctl,
                            int32_t* d_status) {
  hipStream_t st = ctx->stream;
  const long long n_pad = sc_host::rmsd_pad_atoms(n_atoms), m_pad = sc_host::rmsd_pad_frames(n);
  const long long words = sc_host::cluster_words(n);   // (= m_pad / kTile: a tile is a word)
  hipLaunchKernelGGL(k_rmsd_prepare, dim3((unsigned)m_pad), dim3(256), 0, st, d_frames, (long long)n, (long long)n_atoms,
                     n_pad, m_pad, d_weights, fit ? nullptr : d_frames, B.ya, B.ga, B.wsum);
  NeighbourArgs A{};
  A.ya = A.yb = B.ya; A.ga = A.gb = B.ga;
  A.wsum = B.wsum; A.out = nullptr;
  A.m_pad_a = A.m_pad_b = m_pad;
  A.n_a = A.n_b = (int)n;
  A.groups = (int)(n_pad / kRows);
  A.tiles_b = 0;
  A.fit = fit; A.squared = squared;
  A.adj = (u64*)d_adj; A.words = words; A.cutoff = cutoff;
  hipLaunchKernelGGL(k_rmsd_product<NeighbourArgs>, dim3((unsigned)sc_host::rmsd_tiles(n, 0)), dim3(512), 0, st, A);
  hipLaunchKernelGGL(k_neighbour_finish, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, (const u64*)d_adj,
                     (const double*)B.ga, (long long)n, words, d_count, (u64*)d_valid, (u64*)d_alive, d_labels, d_ctl,
                     d_status);
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}
