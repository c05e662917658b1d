// The host decisions of the conformational-ensemble entries (superpose.hip, ensemble_pca.hip, rmsd_matrix.hip,
// api_ensemble.hip): which kernel form a superposition takes, which product an ensemble PCA forms and with how many K
// slices, the pads and tiles of the pairwise RMSD matrix, and the layout of their scratch.  Same rules as gemm_policy.h:
// closed-form functions of their inputs, no HIP, header-only; tests/host_sanitize/test_ensemble_logic.cpp compiles exactly this code with g++ -fsanitize=address,undefined.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "scratch_arena.h"

namespace sc_host {

// ---- superposition: one workgroup per frame ---------------------------------------------------------------------------
// LDS form: the frame (3 N doubles of dynamic LDS) is read once into LDS and written once; kSuperposeRedDoubles more, static,
// hold the partial sums of the workgroup's reductions and the rotation.  2560 atoms are 62720 bytes in all, inside the 64 KB
// a kernel gets without raising its limit (N = 2000: 48 KB + 1280).  Larger frames take the streaming form, which reads the
// frame three times and writes it once.
constexpr int kSuperposeLdsMaxAtoms = 2560;
constexpr int kSuperposeRedDoubles = 160;   // 16 wavefronts x 9 sums, 16 for the rotation and translation
constexpr int kSuperposeFormLds = 0, kSuperposeFormStream = 1;

// SPRINGCRAFT_SUPERPOSE_FORM: unset / "auto": by size; "lds": the LDS form wherever the frame fits; "stream": always the
// streaming form.  Read at every call (a test switches it between two calls of one process).
constexpr int kSuperposeEnvAuto = 0, kSuperposeEnvLds = 1, kSuperposeEnvStream = 2;
static inline int parse_superpose_env(const char* e) {
  if (!e || !*e || !std::strcmp(e, "auto")) return kSuperposeEnvAuto;
  if (!std::strcmp(e, "lds")) return kSuperposeEnvLds;
  if (!std::strcmp(e, "stream")) return kSuperposeEnvStream;
  return kSuperposeEnvAuto;
}
static inline int read_superpose_env() { return parse_superpose_env(std::getenv("SPRINGCRAFT_SUPERPOSE_FORM")); }
// (no override makes a frame that does not fit LDS take the LDS form)
static inline int superpose_form(int env, int64_t n_atoms) {
  if (env == kSuperposeEnvStream) return kSuperposeFormStream;
  return n_atoms <= kSuperposeLdsMaxAtoms ? kSuperposeFormLds : kSuperposeFormStream;
}
static inline size_t superpose_lds_bytes(int64_t n_atoms) {
  return sizeof(double) * (3 * (size_t)n_atoms + kSuperposeRedDoubles);
}
// bytes of HBM traffic per frame (the target, weights and the small outputs left aside): DESIGN section 4
static inline size_t superpose_frame_bytes(int form, int64_t n_atoms) {
  return (form == kSuperposeFormLds ? 2 : 4) * (size_t)24 * (size_t)n_atoms;
}
struct SuperposeBufs { double* target_centre; };   // (cx, cy, cz, sum of the weights)
static inline SuperposeBufs superpose_layout(Arena& a) { return SuperposeBufs{a.take<double>(4)}; }

// ---- mean frame and per-atom mean-square deviation -------------------------------------------------------------------------
// Two-level sum over the frames: level 1 adds chunks of kMeanChunk consecutive frames per coordinate, level 2 the chunks,
// both in ascending order.  The chunk length is fixed, so the bits depend on (M, N) and the data alone.
constexpr int kMeanChunk = 64;
static inline int64_t mean_chunks(int64_t n_frames) { return (n_frames + kMeanChunk - 1) / kMeanChunk; }
struct MeanBufs { double* partial; };   // (chunks, 3 N)
static inline MeanBufs mean_layout(Arena& a, int64_t n_frames, int64_t n_atoms) {
  return MeanBufs{a.take<double>((size_t)mean_chunks(n_frames) * 3 * (size_t)n_atoms)};
}

// ---- pairwise RMSD matrix (rmsd_matrix.hip) ----------------------------------------------------------------------------------
// A workgroup of the product kernel owns kRmsdTile x kRmsdTile frame pairs and stages kRmsdRows atoms at a time.  The
// transposed copy Y (N_pad, 3, M_pad) is padded to both with exact zeros, so the product has no tail code.  (The two are the
// tile of pair_block_tile.h, which asserts so.)
constexpr int kRmsdTile = 64;
constexpr int kRmsdRows = 8;
static inline int64_t rmsd_pad_frames(int64_t n_frames) { return (n_frames + kRmsdTile - 1) / kRmsdTile * kRmsdTile; }
static inline int64_t rmsd_pad_atoms(int64_t n_atoms) { return (n_atoms + kRmsdRows - 1) / kRmsdRows * kRmsdRows; }
// workgroups of the product: the lower triangle of tiles for a self-comparison (n_b = 0), else the rectangle
static inline int64_t rmsd_tiles(int64_t n_a, int64_t n_b) {
  const int64_t ta = rmsd_pad_frames(n_a) / kRmsdTile, tb = rmsd_pad_frames(n_b) / kRmsdTile;
  return n_b == 0 ? ta * (ta + 1) / 2 : ta * tb;
}
struct RmsdBufs {
  double* ya;     // (N_pad, 3, Ma_pad) sqrt(w) times the centred frames of the first ensemble, frame index fastest
  double* ga;     // (Ma_pad) G_f, NaN for a non-finite frame, 0 for a pad frame
  double* yb;     // the same of the second ensemble; a self-comparison takes neither
  double* gb;
  double* wsum;   // (1) W
};
static inline RmsdBufs rmsd_layout(Arena& a, int64_t n_a, int64_t n_b, int64_t n_atoms) {
  const size_t rows = 3 * (size_t)rmsd_pad_atoms(n_atoms);
  const size_t ma = (size_t)rmsd_pad_frames(n_a), mb = (size_t)rmsd_pad_frames(n_b);
  RmsdBufs B{};
  B.ya = a.take<double>(rows * ma);
  B.ga = a.take<double>(ma);
  B.yb = a.take<double>(n_b > 0 ? rows * mb : 0);
  B.gb = a.take<double>(n_b > 0 ? mb : 0);
  B.wsum = a.take<double>(1);
  return B;
}
static inline size_t rmsd_scratch_bytes(int64_t n_a, int64_t n_b, int64_t n_atoms) {
  Arena a;
  rmsd_layout(a, n_a, n_b, n_atoms);
  return a.bytes();
}
// 0: fits; else which rule it breaks.  The sizes are positive here (n_b = 0: self).  The copies must be addressable and the
// tiles fit a grid; the output's own size is the caller's.
static inline int rmsd_shape_error(int64_t n_a, int64_t n_b, int64_t n_atoms) {
  if (n_a <= 0 || n_b < 0 || n_atoms <= 0) return 1;
  if (n_a > 0x7fffffffLL - kRmsdTile || n_b > 0x7fffffffLL - kRmsdTile || n_atoms > 0x7fffffffLL / 3 - kRmsdRows) return 2;
  const long double cells = 3.0L * (long double)rmsd_pad_atoms(n_atoms) * (long double)rmsd_pad_frames(n_a > n_b ? n_a : n_b);
  if (cells > 0x1p58L) return 3;                       // (bytes of one copy stay far inside size_t)
  if (rmsd_tiles(n_a, n_b) > 0x3fffffffLL) return 4;   // (one grid axis, and the triangle decode's int arithmetic)
  return 0;
}

// ---- ensemble PCA ----------------------------------------------------------------------------------------------------------
// Gram route (order M) while M - 1 < 3 N, else the covariance (order 3 N): the smaller symmetric eigenproblem; both have
// the same non-zero spectrum.
constexpr int kPcaGram = 0, kPcaCovariance = 1;
struct PcaPlan {
  int route;
  int64_t order;     // of the symmetric matrix
  int64_t k_len;     // length of the product's K axis: 3 N (Gram) or M (covariance)
  int split_k;       // K slices of the product (1: none)
  bool lower_grid;   // covariance route without slices: only the lower triangle is computed, then mirrored
  bool full;         // n_modes == order: the full-spectrum solver
};
static inline PcaPlan pca_plan(int64_t n_frames, int64_t n_atoms, int64_t n_modes, int num_cus) {
  PcaPlan P{};
  const int64_t n3 = 3 * n_atoms;
  P.route = n_frames - 1 < n3 ? kPcaGram : kPcaCovariance;
  P.order = P.route == kPcaGram ? n_frames : n3;
  P.k_len = P.route == kPcaGram ? n3 : n_frames;
  // K slices where the 64 x 64 tiles of the result leave most of the device idle and K is long (stein.hip's CholQR rule
  // for the slice count)
  const int64_t tiles = ((P.order + 63) / 64) * ((P.order + 63) / 64);
  const int64_t cus = num_cus > 0 ? num_cus : 256;
  P.split_k = tiles < 2 * cus ? (int)std::max<int64_t>(1, std::min<int64_t>(32, P.k_len / 512)) : 1;
  P.lower_grid = P.route == kPcaCovariance && P.split_k == 1;
  P.full = n_modes == P.order;
  return P;
}
struct PcaBufs {
  double* xc;        // (M, 3 N) centred, mass-scaled frames
  double* frame_ss;  // (M) sums of squares of the rows of xc
  double* mat;       // (order, order)
  double* slices;    // (split_k, order, order) when split_k > 1
  double* evals;     // (n_modes) ascending
  double* evecs;     // (n_modes, order)
  double* raw;       // (n_modes, 3 N) expanded, not yet normalised (Gram route)
  char* descs;       // two GEMM records
};
static inline PcaBufs pca_layout(Arena& a, const PcaPlan& P, int64_t n_frames, int64_t n_atoms, int64_t n_modes,
                                 size_t desc_bytes) {
  const size_t n3 = 3 * (size_t)n_atoms, ord = (size_t)P.order;
  PcaBufs B{};
  B.xc = a.take<double>((size_t)n_frames * n3);
  B.frame_ss = a.take<double>((size_t)n_frames);
  B.mat = a.take<double>(ord * ord);
  B.slices = a.take<double>(P.split_k > 1 ? (size_t)P.split_k * ord * ord : 0);
  B.evals = a.take<double>((size_t)n_modes);
  B.evecs = a.take<double>((size_t)n_modes * ord);
  B.raw = a.take<double>(P.route == kPcaGram ? (size_t)n_modes * n3 : 0);
  B.descs = a.take<char>(2 * desc_bytes);
  return B;
}
static inline size_t pca_scratch_bytes(const PcaPlan& P, int64_t n_frames, int64_t n_atoms, int64_t n_modes, size_t desc_bytes) {
  Arena a;
  pca_layout(a, P, n_frames, n_atoms, n_modes, desc_bytes);
  return a.bytes();
}

}  // namespace sc_host
