// The host decisions of the device Cholesky solver (potrf.hip) and of the subsystem reduction on it (subsystem.hip): the
// block plan of a factorisation, the steps of a triangular solve, the number and shapes of the GEMM records per step and the
// layout of the scratch.  Same rules as gemm_policy.h / ensemble_policy.h: closed-form functions of their inputs, no HIP,
// header-only; tests/host_sanitize/test_potrf_policy.cpp compiles exactly this code with g++ -fsanitize=address,undefined.
//
// Factorisation A = L L^T (lower, in place), two levels.  The inner level walks diagonal blocks of kPotrfInner columns: the
// block is factored and inverted by one workgroup (k_diag_block), the panel below it is multiplied by the inverse (one GEMM
// into a side buffer, then a copy back) and the columns up to the end of the OUTER block are updated with that panel
// (K = kPotrfInner, a short-K product on few columns).  At the end of an outer block of potrf_outer_block(n) columns the
// whole trailing matrix is updated once with K = the outer block, the lower_grid SYRK form.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "scratch_arena.h"

namespace sc_host {

constexpr int kPotrfInner = 64;   // columns of a diagonal block: k_diag_block holds it in LDS (64 x 65 doubles)
constexpr int kPotrsForward = 0, kPotrsBackward = 1, kPotrsBoth = 2;   // sc_dev_potrs_f64's mode
constexpr int64_t kPotrfMaxOrder = 0x7fffffffLL / 2;   // (GEMM records carry int sizes)

// Columns of an outer block: a multiple of kPotrfInner.  `env`: SPRINGCRAFT_POTRF_OUTER (0: unset), for the sweep of
// tools/subsystem_timing.py; rounded down to a multiple of the inner block, at least one of them.
// The default is the best of the sweep on an MI355X at n = 12000 (profiles/subsystem.txt: 64 / 128 / 256 / 384 / 512 / 1024
// columns: 44.7 / 38.6 / 35.5 / 34.8 / 34.5 / 35.2 ms): wider blocks give the trailing update a longer K, narrower ones leave
// less of the matrix to the short-K updates inside the block.  Other orders were not swept; one size for all of them keeps
// the rule trivial, and a matrix below 512 rows is one outer block.
constexpr int kPotrfOuter = 512;
static inline int potrf_outer_block(int64_t n, int env) {
  (void)n;
  if (env > 0) return std::max(kPotrfInner, env / kPotrfInner * kPotrfInner);
  return kPotrfOuter;
}
static inline int64_t potrf_blocks(int64_t n) { return (n + kPotrfInner - 1) / kPotrfInner; }

// ---- the steps of a factorisation ---------------------------------------------------------------------------------------
constexpr int kPotrfDiag = 0, kPotrfPanel = 1, kPotrfUpdate = 2;
struct PotrfOp {
  int kind;
  int c, w;      // Diag / Panel: first column and width of the diagonal block.  Update: first column and count of the K range
  int r0, rows;  // Panel / Update: first row and number of rows (r0 + rows = n)
  int cols;      // Update: columns r0 .. r0 + cols - 1 are updated (lower part); cols == rows: the lower_grid form
};
// Diag: one workgroup per matrix.  Panel: one GEMM record per matrix, (rows, w) = A[r0:, c:c+w] inv(L_cc)^T, and a copy.
// Update: one GEMM record per matrix, A[r0:, r0:r0+cols] -= A[r0:, c:c+w] A[r0:r0+cols, c:c+w]^T, lower_only.
static inline std::vector<PotrfOp> potrf_plan(int64_t n64, int outer) {
  std::vector<PotrfOp> ops;
  const int n = (int)n64;
  for (int j0 = 0; j0 < n; j0 += outer) {
    const int jend = std::min(n, j0 + outer);
    for (int c = j0; c < jend; c += kPotrfInner) {
      const int w = std::min(kPotrfInner, n - c), r0 = c + w;
      ops.push_back({kPotrfDiag, c, w, 0, 0, 0});
      if (r0 >= n) continue;
      ops.push_back({kPotrfPanel, c, w, r0, n - r0, 0});
      if (r0 < jend) ops.push_back({kPotrfUpdate, c, w, r0, n - r0, jend - r0});
    }
    if (jend < n) ops.push_back({kPotrfUpdate, j0, jend - j0, jend, n - jend, n - jend});
  }
  return ops;
}
static inline size_t potrf_record_count(const std::vector<PotrfOp>& ops, int64_t batch) {
  size_t r = 0;
  for (const PotrfOp& o : ops) r += o.kind == kPotrfDiag ? 0 : (size_t)batch;
  return r;
}

// ---- the steps of a triangular solve with the factor ----------------------------------------------------------------------
// Left solves on an (n, q) column-major right-hand side, block by block with the inverted diagonal blocks:
//   forward  L Y = B:    blocks ascending,  T = inv(L_kk) B_k,    B_k <- T,  B[below] -= L[below, k] T
//   backward L^T X = Y:  blocks descending, T = inv(L_kk)^T B_k,  B_k <- T,  B[above] -= L[k, above]^T T
// Right solve X L^T = B on a (rows, n) column-major B (the reduction's Y^T = H_se L^-T), blocks ascending:
//   T = B[:, k] inv(L_kk)^T,  B[:, k] <- T,  B[:, after] -= T L[after, k]^T
// Every block step is two GEMM records per matrix (the second one is absent at the last block) and one copy.
struct TrsmStep { int c, w, rest0, rest; };   // diagonal block, and the rows / columns the second product updates
static inline std::vector<TrsmStep> trsm_steps(int64_t n64, bool ascending) {
  std::vector<TrsmStep> s;
  const int n = (int)n64, nb = (int)potrf_blocks(n64);
  for (int t = 0; t < nb; ++t) {
    const int k = ascending ? t : nb - 1 - t;
    const int c = k * kPotrfInner, w = std::min(kPotrfInner, n - c);
    if (ascending) s.push_back({c, w, c + w, n - c - w});
    else s.push_back({c, w, 0, c});
  }
  return s;
}
static inline size_t trsm_record_count(int64_t n, int64_t batch) { return 2 * (size_t)potrf_blocks(n) * (size_t)batch; }

// ---- scratch -------------------------------------------------------------------------------------------------------------------
struct PotrfBufs {
  double* dinv;    // (batch, blocks, 64, 64) column-major inverses of the diagonal blocks, strict upper triangle 0
  double* panel;   // (batch, n, 64): the panel product before it is copied back
  char* descs;     // the GEMM records of all steps
};
static inline PotrfBufs potrf_layout(Arena& a, int64_t n, int64_t batch, size_t records, size_t desc_bytes) {
  PotrfBufs B{};
  B.dinv = a.take<double>((size_t)batch * (size_t)potrf_blocks(n) * kPotrfInner * kPotrfInner);
  B.panel = a.take<double>((size_t)batch * (size_t)n * kPotrfInner);
  B.descs = a.take<char>(records * desc_bytes);
  return B;
}
struct TrsmBufs {
  double* dinv;    // as PotrfBufs::dinv, recomputed from the factor
  double* tmp;     // (batch, 64, q) left solves / (batch, rows, 64) right solve: T of one block step
  char* descs;
};
// `vectors`: q of a left solve, rows of a right solve; passes: 1, or 2 for kPotrsBoth
static inline TrsmBufs trsm_layout(Arena& a, int64_t n, int64_t batch, int64_t vectors, int passes, size_t desc_bytes) {
  TrsmBufs B{};
  B.dinv = a.take<double>((size_t)batch * (size_t)potrf_blocks(n) * kPotrfInner * kPotrfInner);
  B.tmp = a.take<double>((size_t)batch * (size_t)vectors * kPotrfInner);
  B.descs = a.take<char>((size_t)passes * trsm_record_count(n, batch) * desc_bytes);
  return B;
}
// what sc_dev_potrf_workspace reports: the larger of a factorisation's and a one-vector `both` solve's scratch
static inline size_t potrf_scratch_bytes(int64_t n, int64_t batch, int outer, size_t desc_bytes) {
  Arena f, s;
  potrf_layout(f, n, batch, potrf_record_count(potrf_plan(n, outer), batch), desc_bytes);
  trsm_layout(s, n, batch, 1, 2, desc_bytes);
  return std::max(f.bytes(), s.bytes());
}

// ---- the subsystem reduction: potrf(H_ee), Y^T = H_se L^-T, H_eff = H_ss - Y^T Y --------------------------------------------
// (the reduction's own scratch is batch_reduce_layout below, for one structure as for many)
struct FollowBufs {
  TrsmBufs trsm;
  char* desc;
};
static inline FollowBufs follow_layout(Arena& a, int64_t me, int64_t q, size_t desc_bytes) {
  FollowBufs B{};
  B.trsm = trsm_layout(a, me, 1, q, 1, desc_bytes);
  B.desc = a.take<char>(desc_bytes);
  return B;
}
// flops of a reduction: me^3 / 3 + me^2 ms + me ms^2
static inline double reduce_flops(double me, double ms) { return me * me * me / 3.0 + me * me * ms + me * ms * ms; }

// ---- the batched reduction: B members with one system size and environments of different size in slots of one order -----------
// One member of the packed inputs (coordinates, LOCAL pair indices, gamma, row starts, group / pos back to back).  Atom a of
// the member is packed atom atom0 + a; its n_atoms + 1 row starts are at atom0 + (the member's number) and count from the
// member's own first pair, which is packed pair pair0.
struct SubMember {
  int64_t atom0, n_atoms, pair0, n_pairs, n_e;
};
constexpr int64_t kSubBatchMax = 65535;   // (the member is a grid's y index, as the matrix of a batched factorisation)

// Order of the environment slot.  env_order atoms per slot; a member with fewer gets diag(H_ee, I).
static inline int64_t sub_slot_order(int dim, int64_t env_order) { return (int64_t)dim * env_order; }
// 0 when the shapes can be launched, else the number of the rule they break (api_potrf.hip turns it into a message):
// 1 dim, 2 n_s, 3 batch, 4 env_order, 5 an order above the solver's limit
static inline int sub_batch_shape_error(int dim, int64_t n_s, int64_t env_order, int64_t batch) {
  if (dim != 1 && dim != 3) return 1;
  if (n_s < 1) return 2;
  if (batch < 1 || batch > kSubBatchMax) return 3;
  if (env_order < 0) return 4;
  if (n_s > kPotrfMaxOrder / 3 || env_order > kPotrfMaxOrder / 3) return 5;
  return 0;
}
// -1 when every member fits its slot, else the first member that does not: n_e outside 0 .. env_order, n_s + n_e != n_atoms,
// a negative pair count, or offsets that do not follow the member before (the arrays are packed back to back)
static inline int64_t sub_batch_member_error(const SubMember* mem, int64_t batch, int64_t n_s, int64_t env_order) {
  int64_t atom0 = 0, pair0 = 0;
  for (int64_t b = 0; b < batch; ++b) {
    const SubMember& m = mem[b];
    if (m.n_e < 0 || m.n_e > env_order || m.n_atoms != n_s + m.n_e || m.n_pairs < 0) return b;
    if (m.atom0 != atom0 || m.pair0 != pair0) return b;
    atom0 += m.n_atoms;
    pair0 += m.n_pairs;
  }
  return -1;
}
// the x extent of the two assembly grids: the longest pair list, and every atom of a member plus its slot's pad atoms
static inline int64_t sub_batch_max_pairs(const SubMember* mem, int64_t batch) {
  int64_t k = 0;
  for (int64_t b = 0; b < batch; ++b) k = std::max(k, mem[b].n_pairs);
  return k;
}
static inline int64_t sub_batch_atom_threads(int64_t n_s, int64_t env_order) { return n_s + env_order; }

struct BatchBlocksBufs {
  char* members;   // (batch) SubMember
};
static inline BatchBlocksBufs batch_blocks_layout(Arena& a, int64_t batch) {
  BatchBlocksBufs B{};
  B.members = a.take<char>((size_t)batch * sizeof(SubMember));
  return B;
}
struct BatchReduceBufs {
  PotrfBufs potrf;
  TrsmBufs trsm;
  char* descs;   // (batch) records of the H_eff products
};
// me = sub_slot_order(...) > 0.  A single structure reduces with batch = 1: the carve is then potrf_layout(me, 1, ...),
// trsm_layout(me, 1, ms, 1, ...) and one record, take for take.
static inline BatchReduceBufs batch_reduce_layout(Arena& a, int64_t me, int64_t ms, int64_t batch, int outer, size_t desc_bytes) {
  BatchReduceBufs B{};
  B.potrf = potrf_layout(a, me, batch, potrf_record_count(potrf_plan(me, outer), batch), desc_bytes);
  B.trsm = trsm_layout(a, me, batch, ms, 1, desc_bytes);
  B.descs = a.take<char>((size_t)batch * desc_bytes);
  return B;
}
// what sc_dev_vsa_batch_workspace reports: the reduction's scratch, 0 for env_order = 0 (there is no reduction)
static inline size_t batch_reduce_scratch_bytes(int64_t me, int64_t ms, int64_t batch, int outer, size_t desc_bytes) {
  if (me == 0) return 0;
  Arena a;
  batch_reduce_layout(a, me, ms, batch, outer, desc_bytes);
  return a.bytes();
}
// flops the pad adds to member b's reduction: what a slot of order me costs beyond the member's own me_b
static inline double reduce_pad_flops(double me, double me_b, double ms) { return reduce_flops(me, ms) - reduce_flops(me_b, ms); }

}  // namespace sc_host
