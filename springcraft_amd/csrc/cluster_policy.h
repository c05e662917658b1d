// The host decisions of the clustering entries (cluster.hip, api_cluster.hip): the sizes the kernels can index, the words of
// the neighbour bit matrix, which form the k-medoids evaluation takes, and the layout of the caller-owned workspace that
// holds a run's state between calls.  Same rules as network_policy.h: closed-form functions of their inputs, no HIP,
// header-only; tests/host_sanitize/test_cluster_policy.cpp compiles exactly this code with g++ -fsanitize=address,undefined.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "scratch_arena.h"

namespace sc_host {

// Largest matrix: an item is an int32, a row is one workgroup of a grid axis, and n^2 doubles stay far inside int64.
constexpr int64_t kClusterMaxN = 262144;
// Most medoids: the per-slot sums of one candidate row are held in LDS (2 x 8 k bytes).
constexpr int64_t kClusterMaxK = 1024;

// The status a run keeps on the device, four int32, the only thing the host reads during a run:
//   [0] neighbour-count: items still alive; k-medoids: 1 while SWAP may still improve, 0 once it has converged
//   [1] neighbour-count: clusters made; k-medoids: swaps accepted
//   [2] 1: a NaN between two valid items, no result is defined
//   [3] k-medoids: medoids placed by BUILD (min(k, valid items)); neighbour-count: 0
constexpr int kClusterStatusInts = 4;
// Internal control words beside it in the workspace: [0] the launches that follow a pick / swap have work to do,
// [1] medoids placed so far.
constexpr int kClusterCtlInts = 4;

// 64-bit words of one row of the bit matrix, of the validity and alive sets and of a round's member set
static inline int64_t cluster_words(int64_t n) { return (n + 63) / 64; }
// bytes of the bit matrix, what a neighbour-count round reads at most
static inline size_t cluster_adj_bytes(int64_t n) { return sizeof(uint64_t) * (size_t)n * (size_t)cluster_words(n); }

// 0: fits; else which rule it breaks.  k = 0: neighbour-count clustering; k >= 1: k-medoids with k medoids.
static inline int cluster_shape_error(int64_t n, int64_t k) {
  if (n < 1 || k < 0) return 1;
  if (n > kClusterMaxN) return 2;
  if (k > kClusterMaxK || k > n) return 3;
  return 0;
}

// ---- k-medoids evaluation: one workgroup per candidate row --------------------------------------------------------------
// LDS form: the row (n doubles) is read once, coalesced, into dynamic LDS and gathered from there in segment order; the
// streaming form gathers dist[x, order[t]] from global memory.  Both add the same numbers in the same order.  Beside the
// row both hold two doubles per slot.  The LDS form is taken while all of it fits the 64 KB a kernel gets without raising
// its limit.
constexpr int kClusterFormLds = 0, kClusterFormStream = 1;
constexpr size_t kClusterLdsLimit = 65536;
constexpr size_t kClusterEvalStatic = 1024;   // the workgroup's reduction buffers
static inline size_t cluster_eval_lds_bytes(int form, int64_t n, int64_t k) {
  return sizeof(double) * ((form == kClusterFormLds ? (size_t)n : 0) + 2 * (size_t)k);
}
// SPRINGCRAFT_CLUSTER_FORM: unset / "auto": by size; "lds": the LDS form wherever the row fits; "stream": always the
// streaming form.  Read at every call (a test switches it between two calls of one process).
constexpr int kClusterEnvAuto = 0, kClusterEnvLds = 1, kClusterEnvStream = 2;
static inline int parse_cluster_env(const char* e) {
  if (!e || !*e || !std::strcmp(e, "auto")) return kClusterEnvAuto;
  if (!std::strcmp(e, "lds")) return kClusterEnvLds;
  if (!std::strcmp(e, "stream")) return kClusterEnvStream;
  return kClusterEnvAuto;
}
static inline int read_cluster_env() { return parse_cluster_env(std::getenv("SPRINGCRAFT_CLUSTER_FORM")); }
// (no override makes a row that does not fit LDS take the LDS form)
static inline int cluster_form(int env, int64_t n, int64_t k) {
  if (env == kClusterEnvStream) return kClusterFormStream;
  return cluster_eval_lds_bytes(kClusterFormLds, n, k) + kClusterEvalStatic <= kClusterLdsLimit ? kClusterFormLds
                                                                                                 : kClusterFormStream;
}

// ---- the workspace ---------------------------------------------------------------------------------------------------------
struct ClusterBufs {
  int32_t* ctl;        // (kClusterCtlInts)
  uint64_t* valid;     // (words) bit j: dist[j, j] is not NaN
  // neighbour-count
  uint64_t* alive;     // (words) valid items without a label yet
  uint64_t* members;   // (words) R of the round: adj[centre] & alive
  int32_t* count;      // (n) alive neighbours of every item
  uint64_t* adj;       // (n, words) bit j of row i: dist[i, j] <= cutoff, j valid
  // k-medoids
  int32_t* medoid;     // (k) item of every slot
  int32_t* is_medoid;  // (n)
  int32_t* nearest;    // (n) slot of the nearest medoid, -1 for an invalid item
  double* dn;          // (n) distance to the nearest and
  double* ds;          // (n) to the second-nearest medoid
  double* gain;        // (n) BUILD: gain of every candidate; SWAP: the best delta of its row
  int32_t* best_slot;  // (n) SWAP: the slot of that delta
  int32_t* order;      // (n) valid items grouped by nearest slot, ascending index within a slot
  int32_t* seg;        // (k + 1) offsets of the slots' segments in order
  double* dn_o;        // (n) dn and
  double* ds_o;        // (n) ds in that order
  double* loss;        // (k) sum over a slot's items of ds - dn
  double* seg_dn;      // (k) sum over a slot's items of dn
};
static inline ClusterBufs cluster_layout(Arena& a, int64_t n, int64_t k) {
  const size_t N = (size_t)n, K = (size_t)k, W = (size_t)cluster_words(n);
  ClusterBufs B{};
  B.ctl = a.take<int32_t>(kClusterCtlInts);
  B.valid = a.take<uint64_t>(W);
  if (k == 0) {
    B.alive = a.take<uint64_t>(W);
    B.members = a.take<uint64_t>(W);
    B.count = a.take<int32_t>(N);
    B.adj = a.take<uint64_t>(N * W);
  } else {
    B.medoid = a.take<int32_t>(K);
    B.is_medoid = a.take<int32_t>(N);
    B.nearest = a.take<int32_t>(N);
    B.dn = a.take<double>(N);
    B.ds = a.take<double>(N);
    B.gain = a.take<double>(N);
    B.best_slot = a.take<int32_t>(N);
    B.order = a.take<int32_t>(N);
    B.seg = a.take<int32_t>(K + 1);
    B.dn_o = a.take<double>(N);
    B.ds_o = a.take<double>(N);
    B.loss = a.take<double>(K);
    B.seg_dn = a.take<double>(K);
  }
  return B;
}
static inline size_t cluster_workspace_bytes(int64_t n, int64_t k) {
  Arena a;
  cluster_layout(a, n, k);
  return a.bytes();
}

}  // namespace sc_host
