// The host decisions of the correlation-network entries (corr_network.hip, api_network.hip): tile and round counts of the
// blocked Floyd-Warshall, the sizes the kernels can index, and the layout of the path-usage workspace.  Same rules as
// gemm_policy.h: closed-form functions of their inputs, no HIP, header-only.
#pragma once
#include <cstdint>

#include "scratch_arena.h"

namespace sc_host {

// A member's record, three int64 on the device: n_b, the element offset of its (n_b, n_b) row-major block in the packed
// pair buffers, and the index of its first atom in the packed per-atom buffers.
constexpr int kNetRecInts = 3;

constexpr int kNetTile = 64;   // side of a Floyd-Warshall tile
// Largest member: the tiles of one round are one grid axis (T^2 <= 2^24) and a next hop is an int32.
constexpr int64_t kNetMaxN = 262144;
// Largest member of the path-usage walk: a target's column of next hops and its counters, 2 x 4 n bytes, stay in the
// 64 KB of LDS a kernel gets without raising its limit.
constexpr int64_t kNetUsageMaxN = 8192;
constexpr int64_t kNetMaxMembers = 65535;   // members are grid axis y

static inline int64_t net_tiles(int64_t n) { return (n + kNetTile - 1) / kNetTile; }
// launches of one shortest-path solve: init, three per round, the final pass
static inline int64_t net_path_launches(int64_t n_max) { return 2 + 3 * net_tiles(n_max); }
// add + min operations of one member's solve, the model the measured times are set against
static inline double net_path_ops(int64_t n) { return 2.0 * (double)n * (double)n * (double)n; }
static inline size_t net_usage_lds_bytes(int64_t n_max) { return 2 * sizeof(int32_t) * (size_t)n_max; }

// 0: fits; else which rule it breaks
static inline int net_shape_error(int64_t count, int64_t n_max) {
  if (count < 1 || n_max < 1) return 1;
  if (count > kNetMaxMembers) return 2;
  if (n_max > kNetMaxN) return 3;
  return 0;
}

struct NetUsageBufs { int32_t* through; };   // packed like the pair buffers: row t of member b = counts of the paths that end in t
static inline NetUsageBufs net_usage_layout(Arena& a, int64_t total_sq) {
  return NetUsageBufs{a.take<int32_t>((size_t)total_sq)};
}
static inline size_t net_usage_scratch_bytes(int64_t total_sq) {
  Arena a;
  net_usage_layout(a, total_sq);
  return a.bytes();
}

}  // namespace sc_host
