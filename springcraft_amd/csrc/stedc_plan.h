// The plan of the tridiagonal divide & conquer (stedc.hip): the merge tree, the launch shapes of the kernels of a merge
// level, the layout of the context's auxiliary buffer and which of the ping-pong buffers a level reads and writes.  Same
// form as eigh_policy.h and twostage_policy.h: no HIP, header-only, closed-form functions of integers;
// tests/host_sanitize/test_stedc_plan.cpp compiles exactly this code with g++ -fsanitize=address,undefined.
// stedc_batched builds one DcTree per solve and launches what dc_level_launch says; the kernels carve their LDS through
// dc_setup_carve and the constants below, so a launch and a carve cannot disagree.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "twostage_policy.h"   // SC_POLICY_HD

namespace sc_host {

// ---- the merge tree ---------------------------------------------------------------------------------------------
// A merge joins the solved halves [lo, mid) and [mid, hi); a leaf is the rows [lo, hi) (its mid is not used).
struct DcNode {
  int lo, mid, hi;
};

constexpr int kLeafMax = 32;   // rows of the largest leaf (k_dc_leaves<kLeafMax>: one wave per leaf, a lane per row)

// Every node is halved until no leaf has more than kLeafMax rows: the smallest d with ceil(n / 2^d) <= kLeafMax
inline int dc_depth(int n) {
  int depth = 0;
  while (((n + (1 << depth) - 1) >> depth) > kLeafMax) ++depth;
  return depth;
}
// ... which makes the tree a full one: 2^d leaves and 2^d - 1 merges (what sizes DcLayout::cnt and the merge records)
inline int dc_node_count(int n) { return (2 << dc_depth(n)) - 1; }

struct DcTree {
  std::vector<DcNode> nodes;    // upload order: the leaves, then level 0 (which merges leaves), ..., the root
  int n_leaves = 0;
  std::vector<int> level_off;   // first node of level l in `nodes`; [levels()]: the node count
  std::vector<int> level_maxn;  // rows of the widest node of level l
  int levels() const { return (int)level_maxn.size(); }
  int count() const { return (int)nodes.size(); }
  int level_size(int l) const { return level_off[l + 1] - level_off[l]; }
  const DcNode* level(int l) const { return nodes.data() + level_off[l]; }
  int merges_before(int l) const { return level_off[l] - n_leaves; }   // merges of the levels below l
};

inline DcTree dc_tree(int n) {
  const int depth = dc_depth(n);
  std::vector<std::vector<DcNode>> by_depth(depth + 1);   // segments after 0 .. depth halvings
  by_depth[0].push_back(DcNode{0, n / 2, n});
  for (int dlev = 0; dlev < depth; ++dlev) {
    for (const DcNode& nd : by_depth[dlev]) {
      by_depth[dlev + 1].push_back(DcNode{nd.lo, nd.lo + (nd.mid - nd.lo) / 2, nd.mid});
      by_depth[dlev + 1].push_back(DcNode{nd.mid, nd.mid + (nd.hi - nd.mid) / 2, nd.hi});
    }
  }
  DcTree t;
  t.nodes = by_depth[depth];
  t.n_leaves = (int)t.nodes.size();
  for (int dlev = depth - 1; dlev >= 0; --dlev) {
    t.level_off.push_back(t.count());
    int maxn = 0;
    for (const DcNode& nd : by_depth[dlev]) maxn = std::max(maxn, nd.hi - nd.lo);
    t.level_maxn.push_back(maxn);
    t.nodes.insert(t.nodes.end(), by_depth[dlev].begin(), by_depth[dlev].end());
  }
  t.level_off.push_back(t.count());
  return t;
}

// ---- LDS of the two kernels that keep a merge in it ---------------------------------------------------------------
// The rule: a level whose widest merge has maxN rows keeps the kernel's working set in dynamic LDS while maxN is at most
// the kernel's cap, (bytes per element) * maxN + (fixed part) bytes of it; above the cap the launch asks for no dynamic
// LDS and the kernel works on global memory (use_lds = 0).
// k_dc_setup: the merged order of the two child spectra (dc_setup_carve)
constexpr int kSetupLdsPerElem = 22;
constexpr int kSetupLdsFixed = 32;
constexpr int kLdsCapSetup = 7000;
constexpr int kSetupScratchDoubles = 3;   // above the cap: the same carve in global scratch, this many doubles per row
// k_dc_secular: the poles and the squared weights of a merge (two doubles per pole)
constexpr int kSecularLdsPerPole = 16;
constexpr int kSecularLdsFixed = 16;
constexpr int kLdsCapSecular = 9800;

struct DcSetupCarve {
  double* d;             // pole
  double* z;             // its component of the rank-one vector
  int* col;              // its eigenvector column
  unsigned char* mixed;  // 1: a deflation rotation mixed the column across the two halves
  unsigned char* flag;   // deflation status bits
};
SC_POLICY_HD inline DcSetupCarve dc_setup_carve(double* base, int N) {
  DcSetupCarve c;
  c.d = base;
  c.z = base + N;
  c.col = reinterpret_cast<int*>(base + 2 * N);
  c.mixed = reinterpret_cast<unsigned char*>(c.col + N);
  c.flag = c.mixed + N;
  return c;
}
static_assert(kSetupLdsPerElem == 2 * sizeof(double) + sizeof(int) + 2 * sizeof(unsigned char), "dc_setup_carve");
static_assert(kSetupScratchDoubles * sizeof(double) >= (size_t)kSetupLdsPerElem, "the global carve of a node fits its rows");
static_assert(kSecularLdsPerPole == 2 * sizeof(double), "k_dc_secular keeps dl and z^2");
static_assert((size_t)kLdsCapSetup * kSetupLdsPerElem + kSetupLdsFixed <= kLdsPerWorkgroup, "k_dc_setup's LDS at its cap");
static_assert((size_t)kLdsCapSecular * kSecularLdsPerPole + kSecularLdsFixed <= kLdsPerWorkgroup, "k_dc_secular's LDS at its cap");

// ---- launch shapes of the kernels of one merge level --------------------------------------------------------------
struct DcLaunch {
  unsigned gx = 1, gy = 1, gz = 1;
  int threads = 256;
  size_t lds = 0;         // dynamic LDS bytes
  bool use_lds = false;   // (k_dc_setup, k_dc_secular) the kernel argument of the same name
};
struct DcLevelLaunch {
  DcLaunch zero_offdiag, setup, rotate, secular, zhat, vectors, finalize, copy_deflated;
};
// maxN: rows of the level's widest merge; G: its merges; batch: matrices
inline DcLevelLaunch dc_level_launch(int maxN, int G, int batch) {
  const unsigned g = (unsigned)G, b = (unsigned)batch;
  auto shape = [&](int gx, int threads) {
    DcLaunch s;
    s.gx = (unsigned)gx; s.gy = g; s.gz = b;
    s.threads = threads;
    return s;
  };
  DcLevelLaunch L;
  L.zero_offdiag = shape(std::min(1024, (maxN * maxN / 2 + 255) / 256 + 1), 256);
  // one workgroup per (merge, matrix)
  L.setup.gx = g; L.setup.gy = b;
  L.setup.threads = maxN >= 1024 ? 1024 : (maxN >= 256 ? 256 : 64);
  L.setup.use_lds = maxN <= kLdsCapSetup;
  L.setup.lds = L.setup.use_lds ? (size_t)maxN * kSetupLdsPerElem + kSetupLdsFixed : 0;
  L.rotate = shape((maxN + 255) / 256, 256);   // a thread per row
  // a wave per root
  const int sec_threads = maxN >= 2048 ? 1024 : 256, sec_waves = sec_threads / 64;
  L.secular = shape((maxN + sec_waves - 1) / sec_waves, sec_threads);
  L.secular.use_lds = maxN <= kLdsCapSecular;
  L.secular.lds = L.secular.use_lds ? (size_t)maxN * kSecularLdsPerPole + kSecularLdsFixed : 0;
  L.zhat = shape((maxN + 3) / 4, 256);         // a wave per weight
  L.vectors = shape(maxN, 256);                // a workgroup per root
  L.finalize = shape((maxN + 255) / 256, 256);   // a thread per eigenvalue
  L.copy_deflated = shape(maxN, 256);          // a workgroup per deflated column
  return L;
}

// ---- the context's auxiliary buffer (sc_ctx::dc_aux) during the D&C: byte offsets, every region on a 256-byte boundary ---
struct DcAux {
  size_t nodes = 0;    // DcNode[nodes]: the tree in upload order
  size_t flops = 0;    // 256 spare bytes; profiled solves sum the merge products' flops into the first double
  size_t sorted = 0;   // oversize only: k_dc_setup's carve in global memory, kSetupScratchDoubles * n doubles per matrix
  bool oversize = false;   // n > kLdsCapSetup: the top merges do not fit k_dc_setup's LDS
  size_t total = 0;
};
inline DcAux dc_aux_carve(int nodes, int n, int batch) {
  DcAux A;
  auto take = [&](size_t bytes) { const size_t o = policy_align_up(A.total, 256); A.total = o + bytes; return o; };
  A.nodes = take((size_t)nodes * sizeof(DcNode));
  A.flops = take(256);
  A.oversize = n > kLdsCapSetup;
  if (A.oversize) A.sorted = take((size_t)batch * kSetupScratchDoubles * n * sizeof(double));
  return A;
}

// ---- buffer parity ------------------------------------------------------------------------------------------------
// Stage 0 is what the leaves write, stage l + 1 what level l writes from stage l; stage `nlev` is the result.
// Eigenvectors: true: the caller's output matrix, false: the scratch matrix -- so that the last stage is the caller's
inline bool dc_q_is_out(int nlev, int stage) { return (nlev - stage) % 2 == 0; }
// Eigenvalues: slot 0 / 1 = DcLayout::w0 / w1 (k_dc_unscale reads the slot of stage nlev)
inline int dc_w_slot(int stage) { return stage % 2; }

}  // namespace sc_host
