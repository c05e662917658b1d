// Host-only logic of the clustering entries (springcraft_amd/csrc/cluster_policy.h, scratch_arena.h) under AddressSanitizer
// + UBSan:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I springcraft_amd/csrc \
//       tests/host_sanitize/test_cluster_policy.cpp -o /tmp/test_cluster_policy && /tmp/test_cluster_policy
// (built and run by tests/test_cluster_host.py::test_cluster_policy_under_sanitizers).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cluster_policy.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); std::exit(1); } } while (0)

using namespace sc_host;

// every region lies inside the block, 256-aligned, after the one before it, and can be written end to end
struct Walk {
  char* base;
  size_t size;
  char* at;
  template <typename T>
  void region(T* p, size_t count) {
    CHECK(p != nullptr);
    char* c = reinterpret_cast<char*>(p);
    CHECK(c >= at && (size_t)(c - base) % 256 == 0);
    CHECK(c + sizeof(T) * count <= base + size);
    for (size_t i = 0; i < count; ++i) p[i] = T(1);
    at = c + (count ? sizeof(T) * count : 1);
  }
};

static void carve(int64_t n, int64_t k) {
  const size_t bytes = cluster_workspace_bytes(n, k);
  std::vector<char> block(bytes);
  Arena a(block.data(), block.size());
  const ClusterBufs B = cluster_layout(a, n, k);
  CHECK(!a.overrun() && a.bytes() == bytes);
  const size_t N = (size_t)n, K = (size_t)k, W = (size_t)cluster_words(n);
  Walk w{block.data(), block.size(), block.data()};
  w.region(B.ctl, kClusterCtlInts);
  w.region(B.valid, W);
  if (k == 0) {
    w.region(B.alive, W);
    w.region(B.members, W);
    w.region(B.count, N);
    w.region(B.adj, N * W);
    CHECK(!B.medoid && !B.order && !B.loss);
  } else {
    w.region(B.medoid, K);
    w.region(B.is_medoid, N);
    w.region(B.nearest, N);
    w.region(B.dn, N);
    w.region(B.ds, N);
    w.region(B.gain, N);
    w.region(B.best_slot, N);
    w.region(B.order, N);
    w.region(B.seg, K + 1);
    w.region(B.dn_o, N);
    w.region(B.ds_o, N);
    w.region(B.loss, K);
    w.region(B.seg_dn, K);
    CHECK(!B.adj && !B.alive && !B.count);
  }
  // one byte short: the carve reports the overrun and hands out no pointer past the end
  Arena s(block.data(), block.size() - 1);
  cluster_layout(s, n, k);
  CHECK(s.overrun());
}

int main() {
  // words of a row of the bit matrix around the 64-bit edges
  CHECK(cluster_words(1) == 1 && cluster_words(63) == 1 && cluster_words(64) == 1 && cluster_words(65) == 2);
  CHECK(cluster_words(128) == 2 && cluster_words(129) == 3 && cluster_words(10000) == 157 && cluster_words(kClusterMaxN) == 4096);
  CHECK(cluster_adj_bytes(10000) == (size_t)10000 * 157 * 8 && cluster_adj_bytes(64) == 512 && cluster_adj_bytes(65) == 65 * 16);
  CHECK(cluster_adj_bytes(kClusterMaxN) == (size_t)kClusterMaxN * 4096 * 8);   // (8 GiB: beyond 32 bits)

  // limits
  CHECK(cluster_shape_error(1, 0) == 0 && cluster_shape_error(1, 1) == 0 && cluster_shape_error(kClusterMaxN, kClusterMaxK) == 0);
  CHECK(cluster_shape_error(0, 0) == 1 && cluster_shape_error(-5, 1) == 1 && cluster_shape_error(5, -1) == 1);
  CHECK(cluster_shape_error(kClusterMaxN + 1, 0) == 2 && cluster_shape_error(INT64_MAX, 3) == 2);
  CHECK(cluster_shape_error(5, 6) == 3 && cluster_shape_error(5000, kClusterMaxK + 1) == 3 && cluster_shape_error(5, 5) == 0);

  // the form of the evaluation: the row and two doubles per slot inside 64 KB less the reduction buffers
  for (int env : {kClusterEnvAuto, kClusterEnvLds}) {
    CHECK(cluster_form(env, 1, 1) == kClusterFormLds && cluster_form(env, 2000, 100) == kClusterFormLds);
    CHECK(cluster_form(env, 8062, 1) == kClusterFormLds && cluster_form(env, 8063, 1) == kClusterFormStream);
    CHECK(cluster_form(env, 6016, 1024) == kClusterFormLds && cluster_form(env, 6017, 1024) == kClusterFormStream);
    CHECK(cluster_form(env, 10000, 10) == kClusterFormStream);
  }
  CHECK(cluster_form(kClusterEnvStream, 1, 1) == kClusterFormStream && cluster_form(kClusterEnvStream, 10000, 10) == kClusterFormStream);
  CHECK(cluster_eval_lds_bytes(kClusterFormLds, 2000, 100) == 8 * 2200 && cluster_eval_lds_bytes(kClusterFormStream, 2000, 100) == 1600);
  for (int64_t n : {1, 64, 2000, 8062, 6016})
    for (int64_t k : {1, 7, 1024})
      if (k <= n && cluster_form(kClusterEnvAuto, n, k) == kClusterFormLds)
        CHECK(cluster_eval_lds_bytes(kClusterFormLds, n, k) + kClusterEvalStatic <= kClusterLdsLimit);
  CHECK(cluster_eval_lds_bytes(kClusterFormStream, kClusterMaxN, kClusterMaxK) + kClusterEvalStatic <= kClusterLdsLimit);
  CHECK(parse_cluster_env(nullptr) == kClusterEnvAuto && parse_cluster_env("") == kClusterEnvAuto);
  CHECK(parse_cluster_env("auto") == kClusterEnvAuto && parse_cluster_env("lds") == kClusterEnvLds);
  CHECK(parse_cluster_env("stream") == kClusterEnvStream && parse_cluster_env("Stream") == kClusterEnvAuto);

  // workspace carves
  for (int64_t n : {1, 2, 63, 64, 65, 130, 200, 1000})
    for (int64_t k : {0, 1, 2, 7, 64, 1000})
      if (k <= n) carve(n, k);
  // sizes in closed form: the regions in order, each from the next multiple of 256
  {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    size_t off = 0;
    for (size_t r : {(size_t)16, (size_t)8 * 3, (size_t)8 * 3, (size_t)8 * 3, (size_t)4 * 130, (size_t)8 * 130 * 3}) off = up(off) + r;
    CHECK(cluster_workspace_bytes(130, 0) == off);
  }
  // the largest sizes measure without overflow
  CHECK(cluster_workspace_bytes(kClusterMaxN, 0) > cluster_adj_bytes(kClusterMaxN));
  CHECK(cluster_workspace_bytes(kClusterMaxN, kClusterMaxK) > 8 * (size_t)kClusterMaxN * 5);
  std::printf("cluster policy ok\n");
  return 0;
}
