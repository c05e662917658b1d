// The plan of the tridiagonal divide & conquer (springcraft_amd/csrc/stedc_plan.h) under AddressSanitizer + UBSan:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I springcraft_amd/csrc \
//       tests/host_sanitize/test_stedc_plan.cpp -o /tmp/test_stedc_plan && /tmp/test_stedc_plan
// (built and run by tests/test_abi_and_host.py::test_stedc_plan_under_sanitizers).  The tree is checked by its properties
// at every order and against literals; the launch shapes are literals written out by hand from the rules in words:
//   k_dc_setup    64 threads below 256 rows, 256 below 1024, else 1024; 22 bytes of LDS per row + 32 up to 7000 rows
//   k_dc_secular  256 threads (4 waves) below 2048 rows, else 1024 (16 waves), a wave per root; 16 bytes per pole + 16 up
//                 to 9800 rows
//   the others    256 threads; per row (rotate, finalize), per wave (zhat), per workgroup (vectors, copy_deflated)
// The node counts are those dc_max_nodes(n, 32) of the revision before the plan header returned (taken from that revision's
// library on the host).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "stedc_plan.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); std::exit(1); } } while (0)

using namespace sc_host;

static bool same(const DcNode& a, int lo, int mid, int hi) { return a.lo == lo && a.mid == mid && a.hi == hi; }

static void check_tree(int n, int want_nodes) {
  const DcTree t = dc_tree(n);
  CHECK(t.count() == want_nodes && dc_node_count(n) == want_nodes);
  // the depth is the smallest d with ceil(n / 2^d) <= 32
  int d = 0;
  while ((n + (1LL << d) - 1) / (1LL << d) > 32) ++d;
  CHECK(t.levels() == d && dc_depth(n) == d);
  CHECK(t.n_leaves == (1 << d) && t.count() == (2 << d) - 1);
  CHECK((int)t.level_off.size() == d + 1 && t.level_off[d] == t.count());
  CHECK(t.merges_before(0) == 0 && t.merges_before(d) == t.count() - t.n_leaves);
  // the leaves partition [0, n) in order, none above 32 rows
  int at = 0;
  for (int i = 0; i < t.n_leaves; ++i) {
    CHECK(t.nodes[i].lo == at && t.nodes[i].hi - t.nodes[i].lo <= kLeafMax && t.nodes[i].hi >= t.nodes[i].lo);
    at = t.nodes[i].hi;
  }
  CHECK(at == n);
  // the halves of merge g of level l are nodes 2g and 2g + 1 of the level below (level 0: the leaves)
  for (int l = 0; l < d; ++l) {
    CHECK(t.level_off[l] == t.n_leaves + (1 << d) - (1 << (d - l)));   // levels follow the leaves, bottom up
    CHECK(t.level_size(l) == (1 << (d - 1 - l)));
    const DcNode* below = l == 0 ? t.nodes.data() : t.level(l - 1);
    int maxn = 0;
    for (int g = 0; g < t.level_size(l); ++g) {
      const DcNode& nd = t.level(l)[g];
      CHECK(below[2 * g].lo == nd.lo && below[2 * g].hi == nd.mid);
      CHECK(below[2 * g + 1].lo == nd.mid && below[2 * g + 1].hi == nd.hi);
      CHECK(nd.lo < nd.mid && nd.mid < nd.hi);
      maxn = nd.hi - nd.lo > maxn ? nd.hi - nd.lo : maxn;
    }
    CHECK(t.level_maxn[l] == maxn);
  }
  CHECK(same(t.nodes.back(), 0, n / 2, n));   // the root (n <= 32: the one leaf)
  if (d > 0) CHECK(t.level_maxn[d - 1] == n);
}

// threads, LDS bytes and use_lds of the two kernels with a table
static void check_shape(int maxN, int setup_threads, size_t setup_lds, bool setup_use, int sec_threads, unsigned sec_gx,
                        size_t sec_lds, bool sec_use) {
  const int G = 3, batch = 5;
  const DcLevelLaunch L = dc_level_launch(maxN, G, batch);
  CHECK(L.setup.threads == setup_threads && L.setup.lds == setup_lds && L.setup.use_lds == setup_use);
  CHECK(L.setup.gx == 3 && L.setup.gy == 5 && L.setup.gz == 1);
  CHECK(L.secular.threads == sec_threads && L.secular.lds == sec_lds && L.secular.use_lds == sec_use);
  CHECK(L.secular.gx == sec_gx && L.secular.gy == 3 && L.secular.gz == 5);
  for (const DcLaunch* s : {&L.zero_offdiag, &L.rotate, &L.zhat, &L.vectors, &L.finalize, &L.copy_deflated})
    CHECK(s->threads == 256 && s->lds == 0 && !s->use_lds && s->gy == 3 && s->gz == 5);
  CHECK(L.rotate.gx == (unsigned)(maxN + 255) / 256 && L.finalize.gx == L.rotate.gx);
  CHECK(L.zhat.gx == (unsigned)(maxN + 3) / 4);
  CHECK(L.vectors.gx == (unsigned)maxN && L.copy_deflated.gx == (unsigned)maxN);
  CHECK(L.setup.lds <= 160 * 1024 && L.secular.lds <= 160 * 1024);
  // the carve of the widest merge ends where the per-row bytes say
  std::vector<double> buf((size_t)maxN * 3);
  const DcSetupCarve c = dc_setup_carve(buf.data(), maxN);
  CHECK((char*)c.z == (char*)buf.data() + 8 * (size_t)maxN && (char*)c.col == (char*)buf.data() + 16 * (size_t)maxN);
  CHECK((char*)c.mixed == (char*)buf.data() + 20 * (size_t)maxN && (char*)c.flag == (char*)buf.data() + 21 * (size_t)maxN);
  CHECK((size_t)((char*)(c.flag + maxN) - (char*)buf.data()) == (size_t)maxN * 22);
  c.flag[maxN - 1] = 1;   // (inside the 3 doubles per row of the global form)
}

int main() {
  static_assert(kLeafMax == 32, "the literals below are for leaves of at most 32 rows");

  // ---- the tree
  check_tree(1, 1);
  check_tree(2, 1);
  check_tree(31, 1);
  check_tree(32, 1);
  check_tree(33, 3);
  check_tree(64, 3);
  check_tree(65, 7);
  check_tree(130, 15);
  check_tree(1000, 63);
  check_tree(6000, 511);
  check_tree(7001, 511);
  check_tree(24000, 2047);
  {
    const DcTree t = dc_tree(32);
    CHECK(t.n_leaves == 1 && t.levels() == 0 && same(t.nodes[0], 0, 16, 32));
  }
  {
    const DcTree t = dc_tree(33);
    CHECK(t.n_leaves == 2 && t.levels() == 1 && t.count() == 3);
    CHECK(same(t.nodes[0], 0, 8, 16) && same(t.nodes[1], 16, 24, 33) && same(t.nodes[2], 0, 16, 33));
    CHECK(t.level_off[0] == 2 && t.level_off[1] == 3 && t.level_maxn[0] == 33);
  }
  {
    const DcTree t = dc_tree(6000);
    CHECK(t.n_leaves == 256 && t.levels() == 8 && t.count() == 511);
    CHECK(t.level_maxn[0] == 47 && t.level_maxn[7] == 6000);   // 6000 / 128 = 46.9: pairs of leaves of 23 and 24 rows
  }

  // ---- launch shapes on both sides of every threshold
  //          maxN  setup: threads, LDS, use      secular: threads, grid x, LDS, use
  check_shape(63, 64, 1418, true, 256, 16, 1024, true);
  check_shape(64, 64, 1440, true, 256, 16, 1040, true);
  check_shape(255, 64, 5642, true, 256, 64, 4096, true);
  check_shape(256, 256, 5664, true, 256, 64, 4112, true);
  check_shape(1023, 256, 22538, true, 256, 256, 16384, true);
  check_shape(1024, 1024, 22560, true, 256, 256, 16400, true);
  check_shape(2047, 1024, 45066, true, 256, 512, 32768, true);
  check_shape(2048, 1024, 45088, true, 1024, 128, 32784, true);
  check_shape(7000, 1024, 154032, true, 1024, 438, 112016, true);
  check_shape(7001, 1024, 0, false, 1024, 438, 112032, true);
  check_shape(9800, 1024, 0, false, 1024, 613, 156816, true);
  check_shape(9801, 1024, 0, false, 1024, 613, 0, false);
  // k_dc_zero_offdiag: 256 elements of the two off-diagonal blocks per workgroup and one more, at most 1024
  CHECK(dc_level_launch(33, 1, 1).zero_offdiag.gx == 4);       // 33 * 33 / 2 = 544 -> 3 + 1
  CHECK(dc_level_launch(723, 1, 1).zero_offdiag.gx == 1022);   // 261364 -> 1021 + 1
  CHECK(dc_level_launch(725, 1, 1).zero_offdiag.gx == 1024);   // 262812 -> 1027 + 1, capped
  CHECK(dc_level_launch(46000, 1, 1).zero_offdiag.gx == 1024);   // (the largest order: 46000^2 fits an int)

  // ---- buffer parity: the last stage is the caller's matrix, stages alternate, k_dc_unscale reads the last stage's slot
  for (int nlev = 0; nlev <= 10; ++nlev) {
    CHECK(dc_q_is_out(nlev, nlev));
    for (int s = 0; s < nlev; ++s) {
      CHECK(dc_q_is_out(nlev, s) != dc_q_is_out(nlev, s + 1));
      CHECK(dc_w_slot(s) != dc_w_slot(s + 1));
    }
    CHECK(dc_w_slot(0) == 0);                       // the leaves write w0
    CHECK(dc_w_slot(nlev) == (nlev % 2 == 0 ? 0 : 1));   // w_final = nlev even ? w0 : w1
  }

  // ---- the auxiliary buffer: align_up(12 nodes, 256) + 256 + (n > 7000: batch * 3 n * 8)
  {
    const DcAux A = dc_aux_carve(63, 1000, 4);   // 756 -> 768
    CHECK(A.nodes == 0 && A.flops == 768 && !A.oversize && A.sorted == 0 && A.total == 768 + 256);
  }
  {
    const DcAux A = dc_aux_carve(511, 7000, 2);   // 6132 -> 6144
    CHECK(A.nodes == 0 && A.flops == 6144 && !A.oversize && A.total == 6144 + 256);
  }
  {
    const DcAux A = dc_aux_carve(511, 7001, 3);
    CHECK(A.nodes == 0 && A.flops == 6144 && A.oversize && A.sorted == 6400 && A.total == 6400 + 3 * 3 * 7001 * 8);
    CHECK(A.flops % 256 == 0 && A.sorted % 256 == 0);
  }
  {
    const DcAux A = dc_aux_carve(2047, 24000, 1);   // 24564 -> 24576
    CHECK(A.flops == 24576 && A.oversize && A.sorted == 24832 && A.total == 24832 + 576000);
  }

  std::printf("stedc plan ok\n");
  return 0;
}
