// The plan of the band reduction (springcraft_amd/csrc/sy2sb_plan.h) under AddressSanitizer + UBSan:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I springcraft_amd/csrc \
//       tests/host_sanitize/test_sy2sb_plan.cpp -o /tmp/test_sy2sb_plan && /tmp/test_sy2sb_plan
// (built and run by tests/test_abi_and_host.py::test_sy2sb_plan_under_sanitizers).  Every expected value is a literal written
// out by hand from the algorithm in words (m: rows of the panel below the band, V its 64 reflectors):
//   X1 = L V, X2 = strict(L)^T V     (m x 64, K = m), masks 1 and 2 on the lower-stored trailing matrix
//   Gram = V^T [X1 | X2 | V]         (64 x 192, K = m), 8 K slices
//   W = [X1 | X2 | V] C, and -W      (m x 64, K = 192)
//   trailing update                  (m x m, K = 128; second of a pair 256), C += ..., lower triangle (2 with k_symm3: the
//                                    first super-diagonal entry of even rows as well)
//   first of a pair                  (m x 64, K = 128), C += ...
//   P2 = (-[W1|V1])^T V2             (128 x 64, K = m), 8 K slices;  X1 += [V1|W1] P2  (m x 64, K = 128)
// and the LDS totals are the byte counts the launches asked for before the plan existed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sy2sb_plan.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); std::exit(1); } } while (0)

using namespace sc_host;

static void check_counts_and_roles() {
  for (int n = 2; n <= 30000; ++n) {
    CHECK(panel_count(n) <= n / 64 + 1 && panel_count(n) == (n - 2) / 64);
    for (int batch : {1, 3}) CHECK(stage1_record_count(n, batch) == (n / 64 + 1) * 9 * batch);
    CHECK((long long)panel_count(n) * kRecKinds <= stage1_record_count(n, 1));
  }
  CHECK(kRecKinds == 9 && kRecX1 == 0 && kRecX2 == 1 && kRecGram == 2 && kRecW == 3 && kRecNegW == 4 && kRecTrail == 5 &&
        kRecFirst == 6 && kRecP2 == 7 && kRecCorr == 8);
  const TwoStageEnv E;   // the defaults, whatever the environment holds
  typedef std::vector<int> V;
  CHECK(panel_roles(E, 65) == V{});
  CHECK(panel_roles(E, 66) == V{0});
  CHECK(panel_roles(E, 128) == V{0} && panel_roles(E, 129) == V{0});
  CHECK((panel_roles(E, 384) == V{1, 2, 0, 0, 0}));
  CHECK((panel_roles(E, 512) == V{1, 2, 1, 2, 0, 0, 0}) && panel_roles(E, 513) == panel_roles(E, 512));
  CHECK(symm3_for(E, 512) && !symm3_for(E, 513) && !symm3_for(E, 384));
  PanelGeom g = panel_geom(66, 0);
  CHECK(g.j0 == 0 && g.r0 == 64 && g.m == 2 && g.nr == 1 && g.nchunks == 1);
  g = panel_geom(128, 0);
  CHECK(g.m == 64 && g.nr == 63 && g.nchunks == 1);   // not a full panel
  g = panel_geom(129, 0);
  CHECK(g.m == 65 && g.nr == 64 && g.nchunks == 1);   // a full panel
  g = panel_geom(512, 2);
  CHECK(g.j0 == 128 && g.r0 == 192 && g.m == 320 && g.nr == 64 && g.nchunks == 3);
  g = panel_geom(513, 6);
  CHECK(g.j0 == 384 && g.r0 == 448 && g.m == 65 && g.nr == 64 && g.nchunks == 1);
}

// [p, p + cnt) inside [base, base + size)
static bool inside(const double* p, long long cnt, const double* base, size_t size) {
  return p >= base && cnt >= 1 && p + cnt <= base + size;
}

static void check_records(int n, int batch, int symm_split) {
  const TwoStageEnv E;
  const std::vector<int> role = panel_roles(E, n);
  const bool symm3 = symm3_for(E, n);
  SbLayout SL;
  const size_t slab = sb_slab_layout(n, symm_split, &SL);
  CHECK(SL.slab == (long long)slab && SL.symm_split == symm_split && (SL.xsplit != 0) == (symm_split > 1));
  const long long stride_a = (long long)n * n;
  std::vector<double> a((size_t)batch * n * n), ws((size_t)batch * slab);
  const std::vector<GemmDesc> h = stage1_records(n, batch, role, symm3, a.data(), stride_a, ws.data(), SL);
  CHECK(h.size() == role.size() * 9 * (size_t)batch && (int)h.size() <= stage1_record_count(n, batch));
  for (int p = 0; p < (int)role.size(); ++p) {
    const int m = n - 64 * (p + 1);
    const bool second = role[(size_t)p] == 2;
    const int lower = symm3 ? 2 : 1;
    struct Want { int m, n, k; double alpha, beta; int lower_only, a_tri, slices; };
    const Want want[9] = {
        {m, 64, m, 1.0, 0.0, 0, 1, symm_split},       {m, 64, m, 1.0, 0.0, 0, 2, symm_split},
        {64, 192, m, 1.0, 0.0, 0, 0, 8},              {m, 64, 192, 1.0, 0.0, 0, 0, 1},
        {m, 64, 192, -1.0, 0.0, 0, 0, 1},             {m, m, second ? 256 : 128, 1.0, 1.0, lower, 0, 1},
        {m, 64, 128, 1.0, 1.0, lower, 0, 1},          {128, 64, m, 1.0, 0.0, 0, 0, 8},
        {m, 64, 128, 1.0, 1.0, 0, 0, 1}};
    for (int kind = 0; kind < 9; ++kind)
      for (int b = 0; b < batch; ++b) {
        const size_t at = ((size_t)p * 9 + kind) * batch + b;
        CHECK(stage1_record_index(p, kind, batch, b) == at);
        const GemmDesc& d = h[at];
        const Want& w = want[kind];
        CHECK(d.m == w.m && d.n == w.n && d.k == w.k && d.alpha == w.alpha && d.beta == w.beta);
        CHECK(d.lower_only == w.lower_only && d.a_tri == w.a_tri && d.row_off == 0 && d.col_off == 0);
        CHECK(!d.a_kidx && !d.b_kidx && !d.c_jidx);
        CHECK((d.sa_i == 1 || d.sa_k == 1) && (d.sb_k == 1 || d.sb_j == 1));
        CHECK((w.slices > 1) == (d.split_stride != 0));
        // the footprint of each operand: in matrix b or in slab b, nowhere else
        const double* mat = a.data() + (size_t)b * stride_a;
        const double* sb = ws.data() + (size_t)b * slab;
        const long long ext_a = (d.m - 1) * d.sa_i + (d.k - 1) * d.sa_k + 1, ext_b = (d.k - 1) * d.sb_k + (d.n - 1) * d.sb_j + 1;
        const long long ext_c = (long long)(w.slices - 1) * d.split_stride + (d.n - 1) * d.ldc + d.m;
        CHECK(d.ldc >= d.m);
        CHECK(inside(d.a, ext_a, mat, (size_t)stride_a) || inside(d.a, ext_a, sb, slab));
        CHECK(inside(d.b, ext_b, mat, (size_t)stride_a) || inside(d.b, ext_b, sb, slab));
        // (every panel gets all nine records, launched or not.  The one record that leaves its matrix is never launched:
        // "first of a pair" has 64 columns of C, which a trailing matrix of fewer than 64 rows does not have -- and a first
        // of a pair has at least 320.  Its bytes stay as they always were.)
        const bool never_launched = kind == kRecFirst && role[(size_t)p] != 1 && m < 64;
        CHECK(role[(size_t)p] != 1 || m >= 320);
        CHECK(never_launched || inside(d.c, ext_c, mat, (size_t)stride_a) || inside(d.c, ext_c, sb, slab));
        // which buffer: X1 / X2 / the trailing updates work on the matrix, everything else on the slab
        CHECK(inside(d.a, 1, mat, (size_t)stride_a) == (kind == kRecX1 || kind == kRecX2));
        CHECK(inside(d.c, 1, mat, (size_t)stride_a) == (kind == kRecTrail || kind == kRecFirst));
      }
  }
}

static void check_lds_and_carves() {
  // bytes of dynamic LDS, as the launches computed them before
  CHECK(lds_bytes(lds_panel_qr(9).total) == 12872 && lds_bytes(lds_panel_qr(64).total) == 69632);
  const LdsPanelQr q = lds_panel_qr(9);
  CHECK(q.P == 0 && q.wv == 1161 && q.vv == 1225 && q.red == 1353 && q.total == 1609);
  const size_t blk_a[8] = {71168, 62912, 54656, 46400, 38144, 29888, 21632, 13376};
  const size_t blk_b[8] = {72192, 63936, 55680, 47424, 39168, 30912, 22656, 14400};
  for (int c0 = 0; c0 < 64; c0 += 8) {
    const LdsBlk A = lds_pqr_blk_a(c0), B = lds_pqr_blk_b(c0);
    CHECK(lds_bytes(A.total) == blk_a[c0 / 8] && lds_bytes(B.total) == blk_b[c0 / 8]);
    CHECK(A.P == 0 && A.mid == (64 - c0) * 129 && A.red == A.mid + 128 && A.total == A.red + 512);
    CHECK(B.P == 0 && B.mid == (64 - c0) * 129 && B.red == B.mid + 512 && B.total == B.red + 256);
  }
  CHECK(lds_bytes(lds_panel_wg(1024).total) == 71872 && lds_bytes(lds_panel_wg(512).total) == 38080);
  const LdsPanelWg w = lds_panel_wg(512);
  CHECK(w.red == 0 && w.piv == 128 && w.tauL == 144 && w.Ms == 152 && w.part == 664 && w.total == 4760);
  CHECK(lds_bytes(lds_sb_small().total) == 133120 && lds_sb_small().M1 == 4160 && lds_sb_small().U == 12480);
  const LdsPanelCoop c = lds_panel_coop();
  CHECK(lds_bytes(c.total) == 154256 && c.Pl == 0 && c.Vl == 16448 && c.Ms == 18496 && c.red == 19008 && c.piv == 19072 &&
        c.tauA == 19088 && c.tot4 == 19152 && c.dead == 19280);
  // k_panel_coop's part of the auxiliary buffer
  CHECK(coop_recs_per_matrix(1) == 1056 && coop_recs_per_matrix(128) == 70144);
  struct { int batch, gmax; size_t recs, total; } aux[4] = {{1, 1, 256, 17152}, {3, 1, 256, 50944}, {1, 128, 256, 1122560},
                                                          {3, 128, 256, 3367168}};
  for (const auto& x : aux) {
    const CoopAux A = coop_aux_carve(x.batch, x.gmax);
    CHECK(A.ctl == 0 && A.recs == x.recs && A.total == x.total && A.recs >= (size_t)x.batch * 8 * sizeof(int));
  }
  CHECK(coop_aux_carve(9, 4).recs == 512);   // 9 control records of 32 bytes
  // the parts tile [0, batch) in order, sizes within one of each other
  for (int batch = 1; batch <= 70; ++batch)
    for (int parts = 1; parts <= std::min(4, batch); ++parts) {
      int at = 0, lo_size = batch, hi_size = 0;
      for (int q = 0; q < parts; ++q) {
        const PartBounds pb = part_bounds(batch, parts, q);
        CHECK(pb.lo == at && pb.hi > pb.lo);
        at = pb.hi;
        lo_size = std::min(lo_size, pb.hi - pb.lo);
        hi_size = std::max(hi_size, pb.hi - pb.lo);
      }
      CHECK(at == batch && hi_size - lo_size <= 1);
    }
  CHECK(part_bounds(33, 2, 0).hi == 16 && part_bounds(33, 2, 1).lo == 16 && part_bounds(33, 2, 1).hi == 33);
}

int main() {
  check_counts_and_roles();
  for (int n : {65, 66, 128, 129, 384, 512, 513})
    for (int batch : {1, 3})
      for (int symm_split : {1, 3, 16}) check_records(n, batch, symm_split);
  check_lds_and_carves();
  std::printf("sy2sb plan ok\n");
  return 0;
}
