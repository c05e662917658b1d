// Host-only logic of the C ABI (springcraft_amd/csrc/host_logic.h, scratch_arena.h, twostage_policy.h, gemm_policy.h) under
// AddressSanitizer + UBSan:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I springcraft_amd/csrc \
//       tests/host_sanitize/test_host_logic.cpp -o /tmp/test_host_logic && /tmp/test_host_logic
// (built and run by tests/test_abi_and_host.py::test_host_logic_under_sanitizers).  Expected values restate
// _patch_adjacency_matrix (interaction.py:193-213) and PatchedForceField.force_constant (forcefield.py:199-224).
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gemm_policy.h"
#include "host_logic.h"
#include "scratch_arena.h"
#include "twostage_policy.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); std::exit(1); } } while (0)

static sc_patch_desc desc(const std::vector<int64_t>& shut, const std::vector<int64_t>& off, const std::vector<int64_t>& on,
                          const std::vector<double>* gam) {
  sc_patch_desc d{};
  d.n_shutdown = (int64_t)shut.size(); d.shutdown = shut.empty() ? nullptr : shut.data();
  d.n_pair_off = (int64_t)off.size() / 2; d.pair_off = off.empty() ? nullptr : off.data();
  d.n_pair_on = (int64_t)on.size() / 2; d.pair_on = on.empty() ? nullptr : on.data();
  d.on_force_constants = gam ? gam->data() : nullptr;
  return d;
}

int main() {
  using sc_host::HostPatch;
  std::string err;
  // ---- no patch at all
  {
    HostPatch hp;
    CHECK(sc_host::build_patch(nullptr, 10, hp, err) == SC_OK && !hp.any);
    sc_patch_desc d{};
    CHECK(sc_host::build_patch(&d, 10, hp, err) == SC_OK && !hp.any);
  }
  // ---- shutdown + off + on with overrides, duplicates and both orientations
  {
    const std::vector<int64_t> shut = {3, 3, 0}, off = {1, 2, 4, 5, 2, 1}, on = {1, 2, 6, 7, 7, 6};
    const std::vector<double> gam = {2.5, 1.0, 9.0};
    sc_patch_desc d = desc(shut, off, on, &gam);
    HostPatch hp;
    CHECK(sc_host::build_patch(&d, 8, hp, err) == SC_OK && hp.any);
    CHECK(hp.shut.size() == 8 && hp.shut[0] == 1 && hp.shut[3] == 1 && hp.shut[1] == 0);
    CHECK(hp.row_ptr.size() == 9 && hp.row_ptr[8] == (int32_t)hp.col.size());
    auto find = [&](int i, int j) -> int {
      for (int p = hp.row_ptr[i]; p < hp.row_ptr[i + 1]; ++p) if (hp.col[p] == j) return p;
      return -1;
    };
    // pair_on beats pair_off (applied last), symmetric
    CHECK(find(1, 2) >= 0 && hp.flag[find(1, 2)] == 1 && hp.gam[find(1, 2)] == 2.5);
    CHECK(find(2, 1) >= 0 && hp.flag[find(2, 1)] == 1 && hp.gam[find(2, 1)] == 2.5);
    CHECK(find(4, 5) >= 0 && hp.flag[find(4, 5)] == 0 && find(5, 4) >= 0 && hp.flag[find(5, 4)] == 0);
    // numpy assignment order: m[i, j] = v for all rows, then m[j, i] = v for all rows -> (6,7),(7,6) listed twice:
    // first pass writes m[6,7] = 1.0 then m[7,6] = 9.0, second pass m[7,6] = 1.0 then m[6,7] = 9.0
    CHECK(hp.gam[find(6, 7)] == 9.0 && hp.gam[find(7, 6)] == 1.0);
    for (int i = 0; i < 8; ++i)
      for (int p = hp.row_ptr[i] + 1; p < hp.row_ptr[i + 1]; ++p) CHECK(hp.col[p - 1] < hp.col[p]);   // CSR rows sorted
    CHECK(hp.device_bytes() >= hp.shut.size() + hp.col.size() * 4);
    // device_bytes is the measure of the tables' own layout: carved into exactly that many bytes, the last table ends the buffer
    std::vector<char> buf(hp.device_bytes());
    sc_host::Arena carve(buf.data(), buf.size());
    const HostPatch::Bufs b = hp.layout(carve);
    CHECK(!carve.overrun() && b.shut && b.rp && b.col && b.flag && (char*)(b.gam + hp.gam.size() + 1) == buf.data() + buf.size());
  }
  // ---- the scratch arena (csrc/scratch_arena.h): a layout measures what it carves
  {
    using sc_host::Arena;
    struct Bufs { double* a; char* b; int32_t* c; int64_t* d; double* e; uint8_t* f; };
    const size_t na = 33, nb = 257, nc = 0, nd = 5, ne = 64, nf = 0;   // mixed element types, zero counts in the middle and last
    for (int with_e = 0; with_e < 2; ++with_e) {   // a conditional take (the `v ? take : nullptr` shape of the eigensolver entries)
      auto layout = [&](Arena& s, Bufs& p) {
        p.a = s.take<double>(na);
        p.b = s.take<char>(nb);
        p.c = s.take<int32_t>(nc);
        p.d = s.take<int64_t>(nd);
        p.e = with_e ? s.take<double>(ne) : nullptr;
        p.f = s.take<uint8_t>(nf);
      };
      Arena measure;
      Bufs none{};
      layout(measure, none);
      CHECK(!none.a && !none.b && !none.c && !none.d && !none.e && !none.f && !measure.overrun());   // measuring hands out nothing
      const size_t need = measure.bytes();
      CHECK(need >= na * 8 + nb + nd * 8 + (with_e ? ne * 8 : 0) && need <= 256 * 6 + na * 8 + nb + nd * 8 + ne * 8);
      // a malloc of exactly the measured bytes, so that ASan sees an overrun (malloc aligns to 16 bytes only: the
      // 256-byte alignment is checked on the offsets, which is what it means for a 256-aligned device buffer)
      char* raw = static_cast<char*>(std::malloc(need));
      CHECK(raw != nullptr);
      Arena carve(raw, need);
      Bufs p{};
      layout(carve, p);
      CHECK(!carve.overrun() && carve.bytes() == need);         // measure and carve agree
      CHECK((p.e != nullptr) == (with_e != 0));
      struct Reg { char* at; size_t bytes; };
      const Reg regs[] = {{(char*)p.a, na * 8}, {p.b, nb}, {(char*)p.c, nc * 4}, {(char*)p.d, nd * 8}, {(char*)p.e, with_e ? ne * 8 : 0},
                          {(char*)p.f, nf}};
      char* prev_end = raw;
      unsigned char fill = 1;
      for (const Reg& r : regs) {
        if (!r.at) continue;
        CHECK((size_t)(r.at - raw) % 256 == 0);                 // every region starts on a 256-byte boundary of the buffer
        CHECK(r.at >= prev_end && r.at < raw + need);           // disjoint, in order, and a valid address even when empty
        std::memset(r.at, fill++, r.bytes);                     // written full: an overrun of the malloc is ASan's to report
        prev_end = r.at + (r.bytes ? r.bytes : 1);              // an empty region keeps its address to itself
      }
      CHECK(prev_end == raw + need);
      fill = 1;
      for (const Reg& r : regs) {                               // nothing was overwritten by a later region
        if (!r.at) continue;
        for (size_t i = 0; i < r.bytes; ++i) CHECK((unsigned char)r.at[i] == fill);
        ++fill;
      }
      // one byte short: reported, and the region that does not fit is not handed out
      Arena tight(raw, need - 1);
      Bufs q{};
      layout(tight, q);
      CHECK(tight.overrun() && q.f == nullptr && q.a == p.a && q.d == p.d);
      std::free(raw);
    }
    // zero counts only: distinct valid addresses, one byte each
    {
      Arena m;
      m.take<double>(0);
      m.take<int>(0);
      CHECK(m.bytes() == 257);
      char buf[257];
      Arena c(buf, sizeof(buf));
      double* x = c.take<double>(0);
      int* y = c.take<int>(0);
      CHECK(x && y && (char*)y == (char*)x + 256 && !c.overrun());
      Arena none(buf, 0);
      CHECK(none.take<char>(0) == nullptr && none.overrun());
    }
  }
  // ---- pair_on without force constants: NaN marks "use the base force field" (forcefield.py:221-224)
  {
    const std::vector<int64_t> on = {0, 1};
    sc_patch_desc d = desc({}, {}, on, nullptr);
    HostPatch hp;
    CHECK(sc_host::build_patch(&d, 2, hp, err) == SC_OK);
    CHECK(hp.col.size() == 2 && std::isnan(hp.gam[0]) && std::isnan(hp.gam[1]) && hp.flag[0] == 1);
  }
  // ---- errors: out of range (either column, negative), self pair, inconsistent descriptor
  {
    HostPatch hp;
    const std::vector<int64_t> bad_shut = {8};
    sc_patch_desc d = desc(bad_shut, {}, {}, nullptr);
    CHECK(sc_host::build_patch(&d, 8, hp, err) == SC_ERR_INDEX && err.find("Index 8 is out of bounds") != std::string::npos);
    const std::vector<int64_t> bad_off = {1, -1};
    d = desc({}, bad_off, {}, nullptr);
    CHECK(sc_host::build_patch(&d, 8, hp, err) == SC_ERR_INDEX && err.find("Index -1") != std::string::npos);
    const std::vector<int64_t> bad_on = {9, 1};
    d = desc({}, {}, bad_on, nullptr);
    CHECK(sc_host::build_patch(&d, 8, hp, err) == SC_ERR_INDEX && err.find("Index 9") != std::string::npos);
    const std::vector<int64_t> self = {2, 2};
    d = desc({}, {}, self, nullptr);
    CHECK(sc_host::build_patch(&d, 8, hp, err) == SC_ERR_SELF_PAIR);
    sc_patch_desc e{};
    e.n_pair_on = 3;   // count without pointer
    CHECK(sc_host::build_patch(&e, 8, hp, err) == SC_ERR_INVALID_ARG);
    e = sc_patch_desc{};
    e.n_shutdown = -1;
    CHECK(sc_host::build_patch(&e, 8, hp, err) == SC_ERR_INVALID_ARG);
  }
  // ---- a large random patch: every override lands in its row, nothing out of bounds (ASan / UBSan watch the rest)
  {
    const int64_t n = 5000;
    std::vector<int64_t> shut, off, on;
    std::vector<double> gam;
    unsigned long long s = 12345;
    auto rnd = [&](int64_t m) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (int64_t)((s >> 33) % (unsigned long long)m); };
    for (int i = 0; i < 300; ++i) shut.push_back(rnd(n));
    for (int i = 0; i < 20000; ++i) { off.push_back(rnd(n)); off.push_back(rnd(n)); }
    for (int i = 0; i < 20000; ++i) { int64_t a = rnd(n), b = rnd(n); if (a == b) b = (b + 1) % n; on.push_back(a); on.push_back(b); gam.push_back((double)i); }
    sc_patch_desc d = desc(shut, off, on, &gam);
    HostPatch hp;
    CHECK(sc_host::build_patch(&d, n, hp, err) == SC_OK);
    CHECK((int64_t)hp.row_ptr.size() == n + 1 && hp.row_ptr[0] == 0);
    for (int64_t i = 0; i < n; ++i) {
      CHECK(hp.row_ptr[i] <= hp.row_ptr[i + 1]);
      for (int p = hp.row_ptr[i]; p < hp.row_ptr[i + 1]; ++p) CHECK(hp.col[p] >= 0 && hp.col[p] < n);
    }
    CHECK(hp.col.size() == hp.flag.size() && hp.col.size() == hp.gam.size());
  }
  // ---- force-field descriptor checks
  {
    CHECK(sc_host::check_ff(nullptr, err) == SC_ERR_INVALID_ARG);
    sc_ff_desc f{};
    f.kind = SC_FF_INVARIANT; f.has_cutoff = 0;
    CHECK(sc_host::check_ff(&f, err) == SC_ERR_INVALID_ARG && err == "Cutoff distance must be a float");
    f.has_cutoff = 1; f.cutoff = 7.0; f.cutoff_sq = 49.0;
    CHECK(sc_host::check_ff(&f, err) == SC_OK);
    f.kind = 17;
    CHECK(sc_host::check_ff(&f, err) == SC_ERR_INVALID_ARG);
    f.kind = SC_FF_TABULATED; f.tab = nullptr;
    CHECK(sc_host::check_ff(&f, err) == SC_ERR_INVALID_ARG);
  }
  // ---- launch shape of k_sytrd_resident (one matrix resident on the chip: tridiag.hip)
  {
    using sc_host::ResidentShape;
    ResidentShape S{};
    CHECK(!sc_host::resident_shape(127, 64, 256, 0, 0, &S));                      // too small
    CHECK(sc_host::resident_shape(128, 64, 256, 0, 0, &S) && S.off == 0 && S.m == 128 && S.P == 32 && S.Q == 1 && !S.reg);
    CHECK(sc_host::resident_shape(300, 64, 256, 0, 0, &S) && S.P == 64 && S.logP == 6 && S.Q == 2);
    CHECK(sc_host::resident_shape(300, 64, 256, 0, 256, &S) && S.P == 256 && S.logP == 8);      // more workgroups on request
    CHECK(sc_host::resident_shape(1536, 64, 256, 0, 0, &S) && S.P == 256 && S.Q == 6 && !S.reg &&
          S.lds_bytes == 8 * (size_t)(6 * 1536 + sc_host::kResidentSmallDoubles));
    CHECK(sc_host::resident_shape(2048, 64, 256, 0, 0, &S) && S.Q == 8 && !S.reg && S.lds_bytes <= 160 * 1024);   // the LDS of a CU
    CHECK(sc_host::resident_shape(2049, 64, 256, 0, 0, &S) && S.reg && S.Q == 10 && S.P == 256 && S.off == 0 &&
          S.lds_bytes == 8 * (size_t)sc_host::kResidentSmallDoubles);
    CHECK(sc_host::resident_shape(2561, 64, 256, 0, 0, &S) && S.reg && S.Q == 12);
    CHECK(sc_host::resident_shape(3072, 64, 256, 0, 0, &S) && S.reg && S.off == 0 && (S.m + S.P - 1) / S.P <= sc_host::kResidentRowsReg);
    // larger: the trailing matrix from the first panel boundary at which it fits
    CHECK(sc_host::resident_shape(3073, 64, 256, 0, 0, &S) && S.off == 64 && S.m == 3009);
    CHECK(sc_host::resident_shape(6000, 64, 256, 0, 0, &S) && S.off == 2944 && S.m == 3056 && S.reg);
    CHECK(sc_host::resident_shape(6000, 64, 256, 2048, 0, &S) && S.off == 3968 && S.m == 2032 && !S.reg);   // SPRINGCRAFT_RESIDENT_MAX
    // a device with fewer CUs has no register form and may not fit the workgroups at all
    CHECK(sc_host::resident_shape(3000, 64, 128, 0, 0, &S) == false || (S.m <= 2048 && S.P <= 128));
    CHECK(sc_host::resident_shape(1000, 64, 128, 0, 0, &S) && S.P == 128);
    CHECK(!sc_host::resident_shape(2000, 64, 128, 0, 0, &S));                      // needs 256 workgroups
    for (int n = 128; n <= 7000; n += 37) {
      if (!sc_host::resident_shape(n, 64, 256, 0, 0, &S)) { CHECK(false); continue; }
      const int rows = (S.m - 1) / S.P + 1;
      CHECK(S.off % 64 == 0 && S.off + S.m == n && S.m <= 3072 && (1 << S.logP) == S.P && S.P <= 256);
      CHECK(rows <= (S.reg ? 12 : 8) && 256 * S.Q >= S.m && S.lds_bytes <= 160 * 1024);
    }
  }
  // ---- the pair consumers' grid: one workgroup per unordered pair of tiles
  CHECK(sc_host::tri_tile_count(1, 64) == 1 && sc_host::tri_tile_count(64, 64) == 1 && sc_host::tri_tile_count(65, 64) == 3);
  CHECK(sc_host::tri_tile_count(128, 64) == 3 && sc_host::tri_tile_count(129, 64) == 6 && sc_host::tri_tile_count(2000, 64) == 528);
  CHECK(sc_host::tri_tile_count(0, 64) == 0 && sc_host::tri_tile_count(0x7fffffffLL, 64) == 33554432LL * 33554433LL / 2);
  // ---- the two-stage policy (csrc/twostage_policy.h): the decisions its comments document as measured, on a device of
  // 256 CUs / 8 XCDs with the default environment (a default-constructed TwoStageEnv: the process environment is not read)
  {
    using namespace sc_host;
    const TwoStageEnv E;
    auto form = [&](int batch, int n) { return chase_form_for(E, n, batch, 8, 256, true, -1, -1, 1); };
    CHECK(form(16, 6000) == ChaseForm::Sweep && form(32, 3000) == ChaseForm::Sweep);
    CHECK(form(64, 3000) == ChaseForm::Pair && form(32, 6000) == ChaseForm::Pair && form(64, 6000) == ChaseForm::Pair);
    CHECK(form(512, 1026) == ChaseForm::Stepwise);                                  // 64 matrices per XCD > 32 CUs
    CHECK(form(1, 24000) == ChaseForm::Spread && form(1, 6000) == ChaseForm::Spread);
    CHECK(form(1, 3000) == ChaseForm::Sweep);
    CHECK(form(96, 6000) == ChaseForm::Pair && form(256, 3000) == ChaseForm::Pair);   // work 4500, 6000
    CHECK(form(257, 3000) != ChaseForm::Pair);
    CHECK(chase_form_for(E, 6000, 64, 8, 256, /*pair_attr=*/false, -1, -1, 1) != ChaseForm::Pair);   // LDS refused
    CHECK(chase_form_for(E, 3000, 32, 8, 256, true, -1, -1, /*chase_ok=*/0) == ChaseForm::Stepwise);   // after a time-out
    {
      // 64 x 6000, two pair workgroups per CU: 8 matrices per XCD share its 64 slots; 95 tasks per sweep keep 33 pairs busy
      const ChaseLaunch L = chase_launch(E, ChaseForm::Pair, 6000, 64, 8, 256, 2);
      CHECK(L.nxcd == 8 && L.W == 8 && L.grid == 8 * 64 && L.early_bytes == 0);
      const ChaseLaunch S = chase_launch(E, ChaseForm::Spread, 24000, 1, 8, 256, 2);
      CHECK(S.nxcd == 1 && S.W == chase_len(24000, 0) / 2 + 1 && S.grid == S.W && S.early_bytes == (size_t)24000 * 8 * 16);
      CHECK(chase_launch(E, ChaseForm::Sweep, 3000, 32, 8, 256, 0).W == 0);           // occupancy query failed: no launch
    }
    // parts of the batch
    CHECK(stage1_parts(E, 31, false) == 1 && stage1_parts(E, 32, false) == 2 && stage1_parts(E, 32, true) == 1);
    {
      TwoStageEnv E3;
      E3.stage1_streams = 3;
      CHECK(stage1_parts(E3, 2, false) == 2 && stage1_parts(E3, 64, true) == 3);
    }
    CHECK(bulge_stream_parts(E, 15) == 1 && bulge_stream_parts(E, 16) == 2 && bulge_stream_parts(E, 48) == 3);
    // panel pairs: while the trailing matrix behind the second panel has >= 256 rows
    {
      const std::vector<int> r = panel_roles(E, 6000);
      CHECK((int)r.size() == panel_count(6000) && r.size() == 93 && r[0] == 1 && r[1] == 2 && r[86] == 1 && r[87] == 2 && r[88] == 0 && r[92] == 0);   // 6000 - 90 * 64 = 240 < 256
      TwoStageEnv E1;
      E1.panel_pairs = false;
      for (int x : panel_roles(E1, 6000)) CHECK(x == 0);
      CHECK(panel_roles(E, 65).empty() && panel_roles(E, 3).empty());
    }
    // panel QR form by the rows m of a full-width panel, coop granted, whole batch on one stream: budget 192 workgroups
    {
      auto kind = [&](const CoopPlan& C, bool recs, int m, int nb) { return panel_qr_form(E, C, recs, m, nb, true); };
      const CoopPlan C4 = coop_plan(E, 6145 + 64, 4, 256, false, -1, 1);
      CHECK(C4.ask && C4.budget == 192 && C4.min_many == 6145 && C4.gmax == 25 && C4.nb_max == 4);
      PanelQrForm F = kind(C4, true, 4096, 4);
      CHECK(F.kind == PanelQr::Wg1024 && F.ru == 4 && F.cu == 2);
      F = kind(C4, true, 3072, 4);
      CHECK(F.kind == PanelQr::Wg1024 && F.ru == 3 && F.cu == 4);
      F = kind(C4, true, 4097, 4);
      CHECK(F.kind == PanelQr::Wg512 && F.ru == 10 && F.cu == 1);
      F = kind(C4, true, 5121, 4);
      CHECK(F.kind == PanelQr::Wg512 && F.ru == 12 && F.cu == 1);
      F = kind(C4, true, 6145, 4);
      CHECK(F.kind == PanelQr::Coop && F.coop_g == 25);
      CHECK(panel_qr_form(E, C4, true, 6145, 4, /*main_stream=*/false).kind == PanelQr::Blocked);   // a side stream never
      const CoopPlan C1 = coop_plan(E, 6145 + 64, 1, 256, false, -1, 1);
      CHECK(C1.ask && C1.min_few == 300);
      F = kind(C1, true, 299, 1);
      CHECK(F.kind == PanelQr::Wg1024 && F.ru == 1 && F.cu == 8);
      CHECK(kind(C1, true, 300, 1).kind == PanelQr::Coop && kind(C1, true, 4096, 1).kind == PanelQr::Coop);
      CHECK(kind(C1, false, 4097, 1).kind == PanelQr::Blocked && kind(C1, false, 4096, 1).kind == PanelQr::Wg1024);
      CHECK(kind(C1, false, 64, 1).kind == PanelQr::Unblocked);                       // 63 reflectors: not a full panel
      TwoStageEnv Eu;
      Eu.qr_blocked = false;
      CHECK(panel_qr_form(Eu, C1, false, 4097, 1, true).kind == PanelQr::Unblocked);
      // two stage-1 parts (32 matrices, unprofiled): never coop; profiled, the batch is on one stream again
      CHECK(!coop_plan(E, 6145 + 64, 32, 256, false, -1, 1).ask && coop_plan(E, 6145 + 64, 32, 256, true, -1, 1).ask);
      CHECK(!coop_plan(E, 6145 + 64, 1, 256, false, /*coop_min_rows=*/0, 1).ask);   // switched off per context
      CHECK(!coop_plan(E, 6145 + 64, 1, 256, false, -1, /*coop_ok=*/0).ask);        // after a time-out
      CHECK(!coop_plan(E, 363, 1, 256, false, -1, 1).ask && coop_plan(E, 364, 1, 256, false, -1, 1).ask);   // 300 rows
    }
    // stage-2 back-transformation
    CHECK(bt2_plan(E, 6000, 1, 20, 256).wave && bt2_plan(E, 6000, 16, 64, 256).wave && !bt2_plan(E, 6000, 17, 64, 256).wave);
    CHECK(bt2_plan(E, 6000, 64, 6000, 256).nw == 8 && bt2_plan(E, 3000, 8, 3000, 256).nw == 4);
    CHECK(bt2_plan(E, 16384, 2, 16384, 256).nw == 8 && bt2_plan(E, 16384, 2, 16383, 256).nw == 8 && bt2_plan(E, 16384, 2, 16256, 256).nw == 4);
    {
      const Bt2Plan P = bt2_plan(E, 6000, 64, 6000, 256);
      CHECK(P.xcd && P.nchunk == 47 && P.grid_x == 64u * 47u && P.grid_y == 1u);
      const Bt2Plan Q = bt2_plan(E, 6000, 4, 6000, 256);
      CHECK(!Q.xcd && Q.nw == 4 && Q.nchunk == 94 && Q.grid_x == 94u && Q.grid_y == 4u);
    }
    // K slices of the SYMM: k_symm3 path (even n >= 512) ...
    CHECK(symm3_for(E, 24000) && !symm3_for(E, 24001) && !symm3_for(E, 510));
    CHECK(symm_split_for(E, 24000, 1) == 9);                                      // ceil(1536 / 188)
    CHECK(symm_split_for(E, 6000, 17) == 1 && symm_split_for(E, 6000, 16) == 3);  // 799 items; 752: ceil(1536 / 752)
    CHECK(symm_split_for(E, 6000, 32) == 3 && symm_split_for(E, 6000, 34) == 1);  // half the batch per launch from 32 on
    CHECK(symm_split_for(E, 512, 1) == 16);
    // ... and the odd-order path: 4 -> 5, six and more -> 9
    CHECK(symm_split_for(E, 6001, 6) == 5);     // 564 tiles
    CHECK(symm_split_for(E, 24001, 1) == 9);    // 376 tiles
    CHECK(symm_split_for(E, 4481, 10) == 3);    // 710 tiles
    CHECK(symm_split_for(E, 6001, 11) == 1 && symm_split_for(E, 2047, 1) == 1);   // >= 1024 tiles; n < 2048
    {
      TwoStageEnv Es;
      Es.symm_split = 40;
      CHECK(symm_split_for(Es, 6000, 1) == 16);
    }
    // ---- the shapes of the stage cases of tests/test_stage_ratios_gpu.py (test_form_*): the form of every decision, the
    // counts written out by hand from the rules above; the GPU tests assert the same literals on the context's counters.
    // Panels of order n: p = 0 .. while n - 64 (p + 1) >= 2, of m = n - 64 (p + 1) rows; a pair while n - 64 (p + 2) >= 256;
    // k_panel_wg<ru> for 1024 (ru - 1) < m <= 1024 ru, <10,1,512> for 4096 < m <= 5120, <12,1,512> up to 6144 (four and
    // more matrices), one matrix above 4096 rows: blocked; the last panel of fewer than 65 rows: unblocked.
    {
      struct Shape {
        const char* name;
        int n, batch, coop_min_rows;
        // per solve, summed over the stage-1 parts: Coop, Wg1024 ru 1..4, Wg512 ru 10, 12, Blocked, Unblocked
        int qr[9];
        int role1, role2, slices, s1_parts, chase_parts;
        ChaseForm chase_default;
        int bt2_nw; bool bt2_xcd; unsigned gx, gy;   // (no case takes k_bt2_wave: all n columns)
      };
      const Shape shapes[] = {
          // a: 17 panels of 1036, 972, .., 76, 12 rows; pairs while n - 64 (p + 2) >= 256: p = 0 .. 11; 9 x 1 items: 16 slices
          {"a", 1100, 1, 0, {0, 15, 1, 0, 0, 0, 0, 0, 1}, 6, 6, 16, 1, 1, ChaseForm::Sweep, 4, false, 18u, 1u},
          // b: 33 panels from 2056 rows: one above 2048, 16 above 1024; pairs p = 0 .. 27
          {"b", 2120, 1, 0, {0, 15, 16, 1, 0, 0, 0, 0, 1}, 14, 14, 16, 1, 1, ChaseForm::Sweep, 4, false, 34u, 1u},
          // c: 49 panels from 3076 rows; pairs p = 0 .. 43
          {"c", 3140, 1, 0, {0, 15, 16, 16, 1, 0, 0, 0, 1}, 22, 22, 16, 1, 1, ChaseForm::Sweep, 4, false, 50u, 1u},
          // d: 65 panels from 4098 rows (one matrix: the chunked launches), then 4034 .. 3074: 16 of <4,2>; pairs p = 0 .. 59
          {"d", 4162, 1, 0, {0, 15, 16, 16, 16, 0, 0, 1, 1}, 30, 30, 16, 1, 1, ChaseForm::Sweep, 4, false, 66u, 1u},
          // e: the same panels, four matrices: 4098 rows = 9 x 512 -> <10,1,512>; 33 x 4 = 132 items: ceil(1536 / 132) = 12
          {"e", 4162, 4, -1, {0, 15, 16, 16, 16, 1, 0, 0, 1}, 30, 30, 12, 1, 1, ChaseForm::Sweep, 4, false, 66u, 4u},
          // f: 81 panels from 5126 rows = 11 x 512 -> <12,1,512>, then 5062 .. 4102: 16 of <10,1,512>; pairs p = 0 .. 75;
          // 41 x 4 = 164 items: ceil(1536 / 164) = 10; n > 4500 with fewer matrices than XCDs: the spread chase
          {"f", 5190, 4, -1, {0, 15, 16, 16, 16, 16, 1, 0, 1}, 38, 38, 10, 1, 1, ChaseForm::Spread, 4, false, 82u, 4u},
          // g: 7 panels of 386 .. 66, 2 rows; 450 - 128 = 322 >= 256: one pair, 450 - 256 = 194: no second
          {"g", 450, 7, -1, {0, 6, 0, 0, 0, 0, 0, 0, 1}, 1, 1, 1, 1, 1, ChaseForm::Sweep, 4, false, 8u, 7u},
          // h: 31 panels of 1985 .. 65 rows (the last one full: 64 reflectors), one matrix: k_panel_coop from 300 rows
          // (p = 0 .. 26); odd order: no k_symm3, 33 tiles -> ceil(2048 / 33) >= 6 -> 9 slices; pairs p = 0 .. 27
          {"h", 2049, 1, -1, {27, 4, 0, 0, 0, 0, 0, 0, 0}, 14, 14, 9, 1, 1, ChaseForm::Sweep, 4, false, 33u, 1u},
          // i .. l: 5 panels of 258, 194, 130, 66, 2 rows, no pair (322 - 128 < 256); from 32 matrices on two parts
          {"i", 322, 33, -1, {0, 8, 0, 0, 0, 0, 0, 0, 2}, 0, 0, 1, 2, 2, ChaseForm::Sweep, 4, true, 8u * 5u * 6u, 1u},
          {"j16", 322, 16, -1, {0, 4, 0, 0, 0, 0, 0, 0, 1}, 0, 0, 1, 1, 2, ChaseForm::Sweep, 4, true, 8u * 2u * 6u, 1u},
          {"j48", 322, 48, -1, {0, 8, 0, 0, 0, 0, 0, 0, 2}, 0, 0, 1, 2, 3, ChaseForm::Sweep, 4, true, 8u * 6u * 6u, 1u},
          {"k", 322, 9, -1, {0, 4, 0, 0, 0, 0, 0, 0, 1}, 0, 0, 1, 1, 1, ChaseForm::Sweep, 4, true, 8u * 2u * 6u, 1u},
          // l: 3 x 86 = 258 >= 256 workgroups of 128 columns: eight waves, 3 chunks; 85 matrices would stay on four
          {"l", 322, 86, -1, {0, 8, 0, 0, 0, 0, 0, 0, 2}, 0, 0, 1, 2, 3, ChaseForm::Sweep, 8, true, 8u * 11u * 3u, 1u},
      };
      for (const Shape& S : shapes) {
        const int parts = stage1_parts(E, S.batch, false);
        const CoopPlan C = coop_plan(E, S.n, S.batch, 256, false, S.coop_min_rows, 1);
        const bool recs = C.ask && C.nb_max >= 1;   // (the LDS attribute granted)
        const std::vector<int> role = panel_roles(E, S.n);
        int qr[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, r1 = 0, r2 = 0;
        for (int p = 0; p < (int)role.size(); ++p) {
          r1 += role[(size_t)p] == 1;
          r2 += role[(size_t)p] == 2;
          for (int q = 0; q < parts; ++q) {
            const int lo = (int)((long long)S.batch * q / parts), hi = (int)((long long)S.batch * (q + 1) / parts);
            const PanelQrForm F = panel_qr_form(E, C, recs, S.n - (p + 1) * kBand, hi - lo, q == 0);
            switch (F.kind) {
              case PanelQr::Coop: ++qr[0]; break;
              case PanelQr::Wg1024: CHECK(F.ru >= 1 && F.ru <= 4 && F.cu == (F.ru <= 2 ? 8 : (F.ru == 3 ? 4 : 2))); ++qr[F.ru]; break;
              case PanelQr::Wg512: CHECK((F.ru == 10 || F.ru == 12) && F.cu == 1); ++qr[F.ru == 10 ? 5 : 6]; break;
              case PanelQr::Blocked: ++qr[7]; break;
              case PanelQr::Unblocked: ++qr[8]; break;
            }
          }
        }
        bool same = true;
        for (int k = 0; k < 9; ++k) same = same && qr[k] == S.qr[k];
        if (!same) std::fprintf(stderr, "shape %s: panel QR forms %d %d %d %d %d %d %d %d %d\n", S.name, qr[0], qr[1], qr[2], qr[3],
                                qr[4], qr[5], qr[6], qr[7], qr[8]);
        CHECK(same);
        CHECK(r1 == S.role1 && r2 == S.role2);
        CHECK(symm_split_for(E, S.n, S.batch) == S.slices);
        CHECK(parts == S.s1_parts && bulge_stream_parts(E, S.batch) == S.chase_parts);
        // sc_dbg_set_chase(ctx, 0, 0): the per-wavefront launches; left alone: what the size gives
        CHECK(chase_form_for(E, S.n, S.batch, 8, 256, true, /*chase_mode=*/0, -1, 1) == ChaseForm::Stepwise);
        CHECK(chase_form_for(E, S.n, S.batch, 8, 256, true, -1, -1, 1) == S.chase_default);
        const Bt2Plan P = bt2_plan(E, S.n, S.batch, S.n, 256);
        CHECK(!P.wave && P.nw == S.bt2_nw && P.xcd == S.bt2_xcd && P.grid_x == S.gx && P.grid_y == S.gy);
      }
      // the first stage-1 part of 33 matrices has 16, the second 17
      CHECK((int)(33LL * 1 / 2) == 16 && 33 - 16 == 17);
      CHECK(bt2_plan(E, 322, 85, 322, 256).nw == 4 && bt2_plan(E, 322, 7, 322, 256).xcd == false);
    }
    // the environment is read in one place; unset, it is the default-constructed struct
    if (!getenv("SPRINGCRAFT_STAGE1_STREAMS") && !getenv("SPRINGCRAFT_BULGE_PAIR")) {
      const TwoStageEnv R = read_two_stage_env();
      CHECK(R.stage1_streams == 0 && R.bulge_pair == -1 && R.bulge_pair_max == 6000 && R.bulge_burst >= 1);
    }
  }
  // ---- the launch policy of the float64 GEMMs (csrc/gemm_policy.h) on a device of 256 CUs with the default environment
  // (a default-constructed GemmEnv): every expected value written out by hand from the launchers' rules
  {
    using namespace sc_host;
    const GemmEnv E;
    auto same = [](GemmTile t, int bm, int bn) { return t.bm == bm && t.bn == bn; };
    // block tile: 128 rows from 2 x 256 workgroups of 128 x 64 on, 128 columns from 3 x 256 workgroups of 128 x 128 on
    CHECK(same(gemm2_tile(E, 256, {.count = 511, .max_m = 128, .max_n = 64, .layout = kGemmAmBk}), 64, 64));
    CHECK(same(gemm2_tile(E, 256, {.count = 512, .max_m = 128, .max_n = 64, .layout = kGemmAmBk}), 128, 64));
    CHECK(same(gemm2_tile(E, 256, {.count = 767, .max_m = 128, .max_n = 128, .layout = kGemmAmBk}), 128, 64));
    CHECK(same(gemm2_tile(E, 256, {.count = 768, .max_m = 128, .max_n = 128, .layout = kGemmAmBk}), 128, 128));
    CHECK(same(gemm2_tile(E, 256, {.count = 256, .max_m = 128, .max_n = 128, .layout = kGemmAmBn, .split_k = 3}), 128, 128));   // slices count
    CHECK(same(gemm2_tile(E, 256, {.count = 4096, .max_m = 64, .max_n = 128, .layout = kGemmAmBk}), 64, 64));   // not wider than 64 rows
    // a context that reports no CUs plans for 256; one of 128 CUs has half the thresholds
    CHECK(same(gemm2_tile(E, 0, {.count = 511, .max_m = 128, .max_n = 64, .layout = kGemmAmBk}), 64, 64));
    CHECK(same(gemm2_tile(E, 0, {.count = 512, .max_m = 128, .max_n = 64, .layout = kGemmAmBk}), 128, 64));
    CHECK(same(gemm2_tile(E, 128, {.count = 256, .max_m = 128, .max_n = 64, .layout = kGemmAmBk}), 128, 64));
    // never 128 x 128 with both operands k-contiguous, by size or forced
    CHECK(same(gemm2_tile(E, 256, {.count = 768, .max_m = 128, .max_n = 128, .layout = kGemmAkBk}), 128, 64));
    CHECK(same(gemm2_tile(E, 256, {.count = 1, .max_m = 64, .max_n = 64, .layout = kGemmAkBk, .pin_tile = 1}), 128, 64));
    // precedence: the debug override, then SPRINGCRAFT_GEMM2_TILE, then pin_tile, then the size
    GemmEnv E2;
    E2.gemm2_tile = 2;
    CHECK(same(gemm2_tile(E2, 256, {.count = 1, .max_m = 64, .max_n = 64, .layout = kGemmAmBk, .pin_tile = 1, .dbg = {.force_tile = 3}}), 64, 64));
    CHECK(same(gemm2_tile(E2, 256, {.count = 1, .max_m = 64, .max_n = 64, .layout = kGemmAmBk, .pin_tile = 1}), 128, 64));
    CHECK(same(gemm2_tile(E, 256, {.count = 1, .max_m = 64, .max_n = 64, .layout = kGemmAmBk, .pin_tile = 1}), 128, 128));
    CHECK(same(gemm2_tile(E, 256, {.count = 768, .max_m = 128, .max_n = 128, .layout = kGemmAmBk, .pin_tile = 3}), 64, 64));
    CHECK(same(gemm2_tile(E, 256, {.count = 1, .max_m = 64, .max_n = 64, .layout = kGemmAmBk}), 64, 64));
    // gather launches: by size; only the debug override 2 / 3 forces them, the environment and pin_tile do not
    CHECK(same(gemm2_gather_tile(256, {.count = 511, .max_m = 128, .max_n = 64, .layout = kGemmAmBk, .gather = true}), 64, 64));
    CHECK(same(gemm2_gather_tile(256, {.count = 512, .max_m = 128, .max_n = 64, .layout = kGemmAmBk, .gather = true}), 128, 64));
    CHECK(same(gemm2_gather_tile(0, {.count = 512, .max_m = 128, .max_n = 64, .layout = kGemmAmBk, .gather = true}), 128, 64));
    CHECK(same(gemm2_gather_tile(256, {.count = 512, .max_m = 128, .max_n = 64, .layout = kGemmAmBk, .gather = true, .pin_tile = 3}), 128, 64));
    CHECK(same(gemm2_gather_tile(256, {.count = 512, .max_m = 128, .max_n = 64, .layout = kGemmAmBk, .gather = true, .dbg = {.force_tile = 3}}), 64, 64));
    CHECK(same(gemm2_gather_tile(256, {.count = 1, .max_m = 128, .max_n = 64, .layout = kGemmAmBk, .gather = true, .dbg = {.force_tile = 2}}), 128, 64));
    CHECK(same(gemm2_gather_tile(256, {.count = 1, .max_m = 128, .max_n = 64, .layout = kGemmAmBk, .gather = true, .dbg = {.force_tile = 1}}), 64, 64));
    // grid: (mode; tile grid the kernel decodes against; grid of the launch)
    auto grid_is = [](GemmGrid g, int mode, int gx, int gy, int gz, unsigned x, unsigned y, unsigned z) {
      return g.mode == mode && g.gx == gx && g.gy == gy && g.gz == gz && g.x == x && g.y == y && g.z == z;
    };
    // lower triangle of 5 row tiles: 5 * 6 / 2 = 15 tiles of 64 x 64 or 128 x 128, twice as many of 128 x 64; 7 records on y
    CHECK(grid_is(gemm2_grid(E, 64, 64, 5, 5, 7, false, true), 1, 15, 7, 1, 15u, 7u, 1u));
    CHECK(grid_is(gemm2_grid(E, 128, 128, 5, 5, 7, false, true), 1, 15, 7, 1, 15u, 7u, 1u));
    CHECK(grid_is(gemm2_grid(E, 128, 64, 5, 10, 7, false, true), 1, 30, 7, 1, 30u, 7u, 1u));
    CHECK(grid_is(gemm2_grid(E, 128, 64, 1, 2, 3, false, true), 1, 2, 3, 1, 2u, 3u, 1u));   // (2 tiles: a lower grid never pairs)
    // triangular operands: one flat grid, longest tiles first, below 0x7fffffff blocks
    CHECK(grid_is(gemm2_grid(E, 64, 64, 4, 3, 5, true, false), 2, 4, 3, 5, 60u, 1u, 1u));
    CHECK(grid_is(gemm2_grid(E, 64, 64, 0x7ffffffeu, 1, 1, true, false), 2, 0x7ffffffe, 1, 1, 0x7ffffffeu, 1u, 1u));
    CHECK(grid_is(gemm2_grid(E, 64, 64, 0x7fffffffu, 1, 1, true, false), 0, 0x7fffffff, 1, 1, 0x7fffffffu, 1u, 1u));
    CHECK(grid_is(gemm2_grid(E, 64, 64, 65536, 32768, 1, true, false), 0, 65536, 32768, 1, 65536u, 32768u, 1u));   // 2^31 blocks
    // 2 .. 4 row tiles: the records x column tiles rounded up to the 8 XCDs, times the row tiles
    CHECK(grid_is(gemm2_grid(E, 128, 64, 1, 3, 5, false, false), 0, 1, 3, 5, 1u, 3u, 5u));
    CHECK(grid_is(gemm2_grid(E, 128, 64, 2, 3, 5, false, false), 3, 2, 3, 5, 32u, 1u, 1u));
    CHECK(grid_is(gemm2_grid(E, 128, 64, 4, 3, 5, false, false), 3, 4, 3, 5, 64u, 1u, 1u));
    CHECK(grid_is(gemm2_grid(E, 128, 64, 4, 2, 8, false, false), 3, 4, 2, 8, 64u, 1u, 1u));   // 16 is a multiple of 8 already
    CHECK(grid_is(gemm2_grid(E, 128, 64, 5, 3, 5, false, false), 0, 5, 3, 5, 5u, 3u, 5u));
    {
      GemmEnv En;
      En.no_pair = true;
      CHECK(grid_is(gemm2_grid(En, 128, 64, 2, 3, 5, false, false), 0, 2, 3, 5, 2u, 3u, 5u));
      CHECK(grid_is(gemm2_grid(En, 64, 64, 4, 3, 5, true, false), 2, 4, 3, 5, 60u, 1u, 1u));
      En = GemmEnv{};
      En.no_balance = true;
      CHECK(grid_is(gemm2_grid(En, 64, 64, 4, 3, 5, true, false), 0, 4, 3, 5, 4u, 3u, 5u));   // (a tri launch never pairs)
      CHECK(grid_is(gemm2_grid(En, 128, 64, 2, 3, 5, false, false), 3, 2, 3, 5, 32u, 1u, 1u));
    }
    // lower_grid: square launches of layout kGemmAmBn without K slices, masks or gathers
    CHECK(gemm2_lower_grid_allowed(E, {.count = 4, .max_m = 256, .max_n = 256, .layout = kGemmAmBn, .lower_grid = true}));
    CHECK(gemm2_lower_grid_allowed(E, {.count = 4, .max_m = 256, .max_n = 256, .layout = kGemmAmBn, .split_k = 0, .lower_grid = true}));
    CHECK(!gemm2_lower_grid_allowed(E, {.count = 4, .max_m = 256, .max_n = 256, .layout = kGemmAmBn}));
    CHECK(!gemm2_lower_grid_allowed(E, {.count = 4, .max_m = 256, .max_n = 256, .layout = kGemmAmBn, .split_k = 2, .lower_grid = true}));
    CHECK(!gemm2_lower_grid_allowed(E, {.count = 4, .max_m = 256, .max_n = 255, .layout = kGemmAmBn, .lower_grid = true}));
    CHECK(!gemm2_lower_grid_allowed(E, {.count = 4, .max_m = 256, .max_n = 256, .layout = kGemmAmBn, .tri = true, .lower_grid = true}));
    CHECK(!gemm2_lower_grid_allowed(E, {.count = 4, .max_m = 256, .max_n = 256, .layout = kGemmAmBn, .gather = true, .lower_grid = true}));
    CHECK(!gemm2_lower_grid_allowed(E, {.count = 4, .max_m = 256, .max_n = 256, .layout = kGemmAmBk, .lower_grid = true}));
    {
      GemmEnv En;
      En.no_lower_grid = true;
      CHECK(!gemm2_lower_grid_allowed(En, {.count = 4, .max_m = 256, .max_n = 256, .layout = kGemmAmBn, .lower_grid = true}));
    }
    // chunks of at most 65535 records x slices
    CHECK(gemm2_records_per_launch(65535, 1) == 65535 && gemm2_records_per_launch(65536, 1) == 65535);
    CHECK(gemm2_records_per_launch(21845, 3) == 21845 && gemm2_records_per_launch(21846, 3) == 21845);   // 65535, 65538
    CHECK(gemm2_records_per_launch(32768, 2) == 32767 && gemm2_records_per_launch(1 << 24, 65535) == 1);

    // ---- k_gemm3: 1024 records of one 128 x 64 tile each are the least it takes
    const GemmDevice D{256, 1, false}, Dside{256, 1, true};
    const Gemm3Launch base{.count = 1024, .m = 128, .n = 64, .k = 128, .layout = kGemmAmBk, .lower = 0, .alpha = 1.0, .beta = 0.0, .aligned16 = true};
    auto with = [&](auto change) { Gemm3Launch l = base; change(l); return l; };
    CHECK(gemm3_takes(E, D, base) && gemm3_takes(E, GemmDevice{256, -1, false}, base));
    CHECK(gemm3_takes(E, D, with([](Gemm3Launch& l) { l.layout = kGemmAkBk; })) && gemm3_takes(E, D, with([](Gemm3Launch& l) { l.beta = 1.0; })));
    CHECK(!gemm3_takes(E, D, with([](Gemm3Launch& l) { l.k = 112; })));
    CHECK(!gemm3_takes(E, D, with([](Gemm3Launch& l) { l.k = 136; })) && gemm3_takes(E, D, with([](Gemm3Launch& l) { l.k = 144; })));
    CHECK(!gemm3_takes(E, D, with([](Gemm3Launch& l) { l.m = 129; })));
    CHECK(!gemm3_takes(E, D, with([](Gemm3Launch& l) { l.n = 65; l.layout = kGemmAmBn; })));
    CHECK(gemm3_takes(E, D, with([](Gemm3Launch& l) { l.n = 65; })) && gemm3_takes(E, D, with([](Gemm3Launch& l) { l.layout = kGemmAmBn; })));
    CHECK(!gemm3_takes(E, D, with([](Gemm3Launch& l) { l.lower = 1; l.count = 7; })));   // 128 x 64 is not square
    {
      // ... and nothing but "lower needs m == n" declines it: 1024 records of one tile, lower-only launches always taken
      // (SPRINGCRAFT_GEMM3_LOWER = 1), or as a debug entry launches it; the square 128 x 128 (2 tiles each) is taken
      GemmEnv E_l1;
      E_l1.gemm3_lower = 1;
      CHECK(!gemm3_takes(E_l1, D, with([](Gemm3Launch& l) { l.lower = 1; })));
      CHECK(!gemm3_takes(E, D, with([](Gemm3Launch& l) { l.lower = 2; l.dbg.any_size = true; })));
      CHECK(gemm3_takes(E_l1, D, with([](Gemm3Launch& l) { l.lower = 1; l.n = 128; })));
      CHECK(gemm3_takes(E, D, with([](Gemm3Launch& l) { l.lower = 2; l.n = 128; l.dbg.any_size = true; })));
    }
    // no rows or no columns: declined before the tile count (0 tiles would pass a debug entry's any_size)
    CHECK(!gemm3_takes(E, D, with([](Gemm3Launch& l) { l.m = 0; l.dbg.any_size = true; })));
    CHECK(!gemm3_takes(E, D, with([](Gemm3Launch& l) { l.m = -2; l.dbg.any_size = true; })));
    CHECK(!gemm3_takes(E, D, with([](Gemm3Launch& l) { l.n = 0; l.dbg.any_size = true; })));
    CHECK(gemm3_takes(E, D, with([](Gemm3Launch& l) { l.m = 2; l.n = 1; l.count = 1; l.dbg.any_size = true; })));
    CHECK(!gemm3_takes(E, D, with([](Gemm3Launch& l) { l.alpha = -1.0; })));
    CHECK(!gemm3_takes(E, D, with([](Gemm3Launch& l) { l.beta = 0.5; })));
    CHECK(!gemm3_takes(E, D, with([](Gemm3Launch& l) { l.aligned16 = false; })));
    CHECK(!gemm3_takes(E, D, with([](Gemm3Launch& l) { l.layout = 3; })) && !gemm3_takes(E, D, with([](Gemm3Launch& l) { l.count = 0; })));
    CHECK(!gemm3_takes(E, GemmDevice{255, 1, false}, base));
    CHECK(!gemm3_takes(E, GemmDevice{256, 0, false}, base));
    // 1023 tiles: only for SPRINGCRAFT_GEMM3 = 2 and the debug entries; SPRINGCRAFT_GEMM3 = 0 takes nothing
    const Gemm3Launch small = with([](Gemm3Launch& l) { l.count = 1023; });
    GemmEnv E_all, E_off;
    E_all.gemm3 = 2;
    E_off.gemm3 = 0;
    CHECK(!gemm3_takes(E, D, small) && gemm3_takes(E_all, D, small) && !gemm3_takes(E_off, D, base));
    CHECK(gemm3_takes(E, D, with([](Gemm3Launch& l) { l.count = 1023; l.dbg.any_size = true; })));
    // lower-only, m = n = 2048: 16 x 32 tiles of which 16 * 15 lie above the diagonal: 272 per record
    GemmEnv E_low0, E_low1;
    E_low0.gemm3_lower = 0;
    E_low1.gemm3_lower = 1;
    auto lower = [&](int count) {
      return Gemm3Launch{.count = count, .m = 2048, .n = 2048, .k = 128, .layout = kGemmAmBn, .lower = 1, .alpha = 1.0, .beta = 1.0, .aligned16 = true};
    };
    CHECK(gemm3_takes(E, D, lower(7)) && !gemm3_takes(E, D, lower(8)) && gemm3_takes(E, Dside, lower(7)) && gemm3_takes(E, Dside, lower(8)));
    CHECK(!gemm3_takes(E_low0, D, lower(7)) && !gemm3_takes(E_low0, Dside, lower(8)));
    CHECK(gemm3_takes(E_low1, D, lower(7)) && gemm3_takes(E_low1, D, lower(8)));
    CHECK(!gemm3_takes(E, D, lower(3)) && gemm3_takes(E, D, lower(4)));   // 816, 1088 tiles
    {
      Gemm3Launch l = lower(8);
      l.dbg.any_size = true;
      CHECK(gemm3_takes(E_low0, D, l));
      // an odd number of column tiles: m = n = 192 has 2 + 3 = 5 tiles; m = n = 256 has 2 + 4 = 6
      l = lower(204); l.m = l.n = 192;
      CHECK(!gemm3_takes(E_low1, D, l));   // 1020
      l.count = 205;
      CHECK(gemm3_takes(E_low1, D, l));    // 1025
      l = lower(170); l.m = l.n = 256; l.lower = 2;
      CHECK(!gemm3_takes(E_low1, D, l));   // 1020
      l.count = 171;
      CHECK(gemm3_takes(E_low1, D, l));    // 1026
    }
    // workgroups and tile order
    auto wgs_is = [](Gemm3Grid g, int nwg, int order) { return g.nwg == nwg && g.order == order; };
    CHECK(wgs_is(gemm3_workgroups(E, D, base), 256, 1) && wgs_is(gemm3_workgroups(E, Dside, base), 256, 1));
    CHECK(wgs_is(gemm3_workgroups(E, D, lower(8)), 256, 1) && wgs_is(gemm3_workgroups(E, Dside, lower(8)), 224, 1));
    CHECK(gemm_wgs_clamp(100) == 96 && gemm_wgs_clamp(4) == 8 && gemm_wgs_clamp(999) == 256 && gemm_wgs_clamp(224) == 224);
    {
      GemmEnv Ew;
      Ew.gemm3_lower_wgs = gemm_wgs_clamp(100);
      Ew.gemm3_order = 0;
      CHECK(wgs_is(gemm3_workgroups(Ew, Dside, lower(8)), 96, 0) && wgs_is(gemm3_workgroups(Ew, D, base), 256, 0));
      CHECK(wgs_is(gemm3_workgroups(Ew, D, with([](Gemm3Launch& l) { l.dbg.order = 1; })), 256, 1));
      CHECK(wgs_is(gemm3_workgroups(E, D, with([](Gemm3Launch& l) { l.dbg.order = 0; })), 256, 0));
    }

    // ---- k_symm3 (SPRINGCRAFT_SYMM3's value, CUs, count, m, split, aligned16, any_size)
    CHECK(!symm3_takes(1, 256, 128, 254, 1, true, false) && !symm3_takes(1, 256, 128, 255, 1, true, false));
    CHECK(symm3_takes(1, 256, 128, 256, 1, true, false) && !symm3_takes(1, 256, 128, 257, 1, true, false));   // 2 x 128 = 256 items
    CHECK(!symm3_takes(1, 256, 128, 256, 0, true, false) && !symm3_takes(1, 256, 128, 256, 17, true, false));
    // m = 256: 16 + 8 = 24 K steps: six slices of 4, seven of 3
    CHECK(symm3_takes(1, 256, 128, 256, 6, true, false) && !symm3_takes(1, 256, 128, 256, 7, true, false));
    CHECK(symm3_takes(1, 256, 8, 3840, 16, true, false));   // 248 K steps: 16 slices of 15; 30 x 16 x 8 items
    // m = 640: 5 tile rows x 51 matrices = 255 items
    CHECK(!symm3_takes(1, 256, 51, 640, 1, true, false) && symm3_takes(1, 256, 52, 640, 1, true, false));
    CHECK(symm3_takes(1, 256, 51, 640, 1, true, /*any_size=*/true) && symm3_takes(2, 256, 51, 640, 1, true, false));
    CHECK(!symm3_takes(0, 256, 128, 256, 1, true, true) && !symm3_takes(1, 255, 128, 256, 1, true, true));
    CHECK(!symm3_takes(1, 256, 128, 256, 1, /*aligned16=*/false, true) && !symm3_takes(1, 256, 0, 256, 1, true, true));
    CHECK(symm3_workgroups(E, false) == 256 && symm3_workgroups(E, true) == 224);
    {
      GemmEnv Ew;
      Ew.symm3_wgs = gemm_wgs_clamp(250);
      CHECK(symm3_workgroups(Ew, false) == 248 && symm3_workgroups(Ew, true) == 248);
    }
    {
      // m = 2000: 125 + 8 = 133 K steps
      int gb[17];
      for (int& g : gb) g = -1;
      symm3_slice_bounds(2000, 5, gb);
      CHECK(gb[0] == 0 && gb[1] == 26 && gb[2] == 53 && gb[3] == 79 && gb[4] == 106 && gb[5] == 133 && gb[6] == -1);
      for (int q = 0; q < 5; ++q) CHECK(gb[q] < gb[q + 1]);
      for (int& g : gb) g = -1;
      symm3_slice_bounds(2000, 1, gb);
      CHECK(gb[0] == 0 && gb[1] == 133 && gb[2] == -1);
      symm3_slice_bounds(256, 16, gb);   // the most slices: all 17 bounds
      CHECK(gb[0] == 0 && gb[1] == 1 && gb[2] == 3 && gb[15] == 22 && gb[16] == 24);
    }
    // the environment is read in one place; unset, it is the default-constructed struct
    if (!getenv("SPRINGCRAFT_GEMM3") && !getenv("SPRINGCRAFT_GEMM3_LOWER_WGS") && !getenv("SPRINGCRAFT_GEMM3_W") &&
        !getenv("SPRINGCRAFT_GEMM2_TILE") && !getenv("SPRINGCRAFT_SYMM3_WGS")) {
      const GemmEnv R = read_gemm_env();
      CHECK(R.gemm3 == 1 && R.gemm3_lower_wgs == 0 && R.gemm3_w && R.gemm2_tile == 0 && R.symm3_wgs == 0);
    }
  }
  std::puts("host logic ok");
  return 0;
}
