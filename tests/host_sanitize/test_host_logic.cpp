// Host-only logic of the C ABI (springcraft_amd/csrc/host_logic.h, scratch_arena.h) under AddressSanitizer + UBSan:
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
  std::puts("host logic ok");
  return 0;
}
