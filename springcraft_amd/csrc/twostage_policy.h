// The policy of the two-stage tridiagonalisation: which kernel form a given (n, batch, device) gets.  Every rule is a
// closed-form function of integers -- the environment (read once, TwoStageEnv), the context's overrides and what the
// runtime answered (occupancy, granted attributes) are INPUTS.  No HIP, header-only, same rules as host_logic.h:
// tests/host_sanitize/ compiles exactly this code with g++ -fsanitize=address,undefined.  sy2sb.hip, sb2st.hip, twostage.hip
// and bt2.hip call each function once per solve (or per panel) and launch what it says; the measurements that justify a
// rule stand beside it.  The float64 GEMMs every stage launches have their policy and environment in gemm_policy.h.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <vector>

#if defined(__HIPCC__)
#define SC_POLICY_HD __host__ __device__
#else
#define SC_POLICY_HD
#endif

namespace sc_host {

constexpr int kBand = 64;              // band half-width = panel width = reflector length of stage 2 (kB of the kernels)
constexpr int kWgRows1024 = 4 * 1024;  // tallest panel of k_panel_wg with 1024 threads (4 rows per thread)
constexpr int kWgRows512 = 12 * 512;   // ... with 512 threads (12 rows per thread)
constexpr int kCoopRows = 256;         // rows of a panel per workgroup of k_panel_coop
constexpr int kCoopMaxG = 128;         // most workgroups per matrix of k_panel_coop
constexpr int kEarlyRing = 8;          // early hand-off records per sweep of k_bulge_chase (16 bytes each)
constexpr size_t kLdsPerWorkgroup = 160 * 1024;   // LDS of a CU: the most one workgroup can be launched with

static inline size_t policy_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// tasks of sweep s of an order-n band (one per 64 rows the bulge is chased through)
SC_POLICY_HD inline int chase_len(int n, int s) { return (n - 1 - s + kBand - 1) / kBand; }

// ---- every SPRINGCRAFT_* value the two-stage path reads, read once per process; those of its GEMM
// launches (SPRINGCRAFT_GEMM*, SPRINGCRAFT_SYMM3_WGS): GemmEnv, gemm_policy.h
struct TwoStageEnv {
  int symm3 = 1;                    // SPRINGCRAFT_SYMM3: 0 never k_symm3, 2 every launch that qualifies
  int symm_split = 0;               // SPRINGCRAFT_SYMM_SPLIT: 1 .. 16 K slices of the SYMM (0: automatic)
  bool panel_pairs = true;          // SPRINGCRAFT_PANEL_PAIRS = 0: one trailing update per panel
  bool qr_blocked = true;           // SPRINGCRAFT_QR_UNBLOCKED set: chunked panel QR without the inner blocks
  int qr_wg = -1;                   // SPRINGCRAFT_QR_WG: 0 always chunked launches, 1 k_panel_wg up to 4096 rows only
  int qr_coop = 1;                  // SPRINGCRAFT_QR_COOP = 0: never k_panel_coop
  int qr_coop_min = 0;              // SPRINGCRAFT_QR_COOP_MIN: rows from which a panel takes it (0: by matrix count)
  int stage1_streams = 0;           // SPRINGCRAFT_STAGE1_STREAMS: parts of the batch in the band reduction (0: automatic)
  int bulge_persistent = 1;         // SPRINGCRAFT_BULGE_PERSISTENT: 0 off, 1 by size, 2 always
  int bulge_pair = -1;              // SPRINGCRAFT_BULGE_PAIR: 0 never the pair form, 2 for every persistent chase
  long long bulge_pair_max = 6000;  // SPRINGCRAFT_BULGE_PAIR_MAX: upper end (batch n / 128) of the pair form's range
  int bulge_spread = -1;            // SPRINGCRAFT_BULGE_SPREAD: 0 never, 1 for every chase with fewer matrices than XCDs
  bool bulge_no_early = false;      // SPRINGCRAFT_BULGE_NO_EARLY set: k_bulge_chase without the early hand-off records
  int bulge_streams = 0;            // SPRINGCRAFT_BULGE_STREAMS: parts of the batch of the per-wavefront launches
  int bulge_burst = 32;             // SPRINGCRAFT_BULGE_BURST: launches per stream burst
  int bt2_wave = -1;                // SPRINGCRAFT_BT2_WAVE: 0 never / 1 always one launch per wavefront of diamonds
  int bt2_nw = 0;                   // SPRINGCRAFT_BT2_NW: 4 / 8 waves of k_bt2_apply
};

static inline TwoStageEnv read_two_stage_env() {
  TwoStageEnv E;
  auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
  E.symm3 = num("SPRINGCRAFT_SYMM3", 1);
  E.symm_split = num("SPRINGCRAFT_SYMM_SPLIT", 0);
  E.panel_pairs = num("SPRINGCRAFT_PANEL_PAIRS", 1) != 0;
  E.qr_blocked = getenv("SPRINGCRAFT_QR_UNBLOCKED") == nullptr;
  E.qr_wg = num("SPRINGCRAFT_QR_WG", -1);
  E.qr_coop = num("SPRINGCRAFT_QR_COOP", 1);
  if (const char* e = getenv("SPRINGCRAFT_QR_COOP_MIN")) E.qr_coop_min = std::max(2 * kBand, atoi(e));
  E.stage1_streams = num("SPRINGCRAFT_STAGE1_STREAMS", 0);
  E.bulge_persistent = num("SPRINGCRAFT_BULGE_PERSISTENT", 1);
  E.bulge_pair = num("SPRINGCRAFT_BULGE_PAIR", -1);
  if (const char* e = getenv("SPRINGCRAFT_BULGE_PAIR_MAX")) E.bulge_pair_max = atoll(e);
  E.bulge_spread = num("SPRINGCRAFT_BULGE_SPREAD", -1);
  E.bulge_no_early = getenv("SPRINGCRAFT_BULGE_NO_EARLY") != nullptr;
  E.bulge_streams = num("SPRINGCRAFT_BULGE_STREAMS", 0);
  E.bulge_burst = std::max(1, num("SPRINGCRAFT_BULGE_BURST", 32));
  E.bt2_wave = num("SPRINGCRAFT_BT2_WAVE", -1);
  E.bt2_nw = num("SPRINGCRAFT_BT2_NW", 0);
  return E;
}
// the process's instance (symm3.hip takes its SPRINGCRAFT_SYMM3 from here too)
inline const TwoStageEnv& two_stage_env() {
  static const TwoStageEnv E = read_two_stage_env();
  return E;
}

// ================================================================================================================
// Stage 1

// Parts of the batch that run the band reduction side by side on separate streams: the latency-bound panel QR of one part
// runs beside the GEMMs of the other (618 -> 591 ms per step at 64 matrices).  A profiled solve keeps everything on one
// stream, because the kernel-group times (panel_qr / symm / syr2k) are event brackets on that stream: its band reduction
// is therefore about 30 ms longer than in an unprofiled solve.
// THE one place that knows: whether k_panel_coop may run (whole batch on one stream only) and for which record count a
// panel's SYMM form is decided (the smallest part) follow from this number -- the parts of a split batch must not be
// factored or multiplied by different kernels (other reduction trees / summation orders, other last bits), or the same
// structure at two batch positions gives different eigenvalues; found by tools/test_matrix.sh with three parts of unequal
// size, profiles/r06_test_matrix.txt.
static inline int stage1_parts(const TwoStageEnv& E, int batch, bool profiled) {
  const int want = E.stage1_streams > 0 ? E.stage1_streams : ((batch >= 32 && !profiled) ? 2 : 1);
  return std::max(1, std::min(want, std::min(batch, 4)));
}

// panels of the band reduction of an order-n matrix
static inline int panel_count(int n) {
  int npanels = 0;
  while (n - (npanels + 1) * kBand >= 2) ++npanels;
  return npanels;
}
// Role of every panel: 0 single, 1 first of a pair, 2 second of a pair.
// Panels are taken in PAIRS where the trailing matrix is large enough: the second panel of a pair is factored from
// columns that received the first panel's update alone (record kRecFirst of sy2sb_plan.h), its X = A22 V2 is computed from
// the NOT yet updated trailing matrix and corrected by - [V1|W1] ([W1|V1]^T V2) (records kRecP2, kRecCorr), and one
// trailing update (kRecTrail)
// A22 -= [V1|W1|V2|W2] [W1|V1|W2|V2]^T (K = 256) serves both panels: the lower triangle is read and written once per
// 128 columns of band instead of once per 64 (at K = 128 the C traffic of a tile takes as long as its MFMAs).
static inline std::vector<int> panel_roles(const TwoStageEnv& E, int n) {
  const int npanels = panel_count(n);
  std::vector<int> role((size_t)npanels, 0);
  if (E.panel_pairs)
    for (int p = 0; p + 1 < npanels;) {
      const int m2 = n - (p + 2) * kBand;
      if (m2 >= 4 * kBand) { role[(size_t)p] = 1; role[(size_t)p + 1] = 2; p += 2; }
      else ++p;
    }
  return role;
}

// Whether the band reduction of order-n matrices runs its SYMM on k_symm3 (symm3.hip; the launcher may still decline a
// panel -- too few tiles late in the reduction -- which then takes the two triangular-operand launches)
static inline bool symm3_for(const TwoStageEnv& E, int n) { return E.symm3 != 0 && n >= 512 && (n & 1) == 0; }

// K slices of the SYMM X = A22 V: with few matrices its launch has only n / 64 tiles per matrix, each walking a K range of
// up to n (longest first, but the longest IS the critical path): slices of the K range give the launch 2 - 8 times the
// workgroups and a fraction of the critical path.  Config C5 (one 24000 x 24000 matrix): 596 -> 307 ms.
static inline int symm_split_for(const TwoStageEnv& E, int n, int batch) {
  if (E.symm_split >= 1) return std::min(E.symm_split, 16);
  if (symm3_for(E, n)) {
    // k_symm3: a work item is (128-row tile, K slice), all of equal length; 256 persistent workgroups want a few rounds
    // of them (a launch holds half the batch from 32 matrices on: the two half batches run on two streams)
    const long long items = (long long)((n + 127) / 128) * (batch >= 32 ? batch / 2 : batch);
    // (C5, one n = 24000 matrix = 188 tile rows, tools/r06_cfgs.sh: 3 / 4 / 5 / 6 / 8 slices 1143 / 1114 / 1105 / 1092 / 1083 ms)
    if (items >= 768) return 1;
    return (int)std::min<long long>(16, (1536 + items - 1) / items);
  }
  const long long tiles = (long long)batch * ((n + 63) / 64);
  if (tiles >= 1024 || n < 2048) return 1;
  // (one 24000 x 24000 matrix: 3 slices 338 ms, 6 slices 307 ms, 8 slices 378 ms of SYMM time)
  // Round 5, same matrix, `tools/r05_symm_sweep.sh`: 4 slices 407 ms, 5: 312, 6: 325, 7: 299, 8: 395, 9: 285, 10: 295,
  // 12: 303 -- slice counts that share a factor with the 8 XCDs put the same slice of every tile on the same XCD (the
  // workgroups are dealt round-robin) and with it the long K ranges of the triangle: ODD counts spread them.  Nine where six
  // were taken (at most 409 tiles: one large matrix or a few); the smaller counts of larger launches are unchanged
  // (n = 6000, one to four matrices: 6, 7 and 9 slices within 1 %).
  // The middle regime follows the same rule (`tools/r05_symm_mid.sh`, 6 x n = 6000 = 564 tiles: 4 slices 38.9 ms of SYMM
  // per step, 5 slices 31.0): an even count takes the next odd one.
  // (ceil(2048 / tiles) is 3 for 683 .. 1023 tiles, 4 for 512 .. 682, 5 for 410 .. 511, 6 and more below: the only even
  // count the rule replaces is the measured 4 -> 5)
  const long long s0 = std::min<long long>(6, (2048 + tiles - 1) / tiles);
  return s0 >= 6 ? 9 : (s0 == 4 ? 5 : (int)s0);
}

// ---- the cooperative panel kernel (k_panel_coop) for tall panels of a few matrices: SPRINGCRAFT_QR_COOP = 0 keeps the
// chunked launches, SPRINGCRAFT_QR_COOP_MIN = rows from which a panel takes it (default: above k_panel_wg's range)
// (one matrix, per panel: 0.77 ms by the chunked launches whatever the height, 0.3 - 0.5 ms by k_panel_wg's single
// workgroup, 0.25 - 0.3 ms here -- C5: panel QR 289 -> 109 ms, a single n = 6000 matrix: 52 -> 23 ms.  With four and more
// matrices the single-workgroup kernels run them side by side and keep their range; the taller panels come here)
struct CoopPlan {
  bool ask;        // the solve may use the kernel: raise its LDS attribute (once per context) ...
  int nb_max;      // ... and, when that was granted and nb_max >= 1, reserve and zero its records
  int min_few;     // rows from which a panel of fewer than four matrices takes it
  int min_many;    // ... of four and more matrices
  int budget;      // workgroups of one launch (every workgroup waits for all others: well below the CUs of the device)
  int gmax;        // workgroups per matrix of the tallest panel
};
// coop_min_rows (sc_dbg_set_panel_coop): > 0 rows from which panels take it, 0 never, < 0 the environment decides;
// coop_ok: 0 once a launch of this context ran into its time-out
static inline CoopPlan coop_plan(const TwoStageEnv& E, int n, int batch, int num_cus, bool profiled, int coop_min_rows,
                                 int coop_ok) {
  CoopPlan C{};
  C.min_few = coop_min_rows > 0 ? coop_min_rows : (E.qr_coop_min > 0 ? E.qr_coop_min : 300);
  C.min_many = coop_min_rows > 0 ? coop_min_rows : (E.qr_coop_min > 0 ? E.qr_coop_min : kWgRows512 + 1);
  C.budget = num_cus * 3 / 4;
  C.gmax = (std::max(n - kBand, 1) + kCoopRows - 1) / kCoopRows;
  // (only when the whole batch runs on one stream: see stage1_parts)
  C.ask = (coop_min_rows > 0 || (coop_min_rows < 0 && E.qr_coop != 0)) && coop_ok != 0 &&
          n - kBand >= std::min(C.min_few, C.min_many) && C.gmax <= kCoopMaxG && stage1_parts(E, batch, profiled) == 1;
  C.nb_max = std::min(batch, C.budget / C.gmax);
  return C;
}

// Panel QR of the m rows below the band, nb matrices on one stream.
enum class PanelQr {
  Coop,       // k_panel_coop, coop_g workgroups per matrix (+ k_panel_serial, the take-over)
  Wg1024,     // k_panel_wg<ru, cu>: one workgroup of 1024 threads per matrix
  Wg512,      // k_panel_wg<ru, 1, 512>
  Blocked,    // chunked launches, inner blocks of 8 columns (k_panel_qr, k_pqr_blk_a / b)
  Unblocked,  // chunked launches, one per column (k_panel_qr)
};
struct PanelQrForm {
  PanelQr kind;
  int ru, cu;   // template arguments of k_panel_wg
  int coop_g;   // workgroups per matrix of k_panel_coop
};
// have_recs: the solve reserved k_panel_coop's records (coop_plan); main_stream: the launch goes to the solve's own stream
static inline PanelQrForm panel_qr_form(const TwoStageEnv& E, const CoopPlan& C, bool have_recs, int m, int nb,
                                        bool main_stream) {
  PanelQrForm F{PanelQr::Unblocked, 0, 0, (m + kCoopRows - 1) / kCoopRows};
  const bool full = std::min(kBand, m - 1) == kBand;   // a panel of 64 reflectors
  // (one workgroup per matrix while the panel is short enough for its rows to sit in the registers of 1024 threads --
  // also for a single matrix: N = 512 two-stage 45 -> 37 ms; SPRINGCRAFT_QR_WG = 0 keeps the chunked launches)
  // (round 4: panels of 4097 .. 6144 rows -- the first 29 of n = 6000 -- by 512 threads with up to 12 rows each: twice
  // the registers per thread; SPRINGCRAFT_QR_WG = 1 keeps them on the chunked launches)
  const bool use_wg = full && m <= kWgRows1024 && E.qr_wg != 0;
  // (not for a few matrices: one workgroup streams its panel at the rate of ONE CU -- a single N = 2000 structure's
  // panel QRs take 70 instead of 52 ms that way)
  const bool use_wg512 = full && !use_wg && m <= kWgRows512 && E.qr_wg != 0 && E.qr_wg != 1 && nb >= 4;
  const bool use_coop = have_recs && full && m >= (nb < 4 ? C.min_few : C.min_many) && nb * F.coop_g <= C.budget && main_stream;
  if (use_coop) {
    F.kind = PanelQr::Coop;
  } else if (use_wg) {
    F.kind = PanelQr::Wg1024;
    const int ru = (m + 1023) / 1024;
    F.ru = ru <= 1 ? 1 : std::min(ru, 4);
    F.cu = ru <= 2 ? 8 : (ru == 3 ? 4 : 2);
  } else if (use_wg512) {
    F.kind = PanelQr::Wg512;
    F.ru = (m + 511) / 512 <= 10 ? 10 : 12;
    F.cu = 1;
  } else if (full && E.qr_blocked) {
    F.kind = PanelQr::Blocked;
  }
  return F;
}

// ================================================================================================================
// Stage 2

enum class ChaseForm {
  Stepwise,  // one launch of k_bulge_step per wavefront of tasks
  Sweep,     // k_bulge_chase<0>: one launch, one sweep per workgroup, a matrix confined to one XCD
  Spread,    // k_bulge_chase<1>: the same with the workgroups of a matrix on all XCDs
  Pair,      // k_bulge_pair: two sweeps per workgroup
};
// Which form (profiles/r04_bulge_sweep.txt, batch x n: pair / one sweep per workgroup / per-wavefront launches, ms):
// 16 x 6000: 126 / 115 / 169, 32 x 3000: 63 / 56 / 82, 64 x 3000: 92 / 99 / 124, 32 x 6000: 182 / 223 / 256,
// 64 x 6000: 335 / 435 / 436.  While the stage is latency-bound (batch * n / 128 <= 1100) one sweep per workgroup has
// the shorter dependent chain; above that the stage is bound by bytes and the pair form moves half of them.  With
// fewer matrices than XCDs (a matrix is confined to one XCD) only while the order is moderate: a single n = 24000
// matrix chases 1.6 x faster with its ~188 tasks per wavefront spread over the whole chip (411 vs 676 ms).
// nxcd: XCDs of the device (counted by a probe launch); pair_attr: the device grants k_bulge_pair its dynamic LDS;
// chase_mode / chase_form (sc_dbg_set_chase): < 0 the environment / the size decides, else SPRINGCRAFT_BULGE_PERSISTENT's
// value / 0 one sweep per workgroup, 1 pair, 2 spread; chase_ok: 0 once a chase of this context ran into its time-out (it
// is not asked again: every further attempt could cost another bound's worth of spinning before the fallback).
static inline ChaseForm chase_form_for(const TwoStageEnv& E, int n, int batch, int nxcd, int num_cus, bool pair_attr,
                                       int chase_mode, int chase_form, int chase_ok) {
  const int persist = chase_mode >= 0 ? chase_mode : E.bulge_persistent;
  const long long work = (long long)batch * n / 128;
  // SPRINGCRAFT_BULGE_PAIR = 0: never the pair form, 2: the pair form for every persistent chase (tests), else by size
  // (by size only inside the measured range -- profiles/r04_bulge_sweep.txt up to 64 x 6000, profiles/r05_bulge_sweep_ext.txt
  // up to 96 x 6000 and 256 x 3000, B n / 128 = 6000: the pair form wins everywhere there (622 vs 742 / 775 ms, 354 vs
  // 467 / 558) -- and only while every matrix of an XCD has a pair workgroup of its own (one per CU): 512 x 1026 puts 64
  // matrices on the 32 CUs of an XCD, a workgroup then walks the matrices one after the other, 687 ms against 110 by
  // the per-wavefront launches.  ADVICE round 4.)
  const bool pair_measured = work <= E.bulge_pair_max && (batch + nxcd - 1) / nxcd <= std::max(1, num_cus / nxcd);
  const bool pair = chase_form >= 0 ? (chase_form == 1 && pair_attr)
                                    : E.bulge_pair != 0 && pair_attr &&
                                          (E.bulge_pair == 2 || (work > 1100 && batch >= 8 && pair_measured));
  // Round 6, "spread": a few LARGE matrices (fewer than XCDs, n > 4500 -- config C5's single n = 24000 matrix has ~188
  // tasks per wavefront, three times the workgroups one XCD holds) are chased by k_bulge_chase<1> from ALL XCDs, their
  // band handed on by write-through stores; until round 5 the largest took one launch per wavefront.  One matrix on one XCD
  // against all XCDs, bulge chasing in ms (tools/spread_sweep.py, profiles/r06_spread_chase.txt): n = 2100 24.3 / 26.4, 3000
  // 35.2 / 38.2, 4200 54.0 / 53.4, 6000 84.2 / 76.9 (2 and 4 matrices: 86 / 78), 9000 144.6 / 116.3, 12000 195.6 / 156.3, 24000
  // (per-wavefront launches) 418 / 318.  SPRINGCRAFT_BULGE_SPREAD = 0 / 1: never / for every chase with fewer matrices than
  // XCDs (tests).
  // (debug entry sc_dbg_set_chase: mode 5 forces it, modes 3 / 4 keep it off)
  const bool spread = !pair && batch < nxcd &&
                      (chase_form == 2 || (chase_form < 0 && E.bulge_spread != 0 && (E.bulge_spread == 1 || n > 4500)));
  // ---- persistent chase (one launch, sweeps claimed dynamically) while the stage is latency-bound; else, or with
  // SPRINGCRAFT_BULGE_PERSISTENT = 0, one launch per wavefront
  const bool want_chase = persist == 2 || (persist == 1 && (pair || spread || (work <= 2800 && (batch >= 8 || n <= 6144))));
  if (!(want_chase && num_cus > 0 && (chase_ok != 0 || persist == 2))) return ChaseForm::Stepwise;
  return pair ? ChaseForm::Pair : (spread ? ChaseForm::Spread : ChaseForm::Sweep);
}

// The launch of a persistent chase.  per_cu: workgroups of the form's kernel one CU holds (the occupancy query; 0: failed).
struct ChaseLaunch {
  int nxcd;             // XCDs as the kernel counts them
  int W;                // workgroups per matrix; 0: no launch (per-wavefront launches instead)
  int grid;             // workgroups of the launch
  size_t prog_bytes;    // progress counters (batch x n)
  size_t next_bytes;    // claim counters (batch)
  size_t early_bytes;   // early hand-off records of k_bulge_chase (0: none)
};
static inline ChaseLaunch chase_launch(const TwoStageEnv& E, ChaseForm form, int n, int batch, int nxcd_device, int num_cus,
                                       int per_cu) {
  const bool pair = form == ChaseForm::Pair;
  ChaseLaunch L{};
  // XCDs of this device: the kernels bind matrix b to XCD b mod nxcd (an MI355X in SPX mode has 8 XCDs of 32 CUs; a
  // partition of it has fewer, and a matrix bound to an XCD that is not there would never be claimed)
  // (counted on the device, not derived from the CU count: ADVICE round 4)
  L.nxcd = form == ChaseForm::Spread ? 1 : nxcd_device;   // (spread: every workgroup counts as "XCD 0" and serves every matrix)
  const int slots_per_xcd = per_cu * num_cus / L.nxcd;
  const int mpx = (batch + L.nxcd - 1) / L.nxcd;   // matrices per XCD (XCD 0 has the most)
  // workgroups per matrix: all the XCD's slots divided by its matrices, but no more than sweeps can be in flight
  // (every sweep trails its predecessor by two tasks; a pair its predecessor pair by three steps)
  const int useful = pair ? std::max(4, chase_len(n, 0) / 3 + 2) : std::max(8, chase_len(n, 0) / 2 + 1);
  L.W = slots_per_xcd > 0 ? std::max(1, std::min(useful, slots_per_xcd / mpx)) : 0;
  // the dispatcher deals workgroups round-robin over the XCDs, so 8 x (workgroups one XCD needs) gives every XCD
  // its share; the kernel does not rely on it (a short-changed XCD is just slower, see the kernel's header)
  L.grid = L.nxcd * std::min(slots_per_xcd, mpx * L.W);
  L.prog_bytes = policy_align_up((size_t)batch * n * sizeof(int), 256);
  L.next_bytes = policy_align_up((size_t)batch * sizeof(int), 256);
  // (16 B x kEarlyRing per sweep; zeroed with the counters: a stale tag of the previous solve would pass for this one's)
  L.early_bytes = (pair || E.bulge_no_early) ? 0 : policy_align_up((size_t)batch * n * kEarlyRing * 16, 256);
  return L;
}

// Parts of the batch whose per-wavefront launches run on separate streams: the launches of one chase are strictly ordered
// and every one of them ends with a partly filled last round of workgroups, so the tail of one part's launch is filled by
// the next launch of another part.
// (three parts from 48 matrices on: 477 -> 431 ms at 64; four and more exceed the ~11 us per launch one host thread
// needs -- the stage then takes 48 k launches x 11.4 us --, and replaying the launches as a captured hipGraph is slower
// still: 569 ms with three parts)
static inline int bulge_stream_parts(const TwoStageEnv& E, int batch) {
  const int want = E.bulge_streams > 0 ? E.bulge_streams : (batch >= 48 ? 3 : (batch >= 16 ? 2 : 1));
  return std::max(1, std::min(want, std::min(batch, 8)));
}
// launches go out in bursts of 32 wavefronts per stream rather than alternating streams launch by launch: the host
// needs ~11-13 us per launch and three parts x 12 k launches are close to the stage's own time (451 -> 434 ms with
// bursts of 16; round 3, same-box A/B on two boxes: 8 / 16 / 32 / 64 -> 465 / 464 / 421 / 463 and 437-467 / 430-434)
static inline int bulge_burst(const TwoStageEnv& E) { return E.bulge_burst; }

// ================================================================================================================
// Stage-2 back-transformation
struct Bt2Plan {
  bool wave;            // k_bt2_wave: one launch per wavefront of independent diamonds (few columns: partial spectrum)
  int nw;               // else k_bt2_apply<nw>: 8 waves (128 columns per workgroup) when that still gives every CU a
                        // workgroup, else 4 (64 columns)
  int nchunk;           // column chunks of 16 nw
  bool xcd;             // workgroups dealt to the XCDs by matrix (one grid dimension); else a (chunk, matrix) grid
  unsigned grid_x, grid_y;
};
static inline Bt2Plan bt2_plan(const TwoStageEnv& E, int n, int batch, int ncols, int num_cus) {
  (void)n;
  Bt2Plan P{};
  const long long col_wgs = (long long)((ncols + 63) / 64) * batch;
  P.wave = E.bt2_wave >= 0 ? E.bt2_wave != 0 : col_wgs <= 16;
  const int cus = num_cus > 0 ? num_cus : 256;
  P.nw = ((long long)((ncols + 127) / 128) * batch >= cus) ? 8 : 4;
  if (E.bt2_nw == 4 || E.bt2_nw == 8) P.nw = E.bt2_nw;
  P.nchunk = (ncols + 16 * P.nw - 1) / (16 * P.nw);
  P.xcd = batch >= 8;
  P.grid_x = P.xcd ? (unsigned)(8 * ((batch + 7) / 8) * P.nchunk) : (unsigned)P.nchunk;
  P.grid_y = P.xcd ? 1u : (unsigned)batch;
  return P;
}

}  // namespace sc_host
