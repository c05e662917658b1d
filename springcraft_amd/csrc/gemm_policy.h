// The launch policy of the three float64 GEMM launchers (gemm_f64.hip: k_gemm2; gemm3.hip: k_gemm3; symm3.hip: k_symm3):
// which block tile, grid order, workgroup count and K slices a launch gets, and whether the role-split kernels take it.
// Same rules as twostage_policy.h: every function is a closed-form function of its inputs -- the environment (read once,
// GemmEnv), the debug entries' overrides (GemmOverrides, carried in the launch description), the launch shape and what
// the context knows (GemmDevice) --, no HIP, header-only; tests/host_sanitize/ compiles exactly this code with
// g++ -fsanitize=address,undefined.  The launchers call each function once and launch what it says.
#pragma once
#include <algorithm>
#include <cstdlib>

// which axis of each operand has stride 1 in ALL records of a launch: "NN" (sa_i = 1, sb_k = 1), "TN" (sa_k = 1,
// sb_k = 1), "NT" (sa_i = 1, sb_j = 1)
constexpr int kGemmAmBk = 0, kGemmAkBk = 1, kGemmAmBn = 2;

// One problem of a launch, in device memory (what the fields mean to the kernels: gemm_f64.h).  Here, without HIP, for the
// plans that build records on the host (sy2sb_plan.h); global, as the kernels' signatures name it.
struct GemmDesc {
  const double* a;
  const double* b;
  double* c;
  int m, n, k;
  long long sa_i, sa_k;   // element strides of A(i,k)
  long long sb_k, sb_j;   // element strides of B(k,j)
  long long ldc;          // column stride of C (row stride is 1)
  double alpha, beta;
  const int* a_kidx;      // optional gather on A's k axis: A(i,k) = a[i*sa_i + a_kidx[k]*sa_k]
  const int* b_kidx;      // optional gather on B's k axis: B(k,j) = b[b_kidx[k]*sb_k + j*sb_j]
  const int* c_jidx;      // optional scatter on C's column axis: C(:, j) lives at column c_jidx[j]
  int lower_only;         // 1: store only elements with (row + row_off) >= (col + col_off) (SYR2K); 2: ((row + row_off) | 1) >= ...
  int row_off, col_off;
  long long split_stride; // split-K launches: slice s writes alpha*partial to C + s*split_stride (beta ignored)
  int a_tri;              // launches with tri = true: 1: A(i,k) counts only for i >= k; 2: only for k > i
};

namespace sc_host {
// ---- every SPRINGCRAFT_* value the GEMM launchers read, read once per process.
// (SPRINGCRAFT_SYMM3 is TwoStageEnv's: the band reduction plans with it, symm3_takes receives it)
struct GemmEnv {
  int gemm3 = 1;               // SPRINGCRAFT_GEMM3: 0 never k_gemm3, 2 every launch that qualifies whatever its size
  int gemm3_lower = -1;        // SPRINGCRAFT_GEMM3_LOWER: lower-only launches on k_gemm3 0 never / 1 always (unset: gemm3_takes)
  int gemm3_order = 1;         // SPRINGCRAFT_GEMM3_ORDER: 0 flat tile order, 1 strips
  int gemm3_lower_wgs = 0;     // SPRINGCRAFT_GEMM3_LOWER_WGS: workgroups of a lower-only launch (gemm_wgs_clamp; 0: unset)
  bool gemm3_w = true;         // SPRINGCRAFT_GEMM3_W = 0: W = V^T Z of the Q1 back-transformation stays on k_gemm2
  bool no_balance = false;     // SPRINGCRAFT_GEMM_NO_BALANCE set: natural tile order for triangular-operand launches
  bool no_pair = false;        // SPRINGCRAFT_GEMM_NO_PAIR set: no XCD pairing of launches with 2 - 4 row tiles
  bool no_lower_grid = false;  // SPRINGCRAFT_GEMM_NO_LOWER_GRID set: rectangular grid for lower-only launches
  int gemm2_tile = 0;          // SPRINGCRAFT_GEMM2_TILE: 1 / 2 / 3 = 128 x 128 / 128 x 64 / 64 x 64 for every k_gemm2 launch
  int symm3_wgs = 0;           // SPRINGCRAFT_SYMM3_WGS: workgroups of k_symm3 (gemm_wgs_clamp; 0: unset)
  int symm3_hot = 0;           // SPRINGCRAFT_SYMM3_DBG_HOT: diagnostic bits handed to k_symm3 (results wrong)
};
// a workgroup count from the environment: a multiple of 8 (one per XCD) in 8 .. 256
static inline int gemm_wgs_clamp(int v) { return std::max(8, std::min(256, v / 8 * 8)); }
static inline GemmEnv read_gemm_env() {
  GemmEnv E;
  auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
  E.gemm3 = num("SPRINGCRAFT_GEMM3", 1);
  E.gemm3_lower = num("SPRINGCRAFT_GEMM3_LOWER", -1);
  E.gemm3_order = num("SPRINGCRAFT_GEMM3_ORDER", 1);
  if (const char* e = getenv("SPRINGCRAFT_GEMM3_LOWER_WGS")) E.gemm3_lower_wgs = gemm_wgs_clamp(atoi(e));
  E.gemm3_w = num("SPRINGCRAFT_GEMM3_W", 1) != 0;
  E.no_balance = getenv("SPRINGCRAFT_GEMM_NO_BALANCE") != nullptr;
  E.no_pair = getenv("SPRINGCRAFT_GEMM_NO_PAIR") != nullptr;
  E.no_lower_grid = getenv("SPRINGCRAFT_GEMM_NO_LOWER_GRID") != nullptr;
  E.gemm2_tile = num("SPRINGCRAFT_GEMM2_TILE", 0);
  if (const char* e = getenv("SPRINGCRAFT_SYMM3_WGS")) E.symm3_wgs = gemm_wgs_clamp(atoi(e));
  E.symm3_hot = num("SPRINGCRAFT_SYMM3_DBG_HOT", 0);
  return E;
}
inline const GemmEnv& gemm_env() { static const GemmEnv E = read_gemm_env(); return E; }

// What the debug entries (gemm_debug.hip) ask of ONE launch; everything else leaves it default-constructed.
struct GemmOverrides {
  int force_tile = 0;     // k_gemm2's block tile: 1 = 128 x 128, 2 = 128 x 64, 3 = 64 x 64
  bool any_size = false;  // k_gemm3: take every launch that qualifies, whatever its size
  int order = -1;         // k_gemm3's tile order; -1: SPRINGCRAFT_GEMM3_ORDER
};
// What the context knows about its device and its caller
struct GemmDevice {
  int num_cus;        // 0: not reported
  int gemm3_attr;     // k_gemm3's dynamic LDS: -1 not asked yet, 0 refused (or a launch was), 1 granted
  bool side_by_side;  // the caller runs parts of the batch on several streams (band reduction)
};

// ---- k_gemm2 (launch_gemm_f64; the fields are documented in gemm_f64.h)
struct GemmLaunch {
  int count, max_m, max_n, layout;
  int split_k = 1;
  bool gather = false, tri = false, lower_grid = false;
  int pin_tile = 0;
  GemmOverrides dbg{};
};
struct GemmTile { int bm, bn; };
// Block tile: 128-wide in a dimension when the problem is at least that wide there and the launch still has >= 2
// workgroups per CU, 3 for 128 x 128 (lower-only launches: about half of the square grid does work).  Never 128 x 128 for
// kGemmAkBk: both operands k-contiguous would spill (8 + 8 row offsets on top of 128 accumulator registers).
static inline GemmTile gemm2_tile(const GemmEnv& E, int num_cus, const GemmLaunch& L) {
  const int force = L.dbg.force_tile ? L.dbg.force_tile : E.gemm2_tile ? E.gemm2_tile : L.pin_tile;
  if (force == 1) return {128, L.layout != kGemmAkBk ? 128 : 64};
  if (force == 2) return {128, 64};
  if (force == 3) return {64, 64};
  const long long cus = num_cus > 0 ? num_cus : 256;
  auto blocks = [&](int a, int b) { return (long long)((L.max_m + a - 1) / a) * ((L.max_n + b - 1) / b) * L.count * L.split_k; };
  GemmTile T{64, 64};
  if (L.max_m > 64 && blocks(128, 64) >= 2 * cus) T.bm = 128;
  if (T.bm == 128 && L.max_n > 64 && L.layout != kGemmAkBk && blocks(128, 128) >= 3 * cus) T.bn = 128;
  return T;
}
// Gather launches (the merges of the divide & conquer): 128 x 64 tiles while they fill the chip, else 64 x 64.
// An asymmetry that is kept as it was: only the debug entries' override 2 / 3 picks the instantiation whatever the size;
// SPRINGCRAFT_GEMM2_TILE and pin_tile do not reach this path.
static inline GemmTile gemm2_gather_tile(int num_cus, const GemmLaunch& L) {
  const long long cus = num_cus > 0 ? num_cus : 256;
  const long long gz = (long long)L.count * L.split_k;
  const bool by_size = L.max_m > 64 && (long long)((L.max_m + 127) / 128) * ((L.max_n + 63) / 64) * gz >= 2 * cus;
  const bool big = L.dbg.force_tile == 2 ? true : (L.dbg.force_tile == 3 ? false : by_size);
  return {big ? 128 : 64, 64};
}
// lower_grid (every record square, lower_only, no offsets: the SYR2K of the band reduction) launches only the tiles on and
// below the diagonal -- where the launch is one the triangular walk is written for
static inline bool gemm2_lower_grid_allowed(const GemmEnv& E, const GemmLaunch& L) {
  return L.lower_grid && !E.no_lower_grid && L.layout == kGemmAmBn && !L.tri && !L.gather && L.split_k <= 1 && L.max_m == L.max_n;
}
// grid.z (records x K slices) is limited to 65535: longer record lists go out in chunks of this many records (the D&C
// merges of a batch of some thousand matrices get there)
static inline int gemm2_records_per_launch(int count, int split_k) { return (long long)count * split_k > 65535 ? 65535 / split_k : count; }
// mode 0: natural (x, y, z); 1: lower triangle; 2: longest tiles first, over all records; 3: the row tiles of one B panel
// on one XCD.  (gx, gy, gz): the tile grid the kernel decodes its block index against; (x, y, z): the grid of the launch.
struct GemmGrid { int mode, gx, gy, gz; unsigned x, y, z; };
// In: (x, y, z) = row tiles, column tiles, records x slices of a BM x BN launch; tri: the triangular-operand
// instantiation; lower: gemm2_lower_grid_allowed
static inline GemmGrid gemm2_grid(const GemmEnv& E, int bm, int bn, unsigned x, unsigned y, unsigned z, bool tri, bool lower) {
  if (lower) {   // square launch: only the tiles of the lower triangle, (BM / BN) x (x + 1) / 2 of them per record
    x = (unsigned)((long long)(bm / bn) * x * (x + 1) / 2);
    y = z; z = 1;
  }
  GemmGrid G{lower ? 1 : 0, (int)x, (int)y, (int)z, x, y, z};
  const long long gx = G.gx, gy = G.gy, gz = G.gz;   // (64-bit: gy * gz of a large launch does not fit an int)
  if (tri && !lower && !E.no_balance && (long long)x * y * z < 0x7fffffffLL) {
    G.mode = 2;
    G.x = x * y * z; G.y = 1; G.z = 1;
  }
  if (!tri && !lower && !E.no_pair && gx >= 2 && gx <= 4 && (gy * gz + 8) * gx < 0x7fffffffLL) {
    G.mode = 3;
    G.x = (unsigned)((gy * gz + 7) / 8 * 8 * gx); G.y = 1; G.z = 1;
  }
  return G;
}

// ---- k_gemm3 (launch_gemm3_uniform / gemm3_would_take; the fields are documented in gemm_f64.h)
struct Gemm3Launch {
  int count, m, n, k, layout, lower;
  double alpha, beta;
  bool aligned16;
  GemmOverrides dbg{};
};

// Taken: alpha = 1, beta in {0, 1}, k a multiple of 16 and >= 128, m (and n for kGemmAmBn) even, pointers and leading
// dimensions that keep 16-byte alignment (aligned16: the caller knows its records), enough tiles to give every CU a few.
static inline bool gemm3_takes(const GemmEnv& E, const GemmDevice& D, const Gemm3Launch& L) {
  if (E.gemm3 == 0 || L.count <= 0) return false;
  if (L.layout != kGemmAmBn && L.layout != kGemmAmBk && L.layout != kGemmAkBk) return false;
  if (L.alpha != 1.0 || (L.beta != 0.0 && L.beta != 1.0)) return false;
  if (!L.aligned16 || L.k < 128 || (L.k & 15) || (L.m & 1) || L.m < 2 || L.n < 1) return false;
  if (L.layout == kGemmAmBn && (L.n & 1)) return false;
  if (L.lower && L.m != L.n) return false;
  // (the lower-only trailing update of the band reduction: 0.66 against k_gemm2's 0.65 of the MFMA peak on 32 matrices
  // alone, 192 against 187 ms inside the C3 step -- its diagonal tiles store under lane predicates and its strips start
  // with few tiles --: left to k_gemm2 unless SPRINGCRAFT_GEMM3_LOWER = 1)
  // For a few large matrices it wins (one n = 24000 matrix, config C5: 186 -> 178 ms of trailing updates per solve): there
  // the two half batches on two streams, whose panel QRs hide beside k_gemm2's workgroups, do not exist.
  // Round 6: with the two half batches on two streams (D.side_by_side, set by the band reduction) it takes the
  // update after all -- on 224 workgroups instead of 256, which leaves an eighth of the CUs to the other half's panel QR
  // and small products: C3 step 2200 -> 2150-2160 ms (same box, tools/quick_env_ab.sh: 208 / 216 / 224 workgroups 2157-2177 /
  // 2149-2169 / 2145-2166, 232 / 240: 2190-2210, 256: 2191-2196; profiles/r06_syr2k_wgs.txt).
  if (L.lower && !L.dbg.any_size && (E.gemm3_lower == 0 || (E.gemm3_lower < 0 && L.count >= 8 && !D.side_by_side))) return false;
  // (the kernel's tile order is built on 8 XCDs x 32 workgroups: a device -- or a partition -- with fewer CUs stays on k_gemm2)
  if (D.num_cus < 256 || D.gemm3_attr == 0) return false;
  const long long TM = (L.m + 127) / 128, TN = (L.n + 63) / 64;
  const long long hN = TN / 2;
  const long long T1 = L.lower ? TM * TN - hN * (hN - 1) - ((TN & 1) ? hN : 0) : TM * TN;
  const long long total = T1 * L.count;
  if (E.gemm3 != 2 && !L.dbg.any_size && total < 4LL * 256) return false;   // (SPRINGCRAFT_GEMM3 = 2: for the tests)
  return total <= 0x3fffffffLL;
}

struct Gemm3Grid { int nwg, order; };
// Workgroups: one per CU; a lower-only launch (the band reduction's trailing update) SPRINGCRAFT_GEMM3_LOWER_WGS, else 224
// beside another half batch: fewer than one per CU leaves CUs to the other half's panel QR that runs beside it
static inline Gemm3Grid gemm3_workgroups(const GemmEnv& E, const GemmDevice& D, const Gemm3Launch& L) {
  const int nwg = L.lower ? (E.gemm3_lower_wgs > 0 ? E.gemm3_lower_wgs : (D.side_by_side ? 224 : 256)) : 256;
  return {nwg, L.dbg.order >= 0 ? L.dbg.order : E.gemm3_order};
}

// ---- k_symm3 (launch_symm3 / symm3_would_take): X = A V for `count` symmetric matrices of order m with `split` K slices.
// env_symm3: TwoStageEnv::symm3; any_size: skip the "enough work items" part
static inline bool symm3_takes(int env_symm3, int num_cus, int count, int m, int split, bool aligned16, bool any_size) {
  if (env_symm3 == 0 || count <= 0 || !aligned16) return false;
  if (m < 256 || (m & 1)) return false;
  if (split < 1 || split > 16 || ((m + 15) / 16 + 8) / split < 4) return false;   // (every item has a few K steps)
  if (num_cus < 256) return false;   // (the item order is built on 8 XCDs x 32 workgroups)
  const long long items = (long long)((m + 127) / 128) * split * count;
  if (env_symm3 != 2 && !any_size && items < 256) return false;
  return items <= 0x3fffffffLL;
}
// (workgroups: one per CU, or 224 while the caller runs parts of the batch on several streams -- the other part's panel
// QR and small products then find CUs beside this launch, as for k_gemm3's trailing update; SPRINGCRAFT_SYMM3_WGS)
static inline int symm3_workgroups(const GemmEnv& E, bool side_by_side) {
  return E.symm3_wgs > 0 ? E.symm3_wgs : (side_by_side ? 224 : 256);
}
// K steps of 16 at which slice q starts (gb[split]: the end; split <= 16, symm3_takes).  A last step that reaches beyond
// the matrix takes its pieces from the zeros.
static inline void symm3_slice_bounds(int m, int split, int gb[17]) {
  const int ks_all = (m + 15) / 16 + 8;
  for (int q = 0; q <= split; ++q) gb[q] = (int)((long long)ks_all * q / split);
}

}  // namespace sc_host
