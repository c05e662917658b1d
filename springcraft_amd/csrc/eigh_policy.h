// The top-level policy of the eigensolver (eigh.hip, tridiag.hip): panel width, one-stage or two-stage tridiagonalisation,
// what runs on the second stream.  Same form as twostage_policy.h: no HIP, header-only, the environment read once into a
// struct that is then an INPUT; tests/host_sanitize/test_eigh_policy.cpp compiles exactly this code with
// g++ -fsanitize=address,undefined.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "twostage_policy.h"

namespace sc_host {

// ---- every SPRINGCRAFT_* value the drivers and the one-stage tridiagonalisation read
struct EighEnv {
  // Tridiagonalisation panel width nb (SYR2K inner dimension K = 2 nb).  Measured on MI355X, N = 2000 C-alpha,
  // 16 structures in flight (profiles/r01_panel_width.txt): nb = 64: SYR2K 32.2 TFLOP/s (41 % of the 78.6 TFLOP/s
  // f64-MFMA peak), 57.8k modes/s; nb = 96: 36.5 TFLOP/s (46 %), 56.8k; nb = 128: 38.3 TFLOP/s (49 %), 55.4k
  // (wider panels make the per-column kernels read more V / W).
  int nb = 64;                  // SPRINGCRAFT_NB = 32|64|96|128
  int two_stage = -1;           // SPRINGCRAFT_TWO_STAGE = 0 / 1: force the one-stage / two-stage path
  bool no_aux = false;          // SPRINGCRAFT_NO_AUX set: nothing on the second stream
  int aux_single = -1;          // SPRINGCRAFT_AUX_SINGLE = 0 / 1: one structure never / always forks
  int resident = -1;            // SPRINGCRAFT_RESIDENT = 0: never k_sytrd_resident
  int resident_wgs = 0;         // SPRINGCRAFT_RESIDENT_WGS: its workgroups (0: by size)
  int resident_max = 0;         // SPRINGCRAFT_RESIDENT_MAX: largest trailing order it takes (0: the default)
  bool resident_no_chain = false;   // SPRINGCRAFT_RESIDENT_NO_CHAIN set (diagnostic): its launches are not chained by an event
  int resident_delay = 24;      // SPRINGCRAFT_RESIDENT_DELAY: pause before a step's first poll, units of 64 cycles
};

static inline EighEnv read_eigh_env() {
  EighEnv E;
  auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
  const int nb = num("SPRINGCRAFT_NB", 64);
  E.nb = (nb == 128 || nb == 96 || nb == 64 || nb == 32) ? nb : 64;
  E.two_stage = num("SPRINGCRAFT_TWO_STAGE", -1);
  E.no_aux = getenv("SPRINGCRAFT_NO_AUX") != nullptr;
  E.aux_single = num("SPRINGCRAFT_AUX_SINGLE", -1);
  E.resident = num("SPRINGCRAFT_RESIDENT", -1);
  E.resident_wgs = num("SPRINGCRAFT_RESIDENT_WGS", 0);
  E.resident_max = num("SPRINGCRAFT_RESIDENT_MAX", 0);
  E.resident_no_chain = getenv("SPRINGCRAFT_RESIDENT_NO_CHAIN") != nullptr;
  E.resident_delay = num("SPRINGCRAFT_RESIDENT_DELAY", 24);
  return E;
}
// the process's instance
inline const EighEnv& eigh_env() {
  static const EighEnv E = read_eigh_env();
  return E;
}

// Two-stage tridiagonalisation (twostage.hip and the files it names) instead of the one-stage panel algorithm.  The one-stage SYMV streams
// 4/3 n^3 bytes per matrix and is bandwidth-bound as soon as a few matrices are in flight; the two-stage path does its
// O(n^3) work in MFMA GEMMs but pays ~3 n short launches and twice the back-transformation flops.  Measured crossover
// on MI355X: batch * n^2 above ~ max(1.7e7, 5e3 n) (round 4: max(2e7, 1e4 n), round 2: 5e7 + 6.7e3 n, round 1: 1.2e8;
// profiles/r0*_two_stage_crossover.txt).
// ctx_mode: sc_ctx_set_two_stage (1 / 0 force it on / off, < 0: SPRINGCRAFT_TWO_STAGE decides); resident: a one-matrix
// solve of this context goes to k_sytrd_resident (tridiag.hip:resident_enabled).
static inline bool two_stage_for(const EighEnv& E, int ctx_mode, bool resident, int n, int batch) {
  const int mode = ctx_mode >= 0 ? ctx_mode : E.two_stage;
  if (n < 4 * kBand) return false;
  if (mode == 0) return false;
  if (mode == 1) return true;
  // round 4 (tools/crossover.py, profiles/r04_two_stage_crossover.txt; panel QR in one workgroup, the persistent chase
  // with two workgroups per CU and the secular solver of round 3 moved it down again): n = 6000 from 2 matrices (a tie
  // there), 3000 from 4, 1500 from ~8, 1026 and 513 with large batches (513 x 256: 49 vs 63 ms); one matrix at a time
  // stays on the one-stage path up to n ~ 12000 (n = 6000: 192 vs 237 ms, 3000: 67 vs 82)
  // round 5 (profiles/r05_two_stage_crossover.txt; the panel QR of a few matrices by several workgroups of one launch,
  // k_panel_coop): one matrix ties at n = 4500 (124 vs 122 ms) and n = 6000 (191 vs 187), two-stage from there on (7500:
  // 310 vs 273, 9000: 441 vs 360, 12000: 856 vs 581); 2 x 4500: 157 vs 133, 8 x 1500: 43.5 vs 39.5
  // round 6 (profiles/r06_two_stage_crossover.txt): ONE matrix whose trailing 3072 columns k_sytrd_resident reduces in
  // one launch stays on the one-stage path up to n ~ 7000 (n = 3000: 32 vs 71 ms, 5100: 110 vs 142, 6000: 152 vs 178,
  // 6600: 196 vs 201, 7200: 233 vs 230, 7800: 285 vs 263)
  if (batch == 1 && resident) return n > 7000;
  return n >= 512 && (double)batch * n * n >= std::max(1.7e7, 5.0e3 * n);
}

// What a solve with eigenvectors runs beside the D&C on the context's second stream.
enum class AuxPlan {
  None,          // nothing: the back-transformation prepares after the D&C, on the main stream
  TFactorsMain,  // two-stage with SPRINGCRAFT_NO_AUX: the diamonds' T factors on the main stream, before the D&C
  Fork,          // the back-transformations' preparation (and the T factors, two-stage) on the second stream
};
// two: the plan's tridiagonalisation is the two-stage one; resident: as for two_stage_for
static inline AuxPlan aux_plan(const EighEnv& E, bool two, int batch, bool resident) {
  if (E.no_aux) return two ? AuxPlan::TFactorsMain : AuxPlan::None;
  // (one structure on the one-stage path with its launches per column: the fork / join costs more than the overlap
  // brings, 30.0 -> 31.3 ms at N = 512)
  // (round 6: one structure whose tridiagonalisation is the single launch of k_sytrd_resident forks as well -- the T
  // factors' 0.6 ms beside a D&C of 2 ms: N = 100 2.46 -> 1.88 ms, N = 512 9.23 -> 8.69; SPRINGCRAFT_AUX_SINGLE = 0 / 1)
  const bool single_fork = E.aux_single >= 0 ? E.aux_single != 0 : (batch == 1 && resident);
  return (two || batch >= 4 || single_fork) ? AuxPlan::Fork : AuxPlan::None;
}

}  // namespace sc_host
