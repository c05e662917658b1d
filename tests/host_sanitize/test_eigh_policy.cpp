// The eigensolver's top-level policy (springcraft_amd/csrc/eigh_policy.h) under AddressSanitizer + UBSan:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I springcraft_amd/csrc \
//       tests/host_sanitize/test_eigh_policy.cpp -o /tmp/test_eigh_policy && /tmp/test_eigh_policy
// (built and run by tests/test_abi_and_host.py::test_eigh_policy_under_sanitizers, which clears the SPRINGCRAFT_* variables
// read here).  Every expected value is a literal worked out by hand from the rule in words, with kBand = 64: the context's
// mode (>= 0) beats the environment's; below 4 kBand never, mode 0 never, mode 1 always; else one matrix that
// k_sytrd_resident takes from n > 7000, everything else from n >= 512 and batch n^2 >= max(1.7e7, 5e3 n).  The second
// stream: nothing with SPRINGCRAFT_NO_AUX (two-stage: the T factors on the main stream); else a fork for two-stage, for
// four and more matrices, and for one matrix as SPRINGCRAFT_AUX_SINGLE says (any batch) or, unset, when it is resident.
#include <cstdio>
#include <cstdlib>

#include "eigh_policy.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); std::exit(1); } } while (0)

using namespace sc_host;

int main() {
  static_assert(kBand == 64, "the literals below are for a band of 64");

  // ---- the environment: defaults, then what read_eigh_env makes of set variables
  {
    const EighEnv E = read_eigh_env();
    CHECK(E.nb == 64 && E.two_stage == -1 && !E.no_aux && E.aux_single == -1);
    CHECK(E.resident == -1 && E.resident_wgs == 0 && E.resident_max == 0 && !E.resident_no_chain && E.resident_delay == 24);
  }
  setenv("SPRINGCRAFT_NB", "96", 1);
  CHECK(read_eigh_env().nb == 96);
  setenv("SPRINGCRAFT_NB", "100", 1);
  CHECK(read_eigh_env().nb == 64);
  setenv("SPRINGCRAFT_NB", "32", 1);
  CHECK(read_eigh_env().nb == 32);
  setenv("SPRINGCRAFT_NB", "128", 1);
  CHECK(read_eigh_env().nb == 128);
  unsetenv("SPRINGCRAFT_NB");
  setenv("SPRINGCRAFT_TWO_STAGE", "1", 1);
  setenv("SPRINGCRAFT_NO_AUX", "", 1);   // (set or not)
  setenv("SPRINGCRAFT_AUX_SINGLE", "0", 1);
  setenv("SPRINGCRAFT_RESIDENT", "0", 1);
  setenv("SPRINGCRAFT_RESIDENT_WGS", "256", 1);
  setenv("SPRINGCRAFT_RESIDENT_MAX", "2048", 1);
  setenv("SPRINGCRAFT_RESIDENT_NO_CHAIN", "1", 1);
  setenv("SPRINGCRAFT_RESIDENT_DELAY", "0", 1);
  {
    const EighEnv E = read_eigh_env();
    CHECK(E.nb == 64 && E.two_stage == 1 && E.no_aux && E.aux_single == 0);
    CHECK(E.resident == 0 && E.resident_wgs == 256 && E.resident_max == 2048 && E.resident_no_chain && E.resident_delay == 0);
  }

  // ---- one-stage or two-stage
  const EighEnv unset{};
  EighEnv env1{}, env0{};
  env1.two_stage = 1;
  env0.two_stage = 0;
  // forced on: from 4 kBand = 256, never below
  CHECK(!two_stage_for(unset, 1, false, 255, 1) && two_stage_for(unset, 1, false, 256, 1));
  CHECK(!two_stage_for(env1, -1, true, 255, 64) && two_stage_for(env1, -1, true, 256, 1));
  // forced off
  for (int n : {1, 255, 256, 6000, 20000}) {
    CHECK(!two_stage_for(unset, 0, false, n, 1) && !two_stage_for(unset, 0, true, n, 64) && !two_stage_for(env0, -1, false, n, 64));
    CHECK(!two_stage_for(env1, 0, false, n, 64));   // the context's mode beats the environment's
  }
  CHECK(two_stage_for(env0, 1, false, 300, 1));
  CHECK(two_stage_for(env1, -1, false, 300, 1) && two_stage_for(env1, -1, true, 300, 1));
  // automatic, one matrix that k_sytrd_resident takes: n > 7000
  CHECK(!two_stage_for(unset, -1, true, 7000, 1) && two_stage_for(unset, -1, true, 7001, 1));
  // automatic, one matrix otherwise: n^2 >= 5e3 n from n = 5000 on (4999^2 = 24 990 001 < 24 995 000; 25e6 = 25e6, the >= edge)
  CHECK(!two_stage_for(unset, -1, false, 4999, 1) && two_stage_for(unset, -1, false, 5000, 1));
  // automatic, four matrices: 4 * 2061^2 = 16 990 884 < 1.7e7 <= 17 007 376 = 4 * 2062^2 (resident plays no part in a batch)
  CHECK(!two_stage_for(unset, -1, false, 2061, 4) && two_stage_for(unset, -1, false, 2062, 4));
  CHECK(!two_stage_for(unset, -1, true, 2061, 4) && two_stage_for(unset, -1, true, 2062, 4));
  CHECK(two_stage_for(unset, -1, true, 6000, 4));   // (tests/test_batched_configs_gpu.py asserts this one on the device)
  // automatic, n = 512: 64 * 512^2 = 16 777 216 < 1.7e7 <= 17 039 360 = 65 * 512^2; below 512 never
  CHECK(!two_stage_for(unset, -1, false, 512, 64) && two_stage_for(unset, -1, false, 512, 65));
  CHECK(!two_stage_for(unset, -1, false, 511, 1000000));

  // ---- the second stream
  EighEnv no_aux{}, single0{}, single1{};
  no_aux.no_aux = true;
  single0.aux_single = 0;
  single1.aux_single = 1;
  CHECK(aux_plan(unset, true, 1, false) == AuxPlan::Fork && aux_plan(unset, true, 64, true) == AuxPlan::Fork);
  CHECK(aux_plan(no_aux, true, 1, false) == AuxPlan::TFactorsMain && aux_plan(no_aux, true, 64, true) == AuxPlan::TFactorsMain);
  CHECK(aux_plan(unset, false, 3, false) == AuxPlan::None);
  CHECK(aux_plan(unset, false, 4, false) == AuxPlan::Fork);
  CHECK(aux_plan(unset, false, 1, true) == AuxPlan::Fork);
  CHECK(aux_plan(unset, false, 1, false) == AuxPlan::None);
  CHECK(aux_plan(unset, false, 2, true) == AuxPlan::None);   // (resident is the one-matrix kernel)
  CHECK(aux_plan(single0, false, 1, true) == AuxPlan::None);
  CHECK(aux_plan(single0, false, 4, true) == AuxPlan::Fork && aux_plan(single0, true, 1, true) == AuxPlan::Fork);
  CHECK(aux_plan(single1, false, 2, false) == AuxPlan::Fork);
  CHECK(aux_plan(no_aux, false, 64, true) == AuxPlan::None);

  std::printf("eigh policy ok\n");
  return 0;
}
