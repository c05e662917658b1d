// Host-only logic of the conformational-ensemble entries (springcraft_amd/csrc/ensemble_policy.h, scratch_arena.h) under
// AddressSanitizer + UBSan:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I springcraft_amd/csrc \
//       tests/host_sanitize/test_ensemble_logic.cpp -o /tmp/test_ensemble_logic && /tmp/test_ensemble_logic
// (built and run by tests/test_ensemble_host.py::test_ensemble_logic_under_sanitizers).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ensemble_policy.h"
#include "scratch_arena.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); std::exit(1); } } while (0)

using namespace sc_host;

// a carved layout: every buffer inside the block, 256-byte aligned, none overlapping the next; the block is written end to end
template <typename Layout>
static void check_layout(const Layout& layout, const std::vector<size_t>& bytes_of) {
  Arena measure;
  layout(measure);
  std::vector<char> block(measure.bytes());
  Arena carve(block.data(), block.size());
  const std::vector<char*> ptrs = layout(carve);
  CHECK(!carve.overrun() && carve.bytes() == measure.bytes() && ptrs.size() == bytes_of.size());
  for (size_t i = 0; i < ptrs.size(); ++i) {
    CHECK(ptrs[i] != nullptr);
    CHECK((size_t)(ptrs[i] - block.data()) % 256 == 0);
    CHECK(ptrs[i] + bytes_of[i] <= block.data() + block.size());
    if (i + 1 < ptrs.size()) CHECK(ptrs[i] + (bytes_of[i] ? bytes_of[i] : 1) <= ptrs[i + 1]);
    for (size_t b = 0; b < bytes_of[i]; ++b) ptrs[i][b] = (char)i;   // (ASan: inside the block)
  }
}

int main() {
  // ---- the form switch
  CHECK(parse_superpose_env(nullptr) == kSuperposeEnvAuto && parse_superpose_env("") == kSuperposeEnvAuto);
  CHECK(parse_superpose_env("auto") == kSuperposeEnvAuto && parse_superpose_env("nonsense") == kSuperposeEnvAuto);
  CHECK(parse_superpose_env("lds") == kSuperposeEnvLds && parse_superpose_env("stream") == kSuperposeEnvStream);
  CHECK(read_superpose_env() == kSuperposeEnvAuto);   // (the test runs it without the variable)
  for (int env : {kSuperposeEnvAuto, kSuperposeEnvLds}) {
    CHECK(superpose_form(env, 1) == kSuperposeFormLds && superpose_form(env, 2000) == kSuperposeFormLds);
    CHECK(superpose_form(env, kSuperposeLdsMaxAtoms) == kSuperposeFormLds);
    CHECK(superpose_form(env, kSuperposeLdsMaxAtoms + 1) == kSuperposeFormStream);
    CHECK(superpose_form(env, 50000) == kSuperposeFormStream);
  }
  CHECK(superpose_form(kSuperposeEnvStream, 1) == kSuperposeFormStream);
  CHECK(superpose_form(kSuperposeEnvStream, 50000) == kSuperposeFormStream);
  // the LDS form fits the 64 KB a kernel gets without asking; N = 2000 is 48 KB of frame
  CHECK(superpose_lds_bytes(kSuperposeLdsMaxAtoms) <= 65536 && superpose_lds_bytes(kSuperposeLdsMaxAtoms + 118) > 65536);
  CHECK(superpose_lds_bytes(2000) == 48000 + 8 * (size_t)kSuperposeRedDoubles);
  CHECK(superpose_frame_bytes(kSuperposeFormLds, 2000) == 96000 && superpose_frame_bytes(kSuperposeFormStream, 50000) == 4800000);

  // ---- scratch of the superposition and the mean
  check_layout([](Arena& a) { return std::vector<char*>{(char*)superpose_layout(a).target_centre}; }, {32});
  CHECK(mean_chunks(1) == 1 && mean_chunks(64) == 1 && mean_chunks(65) == 2 && mean_chunks(10000) == 157);
  for (long long m : {1LL, 64LL, 65LL, 1000LL})
    for (long long n : {1LL, 7LL, 257LL})
      check_layout([&](Arena& a) { return std::vector<char*>{(char*)mean_layout(a, m, n).partial}; },
                   {(size_t)mean_chunks(m) * 3 * (size_t)n * 8});

  // ---- the PCA plan: route, order, slices, lower triangle
  {
    PcaPlan P = pca_plan(5, 7, 4, 256);            // Gram, tiny
    CHECK(P.route == kPcaGram && P.order == 5 && P.k_len == 21 && P.split_k == 1 && !P.lower_grid && !P.full);
    P = pca_plan(40, 7, 15, 256);                  // covariance
    CHECK(P.route == kPcaCovariance && P.order == 21 && P.k_len == 40 && P.split_k == 1 && P.lower_grid && !P.full);
    P = pca_plan(22, 7, 15, 256);                  // the boundary M - 1 = 3 N: covariance
    CHECK(P.route == kPcaCovariance && P.order == 21);
    P = pca_plan(21, 7, 15, 256);                  // one frame fewer: Gram
    CHECK(P.route == kPcaGram && P.order == 21);
    P = pca_plan(1000, 2000, 20, 256);             // Gram, 16 x 16 tiles, K = 6000: 11 slices
    CHECK(P.route == kPcaGram && P.order == 1000 && P.k_len == 6000 && P.split_k == 11 && !P.lower_grid);
    P = pca_plan(10000, 2000, 20, 256);            // covariance of order 6000: enough tiles, lower triangle
    CHECK(P.route == kPcaCovariance && P.order == 6000 && P.split_k == 1 && P.lower_grid);
    P = pca_plan(100000, 7, 15, 256);              // a short result with a long K axis: slices, no lower grid
    CHECK(P.route == kPcaCovariance && P.split_k == 32 && !P.lower_grid);
    P = pca_plan(100000, 7, 21, 0);                // all components of the covariance; a device that reports no CUs
    CHECK(P.full && P.split_k == 32);
  }
  // ---- scratch of the PCA: each carve sized from its own takes
  const size_t desc = 136;
  const long long cases[][3] = {{5, 7, 4}, {40, 7, 15}, {22, 7, 12}, {65, 64, 64}, {1000, 2000, 20}, {100000, 7, 21}};
  for (const auto& c : cases) {
    const long long m = c[0], n = c[1], k = c[2];
    const PcaPlan P = pca_plan(m, n, k, 256);
    const size_t n3 = 3 * (size_t)n, ord = (size_t)P.order;
    const std::vector<size_t> bytes = {(size_t)m * n3 * 8, (size_t)m * 8, ord * ord * 8,
                                       P.split_k > 1 ? (size_t)P.split_k * ord * ord * 8 : 0, (size_t)k * 8,
                                       (size_t)k * ord * 8, P.route == kPcaGram ? (size_t)k * n3 * 8 : 0, 2 * desc};
    if (m * n > 1000000) {   // (measured only: the block would be gigabytes)
      size_t least = 0;
      for (size_t b : bytes) least += b;
      CHECK(pca_scratch_bytes(P, m, n, k, desc) >= least);
      continue;
    }
    check_layout([&](Arena& a) {
      const PcaBufs B = pca_layout(a, P, m, n, k, desc);
      return std::vector<char*>{(char*)B.xc, (char*)B.frame_ss, (char*)B.mat, (char*)B.slices, (char*)B.evals,
                                (char*)B.evecs, (char*)B.raw, B.descs};
    }, bytes);
    Arena measure;
    pca_layout(measure, P, m, n, k, desc);
    CHECK(pca_scratch_bytes(P, m, n, k, desc) == measure.bytes());
  }
  std::printf("ensemble logic ok\n");
  return 0;
}
