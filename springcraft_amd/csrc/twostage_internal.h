// What twostage.hip (stages 1 and 2, driver, slab layout) and bt2.hip (the Q2 back-transformation) share; everything
// else is in its file.
#pragma once

#include <algorithm>
#include <vector>

#include "eigh_internal.h"
#include "twostage_policy.h"

// (internal linkage: both files get their own copy of the constants and of the device helper, which is always inlined)
namespace {

constexpr int kB = sc_host::kBand;  // band half-width = panel width = reflector length of stage 2
constexpr int kG = 64;            // sweeps per diamond
constexpr int kDiaLd = 128;       // leading dimension of a diamond (kB + kG - 1 = 127 rows used)
constexpr int kDiaSize = kDiaLd * kG;

// sizes of the fragment storage of a diamond (the slab layout needs them; their order and use: bt2.hip)
constexpr int kMiniFrags = 40;                     // fragments per mini: 20 of V^T, 20 of -(V T)
constexpr int kDiaFrags = 4 * kMiniFrags;          // 160 per diamond
constexpr int kFragDoubles = kDiaFrags * 64;       // 10240 doubles = 80 KB

typedef double __attribute__((address_space(1)))* gdptr;          // global memory: global_load / global_store, never flat
// a pointer every lane of the wave holds the same value of, told so to the compiler (scalar registers, and memory
// instructions of the form scalar base + 32-bit lane offset instead of a 64-bit address per access)
__device__ __forceinline__ gdptr wave_uniform(double* p) {
  const unsigned long long b = (unsigned long long)(size_t)p;
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
  return (gdptr)(size_t)(((unsigned long long)hi << 32) | (unsigned long long)lo);
}

}  // namespace

// Diamond offsets per sweep group (shared by all matrices of the batch): host copy, (ngroups + 1) ints.
inline std::vector<int> dia_offsets(int n) {
  const int nsweep = std::max(n - 2, 0);
  const int ng = (nsweep + kG - 1) / kG;
  std::vector<int> off((size_t)ng + 1, 0);
  for (int S = 0; S < ng; ++S) off[(size_t)S + 1] = off[(size_t)S] + (n - 1 - S * kG + kB - 1) / kB;
  return off;
}
