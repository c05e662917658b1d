// Grouped / batched float64 GEMM on the gfx950 matrix cores (v_mfma_f64_16x16x4_f64).
//
//     C[i,j] = beta * C[i,j] + alpha * sum_k A(i,k) * B(k,j)          (column-major C, ldc)
//
// A(i,k) = a[i*sa_i + k*sa_k + (a_kidx ? a_kidx[k]*sa_k ... see below)], B(k,j) = b[k*sb_k + j*sb_j]:
// arbitrary strides, so NN / NT / TN products and sub-matrix views need no copies.  One of
// (sa_i, sa_k) and one of (sb_k, sb_j) must be 1 (the loader runs its lanes along that axis).
//
// alpha must not be 0 when beta != 0: the kernel carries beta * C through its accumulators as (beta / alpha) * C and
// would store 0 instead of beta * C.  No caller scales C alone; the debug entries refuse such a record.
//
// Problems are described by GemmDesc records in DEVICE memory, so sizes may be produced by a
// previous kernel (the divide & conquer merges: the number of non-deflated eigenvalues is only
// known on the device).  blockIdx.z selects the record; blocks outside m x n exit at once.
#pragma once

#include <cstdint>

#include "common.h"
#include "gemm_policy.h"
// (GemmDesc, the record of one problem, lives in gemm_policy.h beside GemmLaunch: the plans that build records need it without HIP)

// One launch of `count` problems (records d_desc[0..count)) on k_gemm2; max_m / max_n bound the grid.  The policy --
// block tile, grid order, chunks of at most 65535 records x slices -- is gemm_policy.h's.
// layout (no default, every caller names it): kGemmAmBk / kGemmAkBk / kGemmAmBn, the records live in device memory.
// split_k > 1: every record is cut into split_k K-slices (all records of a launch share it).
// gather: the records carry a_kidx / b_kidx lists (D&C merges; layout kGemmAmBk only).
// tri: the records carry a_tri masks (lower-stored symmetric A; band reduction; layouts kGemmAmBk / kGemmAkBk), no gathers.
// lower_grid: every record of the launch is square, lower_only with row_off = col_off = 0 (the SYR2K of the band
// reduction): only the tiles on and below the diagonal are launched (layout kGemmAmBn, no split-K).
// pin_tile: 0 = the block tile follows the launch size; 1 / 2 / 3 = 128 x 128 / 128 x 64 / 64 x 64 whatever the size, for
// callers that cut one piece of work into several launches and want every piece to round alike (gemm_f64_tile returns
// the code the size rule picks for a launch).
// dbg: the debug entries' overrides (gemm_debug.hip); every other caller leaves it alone.
using sc_host::GemmLaunch, sc_host::Gemm3Launch, sc_host::GemmOverrides;
int launch_gemm_f64(sc_ctx* ctx, const GemmDesc* d_desc, const GemmLaunch& L);
int gemm_f64_tile(const sc_ctx* ctx, int count, int max_m, int max_n, int layout);
// (what the policy needs to know of a context)
inline sc_host::GemmDevice gemm_device(const sc_ctx* ctx) { return {ctx->num_cus, ctx->gemm3_attr, ctx->gemm3_side_by_side}; }

// The role-split persistent kernel k_gemm3 (gemm3.hip) for launches whose `count` records share (m, n, k): returns SC_OK
// when it took the launch, 1 when the launch is not one it takes (the caller then uses launch_gemm_f64).  alpha must be 1
// and beta 0 or 1 -- callers fold a sign into an operand --; aligned16: every operand pointer and leading dimension of
// the records keeps 16-byte alignment (the host built them).  SPRINGCRAFT_GEMM3 = 0 switches it off, = 2 takes every
// launch that qualifies whatever its size (tests).
// lower: 0 all of C; 1 the lower triangle (as lower_only = 1 with row_off = col_off = 0, m == n); 2 as lower_only = 2.
int launch_gemm3_uniform(sc_ctx* ctx, const GemmDesc* d_desc, const Gemm3Launch& L);
// (the launcher's decision without the launch: callers that lay out their records differently for the two kernels)
bool gemm3_would_take(sc_ctx* ctx, const Gemm3Launch& L);

// The symmetric product X = A V (A lower stored, V and X with 64 columns) of the band reduction on k_symm3 (symm3.hip):
// SC_OK when it took the launch, 1 when the launch is not one it takes (m even and >= 256, 16-byte aligned operands,
// enough tiles; SPRINGCRAFT_SYMM3 = 0 switches it off, = 2 takes every launch that qualifies).  split: K slices, slice s
// into c + s * split_stride.  The kernel reads A where (row | 1) >= col: see its header for what the writers of A keep.
// any_size: skip the "enough work items" part of the decision (the caller made it with symm3_would_take for another
// record count -- the parts of a split batch --, or is a debug entry).
int launch_symm3(sc_ctx* ctx, const GemmDesc* d_desc, int count, int m, int split, bool aligned16, bool any_size);
bool symm3_would_take(sc_ctx* ctx, int count, int m, int split, bool aligned16);
