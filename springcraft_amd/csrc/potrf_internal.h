// Declarations shared by potrf.hip, subsystem.hip and api_potrf.hip; the host decisions are potrf_policy.h's.
#pragma once
#include "common.h"
#include "potrf_policy.h"

// word of sc_ctx::d_status a failed factorisation stores 1 + the matrix' number in (sc_collect_events keeps it for
// sc_deferred_status)
constexpr int kStatusPotrf = 11;
constexpr int kTrsmForward = 0, kTrsmBackward = 1, kTrsmRight = 2;

size_t potrf_desc_bytes();
int potrf_outer_block(int64_t n);   // sc_host::potrf_outer_block with SPRINGCRAFT_POTRF_OUTER
// d_a (batch matrices, lower, column-major, ld, stride) <- L; d_info (batch) int64: 0, or 1 + the failing column.  Enqueue only.
int launch_potrf(sc_ctx* ctx, const sc_host::PotrfBufs& B, double* d_a, int64_t n, int64_t ld, int64_t stride,
                 int64_t batch, int outer, long long* d_info);
// One pass of block substitution with the factor d_l.  kTrsmForward / kTrsmBackward: d_b (n, vectors) column-major <-
// L^-1 d_b / L^-T d_b; kTrsmRight: d_b (vectors, n) column-major <- d_b L^-T.  pass: 0 inverts the factor's diagonal blocks
// into B.dinv first; 1 (the second half of a `both` solve) reuses them and takes the second half of B.descs.  Enqueue only.
int launch_trsm(sc_ctx* ctx, const sc_host::TrsmBufs& B, int pass, int kind, const double* d_l, int64_t n, int64_t ld,
                int64_t stride, int64_t batch, double* d_b, int64_t vectors, int64_t ldb, int64_t strideb);

// ---- subsystem.hip -----------------------------------------------------------------------------------------------------------
// One path for one structure and for many: `batch` members with n_s system atoms each and environments of up to env_order
// atoms, inputs packed back to back (h_members: the host records, staged into B.members); a single structure is a batch of
// one with env_order = n_e.  ms = dim n_s, me = dim env_order.
//
// d_hss (batch, ms, ms), d_hes (batch, me, ms) row-major and d_hee (batch, me, me) of the partitioned networks from the ordered
// pair lists; a member with a smaller environment gets diag(H_ee, I) and zero pad rows of H_es.  d_group int32: 0 system, 1
// environment; d_pos int32: the atom's place in its group; d_ism (batch, n_s) or null: 1 / sqrt(mass) of the system atoms.
// Every entry of every slot is written; no atomics; enqueue only.
int launch_subsystem_assembly(sc_ctx* ctx, const sc_host::BatchBlocksBufs& B, const sc_host::SubMember* h_members,
                              int64_t batch, int64_t max_pairs, const double* d_coord, int dim, const int64_t* d_pairs,
                              const double* d_gamma, const int64_t* d_row_start, const int32_t* d_group,
                              const int32_t* d_pos, int64_t n_s, int64_t env_order, const double* d_ism, double* d_hss,
                              double* d_hes, double* d_hee);
// Every slot: d_hee <- L (lower, column-major), d_hes <- Y = L^-1 H_es (me, ms) row-major, d_hss <- H_eff = H_ss - Y^T Y,
// mirrored.  One batched factorisation, one batched substitution, one grouped product, one mirror.
int launch_subsystem_reduction(sc_ctx* ctx, const sc_host::BatchReduceBufs& B, double* d_hss, double* d_hes, double* d_hee,
                               int64_t ms, int64_t me, int64_t batch, int outer, long long* d_info);
// One slot: d_xe (q, me) <- -L^-T (Y x_s) for the q rows d_xs (q, ms)
int launch_subsystem_follow(sc_ctx* ctx, const sc_host::FollowBufs& B, const double* d_l, const double* d_y, int64_t ms,
                            int64_t me, const double* d_xs, int64_t q, double* d_xe);
