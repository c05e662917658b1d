// C ABI (include/springcraft_hip.h), device-pointer entries of the Cholesky solver (potrf.hip) and of the subsystem reduction
// on it (subsystem.hip): argument checks before anything is launched, the scratch carve, the launcher calls.
#include "api_internal.h"
#include "potrf_internal.h"

namespace {

int potrf_shape_check(sc_ctx* ctx, const char* what, int64_t n, int64_t ld, int64_t stride, int64_t batch) {
  if (n <= 0 || batch <= 0)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: the order and the batch must be positive, got n = %lld, batch = %lld", what,
                        (long long)n, (long long)batch);
  if (n > sc_host::kPotrfMaxOrder || batch > 65535)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: at most order %lld and 65535 matrices", what,
                        (long long)sc_host::kPotrfMaxOrder);
  if (ld < n)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: the leading dimension %lld is below the order %lld", what, (long long)ld,
                        (long long)n);
  if (batch > 1 && stride < ld * (n - 1) + n)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: the matrix stride %lld is below the %lld elements of a matrix", what,
                        (long long)stride, (long long)(ld * (n - 1) + n));
  return SC_OK;
}

}  // namespace

extern "C" {

int sc_dev_potrf_workspace(int64_t n, int64_t batch, size_t* bytes) {
  if (!bytes || n <= 0 || batch <= 0 || n > sc_host::kPotrfMaxOrder || batch > 65535) return SC_ERR_INVALID_ARG;
  *bytes = sc_host::potrf_scratch_bytes(n, batch, potrf_outer_block(n), potrf_desc_bytes());
  return SC_OK;
}

int sc_dev_potrf_f64(sc_ctx* ctx, double* d_a, int64_t n, int64_t ld, int64_t stride, int64_t batch, int64_t* d_info) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(potrf_shape_check(ctx, "potrf", n, ld, stride, batch));
  if (!d_a || !d_info) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "potrf: the matrices and the info words are required");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const int outer = potrf_outer_block(n);
  const size_t records = sc_host::potrf_record_count(sc_host::potrf_plan(n, outer), batch);
  sc_host::PotrfBufs B{};
  SC_TRY(carve_scratch(ctx, [&](sc_host::Arena& a) { B = sc_host::potrf_layout(a, n, batch, records, potrf_desc_bytes()); }));
  SC_TRY(launch_potrf(ctx, B, d_a, n, ld, stride, batch, outer, (long long*)d_info));
  return sc_stage_end(ctx);
}

int sc_dev_potrs_f64(sc_ctx* ctx, const double* d_l, int64_t n, int64_t ld, int64_t stride, int64_t batch, double* d_b,
                     int64_t q, int64_t ldb, int64_t strideb, int mode) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(potrf_shape_check(ctx, "potrs", n, ld, stride, batch));
  if (mode != sc_host::kPotrsForward && mode != sc_host::kPotrsBackward && mode != sc_host::kPotrsBoth)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "potrs: mode must be 0 (forward), 1 (backward) or 2 (both), got %d", mode);
  if (q < 0 || q > 0x7fffffffLL / 64)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "potrs: the number of right-hand sides must lie in 0 .. %lld", 0x7fffffffLL / 64);
  if (ldb < n)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "potrs: the leading dimension %lld of the right-hand sides is below the order %lld",
                        (long long)ldb, (long long)n);
  if (batch > 1 && q > 0 && strideb < ldb * (q - 1) + n)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "potrs: the stride %lld of the right-hand sides is below their %lld elements",
                        (long long)strideb, (long long)(ldb * (q - 1) + n));
  if (!d_l || (q > 0 && !d_b)) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "potrs: the factor and the right-hand sides are required");
  if (q == 0) return SC_OK;
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const bool both = mode == sc_host::kPotrsBoth;
  sc_host::TrsmBufs B{};
  SC_TRY(carve_scratch(ctx, [&](sc_host::Arena& a) { B = sc_host::trsm_layout(a, n, batch, q, both ? 2 : 1, potrf_desc_bytes()); }));
  if (mode != sc_host::kPotrsBackward)
    SC_TRY(launch_trsm(ctx, B, 0, kTrsmForward, d_l, n, ld, stride, batch, d_b, q, ldb, strideb));
  if (mode != sc_host::kPotrsForward)
    SC_TRY(launch_trsm(ctx, B, both ? 1 : 0, kTrsmBackward, d_l, n, ld, stride, batch, d_b, q, ldb, strideb));
  return sc_stage_end(ctx);
}

int sc_dev_subsystem_blocks_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs,
                                int64_t k, const double* d_gamma, const int64_t* d_row_start, const int32_t* d_group,
                                const int32_t* d_pos, int64_t n_s, int64_t n_e, const double* d_inv_sqrt_mass, double* d_hss,
                                double* d_hes, double* d_hee) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (dim != 1 && dim != 3) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem: dim must be 1 or 3, got %d", dim);
  if (n_s <= 0 || n_e <= 0 || n_s + n_e != n_atoms || k < 0)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem: %lld system and %lld environment atoms (both positive) must make up the %lld atoms; k must not be negative",
                        (long long)n_s, (long long)n_e, (long long)n_atoms);
  if (n_atoms > 0x7fffffffLL / 3) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem: at most %lld atoms", 0x7fffffffLL / 3);
  if (!d_group || !d_pos || !d_hss || !d_hes || !d_hee || (dim == 3 && !d_coord))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem: a required pointer is NULL");
  if (k > 0 && (!d_pairs || !d_gamma || !d_row_start))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem: pairs, gamma and row starts are required with k > 0");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (k == 0) {   // no spring at all: three zero blocks (the row starts may be absent, so the atom kernel must not run)
    const size_t ms = (size_t)dim * (size_t)n_s, me = (size_t)dim * (size_t)n_e;
    SC_HIP(ctx, hipMemsetAsync(d_hss, 0, sizeof(double) * ms * ms, ctx->stream));
    SC_HIP(ctx, hipMemsetAsync(d_hes, 0, sizeof(double) * me * ms, ctx->stream));
    SC_HIP(ctx, hipMemsetAsync(d_hee, 0, sizeof(double) * me * me, ctx->stream));
    return SC_OK;
  }
  // one structure is a batch of one whose slot is exactly its environment
  const sc_host::SubMember one{0, n_atoms, 0, k, n_e};
  sc_host::BatchBlocksBufs B{};
  SC_TRY(carve_scratch(ctx, [&](sc_host::Arena& a) { B = sc_host::batch_blocks_layout(a, 1); }));
  SC_TRY(launch_subsystem_assembly(ctx, B, &one, 1, k, d_coord, dim, d_pairs, d_gamma, d_row_start, d_group, d_pos, n_s, n_e,
                                   d_inv_sqrt_mass, d_hss, d_hes, d_hee));
  return sc_stage_end(ctx);
}

int sc_dev_subsystem_reduce_f64(sc_ctx* ctx, double* d_hss, double* d_hes, double* d_hee, int64_t ms, int64_t me,
                                int64_t* d_info) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (ms <= 0 || me <= 0 || ms > sc_host::kPotrfMaxOrder || me > sc_host::kPotrfMaxOrder)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem: the orders of the system and the environment must be positive");
  if (!d_hss || !d_hes || !d_hee || !d_info) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem: a required pointer is NULL");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const int outer = potrf_outer_block(me);
  sc_host::BatchReduceBufs B{};
  SC_TRY(carve_scratch(ctx, [&](sc_host::Arena& a) { B = sc_host::batch_reduce_layout(a, me, ms, 1, outer, potrf_desc_bytes()); }));
  SC_TRY(launch_subsystem_reduction(ctx, B, d_hss, d_hes, d_hee, ms, me, 1, outer, (long long*)d_info));
  return sc_stage_end(ctx);
}

int sc_dev_subsystem_follow_f64(sc_ctx* ctx, const double* d_l, const double* d_y, int64_t ms, int64_t me, const double* d_xs,
                                int64_t q, double* d_xe) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (ms <= 0 || me <= 0 || ms > sc_host::kPotrfMaxOrder || me > sc_host::kPotrfMaxOrder)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem: the orders of the system and the environment must be positive");
  if (q <= 0 || q > 0x7fffffffLL / 64)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem: the number of rows must lie in 1 .. %lld", 0x7fffffffLL / 64);
  if (!d_l || !d_y || !d_xs || !d_xe) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem: a required pointer is NULL");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  sc_host::FollowBufs B{};
  SC_TRY(carve_scratch(ctx, [&](sc_host::Arena& a) { B = sc_host::follow_layout(a, me, q, potrf_desc_bytes()); }));
  SC_TRY(launch_subsystem_follow(ctx, B, d_l, d_y, ms, me, d_xs, q, d_xe));
  return sc_stage_end(ctx);
}

int sc_dev_vsa_batch_workspace(int dim, int64_t n_s, int64_t env_order, int64_t batch, size_t* bytes) {
  if (!bytes || sc_host::sub_batch_shape_error(dim, n_s, env_order, batch)) return SC_ERR_INVALID_ARG;
  const int64_t me = sc_host::sub_slot_order(dim, env_order);
  *bytes = sc_host::batch_reduce_scratch_bytes(me, dim * n_s, batch, potrf_outer_block(me), potrf_desc_bytes());
  return SC_OK;
}

int sc_dev_vsa_batch_blocks_f64(sc_ctx* ctx, const int64_t* members, int64_t batch, int dim, int64_t n_s, int64_t env_order,
                                const double* d_coord, const int64_t* d_pairs, const double* d_gamma,
                                const int64_t* d_row_start, const int32_t* d_group, const int32_t* d_pos,
                                const double* d_inv_sqrt_mass, double* d_hss, double* d_hes, double* d_hee) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  static const char* const kRule[] = {"", "dim must be 1 or 3", "the system needs at least one atom",
                                      "the batch must hold 1 .. 65535 members", "env_order must not be negative",
                                      "the orders exceed the solver's limit"};
  if (const int e = sc_host::sub_batch_shape_error(dim, n_s, env_order, batch))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem batch: %s (dim = %d, n_s = %lld, env_order = %lld, batch = %lld)", kRule[e],
                        dim, (long long)n_s, (long long)env_order, (long long)batch);
  if (!members) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem batch: the member records are required");
  static_assert(sizeof(sc_host::SubMember) == 5 * sizeof(int64_t), "the C ABI passes a member as five int64");
  const sc_host::SubMember* mem = reinterpret_cast<const sc_host::SubMember*>(members);
  const int64_t bad = sc_host::sub_batch_member_error(mem, batch, n_s, env_order);
  if (bad >= 0)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem batch: member %lld does not fit (n_atoms = %lld, n_e = %lld with n_s = %lld and env_order = %lld, %lld pairs, offsets %lld / %lld)",
                        (long long)bad, (long long)mem[bad].n_atoms, (long long)mem[bad].n_e, (long long)n_s, (long long)env_order,
                        (long long)mem[bad].n_pairs, (long long)mem[bad].atom0, (long long)mem[bad].pair0);
  const int64_t total_pairs = mem[batch - 1].pair0 + mem[batch - 1].n_pairs;
  if (mem[batch - 1].atom0 + mem[batch - 1].n_atoms > 0x7fffffffLL / 3)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem batch: at most %lld atoms in all", 0x7fffffffLL / 3);
  if (!d_row_start || !d_group || !d_pos || !d_hss || (env_order > 0 && (!d_hes || !d_hee)) || (dim == 3 && !d_coord))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem batch: a required pointer is NULL");
  if (total_pairs > 0 && (!d_pairs || !d_gamma))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem batch: pairs and gamma are required with pairs");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  sc_host::BatchBlocksBufs B{};
  SC_TRY(carve_scratch(ctx, [&](sc_host::Arena& a) { B = sc_host::batch_blocks_layout(a, batch); }));
  SC_TRY(launch_subsystem_assembly(ctx, B, mem, batch, sc_host::sub_batch_max_pairs(mem, batch), d_coord, dim, d_pairs,
                                   d_gamma, d_row_start, d_group, d_pos, n_s, env_order, d_inv_sqrt_mass, d_hss, d_hes,
                                   d_hee));
  return sc_stage_end(ctx);
}

int sc_dev_vsa_batch_reduce_f64(sc_ctx* ctx, double* d_hss, double* d_hes, double* d_hee, int64_t ms, int64_t me,
                                int64_t batch, int64_t* d_info) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (ms <= 0 || me < 0 || ms > sc_host::kPotrfMaxOrder || me > sc_host::kPotrfMaxOrder)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem batch: the system's order must be positive, the slot's not negative");
  if (batch < 1 || batch > sc_host::kSubBatchMax)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem batch: the batch must hold 1 .. 65535 members, got %lld", (long long)batch);
  if (!d_hss || !d_info || (me > 0 && (!d_hes || !d_hee)))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "subsystem batch: a required pointer is NULL");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (me == 0) {   // every member is exactly the core: H_eff = H_ss
    SC_HIP(ctx, hipMemsetAsync(d_info, 0, sizeof(int64_t) * (size_t)batch, ctx->stream));
    return SC_OK;
  }
  const int outer = potrf_outer_block(me);
  sc_host::BatchReduceBufs B{};
  SC_TRY(carve_scratch(ctx, [&](sc_host::Arena& a) { B = sc_host::batch_reduce_layout(a, me, ms, batch, outer, potrf_desc_bytes()); }));
  SC_TRY(launch_subsystem_reduction(ctx, B, d_hss, d_hes, d_hee, ms, me, batch, outer, (long long*)d_info));
  return sc_stage_end(ctx);
}

}  // extern "C"
