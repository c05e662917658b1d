// C ABI (include/springcraft_hip.h), device-pointer entries of the rotation-translation blocks (rtb.hip) and of the network
// as an operator on the pair list (pair_operator.hip, pair_panel.hip, pair_cg.hip): argument checks and the launcher call.
#include "api_internal.h"

namespace {

int pairs_network_check(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs, int64_t k,
                        const double* d_gamma, const double* d_x, int64_t q) {
  if (dim != 1 && dim != 3) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: dim must be 1 or 3, got %d", dim);
  if (n_atoms <= 0 || k < 0 || q < 0)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: n_atoms must be positive, k and q not negative");
  if (n_atoms > ((int64_t)1 << 32))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: at most 2^32 atoms");
  if (dim == 3 && !d_coord) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: dim 3 needs the coordinates");
  if (k > 0 && (!d_pairs || !d_gamma))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: pairs and gamma are required with k > 0");
  if (q > 0 && !d_x) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the rows are required with q > 0");
  return SC_OK;
}

int pairs_cg_panel_check(sc_ctx* ctx, int64_t n_atoms, int64_t ld, int64_t q, const void* const* panels, int count,
                         const void* d_state, const void* d_work, size_t work_bytes) {
  if (ld < q) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the leading dimension %lld is below the %lld columns",
                                  (long long)ld, (long long)q);
  if (q > 65535 * (int64_t)64) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: at most 4194240 columns per panel");
  if (q == 0) return SC_OK;
  for (int a = 0; a < count; ++a) {
    if (!panels[a]) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the X, R, P and Q panels are required with q > 0");
    for (int b = 0; b < a; ++b)
      if (panels[a] == panels[b]) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the X, R, P and Q panels must be distinct");
  }
  if (!d_state || !d_work) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the state and the workspace are required");
  if (work_bytes < pairs_cg_workspace_bytes(n_atoms, q))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the workspace holds %zu bytes, %zu are needed", work_bytes,
                        pairs_cg_workspace_bytes(n_atoms, q));
  return SC_OK;
}

}  // namespace

extern "C" {

// ---- rotation-translation blocks (rtb.hip) --------------------------------------------------------------------------
int sc_dev_rtb_hessian_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, const int64_t* d_pairs, int64_t k,
                           const double* d_gamma, const double* d_inv_sqrt_mass, const double* d_P,
                           const int32_t* d_block_of_atom, const int64_t* d_offset, int64_t n_blocks, int64_t nr,
                           const int64_t* d_order, const int64_t* d_seg_start, int64_t n_seg,
                           const int64_t* d_block_start, double* d_hb) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (n_atoms <= 0 || n_blocks <= 0 || nr <= 0 || k < 0 || n_seg < 0)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "rtb: sizes must be positive (k, n_seg: not negative)");
  if (n_blocks > n_atoms || nr > 6 * n_blocks || n_seg > k)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "rtb: %lld blocks / %lld rows / %lld segments do not fit %lld atoms, %lld pairs",
                        (long long)n_blocks, (long long)nr, (long long)n_seg, (long long)n_atoms, (long long)k);
  if (!d_coord || !d_P || !d_block_of_atom || !d_offset || !d_hb)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "rtb: a required pointer is NULL");
  if (k > 0 && (!d_pairs || !d_gamma || !d_order || !d_seg_start || !d_block_start || n_seg == 0))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "rtb: pairs / gamma / order / segment starts are required with k > 0");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_rtb_hessian(ctx, d_coord, n_atoms, d_pairs, k, d_gamma, d_inv_sqrt_mass, d_P, d_block_of_atom, d_offset,
                            n_blocks, nr, d_order, d_seg_start, n_seg, d_block_start, d_hb);
}

int sc_dev_rtb_expand_f64(sc_ctx* ctx, const double* d_u, int64_t nvec, int64_t nr, const double* d_P,
                          const int32_t* d_block_of_atom, const int64_t* d_offset, int64_t n_atoms, double* d_v) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (nvec <= 0 || nr <= 0 || n_atoms <= 0 || nvec > 8 * (int64_t)65535)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "rtb: sizes must be positive (nvec at most 524280)");
  if (!d_u || !d_P || !d_block_of_atom || !d_offset || !d_v)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "rtb: a required pointer is NULL");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_rtb_expand(ctx, d_u, nvec, nr, d_P, d_block_of_atom, d_offset, n_atoms, d_v);
}

// ---- the network as an operator on the pair list (pair_operator.hip) -------------------------------------------------
int sc_dev_pairs_apply_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs,
                           int64_t k, const double* d_gamma, const int64_t* d_row_start, const double* d_atom_scale,
                           const double* d_x, int64_t q, double* d_y, double* d_energy) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (!d_y && !d_energy) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: neither a product nor energies asked for");
  SC_TRY(pairs_network_check(ctx, d_coord, n_atoms, dim, d_pairs, k, d_gamma, d_x, q));
  if (k > 0 && !d_row_start) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: row starts are required with k > 0");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_pairs_apply(ctx, d_coord, n_atoms, dim, d_pairs, k, d_gamma, d_row_start, d_atom_scale, d_x, q, d_y,
                            d_energy);
}

int sc_dev_pairs_strain_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs,
                            int64_t k, const double* d_gamma, const double* d_atom_scale, const int64_t* d_pair_idx,
                            int64_t ks, const double* d_x, int64_t q, double* d_out) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(pairs_network_check(ctx, d_coord, n_atoms, dim, d_pairs, k, d_gamma, d_x, q));
  if (ks < 0 || ks > ((int64_t)1 << 38))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the number of listed pairs must lie in 0 .. 2^38");
  if (ks > 0 && q > 0 && (!d_pair_idx || !d_out))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the pair indices and the result are required");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_pairs_strain(ctx, d_coord, n_atoms, dim, d_pairs, k, d_gamma, d_atom_scale, d_pair_idx, ks, d_x, q,
                             d_out);
}

int sc_dev_pairs_panel_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs,
                           int64_t k, const double* d_gamma, const int64_t* d_row_start, const double* d_atom_scale,
                           const double* d_x, double* d_z, int64_t ld, int64_t q, double alpha, double beta,
                           double gamma_c) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(pairs_network_check(ctx, d_coord, n_atoms, dim, d_pairs, k, d_gamma, d_x, q));
  if (k > 0 && !d_row_start) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: row starts are required with k > 0");
  if (ld < q) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the leading dimension %lld is below the %lld columns",
                                  (long long)ld, (long long)q);
  if (q > 65535 * (int64_t)64) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: at most 4194240 columns per panel");
  if (q > 0 && !d_z) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the result panel is required with q > 0");
  if (d_z && d_z == d_x) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the result panel must not be the input panel");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_pairs_panel(ctx, d_coord, n_atoms, dim, d_pairs, k, d_gamma, d_row_start, d_atom_scale, d_x, d_z, ld, q,
                            alpha, beta, gamma_c);
}

// ---- conjugate gradients on the pair list (pair_cg.hip) ---------------------------------------------------------------
int sc_dev_pairs_cg_workspace(int64_t n_atoms, int64_t q, size_t* bytes) {
  if (!bytes || n_atoms <= 0 || q < 0 || n_atoms > ((int64_t)1 << 32) || q > 65535 * (int64_t)64) return SC_ERR_INVALID_ARG;
  *bytes = pairs_cg_workspace_bytes(n_atoms, q);
  return SC_OK;
}

int sc_dev_pairs_cg_init_f64(sc_ctx* ctx, int64_t n_atoms, int dim, double* d_x, const double* d_r, double* d_p, int64_t ld,
                             int64_t q, double tol, double* d_state, void* d_work, size_t work_bytes) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (dim != 1 && dim != 3) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: dim must be 1 or 3, got %d", dim);
  if (n_atoms <= 0 || q < 0 || n_atoms > ((int64_t)1 << 32))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: n_atoms must lie in 1 .. 2^32, q must not be negative");
  if (!(tol > 0.0)) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: tol must be positive");
  const void* panels[3] = {d_x, d_r, d_p};
  SC_TRY(pairs_cg_panel_check(ctx, n_atoms, ld, q, panels, 3, d_state, d_work, work_bytes));
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_pairs_cg_init(ctx, n_atoms, dim, d_x, d_r, d_p, ld, q, tol, d_state, (double*)d_work);
}

int sc_dev_pairs_cg_step_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs,
                             int64_t k, const double* d_gamma, const int64_t* d_row_start, const double* d_atom_scale,
                             double* d_x, double* d_r, double* d_p, double* d_q, int64_t ld, int64_t q, double* d_state,
                             void* d_work, size_t work_bytes, int64_t iterations) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(pairs_network_check(ctx, d_coord, n_atoms, dim, d_pairs, k, d_gamma, d_p, q));
  if (k > 0 && !d_row_start) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: row starts are required with k > 0");
  if (iterations < 0) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the number of iterations must not be negative");
  const void* panels[4] = {d_x, d_r, d_p, d_q};
  SC_TRY(pairs_cg_panel_check(ctx, n_atoms, ld, q, panels, 4, d_state, d_work, work_bytes));
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_pairs_cg_step(ctx, d_coord, n_atoms, dim, d_pairs, k, d_gamma, d_row_start, d_atom_scale, d_x, d_r, d_p,
                              d_q, ld, q, d_state, (double*)d_work, iterations);
}

}  // extern "C"
