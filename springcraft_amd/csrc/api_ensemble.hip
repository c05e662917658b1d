// C ABI (include/springcraft_hip.h), device-pointer entries of the conformational ensembles: superposition and the mean frame
// (superpose.hip), ensemble PCA (ensemble_pca.hip), the pairwise RMSD matrix and the frames' neighbour bits
// (rmsd_matrix.hip).  Argument checks, the scratch carve, the launcher call.
#include <cmath>

#include "api_internal.h"
#include "cluster_policy.h"
#include "ensemble_internal.h"

namespace {

int ensemble_sizes_check(sc_ctx* ctx, const char* what, int64_t n_frames, int64_t n_atoms) {
  if (n_frames <= 0 || n_atoms <= 0)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: the numbers of frames and atoms must be positive", what);
  if (n_frames > 0x7fffffffLL || n_atoms > 0x7fffffffLL / 3)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: at most 2^31 - 1 frames and coordinates per frame", what);
  return SC_OK;
}

// the checks the two neighbour-bit entries share: what the product kernel and the clustering kernels can index, the flags
// of the RMSD matrix, a cutoff a comparison can be made with
int frame_neighbours_check(sc_ctx* ctx, const char* what, int64_t n_frames, int64_t n_atoms, int flags, double cutoff) {
  if (n_frames <= 0 || n_atoms <= 0)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: the numbers of frames and atoms must be positive", what);
  if (flags & ~3) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: flags has bits 0 (fit) and 1 (squared) only", what);
  if (sc_host::cluster_shape_error(n_frames, 0))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: at most %lld frames, got %lld", what, (long long)sc_host::kClusterMaxN,
                        (long long)n_frames);
  if (sc_host::rmsd_shape_error(n_frames, 0, n_atoms))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: %lld frames of %lld atoms are beyond the kernels' index range", what,
                        (long long)n_frames, (long long)n_atoms);
  if (!(cutoff >= 0.0) || std::isinf(cutoff))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: the cutoff must be finite and not negative, got %g", what, cutoff);
  return SC_OK;
}

}  // namespace

extern "C" {

int sc_superpose_form(int64_t n_atoms) {
  return sc_host::superpose_form(sc_host::read_superpose_env(), n_atoms);
}

int sc_dev_superpose_f64(sc_ctx* ctx, const double* d_frames, int64_t n_frames, int64_t n_atoms, const double* d_target,
                         const double* d_weights, double* d_out, double* d_rot, double* d_trans, double* d_rmsd) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(ensemble_sizes_check(ctx, "superpose", n_frames, n_atoms));
  if (!d_frames || !d_target || !d_out)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "superpose: the frames, the target and the output are required");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  sc_host::SuperposeBufs B{};
  SC_TRY(carve_scratch(ctx, [&](sc_host::Arena& a) { B = sc_host::superpose_layout(a); }));
  return launch_superpose(ctx, sc_superpose_form(n_atoms), d_frames, n_frames, n_atoms, d_target, d_weights,
                          B.target_centre, d_out, d_rot, d_trans, d_rmsd);
}

int sc_dev_ensemble_mean_f64(sc_ctx* ctx, const double* d_frames, int64_t n_frames, int64_t n_atoms,
                             const double* d_frame_weights, double* d_mean, double* d_msd) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(ensemble_sizes_check(ctx, "ensemble mean", n_frames, n_atoms));
  if (sc_host::mean_chunks(n_frames) > 65535)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "ensemble mean: at most %d frames", 65535 * sc_host::kMeanChunk);
  if (!d_frames || !d_mean)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "ensemble mean: the frames and the mean are required");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  sc_host::MeanBufs B{};
  SC_TRY(carve_scratch(ctx, [&](sc_host::Arena& a) { B = sc_host::mean_layout(a, n_frames, n_atoms); }));
  return launch_ensemble_mean(ctx, d_frames, n_frames, n_atoms, d_frame_weights, B.partial, d_mean, d_msd);
}

int sc_dev_ensemble_pca_f64(sc_ctx* ctx, const double* d_frames, int64_t n_frames, int64_t n_atoms, const double* d_mean,
                            const double* d_sqrt_mass, int64_t n_modes, double* d_w, double* d_var, double* d_v,
                            double* d_total) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(ensemble_sizes_check(ctx, "ensemble pca", n_frames, n_atoms));
  const int64_t most = std::min<int64_t>(n_frames - 1, 3 * n_atoms);
  if (n_modes < 1 || n_modes > most)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "ensemble pca: %lld components asked for, %lld frames of %lld atoms have at most %lld",
                        (long long)n_modes, (long long)n_frames, (long long)n_atoms, (long long)most);
  if (n_modes > 65535) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "ensemble pca: at most 65535 components");
  if (!d_frames || !d_mean || !d_w || !d_var || !d_v || !d_total)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "ensemble pca: a required pointer is NULL");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const sc_host::PcaPlan P = sc_host::pca_plan(n_frames, n_atoms, n_modes, ctx->num_cus);
  sc_host::PcaBufs B{};
  SC_TRY(carve_scratch(ctx, [&](sc_host::Arena& a) {
    B = sc_host::pca_layout(a, P, n_frames, n_atoms, n_modes, ensemble_pca_desc_bytes());
  }));
  return launch_ensemble_pca(ctx, P, B, d_frames, n_frames, n_atoms, d_mean, d_sqrt_mass, n_modes, d_w, d_var, d_v, d_total);
}

int64_t sc_rmsd_matrix_workspace(int64_t n_a, int64_t n_b, int64_t n_atoms) {
  if (sc_host::rmsd_shape_error(n_a, n_b, n_atoms)) return -1;
  return (int64_t)sc_host::rmsd_scratch_bytes(n_a, n_b, n_atoms);
}

int sc_dev_rmsd_matrix_f64(sc_ctx* ctx, const double* d_a, int64_t n_a, const double* d_b, int64_t n_b, int64_t n_atoms,
                           const double* d_weights, int flags, double* d_out) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (n_a <= 0 || n_b <= 0 || n_atoms <= 0)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "rmsd matrix: the numbers of frames and atoms must be positive");
  if (!d_b && n_b != n_a)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "rmsd matrix: a self-comparison (d_b NULL) has n_b = n_a, got %lld and %lld",
                        (long long)n_b, (long long)n_a);
  if (flags & ~3) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "rmsd matrix: flags has bits 0 (fit) and 1 (squared) only");
  if (sc_host::rmsd_shape_error(n_a, d_b ? n_b : 0, n_atoms))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "rmsd matrix: %lld x %lld frames of %lld atoms are beyond the kernels' index range",
                        (long long)n_a, (long long)n_b, (long long)n_atoms);
  if (!d_a || !d_out) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "rmsd matrix: the frames and the output are required");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  sc_host::RmsdBufs B{};
  SC_TRY(carve_scratch(ctx, [&](sc_host::Arena& a) { B = sc_host::rmsd_layout(a, n_a, d_b ? n_b : 0, n_atoms); }));
  return launch_rmsd_matrix(ctx, B, d_a, n_a, d_b, n_b, n_atoms, d_weights, (flags & 1) != 0, (flags & 2) != 0, d_out);
}

int sc_dev_frame_neighbours_f64(sc_ctx* ctx, const double* d_frames, int64_t n_frames, int64_t n_atoms,
                                const double* d_weights, int flags, double cutoff, uint64_t* d_adj, int32_t* d_count,
                                uint64_t* d_valid) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(frame_neighbours_check(ctx, "frame neighbours", n_frames, n_atoms, flags, cutoff));
  if (!d_frames || !d_adj || !d_count || !d_valid)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "frame neighbours: the frames, the bits, the counts and the validity words are required");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  sc_host::RmsdBufs B{};
  SC_TRY(carve_scratch(ctx, [&](sc_host::Arena& a) { B = sc_host::rmsd_layout(a, n_frames, 0, n_atoms); }));
  return launch_frame_neighbours(ctx, B, d_frames, n_frames, n_atoms, d_weights, (flags & 1) != 0, (flags & 2) != 0, cutoff,
                                 d_adj, d_count, d_valid, nullptr, nullptr, nullptr, nullptr);
}

int sc_dev_frame_neighbours_init_f64(sc_ctx* ctx, const double* d_frames, int64_t n_frames, int64_t n_atoms,
                                     const double* d_weights, int flags, double cutoff, void* d_ws, size_t ws_bytes,
                                     int32_t* d_labels, int32_t* d_status) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  const char* what = "frame neighbours init";
  SC_TRY(frame_neighbours_check(ctx, what, n_frames, n_atoms, flags, cutoff));
  if (!d_ws) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: the workspace is required", what);
  if (ws_bytes < sc_host::cluster_workspace_bytes(n_frames, 0))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: the workspace holds %zu bytes, sc_cluster_workspace asks for %zu", what,
                        ws_bytes, sc_host::cluster_workspace_bytes(n_frames, 0));
  sc_host::Arena ws(d_ws, ws_bytes);
  const sc_host::ClusterBufs K = sc_host::cluster_layout(ws, n_frames, 0);
  if (ws.overrun()) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: the workspace layout overran its buffer", what);
  if (!d_frames || !d_labels || !d_status)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: the frames, the labels and the status are required", what);
  SC_HIP(ctx, hipSetDevice(ctx->device));
  sc_host::RmsdBufs B{};
  SC_TRY(carve_scratch(ctx, [&](sc_host::Arena& a) { B = sc_host::rmsd_layout(a, n_frames, 0, n_atoms); }));
  return launch_frame_neighbours(ctx, B, d_frames, n_frames, n_atoms, d_weights, (flags & 1) != 0, (flags & 2) != 0, cutoff,
                                 K.adj, K.count, K.valid, K.alive, d_labels, K.ctl, d_status);
}

}  // extern "C"
