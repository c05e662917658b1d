// C ABI (include/springcraft_hip.h), device-pointer entries of the clustering kernels (cluster.hip): neighbour-count
// clustering and k-medoids on a square dissimilarity matrix.  They replace a host copy of the matrix and gmx cluster /
// SciPy / a k-medoids package run on it.  Argument checks, the carve of the caller's workspace, the launcher call.
#include <cmath>

#include "api_internal.h"
#include "cluster_internal.h"

namespace {

// the caller's workspace carved by the layout that sized it; SC_ERR_INVALID_ARG when it is too small
int carve_workspace(sc_ctx* ctx, const char* what, int64_t n, int64_t k, void* d_ws, size_t ws_bytes, sc_host::ClusterBufs& B) {
  switch (sc_host::cluster_shape_error(n, k)) {
    case 0: break;
    case 1: return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: the matrix needs at least one item", what);
    case 2: return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: at most %lld items, got %lld", what,
                                (long long)sc_host::kClusterMaxN, (long long)n);
    default: return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: k must lie in 1..min(n, %lld), got %lld for %lld items", what,
                                 (long long)sc_host::kClusterMaxK, (long long)k, (long long)n);
  }
  if (!d_ws) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: the workspace is required", what);
  if (ws_bytes < sc_host::cluster_workspace_bytes(n, k))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: the workspace holds %zu bytes, sc_cluster_workspace asks for %zu", what,
                        ws_bytes, sc_host::cluster_workspace_bytes(n, k));
  sc_host::Arena a(d_ws, ws_bytes);
  B = sc_host::cluster_layout(a, n, k);
  if (a.overrun()) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: the workspace layout overran its buffer", what);
  return SC_OK;
}

}  // namespace

extern "C" {

int64_t sc_cluster_workspace(int64_t n, int64_t k) {
  if (sc_host::cluster_shape_error(n, k)) return -1;
  return (int64_t)sc_host::cluster_workspace_bytes(n, k);
}

int sc_cluster_form(int64_t n, int64_t k) { return sc_host::cluster_form(sc_host::read_cluster_env(), n, k); }

int sc_dev_cluster_gromos_init_f64(sc_ctx* ctx, const double* d_dist, int64_t n, double cutoff, void* d_ws, size_t ws_bytes,
                                   int32_t* d_labels, int32_t* d_status) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  sc_host::ClusterBufs B{};
  SC_TRY(carve_workspace(ctx, "neighbour-count clustering", n, 0, d_ws, ws_bytes, B));
  if (!(cutoff >= 0.0) || std::isinf(cutoff))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "neighbour-count clustering: the cutoff must be finite and not negative, got %g",
                        cutoff);
  if (!d_dist || !d_labels || !d_status)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "neighbour-count clustering: the matrix, the labels and the status are required");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_cluster_gromos_init(ctx, d_dist, n, cutoff, B, d_labels, d_status);
}

int sc_dev_cluster_gromos_rounds(sc_ctx* ctx, int64_t n, int64_t rounds, int64_t max_clusters, void* d_ws, size_t ws_bytes,
                                 int32_t* d_labels, int32_t* d_reps, int32_t* d_sizes, int32_t* d_status) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  sc_host::ClusterBufs B{};
  SC_TRY(carve_workspace(ctx, "neighbour-count rounds", n, 0, d_ws, ws_bytes, B));
  if (rounds < 1 || rounds > n)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "neighbour-count rounds: 1..%lld rounds at a time, got %lld", (long long)n,
                        (long long)rounds);
  if (max_clusters < 1 || max_clusters > n)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "neighbour-count rounds: max_clusters must lie in 1..%lld, got %lld",
                        (long long)n, (long long)max_clusters);
  if (!d_labels || !d_reps || !d_sizes || !d_status)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG,
                        "neighbour-count rounds: the labels, the centres, the sizes and the status are required");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_cluster_gromos_rounds(ctx, n, rounds, max_clusters, B, d_labels, d_reps, d_sizes, d_status);
}

int sc_dev_cluster_kmedoids_init_f64(sc_ctx* ctx, const double* d_dist, int64_t n, int64_t k, void* d_ws, size_t ws_bytes,
                                     int32_t* d_labels, int32_t* d_reps, int32_t* d_sizes, double* d_td, int64_t td_cap,
                                     int32_t* d_status) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (k < 1) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "k-medoids: k must be at least 1, got %lld", (long long)k);
  sc_host::ClusterBufs B{};
  SC_TRY(carve_workspace(ctx, "k-medoids", n, k, d_ws, ws_bytes, B));
  if (td_cap < 1) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "k-medoids: the deviation history needs one entry at least");
  if (!d_dist || !d_labels || !d_reps || !d_sizes || !d_td || !d_status)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG,
                        "k-medoids: the matrix, the labels, the medoids, the sizes, the deviations and the status are required");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_cluster_kmedoids_init(ctx, d_dist, n, k, B, d_labels, d_reps, d_sizes, d_td, td_cap, d_status);
}

int sc_dev_cluster_kmedoids_swaps_f64(sc_ctx* ctx, const double* d_dist, int64_t n, int64_t k, int64_t iterations, void* d_ws,
                                      size_t ws_bytes, int32_t* d_labels, int32_t* d_reps, int32_t* d_sizes, double* d_td,
                                      int64_t td_cap, int32_t* d_status) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (k < 1) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "k-medoids swaps: k must be at least 1, got %lld", (long long)k);
  sc_host::ClusterBufs B{};
  SC_TRY(carve_workspace(ctx, "k-medoids swaps", n, k, d_ws, ws_bytes, B));
  if (iterations < 1 || iterations > 65536)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "k-medoids swaps: 1..65536 iterations at a time, got %lld", (long long)iterations);
  if (td_cap < 1) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "k-medoids swaps: the deviation history needs one entry at least");
  if (!d_dist || !d_labels || !d_reps || !d_sizes || !d_td || !d_status)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG,
                        "k-medoids swaps: the matrix, the labels, the medoids, the sizes, the deviations and the status are required");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_cluster_kmedoids_swaps(ctx, sc_cluster_form(n, k), d_dist, n, k, iterations, B, d_labels, d_reps, d_sizes, d_td,
                                       td_cap, d_status);
}

}  // extern "C"
