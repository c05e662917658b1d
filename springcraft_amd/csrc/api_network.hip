// C ABI (include/springcraft_hip.h), device-pointer entries of the correlation networks (corr_network.hip): edge weights of
// a coupling map, all-pairs shortest paths, path usage.  They replace Bio3D's cna and the shortest paths and betweenness of
// a graph library on host copies of the maps.  Argument checks, the scratch carve, the launcher call.
#include <cmath>

#include "api_internal.h"
#include "network_internal.h"

namespace {

int net_args_check(sc_ctx* ctx, const char* what, const int64_t* d_rec, int64_t count, int64_t n_max) {
  switch (sc_host::net_shape_error(count, n_max)) {
    case 0: break;
    case 1: return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: the number of members and the largest size must be positive", what);
    case 2: return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: at most %lld members, got %lld", what,
                                (long long)sc_host::kNetMaxMembers, (long long)count);
    default: return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: at most %lld nodes per member, got %lld", what,
                                 (long long)sc_host::kNetMaxN, (long long)n_max);
  }
  if (!d_rec) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "%s: the member records are required", what);
  return SC_OK;
}

}  // namespace

extern "C" {

int sc_dev_net_weights_f64(sc_ctx* ctx, const int64_t* d_rec, int64_t count, int64_t n_max, const double* d_corr,
                           const double* d_coord, double contact_cutoff_sq, double min_correlation, double* d_w,
                           int32_t* d_flags) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(net_args_check(ctx, "network weights", d_rec, count, n_max));
  if (!(min_correlation >= 0.0 && min_correlation <= 1.0))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "network weights: min_correlation %g outside [0, 1]", min_correlation);
  if (d_coord && !(contact_cutoff_sq > 0.0))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "network weights: the squared contact cutoff must be positive, got %g",
                        contact_cutoff_sq);
  if (!d_corr || !d_w || !d_flags)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "network weights: the map, the weights and the flags are required");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_net_weights(ctx, d_rec, count, n_max, d_corr, d_coord, contact_cutoff_sq, min_correlation, d_w, d_flags);
}

int sc_dev_net_paths_f64(sc_ctx* ctx, const int64_t* d_rec, int64_t count, int64_t n_max, const double* d_w, double* d_d,
                         int32_t* d_s, int32_t* d_flags) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(net_args_check(ctx, "network paths", d_rec, count, n_max));
  if (!d_w || !d_d || !d_s || !d_flags)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "network paths: the weights, the distances, the next hops and the flags are required");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_net_paths(ctx, d_rec, count, n_max, d_w, d_d, d_s, d_flags);
}

int64_t sc_dev_net_workspace(int64_t total_sq) {
  if (total_sq < 1 || total_sq > (int64_t)1 << 48) return -1;
  return (int64_t)sc_host::net_usage_scratch_bytes(total_sq);
}

int sc_dev_net_usage(sc_ctx* ctx, const int64_t* d_rec, int64_t count, int64_t n_max, int64_t total_sq, const int32_t* d_s,
                     int64_t* d_usage, int32_t* d_flags) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(net_args_check(ctx, "network usage", d_rec, count, n_max));
  if (n_max > sc_host::kNetUsageMaxN)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "network usage: the counters of a target are held in LDS for at most %lld nodes, got %lld",
                        (long long)sc_host::kNetUsageMaxN, (long long)n_max);
  if (sc_dev_net_workspace(total_sq) < 0 || total_sq > count * n_max * n_max)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "network usage: %lld packed pairs do not belong to %lld members of at most %lld nodes",
                        (long long)total_sq, (long long)count, (long long)n_max);
  if (!d_s || !d_usage || !d_flags)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "network usage: the next hops, the usage and the flags are required");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  sc_host::NetUsageBufs B{};
  SC_TRY(carve_scratch(ctx, [&](sc_host::Arena& a) { B = sc_host::net_usage_layout(a, total_sq); }));
  return launch_net_usage(ctx, d_rec, count, n_max, d_s, B.through, d_usage, d_flags);
}

}  // extern "C"
