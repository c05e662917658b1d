// The launchers of corr_network.hip, for api_network.hip.  d_rec: (count, 3) int64 member records (network_policy.h); the
// pair buffers are packed by the records' offsets, d_flags is (count) int32.  Enqueue only.
#pragma once
#include "common.h"
#include "network_policy.h"

// d_w <- edge weights of the correlation maps d_corr; d_coord (sum n, 3) or null; d_flags <- 1 for a member with a NaN input, else 0
int launch_net_weights(sc_ctx* ctx, const int64_t* d_rec, int64_t count, int64_t n_max, const double* d_corr,
                       const double* d_coord, double cutoff_sq, double min_correlation, double* d_w, int32_t* d_flags);
// d_d, d_s <- all-pairs shortest distances and next hops of the weights d_w; d_flags in / out: a set flag stays, a member with
// a NaN or negative weight gets one; a flagged member ends as NaN / -1
int launch_net_paths(sc_ctx* ctx, const int64_t* d_rec, int64_t count, int64_t n_max, const double* d_w, double* d_d,
                     int32_t* d_s, int32_t* d_flags);
// d_usage (sum n) int64 <- how many stored paths pass through every node; d_through: net_usage_layout's workspace
int launch_net_usage(sc_ctx* ctx, const int64_t* d_rec, int64_t count, int64_t n_max, const int32_t* d_s, int32_t* d_through,
                     int64_t* d_usage, int32_t* d_flags);
