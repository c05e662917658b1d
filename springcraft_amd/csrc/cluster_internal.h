// The launchers of cluster.hip, for api_cluster.hip.  d_dist: (n, n) float64 row-major; B: the carved workspace
// (cluster_policy.h); d_status: kClusterStatusInts int32.  Enqueue only.
#pragma once
#include "cluster_policy.h"
#include "common.h"

// validity, the bit matrix, the initial counts, labels <- -1, the status
int launch_cluster_gromos_init(sc_ctx* ctx, const double* d_dist, int64_t n, double cutoff, const sc_host::ClusterBufs& B,
                               int32_t* d_labels, int32_t* d_status);
// `rounds` rounds of pick + discount; a round after the last one, or after max_clusters clusters, does nothing
int launch_cluster_gromos_rounds(sc_ctx* ctx, int64_t n, int64_t rounds, int64_t max_clusters, const sc_host::ClusterBufs& B,
                                 int32_t* d_labels, int32_t* d_reps, int32_t* d_sizes, int32_t* d_status);
// BUILD: k passes over d_dist, then the grouping; d_td[0] <- the total deviation
int launch_cluster_kmedoids_init(sc_ctx* ctx, const double* d_dist, int64_t n, int64_t k, const sc_host::ClusterBufs& B,
                                 int32_t* d_labels, int32_t* d_reps, int32_t* d_sizes, double* d_td, int64_t td_cap,
                                 int32_t* d_status);
// `iterations` SWAP iterations in the given form of the evaluation; an iteration after convergence does nothing
int launch_cluster_kmedoids_swaps(sc_ctx* ctx, int form, const double* d_dist, int64_t n, int64_t k, int64_t iterations,
                                  const sc_host::ClusterBufs& B, int32_t* d_labels, int32_t* d_reps, int32_t* d_sizes,
                                  double* d_td, int64_t td_cap, int32_t* d_status);
