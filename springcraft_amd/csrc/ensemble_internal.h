// The launchers of ensemble_pca.hip and rmsd_matrix.hip, for api_ensemble.hip (the superposition and mean launchers are in
// common.h).
#pragma once
#include "common.h"
#include "ensemble_policy.h"

// bytes of one GEMM record (pca_layout takes two)
size_t ensemble_pca_desc_bytes();
// The n_modes largest principal components of the fitted frames d_frames (M, N, 3) about d_mean (N, 3), d_sqrt_mass (N) or
// null: d_w (n_modes) = 1 / variance ascending, d_var (n_modes) descending, d_v (n_modes, 3 N) unit rows, d_total (1) the
// trace of the covariance.  P / B: pca_plan and its layout carved from ctx->scratch (the eigensolver works in ctx->ws).
// Enqueue only; with ctx->profiling the phases "pca_product", "pca_eigh" and "pca_expand" are timed.
int launch_ensemble_pca(sc_ctx* ctx, const sc_host::PcaPlan& P, const sc_host::PcaBufs& B, const double* d_frames,
                        int64_t n_frames, int64_t n_atoms, const double* d_mean, const double* d_sqrt_mass, int64_t n_modes,
                        double* d_w, double* d_var, double* d_v, double* d_total);

// rmsd_matrix.hip: d_out (n_a, n_b) = the RMSD (squared: the mean-square deviation) of every frame of d_a (n_a, N, 3) with
// every frame of d_b (n_b, N, 3); d_b null: d_a with itself, n_b = n_a, symmetric bit for bit with a zero diagonal.  fit:
// the least-squares rotation's, else of the frames as they are.  B: rmsd_layout of (n_a, d_b ? n_b : 0, N) carved from
// ctx->scratch.  Enqueue only.
int launch_rmsd_matrix(sc_ctx* ctx, const sc_host::RmsdBufs& B, const double* d_a, int64_t n_a, const double* d_b,
                       int64_t n_b, int64_t n_atoms, const double* d_weights, bool fit, bool squared, double* d_out);

// rmsd_matrix.hip: the neighbour bits of the n frames d_frames (n, N, 3) without the matrix.  d_adj (n, cluster_words(n)):
// bit g of row f is set when the value launch_rmsd_matrix would write for (f, g) is <= cutoff or f = g, both frames finite;
// d_count (n): the rows' popcounts; d_valid (words): the finite frames.  Optional (null: not written): d_alive (words) <-
// d_valid, d_labels (n) <- -1, and together d_ctl (kClusterCtlInts) <- 0, d_status (kClusterStatusInts) <- (finite frames,
// 0, 0, 0): with all of them a neighbour-count run's workspace as launch_cluster_gromos_init leaves it.  B: rmsd_layout of
// (n, 0, N) carved from ctx->scratch.  Enqueue only.
int launch_frame_neighbours(sc_ctx* ctx, const sc_host::RmsdBufs& B, const double* d_frames, int64_t n, int64_t n_atoms,
                            const double* d_weights, bool fit, bool squared, double cutoff, uint64_t* d_adj,
                            int32_t* d_count, uint64_t* d_valid, uint64_t* d_alive, int32_t* d_labels, int32_t* d_ctl,
                            int32_t* d_status);
