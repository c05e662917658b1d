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
