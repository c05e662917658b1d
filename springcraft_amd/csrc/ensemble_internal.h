// The PCA launcher of ensemble_pca.hip, for api_ensemble.hip (the superposition and mean launchers are in common.h).
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
