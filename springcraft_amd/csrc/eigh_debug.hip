// Debugging entry points of the eigensolver (include/springcraft_hip_debug.h): the stages of a solve on host data, on the
// plan and the reduction step of the drivers (eigh_plan.h).  tests/test_stage_ratios_gpu.py, tests/test_partial_ratios_gpu.py,
// tools/check_two_stage.py
#include <vector>

#include "api_internal.h"
#include "eigh_plan.h"
#include "springcraft_hip_debug.h"

extern "C" int sc_dbg_reduce_host(sc_ctx* ctx, const double* a, int n, int batch, int which, double* d_out, double* e_out,
                                  double* scale_out, double* band_out, double* q_out, int* two_stage_out) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (!a || !d_out || !e_out || n < 1 || n > 46000 || batch < 1 || which < 0 || which > 2)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  if (ctx->two_stage == 1 && n < 4 * sb_band_width())
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "order %d is below the two-stage minimum %d", n, 4 * sb_band_width());
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const bool vectors = q_out != nullptr;
  const SolvePlan P = make_solve_plan(ctx, n, batch, vectors);
  if (!P.two && vectors && which != 0)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "the one-stage path has one orthogonal factor (which = 0)");
  if (two_stage_out) *two_stage_out = P.two ? 1 : 0;
  hipStream_t st = ctx->stream;
  const size_t elems = (size_t)n * n, band_elems = (size_t)2 * sb_band_width() * n;
  const size_t a_bytes = align_up(elems * 8 * batch, 256), band_bytes = P.two ? align_up(band_elems * 8 * batch, 256) : 0;
  SC_TRY(sc_reserve_ws(ctx, P.total));
  SC_TRY(sc_reserve_scratch(ctx, a_bytes * (vectors ? 2 : 1) + band_bytes));
  char* base = (char*)ctx->ws;
  double* d_a = (double*)ctx->scratch;
  double* d_band = P.two ? (double*)((char*)ctx->scratch + a_bytes) : nullptr;
  double* d_z = vectors ? (double*)((char*)ctx->scratch + a_bytes + band_bytes) : nullptr;
  double* tri_ws = (double*)(base + P.off_tri);
  const long long stride_a = (long long)elems;

  SC_HIP(ctx, hipMemcpyAsync(d_a, a, elems * 8 * batch, hipMemcpyHostToDevice, st));
  SolveProfile prof(ctx);   // (neither marked nor finished: the context's timings stay those of the last solve)
  SC_TRY(tridiagonalise(ctx, d_a, n, batch, P, base, prof, d_band));
  if (vectors) {
    {   // Z = I for every matrix (the host copy must outlive its transfer)
      std::vector<double> eye(elems, 0.0);
      for (int i = 0; i < n; ++i) eye[(size_t)i * n + i] = 1.0;
      SC_HIP(ctx, hipMemcpyAsync(d_z, eye.data(), elems * 8, hipMemcpyHostToDevice, st));
      SC_HIP(ctx, hipStreamSynchronize(st));
    }
    for (int b = 1; b < batch; ++b)
      SC_HIP(ctx, hipMemcpyAsync(d_z + (size_t)b * elems, d_z, elems * 8, hipMemcpyDeviceToDevice, st));
    if (P.two && which != 1) {   // Z <- Q2 Z
      double* sb_ws = (double*)(base + P.off_sb);
      SC_TRY(bt2_prepare(ctx, n, batch, sb_ws, P.SL, st));
      SC_TRY(bt2_batched(ctx, n, batch, sb_ws, P.SL, (const int*)(base + P.off_dia), d_z, stride_a, n));
    }
    if (which != 2)              // Z <- Q1 Z (one-stage: the only factor)
      SC_TRY(backtransform_batched(ctx, d_a, stride_a, n, batch, tri_ws, P.TL, (double*)(base + P.off_bt), P.BL, d_z,
                                   stride_a, n, (double*)(base + P.off_qtmp), P.bt_descs(base),
                                   P.two ? sb_band_width() : 1));
  }
  SC_TRY(sc_stage_end(ctx));
  SC_HIP(ctx, hipStreamSynchronize(st));
  SC_TRY(sc_deferred_status(ctx));
  for (int b = 0; b < batch; ++b) {
    const double* tri = tri_ws + (size_t)b * P.TL.slab;
    SC_HIP(ctx, hipMemcpy(d_out + (size_t)b * n, tri + P.TL.d, sizeof(double) * n, hipMemcpyDeviceToHost));
    SC_HIP(ctx, hipMemcpy(e_out + (size_t)b * n, tri + P.TL.e, sizeof(double) * n, hipMemcpyDeviceToHost));
    e_out[(size_t)b * n + n - 1] = 0.0;
    if (scale_out) SC_HIP(ctx, hipMemcpy(scale_out + b, tri + P.TL.hscale + 2, sizeof(double), hipMemcpyDeviceToHost));
  }
  if (P.two && band_out) SC_HIP(ctx, hipMemcpy(band_out, d_band, band_elems * 8 * batch, hipMemcpyDeviceToHost));
  if (vectors) SC_HIP(ctx, hipMemcpy(q_out, d_z, elems * 8 * batch, hipMemcpyDeviceToHost));
  return SC_OK;
}

extern "C" int sc_dbg_stedc_host(sc_ctx* ctx, const double* d, const double* e, int n, int batch, double* w_out,
                                 double* z_out) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (!d || !e || !w_out || !z_out || n < 1 || n > 46000 || batch < 1)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const SolvePlan P = make_solve_plan(ctx, n, batch, true);
  hipStream_t st = ctx->stream;
  const size_t elems = (size_t)n * n;
  const size_t z_bytes = align_up(elems * 8 * batch, 256);
  SC_TRY(sc_reserve_ws(ctx, P.total));
  SC_TRY(sc_reserve_scratch(ctx, z_bytes + (size_t)n * 8 * batch));
  char* base = (char*)ctx->ws;
  double* d_z = (double*)ctx->scratch;
  double* d_w = (double*)((char*)ctx->scratch + z_bytes);
  double* tri_ws = (double*)(base + P.off_tri);
  for (int b = 0; b < batch; ++b) {
    double* tri = tri_ws + (size_t)b * P.TL.slab;
    SC_TRY(sc_stage_upload(ctx, tri + P.TL.d, d + (size_t)b * n, sizeof(double) * n));
    SC_TRY(sc_stage_upload(ctx, tri + P.TL.e, e + (size_t)b * n, sizeof(double) * n));
  }
  SC_TRY(stedc_batched(ctx, n, batch, tri_ws, P.TL, (double*)(base + P.off_dc), P.DL, d_w, n, d_z,
                       (double*)(base + P.off_qtmp), (double*)(base + P.off_u), (long long)elems, P.mid_descs(base)));
  SC_TRY(sc_stage_end(ctx));
  SC_HIP(ctx, hipStreamSynchronize(st));
  SC_TRY(sc_deferred_status(ctx));
  SC_HIP(ctx, hipMemcpy(w_out, d_w, sizeof(double) * n * batch, hipMemcpyDeviceToHost));
  SC_HIP(ctx, hipMemcpy(z_out, d_z, elems * 8 * batch, hipMemcpyDeviceToHost));
  return SC_OK;
}

extern "C" int sc_dbg_partial_tridiag_host(sc_ctx* ctx, const double* d, const double* e, const double* f, const int* own,
                                           int n, int batch, int window, int il, int m, double vl, double vu,
                                           int vectors, double* w_out, double* z_out, int* win_out,
                                           long long* count_out) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (!d || !e || !w_out || (vectors && !z_out) || n < 1 || n > 46000 || batch < 1)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  if (window) {   // m is the capacity K of every slot
    SC_TRY(check_window(ctx, vl, vu));
    if (m < 1 || m > n) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "window capacity %d outside 1..%d", m, n);
    for (int b = 0; own && b < batch; ++b)
      if (own[b] < m || own[b] > n)
        return sc_set_error(ctx, SC_ERR_INVALID_ARG, "own order %d of matrix %d outside %d..%d", own[b], b, m, n);
    il = 0;
  } else if (il < 0 || m < 1 || m > n || il > n - m) {
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad eigenvalue index range [%d, %d) for order %d", il, il + m, n);
  }
  SC_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  TriLayout TL;
  const size_t slab = tri_slab_doubles(n, sc_host::eigh_env().nb, &TL);
  const size_t rows = (size_t)batch * m;
  double *tri_ws = nullptr, *d_stein = nullptr, *d_w = nullptr, *d_x = nullptr, *d_wcopy = nullptr, *d_xcopy = nullptr;
  GemmDesc* descs = nullptr;
  WinCount* d_win = nullptr;
  long long* d_count = nullptr;
  RaggedRec* d_own = nullptr;
  SC_TRY(carve_scratch(ctx, [&](sc_host::Arena& a) {
    tri_ws = a.take<double>(slab * batch);
    descs = a.take<GemmDesc>(2 * (size_t)batch);
    d_w = a.take<double>(rows);
    if (vectors) {
      d_stein = a.take<double>(stein_workspace_doubles(n, m) * batch);
      d_x = a.take<double>(rows * n);
    }
    if (window) {
      d_win = a.take<WinCount>((size_t)batch);
      d_count = a.take<long long>((size_t)batch);
      d_wcopy = a.take<double>(rows);
      if (vectors) d_xcopy = a.take<double>(rows * n);
      if (own) d_own = a.take<RaggedRec>((size_t)batch);
    }
  }));
  for (int b = 0; b < batch; ++b) {
    double* tri = tri_ws + (size_t)b * TL.slab;
    const double hscale[4] = {0.0, 0.0, f ? f[b] : 1.0, 0.0};   // [2] the factor k_window_count reads, [3] its "bad" word
    SC_TRY(sc_stage_upload(ctx, tri + TL.d, d + (size_t)b * n, sizeof(double) * n));
    SC_TRY(sc_stage_upload(ctx, tri + TL.e, e + (size_t)b * n, sizeof(double) * n));
    SC_TRY(sc_stage_upload(ctx, tri + TL.hscale, hscale, sizeof(hscale)));
  }
  if (window) {
    if (own) {
      std::vector<RaggedRec> rec((size_t)batch, RaggedRec{});
      for (int b = 0; b < batch; ++b) rec[(size_t)b].own = own[b];
      SC_TRY(sc_stage_upload(ctx, d_own, rec.data(), sizeof(RaggedRec) * batch));
    }
    SC_TRY(window_count_batched(ctx, batch, tri_ws, TL, vl, vu, m, d_win, d_count, d_own));
  }
  SC_TRY(stein_batched(ctx, n, batch, tri_ws, TL, il, il + m - 1, d_w, m, d_x, (long long)n * m, d_stein, descs, d_win));
  if (window) SC_TRY(window_compact_batched(ctx, n, batch, m, d_win, d_w, d_x, d_wcopy, d_xcopy));
  SC_TRY(sc_stage_end(ctx));
  SC_HIP(ctx, hipStreamSynchronize(st));
  SC_TRY(sc_deferred_status(ctx));
  SC_HIP(ctx, hipMemcpy(w_out, d_w, sizeof(double) * rows, hipMemcpyDeviceToHost));
  if (vectors) SC_HIP(ctx, hipMemcpy(z_out, d_x, sizeof(double) * rows * n, hipMemcpyDeviceToHost));
  if (window && win_out) SC_HIP(ctx, hipMemcpy(win_out, d_win, sizeof(WinCount) * batch, hipMemcpyDeviceToHost));
  if (window && count_out) SC_HIP(ctx, hipMemcpy(count_out, d_count, sizeof(long long) * batch, hipMemcpyDeviceToHost));
  return SC_OK;
}

extern "C" int sc_dbg_stedc_leaf_max(int) { return sc_host::kLeafMax; }