// Driver of the batched dense symmetric eigensolver (replaces np.linalg.eigh at the reference's
// nma.py:61): mirror -> tridiagonalise (tridiag.hip) -> tridiagonal eigenproblem (stedc.hip, or Sturm
// bisection when only eigenvalues are wanted) -> back-transformation (backtransform.hip).
// Also owns the workspace layout: everything the stages need is carved out of ONE cached device
// allocation per context (sc_ctx::ws), sized by eigh_workspace_bytes().  Which path a solve takes: eigh_policy.h; the
// stages of a solve on host data (debug entries): eigh_debug.hip.
#include <algorithm>
#include <memory>
#include <vector>

#include "eigh_plan.h"

size_t tri_slab_doubles(int n, int nb, TriLayout* out) {
  TriLayout L{};
  L.n = n;
  L.nb = nb;
  const long long nt = (n + 63) / 64 + 1;
  long long off = 0;
  auto take = [&](long long cnt) { long long o = off; off += (cnt + 7) / 8 * 8; return o; };
  L.vw = take((long long)n * 2 * nb);
  L.wv = take((long long)n * 2 * nb);
  L.xraw = take(n);
  L.ypart = take(nt * n);
  L.dpart = take(nt * 2 * nb);
  L.npart = take(nt + 8);
  L.wvpart = take(nt + 8);
  L.d = take(n);
  L.e = take(n);
  L.tau = take(n);
  L.hscale = take(8);
  L.rctl = take(8);
  L.rrec = take(6 * ((n + 63) / 64 * 64));
  L.slab = off;
  if (out) *out = L;
  return (size_t)off;
}

SolvePlan make_solve_plan(const sc_ctx* ctx, int n, int batch, bool vectors, SolveKind kind) {
  const sc_host::EighEnv& E = sc_host::eigh_env();
  SolvePlan P;
  P.nb = E.nb;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes, 256); return o; };
  P.off_tri = take(tri_slab_doubles(n, P.nb, &P.TL) * 8 * batch);
  P.n_tri_desc = (n + P.nb - 1) / P.nb * batch;   // one SYR2K record per (panel, matrix)
  P.two = sc_host::two_stage_for(E, ctx ? ctx->two_stage : -1, resident_enabled(ctx), n, batch);
  if (P.two) {
    P.off_sb = take(sb_slab_doubles(n, batch, &P.SL) * 8 * batch);
    P.off_dia = take(sizeof(int) * ((size_t)n / 64 + 8));
    P.n_tri_desc = std::max(P.n_tri_desc, stage1_record_count(n, batch));
  }
  if (kind.partial) P.n_mid_desc = 2 * batch;
  if (vectors) {
    if (!kind.partial) {
      P.off_dc = take(dc_slab_doubles(n, &P.DL) * 8 * batch);
      P.n_mid_desc = 2 * dc_max_nodes(n) * batch;   // two half-GEMMs per merge
    } else if (kind.m_stein > 0) {
      P.off_stein = take(stein_workspace_doubles(n, kind.m_stein) * 8 * batch);
    }
    P.off_bt = take(bt_slab_doubles(n, &P.BL) * 8 * batch);
    // (the back-transformation indexes its scratch with the matrix stride: n x n per matrix also for m < n columns)
    P.off_qtmp = take((size_t)n * n * 8 * batch);
    if (!kind.partial) P.off_u = take((size_t)n * n * 8 * batch);
    P.n_bt_desc = bt_desc_count(n, batch);
  }
  P.off_desc = take(sizeof(GemmDesc) * ((size_t)P.n_tri_desc + P.n_mid_desc + P.n_bt_desc + 8));
  if (kind.window_k > 0) {
    P.off_win = take(sizeof(WinCount) * batch);
    P.off_wcopy = take(sizeof(double) * batch * (size_t)kind.window_k);
  }
  P.total = off;
  return P;
}

int SolveProfile::mark(int i) {
  if (!ctx->profiling) return SC_OK;
  if (i == 0) {
    ctx->phases.clear();
    for (auto& e : ev) SC_HIP(ctx, hipEventCreate(&e));
  }
  SC_HIP(ctx, hipEventRecord(ev[i], ctx->stream));
  return SC_OK;
}

int SolveProfile::finish(bool two, bool vectors) {
  if (!ctx->profiling) return SC_OK;
  SC_TRY(mark(3));
  SC_HIP(ctx, hipEventSynchronize(ev[3]));
  float t01 = 0, t12 = 0, t23 = 0;
  SC_HIP(ctx, hipEventElapsedTime(&t01, ev[0], ev[1]));
  SC_HIP(ctx, hipEventElapsedTime(&t12, ev[1], ev[2]));
  SC_HIP(ctx, hipEventElapsedTime(&t23, ev[2], ev[3]));
  ctx->last_timings[sc_ctx::kTimeTridiag] = t01;
  ctx->last_timings[sc_ctx::kTimeEigen] = t12;
  ctx->last_timings[sc_ctx::kTimeBacktransform] = t23;
  ctx->last_timings[sc_ctx::kTimeStageA] = ms_a;
  ctx->last_timings[sc_ctx::kTimeStageB] = ms_b;
  ctx->last_timings[sc_ctx::kTimeBt2] = !two ? sc_ctx::kTimeOneStage : (vectors ? ms_bt2 : sc_ctx::kTimeTwoStageValues);
  return SC_OK;
}

// SYR2K records of the one-stage panels, one per (panel, matrix), uploaded to the plan's tridiagonalisation records
static int upload_syr2k_records(sc_ctx* ctx, double* d_a, int n, int batch, const SolvePlan& P, char* base) {
  const long long stride_a = (long long)n * n;
  double* tri_ws = (double*)(base + P.off_tri);
  const int npanels = (n + P.nb - 1) / P.nb;
  std::vector<GemmDesc> h((size_t)npanels * batch);
  for (int p = 0; p < npanels; ++p) {
    const int pend = std::min((p + 1) * P.nb, n);
    for (int b = 0; b < batch; ++b) {
      double* ws = tri_ws + (size_t)b * P.TL.slab;
      GemmDesc D{};
      D.a = ws + P.TL.vw + pend; D.sa_i = 1; D.sa_k = n;
      D.b = ws + P.TL.wv + pend; D.sb_k = n; D.sb_j = 1;
      D.c = d_a + (size_t)b * stride_a + (size_t)pend * n + pend; D.ldc = n;
      D.m = n - pend; D.n = n - pend; D.k = 2 * P.nb;
      D.alpha = -1.0; D.beta = 1.0;
      D.lower_only = 1;
      h[(size_t)p * batch + b] = D;
    }
  }
  return sc_stage_upload(ctx, P.tri_descs(base), h.data(), h.size() * sizeof(GemmDesc));
}

// (the two-stage path uploads records of its own to the same place and reads no others: the SYR2K records are the
// one-stage path's alone)
int tridiagonalise(sc_ctx* ctx, double* d_a, int n, int batch, const SolvePlan& P, char* base, SolveProfile& prof,
                   double* d_band_copy) {
  const long long stride_a = (long long)n * n;
  double* tri_ws = (double*)(base + P.off_tri);
  SC_TRY(prepare_matrix_batched(ctx, d_a, stride_a, n, batch, tri_ws, P.TL));
  if (P.two)
    return sytrd_2stage_batched(ctx, d_a, stride_a, n, batch, tri_ws, P.TL, (double*)(base + P.off_sb), P.SL,
                                (int*)(base + P.off_dia), P.tri_descs(base), &prof.ms_a, &prof.ms_b, d_band_copy);
  SC_TRY(upload_syr2k_records(ctx, d_a, n, batch, P, base));
  return tridiag_batched(ctx, d_a, stride_a, n, batch, tri_ws, P.TL, P.tri_descs(base), &prof.ms_a, &prof.ms_b);
}

namespace {

// ---- eigenvalues only: Sturm bisection, one thread per eigenvalue ------------------------------------------
__global__ __launch_bounds__(256) void k_sturm(const double* __restrict__ tri_all, TriLayout TL,
                                               double* __restrict__ w_all, long long stride_w) {
  const double* tri = tri_all + (size_t)blockIdx.y * TL.slab;
  const double* d = tri + TL.d;
  const double* e = tri + TL.e;
  const int n = TL.n;
  __shared__ double red[8];
  // Gershgorin bounds + pivmin (block-wide)
  double lo = 1e300, hi = -1e300, emax = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const double el = i > 0 ? fabs(e[i - 1]) : 0.0, er = i < n - 1 ? fabs(e[i]) : 0.0;
    lo = fmin(lo, d[i] - el - er);
    hi = fmax(hi, d[i] + el + er);
    emax = fmax(emax, er);
  }
  for (int off = 32; off > 0; off >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, off));
    hi = fmax(hi, __shfl_xor(hi, off));
    emax = fmax(emax, __shfl_xor(emax, off));
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[w] = lo; red[4 + w] = hi; }
  __syncthreads();
  lo = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
  hi = fmax(fmax(red[4], red[5]), fmax(red[6], red[7]));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = emax;
  __syncthreads();
  emax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  const double span = fmax(fabs(lo), fabs(hi));
  const double pivmin = fmax(2.2250738585072014e-308 * fmax(1.0, emax * emax), 1e-290);
  lo -= 2.0 * 2.2e-16 * span * n + 2.0 * pivmin;
  hi += 2.0 * 2.2e-16 * span * n + 2.0 * pivmin;

  const int k = blockIdx.x * blockDim.x + threadIdx.x;  // eigenvalue index (ascending)
  if (k >= n) return;
  if (span == 0.0) {   // d = e = 0: every eigenvalue is exactly 0 (the interval widened by pivmin would give 1e-290 in magnitude)
    w_all[(size_t)blockIdx.y * stride_w + k] = 0.0;
    return;
  }
  double a = lo, b = hi;
  for (int it = 0; it < 120; ++it) {
    const double mid = 0.5 * (a + b);
    if (mid <= a || mid >= b) break;
    int cnt = 0;
    double q = d[0] - mid;
    if (fabs(q) < pivmin) q = -pivmin;
    cnt += q < 0.0;
    for (int i = 1; i < n; ++i) {
      const double ee = e[i - 1];
      q = d[i] - mid - ee * ee / q;
      if (fabs(q) < pivmin) q = -pivmin;
      cnt += q < 0.0;
    }
    if (cnt > k) b = mid; else a = mid;
  }
  w_all[(size_t)blockIdx.y * stride_w + k] = 0.5 * (a + b);
}

}  // namespace

int sturm_bisect_batched(sc_ctx* ctx, int n, int batch, const double* d_tri_ws, const TriLayout& TL,
                         double* d_w, long long stride_w) {
  hipLaunchKernelGGL(k_sturm, dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, ctx->stream,
                     d_tri_ws, TL, d_w, stride_w);
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

size_t eigh_workspace_bytes(int64_t n, int64_t batch, bool want_vectors) {
  return make_solve_plan(nullptr, (int)n, (int)batch, want_vectors).total;
}

// Once work has been forked onto the context's second stream, EVERY way out of the solve must make the main stream wait
// for it: the kernels queued there read and write d_a, the band workspace and the back-transformation workspace, which
// the caller may reuse or free as soon as the call has returned, and the next solve on the context must be ordered
// after them (the band reduction's side streams got the same guard in round 3).
struct AuxJoinGuard {
  sc_ctx* ctx;
  hipStream_t main;
  bool forked = false, joined = false;
  ~AuxJoinGuard() {
    ctx->stream = main;   // (a failing call between the two assignments below must not leave the context on the aux stream)
    if (forked && !joined) {
      (void)hipEventRecord(ctx->aux_join, ctx->aux_stream);
      (void)hipStreamWaitEvent(main, ctx->aux_join, 0);
    }
  }
};

int eigh_batched_async(sc_ctx* ctx, double* d_a, int64_t n64, int64_t batch64, double* d_w, double* d_v) {
  if (n64 > 46000) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "matrix order %lld too large", (long long)n64);
  const int n = (int)n64, batch = (int)batch64;
  const bool vectors = d_v != nullptr;
  hipStream_t st = ctx->stream;
  const SolvePlan P = make_solve_plan(ctx, n, batch, vectors);
  SC_TRY(sc_reserve_ws(ctx, P.total));
  char* base = (char*)ctx->ws;
  double* tri_ws = (double*)(base + P.off_tri);
  const long long stride_a = (long long)n * n;

  SolveProfile prof(ctx);
  double* sb_ws = (double*)(base + P.off_sb);
  std::unique_ptr<PhaseTimer> t_tf;   // T factors of the stage-2 diamonds (second stream)
  SC_TRY(prof.mark(0));
  SC_TRY(tridiagonalise(ctx, d_a, n, batch, P, base, prof, nullptr));
  SC_TRY(prof.mark(1));

  if (!vectors) {
    SC_TRY(sturm_bisect_batched(ctx, n, batch, tri_ws, P.TL, d_w, n));
    SC_TRY(unscale_values_batched(ctx, d_w, n, n, batch, tri_ws, P.TL));
    SC_TRY(prof.mark(2));
  } else {
    double* dc_ws = (double*)(base + P.off_dc);
    double* bt_ws = (double*)(base + P.off_bt);
    double* q_tmp = (double*)(base + P.off_qtmp);
    double* u = (double*)(base + P.off_u);
    GemmDesc* bt_descs = P.bt_descs(base);
    const int bt_off = P.two ? sb_band_width() : 1;
    const sc_host::AuxPlan aux_plan = sc_host::aux_plan(sc_host::eigh_env(), P.two, batch, resident_enabled(ctx));
    const bool use_aux = aux_plan == sc_host::AuxPlan::Fork;
    AuxJoinGuard aux{ctx, st};
    if (aux_plan == sc_host::AuxPlan::TFactorsMain) {
      t_tf.reset(new PhaseTimer(ctx, "dia_tfactor", st));
      t_tf->start();
      SC_TRY(bt2_prepare(ctx, n, batch, sb_ws, P.SL, st));
      t_tf->stop();
    } else if (use_aux) {
      // what the back-transformations need besides Z does not depend on the tridiagonal eigenproblem: the diamonds' T
      // factors (two-stage) and the cleaned reflectors, Gram products and T factors of the Q1 blocks run on a second
      // stream alongside the D&C (their descriptors are uploaded on the main stream before the fork)
      SC_TRY(backtransform_batched(ctx, d_a, stride_a, n, batch, tri_ws, P.TL, bt_ws, P.BL, d_v, stride_a, n, q_tmp,
                                   bt_descs, bt_off, /*phase=*/1));
      SC_TRY(sc_aux_stream(ctx));
      SC_HIP(ctx, hipEventRecord(ctx->aux_fork, st));
      SC_HIP(ctx, hipStreamWaitEvent(ctx->aux_stream, ctx->aux_fork, 0));
      aux.forked = true;
      if (P.two) {
        t_tf.reset(new PhaseTimer(ctx, "dia_tfactor", ctx->aux_stream));
        t_tf->start();
        SC_TRY(bt2_prepare(ctx, n, batch, sb_ws, P.SL, ctx->aux_stream));
        t_tf->stop();
      }
      {
        StreamScope on_aux(ctx, ctx->aux_stream);
        SC_TRY(backtransform_batched(ctx, d_a, stride_a, n, batch, tri_ws, P.TL, bt_ws, P.BL, d_v, stride_a, n, q_tmp,
                                     bt_descs, bt_off, /*phase=*/2));   // (an error: joined by the guard)
      }
      SC_HIP(ctx, hipEventRecord(ctx->aux_join, ctx->aux_stream));
    }
    SC_TRY(stedc_batched(ctx, n, batch, tri_ws, P.TL, dc_ws, P.DL, d_w, n, d_v, q_tmp, u, stride_a, P.mid_descs(base)));
    SC_TRY(unscale_values_batched(ctx, d_w, n, n, batch, tri_ws, P.TL));
    SC_TRY(prof.mark(2));
    if (use_aux) {
      SC_HIP(ctx, hipStreamWaitEvent(st, ctx->aux_join, 0));
      aux.joined = true;
    }
    if (P.two)
      SC_TRY(bt2_batched(ctx, n, batch, sb_ws, P.SL, (const int*)(base + P.off_dia), d_v, stride_a, n, &prof.ms_bt2));
    SC_TRY(backtransform_batched(ctx, d_a, stride_a, n, batch, tri_ws, P.TL, bt_ws, P.BL, d_v, stride_a, n, q_tmp,
                                 bt_descs, bt_off, /*phase=*/use_aux ? 3 : 0));
  }
  SC_TRY(prof.finish(P.two, vectors));
  if (t_tf) t_tf->finish();
  return sc_stage_end(ctx);   // (no synchronisation: the descriptor tables went through the context's pinned arena)
}

// Synchronising form for the host-pointer entry points: errors of THIS solve (non-finite input, QL failure) are
// returned by it, as np.linalg.eigh raises them at nma.py:61.
int eigh_batched(sc_ctx* ctx, double* d_a, int64_t n, int64_t batch, double* d_w, double* d_v) {
  SC_TRY(eigh_batched_async(ctx, d_a, n, batch, d_w, d_v));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return sc_deferred_status(ctx);
}


// ---- partial spectrum --------------------------------------------------------------------------------------
namespace {

// bisection, inverse iteration and back-transformation of m eigenpairs per matrix (il.., or from d_win[b].start);
// d_stein: stein_workspace_doubles(n, m) * batch doubles when vectors are wanted
int partial_eigenpairs(sc_ctx* ctx, double* d_a, int n, int batch, const SolvePlan& P, char* base, int il, int m,
                       const WinCount* d_win, double* d_w, double* d_v, double* d_stein, SolveProfile& prof) {
  const long long stride_a = (long long)n * n;
  double* tri_ws = (double*)(base + P.off_tri);
  GemmDesc* d2 = P.mid_descs(base);
  hipStream_t st = ctx->stream;
  const int iu = il + m - 1;
  if (!d_v) {
    SC_TRY(stein_batched(ctx, n, batch, tri_ws, P.TL, il, iu, d_w, m, nullptr, 0, nullptr, d2, d_win));
    SC_TRY(unscale_values_batched(ctx, d_w, m, m, batch, tri_ws, P.TL));
    return prof.mark(2);
  }
  const long long stride_x = (long long)n * m;
  SC_TRY(stein_batched(ctx, n, batch, tri_ws, P.TL, il, iu, d_w, m, d_v, stride_x, d_stein, d2, d_win));
  SC_TRY(unscale_values_batched(ctx, d_w, m, m, batch, tri_ws, P.TL));
  SC_TRY(prof.mark(2));
  if (P.two) {
    double* sb_ws = (double*)(base + P.off_sb);
    PhaseTimer t_tf(ctx, "dia_tfactor", st);
    t_tf.start();
    SC_TRY(bt2_prepare(ctx, n, batch, sb_ws, P.SL, st));
    t_tf.stop();
    SC_TRY(bt2_batched(ctx, n, batch, sb_ws, P.SL, (const int*)(base + P.off_dia), d_v, stride_x, m, &prof.ms_bt2));
    t_tf.finish();
  }
  return backtransform_batched(ctx, d_a, stride_a, n, batch, tri_ws, P.TL, (double*)(base + P.off_bt), P.BL, d_v,
                               stride_x, m, (double*)(base + P.off_qtmp), P.bt_descs(base), P.two ? sb_band_width() : 1);
}

// one solve of the batch: eigenpairs il .. il + m - 1 of every matrix, or (window) the K = m slots of a value window
struct ValueWindow {
  double vl, vu;
  long long* d_count;
  const RaggedRec* d_own;   // null, or the own orders of padded slots
};

int partial_batched_async(sc_ctx* ctx, double* d_a, int n, int batch, int il, int m, const ValueWindow* window,
                          double* d_w, double* d_v) {
  const SolvePlan P = make_solve_plan(ctx, n, batch, d_v != nullptr, {true, m, window ? m : 0});
  SC_TRY(sc_reserve_ws(ctx, P.total));
  char* base = (char*)ctx->ws;
  SolveProfile prof(ctx);
  SC_TRY(prof.mark(0));
  SC_TRY(tridiagonalise(ctx, d_a, n, batch, P, base, prof, nullptr));
  SC_TRY(prof.mark(1));
  WinCount* d_win = nullptr;
  if (window) {
    d_win = (WinCount*)(base + P.off_win);
    SC_TRY(window_count_batched(ctx, batch, (const double*)(base + P.off_tri), P.TL, window->vl, window->vu, m, d_win,
                                window->d_count, window->d_own));
  }
  SC_TRY(partial_eigenpairs(ctx, d_a, n, batch, P, base, il, m, d_win, d_w, d_v, (double*)(base + P.off_stein), prof));
  if (window)   // (the n x n scratch of the back-transformation is free again: the copy of v goes there)
    SC_TRY(window_compact_batched(ctx, n, batch, m, d_win, d_w, d_v, (double*)(base + P.off_wcopy),
                                  (double*)(base + P.off_qtmp)));
  SC_TRY(prof.finish(P.two, d_v != nullptr));
  return sc_stage_end(ctx);
}

}  // namespace

int check_window(sc_ctx* ctx, double vl, double vu) {
  if (!(vl < vu))   // (also a NaN bound)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "eigenvalue window (%g, %g] is empty or not a number: need vl < vu", vl,
                        vu);
  return SC_OK;
}

int eigh_range_batched_async(sc_ctx* ctx, double* d_a, int64_t n64, int64_t batch64, int64_t il64, int64_t iu64,
                             double* d_w, double* d_v) {
  if (n64 > 46000) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "matrix order %lld too large", (long long)n64);
  const int n = (int)n64, batch = (int)batch64, il = (int)il64, iu = (int)iu64;
  if (il < 0 || iu < il || iu >= n)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad eigenvalue index range [%d, %d] for order %d", il, iu, n);
  return partial_batched_async(ctx, d_a, n, batch, il, iu - il + 1, nullptr, d_w, d_v);
}

int eigh_range_batched(sc_ctx* ctx, double* d_a, int64_t n, int64_t batch, int64_t il, int64_t iu, double* d_w,
                       double* d_v) {
  SC_TRY(eigh_range_batched_async(ctx, d_a, n, batch, il, iu, d_w, d_v));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return sc_deferred_status(ctx);
}

int eigh_window_batched_async(sc_ctx* ctx, double* d_a, int64_t n64, int64_t batch64, double vl, double vu, int64_t K64,
                              double* d_w, double* d_v, int64_t* d_count, const RaggedRec* d_own) {
  if (n64 > 46000) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "matrix order %lld too large", (long long)n64);
  SC_TRY(check_window(ctx, vl, vu));
  if (K64 < 1 || K64 > n64)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "window capacity %lld outside 1..%lld", (long long)K64, (long long)n64);
  const ValueWindow window{vl, vu, (long long*)d_count, d_own};
  return partial_batched_async(ctx, d_a, (int)n64, (int)batch64, 0, (int)K64, &window, d_w, d_v);
}

// One matrix: tridiagonalise, count the window on the device, read m on the host (the one synchronisation), then the m
// eigenpairs exactly as the index range il .. il + m - 1 computes them.  The inverse-iteration workspace and the results
// depend on m, which sc_reserve_ws could not know: they live in a buffer of their own (ctx->win_ws), so that the tri / sb
// slabs the eigenpairs still need never move.  On success *d_w / *d_v point into that buffer (valid until the next
// window solve on the context).
int eigh_window(sc_ctx* ctx, double* d_a, int64_t n64, double vl, double vu, bool vectors, int64_t* m_out, double** d_w,
                double** d_v) {
  if (n64 > 46000) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "matrix order %lld too large", (long long)n64);
  SC_TRY(check_window(ctx, vl, vu));
  const int n = (int)n64;
  *m_out = 0;
  *d_w = *d_v = nullptr;
  const SolvePlan P = make_solve_plan(ctx, n, 1, vectors, {true, 0, 1});
  SC_TRY(sc_reserve_ws(ctx, P.total));
  char* base = (char*)ctx->ws;
  SolveProfile prof(ctx);
  SC_TRY(prof.mark(0));
  SC_TRY(tridiagonalise(ctx, d_a, n, 1, P, base, prof, nullptr));
  SC_TRY(prof.mark(1));
  WinCount* d_win = (WinCount*)(base + P.off_win);
  SC_TRY(window_count_batched(ctx, 1, (const double*)(base + P.off_tri), P.TL, vl, vu, 1, d_win, nullptr));
  WinCount h{};
  SC_HIP(ctx, hipMemcpyAsync(&h, d_win, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  SC_TRY(sc_deferred_status(ctx));   // (a matrix with a NaN / Inf entry: LinAlgError, as the other solves)
  const int m = h.count;
  if (m <= 0) return sc_stage_end(ctx);
  if (h.il < 0 || h.il + m > n)
    return sc_set_error(ctx, SC_ERR_HIP, "window count [%d, %d) outside order %d", h.il, h.il + m, n);
  const size_t stein_bytes = vectors ? align_up(stein_workspace_doubles(n, m) * 8, 256) : 0;
  const size_t w_bytes = align_up((size_t)m * 8, 256);
  SC_TRY(sc_reserve_win(ctx, stein_bytes + w_bytes + (vectors ? (size_t)m * n * 8 : 0)));
  char* wb = (char*)ctx->win_ws;
  double* w = (double*)(wb + stein_bytes);
  double* v = vectors ? (double*)(wb + stein_bytes + w_bytes) : nullptr;
  SC_TRY(partial_eigenpairs(ctx, d_a, n, 1, P, base, h.il, m, nullptr, w, v, (double*)wb, prof));
  SC_TRY(prof.finish(P.two, vectors));
  SC_TRY(sc_stage_end(ctx));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  SC_TRY(sc_deferred_status(ctx));
  *m_out = m;
  *d_w = w;
  *d_v = v;
  return SC_OK;
}


// ---- Hermitian pseudo-inverse from the eigenpairs (F1: covariance) ------------------------------------------
// np.linalg.pinv(M, hermitian=True, rcond) as used at anm.py:115,135 / gnm.py:108,128:
//   M = U diag(w) U^T;  pinv = (U * s) U^T  with  s_i = 1/w_i if |w_i| > rcond * max|w| else 0.
namespace {
__global__ void k_pinv_scale(const double* __restrict__ q, const double* __restrict__ w, int n, double rcond,
                             double* __restrict__ qs) {
  __shared__ double s_cut;
  if (threadIdx.x == 0) {
    double mx = 0.0;
    for (int i = 0; i < n; ++i) mx = fmax(mx, fabs(w[i]));   // w is ascending: max |w| is at one of the ends
    s_cut = rcond * mx;
  }
  __syncthreads();
  const int col = blockIdx.x;
  const double wi = w[col];
  const double s = fabs(wi) > s_cut ? 1.0 / wi : 0.0;
  for (int r = threadIdx.x; r < n; r += blockDim.x) qs[(size_t)col * n + r] = q[(size_t)col * n + r] * s;
}
}  // namespace

int pinvh_device(sc_ctx* ctx, double* d_a, int64_t n64, double rcond, double* d_out) {
  const int n = (int)n64;
  hipStream_t st = ctx->stream;
  // buffers: Q (n^2) | QS (n^2) | w (n) | desc from a cached grow-only allocation of the context (its other cached
  // buffers are all in use by the caller and by eigh_batched while this runs)
  const size_t nn = align_up(sizeof(double) * (size_t)n * n, 256), nw = align_up(sizeof(double) * (size_t)n, 256);
  SC_TRY(sc_reserve_pinv(ctx, 2 * nn + nw + sizeof(GemmDesc)));
  char* d_base = reinterpret_cast<char*>(ctx->pinv_ws);
  double* d_q = reinterpret_cast<double*>(d_base);
  double* d_qs = reinterpret_cast<double*>(d_base + nn);
  double* d_w = reinterpret_cast<double*>(d_base + 2 * nn);
  GemmDesc* d_desc = reinterpret_cast<GemmDesc*>(d_base + 2 * nn + nw);
  int rc = eigh_batched(ctx, d_a, n, 1, d_w, d_q);
  if (rc == SC_OK) {
    hipLaunchKernelGGL(k_pinv_scale, dim3((unsigned)n), dim3(256), 0, st, d_q, d_w, n, rcond, d_qs);
    GemmDesc D{};
    D.a = d_qs; D.sa_i = 1; D.sa_k = n;       // (U * s)
    D.b = d_q; D.sb_k = n; D.sb_j = 1;        // U^T: B(k,j) = U[j, k]
    D.c = d_out; D.ldc = n; D.m = n; D.n = n; D.k = n;
    D.alpha = 1.0; D.beta = 0.0;
    rc = sc_stage_upload(ctx, d_desc, &D, sizeof(D));
    if (rc == SC_OK) rc = launch_gemm_f64(ctx, d_desc, {.count = 1, .max_m = n, .max_n = n, .layout = kGemmAmBn});
    if (rc == SC_OK) rc = sc_stage_end(ctx);
  }
  return rc;
}


