// C ABI (include/springcraft_hip.h), the context: error text, the grow-only device reservations and the scratch protocol,
// the upload staging ring, deferred status and event collection, aux / side streams, create / destroy, profiling,
// counters, the sc_dbg_* switches.  Host-side plumbing only, as all api_*.hip units: no kernel lives in them.
#include <algorithm>
#include <cstdarg>
#include <cstring>

#include "api_internal.h"

int sc_set_error(sc_ctx* ctx, int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf;
  return code;
}

// Grow-only cached device buffers of the context: nothing happens while the buffer is large enough; else the context's
// stream is drained, the buffer freed and a larger one allocated.
static int reserve(sc_ctx* ctx, void*& buf, size_t& have, size_t bytes, bool collect_events = false) {
  if (bytes <= have) return SC_OK;
  if (buf) {
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (collect_events) SC_TRY(sc_collect_events(ctx));
    SC_HIP(ctx, hipFree(buf));
    buf = nullptr;
    have = 0;
  }
  SC_HIP(ctx, hipMalloc(&buf, bytes));
  have = bytes;
  return SC_OK;
}

int sc_reserve_ws(sc_ctx* ctx, size_t bytes) { return reserve(ctx, ctx->ws, ctx->ws_bytes, bytes); }
int sc_reserve_scratch(sc_ctx* ctx, size_t bytes) { return reserve(ctx, ctx->scratch, ctx->scratch_bytes, bytes); }
int sc_reserve_pinv(sc_ctx* ctx, size_t bytes) { return reserve(ctx, ctx->pinv_ws, ctx->pinv_ws_bytes, bytes); }
int sc_reserve_win(sc_ctx* ctx, size_t bytes) { return reserve(ctx, ctx->win_ws, ctx->win_ws_bytes, bytes); }
int sc_reserve_modes(sc_ctx* ctx, size_t bytes) { return reserve(ctx, ctx->modes_ws, ctx->modes_ws_bytes, bytes); }
// (events are collected before the free: the last chase's control block lives in the buffer that goes away)
int sc_reserve_dc_aux(sc_ctx* ctx, size_t bytes) { return reserve(ctx, ctx->dc_aux, ctx->dc_aux_bytes, bytes, true); }

int carve_scratch(sc_ctx* ctx, const ScratchLayout& layout) {
  sc_host::Arena measure;
  layout(measure);
  SC_TRY(sc_reserve_scratch(ctx, measure.bytes()));
  sc_host::Arena carve(ctx->scratch, measure.bytes());
  layout(carve);
  if (carve.overrun())   // only a layout that is not a pure function of its arena gets here
    return sc_set_error(ctx, SC_ERR_HIP, "internal error: a scratch layout carved more than the %zu bytes it measured",
                        measure.bytes());
  return SC_OK;
}

int sc_stage_upload(sc_ctx* ctx, void* d_dst, const void* h_src, size_t bytes) {
  if (bytes == 0) return SC_OK;
  const int c = ctx->h_stage_cur;
  if (ctx->h_stage_pending[c]) {   // this arena was last used two solves ago: its copies must have left it
    SC_HIP(ctx, hipEventSynchronize(ctx->h_stage_done[c]));
    ctx->h_stage_pending[c] = false;
    ctx->h_stage_off[c] = 0;
  }
  const size_t need = align_up(ctx->h_stage_off[c] + bytes, 256);
  if (need > ctx->h_stage_bytes[c]) {
    // grow: copies of this solve may still be reading the old arena
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->h_stage[c]) SC_HIP(ctx, hipHostFree(ctx->h_stage[c]));
    ctx->h_stage[c] = nullptr;
    ctx->h_stage_bytes[c] = 0;
    ctx->h_stage_off[c] = 0;
    const size_t cap = std::max<size_t>(2 * need, (size_t)1 << 20);
    SC_HIP(ctx, hipHostMalloc((void**)&ctx->h_stage[c], cap, hipHostMallocDefault));
    ctx->h_stage_bytes[c] = cap;
  }
  if (!ctx->h_stage_done[c]) SC_HIP(ctx, hipEventCreateWithFlags(&ctx->h_stage_done[c], hipEventDisableTiming));
  char* slot = ctx->h_stage[c] + ctx->h_stage_off[c];
  memcpy(slot, h_src, bytes);
  ctx->h_stage_off[c] = align_up(ctx->h_stage_off[c] + bytes, 256);
  SC_HIP(ctx, hipMemcpyAsync(d_dst, slot, bytes, hipMemcpyHostToDevice, ctx->stream));
  return SC_OK;
}

int sc_stage_end(sc_ctx* ctx) {
  const int c = ctx->h_stage_cur;
  if (!ctx->h_stage_done[c] || ctx->h_stage_off[c] == 0) return SC_OK;
  SC_HIP(ctx, hipEventRecord(ctx->h_stage_done[c], ctx->stream));
  ctx->h_stage_pending[c] = true;
  ctx->h_stage_cur = 1 - c;
  return SC_OK;
}

int sc_collect_events(sc_ctx* ctx) {
  if (!ctx->d_status) return SC_OK;
  unsigned long long h[kSpStatusWords] = {0};
  SC_HIP(ctx, hipMemcpy(h, ctx->d_status, sizeof(h), hipMemcpyDeviceToHost));
  bool any = false;
  for (int i = 2; i < kSpStatusWords; ++i) any = any || h[i] != 0;
  if (any) SC_HIP(ctx, hipMemset(ctx->d_status + 2, 0, sizeof(unsigned long long) * (kSpStatusWords - 2)));
  ctx->cnt_chase_resumed += (long long)h[2];
  ctx->cnt_chase_timeouts += (long long)h[3];
  ctx->cnt_chase_sweeps += (long long)h[4];
  ctx->cnt_coop_timeouts += (long long)h[5];
  ctx->cnt_chase_incomplete += (long long)h[6];
  ctx->cnt_resident_takeovers += (long long)h[7];
  ctx->cnt_resident_rollcalls += (long long)h[8];
  ctx->cnt_resident_lost += (long long)h[9];
  if (h[7]) ctx->resident_lost_at = (long long)h[10];
  if (h[11]) ctx->potrf_failed = (long long)h[11];
  // (one failed roll call can be a launch whose workgroups were dispatched late; the context gives the kernel up at the third)
  ctx->resident_strikes += (int)h[8];
  if (h[9] || (h[8] && ctx->resident_strikes >= 3)) ctx->resident_ok = 0;
  // a context whose persistent kernels ran into a bound keeps to the launch-per-wavefront / chunked forms from here on
  if (h[3] || h[6]) ctx->chase_ok = 0;
  if (h[5]) ctx->coop_ok = 0;
  if (ctx->last_chase_ctl) {   // the most recent chase's control block: tickets per XCD, where a wait timed out
    int c[kChaseCtlInts] = {0};
    SC_HIP(ctx, hipMemcpy(c, ctx->last_chase_ctl, sizeof(c), hipMemcpyDeviceToHost));
    for (int x = 0; x < 8; ++x) ctx->chase_tickets[x] = c[2 + x];
    if (c[0] && c[1] == 0) { ctx->chase_wait[0] = c[10]; ctx->chase_wait[1] = c[11]; ctx->chase_wait[2] = c[12]; }
    ctx->last_chase_ctl = nullptr;
  }
  return SC_OK;
}

int sc_deferred_status(sc_ctx* ctx) {
  if (!ctx->d_status) return SC_OK;
  SC_TRY(sc_collect_events(ctx));
  unsigned long long h[2] = {0, 0};
  SC_HIP(ctx, hipMemcpy(h, ctx->d_status, sizeof(h), hipMemcpyDeviceToHost));
  const long long potrf_failed = ctx->potrf_failed;
  ctx->potrf_failed = 0;
  if (h[0] == 0 && h[1] == 0 && potrf_failed == 0) return SC_OK;
  if (h[0] || h[1]) SC_HIP(ctx, hipMemset(ctx->d_status, 0, sizeof(h)));
  // np.linalg.cholesky raises LinAlgError("Matrix is not positive definite"); the NaN that a failed factor hands to an
  // eigensolve behind it is the same failure, named by its cause
  if (potrf_failed)
    return sc_set_error(ctx, SC_ERR_NOCONV, "Matrix is not positive definite: the Cholesky factorisation of matrix %lld of the batch "
                        "met a pivot that is not positive", potrf_failed - 1);
  if (h[0])   // np.linalg.eigh raises LinAlgError("Eigenvalues did not converge") for such input (nma.py:61)
    return sc_set_error(ctx, SC_ERR_NOCONV, "Eigenvalues did not converge: matrix %llu of the batch contains NaN or Inf",
                        h[0] - 1ull);
  return sc_set_error(ctx, SC_ERR_NOCONV, "tridiagonal QL iteration did not converge");
}

int sc_aux_stream(sc_ctx* ctx) {
  if (ctx->aux_stream) return SC_OK;
  SC_HIP(ctx, hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking));
  SC_HIP(ctx, hipEventCreateWithFlags(&ctx->aux_fork, hipEventDisableTiming));
  SC_HIP(ctx, hipEventCreateWithFlags(&ctx->aux_join, hipEventDisableTiming));
  return SC_OK;
}

int sc_side_streams(sc_ctx* ctx, int count) {
  while ((int)ctx->side_streams.size() < count) {
    hipStream_t s = nullptr;
    hipEvent_t e = nullptr;
    SC_HIP(ctx, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      (void)hipStreamDestroy(s);
      return sc_set_error(ctx, SC_ERR_HIP, "hipEventCreateWithFlags failed");
    }
    ctx->side_streams.push_back(s);
    ctx->side_joins.push_back(e);
  }
  return SC_OK;
}

static int ctx_create_impl(int device, void* stream, bool own, sc_ctx** out) {
  if (!out) return SC_ERR_INVALID_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count)
    return SC_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return SC_ERR_NO_DEVICE;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return SC_ERR_NO_DEVICE;  // gfx950 code objects only
  if (hipSetDevice(device) != hipSuccess) return SC_ERR_NO_DEVICE;
  sc_ctx* ctx = new sc_ctx();
  ctx->device = device;
  ctx->num_cus = prop.multiProcessorCount;
  if (own) {
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
      delete ctx;
      return SC_ERR_HIP;
    }
    ctx->own_stream = true;
  } else {
    ctx->stream = (hipStream_t)stream;
  }
  // (d_zeros: the page of zeros k_symm3's loaders read -- symm3.hip --, zeroed here, long before any stream uses it)
  if (hipMalloc((void**)&ctx->d_status, kSpStatusWords * sizeof(unsigned long long)) != hipSuccess ||
      hipMemset(ctx->d_status, 0, kSpStatusWords * sizeof(unsigned long long)) != hipSuccess ||
      hipMalloc((void**)&ctx->d_zeros, 16384) != hipSuccess || hipMemset(ctx->d_zeros, 0, 16384) != hipSuccess ||
      hipMalloc((void**)&ctx->d_chase_ctl, kChaseCtlInts * sizeof(int)) != hipSuccess ||
      hipMemset(ctx->d_chase_ctl, 0, kChaseCtlInts * sizeof(int)) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess) {
    if (ctx->d_status) (void)hipFree(ctx->d_status);
    if (ctx->d_zeros) (void)hipFree(ctx->d_zeros);
    if (ctx->d_chase_ctl) (void)hipFree(ctx->d_chase_ctl);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return SC_ERR_NOMEM;
  }
  *out = ctx;
  return SC_OK;
}

extern "C" {

int sc_ctx_create(int device, sc_ctx** out) { return ctx_create_impl(device, nullptr, true, out); }

int sc_ctx_create_on_stream(int device, void* hip_stream, sc_ctx** out) {
  return ctx_create_impl(device, hip_stream, false, out);
}

void sc_ctx_destroy(sc_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->ws) (void)hipFree(ctx->ws);
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  if (ctx->dc_aux) (void)hipFree(ctx->dc_aux);
  if (ctx->pinv_ws) (void)hipFree(ctx->pinv_ws);
  if (ctx->win_ws) (void)hipFree(ctx->win_ws);
  if (ctx->modes_ws) (void)hipFree(ctx->modes_ws);
  if (ctx->d_status) (void)hipFree(ctx->d_status);
  if (ctx->d_zeros) (void)hipFree(ctx->d_zeros);
  if (ctx->d_chase_ctl) (void)hipFree(ctx->d_chase_ctl);
  for (int c = 0; c < 2; ++c) {
    if (ctx->h_stage[c]) (void)hipHostFree(ctx->h_stage[c]);
    if (ctx->h_stage_done[c]) (void)hipEventDestroy(ctx->h_stage_done[c]);
  }
  if (ctx->aux_stream) {
    (void)hipStreamSynchronize(ctx->aux_stream);
    (void)hipStreamDestroy(ctx->aux_stream);
    (void)hipEventDestroy(ctx->aux_fork);
    (void)hipEventDestroy(ctx->aux_join);
  }
  for (size_t i = 0; i < ctx->side_streams.size(); ++i) {
    (void)hipStreamSynchronize(ctx->side_streams[i]);
    (void)hipStreamDestroy(ctx->side_streams[i]);
    (void)hipEventDestroy(ctx->side_joins[i]);
  }
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

const char* sc_last_error(sc_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int sc_host_alloc(size_t bytes, void** out) {
  if (!out || bytes == 0) return SC_ERR_INVALID_ARG;
  *out = nullptr;
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess || !p) {
    (void)hipGetLastError();
    return SC_ERR_NOMEM;
  }
  *out = p;
  return SC_OK;
}

int sc_host_free(void* p) {
  if (!p) return SC_OK;
  return hipHostFree(p) == hipSuccess ? SC_OK : SC_ERR_HIP;
}

int sc_ctx_synchronize(sc_ctx* ctx) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_HIP(ctx, hipSetDevice(ctx->device));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return sc_deferred_status(ctx);   // errors of the device-pointer solves enqueued since the last call
}

int sc_device_info(sc_ctx* ctx, char* buf, size_t buflen) {
  if (!ctx || !buf || buflen == 0) return SC_ERR_INVALID_ARG;
  hipDeviceProp_t prop;
  SC_HIP(ctx, hipGetDeviceProperties(&prop, ctx->device));
  snprintf(buf, buflen, "%s %s, %d CUs, %.0f GiB", prop.gcnArchName, prop.name,
           prop.multiProcessorCount, (double)prop.totalGlobalMem / (1 << 30));
  return SC_OK;
}

int sc_ctx_set_profiling(sc_ctx* ctx, int enabled) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  ctx->profiling = enabled != 0;
  return SC_OK;
}

int sc_ctx_set_two_stage(sc_ctx* ctx, int mode) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (mode < -1 || mode > 1) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "mode must be -1, 0 or 1");
  ctx->two_stage = mode;
  return SC_OK;
}

int sc_last_eigh_timings(sc_ctx* ctx, double* out6) {
  if (!ctx || !out6) return SC_ERR_INVALID_ARG;
  for (int i = 0; i < 6; ++i) out6[i] = ctx->last_timings[i];
  return SC_OK;
}

int sc_last_eigh_phase_ms(sc_ctx* ctx, const char* name, double* ms) {
  if (!ctx || !name || !ms) return SC_ERR_INVALID_ARG;
  for (const auto& p : ctx->phases)
    if (p.first == name) { *ms = p.second; return SC_OK; }
  // a phase the last solve did not run is an answer, not a failure: the context's error string is left alone
  *ms = 0.0;
  return SC_ERR_INVALID_ARG;
}

int sc_ctx_get_counter(sc_ctx* ctx, const char* name, int64_t* value) {
  if (!ctx || !name || !value) return SC_ERR_INVALID_ARG;
  const std::string k(name);
  // (round 6: what the persistent kernels report is collected on the device while solves are enqueued; a diagnostic call
  // may wait for the stream)
  SC_HIP(ctx, hipSetDevice(ctx->device));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  SC_TRY(sc_collect_events(ctx));
  // (over the ticket slots the last chase drew from: one for the spread form, whose workgroups all count as XCD 0, or
  // the device's XCDs; the sum is the chase's grid)
  int tmin = ctx->chase_tickets[0], tmax = ctx->chase_tickets[0];
  long long tsum = 0;
  for (int x = 0; x < std::max(1, std::min(8, ctx->chase_ctl_xcds)); ++x) {
    tmin = std::min(tmin, ctx->chase_tickets[x]);
    tmax = std::max(tmax, ctx->chase_tickets[x]);
    tsum += ctx->chase_tickets[x];
  }
  if (k == "chase_launches") *value = ctx->cnt_chase_launches;
  else if (k == "chase_pair_launches") *value = ctx->cnt_pair_launches;
  else if (k == "chase_pair_fallbacks") *value = ctx->cnt_pair_fallbacks;
  else if (k == "xcd_count") *value = ctx->nxcd;
  else if (k == "gemm3_launches") *value = ctx->cnt_gemm3_launches;
  else if (k == "symm3_launches") *value = ctx->cnt_symm3_launches;
  else if (k == "resident_launches") *value = ctx->cnt_resident_launches;
  else if (k == "resident_takeovers") *value = ctx->cnt_resident_takeovers;
  else if (k == "resident_rollcall_failures") *value = ctx->cnt_resident_rollcalls;
  else if (k == "resident_lost_waits") *value = ctx->cnt_resident_lost;
  else if (k == "resident_lost_at") *value = ctx->resident_lost_at;
  else if (k == "panel_coop_launches") *value = ctx->cnt_coop_launches;
  else if (k == "panel_coop_timeouts") *value = ctx->cnt_coop_timeouts;
  else if (k == "chase_timeouts") *value = ctx->cnt_chase_timeouts;
  else if (k == "chase_incomplete") *value = ctx->cnt_chase_incomplete;
  else if (k == "chase_resumed") *value = ctx->cnt_chase_resumed;
  else if (k == "chase_sweeps") *value = ctx->cnt_chase_sweeps;
  else if (k == "stepwise_chases") *value = ctx->cnt_stepwise_chases;
  else if (k == "panel_wg1_launches") *value = ctx->cnt_panel_form[0];
  else if (k == "panel_wg2_launches") *value = ctx->cnt_panel_form[1];
  else if (k == "panel_wg3_launches") *value = ctx->cnt_panel_form[2];
  else if (k == "panel_wg4_launches") *value = ctx->cnt_panel_form[3];
  else if (k == "panel_wg10_launches") *value = ctx->cnt_panel_form[4];
  else if (k == "panel_wg12_launches") *value = ctx->cnt_panel_form[5];
  else if (k == "panel_blocked_launches") *value = ctx->cnt_panel_form[6];
  else if (k == "panel_unblocked_launches") *value = ctx->cnt_panel_form[7];
  else if (k == "panel_pair_first") *value = ctx->cnt_panel_role[0];
  else if (k == "panel_pair_second") *value = ctx->cnt_panel_role[1];
  else if (k == "symm_tri_launches") *value = ctx->cnt_symm_tri;
  else if (k == "symm_slices") *value = ctx->last_symm_slices;
  else if (k == "gemm3_declined") *value = ctx->cnt_gemm3_declined;
  else if (k == "stage1_parts") *value = ctx->last_stage1_parts;
  else if (k == "chase_stream_parts") *value = ctx->last_chase_stream_parts;
  else if (k == "bt2_wave_solves") *value = ctx->cnt_bt2_form[0];
  else if (k == "bt2_apply4_solves") *value = ctx->cnt_bt2_form[1];
  else if (k == "bt2_apply8_solves") *value = ctx->cnt_bt2_form[2];
  else if (k == "bt2_xcd_launches") *value = ctx->cnt_bt2_xcd;
  else if (k == "chase_xcd_min") *value = tmin;
  else if (k == "chase_xcd_max") *value = tmax;
  else if (k == "chase_xcd_total") *value = tsum;
  else if (k == "chase_wait_matrix") *value = ctx->chase_wait[0];
  else if (k == "chase_wait_sweep") *value = ctx->chase_wait[1];
  else if (k == "chase_wait_task") *value = ctx->chase_wait[2];
  else { *value = 0; return SC_ERR_INVALID_ARG; }
  return SC_OK;
}

// debugging entry point (include/springcraft_hip_debug.h)
int sc_dbg_set_chase(sc_ctx* ctx, int mode, int give_up_after) {
  if (!ctx || mode < -1 || mode > 5 || give_up_after < 0) return SC_ERR_INVALID_ARG;
  // 3 / 4 / 5: persistent always, in the pair form / with one sweep per workgroup, a matrix on one XCD / with one sweep per
  // workgroup and the workgroups of a matrix on all XCDs ("spread": fewer matrices than XCDs only); 2: always, the form by size
  ctx->chase_form = mode == 3 ? 1 : (mode == 4 ? 0 : (mode == 5 ? 2 : -1));
  if (mode > 2) mode = 2;
  ctx->chase_mode = mode;
  ctx->chase_give_up = give_up_after;
  if (mode >= 0) ctx->chase_ok = -1;
  return SC_OK;
}

int sc_dbg_set_panel_coop_fail(sc_ctx* ctx, int panel) {
  if (!ctx || panel < -1) return SC_ERR_INVALID_ARG;
  ctx->coop_fail_panel = panel;
  if (panel >= 0) ctx->coop_ok = -1;
  return SC_OK;
}

int sc_dbg_set_resident(sc_ctx* ctx, int mode, int hook, int workgroups) {
  if (!ctx || mode < -1 || mode > 1 || hook < 0 || workgroups < 0 || workgroups > 256) return SC_ERR_INVALID_ARG;
  ctx->resident_mode = mode;
  ctx->resident_hook = hook;
  ctx->resident_wgs = workgroups;
  if (mode != 0) { ctx->resident_ok = -1; ctx->resident_strikes = 0; }
  return SC_OK;
}

int sc_dbg_set_panel_coop(sc_ctx* ctx, int min_rows) {
  if (!ctx || min_rows < -1 || (min_rows > 0 && min_rows < 128)) return SC_ERR_INVALID_ARG;
  ctx->coop_min_rows = min_rows;
  if (min_rows != 0) ctx->coop_ok = -1;
  return SC_OK;
}

}  // extern "C"
