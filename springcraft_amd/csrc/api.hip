// C-ABI entry points of libspringcraft_hip.so (declared in include/springcraft_hip.h).
// Host-side plumbing only: argument validation, patch-table construction, transfers and
// kernel sequencing.  All arithmetic lives in assembly.hip / the eigensolver units.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstring>
#include <map>
#include <new>
#include <utility>

#include "common.h"
#include "host_logic.h"

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
  if (h[0] == 0 && h[1] == 0) return SC_OK;
  SC_HIP(ctx, hipMemset(ctx->d_status, 0, sizeof(h)));
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

namespace {

int ctx_create_impl(int device, void* stream, bool own, sc_ctx** out) {
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

int check_ff(sc_ctx* ctx, const sc_ff_desc* ff) {
  std::string err;
  const int rc = sc_host::check_ff(ff, err);
  return rc == SC_OK ? SC_OK : sc_set_error(ctx, rc, "%s", err.c_str());
}

struct Bump {  // carves sub-buffers out of ctx->scratch
  char* base;
  size_t off = 0;
  template <typename T>
  T* take(size_t count) {
    off = align_up(off, 256);
    T* p = reinterpret_cast<T*>(base + off);
    off += count * sizeof(T);
    return p;
  }
};

using sc_host::HostPatch;

int build_patch(sc_ctx* ctx, const sc_patch_desc* pd, int64_t n, HostPatch& hp) {
  std::string err;
  const int rc = sc_host::build_patch(pd, n, hp, err);
  return rc == SC_OK ? SC_OK : sc_set_error(ctx, rc, "%s", err.c_str());
}

int upload_patch(sc_ctx* ctx, const HostPatch& hp, Bump& bump, PatchDev& dev) {
  uint8_t* d_shut = bump.take<uint8_t>(hp.shut.size());
  int32_t* d_rp = bump.take<int32_t>(hp.row_ptr.size());
  int32_t* d_col = bump.take<int32_t>(hp.col.size() + 1);
  int8_t* d_flag = bump.take<int8_t>(hp.flag.size() + 1);
  double* d_gam = bump.take<double>(hp.gam.size() + 1);
  SC_HIP(ctx, hipMemcpyAsync(d_shut, hp.shut.data(), hp.shut.size(), hipMemcpyHostToDevice, ctx->stream));
  SC_HIP(ctx, hipMemcpyAsync(d_rp, hp.row_ptr.data(), hp.row_ptr.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  if (!hp.col.empty()) {
    SC_HIP(ctx, hipMemcpyAsync(d_col, hp.col.data(), hp.col.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(d_flag, hp.flag.data(), hp.flag.size(), hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(d_gam, hp.gam.data(), hp.gam.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  // the source vectors must outlive the async copies
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  dev = PatchDev{d_shut, d_rp, d_col, d_flag, d_gam, hp.mask_gamma};
  return SC_OK;
}

int check_coord_args(sc_ctx* ctx, const double* coord, int64_t n) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (n < 0 || n > 2000000) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad atom count %lld", (long long)n);
  if (n > 0 && !coord) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "coord is NULL");
  return SC_OK;
}

// Shared body of sc_kirchhoff_f64 / sc_hessian_f64 / sc_contacts / fused eigen entry points:
// stages coord (+ weights, patches) into scratch, returns device pointers.
struct Staged {
  double* d_coord = nullptr;
  double* d_w = nullptr;
  PatchDev patch{};
  bool has_patch = false;
  HostPatch hp;  // keeps host vectors alive until the stream is synchronised
  sc_tab_desc tab_dev{};   // SC_FF_TABULATED: same fields, DEVICE pointers
  sc_ff_desc ff_dev{};     // copy of the caller's descriptor with .tab -> &tab_dev
};

size_t tab_device_bytes(const sc_ff_desc* ff, int64_t n) {
  if (!ff || ff->kind != SC_FF_TABULATED || !ff->tab) return 0;
  const size_t nb = (size_t)ff->tab->n_bins;
  return align_up(nb * 8, 256) + align_up(3 * 400 * nb * 4, 256) + 2 * align_up((size_t)n * 4, 256) +
         align_up((size_t)n, 256) + 2048;
}

// Upload the tabulated force-field tables; st.ff_dev is what the kernel launchers must be given.
int stage_tab(sc_ctx* ctx, const sc_ff_desc* ff, int64_t n, Staged& st, Bump& bump) {
  st.ff_dev = *ff;
  if (ff->kind != SC_FF_TABULATED) return SC_OK;
  const sc_tab_desc* t = ff->tab;
  const size_t nb = (size_t)t->n_bins;
  for (int64_t i = 0; i < n; ++i)
    if (t->atom_type[i] < 0 || t->atom_type[i] >= 20)
      return sc_set_error(ctx, SC_ERR_INDEX, "amino-acid type %d of atom %lld out of range", t->atom_type[i],
                          (long long)i);
  double* d_edges = bump.take<double>(nb);
  float* d_tab = bump.take<float>(3 * 400 * nb);
  int32_t* d_type = bump.take<int32_t>((size_t)n);
  int32_t* d_chain = bump.take<int32_t>((size_t)n);
  uint8_t* d_bond = bump.take<uint8_t>((size_t)n);
  hipStream_t s = ctx->stream;
  if (t->edges_sq) SC_HIP(ctx, hipMemcpyAsync(d_edges, t->edges_sq, nb * 8, hipMemcpyHostToDevice, s));
  SC_HIP(ctx, hipMemcpyAsync(d_tab, t->bonded, 400 * nb * 4, hipMemcpyHostToDevice, s));
  SC_HIP(ctx, hipMemcpyAsync(d_tab + 400 * nb, t->intra_chain, 400 * nb * 4, hipMemcpyHostToDevice, s));
  SC_HIP(ctx, hipMemcpyAsync(d_tab + 800 * nb, t->inter_chain, 400 * nb * 4, hipMemcpyHostToDevice, s));
  SC_HIP(ctx, hipMemcpyAsync(d_type, t->atom_type, (size_t)n * 4, hipMemcpyHostToDevice, s));
  SC_HIP(ctx, hipMemcpyAsync(d_chain, t->chain, (size_t)n * 4, hipMemcpyHostToDevice, s));
  SC_HIP(ctx, hipMemcpyAsync(d_bond, t->bonded_next, (size_t)n, hipMemcpyHostToDevice, s));
  SC_HIP(ctx, hipStreamSynchronize(s));
  st.tab_dev = *t;
  st.tab_dev.edges_sq = d_edges;
  st.tab_dev.bonded = d_tab;
  st.tab_dev.intra_chain = d_tab + 400 * nb;
  st.tab_dev.inter_chain = d_tab + 800 * nb;
  st.tab_dev.atom_type = d_type;
  st.tab_dev.chain = d_chain;
  st.tab_dev.bonded_next = d_bond;
  st.ff_dev.tab = &st.tab_dev;
  return SC_OK;
}

int stage_inputs(sc_ctx* ctx, const double* coord, int64_t n, const sc_ff_desc* ff, const sc_patch_desc* pd,
                 const double* inv_sqrt_mass, size_t extra_bytes, Staged& st, Bump& bump) {
  SC_TRY(build_patch(ctx, pd, n, st.hp));
  size_t need = align_up((size_t)n * 24, 256) + align_up((size_t)n * 8, 256) + 1024 + extra_bytes +
                tab_device_bytes(ff, n);
  if (st.hp.any) need += st.hp.device_bytes();
  SC_TRY(sc_reserve_scratch(ctx, need));
  bump.base = (char*)ctx->scratch;
  bump.off = 0;
  st.d_coord = bump.take<double>((size_t)n * 3);
  SC_HIP(ctx, hipMemcpyAsync(st.d_coord, coord, (size_t)n * 24, hipMemcpyHostToDevice, ctx->stream));
  if (inv_sqrt_mass) {
    st.d_w = bump.take<double>((size_t)n);
    SC_HIP(ctx, hipMemcpyAsync(st.d_w, inv_sqrt_mass, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  if (st.hp.any) {
    SC_TRY(upload_patch(ctx, st.hp, bump, st.patch));
    st.has_patch = true;
  }
  SC_TRY(stage_tab(ctx, ff, n, st, bump));
  return SC_OK;
}

}  // namespace

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

int sc_contacts(sc_ctx* ctx, const double* coord, int64_t n, const sc_ff_desc* ff,
                const sc_patch_desc* patch, int64_t* counts, int64_t* n_pairs) {
  SC_TRY(check_coord_args(ctx, coord, n));
  SC_TRY(check_ff(ctx, ff));
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (n_pairs) *n_pairs = 0;
  if (n == 0) return SC_OK;
  Staged st;
  Bump bump{};
  SC_TRY(stage_inputs(ctx, coord, n, ff, patch, nullptr, (size_t)n * 8 + 256, st, bump));
  int64_t* d_counts = bump.take<int64_t>((size_t)n);
  SC_TRY(launch_contact_counts(ctx, st.d_coord, n, st.ff_dev, st.has_patch ? &st.patch : nullptr, d_counts));
  std::vector<int64_t> h((size_t)n);
  SC_HIP(ctx, hipMemcpyAsync(h.data(), d_counts, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  int64_t total = 0;
  for (int64_t i = 0; i < n; ++i) total += h[(size_t)i];
  if (counts) std::memcpy(counts, h.data(), (size_t)n * 8);
  if (n_pairs) *n_pairs = total;
  return SC_OK;
}

int sc_pairs(sc_ctx* ctx, const double* coord, int64_t n, const sc_ff_desc* ff,
             const sc_patch_desc* patch, int64_t capacity, int64_t* pairs, double* sq_dist,
             int64_t* n_pairs) {
  SC_TRY(check_coord_args(ctx, coord, n));
  SC_TRY(check_ff(ctx, ff));
  if (capacity < 0 || (capacity > 0 && !pairs))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs buffer is NULL");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (n_pairs) *n_pairs = 0;
  if (n == 0) return SC_OK;
  Staged st;
  Bump bump{};
  const size_t extra = (size_t)(2 * n + 2) * 8 + (size_t)capacity * 24 + 2048;
  SC_TRY(stage_inputs(ctx, coord, n, ff, patch, nullptr, extra, st, bump));
  int64_t* d_counts = bump.take<int64_t>((size_t)n);
  int64_t* d_off = bump.take<int64_t>((size_t)n + 1);
  int64_t* d_pairs = bump.take<int64_t>((size_t)capacity * 2 + 2);
  double* d_sq = sq_dist ? bump.take<double>((size_t)capacity + 1) : nullptr;
  const PatchDev* pdev = st.has_patch ? &st.patch : nullptr;
  SC_TRY(launch_contact_counts(ctx, st.d_coord, n, st.ff_dev, pdev, d_counts));
  // offsets of the rows in the ordered pair list: exclusive scan on the device, only the total comes back
  SC_TRY(launch_exclusive_scan_i64(ctx, d_counts, n, d_off));
  int64_t k = 0;
  SC_HIP(ctx, hipMemcpyAsync(&k, d_off + n, 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (n_pairs) *n_pairs = k;
  if (k > capacity)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pair buffer too small: %lld > %lld", (long long)k,
                        (long long)capacity);
  if (k == 0) return SC_OK;
  SC_TRY(launch_pair_fill(ctx, st.d_coord, n, st.ff_dev, pdev, d_off, d_pairs, d_sq));
  SC_HIP(ctx, hipMemcpyAsync(pairs, d_pairs, (size_t)k * 16, hipMemcpyDeviceToHost, ctx->stream));
  if (sq_dist)
    SC_HIP(ctx, hipMemcpyAsync(sq_dist, d_sq, (size_t)k * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

static int assemble_host(sc_ctx* ctx, const double* coord, int64_t n, const sc_ff_desc* ff,
                         const sc_patch_desc* patch, const double* inv_sqrt_mass, double* out,
                         int dim) {
  SC_TRY(check_coord_args(ctx, coord, n));
  SC_TRY(check_ff(ctx, ff));
  if (n > 0 && !out) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "output matrix is NULL");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (n == 0) return SC_OK;
  const size_t elems = (size_t)n * n * dim * dim;
  Staged st;
  Bump bump{};
  SC_TRY(stage_inputs(ctx, coord, n, ff, patch, inv_sqrt_mass, elems * 8 + 512, st, bump));
  double* d_m = bump.take<double>(elems);
  const PatchDev* pdev = st.has_patch ? &st.patch : nullptr;
  if (dim == 1)
    SC_TRY(launch_kirchhoff(ctx, st.d_coord, n, 1, st.ff_dev, pdev, st.d_w, d_m, nullptr));
  else
    SC_TRY(launch_hessian(ctx, st.d_coord, n, 1, st.ff_dev, pdev, st.d_w, d_m));
  SC_HIP(ctx, hipMemcpyAsync(out, d_m, elems * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

int sc_kirchhoff_f64(sc_ctx* ctx, const double* coord, int64_t n, const sc_ff_desc* ff,
                     const sc_patch_desc* patch, const double* inv_sqrt_mass, double* kirchhoff) {
  return assemble_host(ctx, coord, n, ff, patch, inv_sqrt_mass, kirchhoff, 1);
}

int sc_hessian_f64(sc_ctx* ctx, const double* coord, int64_t n, const sc_ff_desc* ff,
                   const sc_patch_desc* patch, const double* inv_sqrt_mass, double* hessian) {
  return assemble_host(ctx, coord, n, ff, patch, inv_sqrt_mass, hessian, 3);
}

static int check_pairs(sc_ctx* ctx, int64_t n, const int64_t* pairs, int64_t k, const double* gamma) {
  if (k < 0 || (k > 0 && (!pairs || !gamma)))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs / gamma is NULL");
  for (int64_t p = 0; p < 2 * k; ++p)
    if (pairs[p] < 0 || pairs[p] >= n)
      return sc_set_error(ctx, SC_ERR_INDEX, "pair index %lld out of range for %lld atoms",
                          (long long)pairs[p], (long long)n);
  return SC_OK;
}

int sc_kirchhoff_from_pairs_f64(sc_ctx* ctx, int64_t n, const int64_t* pairs, int64_t k,
                                const double* gamma, double* kirchhoff) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (n < 0 || (n > 0 && !kirchhoff)) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_TRY(check_pairs(ctx, n, pairs, k, gamma));
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (n == 0) return SC_OK;
  const size_t elems = (size_t)n * n;
  SC_TRY(sc_reserve_scratch(ctx, elems * 8 + (size_t)k * 24 + 4096));
  Bump bump{(char*)ctx->scratch};
  double* d_m = bump.take<double>(elems);
  int64_t* d_pairs = bump.take<int64_t>((size_t)k * 2 + 2);
  double* d_g = bump.take<double>((size_t)k + 1);
  if (k > 0) {
    SC_HIP(ctx, hipMemcpyAsync(d_pairs, pairs, (size_t)k * 16, hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(d_g, gamma, (size_t)k * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  SC_TRY(launch_kirchhoff_from_pairs(ctx, n, d_pairs, k, d_g, d_m));
  SC_HIP(ctx, hipMemcpyAsync(kirchhoff, d_m, elems * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

int sc_hessian_from_pairs_f64(sc_ctx* ctx, const double* coord, int64_t n, const int64_t* pairs,
                              int64_t k, const double* gamma, double* hessian) {
  SC_TRY(check_coord_args(ctx, coord, n));
  if (n > 0 && !hessian) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "output matrix is NULL");
  SC_TRY(check_pairs(ctx, n, pairs, k, gamma));
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (n == 0) return SC_OK;
  const size_t elems = (size_t)n * n * 9;
  SC_TRY(sc_reserve_scratch(ctx, elems * 8 + (size_t)k * 24 + (size_t)n * 24 + 4096));
  Bump bump{(char*)ctx->scratch};
  double* d_m = bump.take<double>(elems);
  double* d_coord = bump.take<double>((size_t)n * 3);
  int64_t* d_pairs = bump.take<int64_t>((size_t)k * 2 + 2);
  double* d_g = bump.take<double>((size_t)k + 1);
  SC_HIP(ctx, hipMemcpyAsync(d_coord, coord, (size_t)n * 24, hipMemcpyHostToDevice, ctx->stream));
  if (k > 0) {
    SC_HIP(ctx, hipMemcpyAsync(d_pairs, pairs, (size_t)k * 16, hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(d_g, gamma, (size_t)k * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  SC_TRY(launch_hessian_from_pairs(ctx, d_coord, n, d_pairs, k, d_g, d_m));
  SC_HIP(ctx, hipMemcpyAsync(hessian, d_m, elems * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

int sc_eigh_f64(sc_ctx* ctx, const double* a, int64_t n, double* w, double* v) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (n < 0 || (n > 0 && (!a || !w))) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (n == 0) return SC_OK;
  const size_t elems = (size_t)n * n;
  SC_TRY(sc_reserve_scratch(ctx, elems * 8 * (v ? 2 : 1) + (size_t)n * 8 + 4096));
  Bump bump{(char*)ctx->scratch};
  double* d_a = bump.take<double>(elems);
  double* d_w = bump.take<double>((size_t)n);
  double* d_v = v ? bump.take<double>(elems) : nullptr;
  SC_HIP(ctx, hipMemcpyAsync(d_a, a, elems * 8, hipMemcpyHostToDevice, ctx->stream));
  SC_TRY(eigh_batched(ctx, d_a, n, 1, d_w, d_v));
  SC_HIP(ctx, hipMemcpyAsync(w, d_w, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (v) SC_HIP(ctx, hipMemcpyAsync(v, d_v, elems * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

int sc_pinvh_f64(sc_ctx* ctx, const double* a, int64_t n, double rcond, double* out) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (n < 0 || (n > 0 && (!a || !out))) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (n == 0) return SC_OK;
  const size_t elems = (size_t)n * n;
  SC_TRY(sc_reserve_scratch(ctx, 2 * elems * 8 + 4096));
  Bump bump{(char*)ctx->scratch};
  double* d_a = bump.take<double>(elems);
  double* d_out = bump.take<double>(elems);
  SC_HIP(ctx, hipMemcpyAsync(d_a, a, elems * 8, hipMemcpyHostToDevice, ctx->stream));
  SC_TRY(pinvh_device(ctx, d_a, n, rcond, d_out));
  SC_HIP(ctx, hipMemcpyAsync(out, d_out, elems * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

int sc_eigh_range_f64(sc_ctx* ctx, const double* a, int64_t n, int64_t il, int64_t iu, double* w, double* v) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (n <= 0 || !a || !w || il < 0 || iu < il || iu >= n)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t m = iu - il + 1;
  const size_t elems = (size_t)n * n;
  SC_TRY(sc_reserve_scratch(ctx, elems * 8 + (size_t)m * 8 + (v ? (size_t)m * n * 8 : 0) + 4096));
  Bump bump{(char*)ctx->scratch};
  double* d_a = bump.take<double>(elems);
  double* d_w = bump.take<double>((size_t)m);
  double* d_v = v ? bump.take<double>((size_t)m * n) : nullptr;
  SC_HIP(ctx, hipMemcpyAsync(d_a, a, elems * 8, hipMemcpyHostToDevice, ctx->stream));
  SC_TRY(eigh_range_batched(ctx, d_a, n, 1, il, iu, d_w, d_v));
  SC_HIP(ctx, hipMemcpyAsync(w, d_w, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (v) SC_HIP(ctx, hipMemcpyAsync(v, d_v, (size_t)m * n * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

int sc_anm_eigen_range_f64(sc_ctx* ctx, const double* coord, int64_t n, const sc_ff_desc* ff,
                           const sc_patch_desc* patch, const double* inv_sqrt_mass, int64_t il, int64_t iu,
                           double* w, double* v) {
  SC_TRY(check_coord_args(ctx, coord, n));
  SC_TRY(check_ff(ctx, ff));
  const int64_t dim3n = 3 * n;
  if (n <= 0 || !w || il < 0 || iu < il || iu >= dim3n)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t m = iu - il + 1;
  const size_t elems = (size_t)dim3n * dim3n;
  Staged st;
  Bump bump{};
  SC_TRY(stage_inputs(ctx, coord, n, ff, patch, inv_sqrt_mass,
                      elems * 8 + (size_t)m * 8 + (v ? (size_t)m * dim3n * 8 : 0) + 4096, st, bump));
  double* d_m = bump.take<double>(elems);
  double* d_w = bump.take<double>((size_t)m);
  double* d_v = v ? bump.take<double>((size_t)m * dim3n) : nullptr;
  SC_TRY(launch_hessian(ctx, st.d_coord, n, 1, st.ff_dev, st.has_patch ? &st.patch : nullptr, st.d_w, d_m));
  SC_TRY(eigh_range_batched(ctx, d_m, dim3n, 1, il, iu, d_w, d_v));
  SC_HIP(ctx, hipMemcpyAsync(w, d_w, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (v) SC_HIP(ctx, hipMemcpyAsync(v, d_v, (size_t)m * dim3n * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

int sc_dev_eigh_range_f64(sc_ctx* ctx, double* d_a, int64_t n, int64_t batch, int64_t il, int64_t iu,
                          double* d_w, double* d_v) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (n <= 0 || batch <= 0 || !d_a || !d_w) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return eigh_range_batched_async(ctx, d_a, n, batch, il, iu, d_w, d_v);
}

// Results of a one-matrix window solve (device, in ctx->win_ws) -> page-locked host blocks of exactly (m,) and (m, n)
// that the caller owns (sc_host_free); m = 0: none, *w = *v = NULL.
static int window_results_to_host(sc_ctx* ctx, int64_t m, int64_t n, const double* d_w, const double* d_v, double** w,
                                  double** v) {
  if (m == 0) return SC_OK;
  void* hw = nullptr;
  void* hv = nullptr;
  int rc = sc_host_alloc((size_t)m * 8, &hw);
  if (rc == SC_OK && d_v) rc = sc_host_alloc((size_t)m * n * 8, &hv);
  if (rc == SC_OK && hipMemcpyAsync(hw, d_w, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = SC_ERR_HIP;
  if (rc == SC_OK && d_v && hipMemcpyAsync(hv, d_v, (size_t)m * n * 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
    rc = SC_ERR_HIP;
  if (rc == SC_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = SC_ERR_HIP;
  if (rc != SC_OK) {
    (void)hipGetLastError();
    (void)sc_host_free(hw);
    (void)sc_host_free(hv);
    return sc_set_error(ctx, rc, "cannot return the %lld eigenpairs of the window", (long long)m);
  }
  *w = (double*)hw;
  if (v) *v = (double*)hv;
  return SC_OK;
}

static int check_window_outputs(sc_ctx* ctx, int want_vectors, int64_t* m, double** w, double** v) {
  if (!m || !w || (want_vectors && !v)) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  *m = 0;
  *w = nullptr;
  if (v) *v = nullptr;
  return SC_OK;
}

int sc_eigh_window_f64(sc_ctx* ctx, const double* a, int64_t n, double vl, double vu, int want_vectors, int64_t* m,
                       double** w, double** v) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(check_window_outputs(ctx, want_vectors, m, w, v));
  if (n <= 0 || !a) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const size_t elems = (size_t)n * n;
  SC_TRY(sc_reserve_scratch(ctx, elems * 8 + 4096));
  Bump bump{(char*)ctx->scratch};
  double* d_a = bump.take<double>(elems);
  SC_HIP(ctx, hipMemcpyAsync(d_a, a, elems * 8, hipMemcpyHostToDevice, ctx->stream));
  int64_t mm = 0;
  double *d_w = nullptr, *d_v = nullptr;
  SC_TRY(eigh_window(ctx, d_a, n, vl, vu, want_vectors != 0, &mm, &d_w, &d_v));
  SC_TRY(window_results_to_host(ctx, mm, n, d_w, d_v, w, want_vectors ? v : nullptr));
  *m = mm;
  return SC_OK;
}

int sc_anm_eigen_window_f64(sc_ctx* ctx, const double* coord, int64_t n, const sc_ff_desc* ff,
                            const sc_patch_desc* patch, const double* inv_sqrt_mass, double vl, double vu,
                            int want_vectors, int64_t* m, double** w, double** v) {
  SC_TRY(check_coord_args(ctx, coord, n));
  SC_TRY(check_ff(ctx, ff));
  SC_TRY(check_window_outputs(ctx, want_vectors, m, w, v));
  if (n <= 0) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t dim3n = 3 * n;
  const size_t elems = (size_t)dim3n * dim3n;
  Staged st;
  Bump bump{};
  SC_TRY(stage_inputs(ctx, coord, n, ff, patch, inv_sqrt_mass, elems * 8 + 4096, st, bump));
  double* d_m = bump.take<double>(elems);
  SC_TRY(launch_hessian(ctx, st.d_coord, n, 1, st.ff_dev, st.has_patch ? &st.patch : nullptr, st.d_w, d_m));
  int64_t mm = 0;
  double *d_w = nullptr, *d_v = nullptr;
  SC_TRY(eigh_window(ctx, d_m, dim3n, vl, vu, want_vectors != 0, &mm, &d_w, &d_v));
  SC_TRY(window_results_to_host(ctx, mm, dim3n, d_w, d_v, w, want_vectors ? v : nullptr));
  *m = mm;
  return SC_OK;
}

int sc_dev_eigh_window_f64(sc_ctx* ctx, double* d_a, int64_t n, int64_t batch, double vl, double vu, int64_t capacity,
                           double* d_w, double* d_v, int64_t* d_count) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (n <= 0 || batch <= 0 || !d_a || !d_w || !d_count) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return eigh_window_batched_async(ctx, d_a, n, batch, vl, vu, capacity, d_w, d_v, d_count);
}

static int enm_eigen_host(sc_ctx* ctx, const double* coord, int64_t n, const sc_ff_desc* ff,
                          const sc_patch_desc* patch, const double* inv_sqrt_mass, double* w,
                          double* v, int dim) {
  SC_TRY(check_coord_args(ctx, coord, n));
  SC_TRY(check_ff(ctx, ff));
  if (n > 0 && !w) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "w is NULL");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (n == 0) return SC_OK;
  const int64_t m = n * dim;
  const size_t elems = (size_t)m * m;
  Staged st;
  Bump bump{};
  SC_TRY(stage_inputs(ctx, coord, n, ff, patch, inv_sqrt_mass,
                      elems * 8 * (v ? 2 : 1) + (size_t)m * 8 + 2048, st, bump));
  double* d_m = bump.take<double>(elems);
  double* d_w = bump.take<double>((size_t)m);
  double* d_v = v ? bump.take<double>(elems) : nullptr;
  const PatchDev* pdev = st.has_patch ? &st.patch : nullptr;
  if (dim == 1)
    SC_TRY(launch_kirchhoff(ctx, st.d_coord, n, 1, st.ff_dev, pdev, st.d_w, d_m, nullptr));
  else
    SC_TRY(launch_hessian(ctx, st.d_coord, n, 1, st.ff_dev, pdev, st.d_w, d_m));
  SC_TRY(eigh_batched(ctx, d_m, m, 1, d_w, d_v));
  SC_HIP(ctx, hipMemcpyAsync(w, d_w, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (v) SC_HIP(ctx, hipMemcpyAsync(v, d_v, elems * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

int sc_anm_eigen_f64(sc_ctx* ctx, const double* coord, int64_t n, const sc_ff_desc* ff,
                     const sc_patch_desc* patch, const double* inv_sqrt_mass, double* w, double* v) {
  return enm_eigen_host(ctx, coord, n, ff, patch, inv_sqrt_mass, w, v, 3);
}

int sc_gnm_eigen_f64(sc_ctx* ctx, const double* coord, int64_t n, const sc_ff_desc* ff,
                     const sc_patch_desc* patch, const double* inv_sqrt_mass, double* w, double* v) {
  return enm_eigen_host(ctx, coord, n, ff, patch, inv_sqrt_mass, w, v, 1);
}

int sc_dev_kirchhoff_f64(sc_ctx* ctx, const double* d_coord, int64_t n, int64_t batch,
                         const sc_ff_desc* ff, const double* d_inv_sqrt_mass, double* d_matrix) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(check_ff(ctx, ff));
  if (ff->kind == SC_FF_TABULATED)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "tabulated force fields are not supported on the batched device path");
  if (n < 0 || batch < 0 || (n > 0 && batch > 0 && (!d_coord || !d_matrix)))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_kirchhoff(ctx, d_coord, n, batch, *ff, nullptr, d_inv_sqrt_mass, d_matrix, nullptr);
}

int sc_dev_hessian_f64(sc_ctx* ctx, const double* d_coord, int64_t n, int64_t batch,
                       const sc_ff_desc* ff, const double* d_inv_sqrt_mass, double* d_matrix) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(check_ff(ctx, ff));
  if (ff->kind == SC_FF_TABULATED)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "tabulated force fields are not supported on the batched device path");
  if (n < 0 || batch < 0 || (n > 0 && batch > 0 && (!d_coord || !d_matrix)))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_hessian(ctx, d_coord, n, batch, *ff, nullptr, d_inv_sqrt_mass, d_matrix);
}

int sc_dev_eigh_f64(sc_ctx* ctx, double* d_a, int64_t n, int64_t batch, double* d_w, double* d_v) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (n < 0 || batch < 0 || (n > 0 && batch > 0 && (!d_a || !d_w)))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (n == 0 || batch == 0) return SC_OK;
  return eigh_batched_async(ctx, d_a, n, batch, d_w, d_v);
}

int sc_ctx_set_two_stage(sc_ctx* ctx, int mode) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (mode < -1 || mode > 1) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "mode must be -1, 0 or 1");
  ctx->two_stage = mode;
  return SC_OK;
}

int64_t sc_eigh_workspace_bytes(int64_t n, int64_t batch, int want_vectors) {
  if (n <= 0 || batch <= 0) return 0;
  return (int64_t)eigh_workspace_bytes(n, batch, want_vectors != 0);
}

// ---- ragged / decorated batches ---------------------------------------------------------------------------------
}  // extern "C"

// Everything a batch of structures needs on the device besides coordinates: per-structure records (size, slot order,
// force-field descriptor with device table pointers, patch override tables), uploaded once at plan creation.
struct sc_batch_plan {
  sc_ctx* ctx = nullptr;
  int dim = 3;
  int64_t count = 0, order = 0;
  int max_atoms = 0;
  bool any_patch = false, any_pad = false;
  char* d_blob = nullptr;
  size_t off_items = 0, off_bound = 0, off_ragged = 0;
  std::vector<int64_t> atom_off;   // count + 1: first atom of every structure in the packed buffers
  int64_t total_sq = 0;            // sum of n_atoms^2: elements of a packed dcc
  int min_atoms = 0;
};

namespace {

// Host image of the plan's device blob: take() reserves an aligned region and returns its offset.
struct Blob {
  std::vector<char> bytes;
  size_t take(size_t n) {
    const size_t off = align_up(bytes.size(), 256);
    bytes.resize(off + n, 0);
    return off;
  }
  template <typename T>
  size_t put(const T* src, size_t count) {
    const size_t off = take(count * sizeof(T) + 16);   // (+16: the kernels may read one element past empty tables)
    if (count) memcpy(bytes.data() + off, src, count * sizeof(T));
    return off;
  }
};

// ---- mode consumers of a batch (batch_consumers.hip, dist_fluct.hip, mode_overlap.hip, mode_response.hip) -------------
// Whose modes a consumer works on: the (batch, nvec, m) results of a uniform batch (sc_dev_modes_*: m = dim * n_atoms) or
// of a plan's padded slots (sc_batch_plan_modes_*).  Each consumer has ONE body, modes_* below, which runs every check and
// calls the launcher; its two entries only build this description.
struct ModesOf {
  sc_ctx* ctx = nullptr;
  int64_t m = 0, nvec = 0, batch = 0;
  int dim = 0;
  RaggedView view{};       // a plan's records: m is then the slot order (dim need not divide it) and d_out is packed
  int64_t first_row = 0;   // a plan's global mode index of row 0 of (w, v), as the caller gave it: checked after the rest
  const RaggedView* ragged() const { return view.d_rec ? &view : nullptr; }
};

const RaggedRec* plan_records(const sc_batch_plan* plan) {
  return reinterpret_cast<const RaggedRec*>(plan->d_blob + plan->off_ragged);
}

// (a NULL plan gives the empty description, which every body answers as it answers a NULL ctx)
ModesOf plan_modes_of(const sc_batch_plan* plan, int64_t nvec, int64_t first_row) {
  if (!plan) return ModesOf{};
  const RaggedView rv{plan_records(plan), (int)first_row, plan->max_atoms, plan->atom_off.back(), plan->total_sq};
  return ModesOf{plan->ctx, plan->order, nvec, plan->count, plan->dim, rv, first_row};
}

// The (m, nvec, batch, dim) checks of every consumer; `pointers`: the consumer's required pointers are all there
int check_modes_shape(const ModesOf& who, bool pointers) {
  sc_ctx* ctx = who.ctx;
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (who.m <= 0 || who.nvec <= 0 || who.batch <= 0 || !pointers) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  if ((who.dim != 1 && who.dim != 3) || (!who.ragged() && who.m % who.dim != 0))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "dim must be 1 or 3 and divide m = %lld", (long long)who.m);
  if (who.m > INT32_MAX || who.nvec > who.m || who.batch > INT32_MAX || (size_t)who.batch * who.nvec > (size_t)INT32_MAX)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "(batch, nvec, m) = (%lld, %lld, %lld) is not a solver's result shape",
                        (long long)who.batch, (long long)who.nvec, (long long)who.m);
  return SC_OK;
}

int check_first_row(const ModesOf& who) {
  if (!who.ragged() || (who.first_row >= 0 && who.first_row < who.m)) return SC_OK;
  return sc_set_error(who.ctx, SC_ERR_INDEX, "first row %lld outside 0..%lld", (long long)who.first_row, (long long)who.m - 1);
}

int check_modes_args(const ModesOf& who, const double* d_w, const double* d_v, const sc_mode_selection* sel,
                     const double* d_out) {
  SC_TRY(check_modes_shape(who, d_w && d_v && sel && d_out));
  switch (sel->kind) {
    case SC_SEL_FROM_ROW:
      if (sel->row0 < 0 || sel->row0 > who.nvec)
        return sc_set_error(who.ctx, SC_ERR_INDEX, "row0 %lld outside 0..%lld", (long long)sel->row0, (long long)who.nvec);
      break;
    case SC_SEL_ROWS:
      if (sel->n_rows < 0 || sel->n_rows > INT32_MAX / 4 || (sel->n_rows > 0 && !sel->d_rows))
        return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "bad row list");
      break;
    case SC_SEL_PINV:
      if (!(sel->rcond >= 0.0)) return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "rcond must be >= 0");
      break;
    default:
      return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "unknown selection kind %d", (int)sel->kind);
  }
  return check_first_row(who);
}

int modes_msf(const ModesOf& who, const double* d_w, const double* d_v, const sc_mode_selection* sel,
              const int64_t* d_counts, double* d_out) {
  SC_TRY(check_modes_args(who, d_w, d_v, sel, d_out));
  SC_HIP(who.ctx, hipSetDevice(who.ctx->device));
  return batch_msf_device(who.ctx, d_w, d_v, who.m, who.nvec, who.batch, who.dim, *sel, d_counts, 0, d_out, who.ragged());
}

int modes_dcc(const ModesOf& who, const double* d_w, const double* d_v, const sc_mode_selection* sel,
              const int64_t* d_counts, int norm, int64_t budget_bytes, double* d_out) {
  SC_TRY(check_modes_args(who, d_w, d_v, sel, d_out));
  if (budget_bytes < 0) return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "budget_bytes must be >= 0");
  SC_HIP(who.ctx, hipSetDevice(who.ctx->device));
  return batch_dcc_device(who.ctx, d_w, d_v, who.m, who.nvec, who.batch, who.dim, *sel, d_counts, norm,
                          (size_t)budget_bytes, d_out, who.ragged());
}

// (aniso, distfluct: the sc_dev entries have no dim argument and describe dim 3, so only a plan can fail the dim check)
int modes_aniso(const ModesOf& who, const double* d_w, const double* d_v, const sc_mode_selection* sel,
                const int64_t* d_counts, double* d_out) {
  SC_TRY(check_modes_args(who, d_w, d_v, sel, d_out));
  if (who.dim != 3)
    return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "anisotropic fluctuation tensors need an ANM plan (dim 3)");
  SC_HIP(who.ctx, hipSetDevice(who.ctx->device));
  return batch_aniso_device(who.ctx, d_w, d_v, who.m, who.nvec, who.batch, *sel, d_counts, 0, d_out, who.ragged());
}

int modes_distfluct(const ModesOf& who, const double* d_w, const double* d_v, const sc_mode_selection* sel,
                    const int64_t* d_counts, const double* d_coord, const double* d_atom_scale, double* d_out) {
  SC_TRY(check_modes_args(who, d_w, d_v, sel, d_out));
  if (who.dim != 3) return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "distance fluctuations need an ANM plan (dim 3)");
  if (!d_coord) return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "distance fluctuations need the coordinates");
  SC_HIP(who.ctx, hipSetDevice(who.ctx->device));
  return batch_distfluct_device(who.ctx, d_w, d_v, who.m, who.nvec, who.batch, *sel, d_counts, d_coord, d_atom_scale,
                                d_out, who.ragged());
}

int modes_overlap(const ModesOf& who, const double* d_v, const double* d_disp, int64_t q, const int64_t* d_counts,
                  double* d_overlap, double* d_collectivity) {
  SC_TRY(check_modes_shape(who, d_v != nullptr));
  sc_ctx* ctx = who.ctx;
  if (q < 0 || q > INT32_MAX / 4) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "q = %lld displacement vectors", (long long)q);
  if (!d_overlap && !d_collectivity) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "both outputs are NULL");
  if ((q > 0 && (!d_disp || !d_overlap)) || (q == 0 && !d_collectivity))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "q = %lld needs %s", (long long)q,
                        q > 0 ? "d_disp and d_overlap" : "d_collectivity");
  SC_TRY(check_first_row(who));
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return modes_overlap_device(ctx, d_v, who.m, who.nvec, who.batch, who.dim, nullptr, who.nvec, d_disp, q, d_counts,
                              d_overlap, d_collectivity, who.ragged());
}

// (response: dim 1 is a GNM's, for which the reference defines no linear response; the Python layer refuses it, the
// arithmetic here is the same for both)
int modes_response(const ModesOf& who, const double* d_w, const double* d_v, const sc_mode_selection* sel,
                   const int64_t* d_counts, const double* d_force, int64_t q, const double* d_atom_scale, double* d_out) {
  SC_TRY(check_modes_args(who, d_w, d_v, sel, d_out));
  if (q < 0 || q > INT32_MAX / 4 || (q > 0 && !d_force))
    return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "q = %lld force vectors", (long long)q);
  SC_HIP(who.ctx, hipSetDevice(who.ctx->device));
  return modes_response_device(who.ctx, d_w, d_v, who.m, who.nvec, who.batch, who.dim, *sel, d_counts, d_force, q,
                               d_atom_scale, 0, d_out, who.ragged());
}

int modes_combine(const ModesOf& who, const double* d_v, const double* d_coef, int64_t q, const int64_t* d_counts,
                  const double* d_atom_scale, double* d_out) {
  SC_TRY(check_modes_shape(who, d_v && d_out));
  if (q < 0 || q > INT32_MAX / 4 || (q > 0 && !d_coef))
    return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "q = %lld coefficient vectors", (long long)q);
  SC_TRY(check_first_row(who));
  SC_HIP(who.ctx, hipSetDevice(who.ctx->device));
  return modes_combine_device(who.ctx, d_v, who.m, who.nvec, who.batch, who.dim, nullptr, who.nvec, d_coef, q, d_counts,
                              d_atom_scale, 0, d_out, who.ragged());
}

int64_t modes_workspace_bytes(const ModesOf& who, int64_t n_sel, int what, int64_t budget_bytes) {
  if (who.m <= 0 || who.nvec <= 0 || who.batch <= 0 || n_sel < 0 || (who.dim != 1 && who.dim != 3) || budget_bytes < 0)
    return 0;
  if (what == 3) return 0;   // overlaps and collectivities hold no workspace
  if ((what == 2 || what == 4) && (who.dim != 3 || (!who.ragged() && who.m % 3 != 0))) return 0;
  return (int64_t)batch_modes_workspace_bytes(who.m, who.nvec, who.batch, who.dim, n_sel, what, (size_t)budget_bytes,
                                              who.ragged());
}

}  // namespace

extern "C" {

int sc_batch_plan_create(sc_ctx* ctx, int dim, const sc_structure_desc* structures, int64_t count, int64_t order,
                         sc_batch_plan** out) {
  if (!ctx || !out) return SC_ERR_INVALID_ARG;
  *out = nullptr;
  if ((dim != 1 && dim != 3) || count <= 0 || !structures)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments (dim %d, %lld structures)", dim, (long long)count);
  int64_t max_atoms = 0;
  for (int64_t b = 0; b < count; ++b) {
    if (structures[b].n_atoms <= 0 || structures[b].n_atoms > 2000000)
      return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad atom count %lld of structure %lld",
                          (long long)structures[b].n_atoms, (long long)b);
    SC_TRY(check_ff(ctx, structures[b].ff));
    max_atoms = std::max(max_atoms, structures[b].n_atoms);
  }
  if (order == 0) order = dim * max_atoms;
  if (order < dim * max_atoms || order > 46000)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "slot order %lld does not hold %d x %lld rows (or exceeds 46000)",
                        (long long)order, dim, (long long)max_atoms);
  SC_HIP(ctx, hipSetDevice(ctx->device));

  Blob blob;
  const size_t isz = asm_item_bytes();
  const size_t off_items = blob.take(isz * (size_t)count);
  const size_t off_bound = blob.take(8 * (size_t)count);
  const size_t off_zero = blob.take(4 * ((size_t)max_atoms + 2));   // empty patch tables: shut = 0, row_ptr = 0
  // own order and packed output offsets of every structure, for the window count and the consumers
  const size_t off_ragged = blob.take(sizeof(RaggedRec) * (size_t)count);
  int64_t total_sq = 0, min_atoms = max_atoms;
  {
    int64_t atoms = 0;
    for (int64_t b = 0; b < count; ++b) {
      const int64_t n = structures[b].n_atoms;
      const RaggedRec r{(int)(dim * n), (int)n, (long long)atoms, (long long)total_sq};
      memcpy(blob.bytes.data() + off_ragged + sizeof(RaggedRec) * (size_t)b, &r, sizeof(r));
      atoms += n;
      total_sq += n * n;
      min_atoms = std::min(min_atoms, n);
    }
  }
  struct Rec {
    sc_ff_desc ff; sc_tab_desc tab; bool has_tab = false;
    size_t o_edges = 0, o_tables = 0, o_type = 0, o_chain = 0, o_bond = 0;
    bool has_patch = false; int mask_gamma = 0;
    size_t o_shut = 0, o_rp = 0, o_col = 0, o_flag = 0, o_gam = 0;
  };
  std::vector<Rec> recs((size_t)count);
  // parameter tables are shared by every structure that points at the same host arrays
  std::map<std::pair<const void*, int>, std::pair<size_t, size_t>> tables;   // (bonded ptr, bins) -> (edges, tables)
  bool any_patch = false, any_pad = false;
  for (int64_t b = 0; b < count; ++b) {
    const sc_structure_desc& sd = structures[b];
    Rec& r = recs[(size_t)b];
    const size_t n = (size_t)sd.n_atoms;
    r.ff = *sd.ff;
    if (dim * sd.n_atoms < order) any_pad = true;
    if (sd.ff->kind == SC_FF_TABULATED) {
      const sc_tab_desc* t = sd.ff->tab;
      const size_t nb = (size_t)t->n_bins;
      for (size_t i = 0; i < n; ++i)
        if (t->atom_type[i] < 0 || t->atom_type[i] >= 20)
          return sc_set_error(ctx, SC_ERR_INDEX, "amino-acid type %d of atom %lld of structure %lld out of range",
                              t->atom_type[i], (long long)i, (long long)b);
      r.has_tab = true;
      r.tab = *t;
      const auto key = std::make_pair((const void*)t->bonded, t->n_bins);
      auto it = tables.find(key);
      if (it == tables.end()) {
        const size_t oe = blob.take(nb * 8 + 16);
        if (t->edges_sq) memcpy(blob.bytes.data() + oe, t->edges_sq, nb * 8);
        const size_t ot = blob.take(3 * 400 * nb * 4);
        memcpy(blob.bytes.data() + ot, t->bonded, 400 * nb * 4);
        memcpy(blob.bytes.data() + ot + 400 * nb * 4, t->intra_chain, 400 * nb * 4);
        memcpy(blob.bytes.data() + ot + 800 * nb * 4, t->inter_chain, 400 * nb * 4);
        it = tables.emplace(key, std::make_pair(oe, ot)).first;
      }
      r.o_edges = it->second.first;
      r.o_tables = it->second.second;
      r.o_type = blob.put(t->atom_type, n);
      r.o_chain = blob.put(t->chain, n);
      r.o_bond = blob.put(t->bonded_next, n);
    }
    HostPatch hp;
    SC_TRY(build_patch(ctx, sd.patch, sd.n_atoms, hp));
    if (hp.any) {
      any_patch = true;
      r.has_patch = true;
      r.mask_gamma = hp.mask_gamma;
      r.o_shut = blob.put(hp.shut.data(), hp.shut.size());
      r.o_rp = blob.put(hp.row_ptr.data(), hp.row_ptr.size());
      r.o_col = blob.put(hp.col.data(), hp.col.size());
      r.o_flag = blob.put(hp.flag.data(), hp.flag.size());
      r.o_gam = blob.put(hp.gam.data(), hp.gam.size());
    }
  }
  char* d_blob = nullptr;
  SC_HIP(ctx, hipMalloc((void**)&d_blob, align_up(blob.bytes.size(), 256)));
  // the item records hold device addresses: fill them now that the blob's base is known
  long long atom_off = 0;
  for (int64_t b = 0; b < count; ++b) {
    Rec& r = recs[(size_t)b];
    const size_t nb = r.has_tab ? (size_t)r.tab.n_bins : 0;
    sc_ff_desc ffd = r.ff;
    sc_tab_desc td{};
    if (r.has_tab) {
      td = r.tab;
      td.edges_sq = reinterpret_cast<const double*>(d_blob + r.o_edges);
      td.bonded = reinterpret_cast<const float*>(d_blob + r.o_tables);
      td.intra_chain = td.bonded + 400 * nb;
      td.inter_chain = td.bonded + 800 * nb;
      td.atom_type = reinterpret_cast<const int32_t*>(d_blob + r.o_type);
      td.chain = reinterpret_cast<const int32_t*>(d_blob + r.o_chain);
      td.bonded_next = reinterpret_cast<const uint8_t*>(d_blob + r.o_bond);
      ffd.tab = &td;
    }
    PatchDev pdv{};
    if (r.has_patch) {
      pdv = PatchDev{reinterpret_cast<const uint8_t*>(d_blob + r.o_shut), reinterpret_cast<const int32_t*>(d_blob + r.o_rp),
                     reinterpret_cast<const int32_t*>(d_blob + r.o_col), reinterpret_cast<const int8_t*>(d_blob + r.o_flag),
                     reinterpret_cast<const double*>(d_blob + r.o_gam), r.mask_gamma};
    } else {
      pdv = PatchDev{reinterpret_cast<const uint8_t*>(d_blob + off_zero), reinterpret_cast<const int32_t*>(d_blob + off_zero),
                     reinterpret_cast<const int32_t*>(d_blob + off_zero), reinterpret_cast<const int8_t*>(d_blob + off_zero),
                     reinterpret_cast<const double*>(d_blob + off_zero), 0};
    }
    asm_item_fill(blob.bytes.data() + off_items + isz * (size_t)b, atom_off, (int)structures[b].n_atoms, (int)order, ffd, pdv);
    atom_off += structures[b].n_atoms;
  }
  if (hipMemcpy(d_blob, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d_blob);
    return sc_set_error(ctx, SC_ERR_HIP, "upload of the batch plan failed");
  }
  sc_batch_plan* plan = new (std::nothrow) sc_batch_plan();
  if (!plan) { (void)hipFree(d_blob); return SC_ERR_NOMEM; }
  plan->ctx = ctx; plan->dim = dim; plan->count = count; plan->order = order; plan->max_atoms = (int)max_atoms;
  plan->any_patch = any_patch; plan->any_pad = any_pad;
  plan->d_blob = d_blob; plan->off_items = off_items; plan->off_bound = off_bound; plan->off_ragged = off_ragged;
  plan->total_sq = total_sq; plan->min_atoms = (int)min_atoms;
  plan->atom_off.assign((size_t)count + 1, 0);
  for (int64_t b = 0; b < count; ++b) plan->atom_off[(size_t)b + 1] = plan->atom_off[(size_t)b] + structures[b].n_atoms;
  *out = plan;
  return SC_OK;
}

int sc_batch_plan_assemble_f64(sc_batch_plan* plan, const double* d_coord, const double* d_inv_sqrt_mass,
                               double* d_matrix) {
  if (!plan) return SC_ERR_INVALID_ARG;
  sc_ctx* ctx = plan->ctx;
  if (!d_coord || !d_matrix) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_assemble_items(ctx, plan->dim, plan->d_blob + plan->off_items, plan->count, plan->max_atoms,
                               plan->any_patch, plan->any_pad, d_coord, d_inv_sqrt_mass, d_matrix,
                               reinterpret_cast<unsigned long long*>(plan->d_blob + plan->off_bound));
}

// Contact scan of every structure: counts per atom + their exclusive scan in the context's scratch; the per-structure
// offsets of the pair list (count + 1) come back to `pair_off`.  Leaves d_off (atoms + 1 entries) valid in scratch.
static int plan_scan(sc_batch_plan* plan, const double* d_coord, size_t extra_bytes, Bump& bump, int64_t** d_off_out,
                     std::vector<int64_t>& pair_off) {
  sc_ctx* ctx = plan->ctx;
  const int64_t atoms = plan->atom_off.back();
  SC_TRY(sc_reserve_scratch(ctx, (size_t)(2 * atoms + 2) * 8 + extra_bytes + 4096));
  bump = Bump{(char*)ctx->scratch};
  int64_t* d_counts = bump.take<int64_t>((size_t)atoms);
  int64_t* d_off = bump.take<int64_t>((size_t)atoms + 1);
  SC_TRY(launch_items_counts(ctx, plan->d_blob + plan->off_items, plan->count, plan->max_atoms, plan->any_patch, d_coord,
                             d_counts));
  SC_TRY(launch_exclusive_scan_i64(ctx, d_counts, atoms, d_off));
  std::vector<int64_t> off((size_t)atoms + 1);
  SC_HIP(ctx, hipMemcpyAsync(off.data(), d_off, ((size_t)atoms + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  pair_off.resize((size_t)plan->count + 1);
  for (int64_t b = 0; b <= plan->count; ++b) pair_off[(size_t)b] = off[(size_t)plan->atom_off[(size_t)b]];
  *d_off_out = d_off;
  return SC_OK;
}

int sc_batch_plan_contacts(sc_batch_plan* plan, const double* d_coord, int64_t* n_pairs) {
  if (!plan) return SC_ERR_INVALID_ARG;
  sc_ctx* ctx = plan->ctx;
  if (!d_coord || !n_pairs) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  Bump bump{};
  int64_t* d_off = nullptr;
  std::vector<int64_t> pair_off;
  SC_TRY(plan_scan(plan, d_coord, 0, bump, &d_off, pair_off));
  for (int64_t b = 0; b < plan->count; ++b) n_pairs[b] = pair_off[(size_t)b + 1] - pair_off[(size_t)b];
  return SC_OK;
}

int sc_batch_plan_pairs(sc_batch_plan* plan, const double* d_coord, int64_t capacity, int64_t* pairs, double* sq_dist,
                        int64_t* pair_off) {
  if (!plan) return SC_ERR_INVALID_ARG;
  sc_ctx* ctx = plan->ctx;
  if (!d_coord || !pair_off || capacity < 0 || (capacity > 0 && !pairs))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  Bump bump{};
  int64_t* d_off = nullptr;
  std::vector<int64_t> off;
  SC_TRY(plan_scan(plan, d_coord, (size_t)capacity * 24 + 1024, bump, &d_off, off));
  for (int64_t b = 0; b <= plan->count; ++b) pair_off[b] = off[(size_t)b];
  const int64_t k = off.back();
  if (k > capacity)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pair buffer too small: %lld > %lld", (long long)k, (long long)capacity);
  if (k == 0) return SC_OK;
  int64_t* d_pairs = bump.take<int64_t>((size_t)capacity * 2 + 2);
  double* d_sq = sq_dist ? bump.take<double>((size_t)capacity + 1) : nullptr;
  SC_TRY(launch_items_pair_fill(ctx, plan->d_blob + plan->off_items, plan->count, plan->max_atoms, plan->any_patch, d_coord,
                                d_off, d_pairs, d_sq));
  SC_HIP(ctx, hipMemcpyAsync(pairs, d_pairs, (size_t)k * 16, hipMemcpyDeviceToHost, ctx->stream));
  if (sq_dist) SC_HIP(ctx, hipMemcpyAsync(sq_dist, d_sq, (size_t)k * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

int sc_batch_plan_fill_from_pairs_f64(sc_batch_plan* plan, const double* d_coord, const int64_t* pairs,
                                      const int64_t* pair_off, const double* gamma, const double* d_inv_sqrt_mass,
                                      double* d_matrix) {
  if (!plan) return SC_ERR_INVALID_ARG;
  sc_ctx* ctx = plan->ctx;
  if (!d_coord || !pair_off || !d_matrix) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  if (pair_off[0] != 0) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pair_off[0] must be 0");
  for (int64_t b = 0; b < plan->count; ++b) {
    if (pair_off[b + 1] < pair_off[b]) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pair_off must not decrease");
    const int64_t nb = plan->atom_off[(size_t)b + 1] - plan->atom_off[(size_t)b];
    if (pair_off[b + 1] > pair_off[b] && (!pairs || !gamma))
      return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs / gamma is NULL");
    for (int64_t p = 2 * pair_off[b]; p < 2 * pair_off[b + 1]; ++p)
      if (pairs[p] < 0 || pairs[p] >= nb)
        return sc_set_error(ctx, SC_ERR_INDEX, "pair index %lld out of range for the %lld atoms of structure %lld",
                            (long long)pairs[p], (long long)nb, (long long)b);
  }
  const int64_t k = pair_off[plan->count];
  SC_HIP(ctx, hipSetDevice(ctx->device));
  SC_TRY(sc_reserve_scratch(ctx, (size_t)k * 24 + ((size_t)plan->count + 1) * 8 + 4096));
  Bump bump{(char*)ctx->scratch};
  int64_t* d_poff = bump.take<int64_t>((size_t)plan->count + 1);
  int64_t* d_pairs = bump.take<int64_t>((size_t)k * 2 + 2);
  double* d_g = bump.take<double>((size_t)k + 1);
  // (pageable host memory: the copies are staged by the runtime before the call returns)
  SC_HIP(ctx, hipMemcpyAsync(d_poff, pair_off, ((size_t)plan->count + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  if (k > 0) {
    SC_HIP(ctx, hipMemcpyAsync(d_pairs, pairs, (size_t)k * 16, hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(d_g, gamma, (size_t)k * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  SC_TRY(launch_items_from_pairs(ctx, plan->dim, plan->d_blob + plan->off_items, plan->count, plan->max_atoms, plan->order,
                                 plan->any_pad, d_coord, d_poff, k, d_pairs, d_g, d_inv_sqrt_mass, d_matrix,
                                 reinterpret_cast<unsigned long long*>(plan->d_blob + plan->off_bound)));
  // the scratch arena is reused by the next call: the kernels that read it must have run
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

int64_t sc_batch_plan_order(const sc_batch_plan* plan) { return plan ? plan->order : 0; }

// ---- partial spectrum of a plan's padded slots -----------------------------------------------------------------------------
int sc_batch_plan_eigh_range_f64(sc_batch_plan* plan, double* d_a, int64_t il, int64_t iu, double* d_w, double* d_v) {
  if (!plan) return SC_ERR_INVALID_ARG;
  sc_ctx* ctx = plan->ctx;
  if (!d_a || !d_w) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  const int64_t own_min = (int64_t)plan->dim * plan->min_atoms;
  if (il < 0 || iu < il || iu >= own_min)
    return sc_set_error(ctx, SC_ERR_INDEX, "eigenvalue index range [%lld, %lld] outside the %lld modes of the smallest "
                        "structure", (long long)il, (long long)iu, (long long)own_min);
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return eigh_range_batched_async(ctx, d_a, plan->order, plan->count, il, iu, d_w, d_v);
}

int sc_batch_plan_eigh_window_f64(sc_batch_plan* plan, double* d_a, double vl, double vu, int64_t capacity, double* d_w,
                                  double* d_v, int64_t* d_count) {
  if (!plan) return SC_ERR_INVALID_ARG;
  sc_ctx* ctx = plan->ctx;
  if (!d_a || !d_w || !d_count) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  const int64_t own_min = (int64_t)plan->dim * plan->min_atoms;
  if (capacity < 1 || capacity > own_min)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "window capacity %lld outside 1..%lld, the modes of the smallest structure",
                        (long long)capacity, (long long)own_min);
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return eigh_window_batched_async(ctx, d_a, plan->order, plan->count, vl, vu, capacity, d_w, d_v, d_count,
                                   plan_records(plan));
}

// ---- mode consumers of a uniform batch and of a plan's slots (first_row in sel->reserved): the bodies are modes_* above --
int sc_dev_modes_msf_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                         int dim, const sc_mode_selection* sel, const int64_t* d_counts, double* d_out) {
  return modes_msf(ModesOf{ctx, m, nvec, batch, dim}, d_w, d_v, sel, d_counts, d_out);
}
int sc_batch_plan_modes_msf_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                                const sc_mode_selection* sel, const int64_t* d_counts, double* d_out) {
  return modes_msf(plan_modes_of(plan, nvec, sel ? sel->reserved : 0), d_w, d_v, sel, d_counts, d_out);
}

int sc_dev_modes_dcc_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                         int dim, const sc_mode_selection* sel, const int64_t* d_counts, int norm, int64_t budget_bytes,
                         double* d_out) {
  return modes_dcc(ModesOf{ctx, m, nvec, batch, dim}, d_w, d_v, sel, d_counts, norm, budget_bytes, d_out);
}
int sc_batch_plan_modes_dcc_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                                const sc_mode_selection* sel, const int64_t* d_counts, int norm, int64_t budget_bytes,
                                double* d_out) {
  return modes_dcc(plan_modes_of(plan, nvec, sel ? sel->reserved : 0), d_w, d_v, sel, d_counts, norm, budget_bytes, d_out);
}

int sc_dev_modes_aniso_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                           const sc_mode_selection* sel, const int64_t* d_counts, double* d_out) {
  return modes_aniso(ModesOf{ctx, m, nvec, batch, 3}, d_w, d_v, sel, d_counts, d_out);
}
int sc_batch_plan_modes_aniso_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                                  const sc_mode_selection* sel, const int64_t* d_counts, double* d_out) {
  return modes_aniso(plan_modes_of(plan, nvec, sel ? sel->reserved : 0), d_w, d_v, sel, d_counts, d_out);
}

int sc_dev_modes_distfluct_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                               const sc_mode_selection* sel, const int64_t* d_counts, const double* d_coord,
                               const double* d_atom_scale, double* d_out) {
  return modes_distfluct(ModesOf{ctx, m, nvec, batch, 3}, d_w, d_v, sel, d_counts, d_coord, d_atom_scale, d_out);
}
int sc_batch_plan_modes_distfluct_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                                      const sc_mode_selection* sel, const int64_t* d_counts, const double* d_coord,
                                      const double* d_atom_scale, double* d_out) {
  return modes_distfluct(plan_modes_of(plan, nvec, sel ? sel->reserved : 0), d_w, d_v, sel, d_counts, d_coord,
                         d_atom_scale, d_out);
}

int sc_dev_modes_overlap_f64(sc_ctx* ctx, const double* d_v, int64_t m, int64_t nvec, int64_t batch, int dim,
                             const double* d_disp, int64_t q, const int64_t* d_counts, double* d_overlap,
                             double* d_collectivity) {
  return modes_overlap(ModesOf{ctx, m, nvec, batch, dim}, d_v, d_disp, q, d_counts, d_overlap, d_collectivity);
}
int sc_batch_plan_modes_overlap_f64(sc_batch_plan* plan, const double* d_v, int64_t nvec, int64_t first_row,
                                    const double* d_disp, int64_t q, const int64_t* d_counts, double* d_overlap,
                                    double* d_collectivity) {
  return modes_overlap(plan_modes_of(plan, nvec, first_row), d_v, d_disp, q, d_counts, d_overlap, d_collectivity);
}

int sc_dev_mode_response_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                             int dim, const sc_mode_selection* sel, const int64_t* d_counts, const double* d_force,
                             int64_t q, const double* d_atom_scale, double* d_out) {
  return modes_response(ModesOf{ctx, m, nvec, batch, dim}, d_w, d_v, sel, d_counts, d_force, q, d_atom_scale, d_out);
}
int sc_batch_plan_mode_response_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                                    const sc_mode_selection* sel, const int64_t* d_counts, const double* d_force,
                                    int64_t q, const double* d_atom_scale, double* d_out) {
  return modes_response(plan_modes_of(plan, nvec, sel ? sel->reserved : 0), d_w, d_v, sel, d_counts, d_force, q,
                        d_atom_scale, d_out);
}

int sc_dev_mode_combine_f64(sc_ctx* ctx, const double* d_v, int64_t m, int64_t nvec, int64_t batch, int dim,
                            const double* d_coef, int64_t q, const int64_t* d_counts, const double* d_atom_scale,
                            double* d_out) {
  return modes_combine(ModesOf{ctx, m, nvec, batch, dim}, d_v, d_coef, q, d_counts, d_atom_scale, d_out);
}
int sc_batch_plan_mode_combine_f64(sc_batch_plan* plan, const double* d_v, int64_t nvec, int64_t first_row,
                                   const double* d_coef, int64_t q, const int64_t* d_counts, const double* d_atom_scale,
                                   double* d_out) {
  return modes_combine(plan_modes_of(plan, nvec, first_row), d_v, d_coef, q, d_counts, d_atom_scale, d_out);
}

int64_t sc_dev_modes_workspace_bytes(int64_t m, int64_t nvec, int64_t batch, int dim, int64_t n_sel, int what,
                                     int64_t budget_bytes) {
  return modes_workspace_bytes(ModesOf{nullptr, m, nvec, batch, dim}, n_sel, what, budget_bytes);
}
int64_t sc_batch_plan_modes_workspace_bytes(const sc_batch_plan* plan, int64_t nvec, int64_t n_sel, int what,
                                            int64_t budget_bytes) {
  return modes_workspace_bytes(plan_modes_of(plan, nvec, 0), n_sel, what, budget_bytes);
}

// ---- rotation-translation blocks (rtb.hip) --------------------------------------------------------------------------
int sc_dev_rtb_hessian_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, const int64_t* d_pairs, int64_t k,
                           const double* d_gamma, const double* d_inv_sqrt_mass, const double* d_P,
                           const int32_t* d_block_of_atom, const int64_t* d_offset, int64_t n_blocks, int64_t nr,
                           const int64_t* d_order, const int64_t* d_seg_start, int64_t n_seg,
                           const int64_t* d_block_start, double* d_hb) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (n_atoms <= 0 || n_blocks <= 0 || nr <= 0 || k < 0 || n_seg < 0)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "rtb: sizes must be positive (k, n_seg: not negative)");
  if (n_blocks > n_atoms || nr > 6 * n_blocks || n_seg > k)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "rtb: %lld blocks / %lld rows / %lld segments do not fit %lld atoms, %lld pairs",
                        (long long)n_blocks, (long long)nr, (long long)n_seg, (long long)n_atoms, (long long)k);
  if (!d_coord || !d_P || !d_block_of_atom || !d_offset || !d_hb)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "rtb: a required pointer is NULL");
  if (k > 0 && (!d_pairs || !d_gamma || !d_order || !d_seg_start || !d_block_start || n_seg == 0))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "rtb: pairs / gamma / order / segment starts are required with k > 0");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_rtb_hessian(ctx, d_coord, n_atoms, d_pairs, k, d_gamma, d_inv_sqrt_mass, d_P, d_block_of_atom, d_offset,
                            n_blocks, nr, d_order, d_seg_start, n_seg, d_block_start, d_hb);
}

int sc_dev_rtb_expand_f64(sc_ctx* ctx, const double* d_u, int64_t nvec, int64_t nr, const double* d_P,
                          const int32_t* d_block_of_atom, const int64_t* d_offset, int64_t n_atoms, double* d_v) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (nvec <= 0 || nr <= 0 || n_atoms <= 0 || nvec > 8 * (int64_t)65535)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "rtb: sizes must be positive (nvec at most 524280)");
  if (!d_u || !d_P || !d_block_of_atom || !d_offset || !d_v)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "rtb: a required pointer is NULL");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_rtb_expand(ctx, d_u, nvec, nr, d_P, d_block_of_atom, d_offset, n_atoms, d_v);
}

// ---- the network as an operator on the pair list (pair_operator.hip) -------------------------------------------------
static int pairs_network_check(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs,
                               int64_t k, const double* d_gamma, const double* d_x, int64_t q) {
  if (dim != 1 && dim != 3) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: dim must be 1 or 3, got %d", dim);
  if (n_atoms <= 0 || k < 0 || q < 0)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: n_atoms must be positive, k and q not negative");
  if (n_atoms > ((int64_t)1 << 32))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: at most 2^32 atoms");
  if (dim == 3 && !d_coord) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: dim 3 needs the coordinates");
  if (k > 0 && (!d_pairs || !d_gamma))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: pairs and gamma are required with k > 0");
  if (q > 0 && !d_x) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the rows are required with q > 0");
  return SC_OK;
}

int sc_dev_pairs_apply_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs,
                           int64_t k, const double* d_gamma, const int64_t* d_row_start, const double* d_atom_scale,
                           const double* d_x, int64_t q, double* d_y, double* d_energy) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (!d_y && !d_energy) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: neither a product nor energies asked for");
  SC_TRY(pairs_network_check(ctx, d_coord, n_atoms, dim, d_pairs, k, d_gamma, d_x, q));
  if (k > 0 && !d_row_start) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: row starts are required with k > 0");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_pairs_apply(ctx, d_coord, n_atoms, dim, d_pairs, k, d_gamma, d_row_start, d_atom_scale, d_x, q, d_y,
                            d_energy);
}

int sc_dev_pairs_strain_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs,
                            int64_t k, const double* d_gamma, const double* d_atom_scale, const int64_t* d_pair_idx,
                            int64_t ks, const double* d_x, int64_t q, double* d_out) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(pairs_network_check(ctx, d_coord, n_atoms, dim, d_pairs, k, d_gamma, d_x, q));
  if (ks < 0 || ks > ((int64_t)1 << 38))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the number of listed pairs must lie in 0 .. 2^38");
  if (ks > 0 && q > 0 && (!d_pair_idx || !d_out))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the pair indices and the result are required");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_pairs_strain(ctx, d_coord, n_atoms, dim, d_pairs, k, d_gamma, d_atom_scale, d_pair_idx, ks, d_x, q,
                             d_out);
}

int sc_dev_pairs_panel_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs,
                           int64_t k, const double* d_gamma, const int64_t* d_row_start, const double* d_atom_scale,
                           const double* d_x, double* d_z, int64_t ld, int64_t q, double alpha, double beta,
                           double gamma_c) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(pairs_network_check(ctx, d_coord, n_atoms, dim, d_pairs, k, d_gamma, d_x, q));
  if (k > 0 && !d_row_start) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: row starts are required with k > 0");
  if (ld < q) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the leading dimension %lld is below the %lld columns",
                                  (long long)ld, (long long)q);
  if (q > 65535 * (int64_t)64) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: at most 4194240 columns per panel");
  if (q > 0 && !d_z) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the result panel is required with q > 0");
  if (d_z && d_z == d_x) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the result panel must not be the input panel");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_pairs_panel(ctx, d_coord, n_atoms, dim, d_pairs, k, d_gamma, d_row_start, d_atom_scale, d_x, d_z, ld, q,
                            alpha, beta, gamma_c);
}

// ---- conjugate gradients on the pair list (pair_cg.hip) ---------------------------------------------------------------
static int pairs_cg_panel_check(sc_ctx* ctx, int64_t n_atoms, int64_t ld, int64_t q, const void* const* panels, int count,
                                const void* d_state, const void* d_work, size_t work_bytes) {
  if (ld < q) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the leading dimension %lld is below the %lld columns",
                                  (long long)ld, (long long)q);
  if (q > 65535 * (int64_t)64) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: at most 4194240 columns per panel");
  if (q == 0) return SC_OK;
  for (int a = 0; a < count; ++a) {
    if (!panels[a]) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the X, R, P and Q panels are required with q > 0");
    for (int b = 0; b < a; ++b)
      if (panels[a] == panels[b]) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the X, R, P and Q panels must be distinct");
  }
  if (!d_state || !d_work) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the state and the workspace are required");
  if (work_bytes < pairs_cg_workspace_bytes(n_atoms, q))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the workspace holds %zu bytes, %zu are needed", work_bytes,
                        pairs_cg_workspace_bytes(n_atoms, q));
  return SC_OK;
}

int sc_dev_pairs_cg_workspace(int64_t n_atoms, int64_t q, size_t* bytes) {
  if (!bytes || n_atoms <= 0 || q < 0 || n_atoms > ((int64_t)1 << 32) || q > 65535 * (int64_t)64) return SC_ERR_INVALID_ARG;
  *bytes = pairs_cg_workspace_bytes(n_atoms, q);
  return SC_OK;
}

int sc_dev_pairs_cg_init_f64(sc_ctx* ctx, int64_t n_atoms, int dim, double* d_x, const double* d_r, double* d_p, int64_t ld,
                             int64_t q, double tol, double* d_state, void* d_work, size_t work_bytes) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (dim != 1 && dim != 3) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: dim must be 1 or 3, got %d", dim);
  if (n_atoms <= 0 || q < 0 || n_atoms > ((int64_t)1 << 32))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: n_atoms must lie in 1 .. 2^32, q must not be negative");
  if (!(tol > 0.0)) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: tol must be positive");
  const void* panels[3] = {d_x, d_r, d_p};
  SC_TRY(pairs_cg_panel_check(ctx, n_atoms, ld, q, panels, 3, d_state, d_work, work_bytes));
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_pairs_cg_init(ctx, n_atoms, dim, d_x, d_r, d_p, ld, q, tol, d_state, (double*)d_work);
}

int sc_dev_pairs_cg_step_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs,
                             int64_t k, const double* d_gamma, const int64_t* d_row_start, const double* d_atom_scale,
                             double* d_x, double* d_r, double* d_p, double* d_q, int64_t ld, int64_t q, double* d_state,
                             void* d_work, size_t work_bytes, int64_t iterations) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(pairs_network_check(ctx, d_coord, n_atoms, dim, d_pairs, k, d_gamma, d_p, q));
  if (k > 0 && !d_row_start) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: row starts are required with k > 0");
  if (iterations < 0) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs: the number of iterations must not be negative");
  const void* panels[4] = {d_x, d_r, d_p, d_q};
  SC_TRY(pairs_cg_panel_check(ctx, n_atoms, ld, q, panels, 4, d_state, d_work, work_bytes));
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return launch_pairs_cg_step(ctx, d_coord, n_atoms, dim, d_pairs, k, d_gamma, d_row_start, d_atom_scale, d_x, d_r, d_p,
                              d_q, ld, q, d_state, (double*)d_work, iterations);
}

void sc_batch_plan_destroy(sc_batch_plan* plan) {
  if (!plan) return;
  (void)hipSetDevice(plan->ctx->device);
  (void)hipStreamSynchronize(plan->ctx->stream);
  if (plan->d_blob) (void)hipFree(plan->d_blob);
  delete plan;
}

// ---- device-resident eigenpairs --------------------------------------------------------------------------
}  // extern "C"

struct sc_modes {
  sc_ctx* ctx = nullptr;
  int64_t n = 0;
  int dim = 1;
  double* d_w = nullptr;
  double* d_v = nullptr;
};

namespace {
int modes_alloc(sc_ctx* ctx, int64_t n, int dim, sc_modes** out) {
  sc_modes* m = new (std::nothrow) sc_modes();
  if (!m) return sc_set_error(ctx, SC_ERR_NOMEM, "out of host memory");
  m->ctx = ctx; m->n = n; m->dim = dim;
  if (hipMalloc(&m->d_w, sizeof(double) * (size_t)std::max<int64_t>(n, 1)) != hipSuccess ||
      hipMalloc(&m->d_v, sizeof(double) * (size_t)std::max<int64_t>(n * n, 1)) != hipSuccess) {
    (void)hipFree(m->d_w);
    delete m;
    return sc_set_error(ctx, SC_ERR_NOMEM, "cannot allocate %lld x %lld eigenvectors on the device", (long long)n,
                        (long long)n);
  }
  *out = m;
  return SC_OK;
}

// mode list -> validated int32 list on the device (in scratch)
int stage_mode_list(sc_modes* m, const int64_t* idx, int64_t k, int* d_sel) {
  sc_ctx* ctx = m->ctx;
  std::vector<int> h((size_t)k);
  for (int64_t i = 0; i < k; ++i) {
    int64_t v = idx[i];
    if (v < 0) v += m->n;   // NumPy-style negative indices
    if (v < 0 || v >= m->n)
      return sc_set_error(ctx, SC_ERR_INDEX, "mode index %lld out of bounds for %lld modes", (long long)idx[i],
                          (long long)m->n);
    h[(size_t)i] = (int)v;
  }
  if (k > 0) {
    SC_HIP(ctx, hipMemcpyAsync(d_sel, h.data(), (size_t)k * 4, hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // h goes out of scope
  }
  return SC_OK;
}

// msf / tensors / dcc of one model over a mode list: the validated list and the (out_elems) result in ctx->scratch, `run`
// on them, the result copied to `out`.  `run` is a batch consumer with a batch of one (nvec = m = n, no counts, default
// budget; its workspace is ctx->modes_ws): one arithmetic order for a model, a batch and a ragged batch.
template <typename Run>
int modes_list_call(sc_modes* m, const int64_t* mode_idx, int64_t k, size_t out_elems, double* out, Run run) {
  sc_ctx* ctx = m->ctx;
  if (k < 0 || k > INT32_MAX / 4 || (k > 0 && !mode_idx) || (m->n > 0 && !out))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (m->n == 0) return SC_OK;
  SC_TRY(sc_reserve_scratch(ctx, align_up((size_t)k * 4, 256) + align_up(out_elems * 8, 256) + 1024));
  Bump bump{(char*)ctx->scratch};
  int* d_sel = bump.take<int>((size_t)std::max<int64_t>(k, 1));
  double* d_out = bump.take<double>(out_elems);
  SC_TRY(stage_mode_list(m, mode_idx, k, d_sel));
  sc_mode_selection sel{};
  sel.kind = SC_SEL_ROWS;
  sel.d_rows = d_sel;
  sel.n_rows = k;
  SC_TRY(run(sel, d_out));
  SC_HIP(ctx, hipMemcpyAsync(out, d_out, out_elems * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}
}  // namespace

extern "C" {

int sc_modes_from_coord(sc_ctx* ctx, const double* coord, int64_t n, int dim, const sc_ff_desc* ff,
                        const sc_patch_desc* patch, const double* inv_sqrt_mass, sc_modes** out) {
  SC_TRY(check_coord_args(ctx, coord, n));
  SC_TRY(check_ff(ctx, ff));
  if (!out || (dim != 1 && dim != 3)) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t m = n * dim;
  const size_t elems = (size_t)m * m;
  sc_modes* md = nullptr;
  SC_TRY(modes_alloc(ctx, m, dim, &md));
  int rc = SC_OK;
  if (n > 0) {
    Staged st;
    Bump bump{};
    rc = stage_inputs(ctx, coord, n, ff, patch, inv_sqrt_mass, elems * 8 + 2048, st, bump);
    if (rc == SC_OK) {
      double* d_m = bump.take<double>(elems);
      const PatchDev* pdev = st.has_patch ? &st.patch : nullptr;
      rc = dim == 1 ? launch_kirchhoff(ctx, st.d_coord, n, 1, st.ff_dev, pdev, st.d_w, d_m, nullptr)
                    : launch_hessian(ctx, st.d_coord, n, 1, st.ff_dev, pdev, st.d_w, d_m);
      if (rc == SC_OK) rc = eigh_batched(ctx, d_m, m, 1, md->d_w, md->d_v);
      if (rc == SC_OK && hipStreamSynchronize(ctx->stream) != hipSuccess)
        rc = sc_set_error(ctx, SC_ERR_HIP, "eigensolve failed");
    }
  }
  if (rc != SC_OK) { sc_modes_destroy(md); return rc; }
  *out = md;
  return SC_OK;
}

int sc_modes_from_matrix(sc_ctx* ctx, const double* a, int64_t n, int dim, sc_modes** out) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (n < 0 || (n > 0 && !a) || !out || (dim != 1 && dim != 3) || n % dim != 0)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  sc_modes* md = nullptr;
  SC_TRY(modes_alloc(ctx, n, dim, &md));
  int rc = SC_OK;
  if (n > 0) {
    const size_t elems = (size_t)n * n;
    rc = sc_reserve_scratch(ctx, elems * 8 + 1024);
    if (rc == SC_OK) {
      double* d_a = reinterpret_cast<double*>(ctx->scratch);
      if (hipMemcpyAsync(d_a, a, elems * 8, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        rc = sc_set_error(ctx, SC_ERR_HIP, "upload failed");
      if (rc == SC_OK) rc = eigh_batched(ctx, d_a, n, 1, md->d_w, md->d_v);
      if (rc == SC_OK && hipStreamSynchronize(ctx->stream) != hipSuccess)
        rc = sc_set_error(ctx, SC_ERR_HIP, "eigensolve failed");
    }
  }
  if (rc != SC_OK) { sc_modes_destroy(md); return rc; }
  *out = md;
  return SC_OK;
}

void sc_modes_destroy(sc_modes* m) {
  if (!m) return;
  (void)hipSetDevice(m->ctx->device);
  (void)hipFree(m->d_w);
  (void)hipFree(m->d_v);
  delete m;
}

int64_t sc_modes_order(const sc_modes* m) { return m ? m->n : -1; }

int sc_modes_get(sc_modes* m, double* w, double* v) {
  if (!m) return SC_ERR_INVALID_ARG;
  sc_ctx* ctx = m->ctx;
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (m->n == 0) return SC_OK;
  if (w) SC_HIP(ctx, hipMemcpyAsync(w, m->d_w, (size_t)m->n * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (v) SC_HIP(ctx, hipMemcpyAsync(v, m->d_v, (size_t)m->n * m->n * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

int sc_modes_msf(sc_modes* m, const int64_t* mode_idx, int64_t k, double* out) {
  if (!m) return SC_ERR_INVALID_ARG;
  return modes_list_call(m, mode_idx, k, (size_t)(m->n / m->dim), out, [m](const sc_mode_selection& sel, double* d_out) {
    return batch_msf_device(m->ctx, m->d_w, m->d_v, m->n, m->n, 1, m->dim, sel, nullptr, 0, d_out);
  });
}

int sc_modes_aniso(sc_modes* m, const int64_t* mode_idx, int64_t k, double* out) {
  if (!m) return SC_ERR_INVALID_ARG;
  if (m->dim != 3)
    return sc_set_error(m->ctx, SC_ERR_INVALID_ARG, "anisotropic fluctuation tensors need an ANM (dim 3)");
  return modes_list_call(m, mode_idx, k, (size_t)(m->n / 3) * 6, out, [m](const sc_mode_selection& sel, double* d_out) {
    return batch_aniso_device(m->ctx, m->d_w, m->d_v, m->n, m->n, 1, sel, nullptr, 0, d_out);
  });
}

int sc_modes_distfluct(sc_modes* m, const int64_t* mode_idx, int64_t k, const double* coord, double* out) {
  if (!m) return SC_ERR_INVALID_ARG;
  sc_ctx* ctx = m->ctx;
  if (m->dim != 3) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "distance fluctuations need an ANM (dim 3)");
  if (k < 0 || k > INT32_MAX / 4 || (k > 0 && !mode_idx) || (m->n > 0 && (!coord || !out)))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const size_t N = (size_t)(m->n / 3);
  SC_TRY(sc_reserve_scratch(ctx, align_up((size_t)k * 4, 256) + align_up(N * 24, 256) + align_up(N * N * 8, 256) + 1024));
  Bump bump{(char*)ctx->scratch};
  int* d_sel = bump.take<int>((size_t)std::max<int64_t>(k, 1));
  double* d_coord = bump.take<double>(std::max<size_t>(N * 3, 1));
  double* d_out = bump.take<double>(std::max<size_t>(N * N, 1));
  SC_TRY(stage_mode_list(m, mode_idx, k, d_sel));   // (the index errors come first, whatever else is empty)
  if (m->n == 0) return SC_OK;
  SC_HIP(ctx, hipMemcpyAsync(d_coord, coord, N * 24, hipMemcpyHostToDevice, ctx->stream));
  sc_mode_selection sel{};
  sel.kind = SC_SEL_ROWS;
  sel.d_rows = d_sel;
  sel.n_rows = k;
  // the batch kernel with a batch of one: one arithmetic order for a model, a batch and a ragged batch
  SC_TRY(batch_distfluct_device(ctx, m->d_w, m->d_v, m->n, m->n, 1, sel, nullptr, d_coord, nullptr, d_out));
  SC_HIP(ctx, hipMemcpyAsync(out, d_out, N * N * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

int sc_modes_overlap(sc_modes* m, const int64_t* mode_idx, int64_t k, const double* disp, int64_t q, double* overlap_out,
                     double* collectivity_out) {
  if (!m) return SC_ERR_INVALID_ARG;
  sc_ctx* ctx = m->ctx;
  if (k < 0 || k > INT32_MAX / 4 || (k > 0 && !mode_idx) || q < 0 || q > INT32_MAX / 4 ||
      (!overlap_out && !collectivity_out) || (q > 0 && (!disp || !overlap_out)) || (q == 0 && !collectivity_out))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)m->n, K = (size_t)k, Q = (size_t)q;
  SC_TRY(sc_reserve_scratch(ctx, align_up(K * 4, 256) + align_up(Q * n * 8, 256) + align_up(Q * K * 8, 256) +
                                     align_up(K * 8, 256) + 1024));
  Bump bump{(char*)ctx->scratch};
  int* d_sel = bump.take<int>(std::max<size_t>(K, 1));
  double* d_disp = bump.take<double>(std::max<size_t>(Q * n, 1));
  double* d_ov = bump.take<double>(std::max<size_t>(Q * K, 1));
  double* d_co = bump.take<double>(std::max<size_t>(K, 1));
  SC_TRY(stage_mode_list(m, mode_idx, k, d_sel));   // (the index errors come first, whatever else is empty)
  if (m->n == 0 || k == 0) return SC_OK;
  if (q > 0) SC_HIP(ctx, hipMemcpyAsync(d_disp, disp, Q * n * 8, hipMemcpyHostToDevice, ctx->stream));
  // the batch kernel with a batch of one: one arithmetic order for a model, a batch and a ragged batch
  SC_TRY(modes_overlap_device(ctx, m->d_v, m->n, m->n, 1, m->dim, d_sel, k, d_disp, q, nullptr, q > 0 ? d_ov : nullptr,
                              collectivity_out ? d_co : nullptr));
  if (q > 0) SC_HIP(ctx, hipMemcpyAsync(overlap_out, d_ov, Q * K * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (collectivity_out) SC_HIP(ctx, hipMemcpyAsync(collectivity_out, d_co, K * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

int sc_modes_response(sc_modes* m, const int64_t* mode_idx, int64_t k, double rcond, const double* force, int64_t q,
                      const double* atom_scale, double* out) {
  if (!m) return SC_ERR_INVALID_ARG;
  sc_ctx* ctx = m->ctx;
  const bool pinv = mode_idx == nullptr;
  if (k < 0 || k > INT32_MAX / 4 || (pinv && (k != 0 || !(rcond >= 0.0))) || q < 0 || q > INT32_MAX / 4 ||
      (q > 0 && m->n > 0 && (!force || !out)))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)m->n, K = (size_t)k, Q = (size_t)q, N = n / (size_t)m->dim;
  SC_TRY(sc_reserve_scratch(ctx, align_up(K * 4, 256) + 2 * align_up(Q * n * 8, 256) + align_up(N * 8, 256) + 1024));
  Bump bump{(char*)ctx->scratch};
  int* d_sel = bump.take<int>(std::max<size_t>(K, 1));
  double* d_force = bump.take<double>(std::max<size_t>(Q * n, 1));
  double* d_out = bump.take<double>(std::max<size_t>(Q * n, 1));
  double* d_scale = bump.take<double>(std::max<size_t>(N, 1));
  SC_TRY(stage_mode_list(m, mode_idx, k, d_sel));   // (the index errors come first, whatever else is empty)
  if (m->n == 0 || q == 0) return SC_OK;
  SC_HIP(ctx, hipMemcpyAsync(d_force, force, Q * n * 8, hipMemcpyHostToDevice, ctx->stream));
  if (atom_scale) SC_HIP(ctx, hipMemcpyAsync(d_scale, atom_scale, N * 8, hipMemcpyHostToDevice, ctx->stream));
  sc_mode_selection sel{};
  if (pinv) {
    sel.kind = SC_SEL_PINV;
    sel.rcond = rcond;
  } else {
    sel.kind = SC_SEL_ROWS;
    sel.d_rows = d_sel;
    sel.n_rows = k;
  }
  // the batch kernels with a batch of one: one arithmetic order for a model, a batch and a ragged batch
  SC_TRY(modes_response_device(ctx, m->d_w, m->d_v, m->n, m->n, 1, m->dim, sel, nullptr, d_force, q,
                               atom_scale ? d_scale : nullptr, 0, d_out));
  SC_HIP(ctx, hipMemcpyAsync(out, d_out, Q * n * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

int sc_modes_combine(sc_modes* m, const int64_t* mode_idx, int64_t k, const double* coef, int64_t q, double* out) {
  if (!m) return SC_ERR_INVALID_ARG;
  sc_ctx* ctx = m->ctx;
  if (k < 0 || k > INT32_MAX / 4 || (k > 0 && !mode_idx) || q < 0 || q > INT32_MAX / 4 ||
      (q > 0 && ((k > 0 && !coef) || (m->n > 0 && !out))))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)m->n, K = (size_t)k, Q = (size_t)q;
  SC_TRY(sc_reserve_scratch(ctx, align_up(K * 4, 256) + align_up(Q * K * 8, 256) + align_up(Q * n * 8, 256) + 1024));
  Bump bump{(char*)ctx->scratch};
  int* d_sel = bump.take<int>(std::max<size_t>(K, 1));
  double* d_coef = bump.take<double>(std::max<size_t>(Q * K, 1));
  double* d_out = bump.take<double>(std::max<size_t>(Q * n, 1));
  SC_TRY(stage_mode_list(m, mode_idx, k, d_sel));   // (the index errors come first, whatever else is empty)
  if (m->n == 0 || q == 0) return SC_OK;
  if (k > 0) SC_HIP(ctx, hipMemcpyAsync(d_coef, coef, Q * K * 8, hipMemcpyHostToDevice, ctx->stream));
  // the batch kernels with a batch of one: one arithmetic order for a model, a batch and a ragged batch
  SC_TRY(modes_combine_device(ctx, m->d_v, m->n, m->n, 1, m->dim, d_sel, k, d_coef, q, nullptr, nullptr, 0, d_out));
  SC_HIP(ctx, hipMemcpyAsync(out, d_out, Q * n * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

int sc_modes_dcc(sc_modes* m, const int64_t* mode_idx, int64_t k, int norm, double* out) {
  if (!m) return SC_ERR_INVALID_ARG;
  const size_t N = (size_t)(m->n / m->dim);
  return modes_list_call(m, mode_idx, k, N * N, out, [m, norm](const sc_mode_selection& sel, double* d_out) {
    return batch_dcc_device(m->ctx, m->d_w, m->d_v, m->n, m->n, 1, m->dim, sel, nullptr, norm, 0, d_out);
  });
}

int sc_modes_prs(sc_modes* m, double rcond, int norm, double* out) {
  if (!m) return SC_ERR_INVALID_ARG;
  sc_ctx* ctx = m->ctx;
  if (m->dim != 3) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "perturbation response scanning needs an ANM (dim 3)");
  if (m->n > 0 && !out) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (m->n == 0) return SC_OK;
  const size_t N = (size_t)(m->n / 3);
  const size_t work = prs_scratch_bytes(m->n);
  SC_TRY(sc_reserve_scratch(ctx, work + align_up(N * N * 8, 256) + 1024));
  Bump bump{(char*)ctx->scratch};
  double* d_out = bump.take<double>(N * N);
  char* scratch = bump.take<char>(work);
  SC_TRY(modes_prs_device(ctx, m->d_v, m->d_w, m->n, rcond, norm, scratch, d_out));
  SC_HIP(ctx, hipMemcpyAsync(out, d_out, N * N * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

}  // extern "C"
