// Internal declarations shared by the translation units of libspringcraft_hip.so.
// Nothing here is part of the C ABI (see include/springcraft_hip.h for that).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/springcraft_hip.h"

// ---- context -----------------------------------------------------------------------------
struct sc_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // second stream + events for work that is independent of what runs on `stream` (created on first use)
  hipStream_t aux_stream = nullptr;
  // further side streams (bulge chasing runs parts of the batch side by side) with one join event each
  std::vector<hipStream_t> side_streams;
  std::vector<hipEvent_t> side_joins;
  hipEvent_t aux_fork = nullptr, aux_join = nullptr;
  std::string err;
  int num_cus = 0;

  // cached device workspace for the eigensolver (grown on demand, never shrunk)
  void* ws = nullptr;
  size_t ws_bytes = 0;
  // small cached scratch for the assembly entry points (patch tables, counts, ...)
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  // node tables / oversize-merge copies of the divide-and-conquer solver (lives across a whole eigensolve, so it
  // cannot share `scratch`, which the assembly entry points hold while they call the solver)
  void* dc_aux = nullptr;
  size_t dc_aux_bytes = 0;
  // eigenvector / scaled-eigenvector buffers of pinvh_device (covariance properties), alive across its eigensolve
  void* pinv_ws = nullptr;
  size_t pinv_ws_bytes = 0;
  // what a one-matrix value-window solve sizes only after its count (eigh_window): the inverse-iteration workspace and the
  // m eigenpairs.  Growing `ws` at that point would move the tridiagonalisation's slabs, which are still needed
  void* win_ws = nullptr;
  size_t win_ws_bytes = 0;
  // weights, partial sums and GEMM operands of the batch consumers (batch_consumers.hip): a buffer of their own, so that
  // a consumer enqueued behind a solve never grows -- and thereby moves -- a buffer that solve still uses
  void* modes_ws = nullptr;
  size_t modes_ws_bytes = 0;

  // host -> device uploads of descriptor tables without a stream synchronisation: the tables are copied into this
  // pinned arena first (sc_stage_upload) and the arena is recycled once the event recorded at the end of the solve
  // (sc_stage_end) has passed
  // (two arenas taking turns, so that the host may enqueue solve k + 1 while solve k still runs)
  char* h_stage[2] = {nullptr, nullptr};
  size_t h_stage_bytes[2] = {0, 0}, h_stage_off[2] = {0, 0};
  hipEvent_t h_stage_done[2] = {nullptr, nullptr};
  bool h_stage_pending[2] = {false, false};
  int h_stage_cur = 0;
  // deferred status of the device-pointer eigensolver entries (which do not synchronise): [0] = 1 + index of a matrix
  // with a NaN / Inf entry, [1] = the tridiagonal QL iteration failed.  Read and cleared by sc_deferred_status.
  // Round 6, events a solve no longer looks at from the host (kSpStatusWords words; sc_collect_events adds them to the
  // counters below at the next synchronising call): [2] persistent chases that k_chase_finish had to finish, [3] of
  // those: after a time-out (not the test hook), [4] sweeps the persistent kernels finished, [5] panels factored by
  // k_panel_serial after k_panel_coop gave up, [6] chases left incomplete without a raised flag (an XCD that owns
  // matrices received no workgroup), [7] tridiagonalisations k_sytrd_takeover did after k_sytrd_resident gave up ([8] of
  // those after an aborted roll call, [9] after a wait lost in mid-run, [10] where).
  unsigned long long* d_status = nullptr;
  // [11] = 1 + number of a matrix whose Cholesky factorisation met a pivot <= 0 or NaN (potrf.hip); sc_collect_events moves it
  // here, where it waits for sc_deferred_status
  long long potrf_failed = 0;

  int two_stage = -1;   // eigensolver path: -1 automatic, 0 one-stage, 1 two-stage tridiagonalisation
  // persistent bulge chase (sb2st.hip): chase_ok = 0 once a chase of this context ran into its time-out (never
  // expected; the per-wavefront launches take over from then on); chase_mode / chase_give_up are set through the debug
  // entry sc_dbg_set_chase (-1: SPRINGCRAFT_BULGE_PERSISTENT or the size rule; 0 / 1 / 2 as that variable).
  int chase_ok = -1;
  int chase_mode = -1, chase_give_up = 0;
  int chase_form = -1;   // debug entry: 1 = pair form, 0 = one sweep per workgroup, 2 = that with a matrix' workgroups on all XCDs, -1 = by size
  // XCDs of this device as a probe launch saw them (distinct XCC_ID values; 0 = not probed yet), and whether
  // k_bulge_pair's dynamic LDS size has been raised on THIS context's device (-1 = not tried, 0 = refused, 1 = set):
  // the attribute is per device, a process may own contexts on several
  int nxcd = 0;
  int pair_attr = -1;
  long long cnt_pair_fallbacks = 0;   // pair launches that were refused and re-issued as k_bulge_chase
  // k_gemm3 (gemm3.hip): whether its dynamic LDS size has been raised on this context's device (-1 not tried, 0 refused,
  // 1 set), and the launches it took
  int gemm3_attr = -1;
  // k_symm3 (symm3.hip): a page of zeros its loaders point pieces at that must not count, and the launches it took
  void* d_zeros = nullptr;
  long long cnt_symm3_launches = 0;
  bool gemm3_side_by_side = false;   // the caller runs parts of the batch on several streams (band reduction): see gemm3_would_take
  long long cnt_gemm3_launches = 0;
  // k_panel_coop (sy2sb.hip): dynamic LDS attribute of this device (-1 not tried, 0 refused, 1 set); coop_ok = 0
  // once a wait between its workgroups timed out (the context then keeps to the chunked panel launches)
  int coop_attr = -1, coop_ok = -1;
  int coop_min_rows = -1;   // debug entry sc_dbg_set_panel_coop: rows from which a panel takes it (0 never, -1 default rule)
  int coop_fail_panel = -1; // debug entry sc_dbg_set_panel_coop_fail: panel from which the abort flags are raised (test hook)
  // k_sytrd_resident (tridiag.hip): resident_ok = 0 once a wait was lost or three roll calls failed (the launches per column from
  // then on); resident_mode / _hook / _wgs through the debug entry sc_dbg_set_resident (-1 / 0 / 0: the default rule)
  int resident_ok = -1, resident_mode = -1, resident_hook = 0, resident_wgs = 0;
  long long cnt_resident_launches = 0, cnt_resident_takeovers = 0, cnt_resident_rollcalls = 0, cnt_resident_lost = 0;
  long long resident_lost_at = -1;   // (step << 32 | workgroup) of the most recent lost wait / arrivals at the last failed roll call
  int resident_strikes = 0;          // failed roll calls since the kernel was (re-)armed: the context gives it up at the third
  // control block of the persistent chase (kChaseCtlInts ints, allocated with the context and zeroed before every chase
  // launch): an allocation of its own, since dc_aux is reused by the D&C of the same solve before the block is read --
  // for n > 7000 its global scratch covers the bytes the block sat at in dc_aux.  last_chase_ctl points to it after a
  // chase launch until sc_collect_events has read it; chase_ctl_xcds: ticket slots that launch used (1 for the spread form)
  int* d_chase_ctl = nullptr;
  int* last_chase_ctl = nullptr;
  int chase_ctl_xcds = 8;
  long long cnt_coop_launches = 0, cnt_coop_timeouts = 0;
  // which form the policy (twostage_policy.h) chose, counted on the host where the form is launched (sc_ctx_get_counter):
  // calls of run_panel by panel-QR form ([0..3] k_panel_wg<1,8> <2,8> <3,4> <4,2>, [4] <10,1,512>, [5] <12,1,512>,
  // [6] the blocked and [7] the unblocked chunked launches; k_panel_coop: cnt_coop_launches) and by role (first / second of
  // a pair), with the SYMM on the two triangular-operand launches (k_symm3: cnt_symm3_launches), trailing updates
  // k_gemm3 declined; the K slices, stage-1 parts and per-wavefront stream parts of the most recent solve (0: it did not
  // chase by the per-wavefront launches); bt2_batched by kernel ([0] k_bt2_wave, [1] k_bt2_apply<4>, [2] k_bt2_apply<8>)
  // and its launches with the workgroups dealt to the XCDs
  long long cnt_panel_form[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  long long cnt_panel_role[2] = {0, 0};
  long long cnt_symm_tri = 0, cnt_gemm3_declined = 0;
  int last_symm_slices = 0, last_stage1_parts = 0, last_chase_stream_parts = 0;
  long long cnt_bt2_form[3] = {0, 0, 0}, cnt_bt2_xcd = 0;
  // event counters since the context was created (sc_ctx_get_counter)
  long long cnt_chase_launches = 0, cnt_chase_timeouts = 0, cnt_chase_incomplete = 0, cnt_chase_resumed = 0,
            cnt_chase_sweeps = 0, cnt_stepwise_chases = 0, cnt_pair_launches = 0;
  int chase_tickets[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // workgroups per XCD of the most recent chase launch (chase_ctl_xcds of them)
  int chase_wait[3] = {-1, -1, -1};                  // (matrix, sweep, task) of the wait that timed out last
  bool profiling = false;
  // the most recent profiled eigensolve, ms (sc_last_eigh_timings): the three phases between the solve's four events, then
  // SYMV / SYR2K sums (one-stage) or band reduction / bulge chasing (two-stage); kTimeBt2 names the path as well: the
  // fused back-transformation of the stage-2 reflectors (two-stage with vectors), or one of the two markers
  enum { kTimeTridiag = 0, kTimeEigen = 1, kTimeBacktransform = 2, kTimeStageA = 3, kTimeStageB = 4, kTimeBt2 = 5 };
  static constexpr double kTimeOneStage = 0.0;            // kTimeBt2 of a one-stage solve
  static constexpr double kTimeTwoStageValues = 1e-9;     // kTimeBt2 of a two-stage solve without vectors
  double last_timings[6] = {0, 0, 0, 0, 0, 0};
  // named kernel-group durations of the most recent profiled eigensolve (sc_last_eigh_phase_ms)
  std::vector<std::pair<std::string, double>> phases;
};

// Sum of the device time between start() / stop() pairs on one stream (HIP events; profiling runs only).  The events are
// resolved in finish(), which synchronises on the last one; destroyed with the object on every return path.
class PhaseTimer {
 public:
  PhaseTimer(sc_ctx* ctx, const char* name, hipStream_t st) : ctx_(ctx), name_(name), st_(st), on_(ctx->profiling) {}
  ~PhaseTimer() { for (hipEvent_t e : ev_) (void)hipEventDestroy(e); }
  void start() { mark(); }
  void stop() { mark(); }
  // stores the sum under `name` in ctx->phases; call after everything timed has been enqueued
  void finish() {
    if (!on_ || ev_.size() < 2) return;
    double total = 0.0;
    if (hipEventSynchronize(ev_.back()) != hipSuccess) return;
    for (size_t i = 0; i + 1 < ev_.size(); i += 2) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev_[i], ev_[i + 1]) == hipSuccess) total += ms;
    }
    for (auto& p : ctx_->phases)
      if (p.first == name_) { p.second = total; return; }
    ctx_->phases.emplace_back(name_, total);
  }
 private:
  void mark() {
    if (!on_) return;
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) { on_ = false; return; }
    (void)hipEventRecord(e, st_);
    ev_.push_back(e);
  }
  sc_ctx* ctx_;
  std::string name_;
  hipStream_t st_;
  bool on_;
  std::vector<hipEvent_t> ev_;
};

// N timing events that are destroyed on every return path (profiling runs only create them).
template <int N>
struct ScopedEvents {
  hipEvent_t e[N];
  ScopedEvents() { for (auto& x : e) x = nullptr; }
  ~ScopedEvents() { for (auto& x : e) if (x) (void)hipEventDestroy(x); }
  ScopedEvents(const ScopedEvents&) = delete;
  ScopedEvents& operator=(const ScopedEvents&) = delete;
  hipEvent_t& operator[](int i) { return e[i]; }
  hipEvent_t* begin() { return e; }
  hipEvent_t* end() { return e + N; }
};

int sc_set_error(sc_ctx* ctx, int code, const char* fmt, ...);

#define SC_HIP(ctx, call)                                                              \
  do {                                                                                 \
    hipError_t e__ = (call);                                                           \
    if (e__ != hipSuccess)                                                             \
      return sc_set_error((ctx), e__ == hipErrorOutOfMemory ? SC_ERR_NOMEM : SC_ERR_HIP, \
                          "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__),      \
                          __FILE__, __LINE__);                                         \
  } while (0)

#define SC_TRY(expr)            \
  do {                          \
    int rc__ = (expr);          \
    if (rc__ != SC_OK) return rc__; \
  } while (0)

// Grow-only cached allocations.
int sc_reserve_ws(sc_ctx* ctx, size_t bytes);
int sc_reserve_scratch(sc_ctx* ctx, size_t bytes);
int sc_reserve_dc_aux(sc_ctx* ctx, size_t bytes);
int sc_reserve_pinv(sc_ctx* ctx, size_t bytes);
int sc_reserve_win(sc_ctx* ctx, size_t bytes);
int sc_reserve_modes(sc_ctx* ctx, size_t bytes);
int sc_aux_stream(sc_ctx* ctx);   // creates aux_stream / aux_fork / aux_join if needed
int sc_side_streams(sc_ctx* ctx, int count);   // makes sure side_streams / side_joins hold `count` entries
// The context on another stream for a scope: launch_gemm_f64 and whatever else takes no stream launches on ctx->stream.
struct StreamScope {
  sc_ctx* c;
  hipStream_t old;
  StreamScope(sc_ctx* c_, hipStream_t s) : c(c_), old(c_->stream) { c->stream = s; }
  ~StreamScope() { c->stream = old; }
  StreamScope(const StreamScope&) = delete;
  StreamScope& operator=(const StreamScope&) = delete;
};
// Parts of a batch side by side on the main stream and parts - 1 side streams.  fork: the side streams wait for what the
// main stream holds so far; stream(q): where part q goes (part 0: the main stream); join: the main stream waits for every
// side stream -- by the destructor at the latest, so also on an error path: what the side streams still have queued is
// ordered before whatever the caller enqueues next on the main stream.
class SideFork {
 public:
  SideFork(sc_ctx* ctx, hipStream_t main) : ctx_(ctx), main_(main) {}
  ~SideFork() { (void)join(); }
  SideFork(const SideFork&) = delete;
  SideFork& operator=(const SideFork&) = delete;
  int fork(int parts) {
    SC_TRY(sc_aux_stream(ctx_));   // (its fork event)
    SC_TRY(sc_side_streams(ctx_, parts - 1));
    SC_HIP(ctx_, hipEventRecord(ctx_->aux_fork, main_));
    for (int q = 1; q < parts; ++q) SC_HIP(ctx_, hipStreamWaitEvent(ctx_->side_streams[q - 1], ctx_->aux_fork, 0));
    parts_ = parts;
    return SC_OK;
  }
  hipStream_t stream(int q) const { return q == 0 ? main_ : ctx_->side_streams[q - 1]; }
  int join() {
    const int parts = parts_;
    parts_ = 1;
    for (int q = 1; q < parts; ++q) {
      SC_HIP(ctx_, hipEventRecord(ctx_->side_joins[q - 1], ctx_->side_streams[q - 1]));
      SC_HIP(ctx_, hipStreamWaitEvent(main_, ctx_->side_joins[q - 1], 0));
    }
    return SC_OK;
  }
 private:
  sc_ctx* ctx_;
  hipStream_t main_;
  int parts_ = 1;
};
// d_dst <- bytes at h_src, enqueued on ctx->stream; h_src may be released as soon as the call returns
int sc_stage_upload(sc_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
// end of a solve that used sc_stage_upload: the arena may be reused when everything enqueued so far has run
int sc_stage_end(sc_ctx* ctx);
// after a synchronisation of ctx->stream: SC_ERR_NOCONV (and the flags cleared) if a solve since the last call met
// non-finite input or a QL failure, else SC_OK
constexpr int kSpStatusWords = 16;
// ints of the persistent chase's control block (sc_ctx::d_chase_ctl; layout at k_bulge_chase in sb2st.hip)
constexpr int kChaseCtlInts = 32;
int sc_deferred_status(sc_ctx* ctx);
// adds the device-side event words to the context's counters (the context's stream must be idle)
int sc_collect_events(sc_ctx* ctx);

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- assembly (assembly.hip) ----------------------------------------------------------------
// Device-side patch tables (all device pointers; null when there are no patches).
struct PatchDev {
  const uint8_t* shut;     // (N) 1 = every contact of this atom is switched off
  const int32_t* row_ptr;  // (N+1) CSR over override entries, both directions stored
  const int32_t* col;      // (nnz)
  const int8_t* flag;      // (nnz) 0 = force off, 1 = force on
  const double* gam;       // (nnz) override force constant, NaN = use the base force field
  int mask_gamma;          // PatchedForceField: base gamma is 0 beyond the base cutoff
};

int launch_kirchhoff(sc_ctx* ctx, const double* d_coord, int64_t n, int64_t batch,
                     const sc_ff_desc& ff, const PatchDev* patch, const double* d_w,
                     double* d_k, int64_t* d_counts);
int launch_hessian(sc_ctx* ctx, const double* d_coord, int64_t n, int64_t batch,
                   const sc_ff_desc& ff, const PatchDev* patch, const double* d_w, double* d_h);
int launch_contact_counts(sc_ctx* ctx, const double* d_coord, int64_t n, const sc_ff_desc& ff,
                          const PatchDev* patch, int64_t* d_counts);
// d_offsets: exclusive scan of counts (N+1 entries, last = k)
int launch_pair_fill(sc_ctx* ctx, const double* d_coord, int64_t n, const sc_ff_desc& ff,
                     const PatchDev* patch, const int64_t* d_offsets, int64_t* d_pairs,
                     double* d_sqdist);
int launch_exclusive_scan_i64(sc_ctx* ctx, const int64_t* d_in, int64_t n, int64_t* d_out);
int launch_kirchhoff_from_pairs(sc_ctx* ctx, int64_t n, const int64_t* d_pairs, int64_t k,
                                const double* d_gamma, double* d_k);
int launch_hessian_from_pairs(sc_ctx* ctx, const double* d_coord, int64_t n,
                              const int64_t* d_pairs, int64_t k, const double* d_gamma,
                              double* d_h);
// Ragged / decorated batches (sc_batch_plan, api_plan.hip): records of one structure each, opaque outside assembly.hip.
size_t asm_item_bytes();
// ff_dev: descriptor whose .tab (if any) holds DEVICE pointers; patch: device tables (empty tables when unpatched)
void asm_item_fill(void* dst, long long atom_off, int n, int ld, const sc_ff_desc& ff_dev, const PatchDev& patch);
// d_items: `count` records in device memory.  Writes (count, ld, ld) matrices: the structure's matrix in the leading
// dim * n rows / columns of its slot, the rest padded (see k_pad_fill).  d_bound_bits: count uint64 of scratch.
int launch_assemble_items(sc_ctx* ctx, int dim, const void* d_items, int64_t count, int max_atoms, bool any_patch,
                          bool any_pad, const double* d_coord, const double* d_w, double* d_matrix,
                          unsigned long long* d_bound_bits);
// Host-callback force fields for a whole plan (sc_batch_plan_contacts / _pairs / _fill_from_pairs_f64): contact counts of
// all atoms back to back; ordered pair lists (local indices) behind the exclusive scan of those counts; all slots from
// pairs + gamma.
int launch_items_counts(sc_ctx* ctx, const void* d_items, int64_t count, int max_atoms, bool any_patch,
                        const double* d_coord, int64_t* d_counts);
int launch_items_pair_fill(sc_ctx* ctx, const void* d_items, int64_t count, int max_atoms, bool any_patch,
                           const double* d_coord, const int64_t* d_offsets, int64_t* d_pairs, double* d_sqdist);
int launch_items_from_pairs(sc_ctx* ctx, int dim, const void* d_items, int64_t count, int max_atoms, int64_t order,
                            bool any_pad, const double* d_coord, const int64_t* d_pair_off, int64_t k_total,
                            const int64_t* d_pairs, const double* d_gamma, const double* d_w, double* d_matrix,
                            unsigned long long* d_bound_bits);
// In-place transpose-free symmetric "row-major == column-major" note: the eigensolver reads the
// LOWER triangle in column-major order, i.e. the UPPER triangle of the row-major matrix the
// assembly writes; the matrices are symmetric so both views agree.

struct RaggedRec;   // (ragged batches, below)

// ---- eigensolver (eigh.hip and friends) ----------------------------------------------------
// d_a: (batch, n, n) symmetric (destroyed), d_w: (batch, n), d_v: nullptr or (batch, n, n) rows = modes.
// eigh_batched synchronises the stream and returns this solve's errors (host-pointer entry points); the _async form only
// enqueues: non-finite input / a QL failure then surface through sc_deferred_status at the next synchronising call.
int eigh_batched(sc_ctx* ctx, double* d_a, int64_t n, int64_t batch, double* d_w, double* d_v);
int eigh_batched_async(sc_ctx* ctx, double* d_a, int64_t n, int64_t batch, double* d_w, double* d_v);
size_t eigh_workspace_bytes(int64_t n, int64_t batch, bool want_vectors);
// Partial spectrum: eigenvalues il..iu (0-based, inclusive): d_w (batch, m), d_v nullptr or (batch, m, n).
int eigh_range_batched(sc_ctx* ctx, double* d_a, int64_t n, int64_t batch, int64_t il, int64_t iu,
                       double* d_w, double* d_v);
int eigh_range_batched_async(sc_ctx* ctx, double* d_a, int64_t n, int64_t batch, int64_t il, int64_t iu,
                             double* d_w, double* d_v);
// Eigenvalue window (vl, vu] (scipy's subset_by_value): K slots per matrix, d_w (batch, K), d_v nullptr or (batch, K, n),
// d_count (batch) int64 true counts (may be nullptr); a slot holds the window's first min(count, K) eigenpairs, then NaN /
// zero rows.  Only enqueues.
// d_own: null, or one record per matrix: only the first own eigenvalues of matrix b count and its slot starts at
// min(il, own - K) (padded slots of a ragged batch).
int eigh_window_batched_async(sc_ctx* ctx, double* d_a, int64_t n, int64_t batch, double vl, double vu, int64_t K,
                              double* d_w, double* d_v, int64_t* d_count, const RaggedRec* d_own = nullptr);
// One matrix, synchronising: *m eigenpairs of the window into ctx->win_ws (*d_w (m), *d_v (m, n) or nullptr).
int eigh_window(sc_ctx* ctx, double* d_a, int64_t n, double vl, double vu, bool vectors, int64_t* m, double** d_w,
                double** d_v);
// Hermitian pseudo-inverse of the (n,n) matrix d_a (destroyed) into d_out, numpy.linalg.pinv(hermitian=True) rule.
int pinvh_device(sc_ctx* ctx, double* d_a, int64_t n, double rcond, double* d_out);

// ---- perturbation response scanning on one model's device-resident eigenpairs (consumers.hip) -------------------
// (its msf / dcc / tensors / overlaps are the batch consumers below with a batch of one)
size_t prs_scratch_bytes(int64_t n);
int modes_prs_device(sc_ctx* ctx, const double* d_v, const double* d_w, int64_t n, double rcond, int norm,
                     char* scratch, double* d_out);

// ---- the same quantities for a batch, on the solver's own (w, v, counts) tensors (batch_consumers.hip) ----------
// what: 0 = msf, 1 = dcc, 2 = anisotropic tensors (dim 3), 4 = distance fluctuations (dim 3; dist_fluct.hip), 5 = response, 6 = combine (mode_response.hip), 7 = perturbation-response scanning (dim 3; mode_prs.hip), 8 = generalized correlation (dim 3; mode_lmi.hip).  n_sel: weighted rows per structure (batch_modes_nsel).  budget: bytes the partial sums (msf) /
// the packed GEMM operands (dcc) may take, 0 = modes_budget_default().  ragged: null for a uniform batch (d_out (batch,
// m / dim[, m / dim])), or the plan's records: m is then the slot order and d_out is packed.
// Ragged batches (sc_batch_plan): one record per structure in the plan's device blob, read by the window count and the
// consumers.  own = dim * n_atoms rows / columns of the slot are the structure's, the rest is padding; atom_off / sq_off
// are the structure's places in packed (sum n) and (sum n^2) outputs.
struct RaggedRec {
  int own, n_atoms;
  long long atom_off, sq_off;
};
// d_rec: device records; first_row: global mode index of row 0 of (w, v) (lo of an index-range solve, else 0)
struct RaggedView {
  const RaggedRec* d_rec;
  int first_row, max_atoms;
  int64_t total_atoms, total_sq;
};
size_t modes_budget_default();
int64_t batch_modes_nsel(const sc_mode_selection& sel, int64_t nvec);
size_t batch_modes_workspace_bytes(int64_t m, int64_t nvec, int64_t batch, int dim, int64_t n_sel, int what,
                                   size_t budget, const RaggedView* ragged = nullptr);
int batch_msf_device(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch, int dim,
                     const sc_mode_selection& sel, const int64_t* d_counts, size_t budget, double* d_out,
                     const RaggedView* ragged = nullptr);
int batch_dcc_device(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch, int dim,
                     const sc_mode_selection& sel, const int64_t* d_counts, int norm, size_t budget, double* d_out,
                     const RaggedView* ragged = nullptr);
// dim 3 only: d_out (batch, m / 3, 6), six values per atom in ANISOU order; ragged: packed at 6 * atom_off.  chunk_rows: 0
// cuts the listed rows by msf_chunk; mode_lmi.hip passes its constant and reserves the workspace (what = 8) itself
int batch_aniso_device(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                       const sc_mode_selection& sel, const int64_t* d_counts, size_t budget, double* d_out,
                       const RaggedView* ragged = nullptr, int chunk_rows = 0);

// ---- fluctuations of the inter-atom distances (dist_fluct.hip) ----------------------------------------------------
// dim 3 only: d_out[b, a, c] = sum_r s[b, r] (n_ac . (u_r[c] - u_r[a]))^2, n_ac the unit vector from atom a to atom c of
// d_coord (batch, m / 3, 3), u_r[a] = d_atom_scale[b, a] (null: 1) times the atom's three components of row r.  Exactly
// symmetric, the diagonal exactly 0.  Ragged: coordinates and scales packed at atom_off, d_out packed at sq_off.
int batch_distfluct_device(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                           const sc_mode_selection& sel, const int64_t* d_counts, const double* d_coord,
                           const double* d_atom_scale, double* d_out, const RaggedView* ragged = nullptr);

// ---- perturbation-response scanning over the selected rows (mode_prs.hip) --------------------------------------------
// dim 3 only: d_out[b, a, c] = sum_{d, e} (sum_r s[b, r] u_r[a][d] u_r[c][e])^2, the sum of the squared entries of the 3 x 3
// covariance block (a, c), u_r[a] = d_atom_scale[b, a] (null: 1) times the atom's three components of row r; no covariance
// entry is written to memory.  Without norm exactly symmetric; norm != 0 divides row a by the original d_out[b, a, a].
// Ragged: the scale packed at atom_off, d_out packed at sq_off.  Enqueue only.
size_t modes_prs_diag_bytes(int64_t m, int64_t batch, const RaggedView* ragged);
int batch_prs_device(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                     const sc_mode_selection& sel, const int64_t* d_counts, const double* d_atom_scale, int norm,
                     double* d_out, const RaggedView* ragged = nullptr);

// ---- generalized correlation from the linear mutual information over the selected rows (mode_lmi.hip) -----------------
// dim 3 only: with C_ac = sum_r s[b, r] v_r[a] v_r[c]^T the 3 x 3 covariance block (a, c) and W_a the inverse Cholesky factor
// of C_aa (diagonal pivoting), delta = det(I - M M^T) of M = W_a C_ac W_c^T clamped to [0, 1]; d_out[b, a, c] = sqrt(1 - cbrt(delta)), or with
// information != 0 the mutual information -1/2 ln(delta) in nats.  Exactly symmetric; [a, a] is 1.0 / +inf by definition; an
// atom whose C_aa fails the pivot rule (mode_lmi.hip) has NaN in its row and column.  No covariance entry is written to
// memory.  Ragged: d_out packed at sq_off.  Enqueue only.
// Listed rows per chunk of the tensors that mode_lmi.hip whitens: a constant, so that a chunk's rows do not move when rows
// without weight follow (a ragged slot's pad rows): a structure's bits are the same in a uniform and in a ragged batch.
constexpr int kLmiTensorChunk = 128;
size_t modes_lmi_whiten_bytes(int64_t m, int64_t batch, const RaggedView* ragged);
int batch_lmi_device(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                     const sc_mode_selection& sel, const int64_t* d_counts, int information, double* d_out,
                     const RaggedView* ragged = nullptr);

// ---- pairwise comparison of mode subspaces (mode_subspace.hip) ---------------------------------------------------------
// One operand set: a uniform batch's (w, v, counts) with the selection of its rows.
struct SubspaceSet {
  const double* d_w;              // (batch, nvec)
  const double* d_v;              // (batch, nvec, m)
  const sc_mode_selection* sel;   // validated by the caller
  const int64_t* d_counts;        // null, or (batch) of a window solve
  int64_t nvec, batch;
};
// kind 0 (RMSIP) / 1 (covariance overlap): d_out (a.batch, b.batch) for every pair of a structure of `a` with one of `b`;
// b null: `a` with itself, only the pairs a >= b are computed and both places written from one value.  d_s: null or the raw
// S of the same shape; d_t_a / d_t_b: null or the sums of the weights per structure.  kind 2: d_out (n_pairs, nsel_a,
// nsel_b), the raw table G of the n_pairs listed (structure of a, structure of b) pairs, d_pairs int32 (n_pairs, 2) in
// device memory; a pair that names no structure gives NaN.  Workspace: ctx->modes_ws.  Enqueue only.
int modes_subspace_device(sc_ctx* ctx, const SubspaceSet& a, const SubspaceSet* b, int64_t m, int kind,
                          const int32_t* d_pairs, int64_t n_pairs, double* d_out, double* d_s, double* d_t_a,
                          double* d_t_b);

// ---- overlaps with displacement vectors and collectivities of the modes (mode_overlap.hip) -----------------------
// One pass over the rows of d_v (batch, nvec, m): d_overlap (batch, q, nout) and d_coll (batch, nout), either may be null
// (d_overlap only with q = 0).  Output row kk is row kk of v (d_rows null, nout = nvec) or row d_rows[kk] (a validated
// device list: one model's mode subset).  d_disp: (batch, q, m); ragged: (q, dim * sum n_atoms) packed, structure b's
// vector j at j * dim * sum n + dim * atom_off_b.  Rows behind counts[b] / a slot's own rows are NaN and are not read.
// No workspace; enqueue only.
int modes_overlap_device(sc_ctx* ctx, const double* d_v, int64_t m, int64_t nvec, int64_t batch, int dim,
                         const int* d_rows, int64_t nout, const double* d_disp, int64_t q, const int64_t* d_counts,
                         double* d_overlap, double* d_coll, const RaggedView* ragged = nullptr);

// ---- linear response and linear combinations of modes (mode_response.hip) ------------------------------------------
// Response: d_out[b, j] = S V_sel^T diag(wt) V_sel S f_j over the rows `sel` selects (wt = 1 / lambda from k_mode_weights,
// S = diag(d_atom_scale) per atom, null: 1), in mode space: one pass along the listed rows for the coefficients, one
// across them for the sum, per group of four forces; no covariance.  d_force and d_out (batch, q, m); ragged: (q, dim *
// sum n_atoms) packed, structure b's vector j at j * dim * sum n + dim * atom_off_b.  A row with weight 0.0 is not read.
// Combine: d_out[b, j] = S sum_kk d_coef[b, j, kk] v[b, row(kk)] over the nsel listed rows, row(kk) = d_rows[kk] (a
// validated device list: one model's mode subset) or kk (d_rows null, nsel = nvec): of those only the rows below
// min(counts[b], nvec) / a slot's own rows are read, and only their coefficients.  d_coef (batch, q, nsel).
// budget: bytes the partial sums may take at a time, 0 = modes_budget_default().  Enqueue only.
size_t modes_response_workspace_bytes(int64_t m, int64_t batch, int64_t nsel, int what, size_t budget);
int modes_response_device(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                          int dim, const sc_mode_selection& sel, const int64_t* d_counts, const double* d_force, int64_t q,
                          const double* d_atom_scale, size_t budget, double* d_out, const RaggedView* ragged = nullptr);
int modes_combine_device(sc_ctx* ctx, const double* d_v, int64_t m, int64_t nvec, int64_t batch, int dim,
                         const int* d_rows, int64_t nsel, const double* d_coef, int64_t q, const int64_t* d_counts,
                         const double* d_atom_scale, size_t budget, double* d_out, const RaggedView* ragged = nullptr);

// ---- rotation-translation blocks (rtb.hip) ---------------------------------------------------------------------------
// d_hb (nr, nr) = P^T H P from the ordered pair list, H as launch_hessian_from_pairs fills it times outer(s, s); d_order
// (k): the pairs sorted by (block of the second atom, block of the first), stable; d_seg_start (n_seg + 1): the segments of
// equal block pairs in that order; d_blk_start (n_blocks + 1): per block of the second atom, where its pairs start.  Every
// entry of d_hb is written.  No atomics, no workspace; enqueue only.
int launch_rtb_hessian(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, const int64_t* d_pairs, int64_t k,
                       const double* d_gamma, const double* d_ism, const double* d_P, const int32_t* d_boa,
                       const int64_t* d_offset, int64_t n_blocks, int64_t nr, const int64_t* d_order,
                       const int64_t* d_seg_start, int64_t n_seg, const int64_t* d_blk_start, double* d_hb);
// d_v (nvec, 3 n_atoms) = d_u (nvec, nr) P^T; every entry is written.  Enqueue only.
int launch_rtb_expand(sc_ctx* ctx, const double* d_u, int64_t nvec, int64_t nr, const double* d_P, const int32_t* d_boa,
                      const int64_t* d_offset, int64_t n_atoms, double* d_v);

// ---- conformational ensembles (superpose.hip, ensemble_pca.hip; the host decisions: ensemble_policy.h) ---------------------
// form: sc_host::kSuperposeFormLds (n_atoms <= kSuperposeLdsMaxAtoms) / kSuperposeFormStream; d_tc: 4 doubles of scratch (the
// target's centroid and the sum of the weights); d_out (M, N, 3) may be d_frames; d_rot (M, 3, 3), d_trans (M, 3) and d_rmsd
// (M) may be null.  Enqueue only.
int launch_superpose(sc_ctx* ctx, int form, const double* d_frames, int64_t n_frames, int64_t n_atoms,
                     const double* d_target, const double* d_weights, double* d_tc, double* d_out, double* d_rot,
                     double* d_trans, double* d_rmsd);
// d_mean (N, 3) and, unless null, d_msd (N) over the frames with the frame weights d_fw (M) or null; d_partial:
// mean_chunks(M) x 3 N doubles of scratch.  Enqueue only.
int launch_ensemble_mean(sc_ctx* ctx, const double* d_frames, int64_t n_frames, int64_t n_atoms, const double* d_fw,
                         double* d_partial, double* d_mean, double* d_msd);

// ---- the network as an operator on the pair list (pair_operator.hip) ------------------------------------------------
// Y = (T H T) x and E (per-atom deformation energies) for the q rows of d_x, H as launch_hessian_from_pairs /
// launch_kirchhoff_from_pairs fill it for symmetric constants: d_row_start (N + 1), atom i's pairs are the rows
// row_start[i] .. row_start[i + 1] - 1 of the list; d_y (q, dim N) or null, d_energy (q, N) or null, every entry written.
// One wavefront per atom, a fixed order of the sums.  No atomics, no workspace; enqueue only.
int launch_pairs_apply(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs, int64_t k,
                       const double* d_gamma, const int64_t* d_row_start, const double* d_atom_scale, const double* d_x,
                       int64_t q, double* d_y, double* d_energy);
// d_out (q, ks): the strain gamma_p e_p^2 of the listed pairs p = d_pair_idx[s]; NaN for an index outside 0 .. k - 1.
int launch_pairs_strain(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs, int64_t k,
                        const double* d_gamma, const double* d_atom_scale, const int64_t* d_pair_idx, int64_t ks,
                        const double* d_x, int64_t q, double* d_out);
// (pair_panel.hip) Z <- alpha (T H T) X + beta X + gamma_c Z on column panels (dim N, q) of leading dimension ld, the same
// matrix as launch_pairs_apply: one wavefront per (atom, 64 columns), lane = column, no sum across lanes.  Enqueue only.
int launch_pairs_panel(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs, int64_t k,
                       const double* d_gamma, const int64_t* d_row_start, const double* d_atom_scale, const double* d_x,
                       double* d_z, int64_t ld, int64_t q, double alpha, double beta, double gamma_c);

// (pair_cg.hip) Conjugate gradients on the same matrix for q columns at once; the state is seven rows of ld words (rho, stop,
// alpha, beta, status, iters, pq), the workspace pairs_cg_workspace_bytes(n_atoms, q).  init: X = 0, P = R, rho, stop, status;
// step: `iterations` iterations of five kernels each.  No atomics, no host synchronisation; enqueue only.
size_t pairs_cg_workspace_bytes(int64_t n_atoms, int64_t q);
int launch_pairs_cg_init(sc_ctx* ctx, int64_t n_atoms, int dim, double* d_x, const double* d_r, double* d_p, int64_t ld,
                         int64_t q, double tol, double* d_state, double* d_work);
int launch_pairs_cg_step(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs, int64_t k,
                         const double* d_gamma, const int64_t* d_row_start, const double* d_atom_scale, double* d_x,
                         double* d_r, double* d_p, double* d_q, int64_t ld, int64_t q, double* d_state, double* d_work,
                         int64_t iterations);

// Raises a kernel's dynamic LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) once per (device, kernel).  The
// attribute belongs to the device that is current when it is set: a function-local static done-flag (rounds 2-5) served
// the first device a process used and left contexts on a second GPU with refused launches.  Returns
// whether the limit is in place on the CURRENT device; the caller has made its context's device current.
inline bool sc_raise_dyn_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, bool> done;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  std::lock_guard<std::mutex> g(mu);
  const auto key = std::make_pair(dev, fn);
  const auto it = done.find(key);
  if (it != done.end()) return it->second;
  const bool ok = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
  done[key] = ok;
  return ok;
}
