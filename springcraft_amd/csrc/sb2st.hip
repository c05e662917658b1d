// Stage 2 of the two-stage tridiagonalisation (sb2st): band -> tridiagonal by Householder bulge chasing.  The band
// storage (k_band_extract, k_band_to_tri, k_sb_clean), the three forms of the chase (k_bulge_step: one launch per
// wavefront of tasks; k_bulge_chase: persistent, one sweep per workgroup; k_bulge_pair: persistent, two sweeps per
// workgroup) with the take-over k_chase_finish, their diagnostic stamps, the XCD probe and the host side: launch_chase,
// chase_stepwise and sb_stage2.
//
// Overview of the algorithm: twostage.hip; which form a chase gets: twostage_policy.h.
#include <algorithm>

#include "twostage_internal.h"

namespace {

// ---- XCDs of the device, counted by a probe launch (once per context): every workgroup ORs the bit of the XCC_ID it
// runs on into a mask.  8 x CUs workgroups of one wave: the dispatcher deals consecutive workgroups round-robin over
// the XCDs, so every XCD that exists is seen.  (num_cus / 32 holds for MI350 / MI355 and their partitions only.)
__global__ void k_xcd_probe(unsigned* mask) {
  unsigned id;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
  if (threadIdx.x == 0) atomicOr(mask, 1u << (id & 15u));
}
int probe_xcd_count(sc_ctx* ctx, hipStream_t st) {
  SC_TRY(sc_reserve_dc_aux(ctx, 256));
  unsigned* d_mask = reinterpret_cast<unsigned*>(ctx->dc_aux);
  SC_HIP(ctx, hipMemsetAsync(d_mask, 0, sizeof(unsigned), st));
  const int cus = ctx->num_cus > 0 ? ctx->num_cus : 256;
  hipLaunchKernelGGL(k_xcd_probe, dim3((unsigned)(8 * cus)), dim3(64), 0, st, d_mask);
  SC_HIP(ctx, hipGetLastError());
  unsigned h_mask = 0;
  SC_HIP(ctx, hipMemcpyAsync(&h_mask, d_mask, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  SC_HIP(ctx, hipStreamSynchronize(st));
  int count = 0, top = 0;
  for (int b = 0; b < 16; ++b)
    if (h_mask >> b & 1u) { ++count; top = b + 1; }
  // the kernels bind matrix b to XCD b mod nxcd by XCC_ID value: ids must be 0 .. count - 1 (they are on every part seen)
  ctx->nxcd = (count >= 1 && count == top) ? std::min(count, 8) : 1;
  return SC_OK;
}

// ================================================================================================================
// Band storage and stage 2
__global__ __launch_bounds__(256) void k_band_extract(const double* __restrict__ a_all, long long stride_a,
                                                      double* __restrict__ sb_all, SbLayout SL) {
  const int n = SL.n;
  const double* A = a_all + (size_t)blockIdx.y * stride_a;
  double* ab = sb_all + (size_t)blockIdx.y * SL.slab + SL.ab;
  const size_t total = (size_t)kLdab * n;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int d = (int)(idx % kLdab), jj = (int)(idx / kLdab);
    ab[idx] = (d <= kB && jj + d < n) ? A[(size_t)jj * n + jj + d] : 0.0;
  }
}

__global__ __launch_bounds__(256) void k_band_to_tri(const double* __restrict__ sb_all, SbLayout SL,
                                                     double* __restrict__ tri_all, TriLayout TL) {
  const int n = SL.n;
  const double* ab = sb_all + (size_t)blockIdx.y * SL.slab + SL.ab;
  double* tri = tri_all + (size_t)blockIdx.y * TL.slab;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    tri[TL.d + i] = ab[(size_t)i * kLdab];
    tri[TL.e + i] = i < n - 1 ? ab[(size_t)i * kLdab + 1] : 0.0;
  }
}

// After the band has been copied out: make the stage-1 reflectors a plain sub-matrix view of A for the block
// back-transformation (unit entry at row c + kB, zeros between the diagonal block and the unit entry).
__global__ __launch_bounds__(256) void k_sb_clean(double* __restrict__ a_all, long long stride_a, int n) {
  double* A = a_all + (size_t)blockIdx.y * stride_a;
  const int c = blockIdx.x;   // column
  for (int r = c + 1 + threadIdx.x; r <= std::min(c + kB, n - 1); r += 256) A[(size_t)c * n + r] = r == c + kB ? 1.0 : 0.0;
}

// Number of chase positions of sweep s: blocks of kB rows from row s+1 to n-1
using sc_host::chase_len;

// Diagnostic build (-DBULGE_STAMPS): shader cycles of wave 0 between five points of every task, summed over all tasks
// since the last read (sc_dbg_bulge_stamps, tools/bulge_stamps.py); no stamp executes in the normal build.
#ifdef BULGE_STAMPS
__device__ unsigned long long g_bulge_stamps[8];
#define BULGE_STAMP(var) unsigned long long var; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory");
#else
#define BULGE_STAMP(var)
#endif

typedef const double __attribute__((address_space(1)))* gdptr_c;
__device__ __forceinline__ double ld_l2(gdptr_c p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One task (sweep s, chase position k) of the bulge chase by one workgroup of 256 threads, blocks from and to the band
// storage: the body of k_bulge_step (one launch per wavefront of tasks) and of k_chase_finish (the take-over after a
// persistent chase that gave up).
struct BulgeTaskLds {
  double E[kB * (kB + 1)];
  double vp[kB], vn[kB], u[kB], red[4 * kB];
  double s_tau, s_beta;
};
__device__ __forceinline__ void bulge_task(double* __restrict__ sb, const SbLayout& SL, int s, int k, BulgeTaskLds& W) {
  constexpr int LD = kB + 1;
  double* const E = W.E;
  double* const D = E;   // the diagonal block is processed after E has gone back to memory: same buffer
  double* const vp = W.vp;
  double* const vn = W.vn;
  double* const u = W.u;
  double* const red = W.red;
  double& s_tau = W.s_tau;
  double& s_beta = W.s_beta;
  const int n = SL.n;
  double* ab = sb + SL.ab;
  const int S = s / kG, cc = s - S * kG;
  // diamonds of group S start at sum_{S' < S} chase_len(n, 64 S') = S K0 - S (S - 1) / 2  (K0 = chase_len(n, 0))
  const size_t dia = (size_t)S * chase_len(n, 0) - (size_t)S * (S - 1) / 2 + k;
  // diamonds are stored row-major (sweep index contiguous): element (row r, sweep c) at [c + r * kG]
  double* vd = sb + SL.vd + dia * kDiaSize + (size_t)cc * kG + cc;   // this reflector's first entry (row cc, column cc)
  const int tid = threadIdx.x;
  const int i = tid & 63, q = tid >> 6;

  const int r0 = s + 1 + k * kB;             // first row of the reflector being generated
  const int L = std::min(kB, n - r0);        // its length (>= 1)
  BULGE_STAMP(t0)

  // the diagonal block D = AB(r0 .. r0+L-1, r0 .. r0+L-1) (lower stored) is not touched before its own update:
  // fetch it right away (unconditional loads with clamped indices, masked when they go to LDS)
  // (one wave-uniform base per block + 32-bit element offsets instead of a 64-bit address per access)
  gdptr colbase = wave_uniform(ab + (size_t)r0 * kLdab);                    // AB(r0, r0)
  double d16[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int jc = std::min(q * 16 + u, L - 1);
    const int ic = std::min(std::max(i, jc), L - 1);
    d16[u] = colbase[(unsigned)((ic - jc) + jc * kLdab)];
  }

  if (k > 0) {
    gdptr ebase = wave_uniform(ab + (size_t)(r0 - kB) * kLdab);             // AB(r0 - kB, r0 - kB)
    const double* vdp = sb + SL.vd + (dia - 1) * kDiaSize + (size_t)cc * kG + cc;
    const double tau_p = sb[SL.tau2 + (dia - 1) * kG + cc];
    if (tid < kB) vp[tid] = vdp[(size_t)tid * kG];
    // E(i, j) = AB(r0 + i, c0 + j), rows i < L: thread (i, q) keeps row i, columns 16 q .. 16 q + 15 in registers for the
    // row-wise steps; only the column sums of the second reflector go through an LDS image.
    double t16[16];
    {
      const int ic = std::min(i, L - 1);
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int jj = q * 16 + u;
        t16[u] = ebase[(unsigned)((kB + ic - jj) + jj * kLdab)];
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) t16[u] = i < L ? t16[u] : 0.0;
    }
    lds_barrier();   // vp
#ifdef BULGE_STAMPS
    { BULGE_STAMP(t1) if (tid == 0) atomicAdd(&g_bulge_stamps[0], t1 - t0); }
#endif
    // u = tau_p E vp: partial sums over this wave's 16 columns, every thread adds the four partials of its own row
    {
      double a = 0.0;
#pragma unroll
      for (int u = 0; u < 16; ++u) a += t16[u] * vp[q * 16 + u];
      red[q * kB + i] = a;
    }
    lds_barrier();
    {
      const double ui = tau_p * ((red[i] + red[kB + i]) + (red[2 * kB + i] + red[3 * kB + i]));
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        t16[u] -= ui * vp[q * 16 + u];
        E[i * LD + q * 16 + u] = t16[u];
      }
    }
    // new reflector from the first column of E, which wave 0 holds in t16[0]
    if (q == 0) {
      const double x = t16[0];
      const double t2 = wave_sum((i >= 1 && i < L) ? x * x : 0.0);
      const HH h = householder(__shfl(x, 0), t2);
      vn[i] = i == 0 ? 1.0 : (i < L ? x * h.scale : 0.0);
      if (i == 0) { s_tau = h.tau; s_beta = h.beta; }
    }
    lds_barrier();
    // z_j = sum_i E[i, j] v_i  (j >= 1);  thread (j = i, rows q*16..)
    {
      double a = 0.0;
#pragma unroll
      for (int ii = q * 16; ii < q * 16 + 16; ++ii) a += E[ii * LD + i] * vn[ii];
      red[q * kB + i] = a;
    }
    lds_barrier();
    if (tid < kB) u[tid] = s_tau * ((red[tid] + red[kB + tid]) + (red[2 * kB + tid] + red[3 * kB + tid]));
    lds_barrier();
    // E <- H E (from the registers), first column = beta e1; write back.  Nobody reads the LDS image of E any more (the
    // column sums were two barriers ago), so the diagonal block may take over its buffer without another barrier.
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int jj = q * 16 + c;
      double e = t16[c] - vn[i] * u[jj];
      if (jj == 0) e = i == 0 ? s_beta : 0.0;
      if (i < L) ebase[(unsigned)((kB + i - jj) + jj * kLdab)] = e;
    }
#ifdef BULGE_STAMPS
    { BULGE_STAMP(t2) if (tid == 0) { atomicAdd(&g_bulge_stamps[1], t2 - t0); atomicAdd(&g_bulge_stamps[5], 1ull); } }
#endif
  } else {
    // sweep start: x = AB(s+1 .. s+L, s)
    if (tid < 64) {
      const double xr = ab[(size_t)(1 + std::min(tid, L - 1)) + (size_t)s * kLdab];
      const double x = tid < L ? xr : 0.0;
      const double t2 = wave_sum(tid >= 1 ? x * x : 0.0);
      const double alpha = __shfl(x, 0);
      const HH h = householder(alpha, t2);
      vn[tid] = tid == 0 ? 1.0 : x * h.scale;
      if (tid == 0) { s_tau = h.tau; s_beta = h.beta; }
      if (tid < L) ab[(size_t)(1 + tid) + (size_t)s * kLdab] = tid == 0 ? h.beta : 0.0;
    }
    lds_barrier();
  }

  // two-sided update of the diagonal block D = AB(r0 .. r0+L-1, r0 .. r0+L-1) (lower stored)
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int jj = q * 16 + u;
    if (i >= jj) {
      const double x = (i < L) ? d16[u] : 0.0;
      D[i * LD + jj] = x;
      D[jj * LD + i] = x;
    }
  }
  lds_barrier();
  BULGE_STAMP(t3)
  {
    double a = 0.0;
#pragma unroll
    for (int jj = q * 16; jj < q * 16 + 16; ++jj) a += D[i * LD + jj] * vn[jj];
    red[q * kB + i] = a;
  }
  lds_barrier();
  if (tid < 64) {
    const double p = s_tau * ((red[tid] + red[kB + tid]) + (red[2 * kB + tid] + red[3 * kB + tid]));
    const double dot = wave_sum(p * vn[tid]);
    const double alpha2 = -0.5 * s_tau * dot;
    u[tid] = p + alpha2 * vn[tid];   // w
  }
  lds_barrier();
  for (int jj = q * 16; jj < q * 16 + 16; ++jj)
    if (i >= jj && i < L)
      colbase[(unsigned)((i - jj) + jj * kLdab)] = D[i * LD + jj] - vn[i] * u[jj] - u[i] * vn[jj];

  // the reflector goes into its diamond
  if (tid < L) vd[(size_t)tid * kG] = vn[tid];
  if (tid == 0) sb[SL.tau2 + dia * kG + cc] = s_tau;
#ifdef BULGE_STAMPS
  {
    BULGE_STAMP(t4)
    if (tid == 0) {
      atomicAdd(&g_bulge_stamps[2], t3 - t0);
      atomicAdd(&g_bulge_stamps[3], t4 - t0);
      atomicAdd(&g_bulge_stamps[4], 1ull);
    }
  }
#endif
}

// Launch t of the bulge chase: workgroup x handles task (s, k) with k = (t & 1) + 2x, s = (t - k) / 2.
__global__ __launch_bounds__(256, 4) void k_bulge_step(double* __restrict__ sb_all, SbLayout SL,
                                                    int t, const int* __restrict__ done = nullptr) {
  __shared__ BulgeTaskLds W;
  const int n = SL.n;
  const int k = (t & 1) + 2 * (int)blockIdx.x;
  const int s = (t - k) / 2;
  if (s < 0 || s > n - 3 || k >= chase_len(n, s)) return;
  // resuming a persistent chase that gave up (k_bulge_chase): done[b][s] tasks of sweep s are finished already
  if (done && k < done[(size_t)blockIdx.y * n + s]) return;
  bulge_task(sb_all + (size_t)blockIdx.y * SL.slab, SL, s, k, W);
}

// Take-over after a persistent chase (k_bulge_chase / k_bulge_pair), enqueued behind every one of them so that the host
// never has to look at the chase's outcome inside a solve (round 6: the solve only enqueues).  A chase that completed
// -- always, in practice -- costs this launch a look at the control block.  Otherwise (the stop flag is up: a wait ran
// into its bound or the test hook fired; or an XCD that owns matrices received no workgroup) workgroup b finishes matrix
// b alone, task after task in the order sweep, position from the published counts -- a valid order of the chase's
// dependences whatever the state the workgroups left behind, and slow: it is the last line of defence, counted in
// stats[] (read at the next synchronising call: sc_collect_events), after which the context keeps to the per-wavefront
// launches.  stats (unsigned long long, sc_ctx::d_status): [2] chases that needed it, [3] of those: stop flag raised by a
// time-out (not by the test hook), [4] sweeps finished by the persistent kernels (all chases), [6] incomplete without a flag.
__global__ __launch_bounds__(256) void k_chase_finish(double* __restrict__ sb_all, SbLayout SL, int batch, int nxcd,
                                                      int* __restrict__ progress, const int* __restrict__ ctl,
                                                      unsigned long long* __restrict__ stats) {
  __shared__ BulgeTaskLds W;
  const int n = SL.n;
  const int b = blockIdx.x;
  long long sweeps = 0;
  for (int x = 0; x < 8; ++x) sweeps += ctl[16 + x];
  const bool complete = ctl[0] == 0 && sweeps == (long long)batch * (n - 2);
  if (b == 0 && threadIdx.x == 0) {
    atomicAdd(stats + 4, (unsigned long long)sweeps);
    if (!complete) {
      atomicAdd(stats + 2, 1ull);
      if (ctl[0] && ctl[1] == 0) atomicAdd(stats + 3, 1ull);
      if (!ctl[0]) atomicAdd(stats + 6, 1ull);
    }
  }
  if (complete) return;
  int* prog = progress + (size_t)b * n;
  double* sb = sb_all + (size_t)b * SL.slab;
  for (int s = 0; s <= n - 3; ++s) {
    const int len = chase_len(n, s);
    for (int k = prog[s]; k < len; ++k) {
      bulge_task(sb, SL, s, k, W);
      __syncthreads();   // (the task's stores are visible to this workgroup's next task: same CU, same L1 / L2 path)
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------
// Persistent form of the bulge chase: ONE launch, no launch per wavefront.  A workgroup CLAIMS the next unclaimed sweep
// of a matrix (an atomic counter per matrix) and walks it down the band, task after task; task (s, k) starts when sweep
// s - 1 has published k + 2 finished tasks (progress[b][s - 1], one counter per sweep), which is the only dependence
// the chase has.  The previous reflector of the sweep stays in LDS (no round trip through the diamond storage), a sweep
// never waits for a launch boundary, and the matrices drift apart freely, so no round of workgroups is left half empty.
//
// Forward progress by construction: sweeps are claimed in order by workgroups that are running, so the owner of sweep
// s - 1 is always running or finished when somebody waits for it -- whatever the number of resident workgroups and
// however the dispatcher spreads them over the XCDs.  (Round 2 gave workgroup r of W the sweeps r, r + W, ... statically;
// a role that was not resident orphaned its sweeps and the successor spun into its bound.)  No cooperative launch and no
// placement census is needed any more.
//
// Coherence without L2 write-backs: all workgroups of a matrix sit on ONE XCD (matrix b on XCD b mod 8; a workgroup
// reads the XCD it runs on from XCC_ID and only ever touches that XCD's matrices, their claim counters and progress
// counters), i.e. behind one L2.  A task's stores are drained (vmcnt(0)) and fenced by a workgroup barrier before thread
// 0 publishes the counter; consumers read the counter and the band through agent-scope relaxed atomic loads, which
// bypass the CU's L1 and are served by that L2 (26 us per hand-off with release / acquire at agent scope, 3 us this way:
// tools/probe_handoff.hip).  A workgroup starts on its "home" matrix (ticket mod matrices of the XCD) and moves on to
// the XCD's other matrices when that one has no unclaimed sweep left, so every matrix of an XCD is finished as long as
// ONE workgroup lands there.  Every spin is bounded as a last line of defence: a time-out raises a flag that ends all
// workgroups between tasks; the host counts it (sc_ctx_get_counter "chase_timeouts"), finishes the chase with the
// per-wavefront launches from the published counters and does not use the persistent form on that context again.
//
// ctl (ints): [0] time-out flag, [1] workgroup-local tasks after which the test hook raised it, [2..9] tickets drawn
// per XCD, [10..12] (matrix, sweep, task) of the wait that timed out, [16..23] sweeps finished per XCD (kChaseCtlInts
// ints: sc_ctx::d_chase_ctl).

// Early hand-off (round 4).  Task (s, k) reads three things from sweep s - 1: the blocks task (s - 1, k) has left --
// all its rows but the last --, and from task (s - 1, k + 1) its last row: the entry beta (what remains of the column that
// task annihilated) in the off-diagonal block and the row of the diagonal block.  The right update of the off-diagonal
// block and the new reflector only need beta, which task (s - 1, k + 1) knows as soon as it has generated ITS reflector --
// two thirds of a task before its stores have drained.  So a task publishes (beta, position) in a 16-byte record right
// there, its successor in the next sweep starts when task (s - 1, k) is complete and that record is in, loads its blocks
// and runs the first half of its work, and only then waits for (s - 1, k + 1) to be complete, fetches the last row of its
// diagonal block, and stores.  Nothing is stored before that second wait, so the order of the writes to the band is the
// one of the plain dependence.  The dependent chain of a latency-bound chase -- one task per link -- shortens by the
// loads and the first half of the arithmetic (profiles/r04_bulge_sweep.txt).
// Records: a ring of kEarlyRing per sweep, slot k mod kEarlyRing holds {beta of task k, k + 1}; written and read as ONE
// 16-byte access.  A reader that finds a later tag knows that its task (s - 1, k + 1) is long complete and takes the
// entry from the band instead.
constexpr int kEarlyRing = sc_host::kEarlyRing;
__device__ __forceinline__ void st16(void* p, v4i v) { asm volatile("global_store_dwordx4 %0, %1, off" ::"v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ void st16_sc1(void* p, v4i v) { asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory"); }
// a band entry as the chase's workgroups hand it on.  SPREAD = 0: all workgroups of a matrix sit behind ONE L2, a plain
// store (drained before the counter moves) is what the consumer's sc1 load finds there.  SPREAD = 1 (round 6: one large
// matrix chased from every XCD): a write-through store at agent scope, which a consumer on another XCD reads from memory
// with its sc1 load -- the pair MI355X_MICROARCH.md lists as valid without any fence (k_panel_coop's records use it too)
template <int SPREAD>
__device__ __forceinline__ void st_band(gdptr p, double v) {
  if (SPREAD) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}
__device__ __forceinline__ v4i ld16_l2(const void* p) {
  v4i r;
  asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(r) : "v"(p) : "memory");
  return r;
}

// Diagnostic build (-DCHASE_STAMPS): shader cycles of every wave of k_bulge_chase between ten points of a task, summed over
// all tasks of all workgroups (sc_dbg_chase_stamps, tools/chase_stamps.py): [1] wait for the predecessor sweep (poll +
// barrier), [2] loads of both blocks + first products up to the first barrier, [3] right update of E + the new reflector,
// [4] column sums + u, [5] second wait (early hand-off), [6] E stores issued + D into LDS, [7] D products, [8] w, [9] D update
// + stores issued, [10] store drain + barrier, [11] publish; [15] = waves x tasks.  Tasks at k = 0 have no E block: their
// segments [2] .. [4] are the reflector of the column alone.
#ifdef CHASE_STAMPS
__device__ unsigned long long g_chase_stamps[16];
#define CHASE_STAMP_DECL unsigned long long cs_prev = 0, cs_n = 0, cs_sum[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define CHASE_STAMP(i)                                                                 \
  {                                                                                    \
    unsigned long long t_;                                                             \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");        \
    if ((i) != 0) cs_sum[i] += t_ - cs_prev;                                           \
    cs_prev = t_;                                                                      \
  }
#define CHASE_STAMP_WRITE                                                                          \
  if ((threadIdx.x & 63) == 0) {                                                                   \
    for (int i_ = 1; i_ < 12; ++i_) atomicAdd(&g_chase_stamps[i_], cs_sum[i_]);                    \
    atomicAdd(&g_chase_stamps[15], cs_n);                                                          \
  }
#else
#define CHASE_STAMP_DECL
#define CHASE_STAMP(i)
#define CHASE_STAMP_WRITE
#endif
// SPREAD = 1 (round 6): the workgroups of ONE matrix on all XCDs -- the launch passes nxcd = 1, so every workgroup
// counts as "XCD 0" and serves every matrix; band stores and the early records are written through at agent scope
// (st_band).  For a few large matrices (config C5: one n = 24000 matrix has ~188 tasks per wavefront, three times the
// workgroups one XCD holds): until round 5 those took one launch per wavefront (48 000 launches of 8.7 us).
template <int SPREAD>
__global__ __launch_bounds__(256, 2) void k_bulge_chase(double* __restrict__ sb_all, SbLayout SL, int batch, int W, int nxcd,
                                                     int* __restrict__ progress, int* __restrict__ next_sweep,
                                                     int* __restrict__ ctl, int give_up_after, v4i* __restrict__ early) {
  constexpr int LD = kB + 1;
  __shared__ double E[kB * LD];
  double* D = E;
  __shared__ double vbuf[2][kB], u[kB], red[4 * kB];
  __shared__ double s_tau, s_beta, s_beta_in;
  __shared__ int s_go, s_claim, s_mode;

  const int n = SL.n;
  const int tid = threadIdx.x;
  const int i = tid & 63, q = tid >> 6;
  __shared__ int s_xcd, s_slot;
  if (tid == 0) {
    unsigned id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
    s_xcd = (int)(id & 7u) % nxcd;
    s_slot = atomicAdd(ctl + 2 + s_xcd, 1);
  }
  __syncthreads();
  const int xcd = s_xcd, slot = s_slot;
  const int mpx = xcd < batch ? (batch - xcd + nxcd - 1) / nxcd : 0;   // matrices of this XCD: xcd, xcd + nxcd, ...
  if (mpx == 0 || slot >= mpx * W) return;                      // no more than W workgroups per matrix
  const int K0 = chase_len(n, 0);
  int tasks_left = give_up_after;

  CHASE_STAMP_DECL
  int cur = slot % mpx, exhausted = 0;
  while (exhausted < mpx) {
    const int b = xcd + nxcd * cur;
    int* prog = progress + (size_t)b * n;
    // ---- claim the next sweep of matrix b (the counter is only ever touched from this XCD)
    if (tid == 0) s_claim = atomicAdd(next_sweep + b, 1);
    __syncthreads();
    const int s = __builtin_amdgcn_readfirstlane(s_claim);
    __syncthreads();
    if (s > n - 3) {
      ++exhausted;
      cur = cur + 1 < mpx ? cur + 1 : 0;
      continue;
    }
    exhausted = 0;
    double* sb = sb_all + (size_t)b * SL.slab;
    double* ab = sb + SL.ab;
    {
      const int len = chase_len(n, s);
      const int S = s / kG, cc = s - S * kG;
      const size_t dia0 = (size_t)S * K0 - (size_t)S * (S - 1) / 2;
      const int len_prev = s > 0 ? chase_len(n, s - 1) : 0;
      double tau_p = 0.0;
      for (int k = 0; k < len; ++k) {
        double* vp = vbuf[(k + 1) & 1];   // reflector of task k - 1 of this sweep
        double* vn = vbuf[k & 1];
        // ---- wait for sweep s - 1.  With a task (s - 1, k + 1) to wait for (early hand-off, see above): task (s - 1, k)
        // complete AND either (s - 1, k + 1) complete too (mode 2: everything is in the band) or its record in (mode 1:
        // beta from the record, the last row of the diagonal block after the second wait).  Else (mode 0): all of sweep
        // s - 1 that touches these rows is complete.
        const bool early_task = early != nullptr && s > 0 && k + 1 < len_prev;
        CHASE_STAMP(0)
        if (tid == 0) {
          // (the stop flag and the predecessor's progress are requested TOGETHER: one L2 round trip, ~0.7 us, per task on
          // the sweep-to-sweep critical path instead of two; while waiting, the flag is looked at every 16th poll only)
          const int need = s > 0 ? min(k + (early_task ? 1 : 2), len_prev) : 0;
          const int stop0 = __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          int have = s > 0 ? __hip_atomic_load(prog + s - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
          int go = stop0 ? 0 : 1;
          int mode = 0;
          double beta_in = 0.0;
          const v4i* rec = early_task ? early + ((size_t)b * n + s - 1) * kEarlyRing + ((k + 1) & (kEarlyRing - 1)) : nullptr;
          long spins = 0;
          while (go) {
            if (have >= need) {
              if (!early_task) break;
              if (have >= k + 2) { mode = 2; break; }
              const v4i r = ld16_l2(rec);
              if (r.z == k + 2) {
                mode = 1;
                beta_in = __longlong_as_double((long long)(((unsigned long long)(unsigned)r.y << 32) | (unsigned)r.x));
                break;
              }
            }
            // (2^21 polls of ~1 us: seconds, orders of magnitude above any wait for a running workgroup)
            ++spins;
            if (spins > (1L << 21) ||
                ((spins & 15) == 0 && __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
              if (!__hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                ctl[10] = b; ctl[11] = s; ctl[12] = k;
              }
              __hip_atomic_store(ctl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              go = 0;
              break;
            }
            __builtin_amdgcn_s_sleep(1);
            have = __hip_atomic_load(prog + s - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          s_go = go;
          s_mode = mode;
          s_beta_in = beta_in;
        }
        __syncthreads();
        if (!s_go) return;
        CHASE_STAMP(1)
        const int mode = s_mode;   // 1: the last row of both blocks is not in the band yet
        // second wait of a task that started on the record (mode 1): task (s - 1, k + 1) complete, then the last row of
        // the diagonal block.  Nothing of this task has been stored before.
#define CHASE_SECOND_WAIT()                                                                                       \
        if (mode == 1) {                                                                                          \
          if (tid == 0) {                                                                                         \
            int go = 1;                                                                                           \
            long spins = 0;                                                                                       \
            while (__hip_atomic_load(prog + s - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < k + 2) {         \
              ++spins;                                                                                            \
              if (spins > (1L << 21) ||                                                                           \
                  ((spins & 15) == 0 && __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {    \
                if (!__hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {                        \
                  ctl[10] = b; ctl[11] = s; ctl[12] = k;                                                          \
                }                                                                                                 \
                __hip_atomic_store(ctl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                           \
                go = 0;                                                                                           \
                break;                                                                                            \
              }                                                                                                   \
              __builtin_amdgcn_s_sleep(1);                                                                        \
            }                                                                                                     \
            s_go = go;                                                                                            \
          }                                                                                                       \
          __syncthreads();                                                                                        \
          if (!s_go) return;                                                                                      \
        }

        const int r0 = s + 1 + k * kB;
        const int L = min(kB, n - r0);
        const size_t dia = dia0 + k;
        double* vd = sb + SL.vd + dia * kDiaSize + (size_t)cc * kG + cc;
        // (one wave-uniform base per block + 32-bit element offsets: a 64-bit pointer per access costs the kernel a
        // workgroup per CU in registers)
        gdptr colbase_k = wave_uniform(ab + (size_t)r0 * kLdab);                 // AB(r0, r0)
        double d16[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) {
          const int jc = min(q * 16 + c, L - 1);
          const int ic = min(max(i, jc), L - 1);
          d16[c] = ld_l2(colbase_k + (unsigned)((ic - jc) + jc * kLdab));
        }
        if (k > 0) {
          gdptr ebase_k = wave_uniform(ab + (size_t)(r0 - kB) * kLdab);          // AB(r0 - kB, r0 - kB)
          double t16[16];
          {
            const int ic = min(i, L - 1);
#pragma unroll
            for (int c = 0; c < 16; ++c) {
              const int jj = q * 16 + c;
              t16[c] = ld_l2(ebase_k + (unsigned)((kB + ic - jj) + jj * kLdab));
            }
#pragma unroll
            for (int c = 0; c < 16; ++c) t16[c] = i < L ? t16[c] : 0.0;
            if (mode == 1 && i == kB - 1) {   // the last row: zeros and the predecessor's beta (the band still holds the old entry)
              const double bin = s_beta_in;
#pragma unroll
              for (int c = 0; c < 16; ++c) t16[c] = q * 16 + c == kB - 1 ? bin : 0.0;
            }
          }
          {
            double a = 0.0;
#pragma unroll
            for (int c = 0; c < 16; ++c) a += t16[c] * vp[q * 16 + c];
            red[q * kB + i] = a;
          }
          lds_barrier();
          CHASE_STAMP(2)
          {
            const double ui = tau_p * ((red[i] + red[kB + i]) + (red[2 * kB + i] + red[3 * kB + i]));
#pragma unroll
            for (int c = 0; c < 16; ++c) {
              t16[c] -= ui * vp[q * 16 + c];
              E[i * LD + q * 16 + c] = t16[c];
            }
          }
          if (q == 0) {
            const double x = t16[0];
            const double t2 = wave_sum((i >= 1 && i < L) ? x * x : 0.0);
            const HH h = householder(__shfl(x, 0), t2);
            vn[i] = i == 0 ? 1.0 : (i < L ? x * h.scale : 0.0);
            if (i == 0) {
              s_tau = h.tau; s_beta = h.beta;
              if (early) {   // the record of this task: all its successor in sweep s + 1 needs to start on
                const unsigned long long bb = (unsigned long long)__double_as_longlong(h.beta);
                if (SPREAD) st16_sc1(early + ((size_t)b * n + s) * kEarlyRing + (k & (kEarlyRing - 1)), v4i{(int)(unsigned)bb, (int)(unsigned)(bb >> 32), k + 1, 0});
                else st16(early + ((size_t)b * n + s) * kEarlyRing + (k & (kEarlyRing - 1)), v4i{(int)(unsigned)bb, (int)(unsigned)(bb >> 32), k + 1, 0});
              }
            }
          }
          lds_barrier();
          CHASE_STAMP(3)
          {
            double a = 0.0;
#pragma unroll
            for (int ii = q * 16; ii < q * 16 + 16; ++ii) a += E[ii * LD + i] * vn[ii];
            red[q * kB + i] = a;
          }
          lds_barrier();
          if (tid < kB) u[tid] = s_tau * ((red[tid] + red[kB + tid]) + (red[2 * kB + tid] + red[3 * kB + tid]));
          lds_barrier();
          CHASE_STAMP(4)
          CHASE_SECOND_WAIT()
          CHASE_STAMP(5)
#pragma unroll
          for (int c = 0; c < 16; ++c) {
            const int jj = q * 16 + c;
            double e = t16[c] - vn[i] * u[jj];
            if (jj == 0) e = i == 0 ? s_beta : 0.0;
            if (i < L) st_band<SPREAD>(ebase_k + (unsigned)((kB + i - jj) + jj * kLdab), e);
          }
        } else {
          gdptr col_s = wave_uniform(ab + (size_t)s * kLdab);
          if (tid < 64) {
            const double xr = ld_l2(col_s + (unsigned)(1 + min(tid, L - 1)));
            double x = tid < L ? xr : 0.0;
            if (mode == 1 && tid == kB - 1) x = s_beta_in;   // (its last entry is task (s - 1, 1)'s beta)
            const double t2 = wave_sum(tid >= 1 ? x * x : 0.0);
            const HH h = householder(__shfl(x, 0), t2);
            vn[tid] = tid == 0 ? 1.0 : x * h.scale;
            if (tid == 0) { s_tau = h.tau; s_beta = h.beta; }
          }
          lds_barrier();
          CHASE_STAMP(4)
          CHASE_SECOND_WAIT()
          CHASE_STAMP(5)
          if (tid < L) st_band<SPREAD>(col_s + (unsigned)(1 + tid), tid == 0 ? s_beta : 0.0);
        }
#undef CHASE_SECOND_WAIT
        // ---- diagonal block (after the second wait its last row is in the band)
        if (mode == 1 && i == kB - 1) {
#pragma unroll
          for (int c = 0; c < 16; ++c) {
            const int jc = q * 16 + c;
            d16[c] = ld_l2(colbase_k + (unsigned)((kB - 1 - jc) + jc * kLdab));
          }
        }
#pragma unroll
        for (int c = 0; c < 16; ++c) {
          const int jj = q * 16 + c;
          if (i >= jj) {
            const double x = (i < L) ? d16[c] : 0.0;
            D[i * LD + jj] = x;
            D[jj * LD + i] = x;
          }
        }
        lds_barrier();
        CHASE_STAMP(6)
        {
          double a = 0.0;
#pragma unroll
          for (int jj = q * 16; jj < q * 16 + 16; ++jj) a += D[i * LD + jj] * vn[jj];
          red[q * kB + i] = a;
        }
        lds_barrier();
        CHASE_STAMP(7)
        const double tau_now = s_tau;
        if (tid < 64) {
          const double pp = tau_now * ((red[tid] + red[kB + tid]) + (red[2 * kB + tid] + red[3 * kB + tid]));
          const double dot = wave_sum(pp * vn[tid]);
          u[tid] = pp - 0.5 * tau_now * dot * vn[tid];
        }
        lds_barrier();
        CHASE_STAMP(8)
        for (int jj = q * 16; jj < q * 16 + 16; ++jj)
          if (i >= jj && i < L)
            st_band<SPREAD>(colbase_k + (unsigned)((i - jj) + jj * kLdab), D[i * LD + jj] - vn[i] * u[jj] - u[i] * vn[jj]);
        if (tid < L) vd[(size_t)tid * kG] = vn[tid];
        if (tid == 0) sb[SL.tau2 + dia * kG + cc] = tau_now;
        tau_p = tau_now;
        // ---- publish: this task's stores are in the L2 before the counter moves
        CHASE_STAMP(9)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        CHASE_STAMP(10)
        if (tid == 0) {
          __hip_atomic_store(prog + s, k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (k + 1 == len) atomicAdd(ctl + 16 + xcd, 1);
          // test hook (sc_dbg_set_chase): raise the time-out flag after that many tasks of this workgroup
          if (give_up_after > 0 && --tasks_left == 0) {
            ctl[1] = give_up_after;
            __hip_atomic_store(ctl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
        CHASE_STAMP(11)
#ifdef CHASE_STAMPS
        ++cs_n;
#endif
      }
    }
  }
  CHASE_STAMP_WRITE
}

// ----------------------------------------------------------------------------------------------------------------
// Pair form of the persistent chase (round 4): ONE workgroup walks TWO consecutive sweeps down the band.
//
// Why: every byte a task stores leaves the XCD's L2 (the L2 writes through), so the chase moves 96 KB of HBM traffic
// per task whatever the cache does -- 1.75 TB per 64 x n = 6000 step, the floor of both older forms -- and every
// hand-off between sweeps goes through memory.  Sweep s + 1 touches, two tasks later, the very blocks sweep s has just
// left (shifted by one row and one column).  Here team A (threads 0..255) runs the tasks of sweep sA = 2 p and leaves
// its blocks in LDS; team B (threads 256..511) runs sweep sB = sA + 1 two positions behind and takes its blocks from
// there: per PAIR of tasks one block set is read from memory (A) and one is written (B) -- half the traffic -- and the
// A -> B hand-off costs a workgroup barrier instead of store drain + publish + poll + L2 loads.
//
// LDS: a ring of three position slots (E 64 x 65 + D packed lower, 49 920 B each): at step m, A works on position m
// (slot m % 3), B on position m - 2, position m - 1 waits.  B's block at position k is A's block shifted by (1, 1):
//   E'(i, j) = E_k(i + 1, j + 1),  E'(i, 63) = D_k(i + 1, 0),  E'(63, 63) = E_{k+1}(0, 0),  E'(63, j < 63) = 0
//   D'(i, j) = D_k(i + 1, j + 1),  D'(63, j) = E_{k+1}(0, j + 1),  D'(63, 63) = D_{k+1}(0, 0)
// so every element A leaves behind is consumed by exactly one task of B -- except the entries A has just annihilated
// (E_k(1.., 0)), which no block of sweep sB covers, and the corner D_0(0, 0) of A's first block, which has no task of B
// above it: A stores those to the band itself.  tools/models/bulge_pair_model.py is the NumPy model of this data flow
// (tests/test_bulge_pair_model.py runs it on the CPU).  The column sums a task needs (z = E^T v and the strictly-lower
// half of p = D v) read an LDS image of the block: for A that is its slot, for B the slot it has just emptied.
//
// Both teams keep ONE barrier schedule -- eight workgroup barriers per step, [0] .. [7] -- and differ in where blocks come
// from (A: memory through the L2, B: LDS) and go to (A: LDS, B: memory).  A step is either the common one (both teams on
// full 64-row blocks, neither at a sweep start: pair_step_full<TEAM>, one instruction stream per team without masks,
// clamps or case distinctions) or the general one (pair_step_general: every case, out of line so that its registers are
// not charged to the common step).  B's store drain and its publish sit behind the NEXT step's barrier [1], where team
// A waits for its E loads anyway; A's D loads are issued behind that barrier and land during steps (2)-(4).
//
// Dependences across workgroups are those of k_bulge_chase: pairs are CLAIMED in order (so the owner of sweep sA - 1 is
// running or done), A's task k starts when progress[sA - 1] >= k + 2, B publishes progress[sB] after its stores have
// drained; all workgroups of a matrix sit on one XCD.  When a wait runs into its bound or the stop flag is up, the
// workgroup writes its live slots back to the band and publishes both sweeps' counts, so the per-wavefront launches can
// finish the chase from the counters exactly as after k_bulge_chase.
constexpr int kSlotE = kB * (kB + 1);          // E block, row stride 65 (conflict-free column access)
// D block, lower triangle packed by rows: (i, j) at i (i + 1) / 2 + j (2080 doubles).  The region is a little larger
// (2176 doubles: sized in round 6 for a form of the kernel that has been removed; kept, so that the
// LDS layout and the launch stay what they were).
constexpr int kSlotD = 17 * 128;
constexpr int kSlot = kSlotE + kSlotD;
constexpr int kTeamLds = 2 * kB + kB + 4 * kB + 8;   // vbuf[2][64], u[64], red[256], tau, beta (+ pad)
constexpr size_t kPairLdsBytes = sizeof(double) * (3 * kSlot + 2 * kTeamLds);

// Diagnostic build (-DPAIR_STAMPS): shader cycles of thread 0 between the barriers of every step, summed over all steps
// of all workgroups since the last read (sc_dbg_pair_stamps, tools/pair_stamps.py); nothing of it in the normal build.
// (round 6: the sums are kept in LDS -- one writer per entry: thread 0 [0..15], thread 256 [16..31]; [32..47] are
// unused -- and added to the global table when the thread leaves the kernel: a global atomic per stamp
// more than doubled the stage's time)
#ifdef PAIR_STAMPS
__device__ unsigned long long g_pair_stamps[48];
__shared__ unsigned long long s_pair_stamps[48];
#define PAIR_STAMP(var) unsigned long long var; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory");
#define PAIR_ACC(slot, a, b) if (tid == 0) s_pair_stamps[slot] += (b) - (a);
#define PAIR_ACC_B(slot, a, b) if (tid == 256) s_pair_stamps[16 + (slot)] += (b) - (a);
#define PAIR_FLUSH(first)                                                                         \
  for (int i_ = 0; i_ < 16; ++i_)                                                                 \
    if (s_pair_stamps[(first) + i_]) atomicAdd(&g_pair_stamps[(first) + i_], s_pair_stamps[(first) + i_]);
#else
#define PAIR_STAMP(var)
#define PAIR_ACC(slot, a, b)
#define PAIR_ACC_B(slot, a, b)
#define PAIR_FLUSH(first)
#endif

// The common step of k_bulge_pair: both teams at work on full 64-row blocks, neither at a sweep start.  Same barriers
// and the same arithmetic as the general form inside the kernel, without its masks, clamps and case distinctions -- the
// step is bound by instruction issue, not by flops -- and one instruction stream per team: A (TEAM 0) loads its blocks
// from the band and leaves them in its LDS slot, B (TEAM 1) takes the shifted blocks from the slots and stores to the band.
typedef double __attribute__((address_space(3)))* ldptr;   // LDS: ds_read / ds_write, never flat
struct PairStepArgs {
  double* ab;        // band of this matrix
  double* vd;        // its diamonds
  double* tau2;
  ldptr slots;       // LDS: ring of three position slots
  ldptr vbuf, u, red, sc;   // LDS: this team's vectors
  int* prog;
  int s, k;          // this team's sweep and position
  size_t dia;
  int cc;
  int tid;
};

template <int TEAM>
__device__ __forceinline__ void pair_step_full(const PairStepArgs& P, double& tau_p, int& pend_k) {
  const int tid = P.tid, tt = tid & 255, i = tid & 63;
  const int q = (tid >> 6) & 3;
  const int k = P.k, s = P.s;
  const int r0 = s + 1 + k * kB;
  ldptr vp = P.vbuf + ((k + 1) & 1) * kB;
  ldptr vn = P.vbuf + (k & 1) * kB;
  ldptr Eimg = P.slots + (k % 3) * kSlot;   // A: its slot; B: the slot it consumes, then its scratch image
  ldptr Dimg = Eimg + kSlotE;
  ldptr red = P.red;
  ldptr u = P.u;
  gdptr colbase_k = wave_uniform(P.ab + (size_t)r0 * kLdab);
  gdptr ebase_k = wave_uniform(P.ab + (size_t)(r0 - kB) * kLdab);
  const unsigned o_e = (unsigned)(kB + i + q * 16 * (kLdab - 1));   // E(i, 16 q + c) at ebase[o_e + c (kLdab - 1)]
  const unsigned o_d = (unsigned)(i + q * 16 * (kLdab - 1));        // D(i, 16 q + c) at colbase[o_d + c (kLdab - 1)]
  double d16[16], t16[16], vr[16];
  PAIR_STAMP(f0)
  if (TEAM == 0) {
#pragma unroll
    for (int c = 0; c < 16; ++c) t16[c] = ld_l2(ebase_k + (o_e + (unsigned)(c * (kLdab - 1))));
  } else {
    const ldptr En = P.slots + ((k + 1) % 3) * kSlot;
    const int i1 = min(i + 1, kB - 1);
    const ldptr rowD = i < kB - 1 ? Dimg + i1 * (i1 + 1) / 2 : En;
    const ldptr rowE = Eimg + i1 * (kB + 1) + 1;
#pragma unroll
    for (int c = 0; c < 16; ++c) d16[c] = rowD[q * 16 + c + 1];
#pragma unroll
    for (int c = 0; c < 16; ++c) t16[c] = i < kB - 1 ? rowE[q * 16 + c] : 0.0;
    if (q == 3) {
      const double dcol = Dimg[i1 * (i1 + 1) / 2];
      t16[15] = i < kB - 1 ? dcol : En[0];
      if (i == kB - 1) d16[15] = En[kSlotE];
    }
    PAIR_STAMP(g1)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the previous step's stores are in the L2
    PAIR_STAMP(g2)
    PAIR_ACC_B(10, f0, g1) PAIR_ACC_B(11, g1, g2)
  }
#pragma unroll
  for (int c = 0; c < 16; ++c) vr[c] = vp[q * 16 + c];
  PAIR_STAMP(fa)
  lds_barrier();                                                                  // [1]
  PAIR_STAMP(f1)
  PAIR_ACC(12, f0, fa)
  if (TEAM == 1) {
    if (tt == 0 && pend_k >= 0) __hip_atomic_store(P.prog + s, pend_k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    pend_k = k;
  } else {
    // D is not touched before step (5): its loads are issued here, behind the barrier, so that the other team does not
    // wait for their issue (under load the memory pipeline takes a block's 16 load instructions per wave slowly: issuing
    // them costs as much as waiting for the data) and land behind steps (2)-(4).  Entries above the diagonal: whatever
    // lies in front of the column, masked in step (5).
#pragma unroll
    for (int c = 0; c < 16; ++c) d16[c] = ld_l2(colbase_k + (o_d + (unsigned)(c * (kLdab - 1))));
  }
  {
    double a = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) a += t16[c] * vr[c];
    red[q * kB + i] = a;
  }
  lds_barrier();                                                                  // [2]
  {
    const double ui = tau_p * ((red[i] + red[kB + i]) + (red[2 * kB + i] + red[3 * kB + i]));
    ldptr erow = Eimg + i * (kB + 1) + q * 16;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      t16[c] -= ui * vr[c];
      erow[c] = t16[c];
    }
    if (q == 0) {
      const double x = t16[0];
      const double t2 = wave_sum(i >= 1 ? x * x : 0.0);
      const HH h = householder(__shfl(x, 0), t2);
      vn[i] = i == 0 ? 1.0 : x * h.scale;
      if (i == 0) { P.sc[0] = h.tau; P.sc[1] = h.beta; }
    }
  }
  lds_barrier();                                                                  // [3]
  PAIR_STAMP(f3)
#pragma unroll
  for (int c = 0; c < 16; ++c) vr[c] = vn[q * 16 + c];
  {
    double a = 0.0;
    const ldptr ecol = Eimg + q * 16 * (kB + 1) + i;
#pragma unroll
    for (int c = 0; c < 16; ++c) a += ecol[c * (kB + 1)] * vr[c];
    red[q * kB + i] = a;
  }
  lds_barrier();                                                                  // [4]
  if (tt < kB) u[tt] = P.sc[0] * ((red[tt] + red[kB + tt]) + (red[2 * kB + tt] + red[3 * kB + tt]));
  {
    ldptr rowp = Dimg + i * (i + 1) / 2 + q * 16;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      d16[c] = q * 16 + c <= i ? d16[c] : 0.0;
      if (q * 16 + c <= i) rowp[c] = d16[c];
    }
  }
  lds_barrier();                                                                  // [5]
  PAIR_STAMP(f5)
  {
    const double vi = vn[i];
#pragma unroll
    for (int c = 0; c < 16; ++c) t16[c] -= vi * u[q * 16 + c];
    if (q == 0) t16[0] = i == 0 ? P.sc[1] : 0.0;
    if (TEAM == 0) {
      ldptr erow = Eimg + i * (kB + 1) + q * 16;
#pragma unroll
      for (int c = 0; c < 16; ++c) erow[c] = t16[c];
      if (q == 0 && i >= 1) ebase_k[(unsigned)(kB + i)] = 0.0;   // the annihilated entries, see the kernel's header
    } else {
#pragma unroll
      for (int c = 0; c < 16; ++c) ebase_k[o_e + (unsigned)(c * (kLdab - 1))] = t16[c];
    }
    double a = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int ii = q * 16 + c;
      const double dcolv = Dimg[ii * (ii + 1) / 2 + min(i, ii)];
      a += (d16[c] + (ii > i ? dcolv : 0.0)) * vr[c];     // row half + column half share vn[16 q + c]
    }
    red[q * kB + i] = a;
  }
  lds_barrier();                                                                  // [6]
  PAIR_STAMP(f6)
  const double tau_f = P.sc[0];
  if (tt < kB) {
    const double pp = tau_f * ((red[tt] + red[kB + tt]) + (red[2 * kB + tt] + red[3 * kB + tt]));
    const double dot = wave_sum(pp * vn[tt]);
    u[tt] = pp - 0.5 * tau_f * dot * vn[tt];
  }
  lds_barrier();                                                                  // [7]
  PAIR_STAMP(f7)
  {
    const double vi = vn[i], wi = u[i];
    if (TEAM == 0) {
      ldptr rowp = Dimg + i * (i + 1) / 2 + q * 16;
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (q * 16 + c <= i) rowp[c] = d16[c] - vi * u[q * 16 + c] - wi * vr[c];
    } else {
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (q * 16 + c <= i) colbase_k[o_d + (unsigned)(c * (kLdab - 1))] = d16[c] - vi * u[q * 16 + c] - wi * vr[c];
    }
    double* vd = P.vd + P.dia * kDiaSize + (size_t)P.cc * kG + P.cc;
    if (tt < kB) vd[(size_t)tt * kG] = vn[tt];
    if (tt == 0) P.tau2[P.dia * kG + P.cc] = tau_f;
    tau_p = tau_f;
  }
#ifdef PAIR_STAMPS
  {
    PAIR_STAMP(f8)
    PAIR_ACC(1, f0, f1) PAIR_ACC(2, f1, f3) PAIR_ACC(3, f3, f5) PAIR_ACC(4, f5, f6) PAIR_ACC(5, f6, f7) PAIR_ACC(6, f7, f8)
    PAIR_ACC_B(1, f0, f1) PAIR_ACC_B(2, f1, f3) PAIR_ACC_B(3, f3, f5) PAIR_ACC_B(4, f5, f6) PAIR_ACC_B(5, f6, f7)
    PAIR_ACC_B(13, f7, f8)
  }
#endif
}

// The general step of k_bulge_pair (sweep starts, partial last blocks, steps in which only one team has a position): the
// same barriers as pair_step_full, with every mask and case distinction.  Not inlined: it runs in a few steps per pair
// only, and its registers would otherwise be charged to the common step.
struct PairGenArgs {
  double* ab;
  double* vd;
  double* tau2;
  ldptr slots;
  ldptr vbuf, u, red, sc;
  int* prog;
  int* sweeps_done;
  int n, s, k, my_len, team, to_lds;
  size_t dia0;
  int cc, tid;
};
struct PairCarry {
  double tau_p;
  int pend_k;
};

__device__ __noinline__ PairCarry pair_step_general(const PairGenArgs P, double tau_p, int pend_k) {
  double* const ab = P.ab;
  const ldptr slots = P.slots, vbuf = P.vbuf, u = P.u, red = P.red, sc = P.sc;
  int* const prog = P.prog;
  const int n = P.n, s = P.s, k = P.k, my_len = P.my_len, team = P.team, cc = P.cc, tid = P.tid;
  const bool to_lds = P.to_lds != 0;
  const size_t dia0 = P.dia0;
  const int tt = tid & 255, i = tid & 63, q = (tid >> 6) & 3;
  const bool active = k >= 0 && k < my_len;
  const bool first = k == 0;
  const bool eph = active && !first;            // this team has an off-diagonal block in this step
  const int kk = active ? k : 0;
  const int r0 = s + 1 + kk * kB;
  const int L = active ? min(kB, n - r0) : 0;
  ldptr vp = vbuf + ((kk + 1) & 1) * kB;   // reflector of this sweep's previous task
  ldptr vn = vbuf + (kk & 1) * kB;
  ldptr Eimg = slots + (kk % 3) * kSlot;   // A: its slot; B: the slot it consumes, then its scratch image
  ldptr Dimg = Eimg + kSlotE;
  const size_t dia = dia0 + kk;
  gdptr colbase_k = wave_uniform(ab + (size_t)r0 * kLdab);                        // AB(r0, r0)
  gdptr ebase_k = wave_uniform(ab + (size_t)(r0 - (first ? 0 : kB)) * kLdab);    // AB(r0 - kB, r0 - kB)

  // ---- (1) the blocks into registers: thread (i, q) holds row i, columns 16 q .. 16 q + 15
  double d16[16], t16[16];
  double xcol = 0.0;   // sweep start (k == 0, first wave of the team): x = AB(s + 1 + i, s)
#pragma unroll
  for (int c = 0; c < 16; ++c) { d16[c] = 0.0; t16[c] = 0.0; }
  if (active && team == 0) {
    // (E first: it is needed at once; D is not touched before step (5), its loads land behind steps (2)-(4))
    if (!first) {
      const int ic = min(i, L - 1);
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const int jj = q * 16 + c;
        t16[c] = ld_l2(ebase_k + (unsigned)((kB + ic - jj) + jj * kLdab));
      }
    } else if (q == 0) {
      gdptr col_s = wave_uniform(ab + (size_t)s * kLdab);
      xcol = ld_l2(col_s + (unsigned)(1 + min(i, L - 1)));
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int jc = min(q * 16 + c, L - 1);
      const int ic = min(max(i, jc), L - 1);
      d16[c] = ld_l2(colbase_k + (unsigned)((ic - jc) + jc * kLdab));
    }
  } else if (active) {
    // B's block = A's, shifted by (1, 1) (see the header); row 63 comes from row 0 of A's next position.  Whatever is
    // read from a slot that does not exist (A's last position: then L <= 63) is masked out below
    const ldptr En = slots + ((kk + 1) % 3) * kSlot;
    const int i1 = min(i + 1, kB - 1);
    const ldptr rowD = i < kB - 1 ? Dimg + i1 * (i1 + 1) / 2 : En;   // D'(i, jj) = rowD[jj + 1]
    const ldptr rowE = Eimg + i1 * (kB + 1) + 1;                     // E'(i, jj) = rowE[jj]  (i, jj < 63)
#pragma unroll
    for (int c = 0; c < 16; ++c) d16[c] = rowD[q * 16 + c + 1];
    if (!first) {
#pragma unroll
      for (int c = 0; c < 16; ++c) t16[c] = i < kB - 1 ? rowE[q * 16 + c] : 0.0;
    }
    if (q == 3) {   // column 63: E'(i, 63) = D_k(i + 1, 0); corner (63, 63): D_{k+1}(0, 0) and E_{k+1}(0, 0)
      const double dcol = Dimg[i1 * (i1 + 1) / 2];
      if (!first) t16[15] = i < kB - 1 ? dcol : En[0];
      if (i == kB - 1) d16[15] = En[kSlotE];
    }
    if (first && q == 0) xcol = i < kB - 1 ? Dimg[i1 * (i1 + 1) / 2] : En[0];
  }
#pragma unroll
  for (int c = 0; c < 16; ++c) t16[c] = i < L ? t16[c] : 0.0;
  xcol = i < L ? xcol : 0.0;
  // B (and a lone A): the stores of the previous step are in the L2 -- a wait that overlaps A's for its loads
  // (A's own few stores -- zeros, corner, reflector -- are older than its next loads, whose data it waits for: in
  // order; once A has run out of positions it drains like B)
  if (!to_lds || !active) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  lds_barrier();                                                                    // [1] B's slot reads are done
  if (tt == 0 && pend_k >= 0) {   // publish the previous step's task
    __hip_atomic_store(prog + s, pend_k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (pend_k + 1 == my_len) atomicAdd(P.sweeps_done, 1);
  }
  pend_k = -1;

  // ---- (2) u = tau_p E vp: partial sums over this wave's 16 columns
  if (eph) {
    double a = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) a += t16[c] * vp[q * 16 + c];
    red[q * kB + i] = a;
  }
  lds_barrier();                                                                    // [2]
  // ---- (3) E <- E (I - tau_p vp vp^T) in registers + its LDS image; new reflector; image of D (packed lower)
  if (eph) {
    const double ui = tau_p * ((red[i] + red[kB + i]) + (red[2 * kB + i] + red[3 * kB + i]));
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      t16[c] -= ui * vp[q * 16 + c];
      Eimg[i * (kB + 1) + q * 16 + c] = t16[c];
    }
    if (q == 0) xcol = t16[0];
  }
  if (active && q == 0) {
    const double t2 = wave_sum((i >= 1 && i < L) ? xcol * xcol : 0.0);
    const HH h = householder(__shfl(xcol, 0), t2);
    vn[i] = i == 0 ? 1.0 : (i < L ? xcol * h.scale : 0.0);
    if (i == 0) { sc[0] = h.tau; sc[1] = h.beta; }
    if (first && i < L) {   // the annihilated column: AB(s + 1 .., s) = (beta, 0, ..)
      gdptr col_s = wave_uniform(ab + (size_t)s * kLdab);
      col_s[(unsigned)(1 + i)] = i == 0 ? h.beta : 0.0;
    }
  }
  lds_barrier();                                                                    // [3]
    // ---- (4) z_j = sum_i E[i, j] vn_i: thread (j = i, rows 16 q ..)
  if (eph) {
    double a = 0.0;
#pragma unroll
    for (int ii = q * 16; ii < q * 16 + 16; ++ii) a += Eimg[ii * (kB + 1) + i] * vn[ii];
    red[q * kB + i] = a;
  }
  lds_barrier();                                                                    // [4]
  if (eph && tt < kB) u[tt] = sc[0] * ((red[tt] + red[kB + tt]) + (red[2 * kB + tt] + red[3 * kB + tt]));
  // image of D (packed lower) for the column half of p = D vn; A's D loads have had steps (2)-(4) to land
#pragma unroll
  for (int c = 0; c < 16; ++c) d16[c] = (i < L && q * 16 + c <= i) ? d16[c] : 0.0;
  if (active) {
    ldptr rowp = Dimg + i * (i + 1) / 2 + q * 16;
#pragma unroll
    for (int c = 0; c < 16; ++c)
      if (q * 16 + c <= i) rowp[c] = d16[c];
  }
  lds_barrier();                                                                    // [5]
    // ---- (6) E <- H E, first column = beta e1: to LDS (A) or to the band (B); then p = D vn, row half from the
  // registers, strictly-lower (column) half from the packed image
  if (eph) {
    const double vi = vn[i], beta = sc[1];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int jj = q * 16 + c;
      double e = t16[c] - vi * u[jj];
      if (jj == 0) e = i == 0 ? beta : 0.0;
      if (to_lds) {
        Eimg[i * (kB + 1) + jj] = i < L ? e : 0.0;
        // the annihilated entries (first column below its first row) lie outside every block of sweep sB: B's shifted
        // blocks never write them back, so A zeroes them in the band itself
        if (jj == 0 && i >= 1 && i < L) ebase_k[(unsigned)(kB + i)] = 0.0;
      } else if (i < L) {
        ebase_k[(unsigned)((kB + i - jj) + jj * kLdab)] = e;
      }
    }
  }
  if (active) {
    double a = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) a += d16[c] * vn[q * 16 + c];          // (entries above the diagonal are zero)
#pragma unroll
    for (int ii = q * 16; ii < q * 16 + 16; ++ii) {
      const double dv = Dimg[ii * (ii + 1) / 2 + min(i, ii)];
      a += ii > i ? dv * vn[ii] : 0.0;
    }
    red[q * kB + i] = a;
  }
  lds_barrier();                                                                    // [6]
    const double tau_now = sc[0];
  if (active && tt < kB) {
    const double pp = tau_now * ((red[tt] + red[kB + tt]) + (red[2 * kB + tt] + red[3 * kB + tt]));
    const double dot = wave_sum(pp * vn[tt]);
    u[tt] = pp - 0.5 * tau_now * dot * vn[tt];
  }
  lds_barrier();                                                                    // [7]
    // ---- (8) D <- D - vn w^T - w vn^T: to LDS (A) or to the band (B); the reflector goes into its diamond
  if (active) {
    const double vi = vn[i], wi = u[i];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int jj = q * 16 + c;
      if (jj <= i) {
        const double val = d16[c] - vi * u[jj] - wi * vn[jj];
        if (to_lds) {
          Dimg[i * (i + 1) / 2 + jj] = i < L ? val : 0.0;
          // row 0 of a block is consumed by B's task one position up -- which does not exist for A's first block:
          // its corner AB(sA + 1, sA + 1) is final already and goes to the band here
          if (first && i == 0) colbase_k[0] = val;
        } else if (i < L) {
          colbase_k[(unsigned)((i - jj) + jj * kLdab)] = val;
        }
      }
    }
    double* vd = P.vd + dia * kDiaSize + (size_t)cc * kG + cc;
    if (tt < L) vd[(size_t)tt * kG] = vn[tt];
    if (tt == 0) P.tau2[dia * kG + cc] = tau_now;
    tau_p = tau_now;
    if (!to_lds) pend_k = k;   // published once the stores have drained: behind the next step's loads
  }
  return PairCarry{tau_p, pend_k};
}

// (the few fields of the band workspace's layout the kernel needs, instead of all of SbLayout in scalar registers)
struct PairLayout {
  int n;
  long long slab, ab, vd, tau2;
};

// whether step m of a pair is the common one (both teams on full blocks, neither at a sweep start)
__device__ __forceinline__ bool pair_common_step(bool hasB, int m, int lenA, int sA, int n) {
  return hasB && m >= 3 && m < lenA && sA + 1 + (m + 1) * kB <= n;
}

__global__ __launch_bounds__(512, 1) void k_bulge_pair(double* __restrict__ sb_all, PairLayout SL, int batch, int W, int nxcd,
                                                       int* __restrict__ progress, int* __restrict__ next_pair,
                                                       int* __restrict__ ctl, int give_up_after) {
  extern __shared__ __attribute__((aligned(16))) double pair_lds[];
  __shared__ int s_go, s_claim, s_xcd, s_slot;

  const int n = SL.n;
  const int tid = threadIdx.x;
  // (the team is uniform over a wave: told to the compiler, so that the position, the step's case and the branches on
  // them are scalar)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int team = wave >> 2;
  const int tt = tid & 255;
  double* const slots = pair_lds;
  double* const tl = pair_lds + 3 * kSlot + team * kTeamLds;
  double* const vbuf = tl;
  double* const u = tl + 2 * kB;
  double* const red = tl + 3 * kB;
  double* const sc = tl + 7 * kB;   // [0] tau, [1] beta of the reflector being generated

  if (tid == 0) {
    unsigned id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
    s_xcd = (int)(id & 7u) % nxcd;
    s_slot = atomicAdd(ctl + 2 + s_xcd, 1);
  }
#ifdef PAIR_STAMPS
  if (tid < 48) s_pair_stamps[tid] = 0;
#endif
  __syncthreads();
  const int xcd = s_xcd, slot = s_slot;
  const int mpx = xcd < batch ? (batch - xcd + nxcd - 1) / nxcd : 0;   // matrices of this XCD: xcd, xcd + nxcd, ...
  if (mpx == 0 || slot >= mpx * W) return;
  const int K0 = chase_len(n, 0);
  int steps_left = give_up_after;

  int cur = slot % mpx, exhausted = 0;
  while (exhausted < mpx) {
    const int b = xcd + nxcd * cur;
    int* prog = progress + (size_t)b * n;
    if (tid == 0) s_claim = atomicAdd(next_pair + b, 1);
    __syncthreads();
    const int sA = 2 * __builtin_amdgcn_readfirstlane(s_claim);
    __syncthreads();
    if (sA > n - 3) {
      ++exhausted;
      cur = cur + 1 < mpx ? cur + 1 : 0;
      continue;
    }
    exhausted = 0;
    double* sb = sb_all + (size_t)b * SL.slab;
    double* ab = sb + SL.ab;
    const bool hasB = sA + 1 <= n - 3;
    const int lenA = chase_len(n, sA), lenB = hasB ? chase_len(n, sA + 1) : 0;
    const int s = sA + team;                 // this team's sweep
    const int my_len = team ? lenB : lenA;
    const int S = s / kG, cc = s - S * kG;
    const size_t dia0 = (size_t)S * K0 - (size_t)S * (S - 1) / 2;
    const int len_prev = sA > 0 ? chase_len(n, sA - 1) : 0;
    const bool to_lds = team == 0 && hasB;   // A's results stay in LDS (a lone last sweep writes to memory itself)
    double tau_p = 0.0;

    const int nsteps = hasB ? lenA + 2 : lenA;
    // ---- the look at the predecessor pair (A's dependence; B's are inside the workgroup), by thread 256: the first wave of
    // team B opens a step with LDS reads only.  Followers run at the dependence's limit -- pair p + 1 starts when its
    // workgroup has finished pair p - 3, a few steps behind pair p, and both advance at the same rate -- so the look is
    // needed in 0.6 of all steps and costs 2 300 cycles of a 16 900-cycle step, all other waves waiting at [0]
    // (profiles/r06_pair_stamps.txt; requesting the values a step ahead did not pay: profiles/r06_pair_ab.txt).
    int have_c = 0;      // thread 256: last value seen of the predecessor's counter (it only grows)
    int pend_k = -1;     // task of this team whose stores are on their way: published behind the next step's loads
    for (int m = 0; m < nsteps; ++m) {
      PAIR_STAMP(ts0)
      if (tid == 256) {
        const int need = (sA > 0 && m < lenA) ? min(m + 2, len_prev) : 0;
        int go = 1;
        if (have_c < need || (m & 7) == 0) {
#ifdef PAIR_STAMPS
          s_pair_stamps[16 + 14] += 1ull;
#endif
          const int want = need;
          const int stop0 = __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          int have = sA > 0 ? __hip_atomic_load(prog + sA - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
          if (stop0) go = 0;
          long spins = 0;
          while (go && have < want) {
            // (2^21 polls of ~1 us: seconds, orders of magnitude above any wait for a running workgroup)
            ++spins;
            if (spins > (1L << 21) ||
                ((spins & 15) == 0 && __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
              if (!__hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                ctl[10] = b; ctl[11] = sA; ctl[12] = m;
              }
              __hip_atomic_store(ctl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              go = 0;
              break;
            }
            __builtin_amdgcn_s_sleep(1);
            have = __hip_atomic_load(prog + sA - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          have_c = have;
        }
        s_go = go;
      }
      PAIR_STAMP(tsp)
      lds_barrier();   // [0] (also: A's last slot writes of the previous step are ordered before B's reads below)
      if (!s_go) {
        // ---- give up between steps.  First the pending publish (its stores drained), then: A has finished positions
        // < min(m, lenA), B positions < m - 2; what A left for B (positions m - 2 and m - 1) goes back to the band, and
        // both counts are published
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tt == 0 && pend_k >= 0) __hip_atomic_store(prog + s, pend_k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (hasB) {
          for (int pos = max(m - 2, 0); pos < min(m, lenA); ++pos) {
            const double* Es = slots + (pos % 3) * kSlot;
            const double* Ds = Es + kSlotE;
            const int r0p = sA + 1 + pos * kB;
            const int Lp = min(kB, n - r0p);
            // (row 0 of the older slot has been consumed and rewritten in the band by B's task one position up)
            const int i_lo = (pos == m - 2 && pos >= 1) ? 1 : 0;
            if (pos > 0)
              for (int e = tid; e < kB * kB; e += 512) {
                const int ii = e & 63, jj = e >> 6;
                if (ii >= i_lo && ii < Lp) ab[(size_t)(r0p - kB + jj) * kLdab + (kB + ii - jj)] = Es[ii * (kB + 1) + jj];
              }
            for (int e = tid; e < kB * kB; e += 512) {
              const int ii = e & 63, jj = e >> 6;
              if (ii >= jj && ii >= i_lo && ii < Lp) ab[(size_t)(r0p + jj) * kLdab + (ii - jj)] = Ds[ii * (ii + 1) / 2 + jj];
            }
          }
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __syncthreads();
          if (tid == 0) {
            __hip_atomic_store(prog + sA, min(m, lenA), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(prog + sA + 1, min(max(m - 2, 0), lenB), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
        if (tid == 0) { PAIR_FLUSH(0) }
        if (tid == 256) { PAIR_FLUSH(16) }
        return;
      }

      PAIR_STAMP(ts1)
      const int k = team ? m - 2 : m;
      // ---- the common step: both teams at work on full 64-row blocks, neither at a sweep start (pair_step_full)
      if (pair_common_step(hasB, m, lenA, sA, n)) {
        PairStepArgs pa{ab, sb + SL.vd, sb + SL.tau2, (ldptr)slots, (ldptr)vbuf, (ldptr)u, (ldptr)red, (ldptr)sc, prog, s, k,
                        dia0 + k, cc, tid};
        if (team == 0) pair_step_full<0>(pa, tau_p, pend_k);
        else pair_step_full<1>(pa, tau_p, pend_k);
#ifdef PAIR_STAMPS
        if (tid == 0) { s_pair_stamps[9] += 1ull; s_pair_stamps[0] += ts1 - ts0; }
        if (tid == 256) { s_pair_stamps[16] += ts1 - ts0; s_pair_stamps[16 + 7] += tsp - ts0; }
#endif
      } else {
        PairGenArgs ga{ab, sb + SL.vd, sb + SL.tau2, (ldptr)slots, (ldptr)vbuf, (ldptr)u, (ldptr)red, (ldptr)sc, prog,
                       ctl + 16 + xcd, n, s, k, my_len, team, to_lds ? 1 : 0, dia0, cc, tid};
        const PairCarry pc = pair_step_general(ga, tau_p, pend_k);
        tau_p = pc.tau_p;
        pend_k = pc.pend_k;
      }
      // (no barrier here: the next step's [0] orders this step's slot writes before their readers, and nothing else of
      // the next step touches LDS before it)
#ifdef PAIR_STAMPS
      if (tid == 0) s_pair_stamps[8] += 1ull;
#endif
      if (tid == 0) {
        if (to_lds && m + 1 == lenA) atomicAdd(ctl + 16 + xcd, 1);   // (A's last task; its count is published below)
        // test hook (sc_dbg_set_chase): raise the time-out flag after that many steps of this workgroup
        if (give_up_after > 0 && --steps_left == 0) {
          ctl[1] = give_up_after;
          __hip_atomic_store(ctl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    // ---- end of the pair: the last task's stores, then its count; sweep sA lived in LDS until B had consumed it -- its
    // count only matters to a take-over and is complete now
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tt == 0 && pend_k >= 0) {
      __hip_atomic_store(prog + s, pend_k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (pend_k + 1 == my_len) atomicAdd(ctl + 16 + xcd, 1);
    }
    if (tid == 0 && hasB) __hip_atomic_store(prog + sA, lenA, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid == 0) { PAIR_FLUSH(0) }
  if (tid == 256) { PAIR_FLUSH(16) }
}

}  // namespace

// ================================================================================================================
// Host side of stage 2.  Which kernel form a chase gets: twostage_policy.h.

// The persistent chase of the whole batch as ONE launch (+ k_chase_finish, the take-over) in the form sc_host::chase_form_for
// chose.  Returns whether it went out; if not, the caller chases by the per-wavefront launches.
static int launch_chase(sc_ctx* ctx, sc_host::ChaseForm form, int n, int batch, double* d_sb_ws, const SbLayout& SL,
                        SbTimers& timers, bool* chased) {
  using sc_host::ChaseForm;
  hipStream_t st = ctx->stream;
  const bool pair = form == ChaseForm::Pair;
  int per_cu = 0;
  const hipError_t oe =
      pair ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_bulge_pair, 512, kPairLdsBytes)
           : (form == ChaseForm::Spread ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_bulge_chase<1>, 256, 0)
                                        : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_bulge_chase<0>, 256, 0));
  if (oe != hipSuccess) per_cu = 0;
  const sc_host::ChaseLaunch L =
      sc_host::chase_launch(sc_host::two_stage_env(), form, n, batch, ctx->nxcd, ctx->num_cus, per_cu);
  if (L.W < 1) return SC_OK;
  // progress counters (batch x n) | claim counters (batch) | early hand-off records in dc_aux; the control block is the
  // context's own (dc_aux is reused by the D&C of this solve before sc_collect_events reads the block)
  SC_TRY(sc_reserve_dc_aux(ctx, L.prog_bytes + L.next_bytes + L.early_bytes));
  int* d_prog = reinterpret_cast<int*>(ctx->dc_aux);
  int* d_next = reinterpret_cast<int*>(reinterpret_cast<char*>(ctx->dc_aux) + L.prog_bytes);
  int* d_ctl = ctx->d_chase_ctl;
  v4i* d_early = L.early_bytes ? reinterpret_cast<v4i*>(reinterpret_cast<char*>(ctx->dc_aux) + L.prog_bytes + L.next_bytes)
                               : nullptr;
  SC_HIP(ctx, hipMemsetAsync(ctx->dc_aux, 0, L.prog_bytes + L.next_bytes + L.early_bytes, st));
  SC_HIP(ctx, hipMemsetAsync(d_ctl, 0, kChaseCtlInts * sizeof(int), st));
  timers.bulge.start();
  if (pair)
    hipLaunchKernelGGL(k_bulge_pair, dim3((unsigned)L.grid), dim3(512), kPairLdsBytes, st, d_sb_ws,
                       PairLayout{SL.n, SL.slab, SL.ab, SL.vd, SL.tau2}, batch, L.W, L.nxcd, d_prog, d_next, d_ctl,
                       ctx->chase_give_up);
  else if (form == ChaseForm::Spread)
    hipLaunchKernelGGL(k_bulge_chase<1>, dim3((unsigned)L.grid), dim3(256), 0, st, d_sb_ws, SL, batch, L.W, L.nxcd, d_prog,
                       d_next, d_ctl, ctx->chase_give_up, d_early);
  else
    hipLaunchKernelGGL(k_bulge_chase<0>, dim3((unsigned)L.grid), dim3(256), 0, st, d_sb_ws, SL, batch, L.W, L.nxcd, d_prog,
                       d_next, d_ctl, ctx->chase_give_up, d_early);
  const hipError_t le = hipGetLastError();
  timers.bulge.stop();
  if (le != hipSuccess) {
    // a refused pair launch (e.g. the 157 KB of dynamic LDS on a device that does not grant them): this solve is
    // finished by the per-wavefront launches, later solves of the context leave the pair form alone
    if (pair) {
      ctx->pair_attr = 0;
      ++ctx->cnt_pair_fallbacks;
    }
    return SC_OK;
  }
  // (round 6: no look at the outcome from the host -- the take-over is a launch of its own that returns at once
  // when the chase completed, and the control block's counts reach the context's counters at the next
  // synchronising call: sc_collect_events)
  hipLaunchKernelGGL(k_chase_finish, dim3((unsigned)batch), dim3(256), 0, st, d_sb_ws, SL, batch, L.nxcd, d_prog,
                     (const int*)d_ctl, ctx->d_status);
  SC_HIP(ctx, hipGetLastError());
  ++ctx->cnt_chase_launches;
  if (pair) ++ctx->cnt_pair_launches;
  ctx->last_chase_ctl = d_ctl;
  ctx->chase_ctl_xcds = L.nxcd;
  *chased = true;
  return SC_OK;
}

// The chase as one launch per wavefront of tasks (k_bulge_step), parts of the batch on separate streams.
static int chase_stepwise(sc_ctx* ctx, int n, int batch, double* d_sb_ws, const SbLayout& SL) {
  const sc_host::TwoStageEnv& E = sc_host::two_stage_env();
  hipStream_t st = ctx->stream;
  const int t_max = 2 * (n - 3) + chase_len(n, n - 3) - 1;
  const int gx = chase_len(n, 0) / 2 + 1;
  const int nparts = sc_host::bulge_stream_parts(E, batch);
  ctx->last_chase_stream_parts = nparts;
  if (nparts > 1) {
    SideFork parts(ctx, st);
    SC_TRY(parts.fork(nparts));
    const int burst = sc_host::bulge_burst(E);
    for (int t0 = 0; t0 <= t_max; t0 += burst)
      for (int p = 0; p < nparts; ++p) {
        const sc_host::PartBounds pb = sc_host::part_bounds(batch, nparts, p);
        for (int t = t0; t <= std::min(t_max, t0 + burst - 1); ++t)
          hipLaunchKernelGGL(k_bulge_step, dim3((unsigned)gx, (unsigned)(pb.hi - pb.lo)), dim3(256), 0, parts.stream(p),
                             d_sb_ws + (size_t)pb.lo * SL.slab, SL, t);
      }
    SC_TRY(parts.join());
  } else {
    for (int t = 0; t <= t_max; ++t)
      hipLaunchKernelGGL(k_bulge_step, dim3((unsigned)gx, (unsigned)batch), dim3(256), 0, st, d_sb_ws, SL, t);
  }
  return SC_OK;
}

// Stage 2 on ctx->stream: band -> tridiagonal; d, e into the tri slab.
int sb_stage2(sc_ctx* ctx, double* d_a, long long stride_a, int n, int batch, double* d_tri_ws, const TriLayout& TL,
              double* d_sb_ws, const SbLayout& SL, double* d_band_copy, SbTimers& timers) {
  hipStream_t st = ctx->stream;
  ctx->last_chase_stream_parts = 0;   // (chase_stepwise sets it)
  hipLaunchKernelGGL(k_band_extract, dim3(256, (unsigned)batch), dim3(256), 0, st, d_a, stride_a, d_sb_ws, SL);
  if (d_band_copy)   // debugging aid: the band of every matrix as stage 1 left it, (batch, kLdab * n)
    for (int b = 0; b < batch; ++b)
      SC_HIP(ctx, hipMemcpyAsync(d_band_copy + (size_t)b * kLdab * n, d_sb_ws + (size_t)b * SL.slab + SL.ab,
                                 sizeof(double) * kLdab * n, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k_sb_clean, dim3((unsigned)n, (unsigned)batch), dim3(256), 0, st, d_a, stride_a, n);
  for (int b = 0; b < batch; ++b) {
    double* sb = d_sb_ws + (size_t)b * SL.slab;
    SC_HIP(ctx, hipMemsetAsync(sb + SL.vd, 0, sizeof(double) * (size_t)SL.ndia * kDiaSize, st));
    SC_HIP(ctx, hipMemsetAsync(sb + SL.tau2, 0, sizeof(double) * (size_t)SL.ndia * kG, st));
  }
  if (n >= 3) {
    if (ctx->pair_attr < 0)   // per device, hence per context: the caller made ctx->device current
      ctx->pair_attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bulge_pair),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPairLdsBytes) == hipSuccess;
    if (ctx->nxcd <= 0) SC_TRY(probe_xcd_count(ctx, st));
    const sc_host::ChaseForm form =
        sc_host::chase_form_for(sc_host::two_stage_env(), n, batch, ctx->nxcd, ctx->num_cus, ctx->pair_attr == 1,
                                ctx->chase_mode, ctx->chase_form, ctx->chase_ok);
    bool chased = false;
    if (form != sc_host::ChaseForm::Stepwise) SC_TRY(launch_chase(ctx, form, n, batch, d_sb_ws, SL, timers, &chased));
    if (!chased) {
      ++ctx->cnt_stepwise_chases;
      timers.bulge.start();
      SC_TRY(chase_stepwise(ctx, n, batch, d_sb_ws, SL));
      timers.bulge.stop();
    }
  }
  hipLaunchKernelGGL(k_band_to_tri, dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, st, d_sb_ws, SL,
                     d_tri_ws, TL);
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

// ---- diagnostic build only (-DCHASE_STAMPS): the segment sums of k_bulge_chase; reset after the read
extern "C" int sc_dbg_chase_stamps(unsigned long long* out16) {
#ifdef CHASE_STAMPS
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_chase_stamps), sizeof(unsigned long long) * 16) != hipSuccess) return 5;
  static const unsigned long long zeros[16] = {0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_chase_stamps), zeros, sizeof(zeros)) == hipSuccess ? 0 : 5;
#else
  (void)out16;
  return 1;
#endif
}

// ---- diagnostic build only: {sum t(E in LDS), sum t(E stored) [tasks with k > 0], sum t(D in LDS), sum t(end), tasks,
// tasks with k > 0}, cycles since the task's start; reset after the read
extern "C" int sc_dbg_pair_stamps(unsigned long long* out16) {
#ifdef PAIR_STAMPS
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_pair_stamps), 384) != hipSuccess) return 5;   // (48 entries)
  const unsigned long long z[48] = {0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_pair_stamps), z, 384) == hipSuccess ? 0 : 5;
#else
  (void)out16;
  return 1;
#endif
}

extern "C" int sc_dbg_bulge_stamps(unsigned long long* out6) {
#ifdef BULGE_STAMPS
  if (hipMemcpyFromSymbol(out6, HIP_SYMBOL(g_bulge_stamps), 48) != hipSuccess) return 5;
  unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_bulge_stamps), z, 64) == hipSuccess ? 0 : 5;
#else
  (void)out6;
  return 1;
#endif
}
