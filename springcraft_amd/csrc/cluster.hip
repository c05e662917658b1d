// Clustering of the items of a square float64 dissimilarity matrix (an ensemble's pairwise RMSD matrix, the distances of a
// correlation network, 1 - |dcc|): neighbour-count clustering (Daura et al. 1999, gmx cluster -method gromos) and k-medoids
// (PAM: BUILD, then best-swap SWAP with the FastPAM1 evaluation, Schubert & Rousseeuw 2021).  No reference counterpart.
//
// Item i is invalid when dist[i, i] is NaN (what rmsd_matrix writes for a non-finite frame): label -1, it neither counts nor
// is counted.  A NaN between two valid items sets status[2]; nothing is defined then and every label stays -1.  Both
// methods are dependent rounds of whole-matrix passes.  A run's state lives in the caller's workspace (cluster_policy.h);
// every kernel of a round or an iteration looks at the status and the control words first and does nothing once the run
// is over, so the host enqueues rounds in chunks and reads four int32 per chunk.  Ties go to the lowest index; integer
// atomics only (an LDS histogram); every floating-point sum has one fixed order: a thread's strided terms ascending, a xor
// butterfly over the wavefront, the wavefronts ascending.
//
// Neighbour count.  k_cluster_valid: the validity bitset.  k_cluster_pack, one streaming pass, one workgroup per row: a
// wavefront reads 64 consecutive columns and stores __ballot(d <= cutoff) & valid as one word of the (n, ceil(n / 64)) bit
// matrix; an item is always its own neighbour, so a round removes its centre.  dist is not read again.  A round:
// k_cluster_pick (one workgroup: arg-max of the counts over alive items, R = adj[centre] & alive, labels, alive &= ~R) and
// k_cluster_discount (every alive row: count -= popcount(adj[row] & R); words where R is 0 are not read).
//
// k-medoids.  dn / ds: an item's distance to its nearest and second-nearest medoid along the medoid's row, the lowest slot
// among equals.  BUILD step: k_kmed_gain (one workgroup per candidate row) -> k_kmed_pick -> k_kmed_assign (the new
// medoid's row only).  k_kmed_group: the valid items grouped by nearest slot, stable (order, seg, dn_o, ds_o), each slot's
// loss = sum(ds - dn), the total deviation.  SWAP iteration: k_kmed_eval, one pass over dist, one workgroup per candidate
// row x: its wavefronts take whole segments, lanes stride over a segment reading dist[x, order[t]] beside the contiguous
// dn_o / ds_o, and delta(x, s) = loss[s] + own[s] + shared; the row's best (delta, s) is written.  k_kmed_swap (one
// workgroup) takes the best row and swaps if its delta < 0, else ends the run; k_kmed_assign (all medoid rows) and
// k_kmed_group follow.  The evaluation has two forms with the same arithmetic (cluster_policy.h: cluster_form).
#include "block_sum.h"
#include "cluster_internal.h"

// (every sum is the additions as written)
#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int kCtlActive = 0, kCtlMedoids = 1;
constexpr int kStLeft = 0, kStDone = 1, kStFlag = 2, kStMedoids = 3;
constexpr int kPickThreads = 1024;
constexpr int kGroupWaves = 8;
constexpr int kMaxK = (int)sc_host::kClusterMaxK;

__device__ __forceinline__ bool has_bit(const u64* set, long long j) { return (set[j >> 6] >> (j & 63)) & 1ull; }
__device__ __forceinline__ double pos_inf() { return __builtin_huge_val(); }

// the sum of v over the workgroup in every thread (integers: any order gives the same)
__device__ __forceinline__ int block_sum_int(int v, int* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  int s = 0;
  for (int w = 0; w < nw; ++w) s += red[w];
  return s;
}

// ---- validity: one workgroup -------------------------------------------------------------------------------------------------
// valid (and alive, unless null) <- the items with a diagonal that is not NaN; ctl <- 0; status <- (left0 < 0 ? the number of
// valid items : left0, 0, 0, 0)
__global__ __launch_bounds__(kPickThreads) void k_cluster_valid(const double* __restrict__ dist, long long n, long long words,
                                                                u64* __restrict__ valid, u64* __restrict__ alive, int left0,
                                                                int* __restrict__ ctl, int* __restrict__ status) {
  __shared__ int red[kPickThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int count = 0;
  for (long long w = wave; w < words; w += kPickThreads / 64) {
    const long long j = 64 * w + lane;
    bool ok = false;
    if (j < n) {
      const double d = dist[j * n + j];
      ok = d == d;
    }
    const u64 m = __ballot(ok);
    if (lane == 0) {
      valid[w] = m;
      if (alive) alive[w] = m;
      count += __popcll(m);
    }
  }
  const int total = block_sum_int(count, red);
  if (threadIdx.x < sc_host::kClusterCtlInts) ctl[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    status[kStLeft] = left0 < 0 ? total : left0;
    status[kStDone] = status[kStFlag] = status[kStMedoids] = 0;
  }
}

// ---- neighbour count -----------------------------------------------------------------------------------------------------------
// grid (n), 256 threads
__global__ __launch_bounds__(256) void k_cluster_pack(const double* __restrict__ dist, long long n, long long words, double cutoff,
                                                      const u64* __restrict__ valid, u64* __restrict__ adj,
                                                      int* __restrict__ count, int* __restrict__ labels, int* __restrict__ status) {
  __shared__ int red[4];
  const long long i = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool row_ok = has_bit(valid, i);
  const double* row = dist + i * n;
  int c = 0;
  bool nan_pair = false;
  for (long long w = wave; w < words; w += 4) {
    const long long j = 64 * w + lane;
    const u64 vmask = valid[w];
    const bool col_ok = (vmask >> lane) & 1ull;   // (a column >= n has no bit)
    bool in = false;
    if (j < n) {
      const double d = row[j];
      in = d <= cutoff || j == i;
      nan_pair = nan_pair || (row_ok && col_ok && d != d);
    }
    const u64 m = row_ok ? (__ballot(in) & vmask) : 0ull;
    if (lane == 0) {
      adj[i * words + w] = m;
      c += __popcll(m);
    }
  }
  if (nan_pair) status[kStFlag] = 1;   // (every writer writes the same value)
  const int total = block_sum_int(c, red);
  if (threadIdx.x == 0) {
    count[i] = total;
    labels[i] = -1;
  }
}

// one workgroup of kPickThreads
__global__ __launch_bounds__(kPickThreads) void k_cluster_pick(long long n, long long words, int max_clusters, int* ctl,
                                                               u64* alive, u64* members, const int* __restrict__ count,
                                                               const u64* __restrict__ adj, int* __restrict__ labels,
                                                               int* __restrict__ reps, int* __restrict__ sizes, int* status) {
  __shared__ u64 red_key[kPickThreads / 64];
  __shared__ int red[kPickThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int left = status[kStLeft], made = status[kStDone], flag = status[kStFlag];
  __syncthreads();   // (everyone has read the status before thread 0 changes it)
  if (flag || left <= 0 || made >= max_clusters) {
    if (tid == 0) {
      ctl[kCtlActive] = 0;
      if (flag) status[kStLeft] = 0;
    }
    return;
  }
  // arg-max of (count, lowest index): an alive item counts itself, so every key is positive
  u64 best = 0;
  for (long long i = tid; i < n; i += kPickThreads)
    if (has_bit(alive, i)) {
      const u64 key = ((u64)(unsigned)count[i] << 32) | (u64)(0xffffffffu - (unsigned)i);
      best = key > best ? key : best;
    }
  for (int off = 32; off >= 1; off >>= 1) {
    const u64 other = __shfl_xor(best, off);
    best = other > best ? other : best;
  }
  if (lane == 0) red_key[wave] = best;
  __syncthreads();
  best = red_key[0];
  for (int w = 1; w < kPickThreads / 64; ++w) best = red_key[w] > best ? red_key[w] : best;
  if (best == 0) {   // (cannot be: left > 0 means an alive item)
    if (tid == 0) {
      ctl[kCtlActive] = 0;
      status[kStLeft] = 0;
    }
    return;
  }
  const long long centre = (long long)(0xffffffffu - (unsigned)(best & 0xffffffffull));
  int size = 0;
  for (long long w = tid; w < words; w += kPickThreads) {
    const u64 a = alive[w], r = adj[centre * words + w] & a;
    members[w] = r;
    alive[w] = a & ~r;
    size += __popcll(r);
  }
  size = block_sum_int(size, red);   // (its barriers also order the members' stores before the loads below)
  for (long long j = tid; j < n; j += kPickThreads)
    if (has_bit(members, j)) labels[j] = made;
  if (tid == 0) {
    reps[made] = (int)centre;
    sizes[made] = size;
    status[kStLeft] = left - size;
    status[kStDone] = made + 1;
    ctl[kCtlActive] = 1;
  }
}

// grid (ceil(n / 4)), 256 threads: one wavefront per row
__global__ __launch_bounds__(256) void k_cluster_discount(long long n, long long words, const int* __restrict__ ctl,
                                                          const u64* __restrict__ alive, const u64* __restrict__ members,
                                                          const u64* __restrict__ adj, int* __restrict__ count) {
  if (!ctl[kCtlActive]) return;
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n || !has_bit(alive, i)) return;
  int c = 0;
  for (long long w = lane; w < words; w += 64) {
    const u64 r = members[w];
    if (r) c += __popcll(adj[i * words + w] & r);
  }
  for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
  if (lane == 0 && c) count[i] -= c;
}

// ---- k-medoids: BUILD ----------------------------------------------------------------------------------------------------------
// grid (n), 256 threads.  first: gain = -sum_j dist[i, j] (the first medoid has the smallest sum), labels <- -1 and the NaN
// check; else gain = sum_j max(dn[j] - dist[i, j], 0).  j runs over the valid items.
__global__ __launch_bounds__(256) void k_kmed_gain(const double* __restrict__ dist, long long n, int k, int first,
                                                   const u64* __restrict__ valid, const int* __restrict__ is_medoid,
                                                   const double* __restrict__ dn, const int* __restrict__ ctl,
                                                   double* __restrict__ gain, int* __restrict__ labels, int* status) {
  __shared__ double red[4];
  const long long i = blockIdx.x;
  if (first) {
    if (threadIdx.x == 0) labels[i] = -1;
  } else if (status[kStFlag] || ctl[kCtlMedoids] >= k) {
    return;
  }
  if (!has_bit(valid, i) || (!first && is_medoid[i])) return;
  const double* row = dist + i * n;
  double v[1] = {0.0};
  bool nan_pair = false;
  for (long long j = threadIdx.x; j < n; j += 256) {
    if (!has_bit(valid, j)) continue;
    const double d = row[j];
    if (first) {
      nan_pair = nan_pair || d != d;
      v[0] += d;
    } else {
      const double t = dn[j] - d;
      v[0] += t > 0.0 ? t : 0.0;
    }
  }
  if (nan_pair) status[kStFlag] = 1;
  block_sum<1>(v, red);
  if (threadIdx.x == 0) gain[i] = first ? -v[0] : v[0];
}

// (value, index) of the workgroup's best entry in every thread; index n: none.  kMax: the largest value, else the smallest;
// the lowest index among equals.
template <bool kMax>
__device__ __forceinline__ void block_best(double& val, int& idx, int none, double* red_val, int* red_idx) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  auto take = [&](double ov, int oi) {
    if (oi == none) return;
    const bool better = idx == none || (kMax ? ov > val : ov < val) || (ov == val && oi < idx);
    if (better) {
      val = ov;
      idx = oi;
    }
  };
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(val, off);
    const int oi = __shfl_xor(idx, off);
    take(ov, oi);
  }
  __syncthreads();
  if (lane == 0) {
    red_val[wave] = val;
    red_idx[wave] = idx;
  }
  __syncthreads();
  val = red_val[0];
  idx = red_idx[0];
  for (int w = 1; w < nw; ++w) take(red_val[w], red_idx[w]);
}

// one workgroup: the candidate with the largest gain becomes the next medoid
__global__ __launch_bounds__(kPickThreads) void k_kmed_pick(long long n, int k, const u64* __restrict__ valid, int* is_medoid,
                                                            const double* __restrict__ gain, int* __restrict__ medoid, int* ctl,
                                                            int* status) {
  __shared__ double red_val[kPickThreads / 64];
  __shared__ int red_idx[kPickThreads / 64];
  const int placed = ctl[kCtlMedoids], flag = status[kStFlag];
  __syncthreads();
  if (flag || placed >= k) {
    if (threadIdx.x == 0) ctl[kCtlActive] = 0;
    return;
  }
  const int none = (int)n;
  double val = 0.0;
  int idx = none;
  for (long long i = threadIdx.x; i < n; i += kPickThreads)
    if (has_bit(valid, i) && !is_medoid[i]) {
      const double g = gain[i];
      if (idx == none || g > val) {
        val = g;
        idx = (int)i;
      }
    }
  block_best<true>(val, idx, none, red_val, red_idx);
  if (threadIdx.x == 0) {
    if (idx == none) {   // every valid item is a medoid already
      ctl[kCtlActive] = 0;
    } else {
      medoid[placed] = idx;
      is_medoid[idx] = 1;
      ctl[kCtlMedoids] = status[kStMedoids] = placed + 1;
      ctl[kCtlActive] = 1;
    }
  }
}

// grid (ceil(n / 256)), 256 threads: an item's nearest and second-nearest medoid along the medoids' rows.  incremental: the
// newest medoid against the stored state; else all of them from nothing.
__global__ __launch_bounds__(256) void k_kmed_assign(const double* __restrict__ dist, long long n, int incremental,
                                                     const u64* __restrict__ valid, const int* __restrict__ medoid,
                                                     const int* __restrict__ ctl, int* __restrict__ nearest,
                                                     double* __restrict__ dn, double* __restrict__ ds, int* __restrict__ labels) {
  if (!ctl[kCtlActive]) return;
  const int m = ctl[kCtlMedoids];
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  if (!has_bit(valid, j)) {
    nearest[j] = -1;
    return;
  }
  const int s0 = incremental ? m - 1 : 0;
  double a = pos_inf(), b = pos_inf();
  int near = -1;
  if (s0 > 0) {
    a = dn[j];
    b = ds[j];
    near = nearest[j];
  }
  for (int s = s0; s < m; ++s) {
    const double d = dist[(long long)medoid[s] * n + j];
    if (near < 0 || d < a) {
      b = a;
      a = d;
      near = s;
    } else if (d < b) {
      b = d;
    }
  }
  dn[j] = a;
  ds[j] = b;
  nearest[j] = near;
  labels[j] = near;
}

// one workgroup of kGroupWaves wavefronts.  after_build: runs unless the flag is set, and starts SWAP when there are two
// medoids or more; else runs when a swap was made.
__global__ __launch_bounds__(64 * kGroupWaves) void k_kmed_group(
    long long n, int k, int after_build, const int* __restrict__ ctl, int* status, const int* __restrict__ nearest,
    const double* __restrict__ dn, const double* __restrict__ ds, const int* __restrict__ medoid, int* __restrict__ order,
    int* __restrict__ seg, double* __restrict__ dn_o, double* __restrict__ ds_o, double* __restrict__ loss,
    double* __restrict__ seg_dn, int* __restrict__ reps, int* __restrict__ sizes, double* __restrict__ td, long long td_cap) {
  // a wavefront's items per slot, then its next free place per slot
  __shared__ __attribute__((aligned(8))) int hist[kGroupWaves][kMaxK];
  __shared__ int seg_s[kMaxK + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (after_build ? status[kStFlag] : !ctl[kCtlActive]) return;
  const int m = ctl[kCtlMedoids];
  if (m == 0) {   // no valid item: nothing was assigned, nothing to group
    for (int s = tid; s < k; s += 64 * kGroupWaves) {
      reps[s] = -1;
      sizes[s] = 0;
    }
    if (tid == 0) {
      seg[0] = 0;
      td[0] = 0.0;
      status[kStLeft] = 0;
    }
    return;
  }
  // wavefront w owns the items [w c, (w + 1) c), c a multiple of 64
  const long long chunk = ((n + kGroupWaves - 1) / kGroupWaves + 63) / 64 * 64;
  const long long lo = wave * chunk, hi = lo + chunk < n ? lo + chunk : n;
  for (int e = tid; e < kGroupWaves * kMaxK; e += 64 * kGroupWaves) (&hist[0][0])[e] = 0;
  __syncthreads();
  for (long long j = lo + lane; j < hi; j += 64) {
    const int s = nearest[j];
    if (s >= 0) atomicAdd(&hist[wave][s], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int at = 0;
    for (int s = 0; s < m; ++s) {
      seg_s[s] = at;
      for (int w = 0; w < kGroupWaves; ++w) {
        const int c = hist[w][s];
        hist[w][s] = at;
        at += c;
      }
    }
    seg_s[m] = at;
  }
  __syncthreads();
  for (int s = tid; s <= m; s += 64 * kGroupWaves) seg[s] = seg_s[s];
  for (int s = tid; s < k; s += 64 * kGroupWaves) {
    reps[s] = s < m ? medoid[s] : -1;
    sizes[s] = s < m ? seg_s[s + 1] - seg_s[s] : 0;
  }
  // stable placement: 64 items at a time, an item's rank among the lower lanes of its slot; a wavefront's LDS accesses
  // complete in program order
  volatile int* next = &hist[wave][0];
  for (long long j0 = lo; j0 < hi; j0 += 64) {
    const long long j = j0 + lane;
    const int s = j < hi ? nearest[j] : -1;
    int rank = 0, same = 0;
    for (int l = 0; l < 64; ++l) {
      const int sl = __shfl(s, l);
      same += sl == s;
      rank += sl == s && l < lane;
    }
    if (s >= 0) {
      const int pos = next[s] + rank;
      order[pos] = (int)j;
      dn_o[pos] = dn[j];
      ds_o[pos] = ds[j];
      __builtin_amdgcn_wave_barrier();
      if (rank == same - 1) next[s] = pos + 1;
    }
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();   // (the stores to dn_o / ds_o are visible to the workgroup)
  double* sums = reinterpret_cast<double*>(&hist[0][0]);   // (the places are used up; kGroupWaves kMaxK ints hold kMaxK doubles)
  for (int s = wave; s < m; s += kGroupWaves) {
    double a = 0.0, l = 0.0;
    for (int t = seg_s[s] + lane; t < seg_s[s + 1]; t += 64) {
      const double x = dn_o[t];
      a += x;
      l += ds_o[t] - x;
    }
    for (int off = 32; off >= 1; off >>= 1) {
      a += __shfl_xor(a, off);
      l += __shfl_xor(l, off);
    }
    if (lane == 0) {
      loss[s] = l;
      seg_dn[s] = a;
      sums[s] = a;
    }
  }
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    for (int s = 0; s < m; ++s) total += sums[s];
    const int done = status[kStDone];
    if (done < td_cap) td[done] = total;
    if (after_build) status[kStLeft] = m >= 2 ? 1 : 0;
  }
}

// ---- k-medoids: SWAP ------------------------------------------------------------------------------------------------------------
// grid (n), 256 threads, dynamic LDS cluster_eval_lds_bytes(form, n, k)
template <int kForm>
__global__ __launch_bounds__(256) void k_kmed_eval(const double* __restrict__ dist, long long n, const u64* __restrict__ valid,
                                                   const int* __restrict__ is_medoid, const int* __restrict__ ctl,
                                                   const int* __restrict__ status, const int* __restrict__ order,
                                                   const int* __restrict__ seg, const double* __restrict__ dn_o,
                                                   const double* __restrict__ ds_o, const double* __restrict__ loss,
                                                   double* __restrict__ best_delta, int* __restrict__ best_slot) {
  extern __shared__ double eval_lds[];
  __shared__ double red_val[4];
  __shared__ int red_idx[4];
  if (!status[kStLeft] || status[kStFlag]) return;
  const long long x = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (!has_bit(valid, x) || is_medoid[x]) {
    if (tid == 0) {
      best_delta[x] = pos_inf();
      best_slot[x] = 0;
    }
    return;
  }
  const int m = ctl[kCtlMedoids];
  double* shared_part = eval_lds;   // (m) a segment's sum of d - dn over the items that x would take
  double* own = eval_lds + m;       // (m) a segment's sum of the change for its own slot
  double* row_lds = eval_lds + 2 * m;
  const double* row = dist + x * n;
  if (kForm == sc_host::kClusterFormLds) {
    for (long long j = tid; j < n; j += 256) row_lds[j] = row[j];
    __syncthreads();
  }
  for (int s = wave; s < m; s += 4) {
    double a = 0.0, o = 0.0;
    const int t1 = seg[s + 1];
    for (int t = seg[s] + lane; t < t1; t += 64) {
      const int j = order[t];
      const double d = kForm == sc_host::kClusterFormLds ? row_lds[j] : row[j];
      const double near = dn_o[t], second = ds_o[t];
      if (d < near) {
        a += d - near;
        o += near - second;
      } else if (d < second) {
        o += d - second;
      }
    }
    for (int off = 32; off >= 1; off >>= 1) {
      a += __shfl_xor(a, off);
      o += __shfl_xor(o, off);
    }
    if (lane == 0) {
      shared_part[s] = a;
      own[s] = o;
    }
  }
  __syncthreads();
  double all = 0.0;
  for (int s = 0; s < m; ++s) all += shared_part[s];
  const int none = kMaxK + 1;
  double val = 0.0;
  int idx = none;
  for (int s = tid; s < m; s += 256) {
    const double delta = (loss[s] + own[s]) + all;
    if (idx == none || delta < val) {
      val = delta;
      idx = s;
    }
  }
  block_best<false>(val, idx, none, red_val, red_idx);
  if (tid == 0) {
    best_delta[x] = idx == none ? pos_inf() : val;
    best_slot[x] = idx == none ? 0 : idx;
  }
}

// one workgroup: the best row's swap, if it lowers the total deviation; else the run has converged
__global__ __launch_bounds__(kPickThreads) void k_kmed_swap(long long n, const double* __restrict__ best_delta,
                                                            const int* __restrict__ best_slot, int* __restrict__ medoid,
                                                            int* __restrict__ is_medoid, int* ctl, int* status) {
  __shared__ double red_val[kPickThreads / 64];
  __shared__ int red_idx[kPickThreads / 64];
  const int running = status[kStLeft], flag = status[kStFlag];
  __syncthreads();
  if (!running || flag) {
    if (threadIdx.x == 0) ctl[kCtlActive] = 0;
    return;
  }
  const int none = (int)n;
  double val = 0.0;
  int idx = none;
  for (long long x = threadIdx.x; x < n; x += kPickThreads) {
    const double d = best_delta[x];
    if (idx == none || d < val) {
      val = d;
      idx = (int)x;
    }
  }
  block_best<false>(val, idx, none, red_val, red_idx);
  if (threadIdx.x == 0) {
    if (idx != none && val < 0.0) {
      const int s = best_slot[idx];
      is_medoid[medoid[s]] = 0;
      is_medoid[idx] = 1;
      medoid[s] = idx;
      status[kStDone] = status[kStDone] + 1;
      ctl[kCtlActive] = 1;
    } else {
      status[kStLeft] = 0;
      ctl[kCtlActive] = 0;
    }
  }
}

}  // namespace

int launch_cluster_gromos_init(sc_ctx* ctx, const double* d_dist, int64_t n, double cutoff, const sc_host::ClusterBufs& B,
                               int32_t* d_labels, int32_t* d_status) {
  hipStream_t st = ctx->stream;
  const long long words = sc_host::cluster_words(n);
  hipLaunchKernelGGL(k_cluster_valid, dim3(1), dim3(kPickThreads), 0, st, d_dist, (long long)n, words, (u64*)B.valid,
                     (u64*)B.alive, -1, B.ctl, d_status);
  hipLaunchKernelGGL(k_cluster_pack, dim3((unsigned)n), dim3(256), 0, st, d_dist, (long long)n, words, cutoff,
                     (const u64*)B.valid, (u64*)B.adj, B.count, d_labels, d_status);
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

int launch_cluster_gromos_rounds(sc_ctx* ctx, int64_t n, int64_t rounds, int64_t max_clusters, const sc_host::ClusterBufs& B,
                                 int32_t* d_labels, int32_t* d_reps, int32_t* d_sizes, int32_t* d_status) {
  hipStream_t st = ctx->stream;
  const long long words = sc_host::cluster_words(n);
  for (int64_t r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(k_cluster_pick, dim3(1), dim3(kPickThreads), 0, st, (long long)n, words, (int)max_clusters, B.ctl,
                       (u64*)B.alive, (u64*)B.members, (const int*)B.count, (const u64*)B.adj, d_labels, d_reps, d_sizes,
                       d_status);
    hipLaunchKernelGGL(k_cluster_discount, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, (long long)n, words,
                       (const int*)B.ctl, (const u64*)B.alive, (const u64*)B.members, (const u64*)B.adj, B.count);
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

namespace {

void launch_group(hipStream_t st, int64_t n, int64_t k, int after_build, const sc_host::ClusterBufs& B, int32_t* d_reps,
                  int32_t* d_sizes, double* d_td, int64_t td_cap, int32_t* d_status) {
  hipLaunchKernelGGL(k_kmed_group, dim3(1), dim3(64 * kGroupWaves), 0, st, (long long)n, (int)k, after_build, (const int*)B.ctl,
                     d_status, (const int*)B.nearest, (const double*)B.dn, (const double*)B.ds, (const int*)B.medoid, B.order,
                     B.seg, B.dn_o, B.ds_o, B.loss, B.seg_dn, d_reps, d_sizes, d_td, (long long)td_cap);
}

void launch_assign(hipStream_t st, const double* d_dist, int64_t n, int incremental, const sc_host::ClusterBufs& B,
                   int32_t* d_labels) {
  hipLaunchKernelGGL(k_kmed_assign, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_dist, (long long)n, incremental,
                     (const u64*)B.valid, (const int*)B.medoid, (const int*)B.ctl, B.nearest, B.dn, B.ds, d_labels);
}

}  // namespace

int launch_cluster_kmedoids_init(sc_ctx* ctx, const double* d_dist, int64_t n, int64_t k, const sc_host::ClusterBufs& B,
                                 int32_t* d_labels, int32_t* d_reps, int32_t* d_sizes, double* d_td, int64_t td_cap,
                                 int32_t* d_status) {
  hipStream_t st = ctx->stream;
  const long long words = sc_host::cluster_words(n);
  SC_HIP(ctx, hipMemsetAsync(B.is_medoid, 0, sizeof(int32_t) * (size_t)n, st));
  hipLaunchKernelGGL(k_cluster_valid, dim3(1), dim3(kPickThreads), 0, st, d_dist, (long long)n, words, (u64*)B.valid,
                     (u64*)nullptr, 0, B.ctl, d_status);
  for (int64_t s = 0; s < k; ++s) {
    hipLaunchKernelGGL(k_kmed_gain, dim3((unsigned)n), dim3(256), 0, st, d_dist, (long long)n, (int)k, s == 0 ? 1 : 0,
                       (const u64*)B.valid, (const int*)B.is_medoid, (const double*)B.dn, (const int*)B.ctl, B.gain, d_labels,
                       d_status);
    hipLaunchKernelGGL(k_kmed_pick, dim3(1), dim3(kPickThreads), 0, st, (long long)n, (int)k, (const u64*)B.valid, B.is_medoid,
                       (const double*)B.gain, B.medoid, B.ctl, d_status);
    launch_assign(st, d_dist, n, 1, B, d_labels);
  }
  launch_group(st, n, k, 1, B, d_reps, d_sizes, d_td, td_cap, d_status);
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

int launch_cluster_kmedoids_swaps(sc_ctx* ctx, int form, const double* d_dist, int64_t n, int64_t k, int64_t iterations,
                                  const sc_host::ClusterBufs& B, int32_t* d_labels, int32_t* d_reps, int32_t* d_sizes,
                                  double* d_td, int64_t td_cap, int32_t* d_status) {
  hipStream_t st = ctx->stream;
  const size_t lds = sc_host::cluster_eval_lds_bytes(form, n, k);
  for (int64_t it = 0; it < iterations; ++it) {
    if (form == sc_host::kClusterFormLds)
      hipLaunchKernelGGL(k_kmed_eval<sc_host::kClusterFormLds>, dim3((unsigned)n), dim3(256), lds, st, d_dist, (long long)n,
                         (const u64*)B.valid, (const int*)B.is_medoid, (const int*)B.ctl, (const int*)d_status,
                         (const int*)B.order, (const int*)B.seg, (const double*)B.dn_o, (const double*)B.ds_o,
                         (const double*)B.loss, B.gain, B.best_slot);
    else
      hipLaunchKernelGGL(k_kmed_eval<sc_host::kClusterFormStream>, dim3((unsigned)n), dim3(256), lds, st, d_dist, (long long)n,
                         (const u64*)B.valid, (const int*)B.is_medoid, (const int*)B.ctl, (const int*)d_status,
                         (const int*)B.order, (const int*)B.seg, (const double*)B.dn_o, (const double*)B.ds_o,
                         (const double*)B.loss, B.gain, B.best_slot);
    hipLaunchKernelGGL(k_kmed_swap, dim3(1), dim3(kPickThreads), 0, st, (long long)n, (const double*)B.gain,
                       (const int*)B.best_slot, B.medoid, B.is_medoid, B.ctl, d_status);
    launch_assign(st, d_dist, n, 0, B, d_labels);
    launch_group(st, n, k, 0, B, d_reps, d_sizes, d_td, td_cap, d_status);
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}
