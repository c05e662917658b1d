// Debug / tuning entries of the three float64 GEMM launchers (include/springcraft_hip_debug.h; not part of the public C
// ABI): one launch on host data for the GPU unit tests (tests/test_gemm_gpu.py, tests/test_gemm_records_gpu.py) and timed
// launches on buffers of their own for tools/*.py.  They go through launch_gemm_f64 / launch_gemm3_uniform / launch_symm3
// like every other caller and state what they force in the launch description (GemmOverrides).  The stamp and trace readers
// stay with the kernels whose __device__ symbols they read.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "gemm_f64.h"
#include "springcraft_hip_debug.h"

namespace {
// the first error of an entry: HIP calls after it still run (they free, or fail again), launches are skipped by the entry
struct FirstError {
  sc_ctx* ctx;
  int rc = SC_OK;
  void operator()(hipError_t e) { if (e != hipSuccess && rc == SC_OK) rc = sc_set_error(ctx, SC_ERR_HIP, "%s", hipGetErrorString(e)); }
};

// `count` records of one shape on a fresh device arena: count x ea doubles of A, count x eb of B, count x ec of C, the records
struct Shape {
  sc_ctx* ctx;
  int count;
  size_t ea, eb, ec;
  FirstError fail{ctx};
  char* base = nullptr;
  double *a = nullptr, *b = nullptr, *c = nullptr;
  GemmDesc* d = nullptr;
  ~Shape() { (void)hipFree(base); }
  int alloc() {
    SC_HIP(ctx, hipSetDevice(ctx->device));
    SC_HIP(ctx, hipMalloc((void**)&base, (ea + eb + ec) * count * 8 + sizeof(GemmDesc) * (size_t)count + 256));
    a = (double*)base; b = a + ea * count; c = b + eb * count;
    d = (GemmDesc*)(c + ec * count);
    return SC_OK;
  }
  // the same operands in [-1, 1] for every A and B (random: the clock a launch holds depends on what the matrix pipes
  // multiply -- zeros run ~10 % faster)
  void fill_random() {
    std::vector<double> hv(std::max(ea, eb));
    unsigned long long s = 88172645463325252ull;
    for (auto& x : hv) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; x = (double)((long long)(s % 2001) - 1000) / 1000.0; }
    for (int z = 0; z < count; ++z) {
      fail(hipMemcpy(a + ea * z, hv.data(), ea * 8, hipMemcpyHostToDevice));
      fail(hipMemcpy(b + eb * z, hv.data(), eb * 8, hipMemcpyHostToDevice));
    }
  }
  // record z = D with its operands moved on to the z-th A, B and C
  void upload(GemmDesc D) {
    std::vector<GemmDesc> h((size_t)count);
    for (int z = 0; z < count; ++z) {
      D.a = a + ea * z; D.b = b + eb * z; D.c = c + ec * z;
      h[(size_t)z] = D;
    }
    fail(hipMemcpy(d, h.data(), sizeof(GemmDesc) * (size_t)count, hipMemcpyHostToDevice));
  }
  // `warm` launches, then `iters` launches between two events: *ms_out = ms per launch.  launch() returns an SC_* code.
  template <class Launch>
  int time(int warm, int iters, double* ms_out, Launch&& launch) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    fail(hipEventCreate(&e0));
    fail(hipEventCreate(&e1));
    for (int it = 0; it < warm && fail.rc == SC_OK; ++it) fail.rc = launch();
    fail(hipEventRecord(e0, ctx->stream));
    for (int it = 0; it < iters && fail.rc == SC_OK; ++it) fail.rc = launch();
    fail(hipEventRecord(e1, ctx->stream));
    fail(hipEventSynchronize(e1));
    float ms = 0.f;
    if (fail.rc == SC_OK) fail(hipEventElapsedTime(&ms, e0, e1));
    if (ms_out) *ms_out = ms / iters;
    for (hipEvent_t e : {e0, e1}) if (e) (void)hipEventDestroy(e);
    return fail.rc;
  }
};

// ONE record on host data through k_gemm2, launched once; then(S, L) runs with the result in c and returns the entry's code.
// mode: 0 = NN (A m x k col-major, B k x n col-major), 1 = NT lower-only (SYR2K shape: B stored n x k), 2 = TN (A stored
// k x m); c: m x n column-major, in / out, the K slices summed on the host.
// tile 10 .. 13: 10: automatic block tile, 11: 128 x 128, 12: 128 x 64, 13: 64 x 64
template <class Then>
int run_mode_record(sc_ctx* ctx, const double* a, const double* b, double* c, int m, int n, int k, int mode, int tile,
                    int split_k, double alpha, double beta, bool lower_grid, Then&& then) {
  const int slices = std::max(split_k, 1);
  const size_t mn = (size_t)m * n;
  Shape S{ctx, 1, (size_t)m * std::max(k, 1), (size_t)std::max(k, 1) * n, mn * slices};
  SC_TRY(S.alloc());
  if (k > 0) { S.fail(hipMemcpy(S.a, a, (size_t)m * k * 8, hipMemcpyHostToDevice)); S.fail(hipMemcpy(S.b, b, (size_t)k * n * 8, hipMemcpyHostToDevice)); }
  for (int sl = 0; sl < slices; ++sl) S.fail(hipMemcpy(S.c + sl * mn, c, mn * 8, hipMemcpyHostToDevice));
  GemmDesc D{};
  D.m = m; D.n = n; D.k = k; D.ldc = m; D.alpha = alpha; D.beta = beta;
  if (mode == 0) { D.sa_i = 1; D.sa_k = m; D.sb_k = 1; D.sb_j = k; }
  if (mode == 1) { D.sa_i = 1; D.sa_k = m; D.sb_k = n; D.sb_j = 1; D.lower_only = 1; }
  if (mode == 2) { D.sa_i = k; D.sa_k = 1; D.sb_k = 1; D.sb_j = k; }
  D.split_stride = (long long)mn;
  S.upload(D);
  if (S.fail.rc != SC_OK) return S.fail.rc;
  if (tile < 10 || tile > 13) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "tile id %d (10 .. 13)", tile);
  const GemmLaunch L{.count = 1, .max_m = m, .max_n = n, .layout = mode == 0 ? kGemmAmBk : (mode == 1 ? kGemmAmBn : kGemmAkBk),
                     .split_k = split_k, .lower_grid = lower_grid, .dbg = {.force_tile = tile - 10}};
  S.fail.rc = launch_gemm_f64(ctx, S.d, L);
  S.fail(hipStreamSynchronize(ctx->stream));
  std::vector<double> h(S.ec);
  if (S.fail.rc == SC_OK) S.fail(hipMemcpy(h.data(), S.c, S.ec * 8, hipMemcpyDeviceToHost));
  if (S.fail.rc != SC_OK) return S.fail.rc;
  if (slices == 1) std::copy(h.begin(), h.end(), c);
  else
    for (size_t i = 0; i < mn; ++i) {
      double sum = 0.0;
      for (int sl = 0; sl < slices; ++sl) sum += h[sl * mn + i];
      c[i] = sum;
    }
  return then(S, L);
}

// the record of the k_gemm3 entries: A m x k (lda), or k x m for kGemmAkBk; B n x k (ldbn) for kGemmAmBn, else k x n; C (ldc)
GemmDesc gemm3_record(int m, int n, int k, int layout, int lower, double beta, int lda, int ldbn, int ldc) {
  GemmDesc D{};
  D.m = m; D.n = n; D.k = k; D.ldc = ldc; D.alpha = 1.0; D.beta = beta;
  D.sa_i = 1; D.sa_k = lda;
  if (layout == kGemmAkBk) { D.sa_i = k; D.sa_k = 1; }
  if (layout == kGemmAmBn) { D.sb_k = ldbn; D.sb_j = 1; } else { D.sb_k = 1; D.sb_j = k; }
  D.lower_only = lower;
  return D;
}
// the record of the k_symm3 entries: A m x m, V and X m x 64, the K slices of X behind each other
GemmDesc symm3_record(int m) {
  GemmDesc D{};
  D.m = m; D.n = 64; D.k = m; D.ldc = m; D.alpha = 1.0; D.beta = 0.0;
  D.sa_i = 1; D.sa_k = m; D.sb_k = 1; D.sb_j = m;
  D.split_stride = (long long)m * 64;
  return D;
}
}  // namespace

// ---- Times `iters` launches of one GEMM shape on random operands (mode, tile: run_mode_record) and checks the first.
extern "C" int sc_dbg_gemm_bench(sc_ctx* ctx, int m, int n, int k, int mode, int tile, int split_k, int iters,
                                 int beta_one, double* ms_out, double* max_err_out) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  std::vector<double> ha((size_t)m * k), hb((size_t)k * n), hc((size_t)m * n, 0.0);
  unsigned long long s = 88172645463325252ull;
  auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)((long long)(s % 2001) - 1000) / 1000.0; };
  for (auto& x : ha) x = rnd();
  for (auto& x : hb) x = rnd();
  return run_mode_record(ctx, ha.data(), hb.data(), hc.data(), m, n, k, mode, tile, split_k, 1.0, beta_one ? 1.0 : 0.0,
                         mode == 1 && m == n, [&](Shape& S, const GemmLaunch& L) {
    // spot check 64 entries of the first launch against a host dot product (beta path: C was 0 before it), then the timing
    double maxerr = 0.0;
    for (int t = 0; t < 64; ++t) {
      int i = (int)((t * 7919ull) % m), j = (int)((t * 104729ull) % n);
      if (mode == 1 && i < j) { int tmp = i; i = j; j = tmp; if (i >= m || j >= n) continue; }
      double ref = 0.0;
      for (int kk = 0; kk < k; ++kk) {
        const double av = mode == 2 ? ha[(size_t)i * k + kk] : ha[(size_t)kk * m + i];
        const double bv = mode == 1 ? hb[(size_t)kk * n + j] : hb[(size_t)j * k + kk];
        ref += av * bv;
      }
      maxerr = fmax(maxerr, fabs(hc[(size_t)j * m + i] - ref));
    }
    if (max_err_out) *max_err_out = maxerr;
    return S.time(0, iters, ms_out, [&] { return launch_gemm_f64(ctx, S.d, L); });
  });
}

// ---- debug entry point for the GPU unit tests of the launch paths (tests/test_gemm_gpu.py): ONE launch of one record
// on host data.  a, b as sc_dbg_gemm_bench lays them out for `mode`; c: m x n column-major, in / out (with split_k > 1
// the slices are summed into c on the host and beta must be 0).  lower_grid as launch_gemm_f64 takes it.  alpha == 0
// with beta != 0 is refused (gemm_f64.h).
extern "C" int sc_dbg_gemm_host(sc_ctx* ctx, const double* a, const double* b, double* c, int m, int n, int k, int mode,
                                int tile, int split_k, double alpha, double beta, int lower_grid) {
  if (!ctx || !a || !b || !c || m <= 0 || n <= 0 || k < 0 || split_k < 1) return SC_ERR_INVALID_ARG;
  if (split_k > 1 && beta != 0.0) return SC_ERR_INVALID_ARG;
  if (alpha == 0.0 && beta != 0.0) return SC_ERR_INVALID_ARG;   // not a record the kernel takes (gemm_f64.h)
  return run_mode_record(ctx, a, b, c, m, n, k, mode, tile, split_k, alpha, beta, lower_grid != 0,
                         [](Shape&, const GemmLaunch&) { return (int)SC_OK; });
}

// ---- debug entry point for the GPU unit tests of the record-level launch paths (tests/test_gemm_records_gpu.py): ONE
// launch_gemm_f64 call on records the host describes -- triangular operands, gather lists, grouped launches, sub-matrix
// views, chunked record lists.  Operands live in one arena of doubles (in / out: copied whole to the device and whole
// back), index lists in one arena of ints; a record holds element offsets into them in place of pointers.  Nothing is
// launched unless every address a record can make the kernel touch lies inside its arena.
static_assert(sizeof(sc_dbg_gemm_record) == 144, "the tests mirror this layout as a NumPy record type");
namespace {
constexpr long long kRecGuard = 4096;                // doubles in front of and behind the device copy of the arena
constexpr unsigned long long kRecGuardBits = 0x7ff8a5a5a5a5a5a5ull;   // a quiet NaN that no operand holds

// nullptr, or what is wrong with record r of the launch
const char* gemm_record_problem(const sc_dbg_gemm_record& R, long long arena_len, const int* idx, long long idx_len,
                                const GemmLaunch& L) {
  typedef __int128 wide;
  if (R.m < 0 || R.n < 0 || R.k < 0) return "negative size";
  if (R.m > L.max_m || R.n > L.max_n) return "larger than max_m x max_n";
  if (R.sa_i < 0 || R.sa_k < 0 || R.sb_k < 0 || R.sb_j < 0 || R.ldc < 0 || R.split_stride < 0) return "negative stride";
  if (L.layout == kGemmAmBk && (R.sa_i != 1 || R.sb_k != 1)) return "strides do not match layout kGemmAmBk";
  if (L.layout == kGemmAkBk && (R.sa_k != 1 || R.sb_k != 1)) return "strides do not match layout kGemmAkBk";
  if (L.layout == kGemmAmBn && (R.sa_i != 1 || R.sb_j != 1)) return "strides do not match layout kGemmAmBn";
  if (R.lower_only < 0 || R.lower_only > 2) return "lower_only not 0, 1 or 2";
  if (R.a_tri < 0 || R.a_tri > 2 || (R.a_tri != 0 && !L.tri)) return "a_tri without a tri launch, or not 0, 1 or 2";
  if (!L.gather && (R.a_kidx != -1 || R.b_kidx != -1 || R.c_jidx != -1)) return "index list without a gather launch";
  if (R.alpha == 0.0 && R.beta != 0.0) return "alpha == 0 with beta != 0";
  if (!(R.alpha == R.alpha) || !(R.beta == R.beta)) return "alpha or beta is NaN";
  if (L.lower_grid && (R.lower_only == 0 || R.row_off != 0 || R.col_off != 0)) return "lower_grid needs lower_only records without offsets";
  if (R.a < 0 || R.a > arena_len || R.b < 0 || R.b > arena_len || R.c < 0 || R.c > arena_len) return "operand offset outside the arena";
  // index lists: [off, off + length) inside the int arena, entries >= 0; *last = the largest entry
  auto list = [&](long long off, int len, long long* last) -> bool {
    *last = (long long)len - 1;
    if (off == -1) return true;
    if (off < 0 || off > idx_len || (long long)len > idx_len - off) return false;
    long long mx = -1;
    for (int t = 0; t < len; ++t) {
      if (idx[off + t] < 0) return false;
      mx = std::max<long long>(mx, idx[off + t]);
    }
    *last = mx;
    return true;
  };
  long long ka = 0, kb = 0, jc = 0;
  if (!list(R.a_kidx, R.k, &ka) || !list(R.b_kidx, R.k, &kb) || !list(R.c_jidx, R.n, &jc))
    return "index list outside the int arena, or with a negative entry";
  if (R.m == 0 || R.n == 0) return nullptr;   // every workgroup of the record exits before it touches an operand
  if (R.ldc < R.m) return "ldc < m";
  if (R.k > 0) {
    if ((wide)R.a + (wide)(R.m - 1) * R.sa_i + (wide)ka * R.sa_k >= (wide)arena_len) return "A reaches outside the arena";
    if ((wide)R.b + (wide)kb * R.sb_k + (wide)(R.n - 1) * R.sb_j >= (wide)arena_len) return "B reaches outside the arena";
  }
  if ((wide)R.c + (wide)(L.split_k - 1) * R.split_stride + (wide)jc * R.ldc + (R.m - 1) >= (wide)arena_len)
    return "C reaches outside the arena";
  return nullptr;
}
}  // namespace

extern "C" int sc_dbg_gemm_records_host(sc_ctx* ctx, double* arena, long long arena_len, const int* idx, long long idx_len,
                                        const sc_dbg_gemm_record* recs, int count, int max_m, int max_n, int split_k,
                                        int gather, int tri, int layout, int lower_grid, int tile) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (!arena || arena_len <= 0 || arena_len > (1ll << 34) || idx_len < 0 || idx_len > (1ll << 34) || (idx_len > 0 && !idx) ||
      !recs || count < 0 || count > (1 << 24) || max_m <= 0 || max_n <= 0 || split_k < 1 || split_k > 65535)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "GEMM records: bad launch argument");
  if (tile < 10 || tile > 13) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "tile id %d (10 .. 13)", tile);
  if (layout < 0 || layout > 2 || (gather && (tri || layout != kGemmAmBk)) || (tri && layout == kGemmAmBn))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "GEMM records: no kernel for layout %d, gather %d, tri %d", layout, gather, tri);
  if (lower_grid && (layout != kGemmAmBn || tri || gather || split_k > 1 || max_m != max_n))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "GEMM records: lower_grid is for square launches of layout kGemmAmBn without split-K");
  const GemmLaunch L{.count = count, .max_m = max_m, .max_n = max_n, .layout = layout, .split_k = split_k, .gather = gather != 0,
                     .tri = tri != 0, .lower_grid = lower_grid != 0, .dbg = {.force_tile = tile - 10}};
  for (int r = 0; r < count; ++r) {
    const char* what = gemm_record_problem(recs[r], arena_len, idx, idx_len, L);
    if (what) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "GEMM record %d: %s", r, what);
  }
  SC_HIP(ctx, hipSetDevice(ctx->device));
  // device image: [guard | arena | guard] [records] [index lists], each part on a 256-byte boundary
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t b_arena = up((size_t)(arena_len + 2 * kRecGuard) * 8), b_desc = up((size_t)std::max(count, 1) * sizeof(GemmDesc));
  const size_t b_idx = up((size_t)std::max<long long>(idx_len, 1) * 4);
  char* base = nullptr;
  SC_HIP(ctx, hipMalloc((void**)&base, b_arena + b_desc + b_idx));
  double *d_front = (double*)base, *d_arena = d_front + kRecGuard, *d_back = d_arena + arena_len;
  GemmDesc* d_desc = (GemmDesc*)(base + b_arena);
  int* d_idx = (int*)(base + b_arena + b_desc);
  FirstError fail{ctx};
  std::vector<unsigned long long> guard((size_t)kRecGuard, kRecGuardBits), got((size_t)kRecGuard);
  fail(hipMemcpy(d_front, guard.data(), (size_t)kRecGuard * 8, hipMemcpyHostToDevice));
  fail(hipMemcpy(d_back, guard.data(), (size_t)kRecGuard * 8, hipMemcpyHostToDevice));
  fail(hipMemcpy(d_arena, arena, (size_t)arena_len * 8, hipMemcpyHostToDevice));
  if (idx_len > 0) fail(hipMemcpy(d_idx, idx, (size_t)idx_len * 4, hipMemcpyHostToDevice));
  std::vector<GemmDesc> h_desc((size_t)count);
  for (int r = 0; r < count; ++r) {
    const sc_dbg_gemm_record& R = recs[r];
    GemmDesc& D = h_desc[(size_t)r];
    D = GemmDesc{};
    D.a = d_arena + R.a; D.b = d_arena + R.b; D.c = d_arena + R.c;
    D.m = R.m; D.n = R.n; D.k = R.k;
    D.sa_i = R.sa_i; D.sa_k = R.sa_k; D.sb_k = R.sb_k; D.sb_j = R.sb_j; D.ldc = R.ldc;
    D.alpha = R.alpha; D.beta = R.beta;
    D.a_kidx = R.a_kidx >= 0 ? d_idx + R.a_kidx : nullptr;
    D.b_kidx = R.b_kidx >= 0 ? d_idx + R.b_kidx : nullptr;
    D.c_jidx = R.c_jidx >= 0 ? d_idx + R.c_jidx : nullptr;
    D.lower_only = R.lower_only; D.row_off = R.row_off; D.col_off = R.col_off;
    D.split_stride = R.split_stride; D.a_tri = R.a_tri;
  }
  if (count > 0) fail(hipMemcpy(d_desc, h_desc.data(), (size_t)count * sizeof(GemmDesc), hipMemcpyHostToDevice));
  if (fail.rc == SC_OK) {
    fail.rc = launch_gemm_f64(ctx, d_desc, L);
    fail(hipStreamSynchronize(ctx->stream));
  }
  if (fail.rc == SC_OK) fail(hipMemcpy(arena, d_arena, (size_t)arena_len * 8, hipMemcpyDeviceToHost));
  for (double* g : {d_front, d_back}) {
    if (fail.rc != SC_OK) break;
    fail(hipMemcpy(got.data(), g, (size_t)kRecGuard * 8, hipMemcpyDeviceToHost));
    if (fail.rc == SC_OK && got != guard) fail.rc = sc_set_error(ctx, SC_ERR_HIP, "GEMM records: the launch wrote outside the arena");
  }
  (void)hipFree(base);
  return fail.rc;
}

// ---- debug entry for the GPU unit tests (tests/test_gemm_gpu.py): `count` products of one shape on host data through
// k_gemm3, whatever their size.  a: count x (m x k) column-major (kGemmAkBk: k x m); b: count x (k x n) column-major
// (layout kGemmAmBk) or count x (n x k) column-major (kGemmAmBn); c: count x (m x n) column-major, in / out.
// Returns SC_OK, or SC_ERR_INVALID_ARG when the kernel does not take the shape.
extern "C" int sc_dbg_gemm3_host(sc_ctx* ctx, const double* a, const double* b, double* c, int count, int m, int n, int k,
                                 int layout, int lower, double beta) {
  if (!ctx || !a || !b || !c || count < 1 || m < 1 || n < 1 || k < 1) return SC_ERR_INVALID_ARG;
  Shape S{ctx, count, (size_t)m * k, (size_t)k * n, (size_t)m * n};
  SC_TRY(S.alloc());
  S.fail(hipMemcpy(S.a, a, S.ea * count * 8, hipMemcpyHostToDevice));
  S.fail(hipMemcpy(S.b, b, S.eb * count * 8, hipMemcpyHostToDevice));
  S.fail(hipMemcpy(S.c, c, S.ec * count * 8, hipMemcpyHostToDevice));
  S.upload(gemm3_record(m, n, k, layout, lower, beta, m, n, m));
  if (S.fail.rc == SC_OK) {
    const int took = launch_gemm3_uniform(ctx, S.d, {.count = count, .m = m, .n = n, .k = k, .layout = layout, .lower = lower, .alpha = 1.0,
                                                     .beta = beta, .aligned16 = true, .dbg = {.any_size = true}});
    if (took != SC_OK) S.fail.rc = sc_set_error(ctx, SC_ERR_INVALID_ARG, "k_gemm3 does not take m %d n %d k %d layout %d", m, n, k, layout);
    S.fail(hipStreamSynchronize(ctx->stream));
  }
  if (S.fail.rc == SC_OK) S.fail(hipMemcpy(c, S.c, S.ec * count * 8, hipMemcpyDeviceToHost));
  return S.fail.rc;
}

// ---- debug / tuning entry: `count` matrices of one shape on freshly allocated buffers, timed through k_gemm3 (kernel 3;
// order: its tile order) or k_gemm2 (kernel 2) with the SAME records.  C += A B, or with lower != 0 the lower triangle of
// it (m == n).  tools/gemm3_shapes.py
extern "C" int sc_dbg_gemm3_bench(sc_ctx* ctx, int count, int m, int n, int k, int layout, int lower, int kernel, int order,
                                  int iters, double* ms_out) {
  if (!ctx || count < 1 || iters < 1) return SC_ERR_INVALID_ARG;
  // (experiments: leading dimensions of A / C and of an n-contiguous B other than m / n)
  static const int ld_a = [] { const char* e = getenv("SC_DBG_LDA"); return e ? atoi(e) : 0; }();
  static const int ld_c = [] { const char* e = getenv("SC_DBG_LDC"); return e ? atoi(e) : 0; }();
  static const int ld_b = [] { const char* e = getenv("SC_DBG_LDB"); return e ? atoi(e) : 0; }();
  const int lda = std::max(m, ld_a), ldc = std::max(m, ld_c), ldbn = std::max(n, ld_b);
  Shape S{ctx, count, (size_t)lda * k, layout == kGemmAmBn ? (size_t)ldbn * k : (size_t)k * n, (size_t)ldc * n};
  SC_TRY(S.alloc());
  S.fill_random();
  S.fail(hipMemset(S.c, 0, S.ec * count * 8));
  S.upload(gemm3_record(m, n, k, layout, lower, 1.0, lda, ldbn, ldc));
  if (S.fail.rc != SC_OK) return S.fail.rc;
  return S.time(2, iters, ms_out, [&]() -> int {
    if (kernel != 3)
      return launch_gemm_f64(ctx, S.d, {.count = count, .max_m = m, .max_n = n, .layout = layout, .lower_grid = lower != 0 && layout == kGemmAmBn});
    const int took = launch_gemm3_uniform(ctx, S.d, {.count = count, .m = m, .n = n, .k = k, .layout = layout, .lower = lower, .alpha = 1.0,
                                                     .beta = 1.0, .aligned16 = true, .dbg = {.any_size = true, .order = order}});
    return took == SC_OK ? SC_OK : SC_ERR_INVALID_ARG;
  });
}

// ---- debug entry for the GPU unit tests (tests/test_gemm_gpu.py): x = sym(a) v for `count` matrices on host data.
// a: count x (m x m) column-major, only (row | 1) >= col is read; v, x: count x (m x 64).
extern "C" int sc_dbg_symm3_host(sc_ctx* ctx, const double* a, const double* v, double* x, int count, int m, int split) {
  if (!ctx || !a || !v || !x || count < 1 || m < 1 || split < 1) return SC_ERR_INVALID_ARG;
  const size_t ev = (size_t)m * 64;
  Shape S{ctx, count, (size_t)m * m, ev, ev * split};
  SC_TRY(S.alloc());
  S.fail(hipMemcpy(S.a, a, S.ea * count * 8, hipMemcpyHostToDevice));
  S.fail(hipMemcpy(S.b, v, ev * count * 8, hipMemcpyHostToDevice));
  S.fail(hipMemset(S.c, 0xff, S.ec * count * 8));
  S.upload(symm3_record(m));
  if (S.fail.rc == SC_OK) {
    const int took = launch_symm3(ctx, S.d, count, m, split, /*aligned16=*/true, /*any_size=*/true);
    if (took != SC_OK) S.fail.rc = sc_set_error(ctx, SC_ERR_INVALID_ARG, "k_symm3 does not take m %d split %d", m, split);
    S.fail(hipStreamSynchronize(ctx->stream));
  }
  if (S.fail.rc == SC_OK) {
    // the slices summed on the host
    std::vector<double> hx(S.ec * count);
    S.fail(hipMemcpy(hx.data(), S.c, hx.size() * 8, hipMemcpyDeviceToHost));
    for (int z = 0; z < count; ++z)
      for (size_t e = 0; e < ev; ++e) {
        double s = 0.0;
        for (int q = 0; q < split; ++q) s += hx[(size_t)z * S.ec + (size_t)q * ev + e];
        x[(size_t)z * ev + e] = s;
      }
  }
  return S.fail.rc;
}

// ---- debug / tuning entry: `count` matrices of order m on freshly allocated buffers, X = A V timed through k_symm3.
// tools/symm3_bench.py
extern "C" int sc_dbg_symm3_bench(sc_ctx* ctx, int count, int m, int split, int iters, double* ms_out) {
  if (!ctx || count < 1 || iters < 1 || m < 256) return SC_ERR_INVALID_ARG;
  Shape S{ctx, count, (size_t)m * m, (size_t)m * 64, (size_t)m * 64 * split};
  SC_TRY(S.alloc());
  S.fill_random();
  S.upload(symm3_record(m));
  if (S.fail.rc != SC_OK) return S.fail.rc;
  return S.time(2, iters, ms_out, [&] {
    return launch_symm3(ctx, S.d, count, m, split, /*aligned16=*/true, /*any_size=*/true) == SC_OK ? SC_OK : SC_ERR_INVALID_ARG;
  });
}
