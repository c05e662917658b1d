// Dense Cholesky factorisation A = L L^T and triangular solves with the factor, float64, for `batch` symmetric positive
// definite matrices of one order n: lower triangle, column-major (as the GEMM's C), leading dimension ld, matrix stride
// `stride`.  The block plan, the records per step and the scratch are potrf_policy.h's; this file holds the kernels and turns
// the plan into launches.
//
// k_diag_block<true> factors one diagonal block of w <= 64 columns in LDS, one workgroup per matrix: column by column,
// pivot test first (a pivot <= 0 or NaN fails the matrix), and inverts the factor of the block into a side buffer.  With the
// inverses the panel solve below the block and every later triangular solve are products on launch_gemm_f64 with strided
// views of the factor; the trailing updates are its lower_only / lower_grid SYRK form (alpha = -1, beta = 1).  No product reads
// the panel it writes: the panel product goes to a side buffer and is copied back.
//
// The strict upper triangle of A is never written and no result depends on it: k_diag_block does not read it; the SYRK form
// loads the C tile it owns, the elements above the diagonal of a diagonal tile included, and stores only the lower ones.
//
// Failure: the first failing column + 1 goes to the matrix' info word (LAPACK's info) and the matrix' number + 1 to word
// kStatusPotrf of the context's status block, both by plain stores of the one workgroup that owns the matrix at that step
// (several failing matrices store different numbers to the status word; any of them reports the failure).  The failed block
// and its inverse become NaN, the products carry the NaN into every later column, and k_fail_fill sets the earlier ones: the
// whole lower triangle of a failed matrix is NaN, and so is everything solved with it.  The other matrices of the batch are
// not touched: every step works per matrix, on one workgroup or one GEMM record, and the GEMM's block tile is pinned by the
// shape of ONE matrix (gemm_f64_tile with a count of one), so a matrix' bits do not depend on the batch or its place in it.
// Nothing here synchronises with the host, and there are no atomics.
#include "gemm_f64.h"
#include "potrf_internal.h"

namespace {

constexpr int NB = sc_host::kPotrfInner;
constexpr int LDS_LD = NB + 1;   // L(i, k) at S[i * 65 + k], k <= i; inv(i, t) at S[t * 65 + i + 1], i >= t: the two triangles of one array

// One workgroup: block blockIdx.x of the launch (first column c0 + 64 blockIdx.x) of matrix blockIdx.y.
// FACTOR: the block is factored in place first and the info / status words are kept; else it is read as a factor.
// dinv: (batch, nblk, 64, 64) column-major, the strict upper triangle and the rows / columns behind w are 0.
template <bool FACTOR>
__global__ __launch_bounds__(256) void k_diag_block(double* __restrict__ a, long long ld, long long stride, int c0, int n,
                                                    double* __restrict__ dinv, int nblk, long long* __restrict__ info,
                                                    unsigned long long* __restrict__ status) {
  __shared__ double S[NB * LDS_LD];
  __shared__ int s_fail;
  const int tid = threadIdx.x;
  const long long b = blockIdx.y;
  const int c = c0 + NB * (int)blockIdx.x;
  if (c >= n) return;
  const int w = min(NB, n - c);
  double* A = a + b * stride + c + (long long)c * ld;
  double* D = dinv + (b * nblk + c / NB) * (long long)(NB * NB);
  const bool dead = FACTOR && info[b] != 0;   // (an earlier block of this matrix failed)

  for (int idx = tid; idx < NB * NB; idx += 256) {
    const int i = idx & (NB - 1), k = idx >> 6;
    if (i < w && k <= i) S[i * LDS_LD + k] = A[i + (long long)k * ld];
  }
  if (tid == 0) s_fail = -1;
  __syncthreads();

  if (FACTOR && !dead) {
    const int i = tid & (NB - 1), q = tid >> 6;
    for (int j = 0; j < w; ++j) {
      if (tid == 0) {
        const double p = S[j * LDS_LD + j];
        if (p > 0.0) S[j * LDS_LD + j] = sqrt(p);
        else s_fail = j;   // (NaN included)
      }
      __syncthreads();
      if (s_fail >= 0) break;
      if (q == 0 && i > j && i < w) S[i * LDS_LD + j] /= S[j * LDS_LD + j];
      __syncthreads();
      if (i > j && i < w) {
        const double lij = S[i * LDS_LD + j];
        for (int k = j + 1 + q; k <= i; k += 4) S[i * LDS_LD + k] -= lij * S[k * LDS_LD + j];
      }
      __syncthreads();
    }
  }
  const int fail = s_fail;
  const bool bad = dead || fail >= 0;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);

  if (FACTOR) {
    for (int idx = tid; idx < NB * NB; idx += 256) {
      const int i = idx & (NB - 1), k = idx >> 6;
      if (i < w && k <= i) A[i + (long long)k * ld] = bad ? nan : S[i * LDS_LD + k];
    }
    if (!dead && fail >= 0 && tid == 0) {
      info[b] = 1 + c + fail;
      status[kStatusPotrf] = (unsigned long long)(b + 1);
    }
  }
  if (bad) {
    for (int idx = tid; idx < NB * NB; idx += 256) D[idx] = nan;
    return;
  }

  // column t of the inverse by forward substitution, thread t: it reads the factor and its own earlier entries only
  if (tid < w) {
    const int t = tid;
    for (int i = t; i < w; ++i) {
      double s = i == t ? 1.0 : 0.0;
      for (int k = t; k < i; ++k) s -= S[i * LDS_LD + k] * S[t * LDS_LD + k + 1];
      S[t * LDS_LD + i + 1] = s / S[i * LDS_LD + i];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < NB * NB; idx += 256) {
    const int i = idx & (NB - 1), k = idx >> 6;
    D[idx] = (i < w && k <= i) ? S[k * LDS_LD + i + 1] : 0.0;
  }
}

// dst (rows, cols) <- src, both column-major; grid (row chunks, column groups, batch)
__global__ __launch_bounds__(256) void k_copy_block(const double* __restrict__ src, long long lds, long long src_stride,
                                                    double* __restrict__ dst, long long ldd, long long dst_stride, int rows,
                                                    int cols) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const double* s = src + blockIdx.z * src_stride;
  double* d = dst + blockIdx.z * dst_stride;
  for (int col = blockIdx.y; col < cols; col += gridDim.y) d[r + (long long)col * ldd] = s[r + (long long)col * lds];
}

// the lower triangle of every failed matrix <- NaN; grid (groups of 64 columns, batch)
__global__ __launch_bounds__(256) void k_fail_fill(double* __restrict__ a, long long ld, long long stride, int n,
                                                   const long long* __restrict__ info) {
  const long long b = blockIdx.y;
  if (info[b] == 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double* A = a + b * stride;
  const int c1 = min(n, ((int)blockIdx.x + 1) * NB);
  for (int col = blockIdx.x * NB; col < c1; ++col)
    for (int row = col + threadIdx.x; row < n; row += 256) A[row + (long long)col * ld] = nan;
}

// `batch` records of one product: operand pointers advance by their matrix strides
struct Records {
  std::vector<GemmDesc> h;
  int64_t batch;
  void add(const double* a, long long a_step, long long sa_i, long long sa_k, const double* b, long long b_step,
           long long sb_k, long long sb_j, double* c, long long c_step, long long ldc, int m, int n, int k, double alpha,
           double beta, int lower_only) {
    for (int64_t x = 0; x < batch; ++x) {
      GemmDesc G{};
      G.a = a + x * a_step; G.sa_i = sa_i; G.sa_k = sa_k;
      G.b = b + x * b_step; G.sb_k = sb_k; G.sb_j = sb_j;
      G.c = c + x * c_step; G.ldc = ldc;
      G.m = m; G.n = n; G.k = k;
      G.alpha = alpha; G.beta = beta;
      G.lower_only = lower_only;
      h.push_back(G);
    }
  }
};

int gemm_step(sc_ctx* ctx, const GemmDesc* d_desc, int64_t batch, int m, int n, int layout, bool lower_grid = false) {
  return launch_gemm_f64(ctx, d_desc, {.count = (int)batch, .max_m = m, .max_n = n, .layout = layout, .lower_grid = lower_grid,
                                      .pin_tile = gemm_f64_tile(ctx, 1, m, n, layout)});
}

void copy_block(hipStream_t st, const double* src, long long lds, long long src_stride, double* dst, long long ldd,
                long long dst_stride, int rows, int cols, int64_t batch) {
  const dim3 grid((unsigned)((rows + 255) / 256), (unsigned)std::min(cols, 4096), (unsigned)batch);
  hipLaunchKernelGGL(k_copy_block, grid, dim3(256), 0, st, src, lds, src_stride, dst, ldd, dst_stride, rows, cols);
}

}  // namespace

size_t potrf_desc_bytes() { return sizeof(GemmDesc); }

int potrf_outer_block(int64_t n) {
  const char* e = getenv("SPRINGCRAFT_POTRF_OUTER");   // (read at every call: the block-size sweep switches it)
  return sc_host::potrf_outer_block(n, e ? atoi(e) : 0);
}

int launch_potrf(sc_ctx* ctx, const sc_host::PotrfBufs& B, double* d_a, int64_t n, int64_t ld, int64_t stride,
                 int64_t batch, int outer, long long* d_info) {
  using namespace sc_host;
  hipStream_t st = ctx->stream;
  const std::vector<PotrfOp> ops = potrf_plan(n, outer);
  const int nblk = (int)potrf_blocks(n);
  const long long dinv_step = (long long)nblk * NB * NB, panel_step = (long long)n * NB;

  Records R{{}, batch};
  for (const PotrfOp& o : ops) {
    const double* l21 = d_a + o.r0 + (long long)o.c * ld;
    if (o.kind == kPotrfPanel)   // panel(i, j) = sum_k A(r0 + i, c + k) inv(j, k)
      R.add(l21, stride, 1, ld, B.dinv + (long long)(o.c / NB) * NB * NB, dinv_step, NB, 1, B.panel, panel_step, n, o.rows,
            o.w, o.w, 1.0, 0.0, 0);
    else if (o.kind == kPotrfUpdate)   // A(r0 + i, r0 + j) -= sum_k A(r0 + i, c + k) A(r0 + j, c + k), i >= j
      R.add(l21, stride, 1, ld, l21, stride, ld, 1, d_a + o.r0 + (long long)o.r0 * ld, stride, ld, o.rows, o.cols, o.w, -1.0,
            1.0, 1);
  }
  GemmDesc* d_desc = reinterpret_cast<GemmDesc*>(B.descs);
  SC_TRY(sc_stage_upload(ctx, d_desc, R.h.data(), R.h.size() * sizeof(GemmDesc)));
  SC_HIP(ctx, hipMemsetAsync(d_info, 0, sizeof(long long) * (size_t)batch, st));

  size_t r = 0;
  for (const PotrfOp& o : ops) {
    if (o.kind == kPotrfDiag) {
      hipLaunchKernelGGL(k_diag_block<true>, dim3(1, (unsigned)batch), dim3(256), 0, st, d_a, (long long)ld,
                         (long long)stride, o.c, (int)n, B.dinv, nblk, d_info, ctx->d_status);
    } else if (o.kind == kPotrfPanel) {
      SC_TRY(gemm_step(ctx, d_desc + r, batch, o.rows, o.w, kGemmAmBn));
      copy_block(st, B.panel, n, panel_step, d_a + o.r0 + (long long)o.c * ld, ld, stride, o.rows, o.w, batch);
      r += (size_t)batch;
    } else {
      SC_TRY(gemm_step(ctx, d_desc + r, batch, o.rows, o.cols, kGemmAmBn, o.rows == o.cols));
      r += (size_t)batch;
    }
  }
  hipLaunchKernelGGL(k_fail_fill, dim3((unsigned)nblk, (unsigned)batch), dim3(256), 0, st, d_a, (long long)ld,
                     (long long)stride, (int)n, (const long long*)d_info);
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}

int launch_trsm(sc_ctx* ctx, const sc_host::TrsmBufs& B, int pass, int kind, const double* d_l, int64_t n, int64_t ld,
                int64_t stride, int64_t batch, double* d_b, int64_t vectors, int64_t ldb, int64_t strideb) {
  using namespace sc_host;
  hipStream_t st = ctx->stream;
  const int nblk = (int)potrf_blocks(n), nv = (int)vectors;
  const long long dinv_step = (long long)nblk * NB * NB, tmp_step = (long long)vectors * NB;
  const std::vector<TrsmStep> steps = trsm_steps(n, kind != kTrsmBackward);
  // T of a block step: (w, q) with leading dimension 64 for the left solves, (rows, w) with leading dimension rows
  const long long ldt = kind == kTrsmRight ? vectors : NB;

  if (pass == 0)   // the inverses of the factor's diagonal blocks (a failed factor is NaN, and so are they)
    hipLaunchKernelGGL(k_diag_block<false>, dim3((unsigned)nblk, (unsigned)batch), dim3(256), 0, st,
                       const_cast<double*>(d_l), (long long)ld, (long long)stride, 0, (int)n, B.dinv, nblk,
                       (long long*)nullptr, (unsigned long long*)nullptr);

  Records R{{}, batch};
  for (const TrsmStep& s : steps) {
    const double* inv = B.dinv + (long long)(s.c / NB) * NB * NB;
    if (kind == kTrsmForward) {
      R.add(inv, dinv_step, 1, NB, d_b + s.c, strideb, 1, ldb, B.tmp, tmp_step, ldt, s.w, nv, s.w, 1.0, 0.0, 0);
      R.add(d_l + s.rest0 + (long long)s.c * ld, stride, 1, ld, B.tmp, tmp_step, 1, ldt, d_b + s.rest0, strideb, ldb, s.rest,
            nv, s.w, -1.0, 1.0, 0);
    } else if (kind == kTrsmBackward) {
      R.add(inv, dinv_step, NB, 1, d_b + s.c, strideb, 1, ldb, B.tmp, tmp_step, ldt, s.w, nv, s.w, 1.0, 0.0, 0);
      R.add(d_l + s.c, stride, ld, 1, B.tmp, tmp_step, 1, ldt, d_b, strideb, ldb, s.rest, nv, s.w, -1.0, 1.0, 0);
    } else {
      R.add(d_b + (long long)s.c * ldb, strideb, 1, ldb, inv, dinv_step, NB, 1, B.tmp, tmp_step, ldt, nv, s.w, s.w, 1.0, 0.0, 0);
      R.add(B.tmp, tmp_step, 1, ldt, d_l + s.rest0 + (long long)s.c * ld, stride, ld, 1, d_b + (long long)s.rest0 * ldb,
            strideb, ldb, nv, s.rest, s.w, -1.0, 1.0, 0);
    }
  }
  GemmDesc* d_desc = reinterpret_cast<GemmDesc*>(B.descs) + (size_t)pass * trsm_record_count(n, batch);
  SC_TRY(sc_stage_upload(ctx, d_desc, R.h.data(), R.h.size() * sizeof(GemmDesc)));

  const int layout = kind == kTrsmForward ? kGemmAmBk : (kind == kTrsmBackward ? kGemmAkBk : kGemmAmBn);
  size_t r = 0;
  for (const TrsmStep& s : steps) {
    if (kind == kTrsmRight) {
      SC_TRY(gemm_step(ctx, d_desc + r, batch, nv, s.w, layout));
      copy_block(st, B.tmp, ldt, tmp_step, d_b + (long long)s.c * ldb, ldb, strideb, nv, s.w, batch);
      if (s.rest > 0) SC_TRY(gemm_step(ctx, d_desc + r + batch, batch, nv, s.rest, layout));
    } else {
      SC_TRY(gemm_step(ctx, d_desc + r, batch, s.w, nv, layout));
      copy_block(st, B.tmp, ldt, tmp_step, d_b + s.c, ldb, strideb, s.w, nv, batch);
      if (s.rest > 0) SC_TRY(gemm_step(ctx, d_desc + r + batch, batch, s.rest, nv, layout));
    }
    r += 2 * (size_t)batch;
  }
  SC_HIP(ctx, hipGetLastError());
  return SC_OK;
}
