// Host-only logic of the Cholesky solver and the subsystem reduction (springcraft_amd/csrc/potrf_policy.h, scratch_arena.h)
// under AddressSanitizer + UBSan:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I springcraft_amd/csrc \
//       tests/host_sanitize/test_potrf_policy.cpp -o /tmp/test_potrf_policy && /tmp/test_potrf_policy
// (built and run by tests/test_subsystem_host.py::test_potrf_policy_under_sanitizers).
//
// The plan is replayed on a small integer model of the matrix: every entry of the lower triangle counts the K columns that
// were subtracted from it and whether its column was solved; a correct plan subtracts columns 0 .. j - 1 from entry (i, j)
// exactly once each, before the column's diagonal block is factored and its panel solved, and never touches the strict upper
// triangle.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "potrf_policy.h"
#include "scratch_arena.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); std::exit(1); } } while (0)

using namespace sc_host;

static void replay(int n, int outer) {
  const std::vector<PotrfOp> ops = potrf_plan(n, outer);
  std::vector<int> sub((size_t)n * n, 0);      // columns subtracted from (i, j), column-major
  std::vector<char> done((size_t)n * n, 0);    // the entry holds its final value of L
  int next_diag = 0;
  size_t records = 0;
  for (const PotrfOp& o : ops) {
    if (o.kind == kPotrfDiag) {
      CHECK(o.c == next_diag && o.w >= 1 && o.w <= kPotrfInner && o.c + o.w <= n);
      CHECK(o.c % kPotrfInner == 0 && (o.w == kPotrfInner || o.c + o.w == n));
      for (int j = o.c; j < o.c + o.w; ++j)
        for (int i = j; i < o.c + o.w; ++i) {
          CHECK(sub[(size_t)j * n + i] == o.c && !done[(size_t)j * n + i]);   // (the block's own columns are its kernel's)
          done[(size_t)j * n + i] = 1;
        }
      next_diag = o.c + o.w;
    } else if (o.kind == kPotrfPanel) {
      ++records;
      CHECK(o.r0 == o.c + o.w && o.r0 + o.rows == n && o.rows >= 1 && o.c + o.w == next_diag);
      for (int j = o.c; j < o.c + o.w; ++j)
        for (int i = o.r0; i < n; ++i) {
          CHECK(sub[(size_t)j * n + i] == o.c && !done[(size_t)j * n + i]);
          done[(size_t)j * n + i] = 1;
        }
    } else {
      ++records;
      CHECK(o.kind == kPotrfUpdate && o.w >= 1 && o.c + o.w <= o.r0 && o.r0 + o.rows == n && o.cols >= 1 && o.cols <= o.rows);
      for (int k = o.c; k < o.c + o.w; ++k)   // the K columns are final, on all rows the product reads
        for (int i = o.r0; i < n; ++i) CHECK(done[(size_t)k * n + i]);
      for (int j = o.r0; j < o.r0 + o.cols; ++j)
        for (int i = j; i < n; ++i) {
          CHECK(!done[(size_t)j * n + i] && sub[(size_t)j * n + i] == o.c);   // columns are subtracted in order, once
          sub[(size_t)j * n + i] += o.w;
        }
    }
  }
  CHECK(next_diag == n);
  for (int j = 0; j < n; ++j)
    for (int i = j; i < n; ++i) CHECK(done[(size_t)j * n + i]);
  CHECK(potrf_record_count(ops, 1) == records && potrf_record_count(ops, 3) == 3 * records);
}

static void check_steps(int n) {
  for (bool up : {true, false}) {
    const std::vector<TrsmStep> s = trsm_steps(n, up);
    CHECK((int64_t)s.size() == potrf_blocks(n));
    int covered = 0;
    for (size_t t = 0; t < s.size(); ++t) {
      const TrsmStep& x = s[t];
      CHECK(x.w >= 1 && x.w <= kPotrfInner && x.c % kPotrfInner == 0 && x.c + x.w <= n);
      if (up) CHECK(x.c == covered && x.rest0 == x.c + x.w && x.rest0 + x.rest == n);
      else CHECK(x.c + x.w == n - covered && x.rest0 == 0 && x.rest == x.c);
      covered += x.w;
    }
    CHECK(covered == n);
  }
  CHECK(trsm_record_count(n, 3) == 6 * (size_t)potrf_blocks(n));
}

int main() {
  CHECK(potrf_outer_block(100, 0) == 512 && potrf_outer_block(24000, 0) == 512 && kPotrfOuter % kPotrfInner == 0);
  CHECK(potrf_outer_block(5000, 256) == 256 && potrf_outer_block(5000, 100) == 64 && potrf_outer_block(5000, 1) == 64);
  CHECK(potrf_outer_block(5000, 300) == 256 && potrf_outer_block(5000, -3) == 512);
  CHECK(potrf_blocks(1) == 1 && potrf_blocks(64) == 1 && potrf_blocks(65) == 2 && potrf_blocks(24000) == 375);

  for (int n : {1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257, 513, 1030})
    for (int outer : {64, 128, 256, 512}) replay(n, outer);
  for (int n : {1, 2, 63, 64, 65, 129, 200, 1030}) check_steps(n);

  // ---- scratch: carved buffers lie inside the block, aligned, in order, and can be written end to end
  const size_t desc = 136;
  for (int n : {1, 65, 1030})
    for (int batch : {1, 3}) {
      const std::vector<PotrfOp> ops = potrf_plan(n, 128);
      const size_t rec = potrf_record_count(ops, batch);
      Arena m;
      potrf_layout(m, n, batch, rec, desc);
      std::vector<char> block(m.bytes());
      Arena c(block.data(), block.size());
      const PotrfBufs B = potrf_layout(c, n, batch, rec, desc);
      CHECK(!c.overrun() && c.bytes() == m.bytes());
      const size_t dinv = sizeof(double) * batch * potrf_blocks(n) * 64 * 64, panel = sizeof(double) * batch * n * 64;
      CHECK((char*)B.dinv == block.data() && (char*)B.dinv + dinv <= (char*)B.panel && (char*)B.panel + panel <= B.descs);
      CHECK(B.descs + rec * desc <= block.data() + block.size());
      for (size_t i = 0; i < dinv / 8; ++i) B.dinv[i] = 1.0;
      for (size_t i = 0; i < panel / 8; ++i) B.panel[i] = 2.0;
      for (size_t i = 0; i < rec * desc; ++i) B.descs[i] = 3;
      CHECK(potrf_scratch_bytes(n, batch, 128, desc) >= m.bytes());

      for (int passes : {1, 2})
        for (int q : {1, 70}) {
          Arena tm;
          trsm_layout(tm, n, batch, q, passes, desc);
          std::vector<char> tb(tm.bytes());
          Arena tc(tb.data(), tb.size());
          const TrsmBufs T = trsm_layout(tc, n, batch, q, passes, desc);
          CHECK(!tc.overrun() && tc.bytes() == tm.bytes());
          const size_t tmp = sizeof(double) * batch * q * 64, recs = passes * trsm_record_count(n, batch) * desc;
          CHECK((char*)T.dinv + dinv <= (char*)T.tmp && (char*)T.tmp + tmp <= T.descs && T.descs + recs <= tb.data() + tb.size());
          for (size_t i = 0; i < tmp / 8; ++i) T.tmp[i] = 4.0;
          for (size_t i = 0; i < recs; ++i) T.descs[i] = 5;
        }
    }
  {
    // one structure reduces on the batched layout with batch = 1
    Arena m;
    batch_reduce_layout(m, 387, 63, 1, 128, desc);
    // the bytes of the single solver's own layout for (me 387, ms 63, outer 128, 136-byte records) before it was merged
    // into this one, computed once from that revision's potrf_policy.h on the host: the merged carve is the same takes
    CHECK(m.bytes() == 693128);
    std::vector<char> block(m.bytes());
    Arena c(block.data(), block.size());
    const BatchReduceBufs R = batch_reduce_layout(c, 387, 63, 1, 128, desc);
    CHECK(!c.overrun() && c.bytes() == m.bytes());
    CHECK(!c.overrun() && R.potrf.dinv && R.trsm.tmp && R.descs && R.descs + desc <= block.data() + block.size());
    CHECK(R.potrf.descs < (char*)R.trsm.dinv && R.trsm.descs < R.descs);
    Arena fm;
    follow_layout(fm, 387, 5, desc);
    std::vector<char> fb(fm.bytes());
    Arena fc(fb.data(), fb.size());
    const FollowBufs F = follow_layout(fc, 387, 5, desc);
    CHECK(!fc.overrun() && F.trsm.dinv && F.desc + desc <= fb.data() + fb.size());
  }
  CHECK(reduce_flops(3.0, 2.0) == 9.0 + 18.0 + 12.0);
  std::printf("potrf policy ok\n");
  return 0;
}
