// Host-only logic of the batched subsystem reduction (springcraft_amd/csrc/potrf_policy.h, scratch_arena.h) under
// AddressSanitizer + UBSan:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I springcraft_amd/csrc \
//       tests/host_sanitize/test_subsystem_batch_policy.cpp -o /tmp/test_subsystem_batch_policy && /tmp/test_subsystem_batch_policy
// (built and run by tests/test_subsystem_batch_host.py::test_batch_policy_under_sanitizers).
//
// Slot order, shape and member refusals, the extents of the assembly grids, and the scratch carve of the reduction for the
// environment orders of the test family (0, 1, 21, 22, 44 atoms) and batches of 1, 5 and 65535 members.  The carve of 65535
// members is measured and its arithmetic checked, not allocated; the smaller ones are carved and written end to end.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "potrf_policy.h"
#include "scratch_arena.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); std::exit(1); } } while (0)

using namespace sc_host;

static std::vector<SubMember> family(int64_t n_s, const std::vector<int64_t>& n_e, int64_t pairs_per_atom) {
  std::vector<SubMember> m;
  int64_t atom0 = 0, pair0 = 0;
  for (int64_t e : n_e) {
    const int64_t n = n_s + e;
    m.push_back({atom0, n, pair0, n * pairs_per_atom, e});
    atom0 += n;
    pair0 += n * pairs_per_atom;
  }
  return m;
}

static size_t up(size_t x) { return (x + 255) / 256 * 256; }

int main() {
  const size_t desc = 136;
  const int64_t n_s = 12;
  static_assert(sizeof(SubMember) == 5 * sizeof(int64_t), "a member is five int64");

  // ---- slot order and the refusals of the shapes
  for (int dim : {1, 3})
    for (int64_t eo : {0, 1, 21, 22, 44}) CHECK(sub_slot_order(dim, eo) == dim * eo);
  CHECK(sub_batch_shape_error(3, n_s, 44, 5) == 0 && sub_batch_shape_error(1, 1, 0, 1) == 0);
  CHECK(sub_batch_shape_error(3, n_s, 0, kSubBatchMax) == 0);
  CHECK(sub_batch_shape_error(2, n_s, 44, 5) == 1 && sub_batch_shape_error(0, n_s, 44, 5) == 1);
  CHECK(sub_batch_shape_error(3, 0, 44, 5) == 2 && sub_batch_shape_error(3, -1, 44, 5) == 2);
  CHECK(sub_batch_shape_error(3, n_s, 44, 0) == 3 && sub_batch_shape_error(3, n_s, 44, 65536) == 3);
  CHECK(sub_batch_shape_error(3, n_s, -1, 5) == 4);
  CHECK(sub_batch_shape_error(3, kPotrfMaxOrder, 1, 1) == 5 && sub_batch_shape_error(3, 1, kPotrfMaxOrder, 1) == 5);

  // ---- the members of the test family, and every way a member can fail to fit
  const std::vector<int64_t> envs = {0, 1, 21, 22, 44};
  std::vector<SubMember> mem = family(n_s, envs, 7);
  CHECK(sub_batch_member_error(mem.data(), 5, n_s, 44) == -1);
  CHECK(sub_batch_member_error(mem.data(), 5, n_s, 50) == -1);     // a larger slot is allowed
  CHECK(sub_batch_member_error(mem.data(), 5, n_s, 43) == 4);      // n_e above env_order
  CHECK(sub_batch_member_error(mem.data(), 4, n_s, 22) == -1 && sub_batch_member_error(mem.data(), 4, n_s, 21) == 3);
  CHECK(sub_batch_member_error(mem.data(), 1, n_s, 0) == -1);      // exactly the core
  CHECK(sub_batch_max_pairs(mem.data(), 5) == 56 * 7 && sub_batch_max_pairs(mem.data(), 1) == 12 * 7);
  {
    std::vector<SubMember> bad = mem;
    bad[2].n_atoms += 1;                                           // n_s + n_e != n_atoms
    CHECK(sub_batch_member_error(bad.data(), 5, n_s, 44) == 2);
    bad = mem; bad[1].n_e = -1;
    CHECK(sub_batch_member_error(bad.data(), 5, n_s, 44) == 1);
    bad = mem; bad[3].n_pairs = -5;
    CHECK(sub_batch_member_error(bad.data(), 5, n_s, 44) == 3);
    bad = mem; bad[3].atom0 += 1;                                  // not packed back to back
    CHECK(sub_batch_member_error(bad.data(), 5, n_s, 44) == 3);
    bad = mem; bad[0].pair0 = 4;
    CHECK(sub_batch_member_error(bad.data(), 5, n_s, 44) == 0);
  }
  {
    const std::vector<SubMember> none = family(n_s, {0, 0}, 0);    // no pairs at all
    CHECK(sub_batch_member_error(none.data(), 2, n_s, 0) == -1 && sub_batch_max_pairs(none.data(), 2) == 0);
  }
  // every atom thread of a member lands on an atom or on a pad atom of its slot, and every pad atom has a thread
  for (int64_t eo : {0, 1, 21, 22, 44, 50})
    for (int64_t e : envs) {
      if (e > eo) continue;
      const int64_t threads = sub_batch_atom_threads(n_s, eo), n = n_s + e;
      CHECK(threads == n + (eo - e));
      for (int64_t i = n; i < threads; ++i) CHECK(e + (i - n) >= e && e + (i - n) < eo);
    }

  // ---- the scratch of the reduction
  CHECK(batch_reduce_scratch_bytes(0, 36, 5, 512, desc) == 0 && batch_reduce_scratch_bytes(0, 12, 65535, 512, desc) == 0);
  for (int dim : {1, 3})
    for (int64_t eo : {1, 21, 22, 44})
      for (int64_t batch : {(int64_t)1, (int64_t)5, kSubBatchMax}) {
        const int64_t me = sub_slot_order(dim, eo), ms = dim * n_s;
        const int outer = potrf_outer_block(me, 0);
        const size_t rec = potrf_record_count(potrf_plan(me, outer), batch), blocks = (size_t)potrf_blocks(me);
        Arena m;
        batch_reduce_layout(m, me, ms, batch, outer, desc);
        CHECK(m.bytes() == batch_reduce_scratch_bytes(me, ms, batch, outer, desc));
        // the sum of the takes, each on its 256-byte boundary (an empty take occupies one byte)
        const size_t dinv = sizeof(double) * batch * blocks * 64 * 64;
        size_t want = 0;
        for (size_t bytes : {dinv, sizeof(double) * batch * me * 64, rec * desc, dinv, sizeof(double) * batch * ms * 64,
                             (size_t)trsm_record_count(me, batch) * desc, (size_t)batch * desc})
          want = up(want) + (bytes ? bytes : 1);
        CHECK(m.bytes() == want);
        if (batch == kSubBatchMax) continue;
        std::vector<char> block(m.bytes());
        Arena c(block.data(), block.size());
        const BatchReduceBufs R = batch_reduce_layout(c, me, ms, batch, outer, desc);
        CHECK(!c.overrun() && c.bytes() == m.bytes());
        CHECK((char*)R.potrf.dinv == block.data() && (char*)R.potrf.dinv + dinv <= (char*)R.potrf.panel);
        CHECK(R.potrf.descs + rec * desc <= (char*)R.trsm.dinv && (char*)R.trsm.dinv + dinv <= (char*)R.trsm.tmp);
        CHECK((char*)R.trsm.tmp + sizeof(double) * batch * ms * 64 <= R.trsm.descs);
        CHECK(R.trsm.descs + trsm_record_count(me, batch) * desc <= R.descs && R.descs + batch * desc <= block.data() + block.size());
        std::memset(R.potrf.dinv, 1, dinv);
        std::memset(R.potrf.panel, 2, sizeof(double) * batch * me * 64);
        std::memset(R.potrf.descs, 3, rec * desc);
        std::memset(R.trsm.dinv, 4, dinv);
        std::memset(R.trsm.tmp, 5, sizeof(double) * batch * ms * 64);
        std::memset(R.trsm.descs, 6, trsm_record_count(me, batch) * desc);
        std::memset(R.descs, 7, batch * desc);
        CHECK(*(block.data()) == 1 && *(R.descs + batch * desc - 1) == 7 && *(R.trsm.descs - 1) != 6);
      }
  for (int64_t batch : {(int64_t)1, (int64_t)5, kSubBatchMax}) {
    Arena m;
    batch_blocks_layout(m, batch);
    CHECK(m.bytes() == (size_t)batch * sizeof(SubMember));
    if (batch == kSubBatchMax) continue;
    std::vector<char> block(m.bytes());
    Arena c(block.data(), block.size());
    const BatchBlocksBufs B = batch_blocks_layout(c, batch);
    CHECK(!c.overrun() && B.members == block.data());
    std::memset(B.members, 9, (size_t)batch * sizeof(SubMember));
  }
  // the pad's price: nothing for a full slot, the whole slot for a member without environment
  CHECK(reduce_pad_flops(132.0, 132.0, 36.0) == 0.0 && reduce_pad_flops(132.0, 0.0, 36.0) == reduce_flops(132.0, 36.0));
  std::printf("subsystem batch policy ok\n");
  return 0;
}
