// C ABI (include/springcraft_hip.h), ragged / decorated batches: sc_batch_plan (the struct is in api_internal.h) -- the
// blob builder, assembly, contact scan, pair lists, fill from pairs and the range / window solves of its padded slots.
// Its mode consumers are in api_batch_modes.hip.
#include <algorithm>
#include <cstring>
#include <map>
#include <new>

#include "api_internal.h"

using sc_host::Arena;

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

// Contact scan of every structure: counts per atom + their exclusive scan in the context's scratch, carved together with
// the caller's `rest`; the per-structure offsets of the pair list (count + 1) come back to `pair_off`.  Leaves d_off
// (atoms + 1 entries) valid in scratch.
int plan_scan(sc_batch_plan* plan, const double* d_coord, const ScratchLayout& rest, int64_t** d_off_out,
              std::vector<int64_t>& pair_off) {
  sc_ctx* ctx = plan->ctx;
  const int64_t atoms = plan->atom_off.back();
  int64_t *d_counts = nullptr, *d_off = nullptr;
  SC_TRY(carve_scratch(ctx, [&](Arena& a) {
    d_counts = a.take<int64_t>((size_t)atoms);
    d_off = a.take<int64_t>((size_t)atoms + 1);
    rest(a);
  }));
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
    sc_host::HostPatch hp;
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

void sc_batch_plan_destroy(sc_batch_plan* plan) {
  if (!plan) return;
  (void)hipSetDevice(plan->ctx->device);
  (void)hipStreamSynchronize(plan->ctx->stream);
  if (plan->d_blob) (void)hipFree(plan->d_blob);
  delete plan;
}

int64_t sc_batch_plan_order(const sc_batch_plan* plan) { return plan ? plan->order : 0; }

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

int sc_batch_plan_contacts(sc_batch_plan* plan, const double* d_coord, int64_t* n_pairs) {
  if (!plan) return SC_ERR_INVALID_ARG;
  sc_ctx* ctx = plan->ctx;
  if (!d_coord || !n_pairs) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  int64_t* d_off = nullptr;
  std::vector<int64_t> pair_off;
  SC_TRY(plan_scan(plan, d_coord, [](Arena&) {}, &d_off, pair_off));
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
  int64_t *d_off = nullptr, *d_pairs = nullptr;
  double* d_sq = nullptr;
  std::vector<int64_t> off;
  SC_TRY(plan_scan(plan, d_coord, [&](Arena& a) {
    d_pairs = a.take<int64_t>((size_t)capacity * 2 + 2);
    d_sq = sq_dist ? a.take<double>((size_t)capacity + 1) : nullptr;
  }, &d_off, off));
  for (int64_t b = 0; b <= plan->count; ++b) pair_off[b] = off[(size_t)b];
  const int64_t k = off.back();
  if (k > capacity)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pair buffer too small: %lld > %lld", (long long)k, (long long)capacity);
  if (k == 0) return SC_OK;
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
  int64_t *d_poff = nullptr, *d_pairs = nullptr;
  double* d_g = nullptr;
  SC_TRY(carve_scratch(ctx, [&](Arena& a) {
    d_poff = a.take<int64_t>((size_t)plan->count + 1);
    d_pairs = a.take<int64_t>((size_t)k * 2 + 2);
    d_g = a.take<double>((size_t)k + 1);
  }));
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

}  // extern "C"
