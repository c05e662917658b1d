// C ABI (include/springcraft_hip.h), one model: host -> device staging of its inputs, the host entries (contacts, pairs,
// Kirchhoff / Hessian, eigensolves, pseudo-inverse, fused ANM / GNM solves) and the thin sc_dev_* assembly / eigh entries.
// All arithmetic lives in assembly.hip / the eigensolver units.
#include <cstring>

#include "api_internal.h"

using sc_host::Arena;
using sc_host::HostPatch;

int check_ff(sc_ctx* ctx, const sc_ff_desc* ff) {
  std::string err;
  const int rc = sc_host::check_ff(ff, err);
  return rc == SC_OK ? SC_OK : sc_set_error(ctx, rc, "%s", err.c_str());
}

int build_patch(sc_ctx* ctx, const sc_patch_desc* pd, int64_t n, HostPatch& hp) {
  std::string err;
  const int rc = sc_host::build_patch(pd, n, hp, err);
  return rc == SC_OK ? SC_OK : sc_set_error(ctx, rc, "%s", err.c_str());
}

int check_coord_args(sc_ctx* ctx, const double* coord, int64_t n) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (n < 0 || n > 2000000) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad atom count %lld", (long long)n);
  if (n > 0 && !coord) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "coord is NULL");
  return SC_OK;
}

namespace {

// Device tables of a tabulated force field, in the order stage_inputs takes them
struct TabBufs { double* edges; float* tab; int32_t* type; int32_t* chain; uint8_t* bond; };

int upload_patch(sc_ctx* ctx, const HostPatch& hp, const HostPatch::Bufs& d, PatchDev& dev) {
  SC_HIP(ctx, hipMemcpyAsync(d.shut, hp.shut.data(), hp.shut.size(), hipMemcpyHostToDevice, ctx->stream));
  SC_HIP(ctx, hipMemcpyAsync(d.rp, hp.row_ptr.data(), hp.row_ptr.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  if (!hp.col.empty()) {
    SC_HIP(ctx, hipMemcpyAsync(d.col, hp.col.data(), hp.col.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(d.flag, hp.flag.data(), hp.flag.size(), hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(d.gam, hp.gam.data(), hp.gam.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  // the source vectors must outlive the async copies
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  dev = PatchDev{d.shut, d.rp, d.col, d.flag, d.gam, hp.mask_gamma};
  return SC_OK;
}

// Upload the tabulated force-field tables; st.ff_dev is what the kernel launchers must be given.
int upload_tab(sc_ctx* ctx, const sc_ff_desc* ff, int64_t n, const TabBufs& d, Staged& st) {
  st.ff_dev = *ff;
  if (ff->kind != SC_FF_TABULATED) return SC_OK;
  const sc_tab_desc* t = ff->tab;
  const size_t nb = (size_t)t->n_bins;
  for (int64_t i = 0; i < n; ++i)
    if (t->atom_type[i] < 0 || t->atom_type[i] >= 20)
      return sc_set_error(ctx, SC_ERR_INDEX, "amino-acid type %d of atom %lld out of range", t->atom_type[i],
                          (long long)i);
  hipStream_t s = ctx->stream;
  if (t->edges_sq) SC_HIP(ctx, hipMemcpyAsync(d.edges, t->edges_sq, nb * 8, hipMemcpyHostToDevice, s));
  SC_HIP(ctx, hipMemcpyAsync(d.tab, t->bonded, 400 * nb * 4, hipMemcpyHostToDevice, s));
  SC_HIP(ctx, hipMemcpyAsync(d.tab + 400 * nb, t->intra_chain, 400 * nb * 4, hipMemcpyHostToDevice, s));
  SC_HIP(ctx, hipMemcpyAsync(d.tab + 800 * nb, t->inter_chain, 400 * nb * 4, hipMemcpyHostToDevice, s));
  SC_HIP(ctx, hipMemcpyAsync(d.type, t->atom_type, (size_t)n * 4, hipMemcpyHostToDevice, s));
  SC_HIP(ctx, hipMemcpyAsync(d.chain, t->chain, (size_t)n * 4, hipMemcpyHostToDevice, s));
  SC_HIP(ctx, hipMemcpyAsync(d.bond, t->bonded_next, (size_t)n, hipMemcpyHostToDevice, s));
  SC_HIP(ctx, hipStreamSynchronize(s));
  st.tab_dev = *t;
  st.tab_dev.edges_sq = d.edges;
  st.tab_dev.bonded = d.tab;
  st.tab_dev.intra_chain = d.tab + 400 * nb;
  st.tab_dev.inter_chain = d.tab + 800 * nb;
  st.tab_dev.atom_type = d.type;
  st.tab_dev.chain = d.chain;
  st.tab_dev.bonded_next = d.bond;
  st.ff_dev.tab = &st.tab_dev;
  return SC_OK;
}

int assemble_host(sc_ctx* ctx, const double* coord, int64_t n, const sc_ff_desc* ff, const sc_patch_desc* patch,
                  const double* inv_sqrt_mass, double* out, int dim) {
  SC_TRY(check_coord_args(ctx, coord, n));
  SC_TRY(check_ff(ctx, ff));
  if (n > 0 && !out) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "output matrix is NULL");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (n == 0) return SC_OK;
  const size_t elems = (size_t)n * n * dim * dim;
  Staged st;
  double* d_m = nullptr;
  SC_TRY(stage_inputs(ctx, coord, n, ff, patch, inv_sqrt_mass, st, [&](Arena& a) { d_m = a.take<double>(elems); }));
  SC_TRY(launch_model_matrix(ctx, st, n, dim, d_m));
  SC_HIP(ctx, hipMemcpyAsync(out, d_m, elems * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

// Shared body of sc_kirchhoff_from_pairs_f64 (dim 1, no coordinates) / sc_hessian_from_pairs_f64 (dim 3) behind their checks
int from_pairs_host(sc_ctx* ctx, const double* coord, int64_t n, const int64_t* pairs, int64_t k, const double* gamma,
                    double* out, int dim) {
  if (k < 0 || (k > 0 && (!pairs || !gamma)))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "pairs / gamma is NULL");
  for (int64_t p = 0; p < 2 * k; ++p)
    if (pairs[p] < 0 || pairs[p] >= n)
      return sc_set_error(ctx, SC_ERR_INDEX, "pair index %lld out of range for %lld atoms",
                          (long long)pairs[p], (long long)n);
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (n == 0) return SC_OK;
  const size_t elems = (size_t)n * n * dim * dim;
  double *d_m = nullptr, *d_coord = nullptr, *d_g = nullptr;
  int64_t* d_pairs = nullptr;
  SC_TRY(carve_scratch(ctx, [&](Arena& a) {
    d_m = a.take<double>(elems);
    d_coord = dim == 3 ? a.take<double>((size_t)n * 3) : nullptr;
    d_pairs = a.take<int64_t>((size_t)k * 2 + 2);
    d_g = a.take<double>((size_t)k + 1);
  }));
  if (dim == 3) SC_HIP(ctx, hipMemcpyAsync(d_coord, coord, (size_t)n * 24, hipMemcpyHostToDevice, ctx->stream));
  if (k > 0) {
    SC_HIP(ctx, hipMemcpyAsync(d_pairs, pairs, (size_t)k * 16, hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(d_g, gamma, (size_t)k * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  SC_TRY(dim == 1 ? launch_kirchhoff_from_pairs(ctx, n, d_pairs, k, d_g, d_m)
                  : launch_hessian_from_pairs(ctx, d_coord, n, d_pairs, k, d_g, d_m));
  SC_HIP(ctx, hipMemcpyAsync(out, d_m, elems * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

// Window solve of the (n, n) matrix d_a; its results (device, in ctx->win_ws) -> page-locked host blocks of exactly (m,)
// and (m, n) that the caller owns (sc_host_free); m = 0: none, *w = *v = NULL as check_window_outputs left them.
int window_host(sc_ctx* ctx, double* d_a, int64_t n, double vl, double vu, bool vectors, int64_t* m_out, double** w,
                double** v) {
  int64_t m = 0;
  double *d_w = nullptr, *d_v = nullptr;
  SC_TRY(eigh_window(ctx, d_a, n, vl, vu, vectors, &m, &d_w, &d_v));
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
  if (vectors) *v = (double*)hv;
  *m_out = m;
  return SC_OK;
}

int check_window_outputs(sc_ctx* ctx, int want_vectors, int64_t* m, double** w, double** v) {
  if (!m || !w || (want_vectors && !v)) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  *m = 0;
  *w = nullptr;
  if (v) *v = nullptr;
  return SC_OK;
}

// m eigenvalues and, when asked for, velems eigenvector entries of a finished solve to the host
int eigenpairs_to_host(sc_ctx* ctx, const double* d_w, double* w, size_t m, const double* d_v, double* v, size_t velems) {
  SC_HIP(ctx, hipMemcpyAsync(w, d_w, m * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (v) SC_HIP(ctx, hipMemcpyAsync(v, d_v, velems * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

int enm_eigen_host(sc_ctx* ctx, const double* coord, int64_t n, const sc_ff_desc* ff, const sc_patch_desc* patch,
                   const double* inv_sqrt_mass, double* w, double* v, int dim) {
  SC_TRY(check_coord_args(ctx, coord, n));
  SC_TRY(check_ff(ctx, ff));
  if (n > 0 && !w) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "w is NULL");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (n == 0) return SC_OK;
  const int64_t m = n * dim;
  const size_t elems = (size_t)m * m;
  Staged st;
  double *d_m = nullptr, *d_w = nullptr, *d_v = nullptr;
  SC_TRY(stage_inputs(ctx, coord, n, ff, patch, inv_sqrt_mass, st, [&](Arena& a) {
    d_m = a.take<double>(elems);
    d_w = a.take<double>((size_t)m);
    d_v = v ? a.take<double>(elems) : nullptr;
  }));
  SC_TRY(launch_model_matrix(ctx, st, n, dim, d_m));
  SC_TRY(eigh_batched(ctx, d_m, m, 1, d_w, d_v));
  return eigenpairs_to_host(ctx, d_w, w, (size_t)m, d_v, v, elems);
}

// the checks of sc_dev_kirchhoff_f64 / sc_dev_hessian_f64; selects the device
int check_dev_assembly(sc_ctx* ctx, const double* d_coord, int64_t n, int64_t batch, const sc_ff_desc* ff,
                       const double* d_matrix) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(check_ff(ctx, ff));
  if (ff->kind == SC_FF_TABULATED)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "tabulated force fields are not supported on the batched device path");
  if (n < 0 || batch < 0 || (n > 0 && batch > 0 && (!d_coord || !d_matrix)))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return SC_OK;
}

}  // namespace

// (the host patch table is built before the measure pass: its size is an input to the layout)
int stage_inputs(sc_ctx* ctx, const double* coord, int64_t n, const sc_ff_desc* ff, const sc_patch_desc* pd,
                 const double* inv_sqrt_mass, Staged& st, const ScratchLayout& rest) {
  SC_TRY(build_patch(ctx, pd, n, st.hp));
  const HostPatch& hp = st.hp;
  const size_t N = (size_t)n, nb = ff->kind == SC_FF_TABULATED ? (size_t)ff->tab->n_bins : 0;
  HostPatch::Bufs pb{};
  TabBufs tb{};
  SC_TRY(carve_scratch(ctx, [&](Arena& a) {
    st.d_coord = a.take<double>(N * 3);
    st.d_w = inv_sqrt_mass ? a.take<double>(N) : nullptr;
    if (hp.any) pb = hp.layout(a);
    if (nb)   // (a braced list is evaluated in order)
      tb = TabBufs{a.take<double>(nb), a.take<float>(3 * 400 * nb), a.take<int32_t>(N), a.take<int32_t>(N), a.take<uint8_t>(N)};
    rest(a);
  }));
  SC_HIP(ctx, hipMemcpyAsync(st.d_coord, coord, (size_t)n * 24, hipMemcpyHostToDevice, ctx->stream));
  if (inv_sqrt_mass)
    SC_HIP(ctx, hipMemcpyAsync(st.d_w, inv_sqrt_mass, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  if (st.hp.any) {
    SC_TRY(upload_patch(ctx, st.hp, pb, st.patch));
    st.has_patch = true;
  }
  return upload_tab(ctx, ff, n, tb, st);
}

extern "C" {

int sc_contacts(sc_ctx* ctx, const double* coord, int64_t n, const sc_ff_desc* ff,
                const sc_patch_desc* patch, int64_t* counts, int64_t* n_pairs) {
  SC_TRY(check_coord_args(ctx, coord, n));
  SC_TRY(check_ff(ctx, ff));
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (n_pairs) *n_pairs = 0;
  if (n == 0) return SC_OK;
  Staged st;
  int64_t* d_counts = nullptr;
  SC_TRY(stage_inputs(ctx, coord, n, ff, patch, nullptr, st, [&](Arena& a) { d_counts = a.take<int64_t>((size_t)n); }));
  SC_TRY(launch_contact_counts(ctx, st.d_coord, n, st.ff_dev, st.patch_dev(), d_counts));
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
  int64_t *d_counts = nullptr, *d_off = nullptr, *d_pairs = nullptr;
  double* d_sq = nullptr;
  SC_TRY(stage_inputs(ctx, coord, n, ff, patch, nullptr, st, [&](Arena& a) {
    d_counts = a.take<int64_t>((size_t)n);
    d_off = a.take<int64_t>((size_t)n + 1);
    d_pairs = a.take<int64_t>((size_t)capacity * 2 + 2);
    d_sq = sq_dist ? a.take<double>((size_t)capacity + 1) : nullptr;
  }));
  SC_TRY(launch_contact_counts(ctx, st.d_coord, n, st.ff_dev, st.patch_dev(), d_counts));
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
  SC_TRY(launch_pair_fill(ctx, st.d_coord, n, st.ff_dev, st.patch_dev(), d_off, d_pairs, d_sq));
  SC_HIP(ctx, hipMemcpyAsync(pairs, d_pairs, (size_t)k * 16, hipMemcpyDeviceToHost, ctx->stream));
  if (sq_dist)
    SC_HIP(ctx, hipMemcpyAsync(sq_dist, d_sq, (size_t)k * 8, hipMemcpyDeviceToHost, ctx->stream));
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

int sc_kirchhoff_from_pairs_f64(sc_ctx* ctx, int64_t n, const int64_t* pairs, int64_t k,
                                const double* gamma, double* kirchhoff) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (n < 0 || (n > 0 && !kirchhoff)) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  return from_pairs_host(ctx, nullptr, n, pairs, k, gamma, kirchhoff, 1);
}

int sc_hessian_from_pairs_f64(sc_ctx* ctx, const double* coord, int64_t n, const int64_t* pairs,
                              int64_t k, const double* gamma, double* hessian) {
  SC_TRY(check_coord_args(ctx, coord, n));
  if (n > 0 && !hessian) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "output matrix is NULL");
  return from_pairs_host(ctx, coord, n, pairs, k, gamma, hessian, 3);
}

int sc_eigh_f64(sc_ctx* ctx, const double* a, int64_t n, double* w, double* v) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (n < 0 || (n > 0 && (!a || !w))) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (n == 0) return SC_OK;
  const size_t elems = (size_t)n * n;
  double *d_a = nullptr, *d_w = nullptr, *d_v = nullptr;
  SC_TRY(carve_scratch(ctx, [&](Arena& s) {
    d_a = s.take<double>(elems);
    d_w = s.take<double>((size_t)n);
    d_v = v ? s.take<double>(elems) : nullptr;
  }));
  SC_HIP(ctx, hipMemcpyAsync(d_a, a, elems * 8, hipMemcpyHostToDevice, ctx->stream));
  SC_TRY(eigh_batched(ctx, d_a, n, 1, d_w, d_v));
  return eigenpairs_to_host(ctx, d_w, w, (size_t)n, d_v, v, elems);
}

int sc_pinvh_f64(sc_ctx* ctx, const double* a, int64_t n, double rcond, double* out) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (n < 0 || (n > 0 && (!a || !out))) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (n == 0) return SC_OK;
  const size_t elems = (size_t)n * n;
  double *d_a = nullptr, *d_out = nullptr;
  SC_TRY(carve_scratch(ctx, [&](Arena& s) { d_a = s.take<double>(elems); d_out = s.take<double>(elems); }));
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
  double *d_a = nullptr, *d_w = nullptr, *d_v = nullptr;
  SC_TRY(carve_scratch(ctx, [&](Arena& s) {
    d_a = s.take<double>(elems);
    d_w = s.take<double>((size_t)m);
    d_v = v ? s.take<double>((size_t)m * n) : nullptr;
  }));
  SC_HIP(ctx, hipMemcpyAsync(d_a, a, elems * 8, hipMemcpyHostToDevice, ctx->stream));
  SC_TRY(eigh_range_batched(ctx, d_a, n, 1, il, iu, d_w, d_v));
  return eigenpairs_to_host(ctx, d_w, w, (size_t)m, d_v, v, (size_t)m * n);
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
  double *d_m = nullptr, *d_w = nullptr, *d_v = nullptr;
  SC_TRY(stage_inputs(ctx, coord, n, ff, patch, inv_sqrt_mass, st, [&](Arena& a) {
    d_m = a.take<double>(elems);
    d_w = a.take<double>((size_t)m);
    d_v = v ? a.take<double>((size_t)m * dim3n) : nullptr;
  }));
  SC_TRY(launch_hessian(ctx, st.d_coord, n, 1, st.ff_dev, st.patch_dev(), st.d_w, d_m));
  SC_TRY(eigh_range_batched(ctx, d_m, dim3n, 1, il, iu, d_w, d_v));
  return eigenpairs_to_host(ctx, d_w, w, (size_t)m, d_v, v, (size_t)m * dim3n);
}

int sc_dev_eigh_range_f64(sc_ctx* ctx, double* d_a, int64_t n, int64_t batch, int64_t il, int64_t iu,
                          double* d_w, double* d_v) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (n <= 0 || batch <= 0 || !d_a || !d_w) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return eigh_range_batched_async(ctx, d_a, n, batch, il, iu, d_w, d_v);
}

int sc_eigh_window_f64(sc_ctx* ctx, const double* a, int64_t n, double vl, double vu, int want_vectors, int64_t* m,
                       double** w, double** v) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  SC_TRY(check_window_outputs(ctx, want_vectors, m, w, v));
  if (n <= 0 || !a) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const size_t elems = (size_t)n * n;
  double* d_a = nullptr;
  SC_TRY(carve_scratch(ctx, [&](Arena& s) { d_a = s.take<double>(elems); }));
  SC_HIP(ctx, hipMemcpyAsync(d_a, a, elems * 8, hipMemcpyHostToDevice, ctx->stream));
  return window_host(ctx, d_a, n, vl, vu, want_vectors != 0, m, w, v);
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
  double* d_m = nullptr;
  SC_TRY(stage_inputs(ctx, coord, n, ff, patch, inv_sqrt_mass, st, [&](Arena& a) { d_m = a.take<double>(elems); }));
  SC_TRY(launch_hessian(ctx, st.d_coord, n, 1, st.ff_dev, st.patch_dev(), st.d_w, d_m));
  return window_host(ctx, d_m, dim3n, vl, vu, want_vectors != 0, m, w, v);
}

int sc_dev_eigh_window_f64(sc_ctx* ctx, double* d_a, int64_t n, int64_t batch, double vl, double vu, int64_t capacity,
                           double* d_w, double* d_v, int64_t* d_count) {
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (n <= 0 || batch <= 0 || !d_a || !d_w || !d_count) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return eigh_window_batched_async(ctx, d_a, n, batch, vl, vu, capacity, d_w, d_v, d_count);
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
  SC_TRY(check_dev_assembly(ctx, d_coord, n, batch, ff, d_matrix));
  return launch_kirchhoff(ctx, d_coord, n, batch, *ff, nullptr, d_inv_sqrt_mass, d_matrix, nullptr);
}

int sc_dev_hessian_f64(sc_ctx* ctx, const double* d_coord, int64_t n, int64_t batch,
                       const sc_ff_desc* ff, const double* d_inv_sqrt_mass, double* d_matrix) {
  SC_TRY(check_dev_assembly(ctx, d_coord, n, batch, ff, d_matrix));
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

int64_t sc_eigh_workspace_bytes(int64_t n, int64_t batch, int want_vectors) {
  if (n <= 0 || batch <= 0) return 0;
  return (int64_t)eigh_workspace_bytes(n, batch, want_vectors != 0);
}

}  // extern "C"
