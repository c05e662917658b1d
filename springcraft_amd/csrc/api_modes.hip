// C ABI (include/springcraft_hip.h), sc_modes: the device-resident eigenpairs of one model and their host consumers.  The
// consumers are the batch kernels with a batch of one (nvec = m = n, no counts, default budget; workspace ctx->modes_ws):
// one arithmetic order for a model, a batch and a ragged batch.
#include <algorithm>
#include <initializer_list>
#include <new>

#include "api_internal.h"

using sc_host::Arena;

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

bool bad_mode_list(const int64_t* mode_idx, int64_t k) { return k < 0 || k > INT32_MAX / 4 || (k > 0 && !mode_idx); }

// One buffer of doubles in scratch: *dev of max(count, 1) elements, filled from `up` before the run and / or copied to `down`
// after it (a NULL host pointer or count = 0: no copy).
struct ModeBuf {
  double** dev;
  size_t count;
  const double* up;
  double* down;
};

// The one staging body of a model's consumers over a mode list: the validated list and the entry's buffers carved from
// scratch, the index errors, the uploads, `run` on the list as a row selection, the downloads, one synchronisation.
// `empty`: nothing to compute, which is found out only after the index check.
template <typename Run>
int modes_list_call(sc_modes* m, const int64_t* mode_idx, int64_t k, bool empty, std::initializer_list<ModeBuf> bufs,
                    Run run) {
  sc_ctx* ctx = m->ctx;
  int* d_sel = nullptr;
  SC_TRY(carve_scratch(ctx, [&](Arena& a) {
    d_sel = a.take<int>((size_t)std::max<int64_t>(k, 1));
    for (const ModeBuf& b : bufs) *b.dev = a.take<double>(std::max<size_t>(b.count, 1));
  }));
  SC_TRY(stage_mode_list(m, mode_idx, k, d_sel));   // (the index errors come first, whatever else is empty)
  if (empty) return SC_OK;
  for (const ModeBuf& b : bufs)
    if (b.up && b.count) SC_HIP(ctx, hipMemcpyAsync(*b.dev, b.up, b.count * 8, hipMemcpyHostToDevice, ctx->stream));
  sc_mode_selection sel{};
  sel.kind = SC_SEL_ROWS;
  sel.d_rows = d_sel;
  sel.n_rows = k;
  SC_TRY(run(sel));
  for (const ModeBuf& b : bufs)
    if (b.down && b.count) SC_HIP(ctx, hipMemcpyAsync(b.down, *b.dev, b.count * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

// msf / dcc / tensors: one (out_elems) result and nothing else; a model without modes is answered before its list is read
template <typename Run>
int modes_out_call(sc_modes* m, const int64_t* mode_idx, int64_t k, size_t out_elems, double* out, Run run) {
  sc_ctx* ctx = m->ctx;
  if (bad_mode_list(mode_idx, k) || (m->n > 0 && !out)) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  if (m->n == 0) return SC_OK;
  double* d_out = nullptr;
  return modes_list_call(m, mode_idx, k, false, {{&d_out, out_elems, nullptr, out}},
                         [&](const sc_mode_selection& sel) { return run(sel, d_out); });
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
    double* d_m = nullptr;
    rc = stage_inputs(ctx, coord, n, ff, patch, inv_sqrt_mass, st, [&](Arena& a) { d_m = a.take<double>(elems); });
    if (rc == SC_OK) {
      rc = launch_model_matrix(ctx, st, n, dim, d_m);
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
    double* d_a = nullptr;
    rc = carve_scratch(ctx, [&](Arena& s) { d_a = s.take<double>(elems); });
    if (rc == SC_OK) {
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
  return modes_out_call(m, mode_idx, k, (size_t)(m->n / m->dim), out, [m](const sc_mode_selection& sel, double* d_out) {
    return batch_msf_device(m->ctx, m->d_w, m->d_v, m->n, m->n, 1, m->dim, sel, nullptr, 0, d_out);
  });
}

int sc_modes_aniso(sc_modes* m, const int64_t* mode_idx, int64_t k, double* out) {
  if (!m) return SC_ERR_INVALID_ARG;
  if (m->dim != 3)
    return sc_set_error(m->ctx, SC_ERR_INVALID_ARG, "anisotropic fluctuation tensors need an ANM (dim 3)");
  return modes_out_call(m, mode_idx, k, (size_t)(m->n / 3) * 6, out, [m](const sc_mode_selection& sel, double* d_out) {
    return batch_aniso_device(m->ctx, m->d_w, m->d_v, m->n, m->n, 1, sel, nullptr, 0, d_out);
  });
}

int sc_modes_dcc(sc_modes* m, const int64_t* mode_idx, int64_t k, int norm, double* out) {
  if (!m) return SC_ERR_INVALID_ARG;
  const size_t N = (size_t)(m->n / m->dim);
  return modes_out_call(m, mode_idx, k, N * N, out, [m, norm](const sc_mode_selection& sel, double* d_out) {
    return batch_dcc_device(m->ctx, m->d_w, m->d_v, m->n, m->n, 1, m->dim, sel, nullptr, norm, 0, d_out);
  });
}

int sc_modes_distfluct(sc_modes* m, const int64_t* mode_idx, int64_t k, const double* coord, double* out) {
  if (!m) return SC_ERR_INVALID_ARG;
  sc_ctx* ctx = m->ctx;
  if (m->dim != 3) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "distance fluctuations need an ANM (dim 3)");
  if (bad_mode_list(mode_idx, k) || (m->n > 0 && (!coord || !out)))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const size_t N = (size_t)(m->n / 3);
  double *d_coord = nullptr, *d_out = nullptr;
  return modes_list_call(m, mode_idx, k, m->n == 0, {{&d_coord, N * 3, coord, nullptr}, {&d_out, N * N, nullptr, out}},
                         [&](const sc_mode_selection& sel) {
    return batch_distfluct_device(ctx, m->d_w, m->d_v, m->n, m->n, 1, sel, nullptr, d_coord, nullptr, d_out);
  });
}

int sc_modes_overlap(sc_modes* m, const int64_t* mode_idx, int64_t k, const double* disp, int64_t q, double* overlap_out,
                     double* collectivity_out) {
  if (!m) return SC_ERR_INVALID_ARG;
  sc_ctx* ctx = m->ctx;
  if (bad_mode_list(mode_idx, k) || q < 0 || q > INT32_MAX / 4 ||
      (!overlap_out && !collectivity_out) || (q > 0 && (!disp || !overlap_out)) || (q == 0 && !collectivity_out))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)m->n, K = (size_t)k, Q = (size_t)q;
  double *d_disp = nullptr, *d_ov = nullptr, *d_co = nullptr;
  return modes_list_call(m, mode_idx, k, m->n == 0 || k == 0,
                         {{&d_disp, Q * n, disp, nullptr}, {&d_ov, Q * K, nullptr, overlap_out}, {&d_co, K, nullptr, collectivity_out}},
                         [&](const sc_mode_selection& sel) {
    return modes_overlap_device(ctx, m->d_v, m->n, m->n, 1, m->dim, sel.d_rows, k, d_disp, q, nullptr, q > 0 ? d_ov : nullptr,
                                collectivity_out ? d_co : nullptr);
  });
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
  const size_t n = (size_t)m->n, Q = (size_t)q, N = n / (size_t)m->dim;
  double *d_force = nullptr, *d_out = nullptr, *d_scale = nullptr;
  return modes_list_call(m, mode_idx, k, m->n == 0 || q == 0,
                         {{&d_force, Q * n, force, nullptr}, {&d_out, Q * n, nullptr, out}, {&d_scale, N, atom_scale, nullptr}},
                         [&](sc_mode_selection sel) {
    if (pinv) {   // no list: every mode above rcond
      sel = sc_mode_selection{};
      sel.kind = SC_SEL_PINV;
      sel.rcond = rcond;
    }
    return modes_response_device(ctx, m->d_w, m->d_v, m->n, m->n, 1, m->dim, sel, nullptr, d_force, q,
                                 atom_scale ? d_scale : nullptr, 0, d_out);
  });
}

int sc_modes_combine(sc_modes* m, const int64_t* mode_idx, int64_t k, const double* coef, int64_t q, double* out) {
  if (!m) return SC_ERR_INVALID_ARG;
  sc_ctx* ctx = m->ctx;
  if (bad_mode_list(mode_idx, k) || q < 0 || q > INT32_MAX / 4 || (q > 0 && ((k > 0 && !coef) || (m->n > 0 && !out))))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)m->n, K = (size_t)k, Q = (size_t)q;
  double *d_coef = nullptr, *d_out = nullptr;
  return modes_list_call(m, mode_idx, k, m->n == 0 || q == 0, {{&d_coef, Q * K, coef, nullptr}, {&d_out, Q * n, nullptr, out}},
                         [&](const sc_mode_selection& sel) {
    return modes_combine_device(ctx, m->d_v, m->n, m->n, 1, m->dim, sel.d_rows, k, d_coef, q, nullptr, nullptr, 0, d_out);
  });
}

int sc_modes_prs_subset(sc_modes* m, const int64_t* mode_idx, int64_t k, int norm, double* out) {
  if (!m) return SC_ERR_INVALID_ARG;
  if (m->dim != 3) return sc_set_error(m->ctx, SC_ERR_INVALID_ARG, "perturbation response scanning needs an ANM (dim 3)");
  const size_t N = (size_t)(m->n / 3);
  return modes_out_call(m, mode_idx, k, N * N, out, [m, norm](const sc_mode_selection& sel, double* d_out) {
    return batch_prs_device(m->ctx, m->d_w, m->d_v, m->n, m->n, 1, sel, nullptr, nullptr, norm, d_out);
  });
}

int sc_modes_lmi(sc_modes* m, const int64_t* mode_idx, int64_t k, double rcond, int information, double* out) {
  if (!m) return SC_ERR_INVALID_ARG;
  sc_ctx* ctx = m->ctx;
  if (m->dim != 3) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "the generalized correlation needs an ANM (dim 3)");
  const bool pinv = mode_idx == nullptr;
  if (k < 0 || k > INT32_MAX / 4 || (pinv && (k != 0 || !(rcond >= 0.0))) || (m->n > 0 && !out))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const size_t N = (size_t)(m->n / 3);
  double* d_out = nullptr;
  return modes_list_call(m, mode_idx, k, m->n == 0, {{&d_out, N * N, nullptr, out}}, [&](sc_mode_selection sel) {
    if (pinv) {   // no list: every mode above rcond
      sel = sc_mode_selection{};
      sel.kind = SC_SEL_PINV;
      sel.rcond = rcond;
    }
    return batch_lmi_device(ctx, m->d_w, m->d_v, m->n, m->n, 1, sel, nullptr, information, d_out);
  });
}

int sc_modes_subspace(sc_modes* a, sc_modes* b, const int64_t* mode_idx_a, int64_t k_a, const int64_t* mode_idx_b,
                      int64_t k_b, double rcond, int kind, double* out_value, double* out_gram) {
  if (!a || !b) return SC_ERR_INVALID_ARG;
  sc_ctx* ctx = a->ctx;
  if (b->ctx != ctx || b->dim != a->dim || b->n != a->n)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "the two models differ in context, dim or order (%lld, %lld)",
                        (long long)a->n, (long long)b->n);
  // a NULL list (its k must be 0): every mode with |w| > rcond max|w|, the covariance rule; the table needs both lists
  const bool pinv_a = mode_idx_a == nullptr, pinv_b = mode_idx_b == nullptr;
  if ((kind != 0 && kind != 1) || k_a < 0 || k_a > INT32_MAX / 4 || k_b < 0 || k_b > INT32_MAX / 4 ||
      (pinv_a && k_a != 0) || (pinv_b && k_b != 0) || ((pinv_a || pinv_b) && (!(rcond >= 0.0) || out_gram)) ||
      (!out_value && !out_gram))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const size_t gram_elems = out_gram ? (size_t)k_a * (size_t)k_b : 0;
  int *d_sel_a = nullptr, *d_sel_b = nullptr, *d_pair = nullptr;
  double *d_val = nullptr, *d_gram = nullptr;
  SC_TRY(carve_scratch(ctx, [&](Arena& s) {
    d_sel_a = s.take<int>((size_t)std::max<int64_t>(k_a, 1));
    d_sel_b = s.take<int>((size_t)std::max<int64_t>(k_b, 1));
    d_pair = s.take<int>(2);
    d_val = s.take<double>(1);
    d_gram = s.take<double>(std::max<size_t>(gram_elems, 1));
  }));
  SC_TRY(stage_mode_list(a, mode_idx_a, k_a, d_sel_a));
  SC_TRY(stage_mode_list(b, mode_idx_b, k_b, d_sel_b));
  if (a->n == 0) return SC_OK;
  auto selection = [rcond](bool pinv, const int* d_sel, int64_t k) {
    sc_mode_selection sel{};
    if (pinv) {
      sel.kind = SC_SEL_PINV;
      sel.rcond = rcond;
    } else {
      sel.kind = SC_SEL_ROWS;
      sel.d_rows = d_sel;
      sel.n_rows = k;
    }
    return sel;
  };
  const sc_mode_selection sel_a = selection(pinv_a, d_sel_a, k_a), sel_b = selection(pinv_b, d_sel_b, k_b);
  const SubspaceSet sa{a->d_w, a->d_v, &sel_a, nullptr, a->n, 1}, sb{b->d_w, b->d_v, &sel_b, nullptr, b->n, 1};
  if (out_value) {
    SC_TRY(modes_subspace_device(ctx, sa, &sb, a->n, kind, nullptr, 0, d_val, nullptr, nullptr, nullptr));
    SC_HIP(ctx, hipMemcpyAsync(out_value, d_val, 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (gram_elems) {
    SC_HIP(ctx, hipMemsetAsync(d_pair, 0, 8, ctx->stream));   // the one pair (0, 0)
    SC_TRY(modes_subspace_device(ctx, sa, &sb, a->n, 2, d_pair, 1, d_gram, nullptr, nullptr, nullptr));
    SC_HIP(ctx, hipMemcpyAsync(out_gram, d_gram, gram_elems * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
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
  double* d_out = nullptr;
  char* scratch = nullptr;
  SC_TRY(carve_scratch(ctx, [&](Arena& a) {
    d_out = a.take<double>(N * N);
    scratch = a.take<char>(work);
  }));
  SC_TRY(modes_prs_device(ctx, m->d_v, m->d_w, m->n, rcond, norm, scratch, d_out));
  SC_HIP(ctx, hipMemcpyAsync(out, d_out, N * N * 8, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

}  // extern "C"
