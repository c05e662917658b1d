// C ABI (include/springcraft_hip.h), the mode consumers of a batch (batch_consumers.hip, dist_fluct.hip, mode_overlap.hip,
// mode_response.hip, mode_prs.hip, mode_lmi.hip) on device tensors: the sc_dev_modes_* entries of a uniform batch and the sc_batch_plan_modes_* entries
// of a plan's padded slots; and the pairwise comparison of two uniform batches' modes (mode_subspace.hip: sc_dev_subspace_*,
// no plan entry -- members of different size have no common coordinates).
#include "api_internal.h"

namespace {

// Whose modes a consumer works on: the (batch, nvec, m) results of a uniform batch (sc_dev_modes_*: m = dim * n_atoms) or
// of a plan's padded slots (sc_batch_plan_modes_*).  Each consumer has ONE body, modes_* below, which runs every check and
// calls the launcher; its two entries only build this description.
struct ModesOf {
  sc_ctx* ctx = nullptr;
  int64_t m = 0, nvec = 0, batch = 0;
  int dim = 0;
  RaggedView view{};       // a plan's records: m is then the slot order (dim need not divide it) and d_out is packed
  int64_t first_row = 0;   // a plan's global mode index of row 0 of (w, v), as the caller gave it: checked after the rest
  const RaggedView* ragged() const { return view.d_rec ? &view : nullptr; }
};

// (a NULL plan gives the empty description, which every body answers as it answers a NULL ctx)
ModesOf plan_modes_of(const sc_batch_plan* plan, int64_t nvec, int64_t first_row) {
  if (!plan) return ModesOf{};
  const RaggedView rv{plan_records(plan), (int)first_row, plan->max_atoms, plan->atom_off.back(), plan->total_sq};
  return ModesOf{plan->ctx, plan->order, nvec, plan->count, plan->dim, rv, first_row};
}

// The (m, nvec, batch, dim) checks of every consumer; `pointers`: the consumer's required pointers are all there
int check_modes_shape(const ModesOf& who, bool pointers) {
  sc_ctx* ctx = who.ctx;
  if (!ctx) return SC_ERR_INVALID_ARG;
  if (who.m <= 0 || who.nvec <= 0 || who.batch <= 0 || !pointers) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "bad arguments");
  if ((who.dim != 1 && who.dim != 3) || (!who.ragged() && who.m % who.dim != 0))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "dim must be 1 or 3 and divide m = %lld", (long long)who.m);
  if (who.m > INT32_MAX || who.nvec > who.m || who.batch > INT32_MAX || (size_t)who.batch * who.nvec > (size_t)INT32_MAX)
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "(batch, nvec, m) = (%lld, %lld, %lld) is not a solver's result shape",
                        (long long)who.batch, (long long)who.nvec, (long long)who.m);
  return SC_OK;
}

int check_first_row(const ModesOf& who) {
  if (!who.ragged() || (who.first_row >= 0 && who.first_row < who.m)) return SC_OK;
  return sc_set_error(who.ctx, SC_ERR_INDEX, "first row %lld outside 0..%lld", (long long)who.first_row, (long long)who.m - 1);
}

int check_modes_args(const ModesOf& who, const double* d_w, const double* d_v, const sc_mode_selection* sel,
                     const double* d_out) {
  SC_TRY(check_modes_shape(who, d_w && d_v && sel && d_out));
  switch (sel->kind) {
    case SC_SEL_FROM_ROW:
      if (sel->row0 < 0 || sel->row0 > who.nvec)
        return sc_set_error(who.ctx, SC_ERR_INDEX, "row0 %lld outside 0..%lld", (long long)sel->row0, (long long)who.nvec);
      break;
    case SC_SEL_ROWS:
      if (sel->n_rows < 0 || sel->n_rows > INT32_MAX / 4 || (sel->n_rows > 0 && !sel->d_rows))
        return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "bad row list");
      break;
    case SC_SEL_PINV:
      if (!(sel->rcond >= 0.0)) return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "rcond must be >= 0");
      break;
    default:
      return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "unknown selection kind %d", (int)sel->kind);
  }
  return check_first_row(who);
}

int modes_msf(const ModesOf& who, const double* d_w, const double* d_v, const sc_mode_selection* sel,
              const int64_t* d_counts, double* d_out) {
  SC_TRY(check_modes_args(who, d_w, d_v, sel, d_out));
  SC_HIP(who.ctx, hipSetDevice(who.ctx->device));
  return batch_msf_device(who.ctx, d_w, d_v, who.m, who.nvec, who.batch, who.dim, *sel, d_counts, 0, d_out, who.ragged());
}

int modes_dcc(const ModesOf& who, const double* d_w, const double* d_v, const sc_mode_selection* sel,
              const int64_t* d_counts, int norm, int64_t budget_bytes, double* d_out) {
  SC_TRY(check_modes_args(who, d_w, d_v, sel, d_out));
  if (budget_bytes < 0) return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "budget_bytes must be >= 0");
  SC_HIP(who.ctx, hipSetDevice(who.ctx->device));
  return batch_dcc_device(who.ctx, d_w, d_v, who.m, who.nvec, who.batch, who.dim, *sel, d_counts, norm,
                          (size_t)budget_bytes, d_out, who.ragged());
}

// (aniso, distfluct: the sc_dev entries have no dim argument and describe dim 3, so only a plan can fail the dim check)
int modes_aniso(const ModesOf& who, const double* d_w, const double* d_v, const sc_mode_selection* sel,
                const int64_t* d_counts, double* d_out) {
  SC_TRY(check_modes_args(who, d_w, d_v, sel, d_out));
  if (who.dim != 3)
    return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "anisotropic fluctuation tensors need an ANM plan (dim 3)");
  SC_HIP(who.ctx, hipSetDevice(who.ctx->device));
  return batch_aniso_device(who.ctx, d_w, d_v, who.m, who.nvec, who.batch, *sel, d_counts, 0, d_out, who.ragged());
}

int modes_distfluct(const ModesOf& who, const double* d_w, const double* d_v, const sc_mode_selection* sel,
                    const int64_t* d_counts, const double* d_coord, const double* d_atom_scale, double* d_out) {
  SC_TRY(check_modes_args(who, d_w, d_v, sel, d_out));
  if (who.dim != 3) return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "distance fluctuations need an ANM plan (dim 3)");
  if (!d_coord) return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "distance fluctuations need the coordinates");
  SC_HIP(who.ctx, hipSetDevice(who.ctx->device));
  return batch_distfluct_device(who.ctx, d_w, d_v, who.m, who.nvec, who.batch, *sel, d_counts, d_coord, d_atom_scale,
                                d_out, who.ragged());
}

int modes_prs(const ModesOf& who, const double* d_w, const double* d_v, const sc_mode_selection* sel,
              const int64_t* d_counts, const double* d_atom_scale, int norm, double* d_out) {
  SC_TRY(check_modes_args(who, d_w, d_v, sel, d_out));
  if (who.dim != 3 || (!who.ragged() && who.m % 3 != 0))
    return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "perturbation response scanning needs an ANM (dim 3, m = 3 N)");
  SC_HIP(who.ctx, hipSetDevice(who.ctx->device));
  return batch_prs_device(who.ctx, d_w, d_v, who.m, who.nvec, who.batch, *sel, d_counts, d_atom_scale, norm, d_out,
                          who.ragged());
}

int modes_lmi(const ModesOf& who, const double* d_w, const double* d_v, const sc_mode_selection* sel,
              const int64_t* d_counts, int information, double* d_out) {
  SC_TRY(check_modes_args(who, d_w, d_v, sel, d_out));
  if (who.dim != 3 || (!who.ragged() && who.m % 3 != 0))
    return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "the generalized correlation needs an ANM (dim 3, m = 3 N)");
  SC_HIP(who.ctx, hipSetDevice(who.ctx->device));
  return batch_lmi_device(who.ctx, d_w, d_v, who.m, who.nvec, who.batch, *sel, d_counts, information, d_out, who.ragged());
}

int modes_overlap(const ModesOf& who, const double* d_v, const double* d_disp, int64_t q, const int64_t* d_counts,
                  double* d_overlap, double* d_collectivity) {
  SC_TRY(check_modes_shape(who, d_v != nullptr));
  sc_ctx* ctx = who.ctx;
  if (q < 0 || q > INT32_MAX / 4) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "q = %lld displacement vectors", (long long)q);
  if (!d_overlap && !d_collectivity) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "both outputs are NULL");
  if ((q > 0 && (!d_disp || !d_overlap)) || (q == 0 && !d_collectivity))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "q = %lld needs %s", (long long)q,
                        q > 0 ? "d_disp and d_overlap" : "d_collectivity");
  SC_TRY(check_first_row(who));
  SC_HIP(ctx, hipSetDevice(ctx->device));
  return modes_overlap_device(ctx, d_v, who.m, who.nvec, who.batch, who.dim, nullptr, who.nvec, d_disp, q, d_counts,
                              d_overlap, d_collectivity, who.ragged());
}

// (response: dim 1 is a GNM's, for which the reference defines no linear response; the Python layer refuses it, the
// arithmetic here is the same for both)
int modes_response(const ModesOf& who, const double* d_w, const double* d_v, const sc_mode_selection* sel,
                   const int64_t* d_counts, const double* d_force, int64_t q, const double* d_atom_scale, double* d_out) {
  SC_TRY(check_modes_args(who, d_w, d_v, sel, d_out));
  if (q < 0 || q > INT32_MAX / 4 || (q > 0 && !d_force))
    return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "q = %lld force vectors", (long long)q);
  SC_HIP(who.ctx, hipSetDevice(who.ctx->device));
  return modes_response_device(who.ctx, d_w, d_v, who.m, who.nvec, who.batch, who.dim, *sel, d_counts, d_force, q,
                               d_atom_scale, 0, d_out, who.ragged());
}

int modes_combine(const ModesOf& who, const double* d_v, const double* d_coef, int64_t q, const int64_t* d_counts,
                  const double* d_atom_scale, double* d_out) {
  SC_TRY(check_modes_shape(who, d_v && d_out));
  if (q < 0 || q > INT32_MAX / 4 || (q > 0 && !d_coef))
    return sc_set_error(who.ctx, SC_ERR_INVALID_ARG, "q = %lld coefficient vectors", (long long)q);
  SC_TRY(check_first_row(who));
  SC_HIP(who.ctx, hipSetDevice(who.ctx->device));
  return modes_combine_device(who.ctx, d_v, who.m, who.nvec, who.batch, who.dim, nullptr, who.nvec, d_coef, q, d_counts,
                              d_atom_scale, 0, d_out, who.ragged());
}

// (subspace: uniform batches only, two operand sets of one m; d_v_b NULL compares the first set with itself and then
// takes no other argument of the second)
int modes_subspace(sc_ctx* ctx, const double* d_w_a, const double* d_v_a, const sc_mode_selection* sel_a,
                   const int64_t* d_counts_a, int64_t nvec_a, int64_t batch_a, const double* d_w_b, const double* d_v_b,
                   const sc_mode_selection* sel_b, const int64_t* d_counts_b, int64_t nvec_b, int64_t batch_b, int64_t m,
                   int kind, const int32_t* d_pairs, int64_t n_pairs, double* d_out, double* d_s, double* d_t_a,
                   double* d_t_b) {
  SC_TRY(check_modes_args(ModesOf{ctx, m, nvec_a, batch_a, 1}, d_w_a, d_v_a, sel_a, d_out));
  const bool self = d_v_b == nullptr;
  if (self && (d_w_b || sel_b || d_counts_b || d_t_b))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "a self-comparison (d_v_b NULL) takes no second operand set");
  if (!self) SC_TRY(check_modes_args(ModesOf{ctx, m, nvec_b, batch_b, 1}, d_w_b, d_v_b, sel_b, d_out));
  if (kind < 0 || kind > 2) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "unknown kind %d", kind);
  if (kind == 2 && (n_pairs < 0 || n_pairs > INT32_MAX / 4 || (n_pairs > 0 && !d_pairs)))
    return sc_set_error(ctx, SC_ERR_INVALID_ARG, "n_pairs = %lld pairs", (long long)n_pairs);
  SC_HIP(ctx, hipSetDevice(ctx->device));
  const SubspaceSet a{d_w_a, d_v_a, sel_a, d_counts_a, nvec_a, batch_a};
  const SubspaceSet b{d_w_b, d_v_b, sel_b, d_counts_b, nvec_b, batch_b};
  return modes_subspace_device(ctx, a, self ? nullptr : &b, m, kind, d_pairs, n_pairs, d_out, d_s, d_t_a, d_t_b);
}

int64_t modes_workspace_bytes(const ModesOf& who, int64_t n_sel, int what, int64_t budget_bytes) {
  if (who.m <= 0 || who.nvec <= 0 || who.batch <= 0 || n_sel < 0 || (who.dim != 1 && who.dim != 3) || budget_bytes < 0)
    return 0;
  if (what == 3) return 0;   // overlaps and collectivities hold no workspace
  if ((what == 2 || what == 4 || what == 7 || what == 8) && (who.dim != 3 || (!who.ragged() && who.m % 3 != 0))) return 0;
  return (int64_t)batch_modes_workspace_bytes(who.m, who.nvec, who.batch, who.dim, n_sel, what, (size_t)budget_bytes,
                                              who.ragged());
}

}  // namespace

// ---- the entries (a plan's first_row comes in sel->reserved): the bodies are modes_* above ---------------------------------
extern "C" {

int sc_dev_modes_msf_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                         int dim, const sc_mode_selection* sel, const int64_t* d_counts, double* d_out) {
  return modes_msf(ModesOf{ctx, m, nvec, batch, dim}, d_w, d_v, sel, d_counts, d_out);
}
int sc_batch_plan_modes_msf_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                                const sc_mode_selection* sel, const int64_t* d_counts, double* d_out) {
  return modes_msf(plan_modes_of(plan, nvec, sel ? sel->reserved : 0), d_w, d_v, sel, d_counts, d_out);
}

int sc_dev_modes_dcc_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                         int dim, const sc_mode_selection* sel, const int64_t* d_counts, int norm, int64_t budget_bytes,
                         double* d_out) {
  return modes_dcc(ModesOf{ctx, m, nvec, batch, dim}, d_w, d_v, sel, d_counts, norm, budget_bytes, d_out);
}
int sc_batch_plan_modes_dcc_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                                const sc_mode_selection* sel, const int64_t* d_counts, int norm, int64_t budget_bytes,
                                double* d_out) {
  return modes_dcc(plan_modes_of(plan, nvec, sel ? sel->reserved : 0), d_w, d_v, sel, d_counts, norm, budget_bytes, d_out);
}

int sc_dev_modes_aniso_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                           const sc_mode_selection* sel, const int64_t* d_counts, double* d_out) {
  return modes_aniso(ModesOf{ctx, m, nvec, batch, 3}, d_w, d_v, sel, d_counts, d_out);
}
int sc_batch_plan_modes_aniso_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                                  const sc_mode_selection* sel, const int64_t* d_counts, double* d_out) {
  return modes_aniso(plan_modes_of(plan, nvec, sel ? sel->reserved : 0), d_w, d_v, sel, d_counts, d_out);
}

int sc_dev_modes_distfluct_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                               const sc_mode_selection* sel, const int64_t* d_counts, const double* d_coord,
                               const double* d_atom_scale, double* d_out) {
  return modes_distfluct(ModesOf{ctx, m, nvec, batch, 3}, d_w, d_v, sel, d_counts, d_coord, d_atom_scale, d_out);
}
int sc_batch_plan_modes_distfluct_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                                      const sc_mode_selection* sel, const int64_t* d_counts, const double* d_coord,
                                      const double* d_atom_scale, double* d_out) {
  return modes_distfluct(plan_modes_of(plan, nvec, sel ? sel->reserved : 0), d_w, d_v, sel, d_counts, d_coord,
                         d_atom_scale, d_out);
}

int sc_dev_prs_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                   const sc_mode_selection* sel, const int64_t* d_counts, const double* d_atom_scale, int norm,
                   double* d_out) {
  return modes_prs(ModesOf{ctx, m, nvec, batch, 3}, d_w, d_v, sel, d_counts, d_atom_scale, norm, d_out);
}
int sc_batch_plan_prs_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                          const sc_mode_selection* sel, const int64_t* d_counts, const double* d_atom_scale, int norm,
                          double* d_out) {
  return modes_prs(plan_modes_of(plan, nvec, sel ? sel->reserved : 0), d_w, d_v, sel, d_counts, d_atom_scale, norm, d_out);
}

int sc_dev_lmi_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                   const sc_mode_selection* sel, const int64_t* d_counts, int information, double* d_out) {
  return modes_lmi(ModesOf{ctx, m, nvec, batch, 3}, d_w, d_v, sel, d_counts, information, d_out);
}
int sc_batch_plan_lmi_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                          const sc_mode_selection* sel, const int64_t* d_counts, int information, double* d_out) {
  return modes_lmi(plan_modes_of(plan, nvec, sel ? sel->reserved : 0), d_w, d_v, sel, d_counts, information, d_out);
}

int sc_dev_modes_overlap_f64(sc_ctx* ctx, const double* d_v, int64_t m, int64_t nvec, int64_t batch, int dim,
                             const double* d_disp, int64_t q, const int64_t* d_counts, double* d_overlap,
                             double* d_collectivity) {
  return modes_overlap(ModesOf{ctx, m, nvec, batch, dim}, d_v, d_disp, q, d_counts, d_overlap, d_collectivity);
}
int sc_batch_plan_modes_overlap_f64(sc_batch_plan* plan, const double* d_v, int64_t nvec, int64_t first_row,
                                    const double* d_disp, int64_t q, const int64_t* d_counts, double* d_overlap,
                                    double* d_collectivity) {
  return modes_overlap(plan_modes_of(plan, nvec, first_row), d_v, d_disp, q, d_counts, d_overlap, d_collectivity);
}

int sc_dev_mode_response_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                             int dim, const sc_mode_selection* sel, const int64_t* d_counts, const double* d_force,
                             int64_t q, const double* d_atom_scale, double* d_out) {
  return modes_response(ModesOf{ctx, m, nvec, batch, dim}, d_w, d_v, sel, d_counts, d_force, q, d_atom_scale, d_out);
}
int sc_batch_plan_mode_response_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                                    const sc_mode_selection* sel, const int64_t* d_counts, const double* d_force,
                                    int64_t q, const double* d_atom_scale, double* d_out) {
  return modes_response(plan_modes_of(plan, nvec, sel ? sel->reserved : 0), d_w, d_v, sel, d_counts, d_force, q,
                        d_atom_scale, d_out);
}

int sc_dev_mode_combine_f64(sc_ctx* ctx, const double* d_v, int64_t m, int64_t nvec, int64_t batch, int dim,
                            const double* d_coef, int64_t q, const int64_t* d_counts, const double* d_atom_scale,
                            double* d_out) {
  return modes_combine(ModesOf{ctx, m, nvec, batch, dim}, d_v, d_coef, q, d_counts, d_atom_scale, d_out);
}
int sc_batch_plan_mode_combine_f64(sc_batch_plan* plan, const double* d_v, int64_t nvec, int64_t first_row,
                                   const double* d_coef, int64_t q, const int64_t* d_counts, const double* d_atom_scale,
                                   double* d_out) {
  return modes_combine(plan_modes_of(plan, nvec, first_row), d_v, d_coef, q, d_counts, d_atom_scale, d_out);
}

int sc_dev_subspace_f64(sc_ctx* ctx, const double* d_w_a, const double* d_v_a, const sc_mode_selection* sel_a,
                        const int64_t* d_counts_a, int64_t nvec_a, int64_t batch_a, const double* d_w_b,
                        const double* d_v_b, const sc_mode_selection* sel_b, const int64_t* d_counts_b, int64_t nvec_b,
                        int64_t batch_b, int64_t m, int kind, double* d_out, double* d_s, double* d_t_a, double* d_t_b) {
  if (ctx && kind != 0 && kind != 1) return sc_set_error(ctx, SC_ERR_INVALID_ARG, "kind must be 0 or 1, got %d", kind);
  return modes_subspace(ctx, d_w_a, d_v_a, sel_a, d_counts_a, nvec_a, batch_a, d_w_b, d_v_b, sel_b, d_counts_b, nvec_b,
                        batch_b, m, kind, nullptr, 0, d_out, d_s, d_t_a, d_t_b);
}
int sc_dev_subspace_gram_f64(sc_ctx* ctx, const double* d_w_a, const double* d_v_a, const sc_mode_selection* sel_a,
                             int64_t nvec_a, int64_t batch_a, const double* d_w_b, const double* d_v_b,
                             const sc_mode_selection* sel_b, int64_t nvec_b, int64_t batch_b, int64_t m,
                             const int32_t* d_pairs, int64_t n_pairs, double* d_out) {
  return modes_subspace(ctx, d_w_a, d_v_a, sel_a, nullptr, nvec_a, batch_a, d_w_b, d_v_b, sel_b, nullptr, nvec_b, batch_b,
                        m, 2, d_pairs, n_pairs, d_out, nullptr, nullptr, nullptr);
}

int64_t sc_dev_modes_workspace_bytes(int64_t m, int64_t nvec, int64_t batch, int dim, int64_t n_sel, int what,
                                     int64_t budget_bytes) {
  return modes_workspace_bytes(ModesOf{nullptr, m, nvec, batch, dim}, n_sel, what, budget_bytes);
}
int64_t sc_batch_plan_modes_workspace_bytes(const sc_batch_plan* plan, int64_t nvec, int64_t n_sel, int what,
                                            int64_t budget_bytes) {
  return modes_workspace_bytes(plan_modes_of(plan, nvec, 0), n_sel, what, budget_bytes);
}

}  // extern "C"
