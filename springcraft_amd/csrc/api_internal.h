// Declarations shared by the C-ABI units (api_*.hip): host plumbing only -- argument checks, the scratch protocol, staging
// of one model's inputs, the batch plan.  The kernels' header is common.h.
#pragma once
#include <functional>

#include "common.h"
#include "host_logic.h"
#include "scratch_arena.h"

// ---- ctx->scratch (api_context.hip) ----------------------------------------------------------------------------------
// Assigns the caller's pointers from take() calls and does nothing else: it runs twice.
using ScratchLayout = std::function<void(sc_host::Arena&)>;
// The whole protocol of ctx->scratch: measures `layout`, grows the buffer to that size, runs `layout` again on it.  The
// pointers hold until the next carve, which may move the buffer: no entry carves twice or calls another that does (the
// solvers work in ws / pinv_ws / win_ws / modes_ws / dc_aux) between a carve and the last use of its pointers.
int carve_scratch(sc_ctx* ctx, const ScratchLayout& layout);

// ---- one model's inputs (api_model.hip) ------------------------------------------------------------------------------
int check_ff(sc_ctx* ctx, const sc_ff_desc* ff);
int check_coord_args(sc_ctx* ctx, const double* coord, int64_t n);
int build_patch(sc_ctx* ctx, const sc_patch_desc* pd, int64_t n, sc_host::HostPatch& hp);

struct Staged {
  double* d_coord = nullptr;
  double* d_w = nullptr;
  PatchDev patch{};
  bool has_patch = false;
  sc_host::HostPatch hp;   // keeps host vectors alive until the stream is synchronised
  sc_tab_desc tab_dev{};   // SC_FF_TABULATED: same fields, DEVICE pointers
  sc_ff_desc ff_dev{};     // copy of the caller's descriptor with .tab -> &tab_dev: what the kernel launchers must be given
  const PatchDev* patch_dev() const { return has_patch ? &patch : nullptr; }
};
// Shared body of the host entries that start from coordinates: carves coord (+ weights, patch and force-field tables) and
// then the caller's `rest` out of scratch in one carve_scratch, and uploads the inputs.
int stage_inputs(sc_ctx* ctx, const double* coord, int64_t n, const sc_ff_desc* ff, const sc_patch_desc* pd,
                 const double* inv_sqrt_mass, Staged& st, const ScratchLayout& rest);
// the staged model's Kirchhoff (dim 1) or Hessian (dim 3) matrix
static inline int launch_model_matrix(sc_ctx* ctx, const Staged& st, int64_t n, int dim, double* d_m) {
  return dim == 1 ? launch_kirchhoff(ctx, st.d_coord, n, 1, st.ff_dev, st.patch_dev(), st.d_w, d_m, nullptr)
                  : launch_hessian(ctx, st.d_coord, n, 1, st.ff_dev, st.patch_dev(), st.d_w, d_m);
}

// ---- ragged / decorated batches (api_plan.hip) -----------------------------------------------------------------------
// Everything a batch of structures needs on the device besides coordinates: per-structure records (size, slot order,
// force-field descriptor with device table pointers, patch override tables), uploaded once at plan creation.
struct sc_batch_plan {
  sc_ctx* ctx = nullptr;
  int dim = 3;
  int64_t count = 0, order = 0;
  int max_atoms = 0;
  bool any_patch = false, any_pad = false;
  char* d_blob = nullptr;
  size_t off_items = 0, off_bound = 0, off_ragged = 0;
  std::vector<int64_t> atom_off;   // count + 1: first atom of every structure in the packed buffers
  int64_t total_sq = 0;            // sum of n_atoms^2: elements of a packed dcc
  int min_atoms = 0;
};

static inline const RaggedRec* plan_records(const sc_batch_plan* plan) {
  return reinterpret_cast<const RaggedRec*>(plan->d_blob + plan->off_ragged);
}
