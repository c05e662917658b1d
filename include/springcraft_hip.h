/*
 * springcraft_hip.h — C ABI of libspringcraft_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for springcraft's one hot path
 *     C-alpha coordinates -> contact scan -> Kirchhoff / 3x3-block Hessian -> symmetric eigensolve
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference's src/springcraft/).  The reference is pure Python/NumPy and has no FFI; the
 * binding a maintainer would add is a ctypes stub (shown in INTEGRATION.md and implemented
 * in springcraft_amd/_hip.py).
 *
 * Conventions
 *   - plain pointers + sizes only; no C++ / torch types cross this boundary;
 *   - every function returns an int status (SC_OK == 0); no exceptions cross the boundary;
 *     sc_last_error(ctx) returns a human-readable message for the last failure on ctx;
 *   - "host" entry points take host pointers and do their own transfers (they synchronise, and
 *     return the errors of their own call);
 *     "sc_dev_*" and sc_batch_plan_assemble_f64 take device pointers valid on the context's device
 *     and only enqueue work on the context's stream: descriptor tables travel through a pinned
 *     staging arena of the context, and what a solve can only find out on the device (a NaN / Inf
 *     entry in an input matrix, a failed QL iteration) is reported by the next sc_ctx_synchronize.
 *     One exception: a two-stage solve of a latency-bound batch (batch * n / 128 <= 2800) waits for
 *     its persistent bulge chase, whose control block decides whether the chase is complete;
 *   - all matrices are float64; Kirchhoff is (n,n), Hessian (3n,3n), C order, exactly as
 *     numpy returns them in the reference (interaction.py:48,107-109);
 *   - eigenvectors are returned "rows = modes": V[i*n + c] is component c of mode i, the
 *     layout of `eig_vectors` in nma.py:63.
 */
#ifndef SPRINGCRAFT_HIP_H
#define SPRINGCRAFT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes -------------------------------------------------------------------- */
#define SC_OK 0
#define SC_ERR_INVALID_ARG 1   /* bad shape / null pointer / bad enum (-> ValueError)        */
#define SC_ERR_INDEX 2         /* patch index out of range (-> IndexError, forcefield.py:953) */
#define SC_ERR_SELF_PAIR 3     /* contact_pair_on with i == j (-> ValueError, interaction.py:210) */
#define SC_ERR_NO_DEVICE 4     /* no HIP device / wrong architecture                          */
#define SC_ERR_HIP 5           /* a HIP runtime call failed                                   */
#define SC_ERR_NOMEM 6         /* device allocation failed                                    */
#define SC_ERR_NOCONV 7        /* eigensolver failed to converge                              */

/* ---- force-field descriptor ---------------------------------------------------------
 * Device-side restatement of ForceField.force_constant (forcefield.py:67-94) for the
 * force fields whose constants depend only on the distance:
 *   SC_FF_INVARIANT       gamma = 1                       (forcefield.py:264-289)
 *   SC_FF_HINSEN          d = max(sqrt(d2), 2.9); d < 4 ? 860 d - 2390 : 1.28e6 d^-6
 *                                                          (forcefield.py:292-330)
 *   SC_FF_PARAMETER_FREE  gamma = 1 / d2                  (forcefield.py:333-366)
 * TabulatedForceField has its own descriptor (SC_FF_TABULATED below).  Anything else (user subclasses,
 * nested patches) goes through the *_from_pairs entry points: the library returns the ordered pair list + squared distances, the host evaluates
 * force_constant() and hands gamma[k] back.
 */
#define SC_FF_INVARIANT 0
#define SC_FF_HINSEN 1
#define SC_FF_PARAMETER_FREE 2
#define SC_FF_TABULATED 3

/* SC_FF_TABULATED: device-side restatement of TabulatedForceField (forcefield.py:369-533).  gamma(i,j,d2) is
 * looked up in one of three float32 tables [type_i][type_j][bin] (C order (20,20,n_bins), the reference keeps
 * them in float32, forcefield.py:889-891):  `bonded` when the two atoms are consecutive C-alpha of one chain
 * (bonded_next[min(i,j)] and |i-j| == 1, forcefield.py:470-473,504-506), else `intra_chain` when
 * chain[i] == chain[j], else `inter_chain`; bin = number of squared edges < d2
 * (np.searchsorted(edges**2, d2), forcefield.py:521).  All pointers are HOST pointers. */
typedef struct sc_tab_desc {
  int32_t n_bins;             /* >= 1 */
  int32_t reserved;
  const double* edges_sq;     /* (n_bins,) squared right bin edges; may be NULL when n_bins == 1 */
  const float* bonded;        /* (20,20,n_bins) */
  const float* intra_chain;   /* (20,20,n_bins) */
  const float* inter_chain;   /* (20,20,n_bins) */
  const int32_t* atom_type;   /* (n_atoms,) amino-acid index 0..19 (alphabetical by one-letter code) */
  const int32_t* chain;       /* (n_atoms,) integer chain label */
  const uint8_t* bonded_next; /* (n_atoms,) 1: atom i is peptide-bonded to atom i+1 */
} sc_tab_desc;

typedef struct sc_ff_desc {
  int32_t kind;       /* SC_FF_* */
  int32_t has_cutoff; /* 0: cutoff_distance is None -> every i != j is a contact (interaction.py:151-153) */
  double cutoff;      /* cutoff_distance in Angstrom (informational) */
  double cutoff_sq;   /* cutoff_distance**2 evaluated by the host in float64 (interaction.py:166) */
  const sc_tab_desc* tab; /* SC_FF_TABULATED only, else NULL */
} sc_ff_desc;

/* ---- contact patches (ForceField.contact_shutdown / contact_pair_off / contact_pair_on,
 * forcefield.py:96-110; applied in the order of _patch_adjacency_matrix, interaction.py:193-213).
 * All pointers are host pointers and may be NULL when the matching count is 0.
 * on_force_constants (PatchedForceField, forcefield.py:183-226): NULL -> switched-on pairs
 * use the base force field's constant; otherwise one constant per pair_on row (a value of
 * exactly -1 means "no override", the sentinel of forcefield.py:213-224).
 * base_cutoff_masks_gamma: 1 -> pairs farther than the cutoff that are in contact only because
 * of pair_on get gamma = 0 unless overridden (PatchedForceField.force_constant,
 * forcefield.py:184-196); 0 -> the base force constant is evaluated at any distance. */
typedef struct sc_patch_desc {
  int64_t n_shutdown;
  const int64_t* shutdown; /* (n_shutdown,) atom indices */
  int64_t n_pair_off;
  const int64_t* pair_off; /* (n_pair_off, 2) */
  int64_t n_pair_on;
  const int64_t* pair_on;  /* (n_pair_on, 2) */
  const double* on_force_constants; /* (n_pair_on,) or NULL */
  int32_t base_cutoff_masks_gamma;
  int32_t reserved;
} sc_patch_desc;

/* ---- context ---------------------------------------------------------------------------
 * One context = one device + one stream + a cached device workspace.  Contexts are not
 * thread-safe; use one per host thread (the reference is single-threaded Python). */
typedef struct sc_ctx sc_ctx;

int sc_ctx_create(int device, sc_ctx** out);
/* Same, but enqueue on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream). */
int sc_ctx_create_on_stream(int device, void* hip_stream, sc_ctx** out);
void sc_ctx_destroy(sc_ctx* ctx);
const char* sc_last_error(sc_ctx* ctx);
/* Page-locked host memory for results (no reference counterpart: plumbing of the boundary).  The eigenvectors of one
 * N = 2000 ANM are 288 MB; copied into fresh pageable memory they take 17-25 ms, into page-locked memory 5 ms.  The Python
 * host (springcraft_amd/_hip.py:host_array) builds the NumPy arrays it returns on such blocks and keeps a bounded pool of
 * the ones whose arrays are gone.  Any host pointer is accepted by the entry points above; these blocks are merely faster.
 * sc_host_alloc: SC_ERR_NOMEM when the runtime refuses (the caller then uses ordinary memory), SC_ERR_INVALID_ARG for 0 bytes. */
int sc_host_alloc(size_t bytes, void** out);
int sc_host_free(void* p);

/* Block until everything enqueued on the context's stream has finished.  Returns SC_ERR_NOCONV (LinAlgError in the
 * Python layer, what np.linalg.eigh raises at nma.py:61) if a device-pointer eigensolve enqueued since the last call
 * met a matrix with a NaN / Inf entry -- that matrix is solved as the zero matrix and its eigenvalues are returned as
 * NaN, the other matrices of its batch are unaffected -- or a tridiagonal QL iteration that did not converge; the
 * condition is reported once. */
int sc_ctx_synchronize(sc_ctx* ctx);
/* Library / device identification for logs: fills `buf` with e.g. "gfx950 AMD Instinct MI355X, 256 CUs". */
int sc_device_info(sc_ctx* ctx, char* buf, size_t buflen);

/* ---- contact scan (replaces interaction.py:149-178: adjacency + np.where) ---------------
 * counts[i] = number of contacts of atom i (row sums of the adjacency matrix, int64, exact);
 * *n_pairs = total number of directed pairs k. */
int sc_contacts(sc_ctx* ctx, const double* coord, int64_t n_atoms, const sc_ff_desc* ff,
                const sc_patch_desc* patch, int64_t* counts, int64_t* n_pairs);

/* Ordered pair list: pairs is (k,2) int64, sorted by i then j, holding (i,j) and (j,i)
 * (np.where order, interaction.py:177-178).  sq_dist (k,) may be NULL; it is the reference's
 * (dx*dx + dy*dy) + dz*dz with separately rounded products (interaction.py:184).
 * `capacity` is the number of rows the caller allocated; fails with SC_ERR_INVALID_ARG when
 * the scan finds more. */
int sc_pairs(sc_ctx* ctx, const double* coord, int64_t n_atoms, const sc_ff_desc* ff,
             const sc_patch_desc* patch, int64_t capacity, int64_t* pairs, double* sq_dist,
             int64_t* n_pairs);

/* ---- assembly (replaces compute_kirchhoff interaction.py:14-54 and compute_hessian :57-111)
 * inv_sqrt_mass: NULL, or (n_atoms,) 1/sqrt(m_i): the matrix is multiplied element-wise by
 * outer(w, w) as GNM.kirchhoff / ANM.hessian do (gnm.py:85-87,104-105; anm.py:89-94,112-113). */
int sc_kirchhoff_f64(sc_ctx* ctx, const double* coord, int64_t n_atoms, const sc_ff_desc* ff,
                     const sc_patch_desc* patch, const double* inv_sqrt_mass, double* kirchhoff);
int sc_hessian_f64(sc_ctx* ctx, const double* coord, int64_t n_atoms, const sc_ff_desc* ff,
                   const sc_patch_desc* patch, const double* inv_sqrt_mass, double* hessian);

/* Host-callback path: the caller supplies the ordered pair list and gamma[k] (any Python
 * ForceField.force_constant).  Asymmetric gamma is honoured exactly as the reference does:
 * off-diagonal (i,j) from gamma(i,j), diagonal = -sum over the first index (interaction.py:52,104). */
int sc_kirchhoff_from_pairs_f64(sc_ctx* ctx, int64_t n_atoms, const int64_t* pairs, int64_t k,
                                const double* gamma, double* kirchhoff);
int sc_hessian_from_pairs_f64(sc_ctx* ctx, const double* coord, int64_t n_atoms,
                              const int64_t* pairs, int64_t k, const double* gamma,
                              double* hessian);

/* ---- dense symmetric eigensolve (replaces np.linalg.eigh at nma.py:61) -------------------
 * a: (n,n) symmetric, only the lower triangle is read (UPLO='L', numpy's default); not modified.
 * w: (n,) ascending eigenvalues.  v: NULL (values only) or (n,n), rows = modes (nma.py:63). */
int sc_eigh_f64(sc_ctx* ctx, const double* a, int64_t n, double* w, double* v);

/* Partial spectrum (no reference counterpart: np.linalg.eigh always returns all n pairs; this is the path of
 * BASELINE config 5, "lowest 100 modes only").  Eigenvalues with ascending index il..iu (0-based, inclusive):
 * w: (m,), v: NULL or (m,n) rows = modes, m = iu - il + 1.  Bisection + inverse iteration on the tridiagonal
 * matrix, back-transformation of the selected vectors only. */
int sc_eigh_range_f64(sc_ctx* ctx, const double* a, int64_t n, int64_t il, int64_t iu, double* w, double* v);

/* Eigenvalue window: the eigenpairs whose eigenvalues lie in the half-open interval (vl, vu], as
 * scipy.linalg.eigh(a, subset_by_value=(vl, vu)) selects them; vl = -INFINITY / vu = INFINITY are allowed, vl >= vu or a
 * NaN bound is SC_ERR_INVALID_ARG.  The count m is taken on the device by Sturm counts on the tridiagonal matrix that is
 * then solved (one tridiagonalisation), after which exactly m pairs are computed as sc_eigh_range_f64 computes them.  An
 * eigenvalue within about n eps |A| of a bound may fall on either side of it (as in LAPACK's dsyevr).
 * Results: *m, and *w (m,) ascending, *v (m, n) rows = modes (want_vectors != 0; v may be NULL otherwise) in page-locked
 * blocks from sc_host_alloc that the caller releases with sc_host_free; m = 0 leaves *w = *v = NULL. */
int sc_eigh_window_f64(sc_ctx* ctx, const double* a, int64_t n, double vl, double vu, int want_vectors, int64_t* m,
                       double** w, double** v);

/* Hermitian pseudo-inverse, replaces np.linalg.pinv(M, hermitian=True, rcond=1e-6) in the covariance / matrix
 * properties (anm.py:114-117,132-136; gnm.py:107-110,125-131): eigendecomposition on the device, then
 * (U * s) U^T with s_i = 1/w_i where |w_i| > rcond * max|w| and 0 elsewhere (one f64-MFMA GEMM).
 * a: (n,n) symmetric, lower triangle read, not modified; out: (n,n). */
int sc_pinvh_f64(sc_ctx* ctx, const double* a, int64_t n, double rcond, double* out);

/* Fused: coordinates -> Hessian (device) -> eigenpairs, no host round trip of the matrix.
 * Replaces ANM(coord, ff).eigen() (anm.py:150-167 -> nma.py:29-63) for built-in force fields. */
int sc_anm_eigen_f64(sc_ctx* ctx, const double* coord, int64_t n_atoms, const sc_ff_desc* ff,
                     const sc_patch_desc* patch, const double* inv_sqrt_mass, double* w, double* v);
int sc_gnm_eigen_f64(sc_ctx* ctx, const double* coord, int64_t n_atoms, const sc_ff_desc* ff,
                     const sc_patch_desc* patch, const double* inv_sqrt_mass, double* w, double* v);
/* Same, partial spectrum il..iu of the 3n x 3n Hessian (w: (m,), v: NULL or (m, 3n)). */
int sc_anm_eigen_range_f64(sc_ctx* ctx, const double* coord, int64_t n_atoms, const sc_ff_desc* ff,
                           const sc_patch_desc* patch, const double* inv_sqrt_mass, int64_t il, int64_t iu,
                           double* w, double* v);
/* Same, eigenvalue window (vl, vu] of the 3n x 3n Hessian (scipy's subset_by_value; results as sc_eigh_window_f64). */
int sc_anm_eigen_window_f64(sc_ctx* ctx, const double* coord, int64_t n_atoms, const sc_ff_desc* ff,
                            const sc_patch_desc* patch, const double* inv_sqrt_mass, double vl, double vu,
                            int want_vectors, int64_t* m, double** w, double** v);

/* ---- device-resident / batched entry points (bench + multi-structure sharding) ------------
 * All pointers are device pointers on the context's device.  Work is enqueued on the context's
 * stream; nothing synchronises (see the conventions at the top for the one exception and for
 * how errors found on the device are reported). */

/* d_coord: (batch, n_atoms, 3) f64.  d_matrix: (batch, dim*n_atoms, dim*n_atoms) f64, dim = 1
 * (Kirchhoff) or 3 (Hessian).  No patches on this path. d_inv_sqrt_mass: NULL or (batch, n_atoms). */
int sc_dev_kirchhoff_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int64_t batch,
                         const sc_ff_desc* ff, const double* d_inv_sqrt_mass, double* d_matrix);
int sc_dev_hessian_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int64_t batch,
                       const sc_ff_desc* ff, const double* d_inv_sqrt_mass, double* d_matrix);

/* ---- batches of DIFFERENT structures: sizes, force fields (incl. SC_FF_TABULATED) and patches per structure --------
 * The reference models one arbitrary structure per object (anm.py:62-63, gnm.py:58-59) with any force field
 * (forcefield.py:117-261 PatchedForceField, :369-533 TabulatedForceField) and optional mass weighting
 * (anm.py:89-94,112-113).  A plan stages everything but the coordinates once: every structure gets a slot of one common
 * matrix order (`order`, 0 = dim * the largest atom count), so that ONE sc_dev_eigh_f64(ctx, d_matrix, order, count, ..)
 * solves the whole batch.  A slot holds diag(M, D): the structure's matrix M in its leading dim * n_atoms rows / columns
 * and a diagonal pad D whose entries lie above every eigenvalue of M (between 2 and 4 times its largest absolute row
 * sum).  The blocks never mix, so of the slot's ascending eigenpairs the first dim * n_atoms are the structure's, with
 * its eigenvector components in the leading dim * n_atoms columns.
 * All descriptor pointers are HOST pointers and need not outlive sc_batch_plan_create.  For SC_FF_TABULATED the
 * per-atom arrays of ff->tab are the structure's own; parameter tables are uploaded once per distinct host array. */
typedef struct sc_structure_desc {
  int64_t n_atoms;
  const sc_ff_desc* ff;
  const sc_patch_desc* patch; /* NULL: none */
} sc_structure_desc;
typedef struct sc_batch_plan sc_batch_plan;
int sc_batch_plan_create(sc_ctx* ctx, int dim, const sc_structure_desc* structures, int64_t count, int64_t order,
                         sc_batch_plan** out);
/* d_coord: (sum n_atoms, 3) f64, the structures back to back.  d_inv_sqrt_mass: NULL or (sum n_atoms,).
 * d_matrix: (count, order, order) f64.  Enqueued on the context's stream, nothing synchronises. */
int sc_batch_plan_assemble_f64(sc_batch_plan* plan, const double* d_coord, const double* d_inv_sqrt_mass,
                               double* d_matrix);
/* Host-callback force fields for a whole batch: any Python ForceField.force_constant (forcefield.py:67-94; the use
 * doc/advanced.rst:23-70 documents and tests/test_interaction.py:92-116 exercises), which compute_kirchhoff /
 * compute_hessian evaluate on the ordered pair list (interaction.py:49,96).  The plan's descriptors then only drive
 * the contact scan (cutoff + adjacency patches, interaction.py:149-178):
 *   1. sc_batch_plan_contacts: n_pairs[count] (host) = directed contacts per structure;
 *   2. sc_batch_plan_pairs: pair lists of ALL structures in one launch, back to back -- per structure in np.where order
 *      (sorted by i then j, both directions, interaction.py:177-178), LOCAL atom indices; pair_off[count + 1] (host) =
 *      first row of every structure; sq_dist (may be NULL) as in sc_pairs; `capacity` rows were allocated;
 *   3. the caller evaluates gamma[k] per structure;
 *   4. sc_batch_plan_fill_from_pairs_f64: all padded slots from pairs + gamma in one pass over the batch.  Asymmetric
 *      gamma is honoured as the reference does: element (i, j) from gamma(i, j), diagonal (blocks) = minus the sums
 *      over the FIRST index (interaction.py:50-52,103-104); d_inv_sqrt_mass as in sc_batch_plan_assemble_f64.
 * pairs / sq_dist / gamma / pair_off / n_pairs are HOST pointers, d_coord / d_matrix device pointers; all three calls
 * synchronise the context's stream (the constants come from the host in between anyway). */
int sc_batch_plan_contacts(sc_batch_plan* plan, const double* d_coord, int64_t* n_pairs);
int sc_batch_plan_pairs(sc_batch_plan* plan, const double* d_coord, int64_t capacity, int64_t* pairs, double* sq_dist,
                        int64_t* pair_off);
int sc_batch_plan_fill_from_pairs_f64(sc_batch_plan* plan, const double* d_coord, const int64_t* pairs,
                                      const int64_t* pair_off, const double* gamma, const double* d_inv_sqrt_mass,
                                      double* d_matrix);
int64_t sc_batch_plan_order(const sc_batch_plan* plan);
/* Must be destroyed before its context. */
void sc_batch_plan_destroy(sc_batch_plan* plan);

/* Batched eigensolve of `batch` independent (n,n) symmetric matrices.
 * d_a: (batch,n,n), lower triangle read, DESTROYED (used as workspace).
 * d_w: (batch,n).  d_v: NULL or (batch,n,n) rows = modes. */
int sc_dev_eigh_f64(sc_ctx* ctx, double* d_a, int64_t n, int64_t batch, double* d_w, double* d_v);

/* Partial spectrum of `batch` matrices: d_w (batch, m), d_v NULL or (batch, m, n). d_a is destroyed. */
int sc_dev_eigh_range_f64(sc_ctx* ctx, double* d_a, int64_t n, int64_t batch, int64_t il, int64_t iu,
                          double* d_w, double* d_v);
/* Eigenvalue window (vl, vu] of `batch` matrices (scipy's subset_by_value semantics, as sc_eigh_window_f64), enqueue only.
 * Every matrix gets a slot of K = capacity (1 <= K <= n) eigenpairs: d_w (batch, K), d_v NULL or (batch, K, n), and
 * d_count (batch,) int64 receives the TRUE count of every window.  A slot holds the first min(count, K) eigenpairs of its
 * window in ascending order, then NaN in d_w and zero rows in d_v.  A matrix with a NaN / Inf entry gets count 0 (and is
 * reported as sc_dev_eigh_f64 reports it).  d_a is destroyed. */
int sc_dev_eigh_window_f64(sc_ctx* ctx, double* d_a, int64_t n, int64_t batch, double vl, double vu, int64_t capacity,
                           double* d_w, double* d_v, int64_t* d_count);

/* Tridiagonalisation path of the eigensolver: -1 automatic (default: two-stage when n >= 512 and
 * batch * n^2 >= max(2e7, 1e4 n), else one-stage), 0 always one-stage, 1 two-stage whenever n >= 256.  Both give the
 * same eigenpairs to rounding (|dw| ~ 1e-14 |w|max); the choice only affects speed. */
int sc_ctx_set_two_stage(sc_ctx* ctx, int mode);

/* Bytes of device workspace sc_dev_eigh_f64 will hold for (n, batch) (allocated lazily, cached). */
int64_t sc_eigh_workspace_bytes(int64_t n, int64_t batch, int want_vectors);

/* Per-phase device timings (ms, HIP events on the context's stream) of the most recent
 * sc_dev_eigh_f64 when profiling was enabled with sc_ctx_set_profiling(ctx, 1):
 * out[0]=tridiagonalisation, out[1]=tridiagonal eigensolver, out[2]=back-transformation, and
 *   one-stage path (out[5] == 0): out[3]=SYMV kernels only (sum), out[4]=SYR2K kernels only (sum);
 *   two-stage path (out[5] > 0):  out[3]=stage 1 (band reduction), out[4]=stage 2 (bulge chasing),
 *                                 out[5]=the fused stage-2 back-transformation kernel alone. */
int sc_ctx_set_profiling(sc_ctx* ctx, int enabled);
int sc_last_eigh_timings(sc_ctx* ctx, double* out6);
/* Summed device time (ms) of one kernel group of the most recent profiled eigensolve, by name.  Two-stage path:
 * "panel_qr", "symm" (X = A22 V), "syr2k" (trailing update), "bulge", "dia_tfactor", "dc" (tridiagonal divide & conquer),
 * "dc_gemm" (its merge GEMMs), "bt2" (stage-2 back-transformation), "bt1_w" / "bt1_update" (the two GEMMs of the stage-1
 * back-transformation).  One name is not a time: "dc_gemm_gflop" = 1e9 flops those merge GEMMs executed (2 m n k summed on
 * the device over their records: the sizes depend on the deflation and exist nowhere else).
 * Unknown names (or phases the last solve did not run): SC_ERR_INVALID_ARG, *ms = 0. */
int sc_last_eigh_phase_ms(sc_ctx* ctx, const char* name, double* ms);

/* Event counters of the context since it was created (monitoring; nothing in the reference corresponds).  Since round 6
 * the persistent kernels' outcomes are collected on the device while solves are being enqueued; this call waits for the
 * context's stream and reads them (as sc_ctx_synchronize does).  Names:
 *   "chase_launches"   persistent bulge chases started (two-stage path): one launch for the whole stage
 *   "chase_pair_launches"   of those, how many ran in the pair form (two sweeps per workgroup through LDS, the form for
 *                      batches that are bound by memory traffic; smaller ones take one sweep per workgroup)
 *   "chase_timeouts"   of those, how many ran into the bound of an inter-workgroup wait -- expected to stay 0; the
 *                      solve is still finished correctly, on the device, by the take-over launch behind the chase
 *                      ("chase_resumed" counts every such take-over, "chase_incomplete" a chase that ended without a
 *                      flag but with sweeps left), and the context stops using the persistent form
 *   "chase_sweeps"     sweeps the persistent chases finished themselves
 *   "stepwise_chases"  bulge chases that ran as per-wavefront launches from the start
 *   "chase_xcd_min" / "chase_xcd_max"   workgroups per XCD in the most recent persistent chase (the spread form, one
 *                      matrix on all XCDs, counts as one XCD)
 *   "chase_xcd_total"  workgroups of the most recent persistent chase (its grid)
 *   "chase_wait_matrix" / "_sweep" / "_task"   where the last timed-out wait stood (-1: never)
 *   "chase_pair_fallbacks"   pair launches the device refused (dynamic LDS) and that were re-issued in the one-sweep form
 *   "xcd_count"        XCDs of the device as a probe launch saw them (0: not probed yet)
 *   "gemm3_launches"   launches the role-split persistent GEMM (k_gemm3) took
 *   "symm3_launches"   launches of the band reduction's symmetric product X = A22 V as one role-split kernel (k_symm3)
 *   "resident_launches" / "resident_takeovers"   one-stage reductions of one matrix done by the single launch that keeps
 *                      its rows in LDS (k_sytrd_resident), and those of them its take-over kernel had to do instead
 *                      ("resident_rollcall_failures": because its workgroups were not all resident in time;
 *                      "resident_lost_waits": because a wait between them ran into its bound; "resident_lost_at" = step << 32 | workgroup
 *                      of that wait, resp. the workgroups that had arrived when the roll call was given up)
 *   "panel_coop_launches"   panel factorisations by the cooperative kernel (k_panel_coop: several workgroups of one launch)
 *   "panel_coop_timeouts"   panels (per matrix) the cooperative kernel gave up on -- a wait between its workgroups ran
 *                      into its bound; expected to stay 0 -- and the take-over launch behind it factored instead: the
 *                      solve is correct, the context keeps to the chunked panel launches afterwards (until round 5 the
 *                      solve returned SC_ERR_NOCONV)
 * Unknown names: SC_ERR_INVALID_ARG, *value = 0. */
int sc_ctx_get_counter(sc_ctx* ctx, const char* name, int64_t* value);

/* ---- device-resident eigenpairs and their consumers ----------------------------------
 * An sc_modes object holds all n eigenvalues and eigenvectors of one model's Kirchhoff (dim 1) or Hessian
 * (dim 3) matrix in device memory, so that the quantities the reference derives from nma.eigen
 * (nma.py:66-105 frequencies, :108-184 mean_square_fluctuation, :187-230 bfactor, :233-359 dcc, :476-524 prs)
 * are computed without solving again and without moving the (n, n) eigenvector matrix over PCIe.
 * It belongs to the context it was created with and must be destroyed before that context. */
typedef struct sc_modes sc_modes;

/* Assemble the ANM Hessian (dim 3) / GNM Kirchhoff matrix (dim 1) from coordinates and solve it, all on device
 * (same arguments as sc_anm_eigen_f64 / sc_gnm_eigen_f64). */
int sc_modes_from_coord(sc_ctx* ctx, const double* coord, int64_t n_atoms, int dim, const sc_ff_desc* ff,
                        const sc_patch_desc* patch, const double* inv_sqrt_mass, sc_modes** out);
/* Solve a host matrix (n, n) (lower triangle read, as numpy.linalg.eigh at nma.py:61); n must be a multiple of dim. */
int sc_modes_from_matrix(sc_ctx* ctx, const double* a, int64_t n, int dim, sc_modes** out);
void sc_modes_destroy(sc_modes* modes);
int64_t sc_modes_order(const sc_modes* modes);
/* Copy out: w (n) ascending, v (n, n) rows = modes (either may be NULL). */
int sc_modes_get(sc_modes* modes, double* w, double* v);
/* out (n / dim): sum over the k listed modes of v^2 / w, summed over the dim components of every atom. */
int sc_modes_msf(sc_modes* modes, const int64_t* mode_idx, int64_t k, double* out);
/* ANM only (a dim-1 object: SC_ERR_INVALID_ARG).  out (n / 3, 6): per atom the 3 x 3 tensor sum over the k listed modes
 * of v_a v_a^T / w -- the diagonal blocks of the covariance over those modes, the anisotropic displacement parameters --
 * as its six distinct entries in the order of a PDB ANISOU record: xx yy zz xy xz yz.  xx + yy + zz is sc_modes_msf's
 * value.  Computed by the batch kernels below with a batch of one. */
int sc_modes_aniso(sc_modes* modes, const int64_t* mode_idx, int64_t k, double* out);
/* No reference counterpart (ProDy: calcOverlap / calcCollectivity; Bio3D: overlap); replaces pulling v to the host for
 * them.  Host pointers.  disp (q, n): q displacement vectors in the coordinates of a mode (for a mass-weighted solve the
 * caller passes sqrt(mass) * d).  overlap_out (q, k): <v_i, d_j> / (|v_i| |d_j|) for the k listed modes, signed; a zero
 * d_j gives NaN.  collectivity_out (k): exp(-sum_a p_a ln p_a) / (n / dim) with p_a the share of atom a in |v_i|^2
 * (a rigid translation: 1; a mode on one atom: dim / n).  overlap_out may be NULL with q = 0, collectivity_out may be
 * NULL, not both.  GNM and ANM.  A mode index outside 0..n-1 (negative ones count from the end): SC_ERR_INDEX.
 * Computed by sc_dev_modes_overlap_f64's kernel with a batch of one. */
int sc_modes_overlap(sc_modes* modes, const int64_t* mode_idx, int64_t k, const double* disp, int64_t q,
                     double* overlap_out, double* collectivity_out);
/* No reference counterpart (ProDy: calcDistFlucts / calcMechStiff).  ANM only (a dim-1 object: SC_ERR_INVALID_ARG).
 * coord: host (n / 3, 3), the coordinates the model was built from; out: host (n / 3, n / 3), for atoms a, c the
 * fluctuation of their distance over the k listed modes, sum of (n_ac . (v[c] - v[a]))^2 / w with n_ac the unit vector
 * from a to c; symmetric bit for bit, the diagonal exactly 0, NaN for two distinct atoms at one position.  Computed by
 * sc_dev_modes_distfluct_f64's kernel with a batch of one (no atom scale: a mass-weighted model's modes enter as they are). */
int sc_modes_distfluct(sc_modes* modes, const int64_t* mode_idx, int64_t k, const double* coord, double* out);
/* Linear response of the model to q forces (nma.py:422-473 linear_response = covariance @ force) in mode space, without
 * the (n, n) covariance.  Host pointers.  force (q, n), out (q, n): out_j = S sum_i v_i <v_i, S f_j> / w_i over the selected
 * modes, S = diag(atom_scale) per atom (atom_scale (n / dim) or NULL for 1: a mass-weighted model passes 1 / sqrt(mass)
 * for the Cartesian response).  mode_idx != NULL: the k listed modes (rcond is not read).  mode_idx == NULL (k must be 0):
 * every mode with |w| > rcond max|w|, the rule of numpy.linalg.pinv(hermitian=True) behind the reference's covariance
 * (anm.py:114-117), as sc_modes_prs takes it; out is then pinv(H, rcond) f.  A mode index outside 0..n-1 (negative ones
 * count from the end): SC_ERR_INDEX.  Computed by sc_dev_mode_response_f64's kernels with a batch of one. */
int sc_modes_response(sc_modes* modes, const int64_t* mode_idx, int64_t k, double rcond, const double* force, int64_t q,
                      const double* atom_scale, double* out);
/* Displacements built from the modes: no reference counterpart (ProDy: deformAtoms / traverseMode / sampleModes).  Host
 * pointers.  coef (q, k), out (q, n): out_j = sum_i coef[j, i] v_(mode_idx[i]) over the k listed modes, added in the order
 * of the list; the inverse of sc_modes_overlap over a complete set.  GNM and ANM; k = 0 gives zeros.  Computed by
 * sc_dev_mode_combine_f64's kernels with a batch of one. */
int sc_modes_combine(sc_modes* modes, const int64_t* mode_idx, int64_t k, const double* coef, int64_t q, double* out);
/* out (n / dim, n / dim): sum over the listed modes of <v_a, v_b> / w; norm != 0 divides by sqrt(c_aa c_bb). */
int sc_modes_dcc(sc_modes* modes, const int64_t* mode_idx, int64_t k, int norm, double* out);
/* ANM only. out (n / 3, n / 3) row-major: sums of the squared 3x3 blocks of pinv(H, rcond) (numpy hermitian
 * rule); norm != 0 divides row a by out[a, a]. */
int sc_modes_prs(sc_modes* modes, double rcond, int norm, double* out);
/* The same matrix over the k listed modes only (no reference counterpart: the reference scans the whole covariance):
 * out[a, c] = sum over the 3 x 3 entries of (sum_i v_i[a] v_i[c]^T / w_i)^2, i over the list in its order, a mode listed
 * twice counts twice.  ANM only; a mode index outside 0..n-1 (negative ones count from the end): SC_ERR_INDEX; k = 0 gives
 * zeros (NaN under norm).  Computed by sc_dev_prs_f64's kernel with a batch of one: no (n, n) covariance is formed. */
int sc_modes_prs_subset(sc_modes* modes, const int64_t* mode_idx, int64_t k, int norm, double* out);
/* Generalized correlation of every atom pair from the linear mutual information (Lange & Grubmueller 2006; no reference
 * counterpart, Bio3D: lmi) over the k listed modes, or with a NULL list (its k must be 0) over every mode with |w| > rcond
 * max|w|, the covariance rule of sc_modes_prs.  out (n / 3, n / 3): r in [0, 1], or with information != 0 the mutual
 * information in nats; see sc_dev_lmi_f64, whose kernels compute it with a batch of one.  ANM only; a mode index outside
 * 0..n-1 (negative ones count from the end): SC_ERR_INDEX; fewer than three modes give NaN everywhere. */
int sc_modes_lmi(sc_modes* modes, const int64_t* mode_idx, int64_t k, double rcond, int information, double* out);
/* How the modes of model a compare with those of model b: no reference counterpart (Bio3D: rmsip / covsoverlap; ProDy:
 * calcSubspaceOverlap / calcCovOverlap / calcOverlap of two mode sets).  Host pointers.  The two objects must belong to one
 * context and have the same dim and order (SC_ERR_INVALID_ARG otherwise: structures of different size have no common
 * coordinates).  With G[i, j] = <v_a,i, v_b,j> over the k_a / k_b listed modes and S = sum_ij p_a,i p_b,j G[i, j]^2:
 *   kind 0, RMSIP:              p = 1, t = k:                     *out_value = sqrt(S / sqrt(t_a t_b))   (Amadei's sqrt(sum G^2 / k) for k_a = k_b = k)
 *   kind 1, covariance overlap: p = 1 / sqrt(w), t = sum 1 / w:   *out_value = 1 - sqrt(max(0, t_a + t_b - 2 S) / (t_a + t_b))       (Hess 2002)
 * out_gram: NULL, or (k_a, k_b) for G itself, the table one matches modes with; out_value may be NULL when it is given.  A
 * NULL list (its k must be 0, out_gram NULL): every mode with |w| > rcond max|w|, the covariance rule of sc_modes_prs; rcond
 * is not read otherwise.  A mode index outside 0..n-1 (negative ones count from the end): SC_ERR_INDEX; a mode listed twice
 * counts twice.  Computed by sc_dev_subspace_f64's kernel on two batches of one. */
int sc_modes_subspace(sc_modes* a, sc_modes* b, const int64_t* mode_idx_a, int64_t k_a, const int64_t* mode_idx_b,
                      int64_t k_b, double rcond, int kind, double* out_value, double* out_gram);

/* ---- the same consumers for a batch: device pointers in, device pointers out, enqueue only ------------------------
 * What nma.py:108-184 (mean_square_fluctuation) and nma.py:233-359 (dcc) derive from nma.eigen for ONE model, for every
 * structure of a batch at once and on the very tensors the batched solvers above leave in device memory: d_w (batch,
 * nvec), d_v (batch, nvec, m) rows = modes, and, behind a window solve, d_counts (batch,) int64.  Like the solvers they
 * only enqueue on the context's stream; nothing is copied to the host, the eigenvalues included.
 *
 *   msf[b, a]    = sum_r  s[b, r] * sum_d V[b, r, dim a + d]^2
 *   dcc[b, a, c] = sum_r  s[b, r] * sum_d V[b, r, dim a + d] V[b, r, dim c + d]
 *   U[b, a, d, e] = sum_r  s[b, r] * V[b, r, 3 a + d] V[b, r, 3 a + e]      (dim 3 only: anisotropic fluctuation tensors)
 *
 * with s[b, r] = 1 / w[b, r] for a selected row r and exactly 0 for every other one: a row without weight contributes
 * nothing, whatever it holds (the NaN / zero padding of a window solve).  The selection names ROWS of d_w / d_v, not
 * global mode indices -- the caller knows which modes it solved:
 *   SC_SEL_FROM_ROW  every row r >= row0                                 (nma.py:161-163: all non-trivial modes)
 *   SC_SEL_ROWS      the n_rows rows listed in d_rows, int32 in DEVICE memory and shared by all structures; a row listed
 *                    twice counts twice, as NumPy's fancy indexing makes it at nma.py:167-168 / :339-340; an entry
 *                    outside 0..nvec-1 is not read and turns the structure's result into NaN
 *   SC_SEL_PINV      every row with |w| > rcond * max|w|, the maximum taken per structure on the device: the rule of
 *                    numpy.linalg.pinv(hermitian=True) behind the covariance the reference takes for "all modes"
 *                    (nma.py:324-336, anm.py:114-117); only meaningful when all m modes were solved
 * d_counts != NULL clips every selection to the rows r < min(d_counts[b], nvec) of structure b.
 * A structure whose eigenvalues are NaN (a matrix with a NaN / Inf entry) gets NaN results, its neighbours are unaffected. */
#define SC_SEL_FROM_ROW 0
#define SC_SEL_ROWS 1
#define SC_SEL_PINV 2
typedef struct sc_mode_selection {
  int32_t kind;
  int32_t reserved;      /* 0 for the sc_dev_* entries; sc_batch_plan_modes_*: first_row, see there */
  int64_t row0;          /* SC_SEL_FROM_ROW */
  const int32_t* d_rows; /* SC_SEL_ROWS: (n_rows,) device memory */
  int64_t n_rows;
  double rcond;          /* SC_SEL_PINV */
} sc_mode_selection;

/* d_out (batch, m / dim).  One pass over the selected rows of d_v; a structure's result does not depend on the batch
 * size or on its position in the batch, bit for bit. */
int sc_dev_modes_msf_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                         int dim, const sc_mode_selection* sel, const int64_t* d_counts, double* d_out);
/* d_out (batch, m / dim, m / dim); norm != 0 divides by sqrt(c_aa c_cc) (nma.py:352-354; 0 / 0 = NaN for an empty
 * selection, as in NumPy).  One grouped float64 MFMA GEMM per slab of structures: the packed operands take at most
 * budget_bytes (0: SPRINGCRAFT_MODES_BUDGET_BYTES, else 1 GiB) at a time -- structures in slabs, and when one
 * structure's operands do not fit, its rows in chunks that accumulate.  The chunks depend on (m, rows, dim, budget)
 * only and every slab of a call uses the same block tile, so a structure's result does not depend on its position. */
int sc_dev_modes_dcc_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                         int dim, const sc_mode_selection* sel, const int64_t* d_counts, int norm, int64_t budget_bytes,
                         double* d_out);
/* ANM only: m % 3 == 0 is required (SC_ERR_INVALID_ARG otherwise).  d_out (batch, m / 3, 6): per atom the six distinct
 * entries of the symmetric 3 x 3 tensor U above in the order of a PDB ANISOU record, xx yy zz xy xz yz; its trace is the
 * msf of the same selection.  No reference counterpart: these are the diagonal 3 x 3 blocks of the covariance
 * (anm.py:114-117) restricted to the selected modes, without forming it.  One pass over the selected rows of d_v, the
 * rows split in chunks by their number alone and the chunks added in a fixed order: a structure's result does not depend
 * on the batch size or on its position in the batch, bit for bit.  Enqueue only. */
int sc_dev_modes_aniso_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                           const sc_mode_selection* sel, const int64_t* d_counts, double* d_out);
/* Overlaps of every row of d_v with displacement vectors, and the rows' collectivities: no reference counterpart (ProDy:
 * calcOverlap / calcCollectivity; Bio3D: overlap); replaces copying d_v (18 GB at 64 x 6000 x 6000) to the host for a
 * (batch, q, nvec) result.  d_disp (batch, q, m): q vectors per structure in the coordinates of a row (mass-weighted
 * solve: the caller passes sqrt(mass) * d).  d_overlap (batch, q, nvec): O[b, j, r] = <v_r, d_j> / (|v_r| |d_j|), signed;
 * a zero row or a zero d_j gives NaN.  d_collectivity (batch, nvec): exp(-sum_a p_a ln p_a) / N, p_a = s_a / sum s, s_a =
 * the squared norm of atom a's dim components of the row, N = m / dim; a term with p_a = 0 is exactly 0.  d_overlap may
 * be NULL with q = 0 (collectivity only), d_collectivity may be NULL; both NULL, q < 0 or m % dim != 0:
 * SC_ERR_INVALID_ARG.  d_counts: NULL, or the counts of a window solve: rows r >= min(d_counts[b], nvec) are NaN in both
 * outputs and are not read.  One pass over d_v, every row read once for the q vectors (in groups of four) and the
 * collectivity together; no atomics, every sum a fixed sequence given by (m, dim): O[b, j, r] and the collectivity of a
 * row do not depend, bit for bit, on the batch size, the structure's position, its neighbours, q or the vectors beside
 * d_j.  A structure whose d_v is NaN gives NaN and leaves its neighbours alone; d_w is not read, so a structure whose
 * batch solve failed (NaN eigenvalues beside a finite d_v without a meaning) is the caller's to mask, as
 * DeviceBatchSolver.overlap does.  No workspace.  Enqueue only. */
int sc_dev_modes_overlap_f64(sc_ctx* ctx, const double* d_v, int64_t m, int64_t nvec, int64_t batch, int dim,
                             const double* d_disp, int64_t q, const int64_t* d_counts, double* d_overlap,
                             double* d_collectivity);
/* Fluctuations of the inter-atom distances over the selected rows: no reference counterpart (ProDy: calcDistFlucts, and
 * calcMechStiff for k_B T over it; Bio3D derives it from the covariance); replaces copying d_v to the host or forming the
 * 3N x 3N covariance for a (batch, N, N) result.  ANM only: m % 3 == 0 is required (SC_ERR_INVALID_ARG otherwise), N = m / 3.
 *
 *   F[b, a, c] = sum_r  s[b, r] * ( n_ac . (u_r[c] - u_r[a]) )^2,   n_ac = (x_c - x_a) / |x_c - x_a|
 *
 * with s and the selection as above, x = d_coord (batch, N, 3) -- the coordinates the matrices were assembled from -- and
 * u_r[a] = d_atom_scale[b, a] * V[b, r, 3 a .. 3 a + 2]; d_atom_scale (batch, N) may be NULL (1): a mass-weighted solve
 * passes its 1 / sqrt(mass) to get Cartesian distances.  d_out (batch, N, N): F[a, c] and F[c, a] are the same bits, F[a,
 * a] is exactly 0 (also in a structure whose other entries are NaN), F >= 0 for positive weights; two distinct atoms at
 * one position give NaN for that pair (0 / 0 has no direction).  The sum is taken directly, pair by pair on the float64
 * vector unit with the unit vectors and the sums in registers (the expanded form over covariance blocks cancels for
 * neighbours): one fixed sequence over the listed rows per pair, no atomics, no partial sums, so a structure's result does
 * not depend on the batch size or on its position, bit for bit.  A row without weight is not read, nor is a listed row
 * outside 0..nvec-1, which turns the structure's result into NaN.  Enqueue only. */
int sc_dev_modes_distfluct_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                               const sc_mode_selection* sel, const int64_t* d_counts, const double* d_coord,
                               const double* d_atom_scale, double* d_out);
/* Perturbation-response scanning (nma.py:476-524 prs, there cov**2 of one model reduced by two reduceat) for a batch and
 * over the selected rows.  ANM only: m = 3 N (m % 3 != 0: SC_ERR_INVALID_ARG), d_out (batch, N, N),
 *
 *   C_ac[d, e] = sum_r s[b, r] u_r[a][d] u_r[c][e],   u_r[a] = t_a V[b, r, 3 a .. 3 a + 2]
 *   P[b, a, c] = sum_{d, e} C_ac[d, e]^2              norm != 0: P[b, a, c] / P[b, a, a]
 *
 * t = d_atom_scale (batch, N) or NULL for 1 (a mass-weighted solve passes 1 / sqrt(mass) for the Cartesian covariance).
 * One kernel on the float64 matrix units: a block C_ac is accumulated and squared in registers, no covariance entry is
 * written to memory and the only workspace is the weights and one diagonal per structure.  Every unordered pair is computed
 * once, so without norm P equals its transpose bit for bit; no atomics and no partial sums, so a structure's result does
 * not depend on the batch size, its position or its neighbours, bit for bit.  A row without weight is not read, nor is a
 * listed row outside 0..nvec-1, which turns the structure's result into NaN; an empty selection gives zeros, and NaN
 * under norm.  Enqueue only. */
int sc_dev_prs_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                   const sc_mode_selection* sel, const int64_t* d_counts, const double* d_atom_scale, int norm,
                   double* d_out);
/* Generalized correlation of atom pairs from the linear mutual information (Lange & Grubmueller 2006; no reference
 * counterpart, Bio3D: lmi, correlationplus) for a batch and over the selected rows.  ANM only: m = 3 N (m % 3 != 0:
 * SC_ERR_INVALID_ARG), d_out (batch, N, N),
 *
 *   C_ac  = sum_r s[b, r] v_r[a] v_r[c]^T,   v_r[a] = V[b, r, 3 a .. 3 a + 2]          (3 x 3)
 *   P_a C_aa P_a^T = L_a L_a^T (Cholesky with diagonal pivoting),  W_a = L_a^-1 P_a,  M = W_a C_ac W_c^T
 *   delta = det(I - M M^T) clamped to [0, 1]
 *   r[b, a, c] = sqrt(1 - delta^(1/3))          information != 0: I[b, a, c] = -1/2 ln(delta), in nats
 *
 * Both are invariant under any invertible linear map per atom, so there is no temperature and no per-atom scale: a
 * mass-weighted solve gives the Cartesian result.  [a, a] is 1.0 / +inf by definition.  A block C_aa with a Cholesky pivot
 * that is not finite or is <= 2^-40 times its own diagonal entry (fewer than three selected rows, an atom at rest in the
 * selection) cannot be whitened: row and column a are NaN, [a, a] included; so an empty selection gives NaN.  With exactly
 * three rows delta is 0 up to rounding: r = 1 up to rounding and I is large or +inf, never NaN.
 * The diagonal blocks are the tensors of sc_dev_modes_aniso_f64's kernels, summed in chunks of 128 listed rows and whitened
 * in the workspace (nine doubles per atom); then one kernel on the float64 matrix units with the data flow of
 * sc_dev_prs_f64's: a block C_ac is accumulated in registers and reduced to its value there, no covariance entry is
 * written to memory.  Every unordered pair is computed once, so the result equals its transpose bit for bit.  No atomics,
 * no partial sums across workgroups, and the tensors' chunks are cut at fixed rows: a structure's result does not depend
 * on the batch size, its position or its neighbours, bit for bit, and rows without weight behind its last weighted row
 * (the padding of a window, the pad rows of a plan's slot) do not change it either.  A row without weight is not read, nor
 * is a listed row outside 0..nvec-1, which turns the structure's result into NaN, as NaN eigenvalues do.  Enqueue only. */
int sc_dev_lmi_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                   const sc_mode_selection* sel, const int64_t* d_counts, int information, double* d_out);
/* How the modes of structure a compare with those of structure b, for every pair of two uniform batches of one m: no
 * reference counterpart (Bio3D: rmsip / covsoverlap; ProDy: calcSubspaceOverlap / calcCovOverlap); replaces copying d_v
 * to the host.  Two operand sets (d_w, d_v, sel, d_counts, nvec, batch) as above, each with its own selection; GNM and ANM.
 *
 *   G_ab[i, j] = <V_a[row_a(i)], V_b[row_b(j)]>      S[a, b] = sum_ij p[a, i] p[b, j] G_ab[i, j]^2
 *   kind 0, RMSIP:               p = 1 for a selected row,            t = sum_i p,      d_out[a, b] = sqrt(S / sqrt(t_a t_b))
 *   kind 1, covariance overlap:  p = 1 / sqrt(w) for a selected row,  t = sum_i 1 / w,  d_out[a, b] = 1 - sqrt(max(0, t_a + t_b - 2 S) / (t_a + t_b))
 *
 * p is exactly 0 for every other row.  d_out (batch_a, batch_b); d_s NULL or the raw S of that shape; d_t_a (batch_a) and
 * d_t_b (batch_b) NULL or t.  d_v_b NULL: the first set with itself -- every other argument of the second set must be NULL
 * / is not read, only the pairs a >= b are computed and both places written from one value, so d_out equals its transpose
 * bit for bit.  One kernel on the float64 matrix units: a tile of G_ab is accumulated along m, squared and summed in
 * registers; no entry of G reaches memory, the workspace is the weights and one partial sum per (pair, tile).  No
 * atomics, no split along m, one tile size per call from the numbers of listed rows alone: an entry's bits depend on
 * the two structures' own (w, v, selection) and the side each is on, not on the batch sizes, their positions or their
 * neighbours.  A row without weight is not read, nor is a listed row outside 0..nvec-1; such a row, and NaN eigenvalues (a
 * failed structure), turn that structure's row and column of d_out into NaN and no other entry.  An empty selection gives
 * S = 0 (RMSIP: 0 / 0 = NaN).  kind 1 wants positive eigenvalues: a selected w < 0 gives NaN.  Enqueue only. */
int sc_dev_subspace_f64(sc_ctx* ctx, const double* d_w_a, const double* d_v_a, const sc_mode_selection* sel_a,
                        const int64_t* d_counts_a, int64_t nvec_a, int64_t batch_a, const double* d_w_b,
                        const double* d_v_b, const sc_mode_selection* sel_b, const int64_t* d_counts_b, int64_t nvec_b,
                        int64_t batch_b, int64_t m, int kind, double* d_out, double* d_s, double* d_t_a, double* d_t_b);
/* The raw G_ab above, the table one matches modes with, for the n_pairs listed pairs: d_pairs int32 (n_pairs, 2) in DEVICE
 * memory, (structure of the first set, structure of the second); d_out (n_pairs, n_a, n_b) with n_a / n_b the listed rows of
 * the two selections.  The same kernel with a store in place of the squared sum.  d_v_b NULL: both structures of a pair
 * come from the first set.  A pair that names no structure gives NaN, as do NaN eigenvalues and a listed row outside
 * 0..nvec-1; a row without weight gives zeros.  Enqueue only. */
int sc_dev_subspace_gram_f64(sc_ctx* ctx, const double* d_w_a, const double* d_v_a, const sc_mode_selection* sel_a,
                             int64_t nvec_a, int64_t batch_a, const double* d_w_b, const double* d_v_b,
                             const sc_mode_selection* sel_b, int64_t nvec_b, int64_t batch_b, int64_t m,
                             const int32_t* d_pairs, int64_t n_pairs, double* d_out);
/* Linear response to q forces per structure over the selected rows (nma.py:422-473 linear_response = covariance @ force,
 * there for one model and through the (3N, 3N) pseudo-inverse), in mode space: no covariance and no m x m workspace.
 *
 *   c[b, j, r] = <v_r, g_j> s[b, r],  g_j[dim a + d] = t_a f_j[dim a + d]             (one pass ALONG the listed rows)
 *   X[b, j, dim a + d] = t_a sum_r c[b, j, r] V[b, r, dim a + d]                        (one pass ACROSS them)
 *
 * with s and the selection as above and t = d_atom_scale (batch, m / dim), NULL for 1.  d_force and d_out (batch, q, m).
 * With SC_SEL_PINV on a full spectrum and t = 1 this is pinv(H, rcond) f; with t = 1 / sqrt(mass) behind a mass-weighted
 * solve the Cartesian response.  A row without weight is not read and contributes nothing, a listed row outside
 * 0..nvec-1 turns the structure's result into NaN, and so do NaN eigenvalues (a failed structure).  Both passes read the
 * listed rows once per group of four forces.  No atomics: the first pass adds a row's atoms in a fixed order given by (m,
 * dim), the second the rows in ascending order within chunks cut by the number of listed rows alone, then the chunks in
 * ascending order: X[b, j] does not depend, bit for bit, on the batch size, the structure's position, its neighbours, q
 * or the forces beside f_j.  The partial sums of a slab of structures take at most SPRINGCRAFT_MODES_BUDGET_BYTES (else 1
 * GiB).  q = 0 does nothing.  Enqueue only. */
int sc_dev_mode_response_f64(sc_ctx* ctx, const double* d_w, const double* d_v, int64_t m, int64_t nvec, int64_t batch,
                             int dim, const sc_mode_selection* sel, const int64_t* d_counts, const double* d_force,
                             int64_t q, const double* d_atom_scale, double* d_out);
/* The second pass on coefficients the caller chose -- displacements along modes, samples, and the inverse of
 * sc_dev_modes_overlap_f64's result; no reference counterpart (ProDy: deformAtoms / traverseMode / sampleModes):
 *   X[b, j, dim a + d] = t_a sum_r d_coef[b, j, r] V[b, r, dim a + d]
 * over EVERY row r below the structure's row limit, min(d_counts[b], nvec) or nvec without counts, trivial rows included:
 * what is not wanted gets the coefficient 0.  d_coef (batch, q, nvec), d_out (batch, q, m).  Rows at or behind the limit
 * are never read, and neither are their coefficients, whatever they hold.  d_w is not read: a structure whose solve
 * failed is the caller's to mask, as for the overlaps.  Order of the sums and bit-for-bit independence as above.  Enqueue
 * only. */
int sc_dev_mode_combine_f64(sc_ctx* ctx, const double* d_v, int64_t m, int64_t nvec, int64_t batch, int dim,
                            const double* d_coef, int64_t q, const int64_t* d_counts, const double* d_atom_scale,
                            double* d_out);
/* Bytes of device workspace the entries above hold for such a call (allocated lazily, cached, grown on demand --
 * the one step of a first call that waits for the stream).  n_sel: rows that carry a weight (nvec - row0, n_rows, or
 * nvec for SC_SEL_PINV); what: 0 = msf, 1 = dcc, 2 = anisotropic tensors (dim 3 and m % 3 == 0, else 0), 3 = overlaps /
 * collectivities (always 0: sc_dev_modes_overlap_f64 holds no workspace), 4 = distance fluctuations (the weights only; dim
 * 3 and m % 3 == 0, else 0), 5 = response (weights, the coefficients of four forces and the partial sums of a slab), 6 =
 * combine (the partial sums of a slab), 7 = perturbation-response scanning (the weights and one diagonal per structure
 * of a slab of at most 32768; dim 3 and m % 3 == 0, else 0), 8 = generalized correlation (the weights, the tensors'
 * partial sums of a slab in chunks of 128 rows, and six plus nine doubles per atom of the batch: tensors and whitening
 * factors; dim 3 and m % 3 == 0, else 0); budget_bytes as above. */
int64_t sc_dev_modes_workspace_bytes(int64_t m, int64_t nvec, int64_t batch, int dim, int64_t n_sel, int what,
                                     int64_t budget_bytes);

/* ---- partial spectrum and mode consumers of a ragged batch (sc_batch_plan) ---------------------------------------------
 * The reference models one arbitrary structure per object (anm.py:62-63); a plan solves many in padded slots
 * diag(M, D) whose pad eigenvalues lie above M's spectrum (see sc_batch_plan_create), so a slot's lowest eigenpairs are
 * the structure's own.  The plan keeps one small device record per structure (own order dim * n_atoms, atom offset,
 * square offset) that the entries below read; nothing is uploaded per call, all of them only enqueue.
 *
 * Eigenpairs il..iu of every slot, as sc_dev_eigh_range_f64 on (count, order, order): d_w (count, m), d_v NULL or
 * (count, m, order), m = iu - il + 1.  0 <= il <= iu < dim * min(n_atoms), so that every row is a structure's mode and
 * never a pad (SC_ERR_INDEX otherwise).  d_a is destroyed. */
int sc_batch_plan_eigh_range_f64(sc_batch_plan* plan, double* d_a, int64_t il, int64_t iu, double* d_w, double* d_v);
/* Eigenvalue window (vl, vu] of every slot, as sc_dev_eigh_window_f64 with 1 <= capacity <= dim * min(n_atoms), except
 * that only a structure's own dim * n_atoms eigenvalues count: d_count[b] = min(count, dim n_b - il_b) -- the pads are
 * never counted, also for vu = +inf -- and the K = capacity solved rows of slot b start at min(il_b, dim n_b - K). */
int sc_batch_plan_eigh_window_f64(sc_batch_plan* plan, double* d_a, double vl, double vu, int64_t capacity, double* d_w,
                                  double* d_v, int64_t* d_count);
/* The batch consumers above (nma.py:108-184 mean_square_fluctuation, nma.py:233-359 dcc) on a plan's slots: d_w (count,
 * nvec), d_v (count, nvec, order), sel and d_counts as for sc_dev_modes_*.  sel->reserved holds first_row, the global
 * mode index of row 0 (il of an index-range solve, otherwise 0): rows r >= dim n_b - first_row of structure b are pads and
 * never carry a weight, whatever the selection names; SC_SEL_PINV takes its maximum over the structure's own eigenvalues
 * only (the pads are the largest of the slot).  Pad columns are neither read into a sum nor packed.
 * msf: d_out (sum n_atoms,) packed, structure b at its atom offset.  A structure's bits depend on the slot order and the
 * selection, not on its neighbours or its position. */
int sc_batch_plan_modes_msf_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                                const sc_mode_selection* sel, const int64_t* d_counts, double* d_out);
/* dcc: d_out (sum n_atoms^2,) packed, structure b's (n_b, n_b) block at the sum of the squares before it.  One grouped
 * GEMM record per structure with M = N = ldc = n_b; slabs, row chunks and the block tile as for sc_dev_modes_dcc_f64,
 * functions of (order, rows, dim, budget) only. */
int sc_batch_plan_modes_dcc_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                                const sc_mode_selection* sel, const int64_t* d_counts, int norm, int64_t budget_bytes,
                                double* d_out);
/* anisotropic tensors (a plan of dim 1: SC_ERR_INVALID_ARG): d_out (sum n_atoms, 6) packed, structure b's six values per
 * atom (xx yy zz xy xz yz, as sc_dev_modes_aniso_f64) at 6 times its atom offset.  A structure's bits depend on the slot
 * order and the selection, not on its neighbours or its position. */
int sc_batch_plan_modes_aniso_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                                  const sc_mode_selection* sel, const int64_t* d_counts, double* d_out);
/* sc_dev_modes_overlap_f64 for the plan's padded slots: d_v (count, nvec, order); first_row: global mode index of row 0
 * of d_v (lo of an index-range solve, else 0).  d_disp (q, dim * sum n_atoms) packed as the coordinates of
 * sc_batch_plan_assemble_f64 are: structure b's vector j starts at j * dim * sum n + dim * atom_off_b.  d_overlap (count,
 * q, nvec), d_collectivity (count, nvec).  Only a structure's own columns are read and N is its own atom count; a slot's
 * pad rows (r >= own_b - first_row) and the rows behind d_counts[b] are NaN and are not read.  A structure's bits depend
 * on the selection and its own size, not on its neighbours or its position. */
int sc_batch_plan_modes_overlap_f64(sc_batch_plan* plan, const double* d_v, int64_t nvec, int64_t first_row,
                                    const double* d_disp, int64_t q, const int64_t* d_counts, double* d_overlap,
                                    double* d_collectivity);
/* distance fluctuations (a plan of dim 1: SC_ERR_INVALID_ARG), as sc_dev_modes_distfluct_f64 -- no reference counterpart
 * (ProDy: calcDistFlucts / calcMechStiff): d_coord (sum n_atoms, 3) and d_atom_scale (sum n_atoms,) or NULL packed as
 * sc_batch_plan_assemble_f64 takes its coordinates and weights, N the structure's own n_atoms, d_out (sum n_atoms^2,)
 * packed like the dcc.  Pad rows never carry a weight, pad columns are never read.  A structure's bits depend on its own
 * size and the selection, not on its neighbours or its position. */
int sc_batch_plan_modes_distfluct_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                                      const sc_mode_selection* sel, const int64_t* d_counts, const double* d_coord,
                                      const double* d_atom_scale, double* d_out);
/* perturbation-response scanning (a plan of dim 1: SC_ERR_INVALID_ARG), as sc_dev_prs_f64: d_atom_scale (sum n_atoms,)
 * packed or NULL, N the structure's own n_atoms, d_out (sum n_atoms^2,) packed like the dcc.  Pad rows never carry a
 * weight, pad columns are never read.  A structure's bits depend on its own size and the selection, not on its
 * neighbours or its position. */
int sc_batch_plan_prs_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                          const sc_mode_selection* sel, const int64_t* d_counts, const double* d_atom_scale, int norm,
                          double* d_out);
/* generalized correlation (a plan of dim 1: SC_ERR_INVALID_ARG), as sc_dev_lmi_f64: N the structure's own n_atoms, d_out
 * (sum n_atoms^2,) packed like the dcc.  Pad rows never carry a weight, pad columns are never read.  A structure's bits
 * depend on its own size and the selection, not on its neighbours, its position or the slot order (the tensors' chunks
 * are cut at fixed rows, where sc_batch_plan_modes_aniso_f64 cuts them by the slot's row count): they are those of its
 * uniform solve by sc_dev_lmi_f64. */
int sc_batch_plan_lmi_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                          const sc_mode_selection* sel, const int64_t* d_counts, int information, double* d_out);
/* sc_dev_mode_response_f64 for the plan's padded slots (GNM and ANM plans; sel->reserved holds first_row as for the
 * sc_batch_plan_modes_* entries above): d_force and d_out (q, dim * sum n_atoms)
 * packed as sc_batch_plan_modes_overlap_f64's displacement is, structure b's vector j at j * dim * sum n + dim *
 * atom_off_b; d_atom_scale (sum n_atoms,) packed or NULL.  Only a structure's own columns are read and written; pad rows
 * never carry a weight and are not read.  A structure's bits depend on the slot order, its own size and the selection,
 * not on its neighbours or its position. */
int sc_batch_plan_mode_response_f64(sc_batch_plan* plan, const double* d_w, const double* d_v, int64_t nvec,
                                    const sc_mode_selection* sel, const int64_t* d_counts, const double* d_force,
                                    int64_t q, const double* d_atom_scale, double* d_out);
/* sc_dev_mode_combine_f64 for the plan's padded slots: d_coef (count, q, nvec); first_row as for
 * sc_batch_plan_modes_overlap_f64.  Structure b's row limit is min(d_counts[b], nvec, own_b - first_row): pad rows and
 * their coefficients are never read, pad columns neither read nor written.  d_out and d_atom_scale packed as above. */
int sc_batch_plan_mode_combine_f64(sc_batch_plan* plan, const double* d_v, int64_t nvec, int64_t first_row,
                                   const double* d_coef, int64_t q, const int64_t* d_counts, const double* d_atom_scale,
                                   double* d_out);
/* What sc_dev_modes_workspace_bytes answers for a uniform batch, for the plan's (count, order). */
int64_t sc_batch_plan_modes_workspace_bytes(const sc_batch_plan* plan, int64_t nvec, int64_t n_sel, int what,
                                            int64_t budget_bytes);

/* ---- rotation-translation blocks (RTB): the lowest modes of a network without its (3N, 3N) Hessian -------------------
 * No reference counterpart (Durand / Tama / Sanejouand; ProDy: RTB, Bio3D: rtb).  Atoms are grouped into rigid blocks;
 * block b has dof_b <= 6 orthonormal rigid-body fields, the columns offset[b] .. offset[b + 1] - 1 of the (3N, nr)
 * projector, nr = offset[n_blocks].  The projector is passed as d_P (N, 3, 6) row-major -- atom a's three rows of its
 * block's columns, unused columns 0.0 -- with d_block_of_atom (N) int32 and d_offset (n_blocks + 1) int64.  Device
 * pointers, enqueue only.
 *
 * sc_dev_rtb_hessian_f64: d_hb (nr, nr) row-major = P^T H P for the H that sc_hessian_from_pairs_f64 builds from the
 * ordered directed pair list d_pairs (k, 2) and d_gamma (k), times outer(s, s) with s = d_inv_sqrt_mass (N) repeated per
 * coordinate (NULL: 1): with d = r_j - r_i, g = gamma_p / |d|^2 and t_a = s_a P[a]^T d, pair p = (i, j) adds -g t_i t_j^T
 * to the block (block(i), block(j)) and +g t_j t_j^T to the diagonal block of block(j) -- off-diagonal from gamma(i, j),
 * diagonal summed over the first index, as that entry does for asymmetric constants.  The caller supplies the order of
 * the sums: d_order (k) lists the pairs sorted by (block(j), block(i)), stable; d_seg_start (n_seg + 1) the starts of
 * the n_seg runs of equal (block(j), block(i)) in that order, d_seg_start[n_seg] = k; d_block_start (n_blocks + 1) where
 * the pairs with block(j) = b start, d_block_start[n_blocks] = k (a block no pair ends in has an empty range).  One
 * wavefront sums a run in a fixed order and stores its 6 x 6 block once: no atomics, the bits of d_hb depend on the inputs
 * alone.  Every entry of d_hb is written, zero where no contact; blocks need not be contiguous in atom order nor fit a
 * workgroup, atoms need not have contacts.  k = 0 gives the zero matrix (the pair arrays may then be NULL).  No buffer
 * beyond the arguments.  SC_ERR_INVALID_ARG: a non-positive n_atoms / n_blocks / nr, a negative k, a NULL required
 * pointer, n_blocks > n_atoms, nr > 6 n_blocks or n_seg > k.  Entries of the index arrays outside their ranges are
 * skipped, not reported. */
int sc_dev_rtb_hessian_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, const int64_t* d_pairs, int64_t k,
                           const double* d_gamma, const double* d_inv_sqrt_mass, const double* d_P,
                           const int32_t* d_block_of_atom, const int64_t* d_offset, int64_t n_blocks, int64_t nr,
                           const int64_t* d_order, const int64_t* d_seg_start, int64_t n_seg,
                           const int64_t* d_block_start, double* d_hb);
/* d_v (nvec, 3 n_atoms) = d_u (nvec, nr) P^T: V[r, 3 a + al] = sum_c P[a, al, c] U[r, offset[block(a)] + c], one
 * streaming pass, every entry written, no mass factor (the modes stay in the coordinates of the Hessian).  nvec at most
 * 524280.  SC_ERR_INVALID_ARG for non-positive sizes or a NULL pointer. */
int sc_dev_rtb_expand_f64(sc_ctx* ctx, const double* d_u, int64_t nvec, int64_t nr, const double* d_P,
                          const int32_t* d_block_of_atom, const int64_t* d_offset, int64_t n_atoms, double* d_v);

/* ---- the network as an operator: Hessian products, deformation energies and spring strain from the pair list ---------
 * No reference counterpart (Hinsen's deformation energy; Bio3D: deformation.nma).  The network is the ordered directed
 * pair list d_pairs (k, 2) int64 -- sorted by first then second atom, both directions, as the pair-list entry returns
 * it -- with d_gamma (k), d_coord (N, 3) (NULL for dim 1) and d_atom_scale (N) = 1 / sqrt(mass) or NULL for 1.  With
 * d = r_j - r_i, n = d / |d| and, for a row x of length dim N, u[a] = scale_a x[dim a .. dim a + dim - 1], pair p = (i, j)
 * has the elongation e_p = n . (u[i] - u[j]) (dim 1: u[i] - u[j]).  gamma must be symmetric, gamma(i, j) = gamma(j, i):
 * then the sums below belong to the matrix sc_hessian_from_pairs_f64 / sc_kirchhoff_from_pairs_f64 build, times
 * outer(s, s) with s the scale repeated per coordinate; the entries do not check it.  Device pointers, enqueue only on the
 * context's stream, no atomics, no buffer beyond the arguments.
 *
 * sc_dev_pairs_apply_f64: for each of the q rows of d_x (q, dim N)
 *     d_y (q, dim N)   Y[i] = scale_i sum_{p = (i, .)} gamma_p e_p n_p   (dim 1: without n_p), the product (T H T) x
 *     d_energy (q, N)  E[i] = 1/2 sum_{p = (i, .)} gamma_p e_p^2, whose sum over the atoms is x^T (T H T) x
 * either may be NULL, not both.  d_row_start (N + 1) int64: atom i's pairs are the rows row_start[i] ..
 * row_start[i + 1] - 1 of the list.  Every entry of the outputs is written; an atom without pairs gets exactly 0.0.  One
 * wavefront sums an atom's pairs in an order its own pair range fixes: a row's bits depend neither on q nor on the row's
 * position nor on the other rows (a NaN row gives NaN for that row only), and two calls agree bit for bit.  Two atoms of
 * a pair at one position give NaN, as the Hessian entry does.  q = 0 is valid, and so is k = 0 (zeros; the pair arrays
 * and d_row_start may then be NULL).  SC_ERR_INVALID_ARG before anything is launched: both outputs NULL, dim not 1 or 3,
 * dim 3 without d_coord, a non-positive n_atoms, a negative k or q, a NULL required pointer.  Rows of the list whose first
 * atom is not i or whose second lies outside 0 .. N - 1 are skipped, not reported. */
int sc_dev_pairs_apply_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs,
                           int64_t k, const double* d_gamma, const int64_t* d_row_start, const double* d_atom_scale,
                           const double* d_x, int64_t q, double* d_y, double* d_energy);
/* d_out (q, ks): the strain S = gamma_p e_p^2 of the pairs p = d_pair_idx[s] (ks) int64 for every row of d_x, the energy
 * mode x stores in that spring twice over (both directions of a spring carry it; the sum over all directed rows is
 * 2 x^T (T H T) x) and, for an eigenvector, the derivative of its eigenvalue by ln gamma of the directed row.  One thread
 * per (pair, row) term.  An index outside 0 .. k - 1 gives NaN in its column and is not read; a listed pair with an atom
 * outside 0 .. N - 1 gives 0.0.  q = 0 and ks = 0 are valid.  SC_ERR_INVALID_ARG as above, and for a negative ks. */
int sc_dev_pairs_strain_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs,
                            int64_t k, const double* d_gamma, const double* d_atom_scale, const int64_t* d_pair_idx,
                            int64_t ks, const double* d_x, int64_t q, double* d_out);
/* One fused step of a polynomial in T H T on a column panel: Z <- alpha (T H T) X + beta X + gamma_c Z, the three-term
 * recurrence of a Chebyshev filter in one pass.  T H T is exactly the matrix of sc_dev_pairs_apply_f64, from the same pair
 * list, d_row_start, d_gamma, d_coord and d_atom_scale.  A panel has m = dim N rows and q columns with the leading
 * dimension ld >= q: element (row dim a + c, column r) of d_x / d_z lies at [(dim a + c) ld + r]; the columns are the
 * vectors (the transpose of the rows sc_dev_pairs_apply_f64 takes).  d_z must not be d_x (nor overlap it; two panels may
 * interleave in one buffer of a larger ld).  d_z is read only when gamma_c != 0: with gamma_c = 0 it is overwritten and a
 * NaN in it does not propagate.  Columns q .. ld - 1 of d_z are never written and those of d_x never read.  One wavefront
 * owns an atom and 64 columns and adds the atom's pairs in list order, lane = column: a column's bits depend neither on
 * q nor on ld nor on the column's position nor on the other columns (a NaN column gives NaN in that column only), and two
 * calls agree bit for bit; the sum order differs from sc_dev_pairs_apply_f64, whose result it matches to rounding only.
 * An atom without pairs gets beta X + gamma_c Z with the H term exactly 0.0.  q = 0 is valid (nothing is launched), and so
 * is k = 0 (Z <- beta X + gamma_c Z; the pair arrays and d_row_start may then be NULL).  SC_ERR_INVALID_ARG before anything
 * is launched: ld < q, d_z == d_x, dim not 1 or 3, dim 3 without d_coord, a non-positive n_atoms, a negative k, q or ld,
 * q above 4194240 (65535 chunks of 64 columns), a NULL required pointer.  Rows of the list whose first atom is not i or
 * whose second lies outside 0 .. N - 1 are skipped, not reported. */
int sc_dev_pairs_panel_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs,
                           int64_t k, const double* d_gamma, const int64_t* d_row_start, const double* d_atom_scale,
                           const double* d_x, double* d_z, int64_t ld, int64_t q, double alpha, double beta,
                           double gamma_c);

/* ---- conjugate gradients on the pair list: (T H T)^+ f for q right-hand sides at once -------------------------------------
 * The matrix is the one of sc_dev_pairs_panel_f64, from the same network arguments.  Panels d_x, d_r, d_p, d_q are (dim N,
 * q) with leading dimension ld >= q, columns are the vectors.  d_state holds seven rows of ld 8-byte words, row r of column
 * c at [r ld + c]: 0 rho = <r, r>, 1 stop = (tol |f|)^2, 2 alpha, 3 beta as doubles; 4 status (0 running, 1 converged, 2
 * broken down: <p, (T H T) p> was not a finite positive number) and 5 iters as int64; 6 pq = <p, (T H T) p> of the column's
 * last iteration as a double.  d_work is a workspace of the size
 * sc_dev_pairs_cg_workspace returns, one partial sum per (four atoms, column).  Device pointers, enqueue only on the
 * context's stream: no atomics, no host synchronisation inside or between iterations.  Columns q .. ld - 1 of the panels and
 * of the state are never written.  A column's bits in d_x, d_r, d_p, rho and iters depend on its own right-hand side and the
 * network only: not on q, ld, the column's position, the other columns, or the iterations enqueued after it stopped; a column
 * with status != 0 is frozen (its column of d_q is still overwritten).  The right-hand sides must lie in the range of the
 * matrix (the caller projects the null space out).
 *
 * sc_dev_pairs_cg_workspace: No reference counterpart.  *bytes = 8 q ceil(n_atoms / 4).  SC_ERR_INVALID_ARG for a NULL
 * bytes, a non-positive n_atoms, a negative q or sizes above the limits of the step. */
int sc_dev_pairs_cg_workspace(int64_t n_atoms, int64_t q, size_t* bytes);
/* No reference counterpart.  Starts a solve from the projected right-hand sides in d_r: X = 0, P = R, rho = <r, r>, stop =
 * tol^2 rho, alpha = beta = 0, iters = 0, status 0 -- or 1 at once for |f| = 0 (x = 0 is the solution), 2 for a non-finite
 * |f|.  The sum <r, r> runs in an order that depends on n_atoms alone.  q = 0 is valid.  SC_ERR_INVALID_ARG before anything
 * is launched: dim not 1 or 3, a non-positive n_atoms, a negative q, ld < q, q above 4194240, tol not positive, a NULL
 * pointer, two panels at one address, a workspace that is too small. */
int sc_dev_pairs_cg_init_f64(sc_ctx* ctx, int64_t n_atoms, int dim, double* d_x, const double* d_r, double* d_p, int64_t ld,
                             int64_t q, double tol, double* d_state, void* d_work, size_t work_bytes);
/* No reference counterpart.  Enqueues `iterations` CG iterations on the state sc_dev_pairs_cg_init_f64 left: per column
 *     Q = (T H T) P (the bits of sc_dev_pairs_panel_f64 with alpha 1, beta 0, gamma_c 0), alpha = rho / <p, q>,
 *     X += alpha P, R -= alpha Q, rho_new = <r, r>, beta = rho_new / rho, rho = rho_new, iters += 1,
 *     status 1 when rho_new <= stop, P = R + beta P for the columns still running.
 * An atom without pairs contributes exactly 0.0 to Q and to the sums.  iterations = 0 and q = 0 are valid.
 * SC_ERR_INVALID_ARG before anything is launched: what sc_dev_pairs_panel_f64 refuses of the network and of ld and q, a
 * negative number of iterations, a NULL panel, state or workspace, two panels at one address, a workspace that is too small. */
int sc_dev_pairs_cg_step_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs,
                             int64_t k, const double* d_gamma, const int64_t* d_row_start, const double* d_atom_scale,
                             double* d_x, double* d_r, double* d_p, double* d_q, int64_t ld, int64_t q, double* d_state,
                             void* d_work, size_t work_bytes, int64_t iterations);

/* ---- conformational ensembles: superposition, mean frame and principal components on the device ------------------------
 * No reference counterpart (its callers superimpose with biotite; Bio3D: fit.xyz / pca.xyz, ProDy: superpose / iterpose /
 * PCA).  An ensemble is d_frames (M, N, 3), contiguous float64 in device memory: M frames of the same N atoms.  Device
 * pointers, enqueue only on the context's stream, no atomics, every sum in a fixed order: two calls agree bit for bit.
 * Conditions the device finds (a non-finite matrix in the eigensolve) surface at the next sc_ctx_synchronize.
 *
 * sc_superpose_form: which kernel form sc_dev_superpose_f64 takes for frames of n_atoms atoms: 0, one workgroup keeps the
 * frame in LDS (one read and one write of the frame; up to 2560 atoms), or 1, the streaming form (three reads, one write).
 * SPRINGCRAFT_SUPERPOSE_FORM = stream forces 1; = lds and = auto leave the size rule.  Read at every call. */
int sc_superpose_form(int64_t n_atoms);
/* Least-squares superposition of every frame on d_target (N, 3) with the atom weights d_weights (N), non-negative with a
 * positive sum, or NULL for 1: the proper rotation R (det = +1, Horn's quaternion method; a mirror image gets the best
 * rotation, never a reflection; a degenerate frame -- one or two atoms, collinear, planar -- gets one of its minimisers) and
 * the translation t that minimise sum_a w_a |R x_a + t - target_a|^2.
 *     d_out   (M, N, 3)  R x + t, zero-weight atoms included; may be d_frames (in place)
 *     d_rot   (M, 3, 3)  row-major R, or NULL
 *     d_trans (M, 3)     t, or NULL
 *     d_rmsd  (M)        sqrt(sum_a w_a |d_out_a - target_a|^2 / sum w), summed from the residuals, or NULL
 * A frame's bits depend on that frame, the target and the weights alone: not on M, the frame's position or its neighbours.
 * A non-finite coordinate makes that frame's outputs NaN and no other frame's.  Weights that sum to 0 give NaN.
 * SC_ERR_INVALID_ARG: non-positive sizes, more than 2^31 - 1 frames or coordinates per frame, a NULL required pointer. */
int sc_dev_superpose_f64(sc_ctx* ctx, const double* d_frames, int64_t n_frames, int64_t n_atoms, const double* d_target,
                         const double* d_weights, double* d_out, double* d_rot, double* d_trans, double* d_rmsd);
/* d_mean (N, 3) = sum_f p_f x_f / sum p and, unless NULL, d_msd (N) = sum_f p_f |x_f[a] - mean[a]|^2 / sum p, the
 * per-atom mean-square deviation from the mean frame, with the frame weights d_frame_weights (M) or NULL for 1.  Two-level
 * sums: chunks of 64 consecutive frames, then the chunks.  At most 4194240 frames.  SC_ERR_INVALID_ARG as above. */
int sc_dev_ensemble_mean_f64(sc_ctx* ctx, const double* d_frames, int64_t n_frames, int64_t n_atoms,
                             const double* d_frame_weights, double* d_mean, double* d_msd);
/* The n_modes largest principal components of the (fitted) frames about d_mean (N, 3): with Xc (M, 3 N) the frames minus
 * the mean, atom a's columns times d_sqrt_mass[a] (N; NULL: 1), the eigenpairs of the covariance Xc^T Xc / (M - 1) -- from
 * the Gram matrix Xc Xc^T / (M - 1) of order M while M - 1 < 3 N, else from the covariance of order 3 N.
 *     d_var   (n_modes)        the variances, descending
 *     d_w     (n_modes)        1 / variance, ascending: the eigenvalues of the quasi-harmonic Hessian in units of kT
 *     d_v     (n_modes, 3 N)   the components, unit rows in the order of d_var (their signs are not fixed)
 *     d_total (1)              the trace of the covariance, sum Xc^2 / (M - 1)
 * A rank-deficient ensemble gives variances at rounding level (also negative ones) and rows without meaning: the caller
 * compares d_var with its largest entry.  1 <= n_modes <= min(M - 1, 3 N), n_modes <= 65535, the order of the eigenproblem
 * at most 46000.  SC_ERR_INVALID_ARG otherwise, and for what sc_dev_superpose_f64 refuses. */
int sc_dev_ensemble_pca_f64(sc_ctx* ctx, const double* d_frames, int64_t n_frames, int64_t n_atoms, const double* d_mean,
                            const double* d_sqrt_mass, int64_t n_modes, double* d_w, double* d_var, double* d_v,
                            double* d_total);
/* The pairwise least-squares RMSD of conformations.  No reference counterpart (Bio3D: rmsd(xyz, fit = TRUE); ProDy, MDTraj
 * and MDAnalysis have their own pairwise RMSD matrices).  d_out (n_a, n_b): every frame of d_a (n_a, N, 3) with every frame
 * of d_b (n_b, N, 3); d_b NULL: d_a with itself, n_b = n_a.  With W = sum w, c_f = sum w x_f / W, y_f = x_f - c_f, G_f =
 * sum_a w_a |y_f[a]|^2 and S = sum_a w_a y_f[a] y_g[a]^T:
 *     msd(f, g) = max(0, (G_f + G_g) - 2 lambda) / W,   lambda the largest eigenvalue of Horn's 4 x 4 matrix of S
 * (the proper rotation's, also for a mirror image), from one Gram product over the atoms on the matrix pipe: no rotation is
 * formed, no frame written.  flags bit 0: fit (unset: the frames as they are, lambda = tr S about the weighted centroid of
 * d_a's first frame -- 0 where that is not finite); bit 1: squared, d_out = msd, else rmsd = sqrt(msd).
 * A self-comparison equals its transpose bit for bit and its diagonal is exactly 0.0.  A non-finite coordinate turns that
 * frame's row and column into NaN (the diagonal entry included) and no other entry.  An entry's bits depend on its two
 * frames, the weights and the flags alone: not on n_a, n_b, the frames' positions or their neighbours.  Enqueue only.
 * SC_ERR_INVALID_ARG: non-positive sizes, d_b NULL with n_b != n_a, unknown flag bits, a NULL d_a or d_out, sizes for which
 * sc_rmsd_matrix_workspace answers -1.
 *
 * sc_rmsd_matrix_workspace: bytes of context scratch a call occupies, n_b = 0 for a self-comparison: per ensemble a
 * transposed centred copy (8 ceil(N / 8), 3, 64 ceil(M / 64)) and 64 ceil(M / 64) sums, each region rounded up to 256
 * bytes, and one double more.  -1 for non-positive n_a or n_atoms, a negative n_b, or sizes beyond the index range. */
int64_t sc_rmsd_matrix_workspace(int64_t n_a, int64_t n_b, int64_t n_atoms);
int sc_dev_rmsd_matrix_f64(sc_ctx* ctx, const double* d_a, int64_t n_a, const double* d_b, int64_t n_b, int64_t n_atoms,
                           const double* d_weights, int flags, double* d_out);
/* The neighbour bits of the frames of one ensemble without the matrix: what neighbour-count clustering needs of the (n, n)
 * RMSD matrix is `value <= cutoff`, 1 bit per ordered pair instead of 8 bytes, and the product kernel of the matrix writes
 * those bits from its registers.  words = ceil(n / 64); flags as above; cutoff in the value's units (squared with bit 1).
 * d_adj (n, words) uint64: bit g & 63 of word g >> 6 of row f is set when both frames are finite and the value the matrix
 * entry would write for (f, g) is <= cutoff, or f = g: the same double, compared.  A non-finite frame's row and column are
 * zero, the bits of the columns >= n of the last word are zero, d_adj equals its transpose bit for bit, and every word is
 * written exactly once: no memset, no atomics, two calls agree bit for bit.  d_count (n) int32: the rows' popcounts, a
 * frame's number of neighbours, itself included.  d_valid (words) uint64: the finite frames.
 *
 * sc_dev_frame_neighbours_init_f64 writes them into d_ws, a neighbour-count workspace of ws_bytes >=
 * sc_cluster_workspace(n, 0) bytes, with the alive set, d_labels (n, all -1) and d_status (valid frames, 0, 0, 0): the state
 * sc_dev_cluster_gromos_init_f64 leaves from the stored matrix, so sc_dev_cluster_gromos_rounds runs on it unchanged.
 * status[2] stays 0: a NaN pair exists only where a frame is not finite.
 *
 * Both occupy sc_rmsd_matrix_workspace(n, 0, n_atoms) bytes of context scratch and only enqueue.  SC_ERR_INVALID_ARG
 * before anything is launched: non-positive sizes, unknown flag bits, more frames than clustering takes (262144), sizes for
 * which sc_rmsd_matrix_workspace answers -1, a cutoff that is negative or not finite, a NULL pointer, a workspace that is
 * too small. */
int sc_dev_frame_neighbours_f64(sc_ctx* ctx, const double* d_frames, int64_t n_frames, int64_t n_atoms,
                                const double* d_weights, int flags, double cutoff, uint64_t* d_adj, int32_t* d_count,
                                uint64_t* d_valid);
int sc_dev_frame_neighbours_init_f64(sc_ctx* ctx, const double* d_frames, int64_t n_frames, int64_t n_atoms,
                                     const double* d_weights, int flags, double cutoff, void* d_ws, size_t ws_bytes,
                                     int32_t* d_labels, int32_t* d_status);

/* ---- dense Cholesky solver on the device (csrc/potrf.hip) ----------------------------------------------------------------
 * No reference counterpart (LAPACK: dpotrf / dpotrs).  `batch` symmetric positive definite matrices of one order n, float64,
 * LOWER triangle, column-major, leading dimension ld >= n, matrix b at d_a + b * stride.  The strict upper triangle is never
 * written and no result depends on it.  All entries only enqueue on the context's stream; there are no atomics, and the bits
 * of one matrix' results do not depend on the batch or the matrix' place in it.
 *
 * sc_dev_potrf_workspace: *bytes = the context scratch a factorisation (or a one-vector solve) of this shape occupies; the
 * context allocates it itself at the first call.  SC_ERR_INVALID_ARG for a NULL pointer or sizes the entries below refuse.
 *
 * sc_dev_potrf_f64: d_a <- L with A = L L^T, in place.  d_info (batch) int64: 0, or 1 + the first column whose pivot was <= 0
 * or NaN (LAPACK's info).  The whole lower triangle of such a matrix becomes NaN, as does everything solved with it; the
 * other matrices are not affected, and the next synchronising call of the context returns SC_ERR_NOCONV once (LinAlgError in
 * the Python layer), as for a failed eigensolve.  SC_ERR_INVALID_ARG before anything is launched: n <= 0, batch <= 0 or
 * above 65535, ld < n, a stride below a matrix' extent with batch > 1, a NULL pointer.
 *
 * sc_dev_potrs_f64: triangular solves with the factor d_l on the right-hand sides d_b, (n, q) column-major with leading
 * dimension ldb >= n, matrix b's at d_b + b * strideb, in place.  mode 0: L Y = B (forward); 1: L^T X = B (backward); 2: both,
 * A X = B.  q = 0 is valid.  SC_ERR_INVALID_ARG as above, and for another mode, q < 0, ldb < n. */
int sc_dev_potrf_workspace(int64_t n, int64_t batch, size_t* bytes);
int sc_dev_potrf_f64(sc_ctx* ctx, double* d_a, int64_t n, int64_t ld, int64_t stride, int64_t batch, int64_t* d_info);
int sc_dev_potrs_f64(sc_ctx* ctx, const double* d_l, int64_t n, int64_t ld, int64_t stride, int64_t batch, double* d_b,
                     int64_t q, int64_t ldb, int64_t strideb, int mode);

/* ---- vibrational subsystem analysis (csrc/subsystem.hip) -------------------------------------------------------------------
 * No reference counterpart (Hinsen 2000; Zheng & Brooks 2005; ProDy: reduceModel).  The N atoms are split into n_s system and
 * n_e environment atoms: d_group (N) int32 0 / 1, d_pos (N) int32 the atom's place in its group.  ms = dim n_s, me = dim n_e.
 *
 * sc_dev_subsystem_blocks_f64: d_hss (ms, ms), d_hes (me, ms) row-major and d_hee (me, me), the blocks of the matrix that
 * sc_hessian_from_pairs_f64 (dim 3) / sc_kirchhoff_from_pairs_f64 (dim 1) builds from the same ordered pair list with
 * symmetric constants; d_row_start (N + 1): atom i owns the rows row_start[i] .. row_start[i + 1] - 1 of the list.
 * d_inv_sqrt_mass (n_s) or NULL scales the rows and columns of H_ss and the columns of H_es; the environment is massless.
 * Every entry is written; no atomics, two calls agree bit for bit, H_ss and H_ee equal their transposes bit for bit.
 *
 * sc_dev_subsystem_reduce_f64: d_hee <- its Cholesky factor L (lower, column-major; d_info (1) as for sc_dev_potrf_f64),
 * d_hes <- Y = L^-1 H_es, d_hss <- H_eff = H_ss - Y^T Y, equal to its transpose bit for bit.
 *
 * sc_dev_subsystem_follow_f64: d_xe (q, me) <- -L^-T (Y x_s) for the q rows d_xs (q, ms), the environment's motion that
 * follows the system's, with d_l and d_y as the reduction left them.
 *
 * The first two are the batched entries below for one member whose slot is exactly its environment (batch = 1, env_order =
 * n_e): the same kernels and launches, so the same bits.
 *
 * All three only enqueue.  SC_ERR_INVALID_ARG before anything is launched: dim not 1 or 3, n_s or n_e not positive or not
 * summing to n_atoms, a negative k, q < 1, a NULL required pointer. */
int sc_dev_subsystem_blocks_f64(sc_ctx* ctx, const double* d_coord, int64_t n_atoms, int dim, const int64_t* d_pairs,
                                int64_t k, const double* d_gamma, const int64_t* d_row_start, const int32_t* d_group,
                                const int32_t* d_pos, int64_t n_s, int64_t n_e, const double* d_inv_sqrt_mass, double* d_hss,
                                double* d_hes, double* d_hee);
int sc_dev_subsystem_reduce_f64(sc_ctx* ctx, double* d_hss, double* d_hes, double* d_hee, int64_t ms, int64_t me,
                                int64_t* d_info);
int sc_dev_subsystem_follow_f64(sc_ctx* ctx, const double* d_l, const double* d_y, int64_t ms, int64_t me, const double* d_xs,
                                int64_t q, double* d_xe);

/* ---- batched subsystem reduction on a common core (csrc/subsystem.hip) ---------------------------------------------------------
 * No reference counterpart (Bio3D: nma.pdbs with rm.gaps = TRUE; ProDy: reduceModel over an ensemble).  `batch` members keep
 * all their atoms; every member has the same n_s system atoms (the aligned core) and its own n_e(b) <= env_order environment
 * atoms.  ms = dim n_s; me = dim env_order is the order of every environment slot.
 *
 * The members' inputs are packed back to back: d_coord (sum n_b, 3), d_pairs (sum k_b, 2) with LOCAL atom indices, d_gamma
 * (sum k_b), d_group / d_pos (sum n_b) and d_row_start, n_b + 1 entries per member counting from the member's own first pair.
 * `members` is a HOST array (batch, 5) int64: atom offset, atom count, pair offset, pair count, n_e; the offsets must follow
 * the member before.  Member b's row starts begin at entry (atom offset + b).  d_inv_sqrt_mass (batch, n_s) or NULL.
 *
 * sc_dev_vsa_batch_blocks_f64: d_hss (batch, ms, ms), d_hes (batch, me, ms) row-major, d_hee (batch, me, me).  The unpadded
 * region of slot b has the bits sc_dev_subsystem_blocks_f64 gives for that member alone: it runs this code.  The pad of a
 * slot is 1.0 on the pad diagonal of H_ee and exactly 0.0 everywhere else, the pad rows of H_es included: the slot of H_ee is
 * diag(H_ee(b), I).  Every entry of every slot is written; no atomics; two calls agree bit for bit.  With env_order = 0,
 * d_hes and d_hee are not touched and may be NULL.
 *
 * sc_dev_vsa_batch_reduce_f64: per slot as sc_dev_subsystem_reduce_f64 -- d_hee <- diag(L_b, I), d_hes <- Y (pad rows 0),
 * d_hss <- H_eff, equal to its transpose bit for bit -- in one batched factorisation, one batched substitution and one
 * grouped product.  d_info (batch) as for sc_dev_potrf_f64: a failed member's H_eff is NaN, the others are not affected, and
 * the failure is reported once by the next synchronising call.  For a given me, a member's bits do not depend on the batch,
 * its place in it or its neighbours (they may depend on me: the block plan of the factorisation does).  me = 0: nothing is
 * reduced, H_eff = H_ss, d_info <- 0.
 *
 * sc_dev_vsa_batch_workspace: *bytes = the context scratch the reduction occupies (0 for env_order = 0).
 *
 * SC_ERR_INVALID_ARG before anything is launched: dim not 1 or 3, n_s < 1 (ms < 1), batch < 1 or above 65535, a negative
 * env_order (me), a member with n_e outside 0 .. env_order or n_s + n_e != its atom count or offsets out of sequence, a NULL
 * required pointer. */
int sc_dev_vsa_batch_workspace(int dim, int64_t n_s, int64_t env_order, int64_t batch, size_t* bytes);
int sc_dev_vsa_batch_blocks_f64(sc_ctx* ctx, const int64_t* members, int64_t batch, int dim, int64_t n_s, int64_t env_order,
                                const double* d_coord, const int64_t* d_pairs, const double* d_gamma,
                                const int64_t* d_row_start, const int32_t* d_group, const int32_t* d_pos,
                                const double* d_inv_sqrt_mass, double* d_hss, double* d_hes, double* d_hee);
int sc_dev_vsa_batch_reduce_f64(sc_ctx* ctx, double* d_hss, double* d_hes, double* d_hee, int64_t ms, int64_t me,
                                int64_t batch, int64_t* d_info);

/* ---- correlation networks (csrc/corr_network.hip) ---------------------------------------------------------------------------
 * No reference counterpart.  They replace Bio3D's cna on a dccm / lmi map and the all-pairs shortest paths and betweenness
 * of a graph library run on host copies of the maps (Sethi et al. 2009, WISP): the weighted residue graph of a coupling map,
 * the shortest path between every pair of nodes, and how many of those paths every node carries.
 *
 * `count` members in the packed pair layout of the batch consumers' dcc / prs / lmi results: member b is an (n_b, n_b)
 * row-major block at element offset off_b of every pair buffer, and its nodes start at atom_off_b of every per-node buffer.
 * d_rec (count, 3) int64 on the DEVICE holds (n_b, off_b, atom_off_b); n_max >= every n_b sizes the grids (a member with
 * n_b > n_max is skipped).  The caller keeps the records consistent with its buffers.  d_flags (count) int32: non-zero
 * marks a member without a defined result.  A member's bits depend on its own input alone: not on the batch, its place in
 * it or its neighbours; a member of a ragged batch has the bits of a batch of its own.  Every entry only enqueues.
 *
 * sc_dev_net_weights_f64: d_w[a, c] = -log(min(|c_ac|, 1)) where |c_ac| >= min_correlation and, with d_coord (sum n, 3) not
 * NULL, |x_a - x_c|^2 <= contact_cutoff_sq; +inf elsewhere; 0 on the diagonal.  d_flags is written: 1 for a member with a
 * NaN in its map or coordinates, else 0.  One streaming pass.
 *
 * sc_dev_net_paths_f64: d_d (distances, float64) and d_s (next hops, int32) of the non-negative weights d_w, which may be
 * asymmetric; +inf is "no edge", the diagonal is taken as 0.  Blocked Floyd-Warshall with 64 x 64 tiles, D[i, j] = min(D[i,
 * j], D[i, k] + D[k, j]), updated on strict improvement only with k ascending and S[i, j] <- S[i, k]; S starts as j on a
 * finite edge, i on the diagonal, else -1.  2 n^3 additions and comparisons per member, 3 launches per round of 64 pivots
 * whatever the batch.  d_s[i, j] is the node after i on the stored path to j, -1 exactly where d_d is +inf.  A symmetric d_w
 * gives d_d equal to its transpose bit for bit.  d_flags is read and written: a member flagged already, or with a NaN or
 * negative weight, ends with every d_d NaN and every d_s -1; nothing else is touched.  d_d may be d_w.
 *
 * sc_dev_net_usage: d_usage (sum n) int64, for node v the number of ordered pairs (a, t) with a, t, v distinct and t reachable
 * from a whose STORED path a -> d_s[a, t] -> ... -> t passes through v: one path per pair, so on ties not Brandes' fractional
 * betweenness.  A walk that takes more than n_b hops or meets a next hop outside 0 .. n_b - 1 sets the member's flag; a
 * flagged member's usage is -1.  The counters of one target are held in LDS: n_max <= 8192.  It occupies
 * sc_dev_net_workspace bytes of context scratch: an int32 per packed pair (total_sq = sum n_b^2).  That entry answers -1
 * for a total_sq below 1 or above 2^48.
 *
 * SC_ERR_INVALID_ARG before anything is launched: count outside 1 .. 65535, n_max outside 1 .. 262144 (usage: 8192),
 * min_correlation outside [0, 1], coordinates with a squared cutoff that is not positive, a total_sq that the workspace entry
 * refuses or above count n_max^2, a NULL required pointer. */
int sc_dev_net_weights_f64(sc_ctx* ctx, const int64_t* d_rec, int64_t count, int64_t n_max, const double* d_corr,
                           const double* d_coord, double contact_cutoff_sq, double min_correlation, double* d_w,
                           int32_t* d_flags);
int sc_dev_net_paths_f64(sc_ctx* ctx, const int64_t* d_rec, int64_t count, int64_t n_max, const double* d_w, double* d_d,
                         int32_t* d_s, int32_t* d_flags);
int64_t sc_dev_net_workspace(int64_t total_sq);
int sc_dev_net_usage(sc_ctx* ctx, const int64_t* d_rec, int64_t count, int64_t n_max, int64_t total_sq, const int32_t* d_s,
                     int64_t* d_usage, int32_t* d_flags);

/* ---- clustering of a dissimilarity matrix ---------------------------------------------------------------------------------
 * No reference counterpart.  The entries replace a host copy of an (n, n) matrix and gmx cluster -method gromos, Bio3D's
 * hclust / cutree or a k-medoids package run on it.  d_dist (n, n) float64 row-major on the DEVICE: an ensemble's pairwise
 * RMSD matrix, the distances of a correlation network, 1 - |dcc|; symmetry is expected and not verified.  Item i is
 * invalid when d_dist[i, i] is NaN: label -1, it neither counts nor is counted and is never a centre or a medoid.  Ties go
 * to the lowest index; two calls agree bit for bit.
 *
 * A run's state lives in d_ws, ws_bytes >= sc_cluster_workspace(n, k) bytes of device memory the caller owns and leaves
 * alone between the calls of a run; k = 0 sizes neighbour-count clustering, k >= 1 k-medoids with k medoids.  That entry
 * answers -1 for n outside 1 .. 262144 and k outside 0 .. min(n, 1024).  d_status, four int32 on the device, is the only
 * thing a host has to read during a run: [0] neighbour-count: the items without a label yet; k-medoids: 1 while SWAP may
 * still improve, 0 once it has converged; [1] the clusters made / the swaps accepted; [2] 1: a NaN between two valid items
 * -- every label is -1, [1] and [3] stay 0 and nothing else is defined; [3] k-medoids: the medoids placed, min(k, valid
 * items).  d_labels (n) int32.  Every entry only enqueues on the context's stream.
 *
 * sc_dev_cluster_gromos_init_f64 (Daura et al. 1999): reads d_dist once and never again; writes the workspace -- the bit
 * matrix adj[i, j] = (d_dist[i, j] <= cutoff or i == j) over valid i, j, one bit per pair, the counts of every row -- d_labels
 * (all -1) and d_status.  sc_dev_cluster_gromos_rounds: `rounds` rounds, each two launches: the alive item with the most
 * alive neighbours, the lowest index among equals, becomes centre c of the next cluster; its alive neighbours get label c's
 * number and leave; the counts of the rest are lowered.  d_reps / d_sizes (max_clusters) int32 receive the centre and the
 * size of every cluster made.  A round with nothing alive, or after max_clusters clusters, does nothing, so any number of
 * rounds may be enqueued.  Reads and writes the workspace, d_labels, d_status.
 *
 * sc_dev_cluster_kmedoids_init_f64 (PAM BUILD): k passes over d_dist.  The first medoid is the valid item with the smallest
 * sum over its row, every further one the item with the largest gain sum_j max(dn[j] - d_dist[i, j], 0); dn / ds are an
 * item's distances to its nearest and second-nearest medoid, read along the medoid's row, the lowest slot among equals.
 * Writes d_labels (the nearest slot), d_reps / d_sizes (k) int32 (the medoids, -1 / 0 past the medoids placed), d_td[0] (the
 * total deviation sum_j dn[j]), d_status.  sc_dev_cluster_kmedoids_swaps_f64: `iterations` SWAP iterations, each one pass
 * over d_dist and four launches: for every candidate x and slot s the change of the total deviation when x replaces the
 * medoid of s (the FastPAM1 evaluation, Schubert & Rousseeuw 2021); the smallest change, lowest x then lowest s among
 * equals, is applied if it is below 0 and d_td[status[1]] receives the new total deviation (dropped at td_cap entries);
 * else status[0] becomes 0 and every later iteration does nothing.  sc_cluster_form: the form that evaluation takes for
 * (n, k): 0, a workgroup keeps its candidate's row in LDS; 1, it gathers from global memory; same bits.
 * SPRINGCRAFT_CLUSTER_FORM = stream forces 1; = lds and = auto leave the size rule.  Read at every call.
 *
 * SC_ERR_INVALID_ARG before anything is launched: sizes sc_cluster_workspace refuses (k-medoids: k = 0 too), a workspace
 * that is NULL or smaller than it asks for, a cutoff that is negative or not finite, rounds or max_clusters outside 1 .. n,
 * iterations outside 1 .. 65536, td_cap below 1, a NULL required pointer. */
int64_t sc_cluster_workspace(int64_t n, int64_t k);
int sc_cluster_form(int64_t n, int64_t k);
int sc_dev_cluster_gromos_init_f64(sc_ctx* ctx, const double* d_dist, int64_t n, double cutoff, void* d_ws, size_t ws_bytes,
                                   int32_t* d_labels, int32_t* d_status);
int sc_dev_cluster_gromos_rounds(sc_ctx* ctx, int64_t n, int64_t rounds, int64_t max_clusters, void* d_ws, size_t ws_bytes,
                                 int32_t* d_labels, int32_t* d_reps, int32_t* d_sizes, int32_t* d_status);
int sc_dev_cluster_kmedoids_init_f64(sc_ctx* ctx, const double* d_dist, int64_t n, int64_t k, void* d_ws, size_t ws_bytes,
                                     int32_t* d_labels, int32_t* d_reps, int32_t* d_sizes, double* d_td, int64_t td_cap,
                                     int32_t* d_status);
int sc_dev_cluster_kmedoids_swaps_f64(sc_ctx* ctx, const double* d_dist, int64_t n, int64_t k, int64_t iterations, void* d_ws,
                                      size_t ws_bytes, int32_t* d_labels, int32_t* d_reps, int32_t* d_sizes, double* d_td,
                                      int64_t td_cap, int32_t* d_status);

#ifdef __cplusplus
}
#endif
#endif /* SPRINGCRAFT_HIP_H */
