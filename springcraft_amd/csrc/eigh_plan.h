// What the eigensolver's drivers (eigh.hip) share with the debug entries that run single stages (eigh_debug.hip): the
// workspace plan of a solve, its reduction step and its profile.
#pragma once

#include "eigh_internal.h"
#include "eigh_policy.h"

// Full spectrum, or a part of it: m_stein: columns of the inverse-iteration workspace held in the plan (0: none, for values
// only, or when the caller allocates it itself); window_k: slots of a value window (0: an index range).
struct SolveKind {
  bool partial = false;
  int m_stein = 0, window_k = 0;
};

// Workspace of a solve, carved out of ONE cached device allocation per context (sc_ctx::ws):
//   tri slab | [sb slab | diamond offsets] | [D&C slab or stein] | [bt slab | n x n scratch] | [U (n x n)] | descriptors |
//   [window counts | copy of w]
// Descriptors: the tridiagonalisation's records | the middle (two half-GEMMs per D&C merge, or the 2 * batch records of the
// inverse iteration) | the back-transformation's records.
struct SolvePlan {
  TriLayout TL;
  DcLayout DL;
  BtLayout BL;
  SbLayout SL;
  int nb = 0;   // panel width of the one-stage path
  bool two = false;   // the two-stage tridiagonalisation (eigh_policy.h:two_stage_for)
  size_t off_tri = 0, off_sb = 0, off_dia = 0, off_dc = 0, off_stein = 0, off_bt = 0, off_qtmp = 0, off_u = 0, off_desc = 0,
         off_win = 0, off_wcopy = 0, total = 0;
  int n_tri_desc = 0, n_mid_desc = 0, n_bt_desc = 0;
  GemmDesc* tri_descs(char* base) const { return (GemmDesc*)(base + off_desc); }
  GemmDesc* mid_descs(char* base) const { return tri_descs(base) + n_tri_desc; }
  GemmDesc* bt_descs(char* base) const { return mid_descs(base) + n_mid_desc; }
};
// ctx may be null (eigh_workspace_bytes): the environment's two-stage rule
SolvePlan make_solve_plan(const sc_ctx* ctx, int n, int batch, bool vectors, SolveKind kind = {});
size_t tri_slab_doubles(int n, int nb, TriLayout* out);

// Profiled solve: events around [0] tridiagonalisation, [1] tridiagonal eigenproblem, [2] back-transformation; ms_a / ms_b:
// SYMV / SYR2K sums, or the stage-1 / stage-2 times of the two-stage path; ms_bt2: the fused kernel that back-transforms
// the stage-2 reflectors.  finish() stores them in ctx->last_timings.
struct SolveProfile {
  sc_ctx* ctx;
  ScopedEvents<4> ev;
  float ms_a = 0.f, ms_b = 0.f, ms_bt2 = 0.f;
  explicit SolveProfile(sc_ctx* c) : ctx(c) {}
  int mark(int i);
  int finish(bool two, bool vectors);
};

// Mirror + scaling, then the tridiagonalisation the plan chose, into the plan's tri slab.  d_band_copy: null, or
// (batch, 128 x n), the band of every matrix as stage 1 left it (two-stage path, debug entries).
int tridiagonalise(sc_ctx* ctx, double* d_a, int n, int batch, const SolvePlan& P, char* base, SolveProfile& prof,
                   double* d_band_copy);

int check_window(sc_ctx* ctx, double vl, double vu);
