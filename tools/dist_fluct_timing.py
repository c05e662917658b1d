"""
Cost of DeviceBatchSolver.distance_fluctuation() (the pair kernel of csrc/dist_fluct.hip) against dcc(norm=False) -- one
grouped float64 MFMA GEMM -- of the same solver and the same selection; keep the output as profiles/dist_fluct.txt.

  few modes:  N = 2000 ANM, subset_by_index=(6, 25) (20 modes), --structures structures (64 = the benchmarked batch)
  all modes:  N = 1000 ANM, full spectrum, every non-trivial mode (2994), 4 structures

Both are the C entries on preallocated outputs with the selection "every row from the first non-trivial one", so nothing
is allocated or uploaded inside the timed region.  The pair kernel issues 8 float64 vector instructions per (pair, mode)
on N (N + 64) / 2 pairs per structure (only tiles with tile_a >= tile_c exist; diagonal tiles compute both orientations),
plus the unit vectors once per pair; that count over the device time is printed as instructions per second and as a
share of the data sheet's float64 vector rate (78.6 TFLOP/s = 39.3e12 fused multiply-adds per second).  Device events
around --reps back-to-back calls, --runs times after a warm-up, the two consumers alternating run by run; median and
every run are printed.  No pass / fail.

Usage: python tools/dist_fluct_timing.py [--structures B] [--reps R] [--runs K] [--skip-few] [--skip-all]
"""
import argparse
import ctypes as C
import json
import sys
from os.path import abspath, dirname

import numpy as np

sys.path.insert(0, dirname(dirname(abspath(__file__))))
import springcraft_amd as sc  # noqa: E402
from springcraft_amd import _hip  # noqa: E402
from springcraft_amd.batch import DeviceBatchSolver  # noqa: E402

F64_VECTOR_FMA_PER_S = 39.3e12


def coord_of(n_atoms, seed=0):
    return np.random.RandomState(seed).rand(n_atoms, 3) * 5.0 * n_atoms ** (1 / 3)


def alternating_ms(torch, fns, reps, runs, warmup=2):
    """For every callable of `fns`: (median, runs) of the device time of `reps` back-to-back calls / reps; the callables
    take turns run by run, so that a drift of the clocks hits all of them alike."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    out = [[] for _ in fns]
    for _ in range(runs):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) / reps)
    return [(float(np.median(o)), [round(x, 4) for x in o]) for o in out]


def case(torch, label, n_atoms, batch, subset, reps, runs):
    s = DeviceBatchSolver(n_atoms, batch, sc.InvariantForceField(13.0), subset_by_index=subset)
    x = torch.from_numpy(np.stack([coord_of(n_atoms, b) for b in range(batch)])).cuda()
    s.solve(x)
    s.finish()
    nvec, m = s.w.shape[1], s.m
    sel, _ = s._selection(None, pinv_default=False)     # every row from the first non-trivial one
    rows = nvec - int(sel.row0)
    # what is timed is right: the projected figure never exceeds the whole relative displacement, and both are symmetric
    f = s.distance_fluctuation(x)
    u = s.distance_fluctuation(x, projected=False)
    sym = bool(torch.equal(f, f.transpose(1, 2)))
    excess = float((f - u).max() / u.max())
    del f, u
    L = _hip.lib()
    out = torch.empty((batch, n_atoms, n_atoms), dtype=torch.float64, device=s.device)
    wp, vp, op = C.c_void_p(s.w.data_ptr()), C.c_void_p(s.v.data_ptr()), C.c_void_p(out.data_ptr())

    def fluct():
        s.ctx.check(L.sc_dev_modes_distfluct_f64(s.ctx.handle, wp, vp, m, nvec, batch, C.byref(sel), None,
                                                 C.c_void_p(x.data_ptr()), None, op))

    def dcc():
        s.ctx.check(L.sc_dev_modes_dcc_f64(s.ctx.handle, wp, vp, m, nvec, batch, 3, C.byref(sel), None, 0, 0, op))

    (f_ms, f_runs), (d_ms, d_runs) = alternating_ms(torch, [fluct, dcc], reps, runs)
    pairs = batch * n_atoms * (n_atoms + 64) // 2
    ips = 8.0 * pairs * rows / (f_ms * 1e-3)
    print(json.dumps({
        "case": label, "structures": batch, "n_atoms": n_atoms, "rows": rows, "pairs_computed": pairs,
        "symmetric_bit_for_bit": sym, "max_projected_minus_unprojected_over_max": excess,
        "distance_fluctuation_ms_median": round(f_ms, 4), "distance_fluctuation_ms_runs": f_runs,
        "dcc_unnormalised_ms_median": round(d_ms, 4), "dcc_unnormalised_ms_runs": d_runs,
        "distance_fluctuation_over_dcc": round(f_ms / d_ms, 3),
        "f64_vector_instructions_per_s": float(f"{ips:.4g}"),
        "share_of_39.3e12_per_s": round(ips / F64_VECTOR_FMA_PER_S, 3)}), flush=True)
    del s, out, x
    torch.cuda.empty_cache()


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=64)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip-few", action="store_true")
    ap.add_argument("--skip-all", action="store_true")
    args = ap.parse_args()
    print(json.dumps({"device": _hip.context().info(), "cmd": " ".join(sys.argv)}), flush=True)
    if not args.skip_all:
        case(torch, "all modes: 4 x N=1000, full spectrum", 1000, 4, None, args.reps, args.runs)
    if not args.skip_few:
        b = args.structures
        case(torch, f"few modes: {b} x N=2000, subset_by_index=(6, 25)", 2000, b, (6, 25), args.reps, args.runs)


if __name__ == "__main__":
    main()
