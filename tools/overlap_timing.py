"""
Cost of DeviceBatchSolver.overlap() (q = 1 and q = 4) and collectivity() against the MSF pass over the same rows of the
same solved tensors; keep the output as profiles/mode_overlap.txt.

  C3 shape: N = 2000 ANM, full spectrum (6000 modes), --structures structures (64 = the benchmarked batch)
  C5 shape: N = 8000 ANM, subset_by_index=(0, 105) (106 modes), one structure

All four read every row of v exactly once (nvec x m x 8 bytes per structure; the MSF is the C entry with the selection
"all rows from row 0", trivial rows included, so that it reads what the overlap reads), so the yardstick is the MSF pass
of the same solver in the same run: ms, bytes of v per second and the ratio to the MSF are printed.  The overlap also
reads q displacement vectors per two rows from cache and the collectivity takes one logarithm per atom and row.  Device
events around --reps back-to-back calls, --runs times after a warm-up, the consumers alternating run by run; median and
every run are printed.  No pass / fail.

Usage: python tools/overlap_timing.py [--structures B] [--reps R] [--runs K] [--skip-full]
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

HBM_ACHIEVABLE_TBS = 6.3


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
    s.solve(torch.from_numpy(np.stack([coord_of(n_atoms, b) for b in range(batch)])).cuda())
    s.finish()
    nvec, m = s.w.shape[1], s.m
    gen = torch.Generator(device=s.device).manual_seed(1)
    d4 = torch.randn((batch, 4, n_atoms, 3), dtype=torch.float64, device=s.device, generator=gen)
    d1 = d4[:, 0].contiguous()
    # what is timed is right: the overlaps against torch on one structure, the unit norm of the rows
    o = s.overlap(d4)
    ref = torch.einsum("rm,qm->qr", s.v[0], d4[0].reshape(4, m)) / d4[0].reshape(4, m).norm(dim=1)[:, None]
    err = float((o[0] - ref).abs().max())
    del o, ref
    # the MSF pass over ALL rows: the C entry with "all rows from row 0" on a preallocated output
    sel = _hip.ModeSelection()
    sel.kind, sel.row0 = _hip.SC_SEL_FROM_ROW, 0
    out = torch.empty((batch, n_atoms), dtype=torch.float64, device=s.device)
    L = _hip.lib()

    def msf():
        s.ctx.check(L.sc_dev_modes_msf_f64(s.ctx.handle, C.c_void_p(s.w.data_ptr()), C.c_void_p(s.v.data_ptr()), m, nvec,
                                           batch, 3, C.byref(sel), None, C.c_void_p(out.data_ptr())))

    names = ["overlap_q1", "overlap_q4", "collectivity", "msf_all_rows"]
    res = alternating_ms(torch, [lambda: s.overlap(d1), lambda: s.overlap(d4), s.collectivity, msf], reps, runs)
    nbytes = batch * nvec * m * 8
    msf_ms = res[3][0]
    line = {"case": label, "structures": batch, "rows": nvec, "m": m, "bytes_of_v": nbytes,
            "max_abs_err_overlap_vs_torch": err}
    for name, (ms, every) in zip(names, res):
        tbs = nbytes / (ms * 1e-3) / 1e12
        line.update({f"{name}_ms_median": round(ms, 4), f"{name}_ms_runs": every, f"{name}_TBps_of_v": round(tbs, 3),
                     f"{name}_share_of_6.3_TBps": round(tbs / HBM_ACHIEVABLE_TBS, 3),
                     f"{name}_over_msf": round(ms / msf_ms, 3)})
    print(json.dumps(line), flush=True)
    del s, out, d1, d4
    torch.cuda.empty_cache()


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=64)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip-full", action="store_true")
    args = ap.parse_args()
    print(json.dumps({"device": _hip.context().info(), "cmd": " ".join(sys.argv)}), flush=True)
    case(torch, "C5 shape: 1 x N=8000, subset_by_index=(0, 105)", 8000, 1, (0, 105), args.reps * 4, args.runs)
    if not args.skip_full:
        b = args.structures
        case(torch, f"C3 shape: {b} x N=2000, full spectrum", 2000, b, None, args.reps, args.runs)


if __name__ == "__main__":
    main()
