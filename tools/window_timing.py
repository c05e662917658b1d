"""
Cost of the eigenvalue window (subset_by_value) against the index range (subset_by_index) that returns the same
eigenpairs, interleaved in one process: every call is timed behind a device synchronisation, after warm-up calls.

  single ANM, N = 8000, 13 A cutoff (config C5): the 106 lowest non-trivial modes (index 6 .. 111)
  single ANM, N = 2000: 100 modes (index 6 .. 105)
  DeviceBatchSolver, 16 x N = 1000: index 6 .. 105 (m = 100) against a window with K = m (bounds from member 0)

The window's bounds are the midpoints between the neighbouring eigenvalues of the index range.  Target: the window costs
no more than the index path + max(2 ms, 2 %).  Usage: python tools/window_timing.py [--reps R] [--warmup W]
"""
import argparse
import json
import sys
import time
from os.path import abspath, dirname

import numpy as np

sys.path.insert(0, dirname(dirname(abspath(__file__))))
import springcraft_amd as sc  # noqa: E402
from springcraft_amd import _hip  # noqa: E402


def coord_of(n_atoms, seed=0):
    return np.random.RandomState(seed).rand(n_atoms, 3) * 5.0 * n_atoms ** (1 / 3)


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return (time.perf_counter() - t0) * 1e3, out


def compare(label, run_index, run_window, sync, reps, warmup):
    for _ in range(warmup):
        run_index()
        run_window()
    t_i, t_w = [], []
    for _ in range(reps):
        t, _ = timed(run_index, sync)
        t_i.append(t)
        t, _ = timed(run_window, sync)
        t_w.append(t)
    mi, mw = float(np.median(t_i)), float(np.median(t_w))
    allowed = mi + max(2.0, 0.02 * mi)
    r = {"case": label, "index_ms_median": round(mi, 3), "window_ms_median": round(mw, 3),
         "extra_ms": round(mw - mi, 3), "extra_pct": round(100 * (mw - mi) / mi, 2), "allowed_ms": round(allowed, 3),
         "within_target": bool(mw <= allowed), "index_ms": [round(x, 3) for x in t_i],
         "window_ms": [round(x, 3) for x in t_w]}
    print(json.dumps(r), flush=True)
    return r


def single_anm(n_atoms, lo, hi, reps, warmup):
    ctx = _hip.context()
    coord = coord_of(n_atoms)
    ff = sc.InvariantForceField(13.0)
    w = sc.ANM(coord, ff).eigen(subset_by_index=(0, hi + 1))[0]
    vl, vu = 0.5 * (w[lo - 1] + w[lo]), 0.5 * (w[hi] + w[hi + 1])
    m = len(sc.ANM(coord, ff).eigen(subset_by_value=(vl, vu))[0])
    assert m == hi - lo + 1, (m, lo, hi)
    return compare(f"ANM N={n_atoms} modes {lo}..{hi} (m={m})",
                   lambda: sc.ANM(coord, ff).eigen(subset_by_index=(lo, hi)),
                   lambda: sc.ANM(coord, ff).eigen(subset_by_value=(vl, vu)), ctx.synchronize, reps, warmup)


def batch_anm(n_atoms, batch, lo, hi, reps, warmup):
    import torch

    from springcraft_amd.batch import DeviceBatchSolver

    ff = sc.InvariantForceField(13.0)
    coords = np.stack([coord_of(n_atoms, seed) for seed in range(batch)])
    w0 = sc.ANM(coords[0], ff).eigen(subset_by_index=(0, hi + 1))[0]
    vl, vu = 0.5 * (w0[lo - 1] + w0[lo]), 0.5 * (w0[hi] + w0[hi + 1])
    m = hi - lo + 1
    d_coord = torch.from_numpy(coords).cuda()
    s_index = DeviceBatchSolver(n_atoms, batch, ff, subset_by_index=(lo, hi))
    s_window = DeviceBatchSolver(n_atoms, batch, ff, subset_by_value=(vl, vu), max_modes=m)

    def run(s):
        s.solve(d_coord)
        s.ctx.synchronize()

    r = compare(f"DeviceBatchSolver {batch} x ANM N={n_atoms} index {lo}..{hi} / window K={m}",
                lambda: run(s_index), lambda: run(s_window), torch.cuda.synchronize, reps, warmup)
    print(json.dumps({"case": r["case"], "window_counts": s_window.counts.cpu().tolist()}), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-c5", action="store_true")
    args = ap.parse_args()
    print(json.dumps({"device": _hip.context().info()}), flush=True)
    if not args.skip_c5:
        single_anm(8000, 6, 111, args.reps, args.warmup)
    single_anm(2000, 6, 105, args.reps, args.warmup)
    batch_anm(1000, 16, 6, 105, args.reps, args.warmup)


if __name__ == "__main__":
    main()
