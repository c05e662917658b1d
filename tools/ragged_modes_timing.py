"""
Timings of the ragged partial-spectrum solve and its consumers (RaggedBatchSolver); keep the output as
profiles/ragged_modes.txt.

16 ANM structures with N between 1 700 and 2 000 (Hinsen force field, one padded batch of order 6 000), one warm-up and
three timed repeats each, device events on the solver's stream plus the host's wall clock around the same calls:

  (a) full ragged solve + results()                      -- what the library could do before
  (b) subset_by_index=(0, 25)
  (c) (b) + bfactor() + dcc()
  (d) full solve, then ragged mean_square_fluctuation() + dcc() on the device, against the same two quantities computed on
      the host from a copy of ONE structure's eigenpairs (the copy included: that is what a ragged caller had to do)

and the phase split of (b) from last_timings() (one extra profiled run: profiling synchronises between phases).

Usage: python tools/ragged_modes_timing.py [--structures 16] [--repeats 3]
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
from springcraft_amd.batch import RaggedBatchSolver  # noqa: E402


def coord_of(n_atoms, seed):
    return np.random.RandomState(seed).rand(n_atoms, 3) * 5.0 * n_atoms ** (1 / 3)


def timed(torch, fn, repeats):
    """One warm-up, then `repeats` runs: (device ms, wall ms) of each."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append((round(a.elapsed_time(b), 2), round((time.perf_counter() - t0) * 1e3, 2)))
    return out


def med(runs):
    return float(np.median([r[0] for r in runs]))


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    B = args.structures
    sizes = [int(x) for x in np.linspace(1700, 2000, B).round()]
    coords = torch.from_numpy(np.concatenate([coord_of(n, k) for k, n in enumerate(sizes)])).cuda().contiguous()
    ff = sc.HinsenForceField(13.0)
    print(json.dumps({"device": _hip.context().info(), "cmd": " ".join(sys.argv), "sizes": sizes}), flush=True)

    full = RaggedBatchSolver(sizes, ff)

    def run_a():
        full.solve(coords)
        return full.results()

    a = timed(torch, run_a, args.repeats)
    print(json.dumps({"case": "(a) full solve + results()", "order": full.order, "device_ms, wall_ms": a}), flush=True)

    def run_d():
        return full.mean_square_fluctuation(), full.dcc()

    d = timed(torch, run_d, args.repeats)

    def host_one():
        w, v = full.results()[-1]
        w, v = w.cpu().numpy(), v.cpu().numpy()
        n = sizes[-1]
        s = 1.0 / w[6:]
        msf = ((v[6:] ** 2) * s[:, None]).sum(axis=0).reshape(-1, 3).sum(axis=1)
        keep = np.abs(w) > 1e-6 * np.abs(w).max()
        c = np.zeros((n, n))
        for k in range(3):
            vd = np.ascontiguousarray(v[keep][:, k::3])
            c += np.ascontiguousarray(vd.T / w[keep]) @ vd
        dd = np.sqrt(np.diag(c))
        return msf, c / np.outer(dd, dd)

    h = timed(torch, host_one, args.repeats)
    print(json.dumps({"case": "(d) msf() + dcc() of all structures on the device, after a full solve",
                      "device_ms, wall_ms": d,
                      "host: copy of one structure's (w, v) + the same two in NumPy, wall_ms": [r[1] for r in h],
                      "host_one_structure_over_device_all": round(float(np.median([r[1] for r in h])) / med(d), 2)}),
          flush=True)
    del full
    torch.cuda.empty_cache()

    part = RaggedBatchSolver(sizes, ff, subset_by_index=(0, 25))

    def run_b():
        part.solve(coords)
        return part.results()

    b = timed(torch, run_b, args.repeats)
    print(json.dumps({"case": "(b) subset_by_index=(0, 25) + results()", "device_ms, wall_ms": b,
                      "b_over_a": round(med(b) / med(a), 4)}), flush=True)

    def run_c():
        part.solve(coords)
        return part.bfactor(), part.dcc()

    c = timed(torch, run_c, args.repeats)
    print(json.dumps({"case": "(c) (b) + bfactor() + dcc()", "device_ms, wall_ms": c,
                      "c_over_a": round(med(c) / med(a), 4), "consumers_ms": round(med(c) - med(b), 2)}), flush=True)
    part.set_profiling(True)
    part.solve(coords)
    part.finish()
    print(json.dumps({"case": "(b) phases, one profiled run", "last_timings": part.last_timings()}), flush=True)


if __name__ == "__main__":
    main()
