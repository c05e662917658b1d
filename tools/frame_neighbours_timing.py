"""
Timing of the frames' neighbour bits and of matrix-free neighbour-count clustering (csrc/rmsd_matrix.hip's bit epilogue)
with stream events.

    python tools/frame_neighbours_timing.py [--quick] [--baseline-lib OTHER.so] [--large M] > profiles/frame_neighbours.txt

Input: tools/cluster_timing.py's hierarchy of M frames of N = 2000 atoms, so that cutoff 2.5 gives about 10 clusters and
cutoff 0.6 about 1000.

1. M = 10^4, by entry: rmsd_matrix alone, the pack pass of the stored matrix (sc_dev_cluster_gromos_init_f64), their sum, and
   the matrix-free init (sc_dev_frame_neighbours_init_f64), which replaces both; the ratio of the two.  With --baseline-lib
   the first two are also measured on that library (the parent commit's build) in the same process.
2. The bits by which neighbours() differs from rmsd_matrix() <= cutoff (the diagonal forced true) on that input: all pairs,
   no guard band.
3. Whole runs, wall clock around a call that ends in its status read: Ensemble.cluster("gromos") two-step against
   matrix_free=True at the two cutoffs, labels compared.
4. --large M (default 10^5; 0: skip), matrix-free only, max_clusters = 10: time, and the peak device memory of the run:
   torch.cuda.max_memory_allocated above what the frames take, plus the context scratch (sc_rmsd_matrix_workspace).

Every event figure is the median of --repeat runs after one warm-up.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.cluster_timing import event_ms, hierarchy_frames, wall_ms   # noqa: E402


def baseline(path, stream):
    """(library, context handle) of another build of the library, with the three entries the comparison needs typed."""
    B = C.CDLL(path)
    vp, i64, i32, dbl = C.c_void_p, C.c_int64, C.c_int, C.c_double
    B.sc_ctx_create_on_stream.argtypes, B.sc_ctx_create_on_stream.restype = [i32, vp, C.POINTER(vp)], i32
    B.sc_dev_rmsd_matrix_f64.argtypes, B.sc_dev_rmsd_matrix_f64.restype = [vp, vp, i64, vp, i64, i64, vp, i32, vp], i32
    B.sc_dev_cluster_gromos_init_f64.argtypes = [vp, vp, i64, dbl, vp, C.c_size_t, vp, vp]
    B.sc_dev_cluster_gromos_init_f64.restype = i32
    h = vp()
    if B.sc_ctx_create_on_stream(0, vp(int(stream)), C.byref(h)) != 0:
        raise RuntimeError(f"{path}: no context")
    return B, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small shapes: a check that the tool runs")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--baseline-lib", help="another build of the library to time rmsd_matrix and the pack pass on")
    ap.add_argument("--large", type=int, default=None, help="frames of the matrix-free-only run (0: skip)")
    args = ap.parse_args()
    import torch

    import springcraft_amd as sc
    from springcraft_amd import _hip

    L = _hip.lib()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    print(f"# tools/frame_neighbours_timing.py{' --quick' if args.quick else ''}: {_hip.context().info()}")
    n_atoms = 50 if args.quick else 2000
    m = 1000 if args.quick else 10000
    large = (3000 if args.quick else 100000) if args.large is None else args.large
    cut_few, cut_many = 2.5, 0.6
    stream = torch.cuda.current_stream().cuda_stream

    ens = sc.Ensemble(hierarchy_frames(torch, m, n_atoms, m))
    ctx = ens.ctx
    dist = ens.rmsd_matrix()
    size = L.sc_cluster_workspace(m, 0)
    ws = torch.empty((size,), dtype=torch.uint8, device="cuda")
    labels = torch.empty((m,), dtype=torch.int32, device="cuda")
    status = torch.empty((4,), dtype=torch.int32, device="cuda")
    print(f"\n# 1. M = {m}, N = {n_atoms}, by entry (events): dist is {8 * m * m / 1e6:.1f} MB, the bit matrix "
          f"{8 * m * ((m + 63) // 64) / 1e6:.2f} MB")
    t_mat = event_ms(torch, lambda: ctx.check(L.sc_dev_rmsd_matrix_f64(ctx.handle, p(ens.frames), m, None, m, n_atoms, None, 1,
                                                                       p(dist))), args.repeat)
    t_pack = event_ms(torch, lambda: ctx.check(L.sc_dev_cluster_gromos_init_f64(ctx.handle, p(dist), m, cut_many, p(ws), size,
                                                                                p(labels), p(status))), args.repeat)
    t_free = event_ms(torch, lambda: ctx.check(L.sc_dev_frame_neighbours_init_f64(ctx.handle, p(ens.frames), m, n_atoms, None, 1,
                                                                                  cut_many, p(ws), size, p(labels), p(status))),
                      args.repeat)
    print(f"   rmsd_matrix {t_mat:.3f} ms + pack pass {t_pack:.3f} ms = {t_mat + t_pack:.3f} ms; matrix-free init "
          f"{t_free:.3f} ms = {t_free / (t_mat + t_pack):.4f} x the two")
    if args.baseline_lib:
        B, h = baseline(args.baseline_lib, stream)
        b_mat = event_ms(torch, lambda: B.sc_dev_rmsd_matrix_f64(h, p(ens.frames), m, None, m, n_atoms, None, 1, p(dist)),
                         args.repeat)
        b_pack = event_ms(torch, lambda: B.sc_dev_cluster_gromos_init_f64(h, p(dist), m, cut_many, p(ws), size, p(labels),
                                                                          p(status)), args.repeat)
        print(f"   baseline library: rmsd_matrix {b_mat:.3f} ms + pack pass {b_pack:.3f} ms = {b_mat + b_pack:.3f} ms; "
              f"matrix-free init = {t_free / (b_mat + b_pack):.4f} x the baseline's two; rmsd_matrix here / baseline "
              f"{t_mat / b_mat:.4f}")
    del ws

    eye = torch.eye(m, dtype=torch.bool, device="cuda")
    for cut in (cut_few, cut_many):
        differ = int((ens.neighbours(cut).dense() != ((dist <= cut) | eye)).sum())
        print(f"# 2. cutoff {cut}: {differ} of {m * m} bits of neighbours() differ from rmsd_matrix() <= cutoff")
    del eye

    print("# 3. whole runs (wall clock, status reads included)")
    for cut in (cut_few, cut_many):
        t_two, two = wall_ms(torch, lambda: ens.cluster("gromos", cutoff=cut), args.repeat)
        t_one, one = wall_ms(torch, lambda: ens.cluster("gromos", cutoff=cut, matrix_free=True), args.repeat)
        print(f"   cutoff {cut}: {two.n_clusters} clusters; two-step {t_two:.2f} ms, matrix_free {t_one:.2f} ms = "
              f"{t_one / t_two:.4f} x; labels equal: {bool(torch.equal(two.labels, one.labels))}")
    del dist, ens, two, one
    torch.cuda.empty_cache()

    if large:
        ens = sc.Ensemble(hierarchy_frames(torch, large, n_atoms, large))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t, r = wall_ms(torch, lambda: ens.cluster("gromos", cutoff=cut_few, matrix_free=True, max_clusters=10), 1)
        made = r.n_clusters
        peak = torch.cuda.max_memory_allocated() - base
        scratch = L.sc_rmsd_matrix_workspace(large, 0, n_atoms)
        print(f"\n# 4. M = {large}, N = {n_atoms}, matrix_free, max_clusters = 10: {made} clusters, largest {int(r.sizes[0])}, "
              f"{t:.1f} ms (ending in a status read); frames {base / 1e9:.3f} GB; peak above them {peak / 1e9:.3f} GB + context "
              f"scratch {scratch / 1e9:.3f} GB (the centred copy) = {(peak + scratch) / 1e9:.3f} GB; the float64 matrix would be "
              f"{8 * large * large / 1e9:.1f} GB")


if __name__ == "__main__":
    main()
