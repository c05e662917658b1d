"""
Timing of the clustering kernels (csrc/cluster.hip) with stream events.

    python tools/cluster_timing.py [--quick] [--ratios PYTEST_LOG] > profiles/cluster.txt

Input: M frames of N = 2000 atoms in a two-level hierarchy -- 10 groups of 100 sub-groups of M / 1000 frames -- so that one
cutoff gives about 10 clusters and another about 1000; the matrix is Ensemble.rmsd_matrix() of them, M = 2000 and 10^4.

1. The copy rate of the run: a device-to-device copy of the matrix, 16 M^2 bytes moved.  One pass over dist (8 M^2 bytes
   read) at that rate is what the pack pass, a BUILD step and a SWAP iteration are set against.
2. The pack pass (sc_dev_cluster_gromos_init_f64) and a neighbour-count round (the mean of the rounds of a run that makes
   about 1000 clusters) against the bytes of the bit matrix at the copy rate.
3. A BUILD step (sc_dev_cluster_kmedoids_init_f64 at k = 10, per medoid) and the first SWAP iteration after a fresh BUILD
   (sc_dev_cluster_kmedoids_swaps_f64, k = 10 and 100), in the form the size rule takes and, where both exist, forced.
4. Whole runs, wall clock around a call that ends in its status read: cluster_gromos at the two cutoffs, cluster_kmedoids
   at k = 10 and k = 100.
5. The NumPy specification (tests/cluster_model.py) on the host, for scale only, where it ends in reasonable time.
6. With --ratios: the largest measured / gate ratio in the output of ``pytest tests/test_cluster_gpu.py -m gpu -s``.

Every event figure is the median of --repeat runs after one warm-up.
"""
import argparse
import ctypes as C
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def event_ms(torch, fn, repeat, before=None):
    """Median ms of fn() between two events; before() runs outside the timed window every time."""
    times = []
    for r in range(repeat + 1):
        if before is not None:
            before()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if r:
            times.append(a.elapsed_time(b))
    return float(np.median(times))


def wall_ms(torch, fn, repeat):
    fn()
    times = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return float(np.median(times)), out


def hierarchy_frames(torch, m, n_atoms, seed):
    """10 groups (scale 2) of 100 sub-groups (scale 0.5) of m / 1000 frames (noise 0.1), in random order, on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *shape: torch.randn(shape, generator=g, dtype=torch.float64, device="cuda")   # noqa: E731
    base = rnd(1, n_atoms, 3) * 5.0
    top = 2.0 * rnd(10, n_atoms, 3)
    sub = 0.5 * rnd(1000, n_atoms, 3)
    which = torch.randperm(m, generator=g, device="cuda") % 1000
    return base + top[which // 100] + sub[which] + 0.1 * rnd(m, n_atoms, 3)


def ratios(path):
    worst, count = 0.0, 0
    for line in open(path):
        for v in re.findall(r"= (\d+\.\d+)\s*$", line):
            worst, count = max(worst, float(v)), count + 1
    print(f"# 6. largest measured / gate ratio of {count} printed comparisons (tests/test_cluster_gpu.py): {worst:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small shapes: a check that the tool runs")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--ratios", help="output of pytest -s of the GPU tests, to summarise")
    args = ap.parse_args()
    import torch

    import springcraft_amd as sc
    from springcraft_amd import _hip
    from tests import cluster_model as cm

    L = _hip.lib()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    print(f"# tools/cluster_timing.py{' --quick' if args.quick else ''}: {_hip.context().info()}")
    n_atoms = 50 if args.quick else 2000
    for m in ((1000,) if args.quick else (2000, 10000)):
        ens = sc.Ensemble(hierarchy_frames(torch, m, n_atoms, m))
        dist = ens.rmsd_matrix()
        del ens
        torch.cuda.synchronize()
        ctx = _hip.Context(0, stream=torch.cuda.current_stream().cuda_stream)
        host = dist.cpu().numpy()
        off = host[np.triu_indices(m, 1)]
        cut_few, cut_many = 2.5, 0.6
        print(f"\n# M = {m}, N = {n_atoms}: dist is {8 * m * m / 1e6:.1f} MB; off-diagonal RMSD quantiles 1 / 50 / 99 %: "
              f"{np.quantile(off, 0.01):.3f} {np.quantile(off, 0.5):.3f} {np.quantile(off, 0.99):.3f}")
        other = torch.empty_like(dist)
        copy = event_ms(torch, lambda: other.copy_(dist), args.repeat)
        rate = 16.0 * m * m / copy * 1e-6   # GB/s
        one_pass = copy / 2
        del other
        print(f"# 1. device copy of dist: {copy:.3f} ms, {rate:.0f} GB/s; one pass over dist at that rate: {one_pass:.3f} ms")

        # ---- neighbour count, by entry
        size = L.sc_cluster_workspace(m, 0)
        ws = torch.empty((size,), dtype=torch.uint8, device="cuda")
        labels, reps, sizes = (torch.empty((m,), dtype=torch.int32, device="cuda") for _ in range(3))
        status = torch.empty((4,), dtype=torch.int32, device="cuda")
        init = lambda cut: ctx.check(L.sc_dev_cluster_gromos_init_f64(ctx.handle, p(dist), m, cut, p(ws), size, p(labels),   # noqa: E731
                                                                      p(status)))
        rounds = lambda r: ctx.check(L.sc_dev_cluster_gromos_rounds(ctx.handle, m, r, m, p(ws), size, p(labels), p(reps),   # noqa: E731
                                                                    p(sizes), p(status)))
        pack = event_ms(torch, lambda: init(cut_many), args.repeat)
        adj_mb = 8.0 * m * ((m + 63) // 64) / 1e6
        print(f"# 2. pack pass: {pack:.3f} ms = {pack / one_pass:.2f} x one pass at the copy rate")
        made = sc.cluster_gromos(dist, cut_many).n_clusters
        chunk = max(1, min(made, m))
        t = event_ms(torch, lambda: rounds(chunk), args.repeat, before=lambda: init(cut_many))
        print(f"   neighbour-count round: {1e3 * t / chunk:.2f} us (mean of the {chunk} rounds of a run that makes {made} clusters, "
              f"one enqueue); bit matrix {adj_mb:.2f} MB = {1e3 * adj_mb / rate:.2f} us at the copy rate")
        del ws

        # ---- k-medoids, by entry
        print("# 3. k-medoids by entry (events)")
        for k in (10, 100):
            size = L.sc_cluster_workspace(m, k)
            ws = torch.empty((size,), dtype=torch.uint8, device="cuda")
            td = torch.zeros((8,), dtype=torch.float64, device="cuda")
            build = lambda: ctx.check(L.sc_dev_cluster_kmedoids_init_f64(ctx.handle, p(dist), m, k, p(ws), size, p(labels),   # noqa: E731
                                                                         p(reps), p(sizes), p(td), 8, p(status)))
            swap = lambda: ctx.check(L.sc_dev_cluster_kmedoids_swaps_f64(ctx.handle, p(dist), m, k, 1, p(ws), size, p(labels),   # noqa: E731
                                                                         p(reps), p(sizes), p(td), 8, p(status)))
            t_build = event_ms(torch, build, args.repeat)
            print(f"   k = {k:3d}: BUILD {t_build:.3f} ms, {t_build / k:.3f} ms per medoid = {t_build / k / one_pass:.2f} x one pass")
            for form in ("auto", "lds", "stream"):
                os.environ["SPRINGCRAFT_CLUSTER_FORM"] = form
                taken = "lds" if L.sc_cluster_form(m, k) == 0 else "stream"
                if form != "auto" and taken != form:
                    print(f"            SWAP iteration, {form}: not measured (the row does not fit LDS)")
                    continue
                t_swap = event_ms(torch, swap, args.repeat, before=build)
                print(f"            SWAP iteration, {form} ({taken} form): {t_swap:.3f} ms = {t_swap / one_pass:.2f} x one pass")
            os.environ.pop("SPRINGCRAFT_CLUSTER_FORM", None)
            del ws

        # ---- whole runs
        print("# 4. whole runs (wall clock, status reads included)")
        for cut in (cut_few, cut_many):
            t, r = wall_ms(torch, lambda: sc.cluster_gromos(dist, cut), args.repeat)
            print(f"   cluster_gromos(cutoff = {cut}): {r.n_clusters} clusters, largest {int(r.sizes[0])}, {t:.2f} ms, "
                  f"{r.status_reads} status reads")
        for k in (10, 100):
            t, r = wall_ms(torch, lambda: sc.cluster_kmedoids(dist, k), args.repeat)
            print(f"   cluster_kmedoids(k = {k}): {r.iterations} swaps, converged {r.converged}, {t:.2f} ms, "
                  f"{r.status_reads} status reads, total deviation {float(r.total_deviation[0]):.3f} -> "
                  f"{float(r.total_deviation[-1]):.3f}")

        # ---- the specification on the host, for scale only
        print("# 5. the NumPy specification on the host (one run each, for scale only)")
        for cut in (cut_few, cut_many):
            if m > 2000 and cut == cut_many:
                print(f"   gromos model(cutoff = {cut}): not measured (about 1000 rounds over a {m} x {m} boolean matrix)")
                continue
            t = time.perf_counter()
            ref = cm.gromos(host, cut)
            print(f"   gromos model(cutoff = {cut}): {len(ref[1])} clusters, {(time.perf_counter() - t) * 1e3:.0f} ms; "
                  f"labels equal the device's: {np.array_equal(ref[0], sc.cluster_gromos(dist, cut).labels.cpu().numpy())}")
        if m <= 2000:
            t = time.perf_counter()
            ref = cm.kmedoids(host, 10, max_iter=1)
            print(f"   k-medoids model(k = 10, BUILD and one SWAP iteration): {(time.perf_counter() - t) * 1e3:.0f} ms")
        else:
            print("   k-medoids model: not measured (a SWAP iteration is M^2 steps of a Python loop)")
        del dist
        torch.cuda.empty_cache()
    if args.ratios:
        ratios(args.ratios)


if __name__ == "__main__":
    main()
