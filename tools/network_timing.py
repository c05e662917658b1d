"""
Timing of the correlation networks (csrc/corr_network.hip) with stream events.

    python tools/network_timing.py [--quick] [--no-host] > profiles/network.txt

Per shape (batch x N): a DeviceBatchSolver with fake modes (as tools/prs_timing.py) gives dcc(norm=True), the map the network
is built on with min_correlation = 0 (every pair is an edge: the time of the shortest paths does not depend on the graph,
that of the usage walk grows with the hops per path).  Timed separately through the C entries, on the same buffers:

    weights   sc_dev_net_weights_f64, one streaming pass
    paths     sc_dev_net_paths_f64: init, 3 launches per round of 64 pivots, the final pass
    usage     sc_dev_net_usage: the walk and the column sums

The model of the paths is 2 n^3 operations per member, one addition and one comparison per (i, j, k), at the float64 vector
rate: --peak TFLOP/s count a fused multiply-add as two, so a kernel of additions and comparisons can retire --peak / 2 of them.
(The kernel spends three selects per (i, j, k) more, on the two halves of D and on S: the model is a floor, not an estimate.)
The last column sets the three phases together against dcc(norm=True) of the same solver over all its modes.

Once, for scale only: scipy.sparse.csgraph.floyd_warshall on the host at N = 2000 (--no-host leaves it out).
Every event figure is the median of --repeat runs after one warm-up.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(torch, fn, repeat):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def fake_modes(torch, s, seed):
    g = torch.Generator(device=s.device).manual_seed(seed)
    m = s.w.shape[1]
    s.w.copy_(torch.linspace(0.5, 4.0, m, dtype=torch.float64, device=s.device)[None, :].expand(s.batch, -1))
    s.w[:, :6] = 1e-15
    for b in range(s.batch):
        s.v[b].normal_(generator=g).mul_(m ** -0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small shapes: a check that the tool runs")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--peak", type=float, default=78.6, help="float64 vector rate of the device, TFLOP/s (FMA = 2)")
    ap.add_argument("--no-host", action="store_true", help="leave out the host run of SciPy")
    args = ap.parse_args()
    import torch

    import springcraft_amd as sc
    from springcraft_amd import _hip, network as net
    from springcraft_amd.batch import DeviceBatchSolver

    L = _hip.lib()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    print(f"# tools/network_timing.py{' --quick' if args.quick else ''}: {_hip.context().info()}")
    print(f"# ms per call (events, median of {args.repeat}); model = 2 n^3 operations per member at {args.peak / 2:.1f} T operations / s")
    print("#  batch       N   weights ms    paths ms   model ms  fraction    usage ms   hops/path   dcc ms   (w + p + u) / dcc")
    shapes = ((3, 200), (1, 130)) if args.quick else ((64, 2000), (1, 2000), (1, 8000))
    keep_host = None
    for batch, n in shapes:
        s = DeviceBatchSolver(n, batch, sc.InvariantForceField(13.0))
        fake_modes(torch, s, 0)
        dcc_ms = median_ms(torch, lambda: s.dcc(), args.repeat)
        corr = s.dcc().view(-1)
        ctx = s.ctx
        del s
        torch.cuda.empty_cache()
        sizes = [n] * batch
        rec = torch.from_numpy(net.member_records(sizes)).cuda()
        w, d = torch.empty_like(corr), torch.empty_like(corr)
        hop = torch.empty(corr.shape, dtype=torch.int32, device="cuda")
        flags = torch.zeros(batch, dtype=torch.int32, device="cuda")
        usage = torch.empty(batch * n, dtype=torch.int64, device="cuda")

        def check(rc):
            ctx.check(rc)

        t_w = median_ms(torch, lambda: check(L.sc_dev_net_weights_f64(ctx.handle, p(rec), batch, n, p(corr), None, 0.0, 0.0,
                                                                      p(w), p(flags))), args.repeat)
        t_p = median_ms(torch, lambda: check(L.sc_dev_net_paths_f64(ctx.handle, p(rec), batch, n, p(w), p(d), p(hop), p(flags))),
                        args.repeat)
        t_u = median_ms(torch, lambda: check(L.sc_dev_net_usage(ctx.handle, p(rec), batch, n, batch * n * n, p(hop), p(usage),
                                                                p(flags))), args.repeat)
        assert int(flags.sum()) == 0 and bool(torch.isfinite(d).all())
        # every interior node of a path is one count: hops per path = 1 + usage / pairs
        hops = 1.0 + float(usage.sum()) / (batch * n * (n - 1))
        model = batch * 2.0 * n ** 3 / (args.peak / 2 * 1e12) * 1e3
        print(f"  {batch:6d}  {n:6d}   {t_w:10.3f}  {t_p:10.3f}  {model:9.3f}  {model / t_p:8.3f}  {t_u:10.3f}  {hops:10.2f}  "
              f"{dcc_ms:8.3f}   {(t_w + t_p + t_u) / dcc_ms:8.2f}")
        if n == (130 if args.quick else 2000) and batch == 1:
            keep_host = (w.view(n, n).cpu().numpy(), d.view(n, n).cpu().numpy(), t_p)
        del corr, w, d, hop, usage
        torch.cuda.empty_cache()

    if keep_host is not None and not args.no_host:
        from scipy.sparse.csgraph import floyd_warshall

        w, d, t_p = keep_host
        t = time.perf_counter()
        ref = floyd_warshall(w, directed=True)
        host = (time.perf_counter() - t) * 1e3
        worst = float(np.max(np.abs(d - ref) / np.where(ref > 0, ref, 1.0)))
        print(f"# host, for scale: scipy.sparse.csgraph.floyd_warshall at N = {len(w)}, one run: {host:.0f} ms (wall) against "
              f"{t_p:.3f} ms; largest relative difference of the distances {worst:.2e}")


if __name__ == "__main__":
    main()
