"""
Timings of the device Cholesky solver and of a whole subsystem solve (stream events), written to profiles/subsystem.txt:

    python tools/subsystem_timing.py [--out profiles/subsystem.txt] [--quick] [--no-eigh]

  1. sc_dev_potrf_f64 at n = 6000 / 12000 / 24000: ms, TFLOP/s (n^3 / 3 flop), the fraction of the 78.6 TFLOP/s float64 matrix
     peak, and torch.linalg.cholesky on the same tensor beside it (a comparison only: the product never calls it).
  2. The outer block: the same factorisation at n = 12000 with SPRINGCRAFT_POTRF_OUTER = 64 .. 1024.
  3. Subsystem.solve() on N = 8000 atoms with n_s = 500 and 2000, split into assembly, reduction (factorisation, substitution,
     product: the context's phase timers) and eigensolve.
  4. sc_dev_eigh_f64 on a matrix of H_ee's order: the only other way to apply H_ee^-1 the library has.
"""
import argparse
import ctypes as C
import os
import sys
from os.path import abspath, dirname, join

import numpy as np

ROOT = dirname(dirname(abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=join(ROOT, "profiles", "subsystem.txt"))
    ap.add_argument("--quick", action="store_true", help="a quarter of every size")
    ap.add_argument("--no-eigh", action="store_true", help="skip part 4")
    args = ap.parse_args()
    import torch

    import springcraft_amd as sc
    from springcraft_amd import _hip

    L = _hip.lib()
    ctx = _hip.Context(torch.cuda.current_device(), stream=torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    div = 4 if args.quick else 1
    lines = [f"# tools/subsystem_timing.py on {ctx.info()}", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, repeat=3):
        """Median ms of `repeat` runs between stream events, after one warm-up run."""
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(repeat):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
        return float(np.median(out))

    def spd(n):
        g = torch.randn((n, n), dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(n))
        a = g @ g.T / n
        a.diagonal().add_(1.0)
        return a

    def potrf_ms(a, n):
        work, info = torch.empty_like(a), torch.zeros(1, dtype=torch.int64, device="cuda")

        def run():
            work.copy_(a)
            ctx.check(L.sc_dev_potrf_f64(ctx.handle, p(work), n, n, n * n, 1, p(info)))

        copy = timed(lambda: work.copy_(a))
        ms = timed(run) - copy
        ctx.synchronize()
        assert int(info.cpu()[0]) == 0
        return ms, work

    say("## 1. potrf, one matrix: ms, TFLOP/s, fraction of 78.6 TFLOP/s; torch.linalg.cholesky on the same tensor")
    for n in (6000 // div, 12000 // div, 24000 // div):
        a = spd(n)
        ms, work = potrf_ms(a, n)
        ref_ms = timed(lambda: torch.linalg.cholesky(a))
        ref = torch.linalg.cholesky(a)
        err = float((torch.triu(work).T - ref).abs().max() / ref.abs().max())
        flops = n ** 3 / 3.0
        say(f"n = {n:6d}: {ms:9.2f} ms  {flops / ms / 1e9:6.2f} TFLOP/s  {flops / ms * 1e3 / PEAK:5.3f} of peak   "
            f"torch {ref_ms:9.2f} ms   max |L - L_torch| / max|L| = {err:.1e}")
        del a, work, ref
    say()

    say("## 2. outer block sweep at n = %d (SPRINGCRAFT_POTRF_OUTER; inner block 64)" % (12000 // div))
    a = spd(12000 // div)
    for outer in (64, 128, 256, 384, 512, 1024):
        os.environ["SPRINGCRAFT_POTRF_OUTER"] = str(outer)
        say(f"outer = {outer:5d}: {potrf_ms(a, 12000 // div)[0]:9.2f} ms")
    del os.environ["SPRINGCRAFT_POTRF_OUTER"]
    del a
    say()

    say("## 3. Subsystem.solve(), N = %d atoms, InvariantForceField(13): ms per stage" % (8000 // div))
    n_atoms = 8000 // div
    coord = np.random.RandomState(1).rand(n_atoms, 3) * 5.0 * n_atoms ** (1.0 / 3.0)
    orders = []
    for n_s in (500 // div, 2000 // div):
        system = np.sort(np.random.default_rng(1).choice(n_atoms, n_s, replace=False))
        sub = sc.Subsystem(coord, sc.InvariantForceField(13.0), system)
        sub.set_profiling(True)
        sub._allocate(sub.m, sub.m)
        hss = sub.matrix
        t_asm = timed(lambda: sub._blocks_into(hss, sub._hes, sub._hee) if sub._hes is not None else sub._reduce_into(hss))
        t_red = timed(lambda: sub._reduce_into(hss)) - t_asm
        phases = {}
        for name in ("subsystem_potrf", "subsystem_trsm", "subsystem_syrk"):
            ms = C.c_double(0.0)
            L.sc_last_eigh_phase_ms(sub.ctx.handle, name.encode(), C.byref(ms))
            phases[name] = ms.value
        sub.set_profiling(False)
        t_all = timed(lambda: sub.solve(), repeat=2)
        sub.finish()
        flops = 0.0
        me, ms_ = float(sub.m_env), float(sub.m)
        flops = me ** 3 / 3 + me * me * ms_ + me * ms_ * ms_
        say(f"n_s = {n_s:5d} (m = {sub.m}, m_env = {sub.m_env}): assembly {t_asm:8.2f}  reduction {t_red:9.2f} "
            f"(potrf {phases['subsystem_potrf']:9.2f}, substitution {phases['subsystem_trsm']:9.2f}, product + mirror "
            f"{phases['subsystem_syrk']:8.2f}; {flops / t_red / 1e9:5.2f} TFLOP/s)  eigensolve {t_all - t_asm - t_red:9.2f}  "
            f"whole solve {t_all:9.2f}")
        orders.append(sub.m_env)
        del sub, hss
    say()

    if not args.no_eigh:
        n = orders[-1]
        say("## 4. sc_dev_eigh_f64 (values and vectors) on a matrix of H_ee's order, the other route to H_ee^-1")
        a = spd(n)
        work, w, v = torch.empty_like(a), torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty_like(a)

        def run():
            work.copy_(a)
            ctx.check(L.sc_dev_eigh_f64(ctx.handle, p(work), n, 1, p(w), p(v)))

        say(f"n = {n}: {timed(run, repeat=1):10.2f} ms")
        ctx.synchronize()
    say()
    for name in ("chase_timeouts", "panel_coop_timeouts", "resident_lost_waits"):
        say(f"# context counter {name} = {ctx.counter(name)}")
    os.makedirs(dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
