"""
Timings of ensemble NMA on a common core (stream events), written to profiles/subsystem_batch.txt:

    python tools/subsystem_batch_timing.py [--out profiles/subsystem_batch.txt] [--quick] [--test-log LOG]

B = 64 members of N = 1000 +- 10 % atoms (``subsystem_model.synthetic_coord``), a common core of n_s = 800 atoms,
InvariantForceField(13):

  1. SubsystemBatch: assembly, reduction (factorisation, substitution, product + mirror: the context's phase timers) and
     eigensolve separately, and the flops of the padded reduction beside those of the members' own orders.
  2. The whole SubsystemBatch.solve() against 64 successive Subsystem.solve() calls on the same members, the only other way
     to the same result.

``--test-log``: the output of ``pytest tests/test_subsystem_batch_gpu.py -s``; its "measured / gate" lines are appended.
"""
import argparse
import ctypes as C
import os
import sys
from os.path import abspath, dirname, join

import numpy as np

ROOT = dirname(dirname(abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_coord(n, seed):
    return np.random.RandomState(seed).rand(n, 3) * 5.0 * n ** (1.0 / 3.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=join(ROOT, "profiles", "subsystem_batch.txt"))
    ap.add_argument("--quick", action="store_true", help="a quarter of every size, 8 members")
    ap.add_argument("--test-log", default=None)
    args = ap.parse_args()
    import torch

    import springcraft_amd as sc
    from springcraft_amd import _hip

    L = _hip.lib()
    div = 4 if args.quick else 1
    batch, n_mid, n_s = (8 if args.quick else 64), 1000 // div, 800 // div
    lines = [f"# tools/subsystem_batch_timing.py on {_hip.Context(torch.cuda.current_device()).info()}", ""]

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

    rng = np.random.default_rng(0)
    sizes = rng.integers(int(0.9 * n_mid), int(1.1 * n_mid) + 1, batch)
    coords = [synthetic_coord(int(n), 100 + b) for b, n in enumerate(sizes)]
    systems = [np.random.default_rng(100 + b).choice(int(n), n_s, replace=False) for b, n in enumerate(sizes)]
    ff = sc.InvariantForceField(13.0)

    say(f"## 1. SubsystemBatch, B = {batch}, N = {sizes.min()} .. {sizes.max()}, n_s = {n_s}, InvariantForceField(13): ms per stage")
    s = sc.SubsystemBatch(coords, ff, systems, fit=False)
    s.set_profiling(True)
    s._allocate(s.m, s.m)
    s._reduce_into(s.matrix)
    t_asm = timed(lambda: s._blocks_into(s.matrix, s._hes, s._hee))
    t_red = timed(lambda: s._reduce_into(s.matrix)) - t_asm
    phases = {}
    for name in ("subsystem_potrf", "subsystem_trsm", "subsystem_syrk"):
        ms = C.c_double(0.0)
        L.sc_last_eigh_phase_ms(s.ctx.handle, name.encode(), C.byref(ms))
        phases[name] = ms.value
    s.set_profiling(False)
    t_all = timed(lambda: s.solve(), repeat=2)
    s.finish()
    me, ms_ = float(s.m_env), float(s.m)
    flops = lambda e: e ** 3 / 3 + e * e * ms_ + e * ms_ * ms_   # noqa: E731
    padded = batch * flops(me)
    own = sum(flops(3.0 * e) for e in s.n_env)
    say(f"m = {s.m}, slot order m_env = {s.m_env} (members' own orders {3 * min(s.n_env)} .. {3 * max(s.n_env)}), "
        f"scratch {s.workspace_bytes() / 2 ** 20:.1f} MiB")
    say(f"assembly {t_asm:9.2f}   reduction {t_red:9.2f} (potrf {phases['subsystem_potrf']:8.2f}, substitution "
        f"{phases['subsystem_trsm']:8.2f}, product + mirror {phases['subsystem_syrk']:8.2f}; "
        f"{padded / t_red / 1e9:5.2f} TFLOP/s on the padded flops)   eigensolve {t_all - t_asm - t_red:10.2f}   whole solve {t_all:10.2f}")
    say(f"flops of the reduction: padded {padded:.3e}, the members' own {own:.3e}: the pad costs {padded / own - 1:.1%}")
    say()

    say(f"## 2. the same members through {batch} successive Subsystem.solve() calls")
    singles = [sc.Subsystem(c, ff, sy) for c, sy in zip(coords, systems)]

    def loop():
        for one in singles:
            one.solve()

    def loop_reduce():
        for one in singles:
            one.assemble()

    t_loop = timed(loop, repeat=2)
    t_loop_red = timed(loop_reduce, repeat=2)
    for one in singles:
        one.finish()
    say(f"assembly + reduction {t_loop_red:10.2f} ms   whole solves {t_loop:10.2f} ms")
    say(f"batched / successive: assembly + reduction {(t_asm + t_red) / t_loop_red:.3f}, whole solve {t_all / t_loop:.3f}")
    worst = max(float((s.w[b] - one.w[0]).abs().max() / one.w[0].abs().max()) for b, one in enumerate(singles))
    say(f"max |w_batch - w_single| / max|w| over the members = {worst:.2e}")
    say()

    if args.test_log and os.path.exists(args.test_log):
        say("## 3. measured / gate of tests/test_subsystem_batch_gpu.py")
        for line in open(args.test_log):
            if "measured / gate" in line or "/ bound" in line or "max |got - ref|" in line:
                say(line.strip().lstrip(".").strip())
    os.makedirs(dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
