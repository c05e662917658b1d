"""
Cost of DeviceBatchSolver.linear_response() (q = 1 and q = 4) and mode_displacement() (q = 1 and q = 4) against
mean_square_fluctuation() of the SAME solver and the SAME selection; keep the output as profiles/mode_response.txt.

  64 x N = 2000 ANM, full spectrum, all modes the covariance rule selects (5994 of 6000 rows)
  4 x N = 1000 ANM, full spectrum

The MSF reads the selected rows of v once (nsel x m x 8 bytes per structure).  The response reads them twice per group of
four forces -- once along the rows for the coefficients, once across them for the sum -- and mode_displacement once, so
the expectation to confirm or refute is: response about twice the MSF pass for q <= 4, mode_displacement about once.
The MSF is timed through the C entry with the pinv selection the response uses, on a preallocated output.  Device events
on the solver's stream around --reps back-to-back calls, --runs times after a warm-up, the consumers alternating run by
run; median and every run are printed, with the bytes of v per second.  No pass / fail.

--model N times nma.linear_response of ONE model of N atoms instead (wall clock of the call, host copies included; the
first call also solves and is reported apart); with --covariance-route it times ``anm.covariance @ force`` on a fresh
model, which is what nma.linear_response did before the mode-space kernels (pinv on the device, the (3N, 3N) matrix to
the host, the product in NumPy).

Usage: python tools/response_timing.py [--structures B] [--reps R] [--runs K] [--skip-full] | --model N [--covariance-route]
"""
import argparse
import ctypes as C
import json
import sys
import time
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


def case(torch, label, n_atoms, batch, reps, runs):
    s = DeviceBatchSolver(n_atoms, batch, sc.InvariantForceField(13.0))
    s.solve(torch.from_numpy(np.stack([coord_of(n_atoms, b) for b in range(batch)])).cuda())
    s.finish()
    nvec, m = s.w.shape[1], s.m
    gen = torch.Generator(device=s.device).manual_seed(1)
    f4 = torch.randn((batch, 4, n_atoms, 3), dtype=torch.float64, device=s.device, generator=gen)
    f1 = f4[:, 0].contiguous()
    c4 = torch.randn((batch, 4, nvec), dtype=torch.float64, device=s.device, generator=gen)
    c1 = c4[:, 0].contiguous()
    # what is timed is right: structure 0 against torch on the solver's own eigenpairs
    w0 = s.w[0]
    keep = w0.abs() > 1e-6 * w0.abs().max()
    fm = f4[0].reshape(4, m)
    ref = ((fm @ s.v[0][keep].T) / w0[keep]) @ s.v[0][keep]
    err_r = float((s.linear_response(f4)[0].reshape(4, m) - ref).abs().max() / ref.abs().max())
    ref = c4[0] @ s.v[0]
    err_c = float((s.mode_displacement(c4)[0].reshape(4, m) - ref).abs().max() / ref.abs().max())
    nsel = int(keep.sum())
    del ref, fm
    sel = _hip.ModeSelection()
    sel.kind, sel.rcond = _hip.SC_SEL_PINV, 1e-6
    out = torch.empty((batch, n_atoms), dtype=torch.float64, device=s.device)
    L = _hip.lib()

    def msf():
        s.ctx.check(L.sc_dev_modes_msf_f64(s.ctx.handle, C.c_void_p(s.w.data_ptr()), C.c_void_p(s.v.data_ptr()), m, nvec,
                                           batch, 3, C.byref(sel), None, C.c_void_p(out.data_ptr())))

    names = ["response_q1", "response_q4", "displacement_q1", "displacement_q4", "msf_same_selection"]
    res = alternating_ms(torch, [lambda: s.linear_response(f1), lambda: s.linear_response(f4),
                                 lambda: s.mode_displacement(c1), lambda: s.mode_displacement(c4), msf], reps, runs)
    nbytes = batch * nsel * m * 8
    msf_ms = res[-1][0]
    line = {"case": label, "structures": batch, "rows": nvec, "selected_rows_structure_0": nsel, "m": m,
            "bytes_of_selected_v": nbytes, "rel_err_response_vs_torch": err_r, "rel_err_displacement_vs_torch": err_c}
    for name, (ms, every) in zip(names, res):
        passes = 2 if name.startswith("response") else 1
        tbs = passes * nbytes / (ms * 1e-3) / 1e12
        line.update({f"{name}_ms_median": round(ms, 4), f"{name}_ms_runs": every, f"{name}_passes_over_v": passes,
                     f"{name}_TBps_of_v": round(tbs, 3), f"{name}_share_of_6.3_TBps": round(tbs / HBM_ACHIEVABLE_TBS, 3),
                     f"{name}_over_msf": round(ms / msf_ms, 3)})
    print(json.dumps(line), flush=True)
    del s, out, f1, f4, c1, c4
    torch.cuda.empty_cache()


def one_model(n_atoms, runs, covariance_route):
    anm = sc.ANM(coord_of(n_atoms), sc.InvariantForceField(13.0))
    f = np.random.RandomState(1).randn(n_atoms, 3)
    sc.compute_hessian(coord_of(20), sc.InvariantForceField(13.0))   # (the context and the library are up before the clock)
    t = []
    for _ in range(runs + 1):
        t0 = time.perf_counter()
        # the covariance route is what nma.linear_response did before the mode-space kernels: anm.covariance @ force
        x = (anm.covariance @ f.ravel()).reshape(-1, 3) if covariance_route else sc.nma.linear_response(anm, f)
        t.append((time.perf_counter() - t0) * 1e3)
    route = "covariance route (anm.covariance @ force)" if covariance_route else "nma.linear_response"
    print(json.dumps({"case": f"{route}, one model N = {n_atoms}", "first_call_with_solve_ms": round(t[0], 2),
                      "later_calls_ms": [round(v, 2) for v in t[1:]], "later_calls_ms_median": round(float(np.median(t[1:])), 2),
                      "covariance_on_the_model": anm._covariance is not None, "max_abs_x": float(np.abs(x).max())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=64)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip-full", action="store_true")
    ap.add_argument("--model", type=int, default=0)
    ap.add_argument("--covariance-route", action="store_true")
    args = ap.parse_args()
    print(json.dumps({"device": _hip.context().info(), "cmd": " ".join(sys.argv)}), flush=True)
    if args.model:
        one_model(args.model, args.runs, args.covariance_route)
        return
    import torch

    case(torch, "4 x N=1000, full spectrum", 1000, 4, args.reps * 4, args.runs)
    if not args.skip_full:
        b = args.structures
        case(torch, f"{b} x N=2000, full spectrum", 2000, b, args.reps, args.runs)


if __name__ == "__main__":
    main()
