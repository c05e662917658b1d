"""
Gates and timings of the conformational-ensemble feature (springcraft_amd.ensemble) for profiles/ensemble.txt.  Needs an
MI355X; reads nothing but the package and tests/ensemble_model.py.

    python tools/ensemble_timing.py [--out profiles/ensemble.txt] [--repeat 5] [--skip-large]

  * the specification's float64 error against longdouble (the constants of tests/ensemble_model.py), the resulting gates
    and what the device shows against the float64 specification on the same inputs
  * superposition at M x N = 10^4 x 2000 (LDS form) and 200 x 50 000 (streaming form) from stream events, median of
    --repeat runs after one warm-up, against the byte model: one read + one write of the frames at the device-to-device
    copy rate profiles/subspace.txt records
  * the PCA phases (product, eigensolve, expansion; the context's phase timers) at M = 1000 and M = 10^4 for N = 2000,
    20 components
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import springcraft_amd as sc  # noqa: E402
from tests import ensemble_model as em  # noqa: E402

COPY_TBS = 5.12     # profiles/subspace.txt: device-to-device copy of 1 GiB, read + written


def median(xs):
    return float(np.median(np.asarray(xs)))


def gates_section(lines):
    lines.append("# superposition: |device - float64 specification| / gate (gate = max(8 x |float64 - longdouble|, N eps scale))")
    lines.append("#   case      N    M     fitted               R                    rmsd")
    cases = [(n, n, 65, None) for n in em.SUPERPOSE_ATOMS] + [(n, n, em.LIMIT_FRAMES, None) for n in em.LIMIT_ATOMS]
    cases += [("weights", 65, 65, "weights"), ("mirror", 65, 3, "mirror")]
    for case, n, m, kind in cases:
        fixed, frames = em.rotated_ensemble(n, m)
        w = em.atom_weights(n) if kind == "weights" else None
        if kind == "mirror":
            frames = frames * np.array([-1.0, 1.0, 1.0])
        s_rot, _, s_fit, s_rmsd = em.horn_frames(fixed, frames, w)
        fit, rmsd, (rot, _) = sc.superimpose(fixed, frames, weights=w, return_transform=True)
        g_fit, g_rot, g_rmsd = em.superpose_gates(case, n, float(np.abs(fixed - fixed.mean(axis=0)).max()))
        r = "not unique" if g_rot is None else f"{np.abs(rot - s_rot).max():.2e} / {g_rot:.2e}"
        lines.append(f"  {str(case):>8} {n:5d} {m:4d}   {np.abs(fit - s_fit).max():.2e} / {g_fit:.2e}   {r:>19}   "
                     f"{np.abs(rmsd - s_rmsd).max():.2e} / {g_rmsd:.2e}")
    lines.append("# recorded |float64 - longdouble| of the specification (fitted, R, rmsd): tests/ensemble_model.py SPEC_ERR_SUPERPOSE")
    for case, err in em.SPEC_ERR_SUPERPOSE.items():
        lines.append(f"  {str(case):>8}   {err}")
    lines.append("# PCA of the designed spectrum: |variance - eigvalsh| / gate, 1 - |<v, v_spec>| / gate")
    for m, n in em.PCA_CASES:
        frames, var, _ = em.designed_ensemble(m, n)
        ed = sc.Ensemble(frames).pca(len(var))
        _, v = ed.finish()
        s_var, s_comp, _ = em.pca(frames, len(var))
        g_var, g_comp = em.pca_gates(("designed", m, n), m, n, float(s_var[0]))
        lap = np.linalg.eigvalsh(em.covariance(frames))[::-1][:len(var)]
        cos = np.abs((v.cpu().numpy()[0] * s_comp).sum(axis=1))
        lines.append(f"  M = {m:3d} N = {n:3d} ({'Gram' if m - 1 < 3 * n else 'covariance'}):   "
                     f"{np.abs(ed.variances.cpu().numpy() - lap).max():.2e} / {g_var:.2e}   {(1 - cos).max():.2e} / {g_comp:.2e}")
    lines.append("# recorded |float64 - longdouble| (variance, 1 - |cos|): tests/ensemble_model.py SPEC_ERR_PCA")
    for case, err in em.SPEC_ERR_PCA.items():
        lines.append(f"  {case}   {err}")
    lines.append(f"# iterative fit, mean of perturbed_ensemble(65, 9): recorded {em.SPEC_ERR_ITER_MEAN}")


def random_frames(torch, m, n, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    base = torch.rand((n, 3), generator=g, device="cuda", dtype=torch.float64) * 5 * n ** (1 / 3)
    return base[None] + 0.25 * torch.randn((m, n, 3), generator=g, device="cuda", dtype=torch.float64)


def time_superpose(torch, m, n, repeat, lines):
    ens = sc.Ensemble(random_frames(torch, m, n))
    target = ens.frames[0].clone()
    rmsd = ens._empty((m,))
    form = sc._hip.lib().sc_superpose_form(n)
    times = []
    for it in range(repeat + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ens._fit(target, ens.frames, rmsd)
        b.record()
        torch.cuda.synchronize()
        if it:
            times.append(a.elapsed_time(b))
    ms = median(times)
    model_ms = 2 * 24.0 * n * m / (COPY_TBS * 1e12) * 1e3
    moved = (2 if form == 0 else 4) * 24.0 * n * m
    lines.append(f"  M = {m:6d} N = {n:6d} ({'LDS' if form == 0 else 'streaming'} form): {ms:8.3f} ms, byte model (one read + one "
                 f"write at {COPY_TBS} TB/s) {model_ms:.3f} ms: {ms / model_ms:.2f} x the model; the form moves "
                 f"{moved / 1e9:.2f} GB, {moved / ms / 1e9:.2f} TB/s")


def time_pca(torch, m, n, k, repeat, lines):
    ens = sc.Ensemble(random_frames(torch, m, n, seed=1))
    ens.superpose(reference=0)
    L, h = sc._hip.lib(), ens.ctx.handle
    ens.ctx.check(L.sc_ctx_set_profiling(h, 1))
    rows = []
    for it in range(repeat + 1):
        ed = ens.pca(k)
        ed.finish()
        ms = []
        for name in (b"pca_product", b"pca_eigh", b"pca_expand"):
            v = ctypes.c_double(0.0)
            ens.ctx.check(L.sc_last_eigh_phase_ms(h, name, ctypes.byref(v)))
            ms.append(v.value)
        if it:
            rows.append(ms)
    ens.ctx.check(L.sc_ctx_set_profiling(h, 0))
    p, e, x = (median([r[i] for r in rows]) for i in range(3))
    route = "Gram, order M" if m - 1 < 3 * n else "covariance, order 3N"
    flops = 2.0 * (m * m * 3 * n if m - 1 < 3 * n else 9.0 * n * n * m)
    lines.append(f"  M = {m:6d} N = {n} k = {k} ({route}): centring + product {p:9.3f} ms ({flops / p / 1e9:.1f} TFLOP/s of the full "
                 f"product), eigensolve {e:9.3f} ms, expansion + normalisation {x:8.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble.txt"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    import torch

    lines = [f"# tools/ensemble_timing.py on {sc._hip.context().info()}"]
    gates_section(lines)
    lines.append("# superposition, stream events, median of %d runs after one warm-up" % args.repeat)
    time_superpose(torch, 1000, 2000, args.repeat, lines)
    if not args.skip_large:
        time_superpose(torch, 10000, 2000, args.repeat, lines)
        time_superpose(torch, 200, 50000, args.repeat, lines)
    lines.append("# PCA phases (the context's phase timers), median of %d runs after one warm-up" % args.repeat)
    time_pca(torch, 1000, 2000, 20, args.repeat, lines)
    if not args.skip_large:
        time_pca(torch, 10000, 2000, 20, args.repeat, lines)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
