"""
Every mode consumer of DeviceBatchSolver and RaggedBatchSolver on small fixed inputs, written to one .npz: run it on two
commits and compare the files to show that a change of the layers above the kernels moved no bit
(profiles/consumer_layer_ab.txt).

Solvers: DeviceBatchSolver(20, 3) and RaggedBatchSolver((17, 20, 12)), each as ANM and GNM (InvariantForceField(13.0),
coordinates ``rand(n, 3) * 5 n^(1/3)`` from RandomState(seed), as tests/util.py's synthetic_coord), each solved as the full
spectrum, subset_by_index ((6, 25) ANM, (1, 9) GNM) and subset_by_value with max_modes=12 ((1e-3, 4.0): the trivial modes
stay out).  Per solve: w, v, counts, frequencies, collectivity, overlap (one displacement and q = 2), and for mode_subset
None / an unsorted list with a repeat (not behind a window) and tem unset / 300: mean_square_fluctuation, bfactor,
_aniso_packed and anisotropic_fluctuation (ANM), dcc (norm on / off) and distance_fluctuation (projected on (ANM) / off,
atom_scale unset / set).  A ragged solver's lists are stored per structure.

``--group pair_tile`` dumps instead what runs on the 64 x 64 pair-block MFMA core (csrc/pair_block_tile.h and its copy in
csrc/rmsd_matrix.hip; profiles/pair_block_tile.txt), at the sizes where a tile edge, the diagonal tile, the tail of a group of eight rows and
the pads can go wrong.  ANM batches DeviceBatchSolver(N, 2) of N = 5, 63, 64, 65, 130 and RaggedBatchSolver((30, 70, 130)),
each as a full solve and behind subset_by_index (3, min(3 N, 41) - 1): prs (norm on / off, atom_scale unset / set) and
generalized_correlation (information off / on) for mode_subset None, a list of 3 modes, a list of 9 (one more than a row
group), and an unsorted list with a repeat; nma.prs(mode_subset=...) and generalized_correlation of single ANM models;
Ensemble.rmsd_matrix for M = 1, 63, 64, 65, 130 frames of N = 1, 7, 8, 9, 50 atoms (fit, squared, weights on / off),
against another ensemble (65 x 130) and with a NaN frame.  A call that raises is stored as its message.

Usage: python tools/consumer_dump.py OUT.npz [--group pair_tile]
                                                         write OUT.npz, print its sha256 and a digest of the arrays
       python tools/consumer_dump.py OUT.npz --compare OTHER.npz
                                                         also compare array by array (np.array_equal, NaN equal to NaN);
                                                         exit status 1 if any differs or is missing
The file's sha256 covers the zip container (time stamps included); the digest covers names, dtypes, shapes and bytes.
"""
import argparse
import hashlib
import json
import sys
from os.path import abspath, dirname

import numpy as np

sys.path.insert(0, dirname(dirname(abspath(__file__))))
import springcraft_amd as sc  # noqa: E402
from springcraft_amd.batch import DeviceBatchSolver, RaggedBatchSolver  # noqa: E402

UNIFORM = (20, 3)
RAGGED = (17, 20, 12)
INDEX = {3: (6, 25), 1: (1, 9)}
LIST = {3: [9, 7, 20, 7], 1: [4, 2, 8, 2]}
WINDOW, MAX_MODES = (1e-3, 4.0), 12


def coord_of(n_atoms, seed):
    return np.random.RandomState(seed).rand(n_atoms, 3) * 5.0 * n_atoms ** (1.0 / 3.0)


def dump_solver(torch, out, tag, ragged, dim, spectrum):
    kw = {"full": {}, "index": {"subset_by_index": INDEX[dim]},
          "window": {"subset_by_value": WINDOW, "max_modes": MAX_MODES}}[spectrum]
    ff = sc.InvariantForceField(13.0)
    rs = np.random.RandomState(1234)
    if ragged:
        sizes = list(RAGGED)
        s = RaggedBatchSolver(sizes, ff, dim=dim, **kw)
        x = torch.from_numpy(np.concatenate([coord_of(n, 10 + b) for b, n in enumerate(sizes)])).cuda()
        atoms = (sum(sizes),)
        disp_q = rs.randn(2, *atoms, *((3,) if dim == 3 else ()))
    else:
        n, batch = UNIFORM
        s = DeviceBatchSolver(n, batch, ff, dim=dim, **kw)
        x = torch.from_numpy(np.stack([coord_of(n, 10 + b) for b in range(batch)])).cuda()
        atoms = (batch, n)
        disp_q = rs.randn(batch, 2, n, *((3,) if dim == 3 else ()))
    scale = torch.from_numpy(rs.uniform(0.5, 1.5, atoms)).cuda()
    disp_q = torch.from_numpy(disp_q).cuda()
    disp_1 = (disp_q[0] if ragged else disp_q[:, 0]).contiguous()
    s.solve(x)
    try:
        s.finish()
    except ValueError as e:     # a window holding more than max_modes: the slots keep the lowest, which is what is dumped
        out[f"{tag}.finish_error"] = np.frombuffer(str(e).encode(), dtype=np.uint8)

    def put(name, value):
        if isinstance(value, (list, tuple)):
            for b, t in enumerate(value):
                out[f"{tag}.{name}.{b}"] = t.cpu().numpy()
        else:
            out[f"{tag}.{name}"] = value.cpu().numpy()

    put("w", s.w)
    put("v", s.v)
    if s.counts is not None:
        put("counts", s.counts)
    put("frequencies", s.frequencies())
    put("collectivity", s.collectivity())
    put("overlap_one", s.overlap(disp_1))
    put("overlap_q2", s.overlap(disp_q))
    for sub_name, subset in (("all", None), ("list", LIST[dim])):
        if subset is not None and spectrum == "window":
            continue
        for tem in (None, 300.0):
            t = f"{sub_name}.tem_{'off' if tem is None else 'on'}"
            put(f"msf.{t}", s.mean_square_fluctuation(subset, tem=tem))
            put(f"bfactor.{t}", s.bfactor(subset, tem=tem))
            if dim == 3:
                put(f"aniso_packed.{t}", s._aniso_packed(subset, tem=tem))
                put(f"aniso.{t}", s.anisotropic_fluctuation(subset, tem=tem))
            for norm in (True, False):
                put(f"dcc.{t}.norm_{int(norm)}", s.dcc(subset, norm=norm, tem=tem))
            for projected in ((True, False) if dim == 3 else (False,)):
                for sc_name, a_scale in (("off", None), ("on", scale)):
                    put(f"distfluct.{t}.projected_{int(projected)}.scale_{sc_name}",
                        s.distance_fluctuation(x, subset, projected=projected, atom_scale=a_scale, tem=tem))
    torch.cuda.synchronize()


PT_SIZES = (5, 63, 64, 65, 130)
PT_RAGGED = (30, 70, 130)
PT_LISTS = {"all": None, "three": [7, 12, 9], "nine": [6, 7, 8, 9, 10, 11, 12, 13, 14], "repeat": [13, 7, 10, 7]}
PT_FRAMES, PT_ATOMS = (1, 63, 64, 65, 130), (1, 7, 8, 9, 50)


def attempt(out, name, call):
    """out[name...] <- what call() returns (a tensor, an ndarray or a list of tensors), or the message of its exception."""
    try:
        value = call()
    except Exception as e:  # noqa: BLE001  (both commits must then raise the same)
        out[f"{name}.error"] = np.frombuffer(f"{type(e).__name__}: {e}".encode(), dtype=np.uint8)
        return
    for b, t in enumerate(value) if isinstance(value, (list, tuple)) else ((None, value),):
        out[name if b is None else f"{name}.{b}"] = t if isinstance(t, np.ndarray) else t.cpu().numpy()


def dump_pair_tile_modes(torch, out):
    ff = sc.InvariantForceField(13.0)
    rs = np.random.RandomState(4321)
    for sizes in [(n,) for n in PT_SIZES] + [PT_RAGGED]:
        ragged = len(sizes) > 1
        for windowed in (False, True):
            kw = {"subset_by_index": (3, min(3 * min(sizes), 41) - 1)} if windowed else {}
            tag = f"{'ragged' if ragged else f'uniform{sizes[0]}'}.{'index' if windowed else 'full'}"
            if ragged:
                s = RaggedBatchSolver(list(sizes), ff, **kw)
                x = torch.from_numpy(np.concatenate([coord_of(n, 20 + b) for b, n in enumerate(sizes)])).cuda()
                scale = rs.uniform(0.5, 1.5, (sum(sizes),))
            else:
                s = DeviceBatchSolver(sizes[0], 2, ff, **kw)
                x = torch.from_numpy(np.stack([coord_of(sizes[0], 20 + b) for b in range(2)])).cuda()
                scale = rs.uniform(0.5, 1.5, (2, sizes[0]))
            scale = torch.from_numpy(scale).cuda()
            s.solve(x)
            s.finish()
            for sub_name, subset in PT_LISTS.items():
                for norm in (True, False):
                    for sc_name, a_scale in (("off", None), ("on", scale)):
                        attempt(out, f"{tag}.prs.{sub_name}.norm_{int(norm)}.scale_{sc_name}",
                                lambda: s.prs(subset, norm=norm, atom_scale=a_scale))
                for information in (False, True):
                    attempt(out, f"{tag}.lmi.{sub_name}.information_{int(information)}",
                            lambda: s.generalized_correlation(subset, information=information))
            torch.cuda.synchronize()
    for n in (5, 65):
        anm = sc.ANM(coord_of(n, 40), ff)
        for sub_name, subset in PT_LISTS.items():
            if subset is not None:
                for norm in (True, False):
                    attempt(out, f"model{n}.prs.{sub_name}.norm_{int(norm)}", lambda: sc.nma.prs(anm, norm, subset))
            for information in (False, True):
                attempt(out, f"model{n}.lmi.{sub_name}.information_{int(information)}",
                        lambda: anm.generalized_correlation(subset, information))


def dump_pair_tile_rmsd(torch, out):
    rs = np.random.RandomState(987)
    frames = rs.randn(max(PT_FRAMES), max(PT_ATOMS), 3) * 3.0 + rs.randn(1, max(PT_ATOMS), 3) * 10.0
    other = rs.randn(max(PT_FRAMES), max(PT_ATOMS), 3) * 3.0 + frames[:1]
    weights = rs.uniform(0.5, 2.0, max(PT_ATOMS))

    def put(tag, a, b, w):
        ens = sc.Ensemble(np.ascontiguousarray(a), weights=w)
        oth = None if b is None else sc.Ensemble(np.ascontiguousarray(b), weights=w)
        for fit in (True, False):
            for squared in (True, False):
                attempt(out, f"rmsd.{tag}.fit_{int(fit)}.squared_{int(squared)}.weights_{'off' if w is None else 'on'}",
                        lambda: ens.rmsd_matrix(oth, fit=fit, squared=squared))

    for n in PT_ATOMS:
        for w in (None, weights[:n]):
            for m in PT_FRAMES:
                put(f"m{m}.n{n}", frames[:m, :n], None, w)
            put(f"m65.other130.n{n}", frames[:65, :n], other[:130, :n], w)
            put(f"m130.other63.n{n}", frames[:130, :n], other[:63, :n], w)
    bad = frames[:65, :9].copy()
    bad[3, 4, 1] = np.nan
    for w in (None, weights[:9]):
        put("m65.n9.nan_frame3", bad, None, w)
        put("m65.other130.n9.nan_frame3", bad, other[:130, :9], w)
    torch.cuda.synchronize()


def digest(arrays):
    h = hashlib.sha256()
    for k in sorted(arrays):
        a = np.ascontiguousarray(arrays[k])
        h.update(f"{k}|{a.dtype.str}|{a.shape}|".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--compare", default=None)
    ap.add_argument("--group", choices=("layers", "pair_tile"), default="layers")
    args = ap.parse_args()
    out = {}
    if args.group == "pair_tile":
        dump_pair_tile_modes(torch, out)
        dump_pair_tile_rmsd(torch, out)
    for ragged in (False, True) if args.group == "layers" else ():
        for dim in (3, 1):
            for spectrum in ("full", "index", "window"):
                tag = f"{'ragged' if ragged else 'uniform'}.{'anm' if dim == 3 else 'gnm'}.{spectrum}"
                dump_solver(torch, out, tag, ragged, dim, spectrum)
    np.savez(args.out, **out)
    report = {"file": args.out, "arrays": len(out), "values": int(sum(a.size for a in out.values())),
              "nan_values": int(sum(np.isnan(a).sum() for a in out.values() if a.dtype.kind == "f")),
              "file_sha256": hashlib.sha256(open(args.out, "rb").read()).hexdigest(), "arrays_sha256": digest(out)}
    status = 0
    if args.compare is not None:
        other = dict(np.load(args.compare))
        differ = sorted(k for k in out if k in other and not np.array_equal(out[k], other[k], equal_nan=True))
        missing = sorted(set(out) ^ set(other))
        report.update(compared_with=args.compare, other_file_sha256=hashlib.sha256(open(args.compare, "rb").read()).hexdigest(),
                      other_arrays_sha256=digest(other), arrays_that_differ=differ, arrays_in_one_file_only=missing,
                      all_equal=not differ and not missing)
        status = 0 if report["all_equal"] else 1
    print(json.dumps(report), flush=True)
    return status


if __name__ == "__main__":
    sys.exit(main())
