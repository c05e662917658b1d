"""
Builds libspringcraft_hip.so in-tree for gfx950 with hipcc (cross-compiles without a GPU).

    python springcraft_amd/csrc/build.py [--force] [--verbose]

One object per .hip source (compiled in parallel, rebuilt only when the source or a header
changed), linked into springcraft_amd/libspringcraft_hip.so.  assembly.hip is compiled with
-ffp-contract=off (bit-exact contact predicate, see the file header).

A variant library (diagnostic stamps, an experiment's macro) is built the same way next to the product library:
SC_LIB_SUFFIX=_stamps SC_EXTRA_HIPCC_FLAGS=-DPAIR_STAMPS gives obj_stamps/ and libspringcraft_hip_stamps.so
(tools/build_stamps_lib.sh); select it with SPRINGCRAFT_HIP_LIB.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from os.path import abspath, dirname, exists, getmtime, join

HERE = dirname(abspath(__file__))
PKG = dirname(HERE)
REPO = dirname(PKG)
SUFFIX = os.environ.get("SC_LIB_SUFFIX", "")
OBJ = join(HERE, "obj" + SUFFIX)
LIB = join(PKG, "libspringcraft_hip" + SUFFIX + ".so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

COMMON = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function", "-Werror=return-type",
          "-I", join(REPO, "include")] + os.environ.get("SC_EXTRA_HIPCC_FLAGS", "").split()
PER_FILE = {
    "assembly.hip": ["-ffp-contract=off"],
    # a row's bits must not depend on how the row loop was unrolled: every operation is the one written
    "pair_operator.hip": ["-ffp-contract=off"],
    "pair_panel.hip": ["-ffp-contract=off"],   # (the same promise for a column of a panel)
    "pair_cg.hip": ["-ffp-contract=off"],   # (the panel step's walk and bits, and one rounding per written operation)
    "cluster.hip": ["-ffp-contract=off"],   # (every sum of the k-medoids kernels is the additions written, in their fixed order)
    # k_bt2_apply's diamond loop is 80 fully unrolled steps per half-diamond (every register index must be a constant):
    # above LLVM's default budget for `#pragma unroll`, below which the accumulators would live in scratch memory
    "bt2.hip": ["-mllvm", "-pragma-unroll-threshold=1000000"],
    # (stage 1 was built with the flag while it shared a file with bt2: without it k_panel_wg<10, 1, 512> and <12, 1, 512>
    # come out as other code, so it stays; the other kernels of the file are identical either way)
    "sy2sb.hip": ["-mllvm", "-pragma-unroll-threshold=1000000"],
}


def sources():
    return sorted(f for f in os.listdir(HERE) if f.endswith(".hip") and not f.startswith("_"))


def headers_mtime():
    hs = [join(HERE, f) for f in os.listdir(HERE) if f.endswith(".h")]
    hs.append(join(REPO, "include", "springcraft_hip.h"))
    return max(getmtime(h) for h in hs)


def compile_one(src, force, verbose):
    obj = join(OBJ, src.replace(".hip", ".o"))
    spath = join(HERE, src)
    if not force and exists(obj) and getmtime(obj) > max(getmtime(spath), headers_mtime()):
        return obj, False
    cmd = [HIPCC, "-c", spath, "-o", obj] + COMMON + PER_FILE.get(src, [])
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
    if verbose and r.stderr.strip():
        print(r.stderr)
    return obj, True


def build(force=False, verbose=False):
    os.makedirs(OBJ, exist_ok=True)
    srcs = sources()
    with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        results = list(ex.map(lambda s: compile_one(s, force, verbose), srcs))
    objs = [o for o, _ in results]
    if force or not exists(LIB) or any(changed for _, changed in results):
        cmd = [HIPCC, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    return LIB


if __name__ == "__main__":
    lib = build(force="--force" in sys.argv, verbose="--verbose" in sys.argv or "-v" in sys.argv)
    print(lib)
