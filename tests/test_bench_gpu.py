"""
bench.py end to end on small sizes of every configuration: a plain run and a ``--full`` run with the same arguments.
The full line must hold every field of the plain line with the same meaning plus what only ``--full`` computes, the
parity gates must pass, and both runs must dump the same outputs (the dump is taken before the extra profiled step).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = {"roofline", "rooflines", "phases_ms_profiled_step", "counters", "parity_gates", "cpu_baseline"}

CASES = {
    "c3": ["--n-atoms", "200", "--structures-per-gpu", "4", "--cpu-runs", "1"],
    "c2": ["--n-atoms", "150", "--structures-per-gpu", "4", "--cpu-runs", "1"],
    "c4": ["--structures-per-gpu", "2", "--cpu-runs", "1"],
    # the C5 CPU baseline is one N = 3000 partial solve on the host: parity gates and baseline are left to --full runs
    "c5": ["--n-atoms", "400", "--no-cpu-baseline"],
}


def _bench(tmp_path, name, args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1",
           "--dump-outputs", str(tmp_path / name)] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, f"{' '.join(cmd)} exited {r.returncode}:\n{r.stderr[-3000:]}"
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
@pytest.mark.parametrize("config", sorted(CASES))
def test_full_line_is_a_superset_of_the_plain_line(config, tmp_path):
    args = ["--config", config] + CASES[config]
    plain = _bench(tmp_path, "plain", args)
    full = _bench(tmp_path, "full", args + ["--full"])
    assert not FULL_ONLY & set(plain)
    assert set(full) == set(plain) | FULL_ONLY
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain
    for k in set(plain) - {"value", "ms_per_step", "config"}:
        assert full[k] == plain[k], k
    assert plain["steps"] == 1 and plain["value"] > 0 and plain["ms_per_step"] > 0
    if "--no-cpu-baseline" not in args:
        assert full["parity_gates"]["pass"] and full["cpu_baseline"]["value"] > 0
    files = sorted(os.listdir(tmp_path / "plain"))
    assert files == sorted(os.listdir(tmp_path / "full")) and "eigenvalues.npy" in files
    for f in files:
        assert np.array_equal(np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)), f
