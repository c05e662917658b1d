"""
Host LAPACK eigenvalues for tests/test_large_order_gpu.py, written to
``tests/golden/generated/large_order_eigvalsh.npz`` (NumPy and the oracle only; about a minute):

    PYTHONDONTWRITEBYTECODE=1 python oracle/make_large_order_golden.py

  random_7001   np.linalg.eigvalsh(a + a.T), a = RandomState(7001).randn(7001, 7001)
  hinsen_7200   np.linalg.eigvalsh of the oracle's Hessian of synthetic_coord(2400, 24), Hinsen force field
                without cutoff
"""
import os
import sys
from os.path import abspath, dirname, join

import numpy as np

HERE = dirname(abspath(__file__))
REPO = dirname(HERE)
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

from oracle import enm_oracle as orc  # noqa: E402

RANDOM_ORDER, RANDOM_SEED = 7001, 7001
HINSEN_ATOMS, HINSEN_SEED = 2400, 24


def random_matrix():
    a = np.random.RandomState(RANDOM_SEED).randn(RANDOM_ORDER, RANDOM_ORDER)
    return a + a.T


def main():
    h, _ = orc.compute_hessian(orc.synthetic_coord(HINSEN_ATOMS, HINSEN_SEED), orc.hinsen_ff())
    out = join(REPO, "tests", "golden", "generated")
    os.makedirs(out, exist_ok=True)
    np.savez_compressed(join(out, "large_order_eigvalsh.npz"), random_7001=np.linalg.eigvalsh(random_matrix()),
                        hinsen_7200=np.linalg.eigvalsh(h))


if __name__ == "__main__":
    main()
