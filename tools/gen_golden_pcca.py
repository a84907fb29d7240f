#!/usr/bin/env python3
"""Capture golden vectors of the reference's ``align_posterior_rotation`` (``cca_zoo/probabilistic/_utils.py:112-164``),
the generalised-Procrustes alignment that ``ProbabilisticCCA.fit`` applies to its draws.  The function is pure NumPy, so
it runs without numpyro; its module is loaded by path, which keeps the package's optional imports out of the way.

Two cases, each ``tests/golden/pcca_align_<case>.npz`` with the input draws, the aligned draws and the rotations:

* ``k3``: 7 draws of a (9, 3) loading matrix, each a fixed matrix times a random rotation of its own plus small noise;
* ``k1``: 6 draws of a (5, 1) loading vector with the signs + - + - - +  (a rotation of a one-dimensional latent space is a
  sign).

    python tools/gen_golden_pcca.py
"""

from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
REF = "/root/reference"
if not os.path.isdir(REF):
    sys.exit("reference not mounted; goldens can only be regenerated in the build container")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")

_spec = importlib.util.spec_from_file_location("ref_prob_utils", os.path.join(REF, "cca_zoo", "probabilistic", "_utils.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)


def main():
    rng = np.random.default_rng(20)
    base = rng.standard_normal((9, 3))
    draws = []
    for _ in range(7):
        rot, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        draws.append(base @ rot + 0.05 * rng.standard_normal((9, 3)))
    vec = rng.standard_normal((5, 1))
    signs = [1, -1, 1, -1, -1, 1]
    cases = {"k3": np.stack(draws), "k1": np.stack([s * vec + 0.05 * rng.standard_normal((5, 1)) for s in signs])}
    for name, w in cases.items():
        aligned, rotations = ref.align_posterior_rotation(w)
        path = os.path.join(OUT, f"pcca_align_{name}.npz")
        np.savez(path, w_samples=w, aligned=aligned, rotations=rotations)
        print(f"{os.path.relpath(path, ROOT)}: {w.shape} -> rotations {rotations.shape}")


if __name__ == "__main__":
    main()
