#!/usr/bin/env python3
"""Golden vectors for the bootstrap -> tests/golden/boot_rcca.npz.

The REAL reference estimators (cca_zoo/linear: CCA, rCCA(c=[0.1, 0.3]), PLS; latent_dimensions = 3) are fitted on
``[X1[idx], X2[idx]]`` for 8 resamples ``idx = rng.integers(0, n, size=n)`` of one 60 x (5, 3) problem (two shared latents plus
noise and a column offset), the refit loop that ``cca_zoo_amd.model_selection.bootstrap`` replaces.  Import shims as in
tools/gen_golden_half.py; the reference source never travels, only this data file is committed.

Stored: ``X1``, ``X2`` (float64), ``idx`` (8 x 60 int64), ``seed``, and per model ``<name>/w0`` (8 x 5 x 3), ``<name>/w1``
(8 x 3 x 3) the ``weights_`` and ``<name>/score`` (8 x 3) the per-dimension ``score`` on the resampled rows.

    python tools/gen_golden_boot.py --reference /path/to/the/reference/checkout
"""
import argparse
import importlib.metadata as md
import os
import sys
import types

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reference", required=True, help="checkout of the reference project (the directory that holds cca_zoo/)")
ARGS = ap.parse_args()
sys.dont_write_bytecode = True
if not os.path.isdir(os.path.join(ARGS.reference, "cca_zoo")):
    sys.exit("no cca_zoo/ under --reference; goldens can only be regenerated next to the reference")
sys.path.insert(0, ARGS.reference)
_orig_version = md.version
md.version = lambda name: "0.0.0+oracle" if name == "cca_zoo" else _orig_version(name)
_tl = types.ModuleType("tensorly")
_tl.set_backend = lambda *a, **k: None
_dec = types.ModuleType("tensorly.decomposition")
_dec.parafac = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("tensorly stub"))
_tl.decomposition = _dec
sys.modules["tensorly"] = _tl
sys.modules["tensorly.decomposition"] = _dec

from cca_zoo.linear import CCA, PLS, rCCA  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "boot_rcca.npz")
N, P, B, K, SEED = 60, (5, 3), 8, 3, 20261
MODELS = {
    "cca": lambda: CCA(latent_dimensions=K),
    "rcca": lambda: rCCA(latent_dimensions=K, c=[0.1, 0.3]),
    "pls": lambda: PLS(latent_dimensions=K),
}

rng = np.random.default_rng(SEED)
z = rng.standard_normal((N, 2))
X1, X2 = (z @ rng.standard_normal((2, p)) + 0.7 * rng.standard_normal((N, p)) + rng.standard_normal(p) for p in P)
idx = np.stack([rng.integers(0, N, size=N) for _ in range(B)])
store = {"X1": X1, "X2": X2, "idx": idx, "seed": np.int64(SEED)}
for name, ctor in MODELS.items():
    w0, w1, score = [], [], []
    for ix in idx:
        rows = [X1[ix], X2[ix]]
        model = ctor().fit(rows)
        w0.append(np.asarray(model.weights_[0], dtype=np.float64))
        w1.append(np.asarray(model.weights_[1], dtype=np.float64))
        score.append(np.asarray(model.score(rows), dtype=np.float64))
    store[f"{name}/w0"], store[f"{name}/w1"], store[f"{name}/score"] = np.stack(w0), np.stack(w1), np.stack(score)
    print(f"{name}: w0 {store[f'{name}/w0'].shape}  w1 {store[f'{name}/w1'].shape}  first scores {score[0]}")
np.savez_compressed(OUT, **store)
print(OUT, os.path.getsize(OUT), "bytes")
