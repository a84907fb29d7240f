#!/usr/bin/env python3
"""Capture golden vectors of the reference's KCCA / KGCCA (runs only in the build container).

Same shims as ``tools/gen_golden.py`` (metadata version patch, tensorly stub).  Every case stores its inputs, the
reference's weights, means, training and held-out transforms, scores, pairwise correlations, factor loadings and the
dtypes of those outputs in ``tests/golden/kernel_cca_<case>.npz``.  The reference source never travels; only these
data files are committed.

    python tools/gen_golden_kernel.py
"""

from __future__ import annotations

import importlib.metadata as md
import json
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
REF = "/root/reference"
if not os.path.isdir(REF):
    sys.exit("reference not mounted; goldens can only be regenerated in the build container")
sys.path.insert(0, REF)
_orig_version = md.version
md.version = lambda name: "0.0.0+oracle" if name == "cca_zoo" else _orig_version(name)
_tl = types.ModuleType("tensorly")
_tl.set_backend = lambda *a, **k: None
_dec = types.ModuleType("tensorly.decomposition")


def _nope(*a, **k):
    raise RuntimeError("tensorly stub")


_dec.parafac = _nope
_tl.decomposition = _dec
sys.modules["tensorly"] = _tl
sys.modules["tensorly.decomposition"] = _dec

from cca_zoo.nonparametric import KCCA, KGCCA  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
sys.path.insert(0, os.path.dirname(OUT))
from conftest import save_npz_parts  # noqa: E402
os.makedirs(OUT, exist_ok=True)


def views(seed, n, dims, latent=2, noise=0.5, dtype=np.float64):
    """Views sharing a ``latent``-dimensional signal (+ offsets, so that centring matters)."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, latent))
    out = []
    for d in dims:
        A = rng.standard_normal((latent, d))
        x = np.tanh(z @ A) + noise * rng.standard_normal((n, d)) + rng.uniform(-1, 1, d)
        out.append(x.astype(dtype))
    return out


#: case -> (estimator, constructor kwargs, seed, n_train, n_test, dims, dtype)
CASES = {
    "kcca_linear": ("KCCA", dict(latent_dimensions=2, kernel="linear"), 0, 240, 60, [12, 10], np.float64),
    "kcca_poly": ("KCCA", dict(latent_dimensions=2, kernel="poly"), 1, 240, 60, [12, 10], np.float64),
    "kcca_rbf": ("KCCA", dict(latent_dimensions=3, kernel="rbf"), 2, 240, 60, [12, 10], np.float64),
    "kcca_sigmoid": ("KCCA", dict(latent_dimensions=2, kernel="sigmoid"), 3, 240, 60, [12, 10], np.float64),
    "kcca_cosine": ("KCCA", dict(latent_dimensions=2, kernel="cosine"), 4, 240, 60, [12, 10], np.float64),
    "kcca_perview": ("KCCA", dict(latent_dimensions=2, kernel=["linear", "rbf"]), 5, 240, 60, [12, 10], np.float64),
    "kcca_3views": ("KCCA", dict(latent_dimensions=2, kernel="rbf"), 6, 200, 50, [8, 10, 6], np.float64),
    "kcca_nocenter": ("KCCA", dict(latent_dimensions=2, kernel="rbf", center=False), 7, 240, 60, [12, 10], np.float64),
    "kcca_f32": ("KCCA", dict(latent_dimensions=2, kernel="rbf"), 8, 240, 60, [12, 10], np.float32),
    "kcca_params": ("KCCA", dict(latent_dimensions=2, kernel="poly", gamma=0.05, degree=2.0, coef0=0.5), 9, 240, 60,
                    [12, 10], np.float64),
    "kcca_c1e-4": ("KCCA", dict(latent_dimensions=2, kernel="rbf", c=1e-4), 10, 240, 60, [12, 10], np.float64),
    "kcca_c10": ("KCCA", dict(latent_dimensions=2, kernel="rbf", c=10.0), 11, 240, 60, [12, 10], np.float64),
    "kgcca_rbf2": ("KGCCA", dict(latent_dimensions=2, kernel="rbf"), 12, 240, 60, [12, 10], np.float64),
    "kgcca_rbf3": ("KGCCA", dict(latent_dimensions=2, kernel="rbf"), 13, 200, 50, [8, 10, 6], np.float64),
    "kgcca_vw": ("KGCCA", dict(latent_dimensions=2, kernel="rbf", view_weights=[1.0, 0.25]), 14, 240, 60, [12, 10],
                 np.float64),
    "kgcca_linear_full": ("KGCCA", dict(latent_dimensions=2, kernel="linear", c=1.0), 15, 200, 50, [240, 220], np.float64),
}


def main():
    for case, (est, kw, seed, n, nt, dims, dt) in CASES.items():
        allv = views(seed, n + nt, dims, dtype=dt)
        train = [v[:n] for v in allv]
        test = [v[n:] for v in allv]
        model = (KCCA if est == "KCCA" else KGCCA)(**kw).fit(train)
        store = {"params": np.array(json.dumps({"estimator": est, **kw}))}
        for i, (a, b) in enumerate(zip(train, test)):
            store[f"train{i}"], store[f"test{i}"] = a, b
        for i, w in enumerate(model.weights_):
            store[f"w{i}"] = np.asarray(w)
        for i, mu in enumerate(model.means_):
            store[f"mean{i}"] = np.asarray(mu)
        zt, zs = model.transform(train), model.transform(test)
        for i, (a, b) in enumerate(zip(zt, zs)):
            store[f"transform_train{i}"], store[f"transform_test{i}"] = a, b
        store["score_train"] = model.score(train)
        store["score_test"] = model.score(test)
        store["pairwise_train"] = model.pairwise_correlations(train)
        for i, l in enumerate(model.get_factor_loadings(train)):
            store[f"loadings{i}"] = l
        store["dtypes"] = np.array(json.dumps({"weights": str(model.weights_[0].dtype), "means": str(model.means_[0].dtype),
                                               "transform": str(zt[0].dtype), "score": str(store["score_train"].dtype)}))
        save_npz_parts(os.path.join(OUT, f"kernel_cca_{case}.npz"), store)
        print(case, len(store), "arrays", json.loads(str(store["dtypes"])))


if __name__ == "__main__":
    main()
