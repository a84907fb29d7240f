#!/usr/bin/env python3
"""Capture golden vectors of the reference's SCCA_IPLS and ElasticCCA (``cca_zoo/linear/_iterative.py:522-623``,
``:730-831``; regressors ``:938-982``).

Same shims as ``tools/gen_golden_als.py``.  Every case stores its inputs, its parameters (one ``alpha`` / ``l1_ratio`` per
view), the reference's ``weights_`` and their nonzero pattern, and the sweeps per latent dimension, in
``tests/golden/enet_<case>.npz``.  The reference's solver visits coordinates at random, so what these goldens pin down is
its update map, and only where that map is well defined.  A case is rejected (the data seed moves on, then the next
``alpha`` of its grid) when

* scikit-learn emits any ``ConvergenceWarning``;
* an outer delta lies within 1 % of ``tol``;
* at a dimension's last update a coordinate's ``|z|`` lies within 1e-9 (relative to ``max |z|``) of the threshold
  ``n alpha l1_ratio`` (a rounding difference could move it into or out of the support);
* a weight column collapses to zero;
* the restatement's own solver ends a solve on its cap of 1000 sweeps, or the fit takes more than ``BUDGET`` coordinate-descent
  sweeps in all (the GPU tests run every golden three times and are to take a second or so each).

The last line printed is the worst per-column relative error of the float64 restatement (``tests/enet_restatement.py``)
against the reference for each class of cases: ``tol <= 1e-10``, the default ``tol``, float32 views.  The bars of
``tests/test_enet_host.py`` are ten times those numbers.

    python tools/gen_golden_enet.py
"""

from __future__ import annotations

import importlib.metadata as md
import os
import sys
import types
import warnings

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

from sklearn.exceptions import ConvergenceWarning  # noqa: E402

from cca_zoo.linear import _iterative as ref_it  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
sys.path.insert(0, os.path.dirname(OUT))
from conftest import save_npz_parts  # noqa: E402
from enet_restatement import CASES as CLASSES, case_class, col_err, restate  # noqa: E402

os.makedirs(OUT, exist_ok=True)
MODELS = {"SCCA_IPLS": ref_it.SCCA_IPLS, "ElasticCCA": ref_it.ElasticCCA}


class Reject(Exception):
    pass


def views(seed, n, dims, latent=2, noise=0.5, dtype=np.float64):
    """Views sharing a ``latent``-dimensional signal, with offsets so that centring matters."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, latent))
    return [(z @ rng.standard_normal((latent, d)) + noise * rng.standard_normal((n, d)) + rng.uniform(-1, 1, d)).astype(dtype)
            for d in dims]


def fit_recorded(model, params, train):
    """Fit the reference with ``_fit_single`` / ``_update_weight`` wrapped: per dimension the initial vectors and every
    update's (view, z of the coefficients it ended on, threshold, result)."""
    est = MODELS[model](**params)
    m, n = len(train), train[0].shape[0]
    alpha = params["alpha"]
    l1 = params["l1_ratio"]
    dims = []
    orig_single, orig_update = est._fit_single, est._update_weight

    def single(vs, w, d):
        dims.append({"w0": [wi.copy() for wi in w], "updates": []})
        return orig_single(vs, w, d)

    def update(vs, ws, i):
        if model == "SCCA_IPLS":
            t = np.asarray(ref_it._target_score(vs, ws, i), dtype=np.float64)
        else:
            t = sum(np.asarray(vs[j] @ ws[j], dtype=np.float64) for j in range(m))
            nt = np.linalg.norm(t)
            t = t / nt if nt > 1e-12 else t
        out = orig_update(vs, ws, i)
        c = np.asarray(est._regressors[i].coef_, dtype=np.float64).ravel()
        x = np.asarray(vs[i], dtype=np.float64)
        z = x.T @ (t - x @ c) + (x * x).sum(axis=0) * c
        thr = None if l1[i] == 0.0 else n * alpha[i] * l1[i]
        dims[-1]["updates"].append((i, z, thr, np.array(out, copy=True)))
        return out

    est._fit_single, est._update_weight = single, update
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with np.errstate(all="ignore"):
            est.fit(train)
    del est._fit_single, est._update_weight
    nconv = sum(issubclass(w.category, ConvergenceWarning) for w in rec)
    return est, dims, nconv


def check_rules(name, est, dims, m, nconv):
    if nconv:
        raise Reject(f"{name}: scikit-learn emitted {nconv} ConvergenceWarning(s)")
    tol = float(est.tol)
    sweeps = []
    for rec in dims:
        ups = rec["updates"]
        assert len(ups) % m == 0
        prev = rec["w0"]
        for s in range(len(ups) // m):
            cur = [ups[s * m + i][3] for i in range(m)]
            d = max(np.linalg.norm(cur[i] - prev[i]) for i in range(m))
            if tol > 0 and np.isfinite(d) and abs(d - tol) < 0.01 * tol:
                raise Reject(f"{name}: an outer delta {d} is within 1% of tol {tol}")
            prev = cur
        sweeps.append(len(ups) // m)
        for i, z, thr, _ in ups[-m:]:
            if thr is None:
                continue
            if (np.abs(np.abs(z) - thr) / np.abs(z).max()).min() < 1e-9:
                raise Reject(f"{name}: a coordinate lies within 1e-9 of the threshold at the last update of view {i}")
    for i, w in enumerate(est.weights_):
        if np.any(np.linalg.norm(w, axis=0) == 0.0):
            raise Reject(f"{name}: a weight column of view {i} collapsed to zero")
    return sweeps


# name, model, parameters (alpha: one grid entry per attempt, each a number or a per-view list), dims, n, dtype
IPLS_A = [0.05, 0.03, 0.08]
EN_A = [0.02, 0.01, 0.05, 0.005, 0.002, 0.1]
BUDGET = 8000
CASE_DEFS = [
    ("ipls2_tight", "SCCA_IPLS", dict(latent_dimensions=2, l1_ratio=0.7, tol=1e-10, random_state=1), IPLS_A, (12, 9), 60, np.float64),
    ("ipls2", "SCCA_IPLS", dict(latent_dimensions=2, l1_ratio=0.7, random_state=1), IPLS_A, (12, 9), 60, np.float64),
    ("en2_tight", "ElasticCCA", dict(latent_dimensions=2, l1_ratio=0.5, tol=1e-10, random_state=2), EN_A, (12, 9), 60, np.float64),
    ("en2", "ElasticCCA", dict(latent_dimensions=2, l1_ratio=0.5, random_state=2), EN_A, (12, 9), 60, np.float64),
    ("ipls3", "SCCA_IPLS", dict(latent_dimensions=2, l1_ratio=0.6, random_state=3), IPLS_A, (10, 8, 6), 80, np.float64),
    ("en3", "ElasticCCA", dict(latent_dimensions=2, l1_ratio=0.5, random_state=4), EN_A, (10, 8, 6), 80, np.float64),
    ("ipls_lasso_tall", "SCCA_IPLS", dict(latent_dimensions=2, l1_ratio=1.0, tol=1e-10, random_state=5), [0.02, 0.03, 0.05], (12, 9), 60,
     np.float64),
    ("ipls_wide", "SCCA_IPLS", dict(latent_dimensions=2, l1_ratio=0.5, random_state=6), IPLS_A, (300, 200), 40, np.float64),
    ("ipls_perview_ridge", "SCCA_IPLS", dict(latent_dimensions=2, l1_ratio=[0.7, 0.0], tol=1e-10, random_state=7),
     [[0.05, 0.5], [0.03, 1.0], [0.08, 2.0]], (12, 9), 60, np.float64),
    ("en_perview", "ElasticCCA", dict(latent_dimensions=2, l1_ratio=[0.5, 0.3], tol=1e-10, random_state=8),
     [[0.02, 0.05], [0.05, 0.1], [0.01, 0.02], [0.1, 0.05]], (12, 9), 60, np.float64),
    ("ipls_nocenter", "SCCA_IPLS", dict(latent_dimensions=2, center=False, l1_ratio=0.7, tol=1e-10, random_state=9), IPLS_A, (12, 9), 60,
     np.float64),
    ("ipls_f32", "SCCA_IPLS", dict(latent_dimensions=2, l1_ratio=0.7, random_state=10), IPLS_A, (12, 9), 60, np.float32),
    ("en_f32", "ElasticCCA", dict(latent_dimensions=2, l1_ratio=0.5, random_state=11), EN_A, (12, 9), 60, np.float32),
    ("en_maxiter", "ElasticCCA", dict(latent_dimensions=2, l1_ratio=0.5, max_iter=3, random_state=12), EN_A, (12, 9), 60, np.float64),
]


def per_view(x, m):
    return [float(v) for v in x] if isinstance(x, list) else [float(x)] * m


def run_case(name, model, params, dims, n, dtype, seed_shift):
    m = len(dims)
    train = views(sum(name.encode()) + 17 + 1000 * seed_shift, n, dims, dtype=dtype)
    full = dict(center=True, max_iter=500, tol=1e-6)
    full.update(params)
    full["alpha"], full["l1_ratio"] = per_view(full["alpha"], m), per_view(full["l1_ratio"], m)
    est, rec, nconv = fit_recorded(model, full, train)
    sweeps = check_rules(name, est, rec, m, nconv)
    out = {f"X{i}": v for i, v in enumerate(train)}
    out.update({f"W{i}": np.asarray(w, dtype=np.float64) for i, w in enumerate(est.weights_)})
    out.update({f"nz{i}": np.asarray(w) != 0.0 for i, w in enumerate(est.weights_)})
    out["n_iter"] = np.asarray(sweeps, dtype=np.int64)
    out["model"] = np.array(model)
    out["n_views"] = np.int64(m)
    for key in ("latent_dimensions", "max_iter", "random_state"):
        out[key] = np.int64(full[key])
    out["center"] = np.bool_(full["center"])
    out["tol"] = np.float64(full["tol"])
    out["alpha"] = np.asarray(full["alpha"], dtype=np.float64)
    out["l1_ratio"] = np.asarray(full["l1_ratio"], dtype=np.float64)
    W, iters, inner, capped = restate(train, model, **full)
    if capped:
        raise Reject(f"{name}: {capped} solve(s) of the restatement ended on the cap")
    if sum(inner) > BUDGET:
        raise Reject(f"{name}: {sum(inner)} coordinate-descent sweeps exceed the budget of {BUDGET}")
    files = save_npz_parts(os.path.join(OUT, f"enet_{name}.npz"), out)
    assert files == [os.path.join(OUT, f"enet_{name}.npz")], "an elastic-net golden must fit one file"
    err = max(col_err(a, b) for a, b in zip(W, est.weights_))
    same = all(np.array_equal(a != 0.0, np.asarray(b) != 0.0) for a, b in zip(W, est.weights_))
    nnz = [[int(np.count_nonzero(w[:, d])) for d in range(w.shape[1])] for w in est.weights_]
    print(f"{name}: kept alpha={full['alpha']} seed shift={seed_shift} sweeps={sweeps} (restatement {iters}, CD sweeps {inner}, "
          f"capped {capped}) support sizes={nnz} supports identical={same} restatement col err={err:.2e} "
          f"bytes={os.path.getsize(files[0])}", flush=True)
    return err, same


def main():
    worst = {k: 0.0 for k in CLASSES}
    for name, model, params, grid, dims, n, dtype in CASE_DEFS:
        done = False
        for alpha in grid:
            for shift in range(6):
                try:
                    err, same = run_case(name, model, dict(params, alpha=alpha), dims, n, dtype, shift)
                except Reject as e:
                    print("rejected:", e, f"(alpha={alpha}, seed shift={shift})", flush=True)
                    continue
                if not same:
                    raise SystemExit(f"{name}: the restatement's supports differ from the reference's")
                worst[case_class(name)] = max(worst[case_class(name)], err)
                done = True
                break
            if done:
                break
        if not done:
            raise SystemExit(f"{name}: every alpha and data seed was rejected")
    print("worst restatement col err per class: " + ", ".join(f"{k}={v:.2e}" for k, v in worst.items()))


if __name__ == "__main__":
    main()
