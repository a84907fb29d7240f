#!/usr/bin/env python3
"""Capture golden vectors of the reference's ALS models: PLS_ALS, SCCA_PMD, ParkhomenkoCCA, SCCA_Span.

Same shims as ``tools/gen_golden_ey.py``.  Every case stores its inputs, the reference's ``weights_`` and ``means_``,
training and held-out ``transform`` / ``score``, the sweeps taken per latent dimension (``_update_weight`` calls / views)
and the last delta per dimension, in ``tests/golden/als_<case>.npz``.  Two rules reject a case:

* stop margin: a sweep whose delta lies within 1 % of ``tol`` (a rounding difference could move the stop by a sweep);
* support: at a dimension's last update, an entry with ``||raw_j| - threshold| / max|raw| < 1e-9`` (a rounding
  difference could move it into or out of the support).  Entries of SCCA_Span that EQUAL the threshold are the selected
  order statistic and its exact ties; they are kept by ``>=`` on either side and do not count.

    python tools/gen_golden_als.py
"""

from __future__ import annotations

import importlib.metadata as md
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

from cca_zoo.linear import _iterative as ref_it  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
sys.path.insert(0, os.path.dirname(OUT))
from conftest import save_npz_parts  # noqa: E402
os.makedirs(OUT, exist_ok=True)

MODELS = {"PLS_ALS": ref_it.PLS_ALS, "SCCA_PMD": ref_it.SCCA_PMD, "ParkhomenkoCCA": ref_it.ParkhomenkoCCA,
          "SCCA_Span": ref_it.SCCA_Span}


class Reject(Exception):
    pass


def views(seed, n, dims, latent=2, noise=0.5, dtype=np.float64, scale=1.0, sparse=0):
    """Views sharing a ``latent``-dimensional signal (+ offsets, so that centring matters), times ``scale``.
    ``sparse`` > 0: only that many features per view and component carry the signal."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, latent))
    out = []
    for d in dims:
        A = rng.standard_normal((latent, d))
        if sparse:
            mask = np.zeros((latent, d))
            for a in range(latent):
                mask[a, rng.choice(d, min(sparse, d), replace=False)] = 1.0
            A = 3.0 * A * mask
        x = z @ A + noise * rng.standard_normal((n, d)) + rng.uniform(-1, 1, d)
        out.append((scale * x).astype(dtype))
    return out


def threshold_of(model, est, raw, i):
    """The level the reference's update of view ``i`` thresholds ``raw`` at (None: none), from its own parameters."""
    a = np.abs(raw)
    if model == "SCCA_PMD":
        bound = est._l1_bounds[i]
        if np.linalg.norm(raw, 1) <= bound:
            return None
        lo, hi = 0.0, a.max()
        for _ in range(50):
            mid = (lo + hi) / 2.0
            if np.linalg.norm(np.sign(raw) * np.maximum(a - mid, 0.0), 1) > bound:
                lo = mid
            else:
                hi = mid
        return (lo + hi) / 2.0
    if model == "ParkhomenkoCCA":
        return float(est._tau_vals[i])
    if model == "SCCA_Span" and est._spans[i] < len(raw):
        return float(np.sort(a)[-est._spans[i]])
    return None


def fit_recorded(model, params, train):
    """Fit the reference with ``_fit_single`` / ``_update_weight`` wrapped: per dimension the initial vectors and every
    update's (view, raw, threshold, result)."""
    est = MODELS[model](**params)
    dims = []
    orig_single, orig_update = est._fit_single, est._update_weight

    def single(vs, w, d):
        dims.append({"w0": [wi.copy() for wi in w], "updates": []})
        return orig_single(vs, w, d)

    def update(vs, ws, i):
        raw = np.asarray(vs[i].T @ ref_it._target_score(vs, ws, i))
        out = orig_update(vs, ws, i)
        dims[-1]["updates"].append((i, raw, threshold_of(model, est, raw, i), np.array(out, copy=True)))
        return out

    est._fit_single, est._update_weight = single, update
    with np.errstate(all="ignore"):
        est.fit(train)
    del est._fit_single, est._update_weight
    return est, dims


def check_rules(name, model, est, dims, m):
    tol = float(est.tol)
    sweeps, last = [], []
    for rec in dims:
        ups = rec["updates"]
        assert len(ups) % m == 0
        prev = rec["w0"]
        deltas = []
        for s in range(len(ups) // m):
            cur = [ups[s * m + i][3] for i in range(m)]
            deltas.append(max(np.linalg.norm(cur[i] - prev[i]) for i in range(m)))
            prev = cur
        for d in deltas:
            if tol > 0 and np.isfinite(d) and abs(d - tol) < 0.01 * tol:
                raise Reject(f"{name}: a stop margin {d} is within 1% of tol {tol}")
        sweeps.append(len(deltas))
        last.append(deltas[-1])
        for i, raw, thr, _ in ups[-m:]:
            if thr is None:
                continue
            gap = np.abs(np.abs(raw) - thr)
            if model == "SCCA_Span":
                gap = gap[np.abs(raw) != thr]
            if gap.size and gap.min() / np.abs(raw).max() < 1e-9:
                raise Reject(f"{name}: an entry lies within 1e-9 of the threshold at the last update of view {i}")
    return sweeps, last


def save_case(name, model, params, est, train, test, sweeps, last):
    out = {f"X{i}": v for i, v in enumerate(train)}
    out.update({f"T{i}": v for i, v in enumerate(test)})
    out.update({f"W{i}": w for i, w in enumerate(est.weights_)})
    out.update({f"mean{i}": mu for i, mu in enumerate(est.means_)})
    out.update({f"Z{i}": z for i, z in enumerate(est.transform(train))})
    out.update({f"Zt{i}": z for i, z in enumerate(est.transform(test))})
    out["score"] = np.asarray(est.score(train))
    out["score_test"] = np.asarray(est.score(test))
    out["n_iter"] = np.asarray(sweeps, dtype=np.int64)
    out["last_delta"] = np.asarray(last, dtype=np.float64)
    out["model"] = np.array(model)
    out["params"] = np.array(repr(sorted(params.items())))
    out["n_views"] = np.int64(len(train))
    files = save_npz_parts(os.path.join(OUT, f"als_{name}.npz"), out)
    assert files == [os.path.join(OUT, f"als_{name}.npz")], "an ALS golden must fit one file"
    nnz = [[int(np.count_nonzero(w[:, d])) for d in range(w.shape[1])] for w in est.weights_]
    print(f"{name}: sweeps={sweeps} last delta={[f'{d:.2e}' for d in last]} support sizes={nnz} "
          f"bytes={os.path.getsize(files[0])}")


# name, model, params, dims, n, dtype, data options
CASES = [
    ("pls2", "PLS_ALS", dict(latent_dimensions=2, random_state=1), (12, 9), 60, np.float64, {}),
    ("pls3", "PLS_ALS", dict(latent_dimensions=3, random_state=2), (10, 8, 6), 80, np.float64, dict(latent=3)),
    ("pls_maxiter", "PLS_ALS", dict(latent_dimensions=2, max_iter=3, random_state=3), (9, 7), 50, np.float64, {}),
    ("pls_f32_nocenter", "PLS_ALS", dict(latent_dimensions=2, center=False, random_state=4), (11, 6), 70, np.float32, {}),
    ("pmd2", "SCCA_PMD", dict(latent_dimensions=2, tau=0.5, random_state=5), (30, 24), 80, np.float64,
     dict(scale=0.05, sparse=4)),
    ("pmd3_perview", "SCCA_PMD", dict(latent_dimensions=2, tau=[0.4, 0.6, 0.5], random_state=6), (20, 16, 12), 80,
     np.float64, dict(scale=0.02, sparse=4)),
    ("pmd_wide_f32", "SCCA_PMD", dict(latent_dimensions=2, tau=0.3, random_state=7), (1200, 900), 40, np.float32,
     dict(scale=0.05, sparse=8)),
    ("pmd_nothr", "SCCA_PMD", dict(latent_dimensions=2, tau=1.0, random_state=8), (14, 10), 60, np.float64,
     dict(scale=0.01)),
    ("pmd_unscaled", "SCCA_PMD", dict(latent_dimensions=2, tau=0.5, random_state=9), (14, 10), 60, np.float64, {}),
    ("park2", "ParkhomenkoCCA", dict(latent_dimensions=2, tau=0.1, random_state=10), (20, 15), 80, np.float64,
     dict(scale=0.05, sparse=4)),
    ("park_f32_perview", "ParkhomenkoCCA", dict(latent_dimensions=3, tau=[0.05, 0.15], random_state=11), (18, 14), 90,
     np.float32, dict(scale=0.05, sparse=4, latent=3)),
    ("park_nocenter", "ParkhomenkoCCA", dict(latent_dimensions=2, center=False, tau=0.05, random_state=12), (16, 12), 70,
     np.float64, dict(scale=0.05, sparse=4)),
    ("span2", "SCCA_Span", dict(latent_dimensions=2, span=[5, 4], random_state=13), (20, 15), 80, np.float64,
     dict(sparse=4)),
    ("span_all", "SCCA_Span", dict(latent_dimensions=2, random_state=14), (8, 12), 60, np.float64, {}),
    ("span_wide_f32", "SCCA_Span", dict(latent_dimensions=2, span=10, random_state=15), (700, 500), 40, np.float32,
     dict(sparse=6)),
]


def run_case(name, model, params, dims, n, dtype, opts, seed_shift=0):
    data = views(sum(name.encode()) + 17 + 1000 * seed_shift, n + 30, dims, dtype=dtype, **opts)
    train = [v[:n] for v in data]
    test = [v[n:] for v in data]
    est, rec = fit_recorded(model, params, train)
    sweeps, last = check_rules(name, model, est, rec, len(dims))
    save_case(name, model, params, est, train, test, sweeps, last)


def run_tie_case():
    """SCCA_Span with a tie at the threshold: view 0 holds one column twice, once negated, so that the two entries of
    ``raw`` agree in magnitude bit for bit; ``span`` is searched until, at the last update of some dimension, the pair
    sits exactly at the s-th largest magnitude and both entries are kept (support s + 1)."""
    name, dims, n = "span_tie", (16, 12), 70
    for shift in range(20):
        data = views(sum(name.encode()) + 17 + 1000 * shift, n + 30, dims, sparse=5)
        data[0][:, 11] = -data[0][:, 3]
        train = [v[:n] for v in data]
        test = [v[n:] for v in data]
        for s in range(2, 12):
            params = dict(latent_dimensions=2, span=s, random_state=16)
            est, rec = fit_recorded("SCCA_Span", params, train)
            tied = False
            for r in rec:
                i, raw, thr, out = r["updates"][-2]          # view 0's last update
                assert i == 0
                a = np.abs(raw)
                tied = tied or (a[3] == a[11] and a[3] == thr and np.count_nonzero(out) == s + 1)
            if not tied:
                continue
            try:
                sweeps, last = check_rules(name, "SCCA_Span", est, rec, 2)
            except Reject:
                continue
            save_case(name, "SCCA_Span", params, est, train, test, sweeps, last)
            return
    raise SystemExit("span_tie: no data seed / span gives a tie at the threshold")


def main():
    for case in CASES:
        for shift in range(20):
            try:
                run_case(*case, seed_shift=shift)
                break
            except Reject as e:
                print("rejected:", e, "-- moving the data seed")
        else:
            raise SystemExit(f"{case[0]}: every data seed was rejected")
    run_tie_case()


if __name__ == "__main__":
    main()
