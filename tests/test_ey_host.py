"""CPU tests of the gradient (Eckart-Young) models: import surface, parameters, the index producer, and a float64
NumPy restatement of the reference's loop checked against every golden (the comparator of tests/test_gpu_ey.py)."""

import glob
import os

import numpy as np
import pytest

from conftest import load_golden

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[3:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "ey_*.npz")))


def case_params(g):
    """Constructor parameters of a golden case (stored as the repr of a sorted item list)."""
    import ast

    return dict(ast.literal_eval(str(g["params"])))


def case_views(g, prefix="X"):
    return [g[f"{prefix}{i}"] for i in range(int(g["n_views"]))]


def restate(views, kind, latent_dimensions=1, center=True, c=0.0, learning_rate=1e-2, max_iter=1000, batch_size=None,
            tol=1e-6, momentum=0.9, random_state=None, n=None, rowmap=None, permute_full=True, trace=None):
    """The reference's fit in float64 NumPy, written from its equations (cca_zoo/linear/gradient/_base.py:101-130,
    _cca_ey.py:183-225, cca_zoo/_utils/_ey.py).  ``views`` are the raw views in their own dtype; centring is the
    reference's ``v - v.mean(axis=0)`` in that dtype.  ``n`` / ``rowmap``: the views hold only some rows of an
    ``n``-row data set (global row ``r`` is ``views[i][rowmap[r]]``) and are already centred.  ``permute_full=False``
    uses the rows in order when the batch is the whole data set (what the device does).  ``trace`` (a list) receives
    (Z list, W list) of every step.  Returns (weights, steps)."""
    xs = [np.asarray(v) for v in views]
    if center and rowmap is None:
        xs = [x - x.mean(axis=0) for x in xs]
    m = len(xs)
    n = xs[0].shape[0] if n is None else n
    rowmap = np.arange(n) if rowmap is None else rowmap
    k = latent_dimensions
    bs = n if batch_size is None else min(batch_size, n)
    rng = np.random.default_rng(random_state)
    if kind == "pls":
        W = [np.linalg.qr(rng.standard_normal((x.shape[1], k)))[0] for x in xs]
        c = 1.0
    else:
        idx = rowmap[rng.choice(n, bs, replace=False)]
        W = []
        for x in xs:
            w0 = np.linalg.qr(rng.standard_normal((x.shape[1], k)))[0]
            r = np.linalg.qr(x[idx] @ w0)[1]
            W.append(w0 @ np.linalg.solve(r, np.eye(k)))
    vel = [np.zeros_like(w) for w in W]
    prev, steps = np.inf, 0
    full = bs == n
    with np.errstate(all="ignore"):
        for _ in range(max_iter):
            if full and not permute_full:
                idx = rowmap[np.arange(n)]
            else:
                idx = rowmap[rng.choice(n, bs, replace=False)]
            Xb = [x[idx] for x in xs]
            Z = [xb @ w for xb, w in zip(Xb, W)]
            Zc = [z - z.mean(axis=0) for z in Z]
            tot = sum(Zc)
            V = sum(zc.T @ zc for zc in Zc) / ((bs - 1) * m)
            Cm = tot.T @ tot / ((bs - 1) * m)
            B = sum(w.T @ w for w in W) / m
            vb = (1 - c) * V + c * B
            scale = 4.0 / (m * (bs - 1))
            for i in range(m):
                zt = scale * (c * Zc[i] + (1 - c) * (Zc[i] @ vb) - tot)
                # the reference re-centres the batch in the views' dtype (its rounding matters for float32 views)
                g = (Xb[i] - Xb[i].mean(axis=0)).T @ zt + (4.0 * c / m) * (W[i] @ vb)
                vel[i] = momentum * vel[i] - learning_rate * g
                W[i] = W[i] + vel[i]
            if trace is not None:
                trace.append(([z.copy() for z in Z], [w.copy() for w in W]))
            B2 = sum(w.T @ w for w in W) / m
            vo = (1 - c) * V + c * B2
            obj = float(-2.0 * np.trace(Cm - c * V) + np.trace(vo @ vo))
            steps += 1
            if abs(prev - obj) < tol:
                break
            prev = obj
    return W, steps


def restate_case(g, **over):
    p = case_params(g)
    p.update(over)
    kind = "pls" if str(g["model"]) == "PLS_EY" else "cca"
    return restate(case_views(g), kind, **p)


def col_err(w, ref):
    """Largest per-column relative error."""
    num = np.linalg.norm(w - ref, axis=0)
    den = np.maximum(np.linalg.norm(ref, axis=0), 1e-300)
    return float(np.max(num / den))


# ---- import surface and parameters --------------------------------------------------------------------------------
def test_import_surface():
    import cca_zoo_amd.linear as lin
    from cca_zoo_amd.linear import CCA_EY, MCCA_EY, PLS_EY
    from cca_zoo_amd.linear.gradient import CCA_EY as A, MCCA_EY as B, PLS_EY as C

    assert (A, B, C) == (CCA_EY, MCCA_EY, PLS_EY)
    assert {"CCA_EY", "PLS_EY", "MCCA_EY"} <= set(lin.__all__)


def test_get_params_parity():
    from cca_zoo_amd.linear import CCA_EY, MCCA_EY, PLS_EY

    common = {"latent_dimensions": 1, "center": True, "learning_rate": 1e-2, "max_iter": 1000, "batch_size": None,
              "tol": 1e-6, "momentum": 0.9, "random_state": None}
    assert CCA_EY().get_params() == {**common, "c": 0.0}
    assert MCCA_EY().get_params() == {**common, "c": 0.0}
    assert PLS_EY().get_params() == common
    assert "c" not in PLS_EY().get_params()
    assert CCA_EY(c=0.4, batch_size=7).get_params()["batch_size"] == 7


def test_parameter_validation_and_new_errors(monkeypatch):
    from cca_zoo_amd import _dist
    from cca_zoo_amd.linear import CCA_EY, MCCA_EY, PLS_EY

    X, Y = np.zeros((20, 3)), np.zeros((20, 4))
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            CCA_EY(c=bad).fit([X, Y])
        with pytest.raises(ValueError):
            MCCA_EY(c=bad).fit([X, Y])
    with pytest.raises(ValueError):
        CCA_EY(latent_dimensions=0).fit([X, Y])
    with pytest.raises(ValueError, match="smallest view width"):
        CCA_EY(latent_dimensions=4).fit([X, Y])
    with pytest.raises(ValueError, match="smallest view width"):
        PLS_EY(latent_dimensions=5).fit([X, Y])
    monkeypatch.setattr(_dist, "is_sharded", lambda: True)
    for cls in (CCA_EY, PLS_EY, MCCA_EY):
        with pytest.raises(NotImplementedError, match="row_sharded"):
            cls().fit([X, Y])


# ---- index producer -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_index_producer_matches_golden_draws(case):
    from cca_zoo_amd.linear.gradient._base import draw_batches, initial_weights

    g = load_golden(f"ey_{case}")
    p = case_params(g)
    views = case_views(g)
    n = views[0].shape[0]
    bs = n if p.get("batch_size") is None else min(p["batch_size"], n)
    rng = np.random.default_rng(p["random_state"])
    kind = "pls" if str(g["model"]) == "PLS_EY" else "cca"
    seen = []

    def project(idx, w0s):
        seen.append(idx)
        return [np.eye(bs, w.shape[1]) + 0.0 for w in w0s]

    initial_weights(kind, [v.shape[1] for v in views], p["latent_dimensions"], n, bs, rng, project)
    seen.extend(draw_batches(rng, n, bs, 3))
    for t in range(3):
        np.testing.assert_array_equal(seen[t], g[f"draw{t}"])


# ---- the restatement reproduces every golden ------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_golden(case):
    g = load_golden(f"ey_{case}")
    W, steps = restate_case(g)
    assert steps == int(g["n_iter"])
    for i, w in enumerate(W):
        ref = g[f"W{i}"]
        if not np.all(np.isfinite(ref)):
            assert not np.all(np.isfinite(w))
            continue
        assert col_err(w, ref) <= 1e-10, (case, i, col_err(w, ref))


def test_goldens_cover_the_contract():
    """Both branches of Generator.choice, fp32 and fp64, k = 1 and k > 1, early stops and tol = 0, 3 and 4 views."""
    gs = {c: load_golden(f"ey_{c}") for c in CASES}
    assert len(CASES) >= 12
    assert any(g["X0"].dtype == np.float32 for g in gs.values())
    assert any(g["X0"].dtype == np.float64 for g in gs.values())
    assert any(int(g["n_iter"]) < case_params(g)["max_iter"] for g in gs.values())
    assert any(case_params(g).get("tol", 1e-6) == 0.0 for g in gs.values())
    assert {int(g["n_views"]) for g in gs.values()} >= {2, 3, 4}
    assert {case_params(g)["latent_dimensions"] for g in gs.values()} >= {1, 2, 3}
    ns = {(g["X0"].shape[0], case_params(g).get("batch_size")) for g in gs.values()}
    assert any(n > 10000 and bs and bs > n // 50 for n, bs in ns)        # tail shuffle
    assert any(n > 10000 and bs and bs <= n // 50 for n, bs in ns)       # Floyd's method at a large n
