"""CPU tests of the ALS models (PLS_ALS, SCCA_PMD, ParkhomenkoCCA, SCCA_Span): import surface, parameters, and a
float64 NumPy restatement of the fit in the implicit-deflation form the device uses, checked against every golden
(the comparator of tests/test_gpu_als.py)."""

import glob
import os

import numpy as np
import pytest

from conftest import load_golden

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "als_*.npz")))
MODELS = ("PLS_ALS", "SCCA_PMD", "ParkhomenkoCCA", "SCCA_Span")

#: the restatement against the goldens (measured worst per-column error 1.13e-15, DESIGN.md "ALS models"): two orders
#: under the device tolerance of tests/test_gpu_als.py, four over the observed floor
RESTATE_TOL = 1e-10


def case_params(g):
    import ast

    return dict(ast.literal_eval(str(g["params"])))


def case_views(g, prefix="X"):
    return [g[f"{prefix}{i}"] for i in range(int(g["n_views"]))]


def col_err(w, ref):
    """Largest per-column relative error."""
    num = np.linalg.norm(w - ref, axis=0)
    den = np.maximum(np.linalg.norm(ref, axis=0), 1e-300)
    return float(np.max(num / den))


def soft(x, t):
    return np.sign(x) * np.maximum(np.abs(x) - t, 0.0)


def pmd_threshold(raw, bound):
    """None when ``||raw||_1 <= bound`` (no thresholding), else the level 50 halvings of [0, max|raw|] end on."""
    if np.sum(np.abs(raw)) <= bound:
        return None
    lo, hi = 0.0, float(np.max(np.abs(raw)))
    for _ in range(50):
        mid = (lo + hi) / 2.0
        if np.sum(np.maximum(np.abs(raw) - mid, 0.0)) > bound:
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2.0


def apply_rule(rule, raw, par):
    """One model's last step: (new w, threshold or None).  ``par``: the L1 bound (pmd), tau (parkhomenko), s (span)."""
    thr = None
    with np.errstate(all="ignore"):
        if rule == "pmd":
            thr = pmd_threshold(raw, par)
            if thr is None:
                return raw / np.sqrt(np.sum(raw * raw)), None
            out = soft(raw, thr)
        elif rule == "parkhomenko":
            thr = float(par)
            out = soft(raw, thr)
        elif rule == "span" and int(par) < len(raw):
            thr = float(np.sort(np.abs(raw))[-int(par)])
            out = np.where(np.abs(raw) >= thr, raw, 0.0)
        else:
            out = raw.copy()
        nrm = np.sqrt(np.sum(out * out))
        if nrm > 1e-12:
            out = out / nrm
    return out, thr


def rule_parameters(model, params, p):
    """(rule, per-view parameter) of a model, with the reference's broadcasting and defaults."""
    from cca_zoo_amd._utils import perview_parameter

    m = len(p)
    if model == "PLS_ALS":
        return "pls", [0.0] * m
    if model == "SCCA_PMD":
        return "pmd", [float(t) * np.sqrt(pi) for t, pi in zip(perview_parameter("tau", params.get("tau", 1.0), 1.0, m), p)]
    if model == "ParkhomenkoCCA":
        return "parkhomenko", [float(t) for t in perview_parameter("tau", params.get("tau", 0.1), 0.1, m)]
    span = params.get("span")
    return "span", [int(s) for s in perview_parameter("span", p[0] if span is None else span, p[0], m)]


def restate(views, model, latent_dimensions=1, center=True, max_iter=500, tol=1e-6, random_state=None, trace=None,
            **rule_params):
    """The fit in float64 NumPy with the views never rewritten.  After ``d`` dimensions view ``i`` of the reference is
    ``(I - Q_i Q_i') X_i`` with ``Q_i`` (n x d) the normalised scores, so
    ``X_d w = s - Q_i (Q_i' s)``, ``s = (X_i - mu_i) w`` and ``X_d' t = (X_i - mu_i)' (t - Q_i (Q_i' t))``.
    Centring is ``v - v.mean(0)`` in the views' dtype, everything after it float64; one ``default_rng`` draws, per
    dimension and view, one ``standard_normal(p_i)``; the sweep is Gauss-Seidel; guards at 1e-12 as in the reference.
    ``trace`` (a list) receives per dimension the list of (view, raw, threshold) of its last sweep.
    Returns (weights, sweeps per dimension, last delta per dimension)."""
    xs = [np.asarray(v) for v in views]
    if center:
        xs = [x - x.mean(axis=0) for x in xs]
    xs = [x.astype(np.float64) for x in xs]
    m, n = len(xs), xs[0].shape[0]
    p = [x.shape[1] for x in xs]
    k = latent_dimensions
    rule, par = rule_parameters(model, rule_params, p)
    rng = np.random.default_rng(random_state)
    W = [np.zeros((pi, k)) for pi in p]
    Q = [np.zeros((n, 0)) for _ in range(m)]
    sweeps, deltas = [], []

    def score(i, w):
        s = xs[i] @ w
        return s - Q[i] @ (Q[i].T @ s)

    with np.errstate(all="ignore"):
        for d in range(k):
            w = [rng.standard_normal(pi) for pi in p]
            w = [wi / np.linalg.norm(wi) for wi in w]
            S = [score(i, w[i]) for i in range(m)]
            done, delta, last = 0, np.inf, []
            for _ in range(max_iter):
                prev = [wi.copy() for wi in w]
                last = []
                for i in range(m):
                    t = sum(S[j] for j in range(m) if j != i)
                    nt = np.sqrt(np.sum(t * t))
                    if nt > 1e-12:
                        t = t / nt
                    raw = xs[i].T @ (t - Q[i] @ (Q[i].T @ t))
                    w[i], thr = apply_rule(rule, raw, par[i])
                    last.append((i, raw, thr))
                    S[i] = score(i, w[i])
                delta = max(np.sqrt(np.sum((w[i] - prev[i]) ** 2)) for i in range(m))
                done += 1
                if delta < tol:
                    break
            sweeps.append(done)
            deltas.append(delta)
            if trace is not None:
                trace.append(last)
            for i in range(m):
                W[i][:, d] = w[i]
                ns = float(S[i] @ S[i])
                if ns > 1e-12:
                    Q[i] = np.column_stack([Q[i], S[i] / np.sqrt(ns)])
    return W, sweeps, deltas


def restate_case(g, **over):
    p = case_params(g)
    p.update(over)
    return restate(case_views(g), str(g["model"]), **p)


def _classes():
    from cca_zoo_amd.linear import PLS_ALS, SCCA_PMD, SCCA_Span, ParkhomenkoCCA

    return {"PLS_ALS": PLS_ALS, "SCCA_PMD": SCCA_PMD, "ParkhomenkoCCA": ParkhomenkoCCA, "SCCA_Span": SCCA_Span}


# ---- import surface and parameters --------------------------------------------------------------------------------
def test_import_surface():
    import cca_zoo_amd.linear as lin
    from cca_zoo_amd.linear import PLS_ALS, SCCA_PMD, SCCA_Span, ParkhomenkoCCA
    from cca_zoo_amd.linear._iterative import PLS_ALS as A, SCCA_PMD as B, SCCA_Span as D, ParkhomenkoCCA as C_

    assert (A, B, C_, D) == (PLS_ALS, SCCA_PMD, ParkhomenkoCCA, SCCA_Span)
    assert set(MODELS) <= set(lin.__all__)


def test_get_params_parity():
    cls = _classes()
    common = {"latent_dimensions": 1, "center": True, "max_iter": 500, "tol": 1e-6, "random_state": None}
    assert cls["PLS_ALS"]().get_params() == common
    assert cls["SCCA_PMD"]().get_params() == {**common, "tau": 1.0}
    assert cls["ParkhomenkoCCA"]().get_params() == {**common, "tau": 0.1}
    assert cls["SCCA_Span"]().get_params() == {**common, "span": None}
    assert cls["SCCA_PMD"](tau=[0.3, 0.4], max_iter=7).get_params()["tau"] == [0.3, 0.4]
    # positional order of the reference's constructors
    assert cls["SCCA_PMD"](2, False, 0.5, 9, 1e-3, 4).get_params() == {
        "latent_dimensions": 2, "center": False, "tau": 0.5, "max_iter": 9, "tol": 1e-3, "random_state": 4}
    assert cls["SCCA_Span"](2, False, 3).span == 3
    assert cls["PLS_ALS"](2, False, 9, 1e-3, 4).random_state == 4


@pytest.mark.parametrize("name", MODELS)
def test_sklearn_estimator_checks(name):
    from sklearn.utils.estimator_checks import (check_estimator_repr, check_get_params_invariance,
                                                check_no_attributes_set_in_init, check_set_params)

    est = _classes()[name]()
    check_no_attributes_set_in_init(name, est)
    check_get_params_invariance(name, est)
    check_set_params(name, est)
    check_estimator_repr(name, est)


def test_validation_and_new_errors(monkeypatch):
    from cca_zoo_amd import _dist

    cls = _classes()
    X, Y = np.zeros((20, 3)), np.zeros((20, 4))
    with pytest.raises(ValueError):
        cls["PLS_ALS"](latent_dimensions=0).fit([X, Y])
    with pytest.raises(ValueError, match="At least 2 views"):
        cls["SCCA_PMD"]().fit([X])
    with pytest.raises(ValueError, match="same number of samples"):
        cls["SCCA_Span"]().fit([X, Y[:10]])
    with pytest.raises(ValueError, match="Parameter 'tau' must be a scalar or a list of length 2, got length 3"):
        cls["SCCA_PMD"](tau=[0.1, 0.2, 0.3]).fit([X, Y])
    with pytest.raises(ValueError, match="Parameter 'tau' must be a scalar or a list of length 2, got length 1"):
        cls["ParkhomenkoCCA"](tau=[0.1]).fit([X, Y])
    with pytest.raises(ValueError, match="Parameter 'span' must be a scalar or a list of length 2"):
        cls["SCCA_Span"](span=[1, 2, 3]).fit([X, Y])
    with pytest.raises(ValueError, match="at most 32"):
        cls["PLS_ALS"](latent_dimensions=33).fit([np.zeros((50, 40)), np.zeros((50, 40))])
    with pytest.raises(ValueError, match="at most 8 views"):
        cls["PLS_ALS"]().fit([X] * 9)
    monkeypatch.setattr(_dist, "is_sharded", lambda: True)
    for c in cls.values():
        with pytest.raises(NotImplementedError, match="row_sharded"):
            c().fit([X, Y])


def test_span_parameters_follow_the_reference():
    """``span=None``: the width of the first view for every view; ``span=0``: every entry (the reference's
    ``np.sort(np.abs(raw))[-0]`` is the smallest magnitude); a negative ``span`` raises."""
    span = _classes()["SCCA_Span"]
    assert span()._rule_parameters([5, 9]) == [5.0, 5.0]
    assert span(span=[3, 12])._rule_parameters([5, 9]) == [3.0, 12.0]
    assert span(span=0)._rule_parameters([5, 9]) == [5.0, 9.0]
    assert span(span=[0, 2])._rule_parameters([5, 9]) == [5.0, 2.0]
    with pytest.raises(ValueError, match="span must not be negative"):
        span(span=[2, -1])._rule_parameters([5, 9])


def test_mixed_host_and_device_views_rejected(monkeypatch):
    from cca_zoo_amd._utils import _resident

    class FakeTensor:
        shape = (20, 4)

    real = _resident.is_device_tensor
    monkeypatch.setattr(_resident, "is_device_tensor", lambda v: isinstance(v, FakeTensor) or real(v))
    monkeypatch.setattr(_resident, "validate_views", lambda views, **kw: list(views))
    with pytest.raises(ValueError, match="all host arrays or all CUDA tensors"):
        _classes()["PLS_ALS"]().fit([np.zeros((20, 3)), FakeTensor()])


def test_initial_vectors_follow_the_reference_draw_order():
    from cca_zoo_amd.linear._iterative import initial_vectors

    p, k = [5, 7, 3], 2
    got = initial_vectors(11, p, k)
    rng = np.random.default_rng(11)
    assert got.shape == (k, sum(p))
    for d in range(k):
        off = 0
        for pi in p:
            w = rng.standard_normal(pi)
            np.testing.assert_array_equal(got[d, off:off + pi], w / np.linalg.norm(w))
            off += pi


# ---- the restatement reproduces every golden ------------------------------------------------------------------------
def support(w):
    return [np.flatnonzero(w[:, d]) for d in range(w.shape[1])]


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_golden(case):
    g = load_golden(f"als_{case}")
    W, sweeps, deltas = restate_case(g)
    assert sweeps == [int(s) for s in g["n_iter"]], (sweeps, g["n_iter"])
    for i, w in enumerate(W):
        ref = g[f"W{i}"]
        assert ref.dtype == np.float64
        err = col_err(w, ref)
        print(f"restatement {case} view {i}: worst column error {err:.2e}")
        assert err <= RESTATE_TOL, (case, i, err)
        for a, b in zip(support(w), support(ref)):
            np.testing.assert_array_equal(a, b)
    np.testing.assert_allclose(deltas, g["last_delta"], rtol=1e-6, atol=1e-13)


def test_restatement_floor_over_all_goldens():
    worst = 0.0
    for case in CASES:
        g = load_golden(f"als_{case}")
        W, _, _ = restate_case(g)
        worst = max([worst] + [col_err(w, g[f"W{i}"]) for i, w in enumerate(W)])
    print(f"restatement: worst per-column error over {len(CASES)} goldens {worst:.2e}")
    assert worst <= RESTATE_TOL


def test_goldens_cover_the_contract():
    gs = {c: load_golden(f"als_{c}") for c in CASES}
    par = {c: case_params(g) for c, g in gs.items()}
    model = {c: str(g["model"]) for c, g in gs.items()}
    assert set(model.values()) == set(MODELS)
    for name in MODELS:
        assert any(model[c] == name and int(gs[c]["n_views"]) == 2 and par[c]["latent_dimensions"] >= 2 for c in gs), name
    for name in ("PLS_ALS", "SCCA_PMD"):
        assert any(model[c] == name and int(gs[c]["n_views"]) == 3 for c in gs), name
    assert any(g["X0"].shape[1] >= 10 * g["X0"].shape[0] for g in gs.values())                  # p >> n
    assert any(g["X0"].dtype == np.float32 for g in gs.values())
    assert any(par[c].get("center") is False for c in gs)
    assert any(isinstance(par[c].get("tau"), list) or isinstance(par[c].get("span"), list) for c in gs)
    assert any(int(max(gs[c]["n_iter"])) == par[c].get("max_iter", 500) for c in gs)            # hits max_iter
    assert any(int(max(gs[c]["n_iter"])) < par[c].get("max_iter", 500) for c in gs)
    # PMD without thresholding, Span keeping everything, Span with a tie at the threshold, PMD on unscaled data
    assert "pmd_nothr" in gs and all(np.all(gs["pmd_nothr"][f"W{i}"] != 0) for i in range(2))
    assert "span_all" in gs and np.all(gs["span_all"]["W0"] != 0)
    s = par["span_tie"]["span"]
    assert any(len(sup) > s for sup in support(gs["span_tie"]["W0"]))
    assert "pmd_unscaled" in gs and max(len(sup) for i in range(2) for sup in support(gs["pmd_unscaled"][f"W{i}"])) <= 3
    for c, g in gs.items():
        tol = par[c].get("tol", 1e-6)
        assert all(abs(float(d) - tol) >= 0.01 * tol for d in g["last_delta"]), c
        assert os.path.getsize(os.path.join(GOLDEN_DIR, f"als_{c}.npz")) < 1000 * 1000
