"""CPU tests of SCCA_IPLS / ElasticCCA: the float64 restatement (``enet_restatement.py``: implicit deflation, the elastic
net in Gram form by blocked cyclic coordinate descent under scikit-learn's stop rule) against every golden of the real
reference, the pieces of the restatement against their plain forms, and what the estimators check before any device work.

The reference's solver visits coordinates at random, so the goldens pin down its update map to the accuracy its own ``tol``
buys.  The numeric bar of a class of goldens is ten times the worst per-column error ``tools/gen_golden_enet.py`` printed
for that class (its last line):

    worst restatement col err per class: tight=8.72e-09, default=1.76e-04, f32=5.54e-04

The classes differ by what the reference's ``tol`` leaves (and, for float32 views, by its float32 descent in the first
dimension), not by anything in the code under test.  Supports are identical on every golden.
"""

import os

import numpy as np
import pytest

from conftest import GOLDEN as GOLDEN_DIR, load_golden
from enet_restatement import (ALL_CASES, BW, CASES, case_class, case_params, cd_sweep, col_err, duality_gap, enet_solve,
                              restate_case, soft)

#: 10 x the generator's measured worst per class
BAR = {"tight": 8.72e-8, "default": 1.76e-3, "f32": 5.54e-3}


def test_exports_and_contract():
    import cca_zoo_amd.linear as lin
    from sklearn.utils.estimator_checks import (check_estimator_repr, check_get_params_invariance,
                                                check_no_attributes_set_in_init, check_set_params)

    for name in ("SCCA_IPLS", "ElasticCCA"):
        assert name in lin.__all__
        est = getattr(lin, name)()
        check_no_attributes_set_in_init(name, est)
        check_get_params_invariance(name, est)
        check_set_params(name, est)
        check_estimator_repr(name, est)
    p = lin.SCCA_IPLS().get_params()
    assert (p["alpha"], p["l1_ratio"], p["max_iter"], p["tol"], p["latent_dimensions"]) == (0.0, 1.0, 500, 1e-6, 1)
    assert lin.ElasticCCA().get_params()["l1_ratio"] == 0.5


@pytest.mark.parametrize("name", ["SCCA_IPLS", "ElasticCCA"])
def test_error_cases(name, monkeypatch):
    import cca_zoo_amd.linear as lin
    from cca_zoo_amd import _dist
    from cca_zoo_amd.linear._iterative import ENET_MAX_P

    cls = getattr(lin, name)
    X, Y = np.zeros((20, 3)), np.zeros((20, 4))
    with pytest.raises(ValueError, match="'alpha' parameter"):
        cls(alpha=-0.1).fit([X, Y])
    with pytest.raises(ValueError, match="'l1_ratio' parameter"):
        cls(l1_ratio=1.5).fit([X, Y])
    with pytest.raises(ValueError, match="alpha must be finite and not negative"):
        cls(alpha=[0.1, -0.1]).fit([X, Y])
    with pytest.raises(ValueError, match=r"l1_ratio must lie in \[0, 1\]"):
        cls(l1_ratio=[0.5, 2.0]).fit([X, Y])
    with pytest.raises(ValueError, match="Parameter 'alpha' must be a scalar or a list of length 2, got length 3"):
        cls(alpha=[0.1, 0.2, 0.3]).fit([X, Y])
    with pytest.raises(ValueError, match="Parameter 'l1_ratio' must be a scalar or a list of length 2, got length 1"):
        cls(l1_ratio=[0.5]).fit([X, Y])
    with pytest.raises(ValueError, match="'tol' parameter"):
        cls(tol=-1.0).fit([X, Y])
    with pytest.raises(ValueError, match="At least 2 views"):
        cls().fit([X])
    with pytest.raises(ValueError, match="at most 8 views"):
        cls().fit([X] * 9)
    with pytest.raises(ValueError, match="at most 32"):
        cls(latent_dimensions=33).fit([np.zeros((50, 40)), np.zeros((50, 40))])
    # the ceiling of the p x p Gram
    assert ENET_MAX_P == 16384
    with pytest.raises(ValueError, match=r"view 1 has 16385 columns.*at most 16384"):
        cls(alpha=0.1).fit([np.zeros((4, 3), dtype=np.float32), np.zeros((4, ENET_MAX_P + 1), dtype=np.float32)])
    cls(alpha=0.1)._check_shapes(10 ** 6, [ENET_MAX_P, 3])
    # the ridge branch without a penalty on a view that is not tall
    with pytest.raises(ValueError, match="view 1: l1_ratio = 0 with alpha = 0 and p >= n"):
        cls(alpha=[0.1, 0.0], l1_ratio=[0.5, 0.0]).fit([np.zeros((4, 3)), np.zeros((4, 4))])
    cls(alpha=[0.1, 0.0], l1_ratio=[0.5, 0.0])._check_shapes(5, [3, 4])
    cls(alpha=[0.1, 1e-3], l1_ratio=[0.5, 0.0])._check_shapes(4, [3, 4])
    monkeypatch.setattr(_dist, "is_sharded", lambda: True)
    with pytest.raises(NotImplementedError, match="row_sharded"):
        cls().fit([X, Y])


# ---- the pieces of the restatement ----------------------------------------------------------------------------------
def _problem(seed, n, p, zero_col=None):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, p)) / np.sqrt(n)
    if zero_col is not None:
        x[:, zero_col] = 0.0
    t = rng.standard_normal(n)
    t /= np.linalg.norm(t)
    return x, t, rng


@pytest.mark.parametrize("p", [9, BW, BW + 1, 3 * BW + 7])
def test_blocked_sweep_is_the_plain_sweep(p):
    """The blocked sweep against one coordinate at a time on the rows themselves (scikit-learn's loop), a zero column
    included."""
    n, a, b = 40, 0.05, 0.3
    x, t, rng = _problem(p, n, p, zero_col=p // 2)
    c0 = rng.standard_normal(p) * (rng.random(p) < 0.5)
    G, q = x.T @ x, x.T @ t
    c, r = c0.copy(), q - G @ c0
    dmax, cmax, _ = cd_sweep(G, r, c, a, b)
    w, R = c0.copy(), t - x @ c0
    for j in range(p):
        nj = x[:, j] @ x[:, j]
        if nj == 0.0:
            continue
        R += w[j] * x[:, j]
        w[j] = soft(x[:, j] @ R, a) / (nj + b)
        R -= w[j] * x[:, j]
    np.testing.assert_allclose(c, w, rtol=0, atol=1e-13 * np.abs(w).max())
    np.testing.assert_allclose(r, x.T @ R, rtol=0, atol=1e-13)
    assert c[p // 2] == c0[p // 2]                   # the zero column is skipped
    assert abs(dmax - np.abs(c - c0).max()) <= 1e-15 and cmax == np.abs(c).max()


def test_gap_in_gram_form():
    """The Gram-form gap against scikit-learn's expression on the rows, both branches of the dual scaling."""
    x, t, rng = _problem(5, 30, 12)
    G, q, tt = x.T @ x, x.T @ t, float(t @ t)
    for a, b, scale in ((0.05, 0.2, 0.1), (5.0, 0.2, 0.01), (0.0, 0.0, 0.1)):
        c = scale * rng.standard_normal(12)
        R = t - x @ c
        XtA = x.T @ R - b * c
        dual = np.abs(XtA).max()
        if dual > a:
            cst = a / dual
            want = 0.5 * (R @ R + (R @ R) * cst ** 2)
        else:
            cst, want = 1.0, R @ R
        want += a * np.abs(c).sum() - cst * (R @ t) + 0.5 * b * (1 + cst ** 2) * (c @ c)
        got = duality_gap(q, q - G @ c, c, tt, a, b)
        assert abs(got - want) <= 1e-13 * max(1.0, abs(want))


def test_solve_reaches_the_minimiser():
    """The solve against scikit-learn's ElasticNet (cyclic, tight tolerance) and against the ridge normal equations."""
    from sklearn.linear_model import ElasticNet

    n, p = 50, 14
    x, t, _ = _problem(11, n, p)
    x *= np.sqrt(n)
    G, q, tt = x.T @ x, x.T @ t, float(t @ t)
    alpha, l1 = 0.01, 0.6
    c, r, sweeps, capped, gap = enet_solve(G, q, tt, np.zeros(p), n * alpha * l1, n * alpha * (1 - l1), False, 1e-12)
    ref = ElasticNet(alpha=alpha, l1_ratio=l1, fit_intercept=False, tol=1e-14, max_iter=100000).fit(x, t).coef_
    assert not capped and gap < 1e-12 * tt and 0 < np.count_nonzero(ref) < p
    np.testing.assert_array_equal(c != 0, ref != 0)
    assert np.linalg.norm(c - ref) <= 1e-9 * np.linalg.norm(ref)
    np.testing.assert_allclose(r, q - G @ c, rtol=0, atol=1e-12)
    c, _, _, capped, _ = enet_solve(G, q, tt, np.zeros(p), 0.0, 0.7, True, 1e-12)
    want = np.linalg.solve(G + 0.7 * np.eye(p), q)
    assert not capped and np.linalg.norm(c - want) <= 1e-9 * np.linalg.norm(want)


# ---- the restatement reproduces every golden ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated():
    """Every golden's restated fit, computed once."""
    out = {}
    for case in ALL_CASES:
        g = load_golden(f"enet_{case}")
        out[case] = (g, restate_case(g))
    return out


@pytest.mark.parametrize("case", ALL_CASES)
def test_restatement_reproduces_golden(case, restated):
    g, (W, iters, inner, capped) = restated[case]
    assert capped == 0 and len(iters) == len(inner) == int(g["latent_dimensions"])
    for i, w in enumerate(W):
        ref = g[f"W{i}"]
        assert ref.dtype == np.float64
        np.testing.assert_array_equal(w != 0, ref != 0)          # identical supports, every golden
        np.testing.assert_array_equal(ref != 0, g[f"nz{i}"])
        err = col_err(w, ref)
        print(f"restatement {case} view {i}: worst column error {err:.2e} (bar {BAR[case_class(case)]:.2e})")
        assert err <= BAR[case_class(case)], (case, i, err)


def test_goldens_cover_the_contract():
    gs = {c: load_golden(f"enet_{c}") for c in ALL_CASES}
    par = {c: case_params(g) for c, g in gs.items()}
    for model in ("SCCA_IPLS", "ElasticCCA"):
        mine = [c for c in gs if str(gs[c]["model"]) == model]
        two = [c for c in mine if int(gs[c]["n_views"]) == 2 and par[c]["latent_dimensions"] == 2]
        assert any(par[c]["tol"] == 1e-10 for c in two) and any(par[c]["tol"] == 1e-6 for c in two)
        assert any(int(gs[c]["n_views"]) == 3 for c in mine)
        assert any(gs[c]["X0"].dtype == np.float32 for c in mine)
    assert set(CASES["tight"]) == {c for c in gs if par[c]["tol"] <= 1e-10}
    assert set(CASES["f32"]) == {c for c in gs if gs[c]["X0"].dtype == np.float32}
    g = gs["ipls_lasso_tall"]
    assert par["ipls_lasso_tall"]["l1_ratio"] == [1.0, 1.0] and all(g["X0"].shape[0] > g[f"X{i}"].shape[1] for i in range(2))
    g = gs["ipls_wide"]
    assert (g["X0"].shape, g["X1"].shape) == ((40, 300), (40, 200)) and all(0 < l < 1 for l in par["ipls_wide"]["l1_ratio"])
    assert any(0.0 in par[c]["l1_ratio"] and len(set(par[c]["l1_ratio"])) > 1 for c in gs)       # the ridge branch, mixed in
    assert any(len(set(par[c]["alpha"])) > 1 for c in gs)
    assert any(par[c]["center"] is False for c in gs)
    assert any(list(gs[c]["n_iter"]) == [par[c]["max_iter"]] * par[c]["latent_dimensions"] for c in gs)     # ends on max_iter
    for c, g in gs.items():
        assert all(np.all(np.linalg.norm(g[f"W{i}"], axis=0) > 0) for i in range(int(g["n_views"]))), c
        assert os.path.getsize(os.path.join(GOLDEN_DIR, f"enet_{c}.npz")) < 1000 * 1000
