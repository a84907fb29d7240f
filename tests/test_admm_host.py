"""CPU tests of SCCA_ADMM: import surface, parameters, error cases, and a float64 NumPy restatement of the fit in the
matrix-free, implicit-deflation form the device uses, checked against every golden (the comparator of
tests/test_gpu_admm.py)."""

import glob
import os

import numpy as np
import pytest

from conftest import load_golden
from test_als_host import case_params, case_views, col_err, soft, support

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "admm_*.npz")))

#: float64 views: the bar of tests/test_als_host.py (measured worst per-column error over the goldens: DESIGN.md "ALS models")
RESTATE_TOL = 1e-10
#: float32 views: the reference multiplies X'X in float32 at the first dimension, the restatement in float64.  The bar is
#: 10 x the worst per-column error tools/gen_golden_admm.py printed over the committed float32 cases (F32_MEASURED).
F32_MEASURED = 8.26e-8
F32_TOL = 10 * F32_MEASURED


def restate(views, latent_dimensions=1, center=True, tau=0.1, mu=1.0, max_iter=500, tol=1e-6, random_state=None,
            trace=None):
    """SCCA_ADMM (``cca_zoo/linear/_iterative.py:388-514``) in float64 NumPy with the views never rewritten and
    ``X'X`` never formed.  After ``d`` dimensions view ``i`` of the reference is ``X_d = (I - Q_i Q_i') Xc_i``, so

    * ``X_d w = s - Q_i (Q_i' s)``, ``s = Xc_i w``;
    * ``X_d'X_d w - X_d' t = Xc_i' (r - Q_i (Q_i' r))``, ``r = X_d w - t``;
    * ``|X_d'X_d|_F = |X_d X_d'|_F``: ``(I - QQ') K (I - QQ')`` with ``K = Xc Xc'`` when ``n <= p_i``, else
      ``G - A A'`` with ``G = Xc' Xc``, ``A = Xc' Q_i``.

    Centring is ``v - v.mean(0)`` in the views' dtype, everything after it float64.  The targets of all views come from
    the vectors the iteration started with.  ``z`` and ``w`` coincide between iterations, so ``w - z`` in the
    reference's gradient is exactly zero.  ``trace`` (a list) receives per dimension a dict with ``L`` (per view),
    ``deltas`` (per iteration), and of the last iteration per view ``v`` (= w' + eta), ``thr`` and ``znorm``.
    Returns (weights, iterations per dimension, last delta per dimension)."""
    from cca_zoo_amd._utils import perview_parameter

    xs = [np.asarray(v) for v in views]
    if center:
        xs = [x - x.mean(axis=0) for x in xs]
    xs = [x.astype(np.float64) for x in xs]
    m, n = len(xs), xs[0].shape[0]
    p = [x.shape[1] for x in xs]
    k = latent_dimensions
    taus = [float(t) for t in perview_parameter("tau", tau, 0.1, m)]
    rng = np.random.default_rng(random_state)
    W = [np.zeros((pi, k)) for pi in p]
    Q = [np.zeros((n, 0)) for _ in range(m)]
    gram = [x @ x.T if n <= x.shape[1] else x.T @ x for x in xs]
    iters, deltas = [], []

    def score(i, w):
        s = xs[i] @ w
        return s - Q[i] @ (Q[i].T @ s)

    with np.errstate(all="ignore"):
        for d in range(k):
            w = [rng.standard_normal(pi) for pi in p]
            w = [wi / np.linalg.norm(wi) for wi in w]
            L = [lipschitz(gram[i], xs[i], Q[i], n, mu) for i in range(m)]
            eta = [np.zeros(pi) for pi in p]
            rec = {"L": L, "deltas": []}
            done, delta = 0, np.inf
            for _ in range(max_iter):
                S = [score(i, w[i]) for i in range(m)]
                new, last = [], []
                for i in range(m):
                    t = sum((S[j] for j in range(m) if j != i), np.zeros(n))
                    nt = np.sqrt(np.sum(t * t))
                    if nt > 1e-12:
                        t = t / nt
                    r = S[i] - t
                    r = r - Q[i] @ (Q[i].T @ r)
                    wp = w[i] - (xs[i].T @ r + mu * eta[i]) / L[i]
                    z = soft(wp + eta[i], taus[i] / mu)
                    zn = np.sqrt(np.sum(z * z))
                    if zn > 1.0:
                        z = z / zn
                    last.append({"v": wp + eta[i], "thr": taus[i] / mu, "znorm": zn, "r": r})
                    eta[i] = eta[i] + wp - z
                    new.append(z)
                delta = max(np.sqrt(np.sum((new[i] - w[i]) ** 2)) for i in range(m))
                w = new
                done += 1
                rec["deltas"].append(delta)
                rec["last"] = last
                if delta < tol:
                    break
            iters.append(done)
            deltas.append(delta)
            if trace is not None:
                trace.append(rec)
            for i in range(m):
                W[i][:, d] = w[i]
                s = score(i, w[i])
                ns = float(s @ s)
                q = s / np.sqrt(ns) if ns > 1e-12 else np.zeros(n)     # a zero column: no deflation
                Q[i] = np.column_stack([Q[i], q])
    return W, iters, deltas


def lipschitz(gram, x, Q, n, mu):
    """``|X_d' X_d|_F / n + mu`` from the Gram of the centred view on its smaller side and the scores ``Q``."""
    if n <= x.shape[1]:
        P = np.eye(n) - Q @ Q.T
        D = P @ gram @ P
    else:
        A = x.T @ Q
        D = gram - A @ A.T
    return float(np.sqrt(np.sum(D * D))) / n + mu


def restate_case(g, **over):
    p = case_params(g)
    p.update(over)
    return restate(case_views(g), **p)


# ---- import surface, parameters, errors ------------------------------------------------------------------------------
def test_import_surface():
    import cca_zoo_amd.linear as lin
    from cca_zoo_amd.linear import SCCA_ADMM
    from cca_zoo_amd.linear._iterative import SCCA_ADMM as A

    assert A is SCCA_ADMM and "SCCA_ADMM" in lin.__all__


def test_get_params_parity():
    from cca_zoo_amd.linear import SCCA_ADMM

    assert SCCA_ADMM().get_params() == {"latent_dimensions": 1, "center": True, "tau": 0.1, "mu": 1.0, "max_iter": 500,
                                        "tol": 1e-6, "random_state": None}
    # positional order of the reference's constructor
    assert SCCA_ADMM(2, False, [0.5, 0.2], 3.0, 9, 1e-3, 4).get_params() == {
        "latent_dimensions": 2, "center": False, "tau": [0.5, 0.2], "mu": 3.0, "max_iter": 9, "tol": 1e-3, "random_state": 4}
    assert SCCA_ADMM(tau=[1, 2])._rule_parameters([5, 9]) == [1.0, 2.0]
    assert SCCA_ADMM()._rule_parameters([5, 9, 4]) == [0.1, 0.1, 0.1]


def test_sklearn_estimator_checks():
    from sklearn.utils.estimator_checks import (check_estimator_repr, check_get_params_invariance,
                                                check_no_attributes_set_in_init, check_set_params)

    from cca_zoo_amd.linear import SCCA_ADMM

    est = SCCA_ADMM()
    check_no_attributes_set_in_init("SCCA_ADMM", est)
    check_get_params_invariance("SCCA_ADMM", est)
    check_set_params("SCCA_ADMM", est)
    check_estimator_repr("SCCA_ADMM", est)


def test_error_cases(monkeypatch):
    from cca_zoo_amd import _dist
    from cca_zoo_amd.linear import SCCA_ADMM
    from cca_zoo_amd.linear._iterative import ADMM_MAX_SIDE

    X, Y = np.zeros((20, 3)), np.zeros((20, 4))
    for mu in (0.0, -1.0):
        with pytest.raises(ValueError, match="'mu' parameter"):
            SCCA_ADMM(mu=mu).fit([X, Y])
    with pytest.raises(ValueError, match="Parameter 'tau' must be a scalar or a list of length 2, got length 3"):
        SCCA_ADMM(tau=[0.1, 0.2, 0.3]).fit([X, Y])
    with pytest.raises(ValueError, match="At least 2 views"):
        SCCA_ADMM().fit([X])
    with pytest.raises(ValueError, match="at most 8 views"):
        SCCA_ADMM().fit([X] * 9)
    with pytest.raises(ValueError, match="at most 32"):
        SCCA_ADMM(latent_dimensions=33).fit([np.zeros((50, 40)), np.zeros((50, 40))])
    # the ceiling: min(n, p_i) of one view just above it (a wide or a tall view alone is fine)
    assert ADMM_MAX_SIDE == 16384
    big = np.zeros((ADMM_MAX_SIDE + 1, ADMM_MAX_SIDE + 1), dtype=np.float32)
    with pytest.raises(ValueError, match=r"view 1 has min\(n, p\) = 16385.*at most 16384"):
        SCCA_ADMM().fit([np.zeros((ADMM_MAX_SIDE + 1, 3), dtype=np.float32), big])
    SCCA_ADMM()._check_shapes(ADMM_MAX_SIDE, [10 ** 6, 3])
    SCCA_ADMM()._check_shapes(10 ** 6, [ADMM_MAX_SIDE, 3])
    monkeypatch.setattr(_dist, "is_sharded", lambda: True)
    with pytest.raises(NotImplementedError, match="row_sharded"):
        SCCA_ADMM().fit([X, Y])


# ---- the restatement reproduces every golden ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated():
    """Every golden's restated fit, computed once."""
    out = {}
    for case in CASES:
        g = load_golden(f"admm_{case}")
        out[case] = (g, restate_case(g))
    return out


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_golden(case, restated):
    g, (W, iters, _) = restated[case]
    f32 = g["X0"].dtype == np.float32
    assert iters == [int(s) for s in g["n_iter"]], (iters, g["n_iter"])
    for i, w in enumerate(W):
        ref = g[f"W{i}"]
        assert ref.dtype == np.float64
        err = col_err(w, ref)
        print(f"restatement {case} view {i}: worst column error {err:.2e}")
        assert err <= (F32_TOL if f32 else RESTATE_TOL), (case, i, err)
        for a, b in zip(support(w), support(ref)):
            np.testing.assert_array_equal(a, b)


def test_lipschitz_sides_agree():
    """The two forms of the deflated Gram's norm against the explicitly deflated view, 0, 1 and 3 columns in Q."""
    rng = np.random.default_rng(0)
    for n, p in ((19, 37), (40, 12)):
        x = rng.standard_normal((n, p))
        x -= x.mean(axis=0)
        for d in (0, 1, 3):
            Q = np.linalg.qr(rng.standard_normal((n, max(d, 1))))[0][:, :d]
            xd = x - Q @ (Q.T @ x)
            want = np.linalg.norm(xd.T @ xd) / n + 0.7
            got = lipschitz(x @ x.T if n <= p else x.T @ x, x, Q, n, 0.7)
            assert abs(got - want) <= 1e-13 * want


def test_goldens_cover_the_contract():
    gs = {c: load_golden(f"admm_{c}") for c in CASES}
    par = {c: case_params(g) for c, g in gs.items()}

    def nnz(g, i):
        return [int(np.count_nonzero(g[f"W{i}"][:, d])) for d in range(g[f"W{i}"].shape[1])]

    assert any(int(g["n_views"]) == 2 and g["X0"].shape[0] > g["X0"].shape[1] and par[c]["latent_dimensions"] == 2
               for c, g in gs.items())
    assert any(g["X0"].shape[1] >= 5 * g["X0"].shape[0] for g in gs.values())                    # p >> n
    assert any(int(g["n_views"]) == 3 for g in gs.values())
    assert any(par[c].get("center") is False for c in gs)
    assert any(isinstance(par[c].get("tau"), list) for c in gs)
    f32 = [g for g in gs.values() if g["X0"].dtype == np.float32]
    assert any(g["X0"].shape[0] > g["X0"].shape[1] for g in f32) and any(g["X0"].shape[0] < g["X0"].shape[1] for g in f32)
    # collapse: every weight exactly zero, stopped on tol within a few iterations
    g = gs["collapse"]
    assert all(np.all(g[f"W{i}"] == 0) for i in range(2)) and max(g["n_iter"]) <= 4
    # one view collapses at some dimension, the other does not
    g = gs["half_collapse"]
    assert any((a == 0) != (b == 0) for a, b in zip(nnz(g, 0), nnz(g, 1)))
    # the projection onto the unit ball inactive: a non-zero column of norm below 1
    g = gs["inactive_ball"]
    assert any(0 < np.linalg.norm(g[f"W{i}"][:, d]) < 1 - 1e-6 for i in range(2) for d in range(g["W0"].shape[1]))
    assert all(par[c].get("max_iter", 500) <= 200 for c in gs)
    for c in gs:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, f"admm_{c}.npz")) < 1000 * 1000
