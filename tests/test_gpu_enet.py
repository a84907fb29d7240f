"""GPU tests of SCCA_IPLS / ElasticCCA: the elastic-net kernels one at a time through ``ccz_als_peek`` against NumPy (the
p-side Gram, its deflation, one blocked CD sweep, the duality gap), every golden through the estimators (host arrays and
CUDA tensors) against the float64 restatement, determinism, the unit variance of the IPLS scores and the inner cap."""

import ctypes as C
import warnings

import numpy as np
import pytest

from conftest import load_golden
from enet_restatement import ALL_CASES, BW, case_class, case_params, case_views, cd_sweep, col_err, duality_gap, restate_case
from test_enet_host import BAR
from test_gpu_als import _Fit, _init

pytestmark = pytest.mark.gpu

W_TOL = 1e-8          # per-column relative error of weights_ against the restatement, the family's device bar (tol <= 1e-10)
K_TOL = 1e-12         # kernels against NumPy, relative
RULE_ENET = 5
PEEK = {"w": 0, "raw": 1, "score": 2, "target": 3, "Q": 4, "G": 9, "r": 10, "coef": 11, "enet": 12}
_dp = C.POINTER(C.c_double)


class _EnetFit(_Fit):
    """A raw CCZ_ALS_ENET fit state (``test_gpu_als._Fit``) after ``ccz_als_enet_setup``."""

    def __init__(self, views, k, a, b, ridge=None, target_all=False, post_std=False, **kw):
        m = len(views)
        super().__init__(views, k, RULE_ENET, [0.0] * m, **kw)
        self.a, self.b = [float(x) for x in a], [float(x) for x in b]
        self.h.check(self.h.lib.ccz_als_enet_setup(
            self.h.raw, self.state, self.varr, self.marr, (C.c_double * m)(*self.a), (C.c_double * m)(*self.b),
            (C.c_int * m)(*(ridge or [0] * m)), int(target_all), int(post_std)))

    def peek(self, what, view):
        p = self.p[view]
        size = {"w": p, "raw": p, "score": self.n, "target": self.n, "Q": self.k * self.n, "G": p * p, "r": p, "coef": p, "enet": 4}[what]
        out = np.empty(size)
        self.h.check(self.h.lib.ccz_als_peek(self.h.raw, self.state, PEEK[what], view, out.ctypes.data_as(_dp)))
        return out.reshape(self.k, self.n) if what == "Q" else out.reshape(p, p) if what == "G" else out

    def solve(self, view, G, q, c0, tt, sweeps):
        G, q, c0 = (np.ascontiguousarray(x, dtype=np.float64) for x in (G, q, c0))
        self.h.check(self.h.lib.ccz_als_enet_solve(self.h.raw, self.state, view, G.ctypes.data_as(_dp), q.ctypes.data_as(_dp),
                                                   c0.ctypes.data_as(_dp), float(tt), sweeps))


# one partial block; several blocks with a ragged tail
SHAPES = [((12, 9), 60), ((300, 200), 40)]
IDS = ["12x9_n60", "300x200_n40"]


def _data(dims, n, dtype):
    rng = np.random.default_rng(len(dims) * 1000 + n)
    z = rng.standard_normal((n, 2))
    views = [(z @ rng.standard_normal((2, d)) + rng.standard_normal((n, d)) + 0.5).astype(dtype) for d in dims]
    return rng, views


def _close(got, want, what):
    err = np.abs(np.asarray(got) - np.asarray(want)).max() / max(np.abs(want).max(), 1e-300)
    print(f"{what}: {err:.2e}")
    assert err <= K_TOL, (what, err)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gram_and_its_deflation(shape, dtype):
    """G_i after the setup against fl(X - mu)' fl(X - mu); after one dimension against the Gram of the explicitly deflated
    view (Q as the device left it)."""
    dims, n = shape
    rng, views = _data(dims, n, dtype)
    fit = _EnetFit(views, 2, [0.05 * n * 0.7] * 2, [0.05 * n * 0.3] * 2, post_std=True, tol=1e-6, max_iter=2, pad=3)
    try:
        for i in range(2):
            _close(fit.peek("G", i), fit.xs[i].T @ fit.xs[i], f"gram view {i}")
        fit.set_init(_init(rng, list(dims), 2))
        for _ in range(200):                    # unit by unit, so that no unit of the second dimension has run
            fit.sweeps(1)
            if fit.status()[0] >= 1:
                break
        assert fit.status()[:2] == (1, 0)
        for i in range(2):
            q = fit.peek("Q", i)[0]
            assert abs(q @ q - 1.0) <= 1e-12
            xd = fit.xs[i] - np.outer(q, q @ fit.xs[i])
            _close(fit.peek("G", i), xd.T @ xd, f"deflated gram view {i}")
    finally:
        fit.close()


def _cd_problem(p, seed):
    """(G, q, c0) with a zero-diagonal coordinate and, when there is a second block, one that changes nothing: its rows of
    G are the identity's, its q and c0 zero, so z = 0 at every coordinate."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((40, p)) / np.sqrt(40)
    x[:, 3] = 0.0
    if p > 2 * BW:
        x[:, BW:2 * BW] = 0.0
    G = x.T @ x
    t = rng.standard_normal(40)
    q = x.T @ t
    if p > 2 * BW:
        G[np.arange(BW, 2 * BW), np.arange(BW, 2 * BW)] = 1.0
    c0 = rng.standard_normal(p) * (rng.random(p) < 0.5) * 0.1
    if p > 2 * BW:
        c0[BW:2 * BW] = 0.0
    return G, q, c0, float(t @ t)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_cd_sweep(shape):
    """One blocked sweep from a given (G, q, c): the coefficients and r against the restatement's sweep."""
    dims, n = shape
    _, views = _data(dims, n, np.float64)
    a, b = [0.05, 0.02], [0.3, 0.0]
    fit = _EnetFit(views, 1, a, b, tol=0.0)          # tol = 0: the stop rule never holds
    try:
        for i, p in enumerate(dims):
            G, q, c0, tt = _cd_problem(p, p)
            for sweeps in (1, 3):
                fit.solve(i, G, q, c0, tt, sweeps)
                c, r = c0.copy(), q - G @ c0
                for _ in range(sweeps):
                    _, _, blocks = cd_sweep(G, r, c, a[i], b[i])
                if p > 2 * BW:
                    assert blocks[1] == 0.0 and blocks[0] > 0.0 and blocks[-1] > 0.0 and p % BW != 0
                _close(fit.peek("coef", i), c, f"coefficients view {i} after {sweeps} sweep(s)")
                _close(fit.peek("r", i), r, f"r view {i} after {sweeps} sweep(s)")
                _close(fit.peek("raw", i), q, "q")
                assert fit.peek("coef", i)[3] == c0[3]                      # the zero-diagonal coordinate is skipped
                assert fit.peek("enet", i)[3] == sweeps
    finally:
        fit.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gap_value(shape):
    """The duality gap after one sweep (a tol so large that the first sweep computes it and stops), both branches of the
    dual scaling: a below and above max |X'R - b c|."""
    dims, n = shape
    _, views = _data(dims, n, np.float64)
    for a in (0.05, 50.0):
        fit = _EnetFit(views, 1, [a, a], [0.3, 0.3], tol=1e30)
        try:
            for i, p in enumerate(dims):
                G, q, c0, tt = _cd_problem(p, p + 1)
                fit.solve(i, G, q, c0, tt, 5)
                c, r = c0.copy(), q - G @ c0
                cd_sweep(G, r, c, a, 0.3)
                want = duality_gap(q, r, c, tt, a, 0.3)
                t0, gap, _, sweeps = fit.peek("enet", i)
                assert t0 == tt and sweeps == 1                              # stopped after the first sweep
                assert (np.abs(r - 0.3 * c).max() > a) == (a == 0.05)
                err = abs(gap - want) / max(tt, abs(want))
                print(f"gap a={a} view {i}: {gap:.6e} against {want:.6e} ({err:.2e})")
                assert err <= K_TOL
        finally:
            fit.close()


# ---- the reference's fits ------------------------------------------------------------------------------------------
def _model(g, **over):
    import cca_zoo_amd.linear as lin

    p = case_params(g)
    p.update(over)
    return getattr(lin, str(g["model"]))(**p)


@pytest.fixture(scope="module")
def restated():
    """The float64 restatement of every golden, computed once."""
    return {case: restate_case(load_golden(f"enet_{case}")) for case in ALL_CASES}


def _deflated_scores(views, weights, center):
    """The score of every column on the reference's explicitly deflated views, (views, k, n)."""
    X = [np.asarray(v - v.mean(axis=0) if center else v).astype(np.float64) for v in views]
    out = []
    for d in range(weights[0].shape[1]):
        s = [x @ w[:, d] for x, w in zip(X, weights)]
        out.append(s)
        X = [x - np.outer(si, si @ x) / (si @ si) if si @ si > 1e-12 else x for x, si in zip(X, s)]
    return out


@pytest.mark.parametrize("source", ["host", "cuda"])
@pytest.mark.parametrize("case", ALL_CASES)
def test_golden_case(case, source, restated):
    g = load_golden(f"enet_{case}")
    views = case_views(g)
    cls = case_class(case)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)          # no solve of a golden ends on the cap
        if source == "cuda":
            import torch

            tens = [torch.as_tensor(v, device="cuda") for v in views]
            before = [t.clone() for t in tens]
            model = _model(g).fit(tens)
            for x, y in zip(tens, before):
                assert torch.equal(x, y)
        else:
            model = _model(g).fit(views)
    W, iters, inner, _ = restated[case]
    print(f"golden {case} ({source}): sweeps {model.n_iter_} (restatement {iters}), CD sweeps {model.n_inner_iter_} "
          f"(restatement {inner})")
    if cls == "tight":
        assert model.n_iter_ == iters
    # tol <= 1e-10: the family's bar against the restatement; default tol: device and restatement may differ by one inner
    # sweep where the gap sits at its threshold, so the bar is what that tol leaves (the class bar of the CPU test)
    bar = W_TOL if cls == "tight" else BAR["default"]
    for i, w in enumerate(model.weights_):
        assert w.dtype == np.float64 and model.means_[i].dtype == views[i].dtype
        err, gerr = col_err(w, W[i]), col_err(w, g[f"W{i}"])
        print(f"golden {case} ({source}) view {i}: col err to the restatement {err:.2e}, to the golden {gerr:.2e}")
        assert err <= bar, (i, err)
        assert gerr <= BAR[cls], (i, gerr)
        np.testing.assert_array_equal(w != 0, W[i] != 0)
        np.testing.assert_array_equal(w != 0, g[f"nz{i}"])
    if str(g["model"]) == "SCCA_IPLS":
        for s in _deflated_scores(views, model.weights_, bool(g["center"])):
            for si in s:
                assert abs(si.std() - 1.0) <= 1e-10, si.std()


@pytest.mark.parametrize("case", ["ipls_wide", "en2"])
def test_two_fits_are_bit_identical(case):
    g = load_golden(f"enet_{case}")
    a, b = _model(g).fit(case_views(g)), _model(g).fit(case_views(g))
    assert a.n_iter_ == b.n_iter_ and a.n_inner_iter_ == b.n_inner_iter_
    for x, y in zip(a.weights_, b.weights_):
        np.testing.assert_array_equal(x, y)


def test_inner_cap_warns():
    """tol = 0 on the ridge branch, whose stop rule (a coordinate change below zero) can never hold: both solves run to the
    cap of 1000 sweeps, over many units, and the fit says so once."""
    g = load_golden("enet_ipls2")
    with pytest.warns(RuntimeWarning, match="2 coordinate-descent solve") as rec:
        model = _model(g, latent_dimensions=1, max_iter=1, tol=0.0, alpha=0.5, l1_ratio=0.0).fit(case_views(g))
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert model.n_iter_ == [1] and model.n_inner_iter_ == [2000]
    assert all(np.all(np.isfinite(w)) for w in model.weights_)
