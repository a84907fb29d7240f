"""GPU tests of SCCA_ADMM: every golden through the estimator (host arrays and CUDA tensors) against the float64
restatement, the kernels one at a time against NumPy through ``ccz_als_peek``, L_i against the explicitly deflated Gram
on both sides, the Jacobi ordering, determinism, the stop word, and a grid search."""

import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from test_admm_host import CASES, restate, restate_case
from test_als_host import case_params, case_views, col_err, soft, support
from test_gpu_als import _Fit, _init, _rel

pytestmark = pytest.mark.gpu

W_TOL = 1e-8          # per-column relative error of weights_, the family's device bar (fp64 and fp32 views compute in fp64)
RULE_ADMM = 4
PEEK = {"w": 0, "raw": 1, "score": 2, "target": 3, "Q": 4, "z": 6, "eta": 7, "L": 8}


class _AdmmFit(_Fit):
    """A raw CCZ_ALS_ADMM fit state (``test_gpu_als._Fit``) with the Grams set up and the ADMM buffers to peek."""

    def __init__(self, views, k, tau, mu, **kw):
        super().__init__(views, k, RULE_ADMM, tau, **kw)
        self.mu = mu
        self.h.check(self.h.lib.ccz_als_admm_setup(self.h.raw, self.state, self.varr, self.marr, float(mu)))

    def peek(self, what, view):
        size = {"w": self.p[view], "raw": self.p[view], "score": self.n, "target": self.n, "Q": self.k * self.n,
                "z": self.p[view], "eta": self.p[view], "L": 1}[what]
        out = np.empty(size)
        self.h.check(self.h.lib.ccz_als_peek(self.h.raw, self.state, PEEK[what], view, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out.reshape(self.k, self.n) if what == "Q" else out


def _model(g, **over):
    from cca_zoo_amd.linear import SCCA_ADMM

    p = case_params(g)
    p.update(over)
    return SCCA_ADMM(**p)


@pytest.fixture(scope="module")
def restated():
    """The float64 restatement of every golden, computed once."""
    return {case: restate_case(load_golden(f"admm_{case}")) for case in CASES}


# ---- the reference's fits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["host", "cuda"])
@pytest.mark.parametrize("case", CASES)
def test_golden_case(case, source, restated):
    g = load_golden(f"admm_{case}")
    views = case_views(g)
    f32 = views[0].dtype == np.float32
    if source == "cuda":
        import torch

        tens = [torch.as_tensor(v, device="cuda") for v in views]
        before = [t.clone() for t in tens]
        model = _model(g).fit(tens)
        for a, b in zip(tens, before):
            assert torch.equal(a, b)
    else:
        model = _model(g).fit(views)
    W, iters, _ = restated[case]
    assert model.n_iter_ == iters == [int(s) for s in g["n_iter"]]
    for i, w in enumerate(model.weights_):
        assert w.dtype == np.float64
        assert model.means_[i].dtype == g[f"mean{i}"].dtype
        err = col_err(w, W[i])
        gerr = col_err(w, g[f"W{i}"])
        print(f"golden {case} ({source}) view {i}: col err to the restatement {err:.2e}, to the golden {gerr:.2e}")
        assert err <= W_TOL, (i, err)
        if not f32:
            assert gerr <= W_TOL, (i, gerr)
        for a, b, c in zip(support(w), support(W[i]), support(g[f"W{i}"])):
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(a, c)


# ---- kernels through the C ABI --------------------------------------------------------------------------------------
# dims, n: odd widths (scalar loads for float32) on the n side; across the 1024-column strip; two column splits of the score
# kernel; the p side with more than one row chunk (n = 200: 50 chunks of 4 rows)
SHAPES = [((37, 21), 19), ((1030, 517), 64), ((9001, 300), 48), ((16, 12), 200)]
IDS = [f"{'x'.join(map(str, s[0]))}_n{s[1]}" for s in SHAPES]


def _data(dims, n, dtype):
    rng = np.random.default_rng(len(dims) * 1000 + n)
    z = rng.standard_normal((n, 2))
    views = [((z @ rng.standard_normal((2, d)) + rng.standard_normal((n, d))) / np.sqrt(n) + 0.5).astype(dtype) for d in dims]
    return rng, views


def _gram_norm(x, Q):
    """|X_d' X_d|_F of the explicitly deflated view."""
    xd = x - Q @ (Q.T @ x)
    return np.linalg.norm(xd.T @ xd)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kernels_after_one_iteration(shape, dtype):
    """One iteration of the first dimension: every buffer is recomputed in NumPy float64 from the buffers it was made
    from (eta = 0, Q empty)."""
    dims, n = shape
    rng, views = _data(dims, n, dtype)
    m, mu = len(dims), 0.7
    tau = [0.02, 0.05][:m]
    w0 = _init(rng, list(dims), 1)
    fit = _AdmmFit(views, 1, tau, mu, max_iter=5, pad=3, pad_value=1e30)
    try:
        fit.set_init(w0)
        fit.sweeps(1)
        assert fit.status()[:3] == (0, 0, [1])
        w0s = np.split(w0[0], np.cumsum(dims)[:-1])
        s0 = [fit.xs[i] @ w0s[i] for i in range(m)]
        for i in range(m):
            L = fit.peek("L", i)[0]
            want = _gram_norm(fit.xs[i], np.zeros((n, 0))) / n + mu
            print(f"L {np.dtype(dtype).name} {dims} view {i}: {abs(L - want) / want:.2e}")
            assert abs(L - want) <= 1e-12 * want
            t = sum(s0[j] for j in range(m) if j != i)
            t = t / np.linalg.norm(t)
            r = s0[i] - t
            if i == m - 1:                                   # prologue alone: the n-vector of the last view updated
                assert _rel(fit.peek("target", i), r) <= 1e-12
            raw, z, eta = fit.peek("raw", i), fit.peek("z", i), fit.peek("eta", i)
            # xt + fold: w' from the initial vector
            err = _rel(raw, w0s[i] - (fit.xs[i].T @ r) / L)
            print(f"w' {np.dtype(dtype).name} {dims} view {i}: {err:.2e}")
            assert err <= 1e-12
            # apply alone, from the device's own w'
            u = soft(raw, tau[i] / mu)
            nu = np.sqrt(np.sum(u * u))
            ref = u / nu if nu > 1.0 else u
            np.testing.assert_array_equal(z != 0, ref != 0)
            assert np.count_nonzero(z) > 0
            assert _rel(z, ref) <= 1e-14
            assert _rel(eta, raw - z) <= 1e-14
            np.testing.assert_array_equal(fit.peek("w", i), z)
            # the scores of the new vectors
            assert _rel(fit.peek("score", i), fit.xs[i] @ z) <= 1e-12
    finally:
        fit.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[3]], ids=[IDS[0], IDS[1], IDS[3]])
def test_lipschitz_against_the_deflated_gram(shape, dtype):
    """max_iter = 1, so iteration d + 1 is the first of dimension d: L_i of dimensions 0, 1 and 3 against
    ``np.linalg.norm`` of the explicitly deflated Gram with the device's own Q (n side: 37x21 and 1030x517; p side: 16x12
    at n = 200)."""
    dims, n = shape
    rng, views = _data(dims, n, dtype)
    mu, k = 0.3, 4
    fit = _AdmmFit(views, k, [0.01, 0.01], mu, max_iter=1, pad=1, pad_value=1e30)
    try:
        fit.set_init(_init(rng, list(dims), k))
        done = 0
        for d in (0, 1, 3):
            fit.sweeps(d + 1 - done)
            done = d + 1
            for i in range(2):
                Q = fit.peek("Q", i)[:d].T
                if d:
                    assert np.max(np.abs(Q.T @ Q - np.eye(d))) <= 1e-10       # d deflations took place
                want = _gram_norm(fit.xs[i], Q) / n + mu
                L = fit.peek("L", i)[0]
                print(f"L {np.dtype(dtype).name} {dims} dimension {d} view {i}: {L:.17g} vs {want:.17g} ({abs(L - want) / want:.2e})")
                assert abs(L - want) <= 1e-12 * want
        assert fit.status()[:2] == (4, 1)
    finally:
        fit.close()


def test_targets_are_jacobi():
    """Three views, one iteration: the n-vector of view 2 is built from the scores of the INITIAL vectors of views 0
    and 1, not from their updates (which the Gauss-Seidel sweep of the sibling models would use)."""
    dims, n = (37, 21, 9), 19
    rng, views = _data(dims, n, np.float64)
    w0 = _init(rng, list(dims), 1)
    fit = _AdmmFit(views, 1, [0.02] * 3, 0.7, max_iter=5)
    try:
        fit.set_init(w0)
        fit.sweeps(1)
        w0s = np.split(w0[0], np.cumsum(dims)[:-1])
        s0 = [fit.xs[i] @ w0s[i] for i in range(3)]
        s1 = [fit.xs[i] @ fit.peek("w", i) for i in range(3)]

        def vec(s):
            t = s[0] + s[1]
            return s0[2] - t / np.linalg.norm(t)

        got = fit.peek("target", 2)
        assert _rel(got, vec(s0)) <= 1e-12
        assert _rel(got, vec(s1)) > 1e-3
    finally:
        fit.close()


def test_stop_inside_a_chunk_and_later_iterations_are_no_ops(restated):
    g = load_golden("admm_tolstop")
    views, par = case_views(g), case_params(g)
    p = [v.shape[1] for v in views]
    from cca_zoo_amd.linear._iterative import initial_vectors

    want = [int(s) for s in g["n_iter"]]
    assert want[1] < par["max_iter"] and sum(want) % 8 != 0          # the second dimension stops on tol, inside a chunk
    fit = _AdmmFit(views, 2, [par["tau"]] * 2, par["mu"], tol=par["tol"], max_iter=par["max_iter"], chunk=8, pad_value=0.0)
    try:
        fit.set_init(initial_vectors(par["random_state"], p, 2))
        total = 0
        while total < sum(want) + 16:
            fit.sweeps(8)
            total += 8
        done, stopped, iters, deltas = fit.status()
        assert (done, stopped, iters) == (2, 1, want)
        assert deltas[1] < par["tol"] <= deltas[0]
        known, stop_known = fit.sweeps(0)
        assert stop_known == 1 and known == sum(want)
        for i, w in enumerate(fit.weights()):
            assert col_err(w, restated["tolstop"][0][i]) <= W_TOL
    finally:
        fit.close()


@pytest.mark.parametrize("case", ["wide_f32", "three"])
def test_two_fits_are_bit_identical(case):
    g = load_golden(f"admm_{case}")
    a = _model(g).fit(case_views(g))
    b = _model(g).fit(case_views(g))
    assert a.n_iter_ == b.n_iter_ and a.last_delta_ == b.last_delta_
    for x, y in zip(a.weights_, b.weights_):
        np.testing.assert_array_equal(x, y)


def test_max_iter_is_reached_and_scores_are_orthogonal(restated):
    g = load_golden("admm_perview")
    views = case_views(g)
    model = _model(g).fit(views)
    assert model.n_iter_ == [case_params(g)["max_iter"]] * 2
    assert all(d >= 1e-6 for d in model.last_delta_)
    np.testing.assert_allclose(model.last_delta_, restated["perview"][2], rtol=1e-6)
    # dimension d's weights act on the deflated views: their scores are orthogonal across dimensions
    for i, v in enumerate(views):
        x = v - v.mean(axis=0)
        S = []
        for d in range(2):
            s = x @ model.weights_[i][:, d]
            S.append(s / np.linalg.norm(s))
            x = x - np.outer(S[-1], S[-1] @ x)
        assert abs(S[0] @ S[1]) <= 1e-8


def test_zero_view_exercises_the_guards():
    """A zero view: zero scores and a zero Gram (L = mu), the other view's target keeps norm 0 and nothing is deflated
    from it -- against the restatement, and no NaN."""
    from cca_zoo_amd.linear import SCCA_ADMM

    rng = np.random.default_rng(0)
    X, Z = rng.standard_normal((40, 7)), np.zeros((40, 5))
    params = dict(latent_dimensions=2, tau=0.05, mu=0.5, max_iter=7, random_state=0)
    model = SCCA_ADMM(**params).fit([X, Z])
    W, iters, _ = restate([X, Z], **params)
    assert model.n_iter_ == iters
    for w, r in zip(model.weights_, W):
        assert np.all(np.isfinite(w))
        np.testing.assert_allclose(w, r, atol=1e-12)


def test_grid_search_over_tau_runs():
    from cca_zoo_amd.linear import SCCA_ADMM
    from cca_zoo_amd.model_selection import GridSearchCV

    g = load_golden("admm_tall2")
    gs = GridSearchCV(SCCA_ADMM(latent_dimensions=2, max_iter=30, random_state=0), {"tau": [0.3, 0.6, 0.9]}, cv=2)
    gs.fit(case_views(g))
    assert gs.best_params_["tau"] in (0.3, 0.6, 0.9)
    assert np.all(np.isfinite(gs.best_estimator_.weights_[0]))
