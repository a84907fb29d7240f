"""GPU tests of PLS_ALS / SCCA_PMD / ParkhomenkoCCA / SCCA_Span: every kernel against NumPy float64 through the C ABI,
every golden case through the estimators (host arrays and CUDA tensors), determinism, guards, a width no Gram route
takes, and a grid search."""

import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from test_als_host import CASES, apply_rule, case_params, case_views, col_err, restate, support

pytestmark = pytest.mark.gpu

W_TOL = 1e-8          # per-column relative error of weights_, fp64 AND fp32 views (both compute in fp64)
PEEK = {"w": 0, "raw": 1, "score": 2, "target": 3, "Q": 4, "level": 5}
RULES = {"pls": 0, "parkhomenko": 1, "pmd": 2, "span": 3}


def _classes():
    from cca_zoo_amd.linear import PLS_ALS, SCCA_PMD, SCCA_Span, ParkhomenkoCCA

    return {"PLS_ALS": PLS_ALS, "SCCA_PMD": SCCA_PMD, "ParkhomenkoCCA": ParkhomenkoCCA, "SCCA_Span": SCCA_Span}


def _model(g, **over):
    p = case_params(g)
    p.update(over)
    return _classes()[str(g["model"])](**p)


# ---- kernels through the C ABI --------------------------------------------------------------------------------------
class _Fit:
    """A raw fit state on rows uploaded to the device.  ``pad``: extra elements per row (ld = p + pad) filled with
    ``pad_value``; ``offset``: the view starts this many elements into its buffer (base pointer 4 or 8 bytes off a
    16-byte boundary for float32, 8 for float64); ``means``: "auto", None (``means_dev == NULL``) or a list whose None
    entries become NULL entries."""

    def __init__(self, views, k, rule, par, tol=0.0, max_iter=1, chunk=4, pad=0, offset=0, means="auto", pad_value=1e30):
        from cca_zoo_amd import _backend

        self.h = h = _backend.default_handle()
        self.m, self.k = len(views), k
        self.p = [v.shape[1] for v in views]
        self.n = views[0].shape[0]
        f32 = views[0].dtype == np.float32
        if isinstance(means, str):
            means = [v.mean(axis=0).astype(v.dtype) for v in views]
        self.means = means
        self.bufs, self.mbufs = [], []
        self.varr = (_backend.View * self.m)()
        for i, v in enumerate(views):
            ld = v.shape[1] + pad
            padded = np.full((v.shape[0], ld), pad_value, dtype=v.dtype)
            padded[:, : v.shape[1]] = v
            flat = np.concatenate([np.full(offset, pad_value, dtype=v.dtype), padded.reshape(-1)])
            b = h.to_device(flat)
            self.bufs.append(b)
            self.varr[i].data, self.varr[i].cols, self.varr[i].ld = b.ptr + offset * v.dtype.itemsize, v.shape[1], ld
            if means is not None:
                self.mbufs.append(None if means[i] is None else h.to_device(np.asarray(means[i], dtype=v.dtype)))
        self.marr = (C.c_void_p * self.m)(*[None if b is None else b.ptr for b in self.mbufs]) if means is not None else None
        self.state = C.c_void_p()
        h.check(h.lib.ccz_als_create(h.raw, _backend.F32 if f32 else _backend.F64, self.m, (C.c_int64 * self.m)(*self.p),
                                     self.n, k, rule, (C.c_double * self.m)(*[float(x) for x in par]), tol, max_iter, chunk,
                                     C.byref(self.state)))
        # the rows the device multiplies: fl(x - mu) in the views' dtype, as float64
        self.xs = [(v if means is None or means[i] is None else v - np.asarray(means[i], dtype=v.dtype)).astype(np.float64)
                   for i, v in enumerate(views)]

    def set_init(self, w0):
        a = np.ascontiguousarray(w0, dtype=np.float64)
        assert a.shape == (self.k, sum(self.p))
        self.h.check(self.h.lib.ccz_als_set_init(self.h.raw, self.state, a.ctypes.data_as(C.POINTER(C.c_double))))

    def sweeps(self, s):
        a, b = C.c_int64(0), C.c_int(0)
        self.h.check(self.h.lib.ccz_als_sweeps(self.h.raw, self.state, self.varr, self.marr, s, C.byref(a), C.byref(b)))
        return a.value, b.value

    def peek(self, what, view):
        size = {"w": self.p[view], "raw": self.p[view], "score": self.n, "target": self.n, "Q": self.k * self.n,
                "level": 2}[what]
        out = np.empty(size)
        self.h.check(self.h.lib.ccz_als_peek(self.h.raw, self.state, PEEK[what], view, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out.reshape(self.k, self.n) if what == "Q" else out

    def status(self):
        d, s = C.c_int(0), C.c_int(0)
        it, dl = (C.c_int64 * self.k)(), (C.c_double * self.k)()
        self.h.check(self.h.lib.ccz_als_status(self.h.raw, self.state, C.byref(d), C.byref(s), it, dl))
        return d.value, s.value, list(it), list(dl)

    def weights(self):
        out = np.empty(sum(self.p) * self.k)
        self.h.check(self.h.lib.ccz_als_get_weights(self.h.raw, self.state, out.ctypes.data_as(C.POINTER(C.c_double))))
        return np.split(out.reshape(-1, self.k), np.cumsum(self.p)[:-1])

    def close(self):
        self.h.check(self.h.lib.ccz_als_destroy(self.h.raw, self.state))


def _init(rng, p, k):
    w = rng.standard_normal((k, sum(p)))
    off = 0
    for pi in p:
        w[:, off:off + pi] /= np.linalg.norm(w[:, off:off + pi], axis=1, keepdims=True)
        off += pi
    return w


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


# dims, n, k, pad, offset, means: p not a multiple of 4 or of the 1024-column strip, ld > p with poisoned padding, base
# pointers off a 16-byte boundary, NULL means and NULL entries, n not a multiple of the 4-row tile, k = 1 and k = 3 (Q
# non-empty), a view wide enough for two column splits of the score kernel (9001 columns at 37 rows)
SHAPES = [
    ((5, 3), 9, 1, 0, 0, "auto"),
    ((37, 21), 50, 1, 3, 0, "auto"),
    ((1030, 517), 41, 3, 2, 0, "auto"),
    ((1024, 2049, 70), 64, 3, 0, 0, "one_null"),
    ((130, 64), 33, 1, 1, 1, "auto"),
    ((131, 66), 35, 3, 0, 2, "none"),
    ((9001, 300), 37, 3, 3, 0, "auto"),
    ((9000, 4100), 18, 1, 0, 1, "one_null"),
]


def _shape_fit(shape, dtype, rule="pls", par=None, max_iter=1):
    dims, n, k, pad, offset, meanmode = shape
    rng = np.random.default_rng(len(dims) * 1000 + n)
    z = rng.standard_normal((n, 2))
    views = [((z @ rng.standard_normal((2, d)) + rng.standard_normal((n, d))) / np.sqrt(n) + 0.5).astype(dtype) for d in dims]
    means = "auto"
    if meanmode == "none":
        means = None
    elif meanmode == "one_null":
        means = [v.mean(axis=0).astype(dtype) for v in views]
        means[len(dims) // 2] = None
    par = [0.0] * len(dims) if par is None else par
    fit = _Fit(views, k, RULES[rule], par, max_iter=max_iter, pad=pad, offset=offset, means=means)
    fit.set_init(_init(rng, list(dims), k))
    return fit


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{'x'.join(map(str, s[0]))}_n{s[1]}_k{s[2]}" for s in SHAPES])
def test_score_target_and_xt_kernels(shape, dtype):
    """One sweep per dimension (max_iter = 1), so after all k sweeps the buffers hold the LAST dimension's last update
    with k - 1 columns in every Q: each buffer is recomputed in NumPy float64 from the buffers it was made from."""
    dims, n, k = shape[0], shape[1], shape[2]
    fit = _shape_fit(shape, dtype)
    try:
        fit.sweeps(k)
        done, stopped, iters, _ = fit.status()
        assert (done, stopped, iters) == (k, 1, [1] * k)
        m = len(dims)
        Q = [fit.peek("Q", i)[: k - 1].T for i in range(m)]                 # the columns that were in use
        s = [fit.peek("score", i) for i in range(m)]
        w = [fit.peek("w", i) for i in range(m)]
        for i in range(m):
            # score kernel alone: the uncorrected score of the current vector
            err = _rel(s[i], fit.xs[i] @ w[i])
            print(f"score {np.dtype(dtype).name} {dims} view {i}: {err:.2e}")
            assert err <= 1e-12
            if k > 1:
                assert np.max(np.abs(Q[i].T @ Q[i] - np.eye(k - 1))) <= 1e-10   # orthonormal scores
        # prologue alone: the target of the last view from the scores of the others
        sc = [s[j] - Q[j] @ (Q[j].T @ s[j]) for j in range(m)]
        t = sum(sc[j] for j in range(m - 1))
        t = t / np.linalg.norm(t)
        t = t - Q[m - 1] @ (Q[m - 1].T @ t)
        tt = fit.peek("target", m - 1)
        assert _rel(tt, t) <= 1e-12
        # xt kernel + fold alone: raw of the last view from the device's own target
        raw = fit.peek("raw", m - 1)
        err = _rel(raw, fit.xs[m - 1].T @ tt)
        print(f"xt {np.dtype(dtype).name} {dims}: {err:.2e}")
        assert err <= 1e-12
        # the last column of every Q: the corrected score over its norm
        Qk = [fit.peek("Q", i)[k - 1] for i in range(m)]
        for i in range(m):
            assert _rel(Qk[i], sc[i] / np.linalg.norm(sc[i])) <= 1e-11
        # finished columns: the last one is the current vector
        for i, wi in enumerate(fit.weights()):
            np.testing.assert_array_equal(wi[:, k - 1], w[i])
    finally:
        fit.close()


RULE_CASES = [  # rule, parameter as a function of (raw, p)
    ("pls", lambda raw, p: 0.0),
    ("parkhomenko", lambda raw, p: 0.3 * np.max(np.abs(raw))),
    ("parkhomenko", lambda raw, p: 2.0 * np.max(np.abs(raw))),                  # everything thresholded: the 1e-12 guard
    ("pmd", lambda raw, p: 0.35 * np.sum(np.abs(raw))),                         # bisection
    ("pmd", lambda raw, p: 1e-2 * np.max(np.abs(raw))),                         # bisection down to one or two entries
    ("pmd", lambda raw, p: 1.5 * np.sum(np.abs(raw))),                          # within the bound: no thresholding
    ("span", lambda raw, p: 1.0),
    ("span", lambda raw, p: float(max(1, p // 3))),
    ("span", lambda raw, p: float(p - 1)),
    ("span", lambda raw, p: float(p + 5)),                                      # s >= p: everything kept
]


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[6]], ids=["37x21", "1030x517", "9001x300"])
@pytest.mark.parametrize("rc", range(len(RULE_CASES)), ids=[f"{r[0]}{i}" for i, r in enumerate(RULE_CASES)])
def test_rule_kernels(shape, rc):
    """Every rule alone: a first fit with plain normalisation gives the device's ``raw`` of each view's first update (it
    does not depend on the rule for view 0; for later views the check uses the peeked raw of THIS fit); the rule's
    parameter is placed relative to it; the vector the rule made is compared with NumPy on the same ``raw``."""
    rule, parfn = RULE_CASES[rc]
    dims = shape[0]
    probe = _shape_fit(shape, np.float64, max_iter=2)
    try:
        probe.sweeps(1)
        raws = [probe.peek("raw", i) for i in range(len(dims))]
    finally:
        probe.close()
    par = [parfn(r, len(r)) for r in raws]
    fit = _shape_fit(shape, np.float64, rule=rule, par=par, max_iter=2)
    try:
        fit.sweeps(1)
        for i in range(len(dims)):
            raw, w = fit.peek("raw", i), fit.peek("w", i)
            ref, thr = apply_rule(rule, raw, par[i])
            level, applied = fit.peek("level", i)
            if rule == "pmd":
                assert applied == (0.0 if thr is None else 1.0)
            if rule == "pmd" and thr is not None:
                # The level itself.  The reference's 50 halvings end on an interval max|raw| 2^-50 wide and return its
                # middle, so its level is within 2^-51 max|raw| of the root of |soft(raw, t)|_1 = bound, up to the
                # rounding of the L1 sums: a halving whose sum lies within that rounding of the bound may go either
                # way, on the device (another order of summation) as in NumPy.  A pairwise or tree sum of nnz kept entries
                # carries an error of at most log2(nnz) 2^-53 of itself (14 x 2^-53 for the 9001 columns here), the sum is
                # at most nnz max|raw| and falls with slope nnz, so the root moves by at most 1.75 x 2^-50 max|raw|.  Two
                # such levels differ by at most 2 (2^-51 + 1.75 x 2^-50) max|raw| = 4.5 x 2^-50 max|raw| = 4e-15 max|raw|,
                # the "about 1e-15" the contract names.
                mx = float(np.max(np.abs(raw)))
                print(f"pmd level view {i}: device {level:.17g} reference {thr:.17g} diff/max {abs(level - thr) / mx:.2e}")
                assert abs(level - thr) <= 4.5 * 2.0 ** -50 * mx, (i, level, thr)
                # the level is pinned to the bisection's last interval (max|raw| 2^-50 wide), not bit for bit: an absolute
                # error of ~2e-15 max|raw| in every kept entry against a kept norm of >= 1e-2 max|raw| / sqrt(p) is below
                # 1e-10 of the largest entry of w for every p here
                np.testing.assert_array_equal(w != 0, ref != 0)
                assert _rel(w, ref) <= 1e-10, (rule, i, _rel(w, ref))
            else:
                np.testing.assert_array_equal(w != 0, ref != 0)
                assert _rel(w, ref) <= 1e-14, (rule, i, _rel(w, ref))
            if rule == "span" and par[i] < len(raw):
                assert np.count_nonzero(w) == int(par[i])
                assert (level, applied) == (thr, 1.0)                    # the exact s-th largest magnitude
    finally:
        fit.close()


def test_span_keeps_ties_at_the_threshold():
    rng = np.random.default_rng(3)
    n, p = 30, 40
    x = rng.standard_normal((n, p))
    x[:, 17] = -x[:, 5]
    y = rng.standard_normal((n, 6))
    w0 = _init(rng, [p, 6], 1)
    xs = [x - x.mean(axis=0), y - y.mean(axis=0)]
    t = xs[1] @ w0[0, p:]
    raw = xs[0].T @ (t / np.linalg.norm(t))
    s = int(np.sum(np.abs(raw) > abs(raw[5]))) + 1            # the pair sits at ranks s and s + 1
    fit = _Fit([x, y], 1, RULES["span"], [float(s), 6.0], max_iter=2)
    try:
        fit.set_init(w0)
        fit.sweeps(1)
        w, dev_raw = fit.peek("w", 0), fit.peek("raw", 0)
        assert abs(dev_raw[5]) == abs(dev_raw[17])            # equal columns give equal sums on the device
        assert np.count_nonzero(w) == s + 1 and w[5] != 0 and w[17] != 0
    finally:
        fit.close()


def test_stop_inside_a_chunk_and_later_sweeps_are_no_ops():
    g = load_golden("als_pls2")
    views = case_views(g)
    p = [v.shape[1] for v in views]
    from cca_zoo_amd.linear._iterative import initial_vectors

    want = [int(s) for s in g["n_iter"]]
    fit = _Fit(views, 2, RULES["pls"], [0.0, 0.0], tol=1e-6, max_iter=500, chunk=8, pad_value=0.0)
    try:
        fit.set_init(initial_vectors(1, p, 2))
        total = 0
        while total < sum(want) + 16:
            fit.sweeps(8)
            total += 8
        done, stopped, iters, deltas = fit.status()
        assert (done, stopped, iters) == (2, 1, want)
        np.testing.assert_allclose(deltas, g["last_delta"], rtol=1e-5)
        known, stop_known = fit.sweeps(0)
        assert stop_known == 1 and known == sum(want)
        for i, w in enumerate(fit.weights()):
            assert col_err(w, g[f"W{i}"]) <= W_TOL
    finally:
        fit.close()


# ---- the reference's fits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["host", "cuda"])
@pytest.mark.parametrize("case", CASES)
def test_golden_case(case, source):
    g = load_golden(f"als_{case}")
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
    assert model.n_iter_ == [int(s) for s in g["n_iter"]]
    for i, w in enumerate(model.weights_):
        ref = g[f"W{i}"]
        assert w.dtype == np.float64
        assert model.means_[i].dtype == g[f"mean{i}"].dtype
        err = col_err(w, ref)
        print(f"golden {case} ({source}) view {i}: weights col err {err:.2e}")
        assert err <= W_TOL, (i, err)
        for a, b in zip(support(w), support(ref)):
            np.testing.assert_array_equal(a, b)
    np.testing.assert_allclose(model.score(case_views(g, "T")), g["score_test"], atol=1e-3 if f32 else 1e-7)
    for i, z in enumerate(model.transform(case_views(g, "T"))):
        assert col_err(z, g[f"Zt{i}"]) <= (1e-3 if f32 else 1e-7)


@pytest.mark.parametrize("case", ["pmd3_perview", "span_wide_f32", "park_f32_perview"])
def test_two_fits_are_bit_identical(case):
    g = load_golden(f"als_{case}")
    a = _model(g).fit(case_views(g))
    b = _model(g).fit(case_views(g))
    assert a.n_iter_ == b.n_iter_
    for x, y in zip(a.weights_, b.weights_):
        np.testing.assert_array_equal(x, y)


def test_max_iter_is_reached():
    g = load_golden("als_pls_maxiter")
    model = _model(g).fit(case_views(g))
    assert model.n_iter_ == [case_params(g)["max_iter"]] * 2
    assert all(d >= 1e-6 for d in model.last_delta_)


def test_zero_view_exercises_the_guards():
    """A zero view: its scores vanish, so the other view's target keeps norm 0 (no normalisation), raw = 0, the result
    is not normalised and nothing is deflated -- zeros throughout, as the reference gives, and no NaN."""
    from cca_zoo_amd.linear import PLS_ALS, ParkhomenkoCCA

    rng = np.random.default_rng(0)
    X, Z = rng.standard_normal((40, 7)), np.zeros((40, 5))
    for cls in (PLS_ALS, ParkhomenkoCCA):
        model = cls(latent_dimensions=2, max_iter=5, random_state=0).fit([X, Z])
        W, sweeps, _ = restate([X, Z], cls.__name__, latent_dimensions=2, max_iter=5, random_state=0)
        assert model.n_iter_ == sweeps
        for w, r in zip(model.weights_, W):
            assert np.all(np.isfinite(w))
            np.testing.assert_allclose(w, r, atol=1e-12)
        assert np.all(model.weights_[0] == 0)


def test_span_zero_keeps_every_entry():
    """``span=0``: the reference's ``np.sort(np.abs(raw))[-0]`` is the smallest magnitude, so nothing is dropped."""
    from cca_zoo_amd.linear import SCCA_Span

    g = load_golden("als_span2")
    views = case_views(g)
    a = SCCA_Span(latent_dimensions=2, span=0, max_iter=20, random_state=1).fit(views)
    b = SCCA_Span(latent_dimensions=2, span=[v.shape[1] for v in views], max_iter=20, random_state=1).fit(views)
    W, sweeps, _ = restate(views, "SCCA_Span", latent_dimensions=2, span=[v.shape[1] for v in views], max_iter=20,
                           random_state=1)
    assert a.n_iter_ == b.n_iter_ == sweeps
    for x, y, r in zip(a.weights_, b.weights_, W):
        np.testing.assert_array_equal(x, y)
        assert np.all(x != 0) and col_err(x, r) <= W_TOL


def test_latent_dimensions_give_orthogonal_scores():
    from cca_zoo_amd.linear import PLS_ALS

    g = load_golden("als_pls3")
    views = case_views(g)
    model = PLS_ALS(latent_dimensions=3, random_state=2).fit(views)
    # dimension d's weights act on the deflated views: scores of the DEFLATED views are orthogonal across dimensions
    W, _, _ = restate(views, "PLS_ALS", latent_dimensions=3, random_state=2)
    for i, v in enumerate(views):
        x = v - v.mean(axis=0)
        S = []
        for d in range(3):
            s = x @ model.weights_[i][:, d]
            S.append(s / np.linalg.norm(s))
            x = x - np.outer(S[-1], S[-1] @ x)
        G = np.array(S) @ np.array(S).T
        assert np.max(np.abs(G - np.eye(3))) <= 1e-8
        assert col_err(model.weights_[i], W[i]) <= W_TOL


def test_wide_pmd_matches_the_comparator():
    """n = 2048, 2 x 200 000 float32 features, SCCA_PMD, k = 2: a width no Gram route takes, against the NumPy
    restatement on the same data."""
    from cca_zoo_amd.linear import SCCA_PMD

    n, p, k = 2048, 200000, 2
    rng = np.random.default_rng(5)
    z = rng.standard_normal((n, k)).astype(np.float32)
    views = []
    for i in range(2):
        x = rng.standard_normal((n, p), dtype=np.float32)
        for a in range(k):
            cols = rng.choice(p, 300, replace=False)
            x[:, cols] += (2.0 - 0.5 * a) * z[:, a:a + 1]
        x *= np.float32(0.01)
        x += rng.uniform(-0.01, 0.01, p).astype(np.float32)
        views.append(x)
    params = dict(latent_dimensions=k, tau=0.05, max_iter=6, tol=1e-6, random_state=2)
    model = SCCA_PMD(**params).fit(views)
    W, sweeps, _ = restate(views, "SCCA_PMD", **params)
    assert model.n_iter_ == sweeps
    for i in range(2):
        err = col_err(model.weights_[i], W[i])
        nnz = [int(np.count_nonzero(model.weights_[i][:, d])) for d in range(k)]
        print(f"wide PMD view {i}: col err {err:.2e}, support sizes {nnz}, sweeps {sweeps}")
        assert err <= W_TOL
        assert all(1 < c < p for c in nnz)
        for a, b in zip(support(model.weights_[i]), support(W[i])):
            assert len(np.setxor1d(a, b)) == 0


def test_grid_search_over_tau_runs():
    from cca_zoo_amd.linear import SCCA_PMD
    from cca_zoo_amd.model_selection import GridSearchCV

    g = load_golden("als_pmd2")
    gs = GridSearchCV(SCCA_PMD(latent_dimensions=2, max_iter=30, random_state=0), {"tau": [0.3, 0.6, 0.9]}, cv=2)
    gs.fit(case_views(g))
    assert gs.best_params_["tau"] in (0.3, 0.6, 0.9)
    assert np.all(np.isfinite(gs.best_estimator_.weights_[0]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_column_means_equal_numpy_bit_for_bit(dtype):
    """CUDA-tensor fits centre with ``ccz_als_colmeans``: rows added in order in the input precision, as ``v.mean(0)``."""
    import torch

    from cca_zoo_amd import _backend

    h = _backend.default_handle()
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((3000, 517)) + 0.7).astype(dtype)
    t = torch.as_tensor(np.concatenate([x, np.full((3000, 3), 1e30, dtype=dtype)], axis=1), device="cuda")
    out = torch.empty(517, dtype=t.dtype, device="cuda")
    torch.cuda.synchronize()
    view = _backend.View()
    view.data, view.cols, view.ld = t.data_ptr(), 517, t.stride(0)
    h.check(h.lib.ccz_als_colmeans(h.raw, _backend.F32 if dtype == np.float32 else _backend.F64, C.byref(view), 3000,
                                   C.c_void_p(out.data_ptr())))
    h.sync()
    np.testing.assert_array_equal(out.cpu().numpy(), x.mean(axis=0))
