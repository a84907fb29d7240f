"""GPU tests of the sparse-view kernels of the ALS family (CSR score, CSC X' t~, means, projection) through the C ABI:
every buffer against float64 NumPy / scipy recomputed from the device's own inputs, at the dense float64 kernels' own
bars; float32 against float64 values, two fits, chunk lengths and the stop inside a chunk exactly."""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

PEEK = {"w": 0, "raw": 1, "score": 2, "target": 3, "Q": 4, "level": 5}
RULES = {"pls": 0, "parkhomenko": 1, "pmd": 2, "span": 3}


def _sparse(rng, n, p, density, full_row=None, full_col=None, empty_rows=(), empty_cols=()):
    """Non-negative float32-representable values where a Bernoulli mask is set, as float64 CSR."""
    a = np.where(rng.random((n, p)) < density, np.abs(rng.standard_normal((n, p))) + 0.25, 0.0)
    if full_row is not None:
        a[full_row] = np.abs(rng.standard_normal(p)) + 0.25
    if full_col is not None:
        a[:, full_col] = np.abs(rng.standard_normal(n)) + 0.25
    a[list(empty_rows)] = 0.0
    a[:, list(empty_cols)] = 0.0
    return sp.csr_matrix(a.astype(np.float32).astype(np.float64))


def _dense(rng, n, p):
    return ((rng.standard_normal((n, p)) + 0.5).astype(np.float32)).astype(np.float64)


# name -> (views of (kind, p, kwargs), n, k)
CASES = {
    "5x3_half_full": ([("s", 5, dict(density=0.5)), ("s", 3, dict(density=0.5))], 9, 1),
    "37x21": ([("s", 37, dict(density=0.3)), ("s", 21, dict(density=0.3))], 50, 1),
    "1030x517_k3": ([("s", 1030, dict(density=0.05)), ("s", 517, dict(density=0.05))], 41, 3),
    "9001x300_k3": ([("s", 9001, dict(density=0.01)), ("s", 300, dict(density=0.01))], 37, 3),
    "2049x64_full_row_and_column": ([("s", 2049, dict(density=0.02, full_row=7, full_col=11)),
                                     ("s", 64, dict(density=0.02, full_row=7, full_col=11))], 64, 1),
    "nnz0": ([("s", 7, dict(density=0.4)), ("s", 5, dict(density=0.0))], 12, 2),
    "empty_edges": ([("s", 37, dict(density=0.3, empty_rows=(0, 49), empty_cols=(36,))),
                     ("s", 21, dict(density=0.3, empty_rows=(0, 49), empty_cols=(20,)))], 50, 3),
    "mixed_sparse_dense": ([("s", 37, dict(density=0.3)), ("d", 21, {})], 50, 3),
}


def _case_views(name):
    spec, n, k = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    views = [_sparse(rng, n, p, **kw) if kind == "s" else _dense(rng, n, p) for kind, p, kw in spec]
    return views, n, k, rng


def _init(rng, p, k):
    w = rng.standard_normal((k, sum(p)))
    off = 0
    for pi in p:
        w[:, off:off + pi] /= np.linalg.norm(w[:, off:off + pi], axis=1, keepdims=True)
        off += pi
    return w


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


class _Fit:
    """A raw fit state whose sparse views go through ccz_als_set_sparse.  ``views``: float64 CSR matrices and dense
    arrays holding float32-representable numbers, uploaded as ``dtype``; ``means``: "centred", "none" (``means_dev ==
    NULL``) or "one_null" (the middle view's entry NULL)."""

    def __init__(self, views, dtype, k, rule="pls", par=None, tol=0.0, max_iter=1, chunk=4, means="centred"):
        from cca_zoo_amd import _backend
        from cca_zoo_amd._utils._resident import DeviceSparse, canonical_forms

        self.h = h = _backend.default_handle()
        self.m, self.k, self.n = len(views), k, views[0].shape[0]
        self.p = [v.shape[1] for v in views]
        self.views = views
        self.sparse = [sp.issparse(v) for v in views]
        code = _backend.F32 if dtype == np.float32 else _backend.F64
        centred = [means != "none" and not (means == "one_null" and i == self.m // 2) for i in range(self.m)]
        self.keep, self.sarr, self.mu = [], [], []
        self.varr = (_backend.View * self.m)()
        mptr = []
        for i, v in enumerate(views):
            self.varr[i].cols, self.varr[i].ld = self.p[i], self.p[i]
            if self.sparse[i]:
                sv = DeviceSparse(h, *canonical_forms(v, dtype))
                self.sarr.append(sv)
                mu = None
                if centred[i]:
                    mb = h.alloc(self.p[i] * 8)
                    h.check(h.lib.ccz_sparse_colmeans(h.raw, code, C.byref(sv.view), C.c_void_p(mb.ptr)))
                    mu = h.to_host(mb, (self.p[i],))            # the device's own means: float64
                    self.keep.append(mb)
                    mptr.append(mb.ptr)
                else:
                    mptr.append(None)
            else:
                self.sarr.append(None)
                x = v.astype(dtype)
                b = h.to_device(x)
                self.keep.append(b)
                self.varr[i].data = b.ptr
                mu = None
                if centred[i]:
                    mu = x.mean(axis=0)
                    mb = h.to_device(mu)
                    self.keep.append(mb)
                    mptr.append(mb.ptr)
                    self.views[i] = (x - mu).astype(np.float64)     # the rows the dense kernels multiply: fl(x - mu)
                    mu = np.zeros(self.p[i])
                else:
                    mptr.append(None)
            self.mu.append(np.zeros(self.p[i]) if mu is None else np.asarray(mu, dtype=np.float64))
        self.marr = (C.c_void_p * self.m)(*mptr) if means != "none" else None
        self.state = C.c_void_p()
        par = [0.0] * self.m if par is None else par
        h.check(h.lib.ccz_als_create(h.raw, code, self.m, (C.c_int64 * self.m)(*self.p), self.n, k, RULES[rule],
                                     (C.c_double * self.m)(*[float(x) for x in par]), tol, max_iter, chunk, C.byref(self.state)))
        for i, sv in enumerate(self.sarr):
            if sv is not None:
                h.check(h.lib.ccz_als_set_sparse(h.raw, self.state, i, C.byref(sv.view)))

    # float64 references on the device's own inputs
    def xw(self, i, w):
        return self.views[i] @ w - self.mu[i] @ w

    def xt(self, i, t):
        return self.views[i].T @ t - self.mu[i] * np.sum(t)

    def set_init(self, w0):
        a = np.ascontiguousarray(w0, dtype=np.float64)
        assert a.shape == (self.k, sum(self.p))
        self.h.check(self.h.lib.ccz_als_set_init(self.h.raw, self.state, a.ctypes.data_as(C.POINTER(C.c_double))))

    def sweeps(self, s):
        a, b = C.c_int64(0), C.c_int(0)
        self.h.check(self.h.lib.ccz_als_sweeps(self.h.raw, self.state, self.varr, self.marr, s, C.byref(a), C.byref(b)))
        return a.value, b.value

    def peek(self, what, view):
        size = {"w": self.p[view], "raw": self.p[view], "score": self.n, "target": self.n, "Q": self.k * self.n, "level": 2}[what]
        out = np.empty(size)
        self.h.check(self.h.lib.ccz_als_peek(self.h.raw, self.state, PEEK[what], view, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out.reshape(self.k, self.n) if what == "Q" else out

    def everything(self):
        out = {}
        for i in range(self.m):
            for what in ("w", "raw", "score", "Q", "level"):
                out[what, i] = self.peek(what, i)
        out["target"] = self.peek("target", 0)
        out["status"] = self.status()
        out["weights"] = np.concatenate(self.weights())
        return out

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


def _case_fit(name, dtype, means="centred", **kw):
    views, n, k, rng = _case_views(name)
    fit = _Fit(views, dtype, k, means=means, **kw)
    fit.set_init(_init(rng, fit.p, k))
    return fit


def _unit(v):
    """v over its norm under the reference's guards: |v| > 1e-12 for a target, |v|^2 > 1e-12 (else zeros) for a Q column."""
    return v / np.linalg.norm(v) if np.linalg.norm(v) > 1e-12 else v


@pytest.mark.parametrize("means", ["centred", "none", "one_null"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(CASES))
def test_score_target_and_xt_kernels(name, dtype, means):
    """As the dense test of the same name: max_iter = 1 and k sweeps, so the buffers hold the last dimension's last update
    with k - 1 columns in every Q; each is recomputed in float64 from the buffers it was made from."""
    fit = _case_fit(name, dtype, means)
    k, m, n = fit.k, fit.m, fit.n
    try:
        # the means of the sparse views: float64, (sum of the stored entries of a column) / n
        for i in range(m):
            if fit.sparse[i] and np.any(fit.mu[i]):
                err = _rel(fit.mu[i], np.asarray(fit.views[i].sum(axis=0)).ravel() / n)
                print(f"colmeans {name} view {i}: {err:.2e}")
                assert err <= 1e-12
        fit.sweeps(k)
        done, stopped, iters, _ = fit.status()
        assert (done, stopped, iters) == (k, 1, [1] * k)
        Q = [fit.peek("Q", i)[: k - 1].T for i in range(m)]
        s = [fit.peek("score", i) for i in range(m)]
        w = [fit.peek("w", i) for i in range(m)]
        for i in range(m):
            assert np.all(np.isfinite(s[i])) and np.all(np.isfinite(w[i]))
            err = _rel(s[i], fit.xw(i, w[i]))
            print(f"score {name} {np.dtype(dtype).name} {means} view {i}: {err:.2e}")
            assert err <= 1e-12
        sc = [s[j] - Q[j] @ (Q[j].T @ s[j]) for j in range(m)]
        t = _unit(sum(sc[j] for j in range(m - 1)))
        t = t - Q[m - 1] @ (Q[m - 1].T @ t)
        tt = fit.peek("target", m - 1)
        assert _rel(tt, t) <= 1e-12
        raw = fit.peek("raw", m - 1)
        err = _rel(raw, fit.xt(m - 1, tt))
        print(f"xt {name} {np.dtype(dtype).name} {means}: {err:.2e}")
        assert err <= 1e-12
        for i in range(m):
            want = sc[i] / np.linalg.norm(sc[i]) if sc[i] @ sc[i] > 1e-12 else np.zeros(n)
            assert _rel(fit.peek("Q", i)[k - 1], want) <= 1e-11
        for i, wi in enumerate(fit.weights()):
            np.testing.assert_array_equal(wi[:, k - 1], w[i])
        if name == "nnz0":       # the 1e-12 guards: zeros throughout, no NaN
            assert np.all(w[0] == 0) and np.all(raw == 0) and np.all(tt == 0)
    finally:
        fit.close()


def test_group_width_of_the_cases():
    """The cases cover G = 4 (short lines), a G between, and 64 with more than one pass of the lane loop."""
    from cca_zoo_amd._utils._resident import sparse_group

    seen = set()
    for name in CASES:
        views, n, _, _ = _case_views(name)
        for v in views:
            if sp.issparse(v):
                seen |= {sparse_group(v.nnz, v.shape[0]), sparse_group(v.nnz, v.shape[1])}
    assert {4, 64} <= seen and seen & {8, 16, 32}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("k", [1, 3, 11, 32])
@pytest.mark.parametrize("centre", [True, False])
@pytest.mark.parametrize("name", ["1030x517_k3", "2049x64_full_row_and_column", "empty_edges", "nnz0"])
def test_sparse_project(name, k, centre, dtype):
    from cca_zoo_amd import _backend
    from cca_zoo_amd._utils._resident import DeviceSparse, canonical_forms

    h = _backend.default_handle()
    views, n, _, rng = _case_views(name)
    for v in views:
        p = v.shape[1]
        W = rng.standard_normal((p, k))
        mu = rng.standard_normal(p)
        sv = DeviceSparse(h, canonical_forms(v, dtype, csc=False)[0])
        wd, md, od = h.to_device(W), h.to_device(mu), h.alloc(n * k * 8)
        h.check(h.lib.ccz_sparse_project(h.raw, _backend.F32 if dtype == np.float32 else _backend.F64, C.byref(sv.view),
                                         C.c_void_p(md.ptr) if centre else None, C.c_void_p(wd.ptr), k, C.c_void_p(od.ptr)))
        z = h.to_host(od, (n, k))
        ref = v @ W - (mu @ W if centre else 0.0)
        err = _rel(z, ref)
        print(f"project {name} p={p} k={k} centre={centre}: {err:.2e}")
        assert err <= 1e-12


def test_abi_refusals():
    from cca_zoo_amd import _backend
    from cca_zoo_amd._utils._resident import DeviceSparse, canonical_forms

    h = _backend.default_handle()
    views, n, k, _ = _case_views("37x21")
    sv = DeviceSparse(h, *canonical_forms(views[0], np.float64))
    for rule in (4, 5):      # CCZ_ALS_ADMM, CCZ_ALS_ENET need the Gram of a view
        state = C.c_void_p()
        h.check(h.lib.ccz_als_create(h.raw, _backend.F64, 2, (C.c_int64 * 2)(37, 21), n, 1, rule, (C.c_double * 2)(0.1, 0.1),
                                     1e-6, 5, 4, C.byref(state)))
        try:
            with pytest.raises(ValueError, match="sparse"):
                h.check(h.lib.ccz_als_set_sparse(h.raw, state, 0, C.byref(sv.view)))
        finally:
            h.check(h.lib.ccz_als_destroy(h.raw, state))
    state = C.c_void_p()
    h.check(h.lib.ccz_als_create(h.raw, _backend.F64, 2, (C.c_int64 * 2)(37, 21), n, 1, 0, None, 1e-6, 5, 4, C.byref(state)))
    try:
        with pytest.raises(ValueError, match="50 x 37"):      # view 1 of the state is 50 x 21
            h.check(h.lib.ccz_als_set_sparse(h.raw, state, 1, C.byref(sv.view)))
        with pytest.raises(ValueError):
            h.check(h.lib.ccz_als_set_sparse(h.raw, state, 2, C.byref(sv.view)))
        h.check(h.lib.ccz_als_set_sparse(h.raw, state, 0, C.byref(sv.view)))
        h.check(h.lib.ccz_als_set_sparse(h.raw, state, 0, None))          # dense again
    finally:
        h.check(h.lib.ccz_als_destroy(h.raw, state))


# ---- exact ----------------------------------------------------------------------------------------------------------
def _assert_same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        if key == "status":
            assert a[key] == b[key]
        else:
            np.testing.assert_array_equal(a[key], b[key], err_msg=str(key))


@pytest.mark.parametrize("means", ["centred", "none"])
@pytest.mark.parametrize("name", ["1030x517_k3", "9001x300_k3", "2049x64_full_row_and_column", "empty_edges"])
def test_float32_and_float64_values_give_the_same_bits(name, means):
    """No x - mu element is formed and a value is widened exactly, so the precision of the stored values cannot show."""
    out = []
    for dtype in (np.float32, np.float64):
        fit = _case_fit(name, dtype, means)
        try:
            fit.sweeps(fit.k)
            out.append(fit.everything())
        finally:
            fit.close()
    _assert_same(*out)


def _run(name, rule, par, chunk, extra=0):
    fit = _case_fit(name, np.float32, rule=rule, par=par, tol=1e-6, max_iter=12, chunk=chunk)
    try:
        total = 0
        while total < fit.k * 12 + extra:
            fit.sweeps(chunk)
            total += chunk
        return fit.everything()
    finally:
        fit.close()


@pytest.mark.parametrize("name,rule,par", [("1030x517_k3", "pls", None), ("9001x300_k3", "span", [40.0, 25.0]),
                                           ("mixed_sparse_dense", "pls", None)])
def test_two_fits_and_chunk_lengths_give_the_same_bits(name, rule, par):
    a = _run(name, rule, par, 8)
    assert a["status"][:2] == (CASES[name][2], 1)
    _assert_same(a, _run(name, rule, par, 8))
    _assert_same(a, _run(name, rule, par, 1))


def test_stop_inside_a_chunk_and_later_sweeps_are_no_ops():
    name = "1030x517_k3"
    a = _run(name, "pls", None, 8)
    b = _run(name, "pls", None, 8, extra=24)       # three more chunks after the stop
    _assert_same(a, b)
    fit = _case_fit(name, np.float32, tol=1e-6, max_iter=12, chunk=8)
    try:
        for _ in range(8):
            fit.sweeps(8)
        known, stop_known = fit.sweeps(0)
        assert stop_known == 1 and known == sum(a["status"][2])
    finally:
        fit.close()
