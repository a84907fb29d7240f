"""GPU tests of csrc/rrr.hip through the C ABI: the ADMM family against the NumPy restatement's loop
(tests/ccar3_restatement.py: ``admm_loop``) on ``M`` and ``P`` built on the host, the fourth-moment pass ``ccz_rownorm4`` and
``ccz_moments_block`` against NumPy.

Bars: ``B`` within 1e-10 relative Frobenius, equal iteration count, identical zero-row mask, identical bits for chunk lengths
1, 16 and 100 and for two runs.  Every case first checks ON THE RESTATEMENT that the last two residuals are more than 0.1 %
of ``tol`` away from ``tol`` and every row norm of ``B + U`` more than 1e-6 (relative) away from ``lambda_ / rho``: an equal
count and an equal mask are only asked where they are not a coin toss."""

import ctypes as C

import numpy as np
import pytest

from ccar3_restatement import admm_loop

pytestmark = pytest.mark.gpu

BAR = 1e-10
PD = C.POINTER(C.c_double)
REASON_TOL, REASON_MAXITER = 1, 2

#: (tag, p, q, lambda_ in units of 0.1, the norm of P's rows without signal, rho, tol, max_iter): q on the plain kernel (1, 3;
#: 70 rows = two of its row blocks), on one tile per wave (5, 16, 17, 64), two (65), four (129), eight (257) and sixteen
#: (513, 1000); p off the 16-row blocks, 33 row blocks (517), fewer rows than one block (9); a fit that stops at max_iter;
#: lambda_ = 0
CASES = (
    ("plain_q1", 37, 1, 3.0, 1.0, 1e-6, 500),
    ("plain_q3", 70, 3, 3.0, 1.0, 1e-6, 500),
    ("q5", 33, 5, 3.0, 1.0, 1e-6, 500),
    ("q16", 40, 16, 3.0, 2.0, 1e-7, 500),
    ("q17", 50, 17, 3.0, 1.0, 1e-6, 500),
    ("q64_few_rows", 9, 64, 3.0, 1.0, 1e-6, 500),
    ("q65", 35, 65, 3.0, 1.0, 1e-6, 500),
    ("q129", 20, 129, 3.0, 1.0, 1e-6, 500),
    ("q257", 18, 257, 3.0, 1.0, 1e-6, 500),
    ("q513", 17, 513, 3.0, 1.0, 1e-6, 500),
    ("q1000", 33, 1000, 3.0, 1.0, 1e-5, 500),
    ("rows517", 517, 12, 3.0, 1.0, 1e-6, 500),
    ("dense", 45, 12, 0.0, 1.0, 1e-6, 500),
    ("cap", 40, 16, 3.0, 2.0, 1e-12, 7),
)


def case(tag):
    return next(c for c in CASES if c[0] == tag)


def params(tag):
    """The case with lambda_ in absolute terms."""
    _, p, q, mult, rho, tol, max_iter = case(tag)
    return tag, p, q, mult * 0.1, rho, tol, max_iter


def problem(p, q, rho, seed):
    """M = (Sxx + (rho + 1e-8) I)^-1 of a random covariance with a few strong directions, P = Sxy R with signal in the first
    rows only (so a row penalty zeroes some of the others)."""
    rng = np.random.default_rng(seed)
    n = 3 * p + 20
    X = 0.5 * rng.standard_normal((n, 3)) @ rng.standard_normal((3, p)) + rng.standard_normal((n, p))
    Sxx = X.T @ X / n
    M = np.linalg.inv(Sxx + (rho + 1e-8) * np.eye(p))
    P = 0.1 * rng.standard_normal((p, q)) / np.sqrt(q)
    s = max(2, p // 3)
    P[:s] += rng.standard_normal((s, 2)) @ rng.standard_normal((2, q)) / np.sqrt(q)
    return np.ascontiguousarray(0.5 * (M + M.T)), np.ascontiguousarray(P)


_ref = {}


def reference(tag):
    """(M, P, Z, n_iter, residuals) of the restatement, computed once per case; the seed is the first that passes the
    margins (decided on the restatement alone)."""
    if tag not in _ref:
        _, p, q, lam, rho, tol, max_iter = params(tag)
        for seed in range(50):
            M, P = problem(p, q, rho, 1000 + seed)
            Z, it, res, norms = admm_loop(M, P, lam, rho, tol, max_iter)
            thr = lam / rho
            if np.all(np.abs(res.max(axis=1)[-2:] - tol) > 1e-3 * tol) and (thr == 0 or np.all(np.abs(norms - thr) > 1e-6 * thr)):
                break
        else:
            raise AssertionError(f"{tag}: no seed passed the margins")
        for a in (M, P, Z, res):
            a.setflags(write=False)
        _ref[tag] = (M, P, Z, it, res)
    return _ref[tag]


class _Rrr:
    def __init__(self, M, P, lam, rho, tol, max_iter, chunk=16):
        from cca_zoo_amd import _backend

        self.h = h = _backend.default_handle()
        self.p, self.q, self.max_iter = P.shape[0], P.shape[1], max_iter
        self.m, self.pb = h.to_device(M), h.to_device(P)
        self.state = C.c_void_p()
        h.check(h.lib.ccz_rrr_create(h.raw, self.p, self.q, lam, rho, tol, max_iter, chunk, C.byref(self.state)))
        h.check(h.lib.ccz_rrr_setup(h.raw, self.state, C.c_void_p(self.m.ptr), C.c_void_p(self.pb.ptr)))

    def iterations(self, n):
        a, b = C.c_int64(0), C.c_int(0)
        self.h.check(self.h.lib.ccz_rrr_iterations(self.h.raw, self.state, n, C.byref(a), C.byref(b)))
        return a.value, b.value

    def run(self, chunk):
        done = 0
        while done < self.max_iter:
            step = min(chunk, self.max_iter - done)
            if self.iterations(step)[1]:
                break
            done += step
        return self.status()

    def status(self):
        it, st, rs, a, b = C.c_int64(0), C.c_int(0), C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        self.h.check(self.h.lib.ccz_rrr_status(self.h.raw, self.state, C.byref(it), C.byref(st), C.byref(rs), C.byref(a), C.byref(b)))
        return dict(iters=it.value, stopped=st.value, reason=rs.value, primal=a.value, dual=b.value)

    def result(self):
        Z = np.full((self.p, self.q), np.nan)
        self.h.check(self.h.lib.ccz_rrr_get_result(self.h.raw, self.state, Z.ctypes.data_as(PD), None))
        return Z

    def close(self):
        self.h.check(self.h.lib.ccz_rrr_destroy(self.h.raw, self.state))


@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_admm_against_the_restatement(tag):
    _, p, q, lam, rho, tol, max_iter = params(tag)
    M, P, Z, it, res = reference(tag)
    fit = _Rrr(M, P, lam, rho, tol, max_iter)
    try:
        assert fit.status()["iters"] == 0 and not np.any(fit.result())
        st = fit.run(16)
        got = fit.result()
        err = np.linalg.norm(got - Z) / max(np.linalg.norm(Z), 1e-300)
        print(tag, st, "restatement", it, res[-1], "B", err, "zero rows", int((~np.any(Z, axis=1)).sum()))
        assert st["stopped"] == 1 and st["iters"] == it
        assert st["reason"] == (REASON_MAXITER if tag == "cap" else REASON_TOL)
        assert np.array_equal(~np.any(got, axis=1), ~np.any(Z, axis=1))
        assert err <= BAR
        # the residuals are norms of differences of B-sized entries over sqrt(p): B's bar in their units, |M P|_F / sqrt(p)
        scale = np.linalg.norm(M @ P) / np.sqrt(p)
        assert abs(st["primal"] - res[-1, 0]) <= BAR * scale and abs(st["dual"] - res[-1, 1]) <= BAR * scale
    finally:
        fit.close()


def test_the_cases_reach_what_they_are_there_for():
    zero = {t: int((~np.any(reference(t)[2], axis=1)).sum()) for t in ("q5", "q17", "q65", "rows517", "dense")}
    assert all(zero[t] > 0 for t in ("q5", "q17", "q65", "rows517")) and zero["dense"] == 0
    assert reference("rows517")[3] > 16 and reference("cap")[3] == 7


@pytest.mark.parametrize("tag", ["plain_q3", "q17", "q129", "rows517"])
def test_chunk_lengths_and_two_runs_give_the_same_bits(tag):
    _, p, q, lam, rho, tol, max_iter = params(tag)
    M, P, Z, it, res = reference(tag)
    outs = []
    for chunk in (1, 16, 100, 16):
        fit = _Rrr(M, P, lam, rho, tol, max_iter, chunk=chunk)
        try:
            st = fit.run(chunk)
            outs.append((st, fit.result()))
        finally:
            fit.close()
    for st, got in outs[1:]:
        assert st == outs[0][0] and np.array_equal(got, outs[0][1])


def test_the_stop_word_holds_after_the_stop():
    _, p, q, lam, rho, tol, max_iter = params("q17")
    M, P, Z, it, res = reference("q17")
    fit = _Rrr(M, P, lam, rho, tol, max_iter, chunk=100)
    try:
        assert it < 100
        fit.iterations(100)
        st, got = fit.status(), fit.result()
        assert st["iters"] == it and st["stopped"] == 1
        fit.iterations(100)
        fit.iterations(3)
        assert fit.status() == st and np.array_equal(fit.result(), got)
        with pytest.raises(ValueError):
            fit.iterations(101)          # more than chunk_iters
        # a new setup on the same state starts again and gives the same bits
        fit.h.check(fit.h.lib.ccz_rrr_setup(fit.h.raw, fit.state, C.c_void_p(fit.m.ptr), C.c_void_p(fit.pb.ptr)))
        assert fit.status()["iters"] == 0
        fit.iterations(100)
        assert fit.status() == st and np.array_equal(fit.result(), got)
    finally:
        fit.close()


@pytest.mark.parametrize("p, q, kwargs", [
    (16380, 5, {}),                      # p + q above 16384
    (20, 1025, {}),                      # q above 1024
    (0, 4, {}),
    (4, 0, {}),
    (5, 4, {"lam": -1.0}),
    (5, 4, {"lam": float("nan")}),
    (5, 4, {"rho": 0.0}),
    (5, 4, {"tol": -1.0}),
    (5, 4, {"tol": float("nan")}),
    (5, 4, {"max_iter": 0}),
    (5, 4, {"chunk": 0}),
])
def test_create_refuses_what_the_limits_exclude(p, q, kwargs):
    from cca_zoo_amd import _backend

    h = _backend.default_handle()
    state = C.c_void_p()
    rc = h.lib.ccz_rrr_create(h.raw, p, q, kwargs.get("lam", 0.1), kwargs.get("rho", 1.0), kwargs.get("tol", 1e-4),
                              kwargs.get("max_iter", 100), kwargs.get("chunk", 16), C.byref(state))
    unsup = p >= 1 and q >= 1 and (p + q > 16384 or q > 1024)
    assert rc == (-6 if unsup else -1) and not state.value


def test_calls_out_of_order_and_null_arguments_are_refused():
    from cca_zoo_amd import _backend

    h = _backend.default_handle()
    state = C.c_void_p()
    h.check(h.lib.ccz_rrr_create(h.raw, 5, 4, 0.1, 1.0, 1e-4, 100, 16, C.byref(state)))
    try:
        a, b = C.c_int64(0), C.c_int(0)
        assert h.lib.ccz_rrr_iterations(h.raw, state, 1, C.byref(a), C.byref(b)) == -1       # before setup
        assert h.lib.ccz_rrr_status(h.raw, state, None, None, None, None, None) == -1
        assert h.lib.ccz_rrr_get_result(h.raw, state, np.zeros(20).ctypes.data_as(PD), None) == -1
        assert h.lib.ccz_rrr_setup(h.raw, state, None, None) == -1
        assert h.lib.ccz_rrr_setup(h.raw, None, None, None) == -1
    finally:
        h.check(h.lib.ccz_rrr_destroy(h.raw, state))
    assert h.lib.ccz_rrr_destroy(h.raw, None) == 0


@pytest.mark.parametrize("dtype, n, cols, ld, centred", [
    (np.float64, 257, 7, 7, True),
    (np.float64, 1001, 70, 83, True),         # ld > cols, more columns than a wave has lanes
    (np.float32, 333, 12, 12, True),
    (np.float32, 4099, 5, 9, False),          # no mean; several row chunks
    (np.float64, 1, 3, 3, False),            # one row
])
def test_rownorm4_against_numpy(dtype, n, cols, ld, centred):
    from cca_zoo_amd import _backend

    h = _backend.default_handle()
    rng = np.random.default_rng(n + cols)
    buf = (rng.standard_normal((n, ld)) * 1.5 + 2.0).astype(dtype)
    Y = buf[:, :cols].astype(np.float64)
    mean = Y.mean(axis=0) if centred else np.zeros(cols)
    want = float(np.sum(np.sum((Y - mean) ** 2, axis=1) ** 2))
    yd, md = h.to_device(buf), h.to_device(mean)
    view = _backend.View(yd.ptr, cols, ld)
    outs = []
    for _ in range(2):
        out = C.c_double(0.0)
        h.check(h.lib.ccz_rownorm4(h.raw, _backend.F32 if dtype == np.float32 else _backend.F64, C.byref(view), n,
                                   C.c_void_p(md.ptr) if centred else None, C.byref(out)))
        outs.append(out.value)
    print(dtype.__name__, n, cols, "relative error", abs(outs[0] - want) / want)
    assert abs(outs[0] - want) <= 1e-12 * want and outs[0] == outs[1]
    bad = _backend.View(yd.ptr, cols, cols - 1)
    out = C.c_double(0.0)
    assert h.lib.ccz_rownorm4(h.raw, _backend.F64, C.byref(bad), n, None, C.byref(out)) == -1
    assert h.lib.ccz_rownorm4(h.raw, 7, C.byref(view), n, None, C.byref(out)) == -6
    assert h.lib.ccz_rownorm4(h.raw, _backend.F64, C.byref(view), 0, None, C.byref(out)) == -1


@pytest.mark.parametrize("center", [True, False])
def test_moments_block_against_numpy(center):
    from cca_zoo_amd import _backend

    h = _backend.default_handle()
    rng = np.random.default_rng(5)
    n, p, q = 203, 19, 6
    X, Y = rng.standard_normal((n, p)) + 2.5, rng.standard_normal((n, q)) - 2.0
    D = p + q
    xd, yd, mom = h.to_device(X), h.to_device(Y), h.alloc((D * D + D) * 8)
    h.moments([(xd.ptr, p, p), (yd.ptr, q, q)], n, _backend.F64, True, mom.ptr, pilot=False, timed=False)
    W = np.hstack([X, Y])
    if center:
        W = W - W.mean(axis=0)
    S = W.T @ W / n
    for r0, rows, c0, cols, shift in ((0, p, 0, p, 1.25), (0, p, p, q, 0.0), (p, q, p, q, 0.0), (p, q, 0, p, 0.0)):
        out = h.alloc(rows * (cols + 2) * 8)
        h.check(h.lib.ccz_moments_block(h.raw, C.c_void_p(mom.ptr), D, n, int(center), r0, rows, c0, cols, shift, C.c_void_p(out.ptr), cols + 2))
        got = h.to_host(out, (rows, cols + 2))[:, :cols]
        want = S[r0:r0 + rows, c0:c0 + cols] + (shift * np.eye(rows) if shift else 0.0)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(S).max()
    out = h.alloc(p * q * 8)
    assert h.lib.ccz_moments_block(h.raw, C.c_void_p(mom.ptr), D, n, 1, 0, p, p, q, 0.5, C.c_void_p(out.ptr), q) == -1   # a shift off the diagonal
    assert h.lib.ccz_moments_block(h.raw, C.c_void_p(mom.ptr), D, n, 1, 0, p, p, q + 1, 0.0, C.c_void_p(out.ptr), q + 1) == -1
