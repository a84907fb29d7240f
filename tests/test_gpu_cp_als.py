"""GPU tests of the device CP-ALS (csrc/cp_als.hip) through the C ABI, against the NumPy restatement run live
(tests/tcca_fit_restatement.py).  Tensors are planted: factor columns (orthonormal or oblique) with well separated weights
plus dense noise, so every unfolding's leading singular values are apart and the fit stops by ``tol``.

Bars: 1e-8 per column for the init and the factors (the project's standing device bar), equal ``n_iter``, 1e-10 on the
error trace.  Every case first checks ON THE RESTATEMENT that no ``|e_{t-1} - e_t|`` lies within 10 % of ``tol``: an equal
iteration count is only asked where the stop is not a coin toss."""

import ctypes as C

import numpy as np
import pytest

from tcca_fit_restatement import TOL, cp_als, khatri_rao, svd_init

pytestmark = pytest.mark.gpu

BAR, TRACE_BAR = 1e-8, 1e-10
PD = C.POINTER(C.c_double)
REASON_TOL, REASON_MAXITER, REASON_SINGULAR = 1, 2, 3

#: (tag, widths, k, seed, orthonormal factors, noise): order 2 to 5; widths off the 16- and 64-row tiles; a width of 1; k on the
#: plain path (1 .. 4), one MFMA column tile (5, 8), two (32); one tensor with several row tiles and a split contraction axis.
#: The "orthonormal" cases stop after 2 or 3 iterations; the others (oblique factors, more noise) after 10 to 26, two of
#: them beyond the first chunk of 16.  Seeds were chosen on the restatement alone (margin, cond(P) <= 60, the growth of a
#: 1e-9 perturbation of the init below 50 times).
CASES = (
    ("order2", (7, 5), 3, 100, True, 0.02),
    ("order3_k1", (5, 4, 3), 1, 101, True, 0.02),
    ("order3_k4", (17, 16, 9), 4, 102, True, 0.02),
    ("order3_k8", (12, 10, 9), 8, 103, True, 0.02),
    ("order4", (4, 3, 3, 2), 2, 104, True, 0.02),
    ("order5", (3, 2, 3, 2, 2), 2, 105, True, 0.02),
    ("width1", (6, 1, 5), 1, 106, True, 0.02),
    ("narrowest", (3, 4, 5), 3, 107, True, 0.02),
    ("k32", (33, 40, 32), 32, 108, True, 0.02),
    ("split", (70, 65, 66), 5, 109, True, 0.02),
    ("oblique_k4", (17, 16, 9), 4, 0, False, 0.3),
    ("oblique_k3_long", (9, 8, 7), 3, 2, False, 0.6),
    ("oblique_k5_long", (12, 10, 9), 5, 0, False, 0.6),
    ("oblique_order4", (6, 5, 4, 3), 2, 4, False, 0.3),
)


def case(tag):
    return next(c for c in CASES if c[0] == tag)


def planted(dims, k, seed, orth, noise):
    rng = np.random.default_rng(seed)
    A = [rng.standard_normal((d, k)) for d in dims]
    if orth:
        A = [np.linalg.qr(a)[0] for a in A]
    w = (1.08 if k > 8 else 1.3) ** -np.arange(k)
    T = (khatri_rao(A) * w).sum(axis=1).reshape(dims)
    N = rng.standard_normal(dims)
    return T + noise * np.linalg.norm(T) / np.linalg.norm(N) * N


_ref = {}


def reference(tag):
    """(tensor, init, factors, trace) of the restatement, computed once per case."""
    if tag not in _ref:
        _, dims, k, seed, orth, noise = case(tag)
        M = planted(dims, k, seed, orth, noise)
        A0 = svd_init(M, k)
        A, trace = cp_als(M, k, init=A0)
        dec = np.abs(np.diff(trace))
        assert not np.any(np.abs(dec - TOL) < 0.1 * TOL), (tag, dec)
        for a in (M, *A0, *A, trace):
            a.setflags(write=False)
        _ref[tag] = (M, A0, A, trace)
    return _ref[tag]


class _Cp:
    def __init__(self, M, k, chunk=16, tol=TOL, max_iter=100):
        from cca_zoo_amd import _backend

        self.h = h = _backend.default_handle()
        self.dims, self.k, self.max_iter = M.shape, k, max_iter
        self.mbuf = h.to_device(np.ascontiguousarray(M, dtype=np.float64))
        self.state = C.c_void_p()
        h.check(h.lib.ccz_cp_create(h.raw, M.ndim, (C.c_int64 * M.ndim)(*M.shape), k, tol, max_iter, chunk, C.byref(self.state)))
        h.check(h.lib.ccz_cp_setup(h.raw, self.state, C.c_void_p(self.mbuf.ptr)))

    def set_init(self, factors):
        flat = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in factors]))
        self.h.check(self.h.lib.ccz_cp_set_init(self.h.raw, self.state, flat.ctypes.data_as(PD)))

    def iterations(self, n):
        a, b = C.c_int64(0), C.c_int(0)
        self.h.check(self.h.lib.ccz_cp_iterations(self.h.raw, self.state, n, C.byref(a), C.byref(b)))
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
        it, st, rs, e, d = C.c_int64(0), C.c_int(0), C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        self.h.check(self.h.lib.ccz_cp_status(self.h.raw, self.state, C.byref(it), C.byref(st), C.byref(rs), C.byref(e), C.byref(d)))
        return dict(iters=it.value, stopped=st.value, reason=rs.value, err=e.value, dec=d.value)

    def result(self):
        flat = np.empty(sum(self.dims) * self.k)
        trace = np.full(self.max_iter, np.nan)
        n = C.c_int64(0)
        self.h.check(self.h.lib.ccz_cp_get_result(self.h.raw, self.state, flat.ctypes.data_as(PD), trace.ctypes.data_as(PD), C.byref(n)))
        offs = np.cumsum([0] + [d * self.k for d in self.dims])
        return [flat[offs[i]:offs[i + 1]].reshape(d, self.k).copy() for i, d in enumerate(self.dims)], trace[:n.value]

    def close(self):
        self.h.check(self.h.lib.ccz_cp_destroy(self.h.raw, self.state))


def col_err(A, R):
    """Largest per-column relative error, signs as they are (the sign rule of the init fixes them on both sides)."""
    return float((np.linalg.norm(A - R, axis=0) / np.linalg.norm(R, axis=0)).max())


@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_init_factors_iterations_and_trace(tag):
    _, dims, k = case(tag)[:3]
    M, A0, A, trace = reference(tag)
    fit = _Cp(M, k)
    try:
        init, t0 = fit.result()
        assert t0.size == 0 and fit.status()["iters"] == 0
        figures = {"init": max(col_err(a, r) for a, r in zip(init, A0))}
        for source in ("device init", "host init"):
            if source == "host init":
                fit.set_init(A0)
            st = fit.run(16)
            got, tr = fit.result()
            figures[source] = max(col_err(a, r) for a, r in zip(got, A))
            figures[source + " trace"] = float(np.abs(tr - trace[:tr.size]).max()) if tr.size == trace.size else np.inf
            print(tag, source, st, figures)
            assert st["stopped"] == 1 and st["reason"] == REASON_TOL
            assert st["iters"] == trace.size == tr.size
            assert st["err"] == tr[-1] and abs(st["dec"] - abs(tr[-1] - tr[-2])) <= 1e-16
        assert figures["init"] <= BAR, figures
        assert figures["device init"] <= BAR and figures["host init"] <= BAR, figures
        assert figures["device init trace"] <= TRACE_BAR and figures["host init trace"] <= TRACE_BAR, figures
    finally:
        fit.close()


@pytest.mark.parametrize("tag", ["order3_k4", "split", "k32", "oblique_k5_long"])
def test_chunk_lengths_and_two_runs_give_the_same_bits(tag):
    _, dims, k = case(tag)[:3]
    M, A0, A, trace = reference(tag)
    outs = []
    for chunk in (1, 16, 100, 16):
        fit = _Cp(M, k, chunk=chunk)
        try:
            st = fit.run(chunk)
            got, tr = fit.result()
            outs.append((st["iters"], np.concatenate([g.reshape(-1) for g in got]), tr))
        finally:
            fit.close()
    for it, flat, tr in outs[1:]:
        assert it == outs[0][0]
        assert np.array_equal(flat, outs[0][1]) and np.array_equal(tr, outs[0][2])


def test_a_stop_inside_a_chunk_leaves_the_counters_where_the_stop_put_them():
    M, A0, A, trace = reference("order3_k4")
    assert trace.size < 16
    fit = _Cp(M, 4, chunk=16)
    try:
        fit.iterations(16)
        st = fit.status()
        got, tr = fit.result()
        assert st["iters"] == trace.size and st["stopped"] == 1
        fit.iterations(16)
        fit.iterations(3)
        st2 = fit.status()
        got2, tr2 = fit.result()
        assert st2 == st and np.array_equal(tr, tr2)
        assert all(np.array_equal(a, b) for a, b in zip(got, got2))
    finally:
        fit.close()


def test_the_iteration_cap_and_a_partial_chunk():
    """max_iter below the tol stop: the fit stops at the cap with reason MAXITER, the trace has max_iter entries."""
    M, A0, A, trace = reference("oblique_k4")
    assert trace.size > 3
    fit = _Cp(M, 4, chunk=2, max_iter=3)
    try:
        st = fit.run(2)
        got, tr = fit.result()
        assert st["iters"] == 3 and st["stopped"] == 1 and st["reason"] == REASON_MAXITER
        assert np.abs(tr - trace[:3]).max() <= TRACE_BAR
        with pytest.raises(ValueError):
            fit.iterations(3)          # more than chunk_iters
    finally:
        fit.close()


def test_a_singular_hadamard_gram_stops_the_fit():
    """Two equal columns in every other factor make P singular: exactly zero pivots only when the columns are exact copies
    of small integers, which this init provides."""
    M, A0, A, trace = reference("order3_k4")
    init = [np.zeros_like(a) for a in A0]
    for a in init:
        a[0, :] = 1.0
        a[1, :2] = 2.0
        a[1, 2:] = 3.0
        a[2, :] = [1.0, 1.0, 2.0, 4.0]
    fit = _Cp(M, 4)
    try:
        fit.set_init(init)
        fit.iterations(4)
        st = fit.status()
        assert st["stopped"] == 1 and st["reason"] == REASON_SINGULAR and st["iters"] == 0
    finally:
        fit.close()


@pytest.mark.parametrize("dims, k, kwargs", [
    ((5,), 1, {}),                       # order 1
    ((2,) * 9, 1, {}),                   # order 9
    ((4, 4, 4), 0, {}),                  # rank 0
    ((40, 40, 40), 33, {}),              # rank 33
    ((4097, 4096), 2, {}),               # more than 2^24 entries
    ((5, 4, 3), 4, {}),                  # rank above the narrowest mode
    ((5, 0, 3), 1, {}),                  # an empty mode
    ((5, 4, 3), 2, {"tol": -1.0}),
    ((5, 4, 3), 2, {"tol": float("nan")}),
    ((5, 4, 3), 2, {"max_iter": 0}),
    ((5, 4, 3), 2, {"chunk": 0}),
])
def test_create_refuses_what_the_limits_exclude(dims, k, kwargs):
    from cca_zoo_amd import _backend

    h = _backend.default_handle()
    state = C.c_void_p()
    rc = h.lib.ccz_cp_create(h.raw, len(dims), (C.c_int64 * len(dims))(*dims), k, kwargs.get("tol", TOL), kwargs.get("max_iter", 100),
                             kwargs.get("chunk", 16), C.byref(state))
    unsup = len(dims) < 2 or len(dims) > 8 or k < 1 or k > 32 or int(np.prod(dims, dtype=np.int64)) > 2 ** 24
    assert rc == (-6 if unsup else -1) and not state.value


def test_calls_out_of_order_and_null_arguments_are_refused():
    from cca_zoo_amd import _backend

    h = _backend.default_handle()
    state = C.c_void_p()
    h.check(h.lib.ccz_cp_create(h.raw, 3, (C.c_int64 * 3)(5, 4, 3), 2, TOL, 100, 16, C.byref(state)))
    try:
        a, b = C.c_int64(0), C.c_int(0)
        assert h.lib.ccz_cp_iterations(h.raw, state, 1, C.byref(a), C.byref(b)) == -1       # before setup
        assert h.lib.ccz_cp_set_init(h.raw, state, np.zeros(24).ctypes.data_as(PD)) == -1    # before setup
        assert h.lib.ccz_cp_status(h.raw, state, None, None, None, None, None) == -1
        assert h.lib.ccz_cp_setup(h.raw, state, None) == -1
        assert h.lib.ccz_cp_setup(h.raw, None, None) == -1
    finally:
        h.check(h.lib.ccz_cp_destroy(h.raw, state))
    assert h.lib.ccz_cp_destroy(h.raw, None) == 0
