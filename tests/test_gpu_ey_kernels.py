"""Kernel-level GPU tests of csrc/ey.hip: every template instantiation of the projection and the update, the float32
stage fold, several steps of state, the stop inside a chunk, the host-side refusals and strided device tensors.

Every comparator is float64 NumPy computed here (tests/test_ey_host.py holds the case tables, the input builders, the
a-priori bounds and their CPU tests).  Case count: 27 exact projection cases x 2 dtypes = 54, 3 random projections x 2,
9 one-step shapes x 2 = 18, 4 trajectories + 4 call-split checks, 4 stops, 2 refusal tests, 2 view-count tests and
2 x 3 strided fits: 100 tests.
"""

import ctypes as C

import numpy as np
import pytest

from test_ey_host import (EXACT_CASES, STOP_CASES, TRAJ_C, TRAJ_CHUNK, TRAJ_CONFIGS, TRAJ_LR, TRAJ_MOM, TRAJ_STEPS, col_err,
                          exact_inputs, exact_reference, fp32_stage_bound, restate, stop_plan, traj_inputs, traj_trace)
from test_gpu_ey import F32_TOL, F64_TOL, _centred, _Fit, _one_step

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
EINVAL, EUNSUP = -1, -6


def _name(dtype):
    return np.dtype(dtype).name


# ---- the projection in exact arithmetic -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("case", EXACT_CASES, ids=[f"c{i}_k{c[1]}_bs{c[2]}_{len(c[0])}v_{c[4]}" for i, c in enumerate(EXACT_CASES)])
def test_projection_exact(case, dtype):
    """Integer rows, integer means and dyadic weights: Z must equal the float64 product bit for bit, and the 1e30 that
    fills every padding element (and the element in front of an offset view) must never reach it."""
    dims, k, bs, n, ldmode, idxmode, meanmode, offset = case
    views, means, W, idx, lds = exact_inputs(case, dtype)
    fit = _Fit(views, k, bs, pad=[ld - d for ld, d in zip(lds, dims)], means=means, offset=offset, pad_value=1e30)
    try:
        for b, v in zip(fit.bufs, fit.varr):
            assert b.ptr % 16 == 0 and (v.data - b.ptr) == offset * np.dtype(dtype).itemsize
        fit.set_weights(W)
        z = fit.project(idx)
        ref = exact_reference(views, means, W, idx)
        for i in range(len(dims)):
            assert np.array_equal(z[i], ref[i]), (i, float(np.max(np.abs(z[i] - ref[i]))))
    finally:
        fit.close()


RANDOM_PROJ = [  # dims, k, n, bs, pad
    ((5000, 300), 20, 50, 33, 0),
    ((8200, 130), 100, 40, 31, 3),
    ((4097, 700, 64), 48, 70, 65, 0),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", RANDOM_PROJ, ids=[f"k{s[1]}_p{s[0][0]}" for s in RANDOM_PROJ])
def test_projection_random_within_stage_bound(shape, dtype):
    """Gaussian rows through the fold: float32 within the componentwise bound of a 1024-term float32 stage, float64
    within 1e-12 of the largest element."""
    dims, k, n, bs, pad = shape
    rng = np.random.default_rng(k)
    views = [(rng.standard_normal((n, d)) + 2.0).astype(dtype) for d in dims]
    W = [rng.standard_normal((d, k)) / np.sqrt(d) for d in dims]
    fit = _Fit(views, k, bs, pad=pad)
    try:
        fit.set_weights(W)
        idx = rng.choice(n, bs, replace=False)
        z = fit.project(idx)
        xs = _centred(views, dtype == np.float32)
        for i in range(len(dims)):
            if dtype == np.float32:
                Wr = W[i].astype(np.float32).astype(np.float64)
                ref = xs[i][idx] @ Wr
                ratio = np.max(np.abs(z[i] - ref) / fp32_stage_bound(np.abs(xs[i][idx]), np.abs(Wr), 1024))
                print(f"projection float32 dims={dims} k={k} view {i}: error / bound {ratio:.3g}")
                assert ratio <= 1.0, (i, ratio)
            else:
                ref = xs[i][idx] @ W[i]
                err = np.max(np.abs(z[i] - ref)) / np.max(np.abs(ref))
                print(f"projection float64 dims={dims} k={k} view {i}: rel err {err:.2e}")
                assert err <= 1e-12, (i, err)
    finally:
        fit.close()


# ---- one update step at every (dtype, KT, Q) ---------------------------------------------------------------------------
# Launch 3 gives a workgroup 64 Q features: Q = 4 at k <= 32 (KT 1, 2), Q = 1 above (KT 4, 8).
UPDATE_SHAPES = [  # dims, k, n, bs, pad, centre, offset
    ((256, 257, 30), 7, 80, 33, 0, True, 0),                        # KT 1: p = 64 Q, 64 Q + 1, views of 1 and 2 workgroups
    (tuple(3 + 19 * i for i in range(16)), 3, 30, 2, 0, True, 1),  # KT 1, 16 views, bs = 2
    ((256, 257, 600, 40), 20, 70, 65, 3, True, 1),                  # KT 2, partly filled tile, 1 / 2 / 3 / 1 workgroups
    ((513,), 32, 40, 2, 0, False, 0),                               # KT 2, full tile, one view, no centring
    ((64, 65, 200), 40, 90, 90, 0, False, 0),                       # KT 4, partly filled tile, full batch
    ((64, 65, 129, 50, 48), 48, 70, 33, 1, True, 1),                # KT 4, 5 views
    ((128, 129, 300), 100, 66, 33, 0, True, 1),                     # KT 8, partly filled tile
    (tuple(70 + 13 * i for i in range(16)), 65, 65, 65, 0, True, 0),  # KT 8, 16 views, full batch
    ((700,), 128, 300, 300, 0, True, 0),                            # KT 8, full tiles, one view, bs = 300
]


def _step_parts(xs, W, Z, idx, c):
    """T_i and v_blend of one step in float64 from given projections Z."""
    m, bs = len(xs), len(idx)
    Zc = [z - z.mean(axis=0) for z in Z]
    tot = sum(Zc)
    V = sum(z.T @ z for z in Zc) / ((bs - 1) * m)
    vb = (1 - c) * V + c * sum(w.T @ w for w in W) / m
    scale = 4.0 / (m * (bs - 1))
    return [scale * (c * Zc[i] + (1 - c) * Zc[i] @ vb - tot) for i in range(m)], vb


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", UPDATE_SHAPES, ids=[f"k{s[1]}_{len(s[0])}v_bs{s[3]}" for s in UPDATE_SHAPES])
def test_update_one_step(shape, dtype):
    """float64: the update against ``_one_step`` within 1e-11 of its largest element.

    float32: componentwise against the a-priori bound of the device's arithmetic.  With Z the device's own projection
    (checked exactly above), T from it in float64, Tf = fl32(T) and Xc = fl32(X - mu32), the gradient product differs
    from Xc' Tf by at most gamma_33 |Xc|' |Tf| (32 rows and the product rounding per float32 stage, any order inside
    the matrix instruction) + 2**-50 bs |Xc|' |Tf| (float64 across stages) + 2**-23 |Xc|' |Tf| (T is formed in another
    order on the device, which can move fl32(T) by one unit in the last place).  In all that is 2.2e-6 |Xc|' |Tf|.
    One dropped or doubled row changes an element by about 1 / bs of |Xc|' |Tf|: 3.3e-3 at the largest bs here (300),
    1500 times the bound."""
    dims, k, n, bs, pad, centre, offset = shape
    rng = np.random.default_rng(len(dims) * 7 + k)
    views = [(rng.standard_normal((n, d)) + 1.0).astype(dtype) for d in dims]
    W = [rng.standard_normal((d, k)) / np.sqrt(d) for d in dims]
    c, lr, mom = 0.3, 0.05, 0.9
    m = len(dims)
    fit = _Fit(views, k, bs, c=c, lr=lr, mom=mom, pad=pad, center=centre, offset=offset, pad_value=1e30)
    try:
        fit.set_weights(W)
        full = bs == n
        idx = np.arange(n) if full else rng.choice(n, bs, replace=False)
        zdev = fit.project(None if full else idx)
        fit.steps(None if full else idx[None, :], 1)
        got = fit.weights()
        steps, stopped, obj = fit.status()
        assert steps == 1 and not stopped and np.isfinite(obj)
        xs = _centred(views, dtype == np.float32) if centre else [v.astype(np.float64) for v in views]
        if dtype == np.float64:
            ref = _one_step(xs, W, idx, c, lr, mom)
            for i in range(m):
                delta_ref = ref[i] - W[i]
                err = np.max(np.abs((got[i] - W[i]) - delta_ref)) / np.max(np.abs(delta_ref))
                print(f"update float64 dims={dims} k={k} bs={bs} view {i}: rel err {err:.2e}")
                assert err <= 1e-11, (i, err)
            return
        T, vb = _step_parts(xs, W, list(zdev), idx, c)
        for i in range(m):
            Xb = xs[i][idx]
            Tf = T[i].astype(np.float32).astype(np.float64)
            delta_ref = -lr * (Xb.T @ Tf + (4 * c / m) * W[i] @ vb)
            A = np.abs(Xb).T @ np.abs(Tf)
            bound = fp32_stage_bound(np.abs(Xb).T, np.abs(Tf), 32) + 2.0 ** -23 * A
            tol = lr * bound + 1e-11 * np.max(np.abs(delta_ref))
            ratio = np.max(np.abs((got[i] - W[i]) - delta_ref) / tol)
            print(f"update float32 dims={dims} k={k} bs={bs} view {i}: error / bound {ratio:.3g}")
            assert ratio <= 1.0, (i, ratio)
    finally:
        fit.close()


# ---- several steps: velocity, the W double buffer, B carried across steps, chunks and pinned slots -------------------------
CALLS = [(0, 4), (4, 8), (8, 11)]


def _traj_fit(cfg, chunk=TRAJ_CHUNK, tol=0.0):
    views, xs, W0, draws = traj_inputs(cfg)
    return _Fit(views, cfg[1], cfg[4], c=TRAJ_C, lr=TRAJ_LR, mom=TRAJ_MOM, chunk=chunk, tol=tol), W0, draws


def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("cfg", TRAJ_CONFIGS, ids=[f"{_name(c[0])}_k{c[1]}" for c in TRAJ_CONFIGS])
def test_trajectory_matches_restatement(cfg):
    dtype, k, dims, n, bs = cfg
    wtol = F32_TOL if dtype == np.float32 else F64_TOL
    trace, done = traj_trace(cfg)
    assert done == TRAJ_STEPS
    fit, W0, draws = _traj_fit(cfg)
    try:
        fit.set_weights(W0)
        known = []
        for a, b in CALLS:
            known.append(fit.steps(draws[a:b], b - a))
            got = fit.weights()
            werr = max(col_err(g, r) for g, r in zip(got, trace[b - 1][1]))
            steps, stopped, obj = fit.status()
            oerr = _rel(obj, trace[b - 1][2])
            print(f"trajectory {_name(dtype)} k={k} after step {b}: weights col err {werr:.2e}, objective rel err {oerr:.2e}")
            assert (steps, stopped) == (b, 0)
            assert werr <= wtol, (b, werr)
            assert oerr <= wtol, (b, oerr)
        # the status a call returns is that of the call two calls earlier, which used the same pinned slot
        assert known == [(-1, 0), (-1, 0), (CALLS[0][1], 0)], known
    finally:
        fit.close()


@pytest.mark.parametrize("cfg", TRAJ_CONFIGS, ids=[f"{_name(c[0])}_k{c[1]}" for c in TRAJ_CONFIGS])
def test_call_split_does_not_change_the_arithmetic(cfg):
    """4 + 4 + 3 steps, 11 in one call and eleven calls of one step run the same kernels on the same inputs."""
    out = []
    for chunk, calls in ((TRAJ_CHUNK, CALLS), (TRAJ_STEPS, [(0, TRAJ_STEPS)]), (TRAJ_CHUNK, [(t, t + 1) for t in range(TRAJ_STEPS)])):
        fit, W0, draws = _traj_fit(cfg, chunk=chunk)
        try:
            fit.set_weights(W0)
            for a, b in calls:
                fit.steps(draws[a:b], b - a)
            out.append((np.concatenate([w.reshape(-1) for w in fit.weights()]), fit.status()))
        finally:
            fit.close()
    for w, st in out[1:]:
        assert np.array_equal(w, out[0][0])
        assert st == out[0][1]
    assert out[0][1][0] == TRAJ_STEPS


# ---- the stop inside a chunk -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STOP_CASES, ids=[f"{_name(TRAJ_CONFIGS[c[0]][0])}_parity{c[2]}" for c in STOP_CASES])
def test_stop_inside_a_chunk(case):
    """tol lies a factor >= 2 from every margin up to the stop step s* (test_stop_plan_is_robust_to_rounding), s* is
    not the last step of its call, and 11 steps are enqueued whatever s* is, so for an even s* the parity of the steps
    applied and of the steps enqueued differ.  A diverging (NaN) objective is left to
    test_gpu_ey.py::test_divergence_returns_non_finite_weights."""
    cfg = TRAJ_CONFIGS[case[0]]
    dtype = cfg[0]
    wtol = F32_TOL if dtype == np.float32 else F64_TOL
    s, tol, trace = stop_plan(case)
    fit, W0, draws = _traj_fit(cfg, tol=tol)

    def run():
        fit.set_weights(W0)
        for a, b in CALLS:
            fit.steps(draws[a:b], b - a)
        return fit.status(), fit.weights()

    try:
        st, got = run()
        assert st[:2] == (s, 1), st
        errs = {t: max(col_err(g, r) for g, r in zip(got, trace[t - 1][1])) for t in (s - 1, s, s + 1)}
        oerr = _rel(st[2], trace[s - 1][2])
        print(f"stop {_name(dtype)} at step {s}: weights col err {errs[s]:.2e} (step before {errs[s - 1]:.2e}, after "
              f"{errs[s + 1]:.2e}), objective rel err {oerr:.2e}")
        assert errs[s] <= wtol and oerr <= wtol
        assert errs[s - 1] > 100 * wtol and errs[s + 1] > 100 * wtol
        # later calls are no-ops whatever the parity of the steps enqueued
        for a, b in ((0, 4), (4, 7)):
            fit.steps(draws[a:b], b - a)
            st2, got2 = fit.status(), fit.weights()
            assert st2 == st
            assert all(np.array_equal(x, y) for x, y in zip(got, got2))
        # the same state, reset: bit for bit the same fit
        st3, got3 = run()
        assert st3 == st
        assert all(np.array_equal(x, y) for x, y in zip(got, got3))
    finally:
        fit.close()


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_create_refusals():
    from cca_zoo_amd import _backend

    h = _backend.default_handle()

    def create(m, p, k, bs=8, chunk=4):
        state = C.c_void_p(0xDEAD0)
        rc = h.lib.ccz_ey_create(h.raw, _backend.F64, m, (C.c_int64 * max(len(p), 1))(*p), k, bs, chunk, 0.3, 0.01, 0.9, 0.0,
                                 C.byref(state))
        return rc, state.value

    assert create(17, [8] * 17, 2) == (EUNSUP, None)
    assert "1 to 16 views" in h.lib.ccz_last_error(h.raw).decode()
    assert create(0, [], 2) == (EUNSUP, None)
    assert create(2, [8, 8], 0) == (EINVAL, None)
    assert create(2, [200, 200], 129) == (EINVAL, None)
    assert create(2, [8, 3], 4) == (EINVAL, None)
    assert create(2, [8, 8], 2, chunk=0) == (EINVAL, None)
    rc, state = create(16, [8] * 16, 2)
    assert rc == 0 and state
    h.check(h.lib.ccz_ey_destroy(h.raw, C.c_void_p(state)))


def test_steps_refusals_leave_the_state_usable():
    """Every refusal is made on the host before anything is enqueued: no step is counted, the weights keep their bits,
    and the next valid step gives the float64 result."""
    dims, k, n, bs = (300, 40), 5, 40, 8
    rng = np.random.default_rng(11)
    views = [rng.standard_normal((n, d)) + 1.0 for d in dims]
    W = [rng.standard_normal((d, k)) / np.sqrt(d) for d in dims]
    c, lr, mom = 0.3, 0.05, 0.9
    fit = _Fit(views, k, bs, c=c, lr=lr, mom=mom, chunk=2)
    h = fit.h

    def steps_rc(idx, s, n_rows=n):
        ip = None if idx is None else np.ascontiguousarray(idx, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
        a, b = C.c_int64(0), C.c_int(0)
        return h.lib.ccz_ey_steps(h.raw, fit.state, fit.varr, fit.marr, n_rows, ip, s, C.byref(a), C.byref(b))

    try:
        fit.set_weights(W)
        good = rng.choice(n, bs, replace=False)
        assert steps_rc(np.stack([good] * 3), 3) == EINVAL                # n_steps > chunk_steps
        high, neg = good.copy(), good.copy()
        high[bs - 1] = n
        neg[3] = -1
        assert steps_rc(np.stack([good, high]), 2) == EINVAL              # an index equal to n_rows, in the second step
        assert "out of range" in h.lib.ccz_last_error(h.raw).decode()
        assert steps_rc(neg[None, :], 1) == EINVAL
        assert steps_rc(None, 1) == EINVAL                                # no indices, n_rows != batch rows
        assert fit.status()[:2] == (0, 0)
        assert all(np.array_equal(a, b) for a, b in zip(fit.weights(), W))
        assert steps_rc(good[None, :], 1) == 0
        assert fit.status()[:2] == (1, 0)
        ref = _one_step(_centred(views, False), W, good, c, lr, mom)
        for g, r, w in zip(fit.weights(), ref, W):
            assert np.max(np.abs((g - w) - (r - w))) <= 1e-11 * np.max(np.abs(r - w))
    finally:
        fit.close()


# ---- the estimator seam ----------------------------------------------------------------------------------------------
def _many_views(m):
    rng = np.random.default_rng(m)
    z = rng.standard_normal((60, 2))
    return [z @ rng.standard_normal((2, 5 + i)) + rng.standard_normal((60, 5 + i)) for i in range(m)]


def test_sixteen_views_fit():
    from cca_zoo_amd.linear import MCCA_EY

    params = dict(latent_dimensions=2, c=0.3, batch_size=20, max_iter=15, learning_rate=0.01, tol=0.0, random_state=1)
    views = _many_views(16)
    model = MCCA_EY(**params).fit(views)
    W, steps = restate(views, "cca", **params)
    assert model.n_iter_ == steps == 15
    errs = [col_err(a, b) for a, b in zip(model.weights_, W)]
    print("16 views: weights col err", max(errs))
    assert max(errs) <= F64_TOL, errs


def test_seventeen_views_are_refused():
    from cca_zoo_amd.linear import MCCA_EY

    with pytest.raises(ValueError, match="1 to 16 views"):
        MCCA_EY(latent_dimensions=2, c=0.3, batch_size=20, max_iter=3, random_state=1).fit(_many_views(17))


@pytest.mark.parametrize("layout", ["column_slice", "row_slice", "fortran"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_strided_device_tensors(dtype, layout):
    """``fit`` hands a CUDA tensor with unit column stride through unchanged: a column slice (base pointer one element
    off its allocation, row stride > width), a row slice (row stride twice the width) and a Fortran-ordered tensor
    (copied) against the fit on a contiguous copy.  One view is wider than 4096, so the fold runs on the strided path."""
    import torch

    from cca_zoo_amd.linear import CCA_EY

    n, dims, k = 64, (4100, 300), 20
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    rng = np.random.default_rng(21)
    z = rng.standard_normal((2 * n, 3))
    strided = []
    for d in dims:
        host = (z @ rng.standard_normal((3, d + 4)) + rng.standard_normal((2 * n, d + 4))) / np.sqrt(d) + 0.5
        big = torch.as_tensor(host, device="cuda").to(tdt)
        if layout == "column_slice":
            x = big[:n, 1:d + 1]
            assert x.data_ptr() % 16 != 0 and x.stride(0) == d + 4
        elif layout == "row_slice":
            x = big[::2, :d]
            assert x.stride() == (2 * (d + 4), 1) and x.data_ptr() % 16 == 0
        else:
            x = big[:n, :d].t().contiguous().t()
            assert x.stride() == (1, n)
        assert tuple(x.shape) == (n, d)
        strided.append(x)
    params = dict(latent_dimensions=k, c=0.3, batch_size=32, max_iter=8, learning_rate=1e-3, tol=0.0, random_state=2)
    a = CCA_EY(**params).fit(strided)
    b = CCA_EY(**params).fit([x.contiguous() for x in strided])
    assert a.n_iter_ == b.n_iter_ == 8
    errs = [col_err(wa, wb) for wa, wb in zip(a.weights_, b.weights_)]
    print(f"strided {layout} {_name(dtype)}: weights col err vs contiguous {max(errs):.2e}")
    assert all(np.all(np.isfinite(w)) for w in b.weights_)
    assert max(errs) <= (F32_TOL if dtype == np.float32 else 1e-12), errs
