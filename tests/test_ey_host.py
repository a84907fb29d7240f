"""CPU tests of the gradient (Eckart-Young) models: import surface, parameters, the index producer, and a float64
NumPy restatement of the reference's loop checked against every golden (the comparator of tests/test_gpu_ey.py)."""

import glob
import os

import numpy as np
import pytest

from conftest import load_golden

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[3:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "ey_*.npz")))


def case_params(g):
    """Constructor parameters of a golden case (stored as the repr of a sorted item list)."""
    import ast

    return dict(ast.literal_eval(str(g["params"])))


def case_views(g, prefix="X"):
    return [g[f"{prefix}{i}"] for i in range(int(g["n_views"]))]


def restate(views, kind, latent_dimensions=1, center=True, c=0.0, learning_rate=1e-2, max_iter=1000, batch_size=None,
            tol=1e-6, momentum=0.9, random_state=None, n=None, rowmap=None, permute_full=True, trace=None, W0=None,
            draws=None):
    """The reference's fit in float64 NumPy, written from its equations (cca_zoo/linear/gradient/_base.py:101-130,
    _cca_ey.py:183-225, cca_zoo/_utils/_ey.py).  ``views`` are the raw views in their own dtype; centring is the
    reference's ``v - v.mean(axis=0)`` in that dtype.  ``n`` / ``rowmap``: the views hold only some rows of an
    ``n``-row data set (global row ``r`` is ``views[i][rowmap[r]]``) and are already centred.  ``permute_full=False``
    uses the rows in order when the batch is the whole data set (what the device does).  ``trace`` (a list) receives
    (Z list, W list, objective, stop margin ``|prev - obj|``) of every step (the margin of step 1 is inf).  ``W0``: start
    from these weights instead of the model's initialisation (no draw is taken for it); ``draws`` (steps x bs): the rows of
    every step instead of one ``choice`` per step.  Returns (weights, steps)."""
    xs = [np.asarray(v) for v in views]
    if center and rowmap is None:
        xs = [x - x.mean(axis=0) for x in xs]
    m = len(xs)
    n = xs[0].shape[0] if n is None else n
    rowmap = np.arange(n) if rowmap is None else rowmap
    k = latent_dimensions
    bs = n if batch_size is None else min(batch_size, n)
    rng = np.random.default_rng(random_state)
    if kind == "pls":
        c = 1.0
    if W0 is not None:
        W = [np.array(w, dtype=np.float64) for w in W0]
    elif kind == "pls":
        W = [np.linalg.qr(rng.standard_normal((x.shape[1], k)))[0] for x in xs]
    else:
        idx = rowmap[rng.choice(n, bs, replace=False)]
        W = []
        for x in xs:
            w0 = np.linalg.qr(rng.standard_normal((x.shape[1], k)))[0]
            r = np.linalg.qr(x[idx] @ w0)[1]
            W.append(w0 @ np.linalg.solve(r, np.eye(k)))
    vel = [np.zeros_like(w) for w in W]
    prev, steps = np.inf, 0
    full = bs == n
    with np.errstate(all="ignore"):
        for t in range(max_iter):
            if draws is not None:
                idx = rowmap[np.asarray(draws[t])]
            elif full and not permute_full:
                idx = rowmap[np.arange(n)]
            else:
                idx = rowmap[rng.choice(n, bs, replace=False)]
            Xb = [x[idx] for x in xs]
            Z = [xb @ w for xb, w in zip(Xb, W)]
            Zc = [z - z.mean(axis=0) for z in Z]
            tot = sum(Zc)
            V = sum(zc.T @ zc for zc in Zc) / ((bs - 1) * m)
            Cm = tot.T @ tot / ((bs - 1) * m)
            B = sum(w.T @ w for w in W) / m
            vb = (1 - c) * V + c * B
            scale = 4.0 / (m * (bs - 1))
            for i in range(m):
                zt = scale * (c * Zc[i] + (1 - c) * (Zc[i] @ vb) - tot)
                # the reference re-centres the batch in the views' dtype (its rounding matters for float32 views)
                g = (Xb[i] - Xb[i].mean(axis=0)).T @ zt + (4.0 * c / m) * (W[i] @ vb)
                vel[i] = momentum * vel[i] - learning_rate * g
                W[i] = W[i] + vel[i]
            B2 = sum(w.T @ w for w in W) / m
            vo = (1 - c) * V + c * B2
            obj = float(-2.0 * np.trace(Cm - c * V) + np.trace(vo @ vo))
            if trace is not None:
                trace.append(([z.copy() for z in Z], [w.copy() for w in W], obj, abs(prev - obj)))
            steps += 1
            if abs(prev - obj) < tol:
                break
            prev = obj
    return W, steps


def restate_case(g, **over):
    p = case_params(g)
    p.update(over)
    kind = "pls" if str(g["model"]) == "PLS_EY" else "cca"
    return restate(case_views(g), kind, **p)


def col_err(w, ref):
    """Largest per-column relative error."""
    num = np.linalg.norm(w - ref, axis=0)
    den = np.maximum(np.linalg.norm(ref, axis=0), 1e-300)
    return float(np.max(num / den))


# ---- import surface and parameters --------------------------------------------------------------------------------
def test_import_surface():
    import cca_zoo_amd.linear as lin
    from cca_zoo_amd.linear import CCA_EY, MCCA_EY, PLS_EY
    from cca_zoo_amd.linear.gradient import CCA_EY as A, MCCA_EY as B, PLS_EY as C

    assert (A, B, C) == (CCA_EY, MCCA_EY, PLS_EY)
    assert {"CCA_EY", "PLS_EY", "MCCA_EY"} <= set(lin.__all__)


def test_get_params_parity():
    from cca_zoo_amd.linear import CCA_EY, MCCA_EY, PLS_EY

    common = {"latent_dimensions": 1, "center": True, "learning_rate": 1e-2, "max_iter": 1000, "batch_size": None,
              "tol": 1e-6, "momentum": 0.9, "random_state": None}
    assert CCA_EY().get_params() == {**common, "c": 0.0}
    assert MCCA_EY().get_params() == {**common, "c": 0.0}
    assert PLS_EY().get_params() == common
    assert "c" not in PLS_EY().get_params()
    assert CCA_EY(c=0.4, batch_size=7).get_params()["batch_size"] == 7


def test_parameter_validation_and_new_errors(monkeypatch):
    from cca_zoo_amd import _dist
    from cca_zoo_amd.linear import CCA_EY, MCCA_EY, PLS_EY

    X, Y = np.zeros((20, 3)), np.zeros((20, 4))
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            CCA_EY(c=bad).fit([X, Y])
        with pytest.raises(ValueError):
            MCCA_EY(c=bad).fit([X, Y])
    with pytest.raises(ValueError):
        CCA_EY(latent_dimensions=0).fit([X, Y])
    with pytest.raises(ValueError, match="smallest view width"):
        CCA_EY(latent_dimensions=4).fit([X, Y])
    with pytest.raises(ValueError, match="smallest view width"):
        PLS_EY(latent_dimensions=5).fit([X, Y])
    monkeypatch.setattr(_dist, "is_sharded", lambda: True)
    for cls in (CCA_EY, PLS_EY, MCCA_EY):
        with pytest.raises(NotImplementedError, match="row_sharded"):
            cls().fit([X, Y])


def test_mixed_host_and_device_views_rejected(monkeypatch):
    from cca_zoo_amd._utils import _resident
    from cca_zoo_amd.linear import CCA_EY

    class FakeTensor:
        shape = (20, 4)

    real = _resident.is_device_tensor
    monkeypatch.setattr(_resident, "is_device_tensor", lambda v: isinstance(v, FakeTensor) or real(v))
    monkeypatch.setattr(_resident, "validate_views", lambda views, **kw: list(views))
    with pytest.raises(ValueError, match="all host arrays or all CUDA tensors"):
        CCA_EY().fit([np.zeros((20, 3)), FakeTensor()])


# ---- index producer -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_index_producer_matches_golden_draws(case):
    from cca_zoo_amd.linear.gradient._base import draw_batches, initial_weights

    g = load_golden(f"ey_{case}")
    p = case_params(g)
    views = case_views(g)
    n = views[0].shape[0]
    bs = n if p.get("batch_size") is None else min(p["batch_size"], n)
    rng = np.random.default_rng(p["random_state"])
    kind = "pls" if str(g["model"]) == "PLS_EY" else "cca"
    seen = []

    def project(idx, w0s):
        seen.append(idx)
        return [np.eye(bs, w.shape[1]) + 0.0 for w in w0s]

    initial_weights(kind, [v.shape[1] for v in views], p["latent_dimensions"], n, bs, rng, project)
    seen.extend(draw_batches(rng, n, bs, 3))
    for t in range(3):
        np.testing.assert_array_equal(seen[t], g[f"draw{t}"])


# ---- the restatement reproduces every golden ------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_golden(case):
    g = load_golden(f"ey_{case}")
    W, steps = restate_case(g)
    assert steps == int(g["n_iter"])
    for i, w in enumerate(W):
        ref = g[f"W{i}"]
        if not np.all(np.isfinite(ref)):
            assert not np.all(np.isfinite(w))
            continue
        assert col_err(w, ref) <= 1e-10, (case, i, col_err(w, ref))


def test_goldens_cover_the_contract():
    """Both branches of Generator.choice, fp32 and fp64, k = 1 and k > 1, early stops and tol = 0, 3 and 4 views."""
    gs = {c: load_golden(f"ey_{c}") for c in CASES}
    assert len(CASES) >= 12
    assert any(g["X0"].dtype == np.float32 for g in gs.values())
    assert any(g["X0"].dtype == np.float64 for g in gs.values())
    assert any(int(g["n_iter"]) < case_params(g)["max_iter"] for g in gs.values())
    assert any(case_params(g).get("tol", 1e-6) == 0.0 for g in gs.values())
    assert {int(g["n_views"]) for g in gs.values()} >= {2, 3, 4}
    assert {case_params(g)["latent_dimensions"] for g in gs.values()} >= {1, 2, 3}
    ns = {(g["X0"].shape[0], case_params(g).get("batch_size")) for g in gs.values()}
    assert any(n > 10000 and bs and bs > n // 50 for n, bs in ns)        # tail shuffle
    assert any(n > 10000 and bs and bs <= n // 50 for n, bs in ns)       # Floyd's method at a large n


# ---- inputs and a-priori bounds of the kernel-level GPU tests (tests/test_gpu_ey_kernels.py) ------------------------
def fp32_stage_bound(absX, absY, stage_len):
    """Componentwise a-priori bound on ``|fl(X Y) - X Y|`` for a product whose inner dimension is summed in float32 over
    stages of at most ``stage_len`` terms (any order inside a stage, fused or not) and in float64 across stages:
    ``(gamma_m + 2**-50 L) |X| |Y|`` with ``m = stage_len + 1`` (the sums of one stage plus the rounding of the product),
    ``gamma_m = m u / (1 - m u)``, ``u = 2**-24``, and ``L`` the inner dimension (Higham, Accuracy and Stability of
    Numerical Algorithms, section 3.1; the float64 part is far below its generous ``2**-50`` per term)."""
    absX, absY = np.asarray(absX, dtype=np.float64), np.asarray(absY, dtype=np.float64)
    m = stage_len + 1
    gamma = m * 2.0 ** -24 / (1.0 - m * 2.0 ** -24)
    return (gamma + 2.0 ** -50 * absX.shape[1]) * (absX @ absY)


def _crc(obj):
    import zlib

    return zlib.crc32(repr(obj).encode())


# Exact-arithmetic projection cases: (view widths, k, bs, n, ld, idx, means, base offset in elements).
#   ld: "tight" ld = p | "vec" the next multiple of 4 (16-byte loads with a scalar tail where p % 4 != 0) | "odd" an odd
#       ld (scalar loads) | "row" ld = 2 p (one full row of padding).  Every padding element holds 1e30.
#   idx: "edge" gathered rows with row 0, row n - 1 and a repeated neighbourhood | "none" idx_host == NULL (n == bs)
#   means: "int" integer means | "none" means_dev == NULL | "one_null" the middle view's entry NULL
EXACT_CASES = [
    # every k: KT = 1, 2, 4, 8 with full and partly filled column tiles
    ((1, 9), 1, 1, 40, "tight", "edge", "int", 0),
    ((16, 37), 16, 2, 40, "odd", "edge", "none", 1),
    ((17, 70), 17, 31, 40, "vec", "edge", "int", 0),
    ((20, 131), 20, 32, 32, "tight", "none", "int", 1),
    ((32, 33), 32, 33, 50, "row", "edge", "one_null", 1),
    ((33, 101), 33, 65, 70, "odd", "edge", "int", 0),
    ((48, 49), 48, 2, 9, "vec", "edge", "none", 0),
    ((64, 190), 64, 31, 31, "tight", "none", "one_null", 1),
    ((65, 66), 65, 32, 40, "vec", "edge", "int", 1),
    ((100, 257), 100, 33, 33, "row", "none", "int", 0),
    ((127, 130), 127, 1, 1, "odd", "none", "none", 0),
    ((128, 129), 128, 65, 65, "tight", "none", "none", 0),
    # p across the fold (4096 features = 64 slices per wave) and slice edges at a small k
    ((3,), 3, 33, 40, "tight", "edge", "int", 0),
    ((4095, 3), 3, 31, 40, "vec", "edge", "int", 0),
    ((4096, 7), 3, 32, 40, "tight", "edge", "none", 0),
    ((4097, 4096), 3, 2, 40, "odd", "edge", "int", 1),
    ((4111, 4097), 3, 65, 70, "vec", "edge", "one_null", 0),
    ((8200, 4111), 3, 33, 33, "row", "none", "int", 0),
    # the fold at every KT (KT = 1 above)
    ((4097, 8200), 20, 33, 40, "vec", "edge", "int", 0),
    ((8200, 4097), 40, 31, 40, "tight", "edge", "int", 1),
    ((4097, 8200), 100, 2, 40, "odd", "edge", "none", 0),
    # 1, 5 and 16 views of different widths (2 views above)
    ((77,), 5, 2, 2, "vec", "none", "int", 0),
    ((300,), 20, 65, 65, "tight", "none", "none", 1),
    ((40, 33, 64, 129, 50), 33, 31, 31, "odd", "none", "one_null", 0),
    ((9, 300, 17, 4100, 64), 7, 1, 40, "vec", "edge", "int", 1),
    (tuple(range(20, 36)), 20, 32, 32, "tight", "none", "int", 0),
    (tuple(70 + 13 * i for i in range(16)), 65, 65, 70, "row", "edge", "one_null", 1),
]


def exact_ld(mode, p):
    return {"tight": p, "vec": p + (-p) % 4, "odd": p + 1 + p % 2, "row": 2 * p}[mode]


def exact_inputs(case, dtype):
    """Views with integer entries in [-4, 4], integer means in [-2, 2] and weights that are multiples of 2**-3 in
    [-1, 1]: every product is a multiple of 2**-3 and every partial sum stays far below 2**24 such units, so the
    projection is exact in float32 and float64 in any order of summation.  Returns (views, means, W, idx, ld list)."""
    dims, k, bs, n, ldmode, idxmode, meanmode, _ = case
    rng = np.random.default_rng(_crc(case))
    views = [rng.integers(-4, 5, (n, d)).astype(dtype) for d in dims]
    means = [rng.integers(-2, 3, d).astype(dtype) for d in dims]
    W = [rng.integers(-8, 9, (d, k)) / 8.0 for d in dims]
    if meanmode == "none":
        means = None
    elif meanmode == "one_null":
        means[len(dims) // 2] = None
    if idxmode == "none":
        assert n == bs
        idx = None
    else:
        mid = n // 2
        idx = np.concatenate([[0, n - 1, mid, mid + 1, mid, mid + 1, mid - 1, mid], rng.integers(0, n, bs)])[:bs]
    return views, means, W, idx, [exact_ld(ldmode, d) for d in dims]


def exact_reference(views, means, W, idx):
    """(X[idx] - mu) W in float64."""
    out = []
    for i, (v, w) in enumerate(zip(views, W)):
        x = v.astype(np.float64) if means is None or means[i] is None else v.astype(np.float64) - means[i].astype(np.float64)
        out.append((x if idx is None else x[idx]) @ w)
    return out


@pytest.mark.parametrize("case", EXACT_CASES, ids=[f"c{i}" for i in range(len(EXACT_CASES))])
def test_exact_projection_cases_are_exact(case):
    """The precondition of the exact projection tests: 8 max_row sum |x - mu| |w| < 2**24, so every partial sum is an
    integer number of 2**-3 units that float32 holds exactly; and the table reaches what it claims to reach."""
    dims, k, bs, n, ldmode, idxmode, meanmode, offset = case
    for dtype in (np.float32, np.float64):
        views, means, W, idx, lds = exact_inputs(case, dtype)
        for i, (v, w) in enumerate(zip(views, W)):
            mu = 0 if means is None or means[i] is None else means[i].astype(np.float64)
            x = np.abs(v.astype(np.float64) - mu)
            assert np.all(x == np.round(x)) and x.max() <= 6
            assert np.all(w * 8 == np.round(w * 8)) and np.abs(w).max() <= 1
            assert 8 * np.max(x @ np.abs(w)) < 2 ** 24
            assert v.shape[1] >= k and lds[i] >= v.shape[1]
        if idx is not None:
            assert len(idx) == bs and idx.min() >= 0 and idx.max() < n
            if bs >= 8:
                assert 0 in idx and n - 1 in idx and len(np.unique(idx[:8])) < 8
    if ldmode == "vec":
        assert all(ld % 4 == 0 for ld in lds) and any(d % 4 for d in dims)
    if ldmode == "odd":
        assert all(ld % 2 == 1 for ld in lds)


def test_exact_projection_cases_cover_every_axis():
    ks = {c[1] for c in EXACT_CASES}
    assert ks >= {1, 16, 17, 20, 32, 33, 48, 64, 65, 100, 127, 128}
    small = {p for c in EXACT_CASES if c[1] <= 3 for p in c[0]}
    assert small >= {3, 4095, 4096, 4097, 4111, 8200}
    for lo, hi in ((1, 16), (17, 32), (33, 64), (65, 128)):           # the fold at every KT
        assert {4097, 8200} <= {p for c in EXACT_CASES if lo <= c[1] <= hi for p in c[0]}, (lo, hi)
    assert {c[2] for c in EXACT_CASES} >= {1, 2, 31, 32, 33, 65}
    assert {len(c[0]) for c in EXACT_CASES} >= {1, 2, 5, 16}
    assert {c[4] for c in EXACT_CASES} == {"tight", "vec", "odd", "row"}
    assert {c[5] for c in EXACT_CASES} == {"edge", "none"}
    assert {c[6] for c in EXACT_CASES} == {"int", "none", "one_null"}
    assert {c[7] for c in EXACT_CASES} == {0, 1}
    # every value of every axis meets at least two values of every other axis
    axes = {"k": 1, "bs": 2, "views": 0, "ld": 4, "idx": 5, "means": 6, "offset": 7}
    val = lambda c, a: len(c[0]) if a == "views" else c[axes[a]]
    for a in axes:
        for x in {val(c, a) for c in EXACT_CASES}:
            if a == "k" and x not in (3, 20):                         # one case per k; the k axis is crossed at 3 and 20
                continue
            for b in axes:
                if b != a:
                    assert len({val(c, b) for c in EXACT_CASES if val(c, a) == x}) >= 2, (a, x, b)


def _f32_sum(terms, order):
    """Sum float32 ``terms`` in float32: forwards, backwards or pairwise."""
    t = [np.float32(x) for x in terms]
    if order == "backward":
        t = t[::-1]
    if order == "pairwise":
        while len(t) > 1:
            t = [np.float32(t[i] + t[i + 1]) if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
        return t[0]
    acc = np.float32(0)
    for x in t:
        acc = np.float32(acc + x)
    return acc


@pytest.mark.parametrize("order", ["forward", "backward", "pairwise"])
def test_fp32_stage_bound_holds_for_brute_force_sums(order):
    rng = np.random.default_rng(5)
    worst = 0.0
    for L, stage in ((7, 4), (50, 16), (200, 32), (300, 1024)):
        X = (rng.standard_normal((3, L)) + 1.0).astype(np.float32)
        Y = rng.standard_normal((L, 2)).astype(np.float32)
        bound = fp32_stage_bound(np.abs(X), np.abs(Y), stage)
        exact = X.astype(np.float64) @ Y.astype(np.float64)
        for i in range(3):
            for j in range(2):
                prods = [np.float32(X[i, t] * Y[t, j]) for t in range(L)]
                got = sum(float(_f32_sum(prods[s:s + stage], order)) for s in range(0, L, stage))
                worst = max(worst, abs(got - exact[i, j]) / bound[i, j])
                assert abs(got - exact[i, j]) <= bound[i, j]
                # the bound is sharp enough to see one dropped term
                drop = got - float(prods[L // 2])
                assert abs(drop - exact[i, j]) > bound[i, j] or abs(prods[L // 2]) < 1e-3
    assert 0.0 < worst < 1.0


# Multi-step trajectories: (dtype, k, widths, n, bs); c = 0.3, momentum 0.9, 11 steps in calls of 4, 4 and 3.
# Launch 3 gives one workgroup 256 features at k <= 32 and 64 above, so the widest view of each spans several.
TRAJ_CONFIGS = [
    (np.float64, 20, (600, 257, 40), 120, 48),
    (np.float32, 20, (600, 257, 40), 120, 48),
    (np.float64, 100, (300, 129, 100), 150, 65),
    (np.float32, 40, (300, 129, 64), 150, 65),
]
TRAJ_STEPS, TRAJ_CHUNK, TRAJ_C, TRAJ_MOM, TRAJ_LR = 11, 4, 0.3, 0.9, 0.01


def traj_inputs(cfg, seed=0):
    """Views with a shared rank-4 signal, initial weights and the row draws of a trajectory configuration.  Returns
    (views in their dtype, the centred rows the device multiplies as float64, W0, draws)."""
    dtype, k, dims, n, bs = cfg
    rng = np.random.default_rng(_crc((np.dtype(dtype).name,) + tuple(cfg[1:])) + seed)
    z = rng.standard_normal((n, 4))
    views = [((z @ rng.standard_normal((4, d)) * 0.5 + rng.standard_normal((n, d))) / np.sqrt(d) + 0.5).astype(dtype)
             for d in dims]
    xs = [(v - v.mean(axis=0).astype(v.dtype)).astype(np.float64) for v in views]
    W0 = [0.5 * rng.standard_normal((d, k)) for d in dims]
    draws = np.stack([rng.choice(n, bs, replace=False) for _ in range(TRAJ_STEPS)]).astype(np.int64)
    return views, xs, W0, draws


def traj_trace(cfg, seed=0, steps=TRAJ_STEPS, tol=0.0):
    views, xs, W0, draws = traj_inputs(cfg, seed)
    trace = []
    _, done = restate(xs, "cca", latent_dimensions=cfg[1], center=False, c=TRAJ_C, learning_rate=TRAJ_LR, max_iter=steps,
                      batch_size=cfg[4], tol=tol, momentum=TRAJ_MOM, W0=W0, draws=draws, trace=trace)
    return trace, done


# Stop inside a chunk: (trajectory configuration, data seed, parity of the stop step)
STOP_CASES = [(0, 0, 1), (0, 0, 0), (1, 0, 1), (1, 0, 0)]


def stop_plan(case):
    """The stop step s* and a tol for it, from the float64 trace with tol = 0: the first step of the wanted parity that
    is not the last step of a call (calls of TRAJ_CHUNK steps, TRAJ_STEPS in all) and whose margin lies at least a factor
    4 below every earlier margin; tol is the geometric mean of that margin and the smallest earlier one.
    Returns (s*, tol, trace)."""
    ci, seed, parity = case
    trace, _ = traj_trace(TRAJ_CONFIGS[ci], seed)
    margins = [t[3] for t in trace]
    for s in range(3, TRAJ_STEPS):
        if s % 2 != parity or s % TRAJ_CHUNK == 0:
            continue
        lo = min(margins[: s - 1])
        if 4.0 * margins[s - 1] <= lo:
            return s, float(np.sqrt(margins[s - 1] * lo)), trace
    raise AssertionError(f"no stop step of parity {parity} in {margins}")


@pytest.mark.parametrize("case", STOP_CASES, ids=[f"cfg{c[0]}_seed{c[1]}_parity{c[2]}" for c in STOP_CASES])
def test_stop_plan_is_robust_to_rounding(case):
    """Every margin up to and including s* is at least a factor 2 away from tol, the restatement with that tol stops at
    s*, and the weights one step either side of s* differ from those at s* by more than 100 times the tolerance of the
    device comparison, so that comparison can tell the steps apart."""
    s, tol, trace = stop_plan(case)
    dtype = TRAJ_CONFIGS[case[0]][0]
    assert s % 2 == case[2] and s % TRAJ_CHUNK != 0 and 2 < s < TRAJ_STEPS
    margins = [t[3] for t in trace]
    assert all(m >= 2.0 * tol for m in margins[: s - 1]) and margins[s - 1] <= tol / 2.0
    _, done = traj_trace(TRAJ_CONFIGS[case[0]], case[1], tol=tol)
    assert done == s
    wtol = 1e-4 if dtype == np.float32 else 1e-8
    at = np.concatenate(trace[s - 1][1])
    for other in (s - 2, s):
        assert col_err(np.concatenate(trace[other][1]), at) > 100 * wtol


def test_trajectory_configurations():
    assert [(np.dtype(c[0]).name, c[1]) for c in TRAJ_CONFIGS] == [("float64", 20), ("float32", 20), ("float64", 100),
                                                                   ("float32", 40)]
    for dtype, k, dims, n, bs in TRAJ_CONFIGS:
        assert len(set(dims)) == 3 and bs < n and min(dims) >= k
        assert max(dims) > (256 if k <= 32 else 64)
    trace, done = traj_trace(TRAJ_CONFIGS[0])
    assert done == TRAJ_STEPS == len(trace) and np.isinf(trace[0][3])
    assert all(np.isfinite(t[2]) for t in trace)
