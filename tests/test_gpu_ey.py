"""GPU tests of CCA_EY / PLS_EY / MCCA_EY: the kernels against NumPy float64, every golden case, device tensors,
grid search, divergence, and a width the Gram route cannot take."""

import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from test_ey_host import CASES, case_params, case_views, col_err, restate

pytestmark = pytest.mark.gpu

F64_TOL = 1e-8     # fp64 views: per-column relative error of the weights
F32_TOL = 1e-4     # fp32 views: the products run in fp32 (DESIGN.md "Gradient models")


def _model(g, **over):
    from cca_zoo_amd.linear import CCA_EY, MCCA_EY, PLS_EY

    p = case_params(g)
    p.update(over)
    return {"CCA_EY": CCA_EY, "PLS_EY": PLS_EY, "MCCA_EY": MCCA_EY}[str(g["model"])](**p)


# ---- kernels through the C ABI --------------------------------------------------------------------------------------
class _Fit:
    """A raw fit state on rows uploaded to the device (ld > p when pad > 0).  ``pad``: one int or one per view, filled
    with ``pad_value``.  ``means``: "auto" (the column means when ``center``), None (``means_dev == NULL``) or a list of
    vectors whose None entries become NULL entries.  ``offset``: the view starts this many elements into its device
    buffer, so its base pointer is 4 (float32) or 8 (float64) bytes off a 16-byte boundary when ``offset`` is 1."""

    def __init__(self, views, k, bs, c=0.3, lr=0.01, mom=0.9, center=True, pad=0, chunk=4, means="auto", offset=0,
                 pad_value=0.0, tol=0.0):
        from cca_zoo_amd import _backend

        self.h = h = _backend.default_handle()
        self.f32 = views[0].dtype == np.float32
        self.m, self.k, self.bs = len(views), k, bs
        self.p = [v.shape[1] for v in views]
        self.n = views[0].shape[0]
        self.bufs, self.mbufs = [], []
        self.varr = (_backend.View * self.m)()
        pads = list(pad) if isinstance(pad, (list, tuple)) else [pad] * self.m
        if isinstance(means, str):
            means = [v.mean(axis=0).astype(v.dtype) for v in views] if center else None
        for i, v in enumerate(views):
            ld = v.shape[1] + pads[i]
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
        h.check(h.lib.ccz_ey_create(h.raw, _backend.F32 if self.f32 else _backend.F64, self.m,
                                    (C.c_int64 * self.m)(*self.p), k, bs, chunk, c, lr, mom, tol, C.byref(self.state)))

    def set_weights(self, W):
        flat = np.ascontiguousarray(np.concatenate([w.reshape(-1) for w in W]))
        self.h.check(self.h.lib.ccz_ey_set_weights(self.h.raw, self.state, flat.ctypes.data_as(C.POINTER(C.c_double))))

    def project(self, idx):
        z = np.empty((self.m, self.bs, self.k))
        ip = None if idx is None else np.ascontiguousarray(idx, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
        self.h.check(self.h.lib.ccz_ey_project(self.h.raw, self.state, self.varr, self.marr, self.n, ip,
                                               z.ctypes.data_as(C.POINTER(C.c_double))))
        return z

    def steps(self, idx, s):
        ip = None if idx is None else np.ascontiguousarray(idx, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
        a, b = C.c_int64(0), C.c_int(0)
        self.h.check(self.h.lib.ccz_ey_steps(self.h.raw, self.state, self.varr, self.marr, self.n, ip, s, C.byref(a),
                                             C.byref(b)))
        return a.value, b.value

    def weights(self):
        out = np.empty(sum(self.p) * self.k)
        self.h.check(self.h.lib.ccz_ey_get_weights(self.h.raw, self.state, out.ctypes.data_as(C.POINTER(C.c_double))))
        return np.split(out.reshape(-1, self.k), np.cumsum(self.p)[:-1])

    def status(self):
        a, b, o = C.c_int64(0), C.c_int(0), C.c_double(0)
        self.h.check(self.h.lib.ccz_ey_status(self.h.raw, self.state, C.byref(a), C.byref(b), C.byref(o)))
        return a.value, b.value, o.value

    def close(self):
        self.h.check(self.h.lib.ccz_ey_destroy(self.h.raw, self.state))


def _centred(views, f32):
    """The rows the device multiplies: fl(x - mu) in the views' dtype, as float64."""
    return [(v - v.mean(axis=0).astype(v.dtype)).astype(np.float64) for v in views]


def _one_step(xs, W, idx, c, lr, mom):
    """One step of the reference from zero velocity (float64)."""
    m, bs = len(xs), len(idx)
    Xb = [x[idx] for x in xs]
    Z = [xb @ w for xb, w in zip(Xb, W)]
    Zc = [z - z.mean(axis=0) for z in Z]
    tot = sum(Zc)
    V = sum(z.T @ z for z in Zc) / ((bs - 1) * m)
    B = sum(w.T @ w for w in W) / m
    vb = (1 - c) * V + c * B
    scale = 4.0 / (m * (bs - 1))
    return [W[i] - lr * (Xb[i].T @ (scale * (c * Zc[i] + (1 - c) * Zc[i] @ vb - tot)) + (4 * c / m) * W[i] @ vb)
            for i in range(m)]


SHAPES = [  # dims, k, n, bs, pad
    ((5, 3), 1, 40, 1, 0),
    ((37, 21), 7, 50, 3, 3),
    ((130, 17, 64), 7, 90, 90, 0),
    ((200, 150, 70, 129), 64, 300, 128, 5),
    ((300, 129), 128, 260, 260, 1),
    ((1500, 700), 16, 700, 300, 0),
]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{len(s[0])}v_k{s[1]}_bs{s[3]}" for s in SHAPES])
def test_projection_kernel(shape, dtype):
    dims, k, n, bs, pad = shape
    rng = np.random.default_rng(len(dims) * 100 + k)
    views = [(rng.standard_normal((n, d)) + 2.0).astype(dtype) for d in dims]
    W = [rng.standard_normal((d, k)) / np.sqrt(d) for d in dims]
    fit = _Fit(views, k, bs, pad=pad)
    try:
        fit.set_weights(W)
        idx = rng.choice(n, bs, replace=False)
        z = fit.project(idx)
        xs = _centred(views, dtype == np.float32)
        tol = 1e-12 if dtype == np.float64 else 2e-6
        for i in range(len(dims)):
            Wr = W[i].astype(np.float32).astype(np.float64) if dtype == np.float32 else W[i]
            ref = xs[i][idx] @ Wr
            err = np.max(np.abs(z[i] - ref)) / max(np.max(np.abs(ref)), 1e-300)
            print(f"projection {np.dtype(dtype).name} dims={dims} k={k} bs={bs} view {i}: rel err {err:.2e}")
            assert err <= tol, (i, err)
    finally:
        fit.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[3] >= 3], ids=[f"{len(s[0])}v_k{s[1]}_bs{s[3]}" for s in SHAPES
                                                                      if s[3] >= 3])
def test_update_kernel_one_step(shape, dtype):
    dims, k, n, bs, pad = shape
    rng = np.random.default_rng(len(dims) * 7 + k)
    views = [(rng.standard_normal((n, d)) + 1.0).astype(dtype) for d in dims]
    W = [rng.standard_normal((d, k)) / np.sqrt(d) for d in dims]
    c, lr, mom = 0.3, 0.05, 0.9
    fit = _Fit(views, k, bs, c=c, lr=lr, mom=mom, pad=pad)
    try:
        fit.set_weights(W)
        full = bs == n
        idx = np.arange(n) if full else rng.choice(n, bs, replace=False)
        fit.steps(None if full else idx[None, :], 1)
        got = fit.weights()
        steps, stopped, obj = fit.status()
        assert steps == 1 and not stopped and np.isfinite(obj)
        ref = _one_step(_centred(views, dtype == np.float32), W, idx, c, lr, mom)
        tol = 1e-11 if dtype == np.float64 else 2e-5
        for i in range(len(dims)):
            delta_ref = ref[i] - W[i]
            err = np.max(np.abs((got[i] - W[i]) - delta_ref)) / max(np.max(np.abs(delta_ref)), 1e-300)
            print(f"gradient step {np.dtype(dtype).name} dims={dims} k={k} bs={bs} view {i}: rel err {err:.2e}")
            assert err <= tol, (i, err)
    finally:
        fit.close()


# ---- the reference's fits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_golden_case(case):
    g = load_golden(f"ey_{case}")
    model = _model(g).fit(case_views(g))
    assert model.n_iter_ == int(g["n_iter"])
    f32 = g["X0"].dtype == np.float32
    for i, w in enumerate(model.weights_):
        ref = g[f"W{i}"]
        assert w.dtype == np.float64
        assert model.means_[i].dtype == ref.dtype or model.means_[i].dtype == g[f"mean{i}"].dtype
        if not np.all(np.isfinite(ref)):
            assert not np.all(np.isfinite(w))
            continue
        print(f"golden {case} view {i}: weights col err {col_err(w, ref):.2e}")
        assert col_err(w, ref) <= (F32_TOL if f32 else F64_TOL), (i, col_err(w, ref))
    if "score_test" in g:
        np.testing.assert_allclose(model.score(case_views(g, "T")), g["score_test"], atol=1e-3 if f32 else 1e-7)
        for i, z in enumerate(model.transform(case_views(g, "T"))):
            assert col_err(z, g[f"Zt{i}"]) <= (1e-3 if f32 else 1e-7)


def test_divergence_returns_non_finite_weights():
    g = load_golden("ey_diverge_c0")
    model = _model(g).fit(case_views(g))
    assert model.n_iter_ == case_params(g)["max_iter"]
    assert not all(np.all(np.isfinite(w)) for w in model.weights_)


def test_device_tensors_match_host_arrays():
    import torch

    for case in ("mcca3", "f32_k3"):
        g = load_golden(f"ey_{case}")
        host = _model(g).fit(case_views(g))
        dev = _model(g).fit([torch.as_tensor(v, device="cuda") for v in case_views(g)])
        assert dev.n_iter_ == host.n_iter_
        f32 = g["X0"].dtype == np.float32
        for a, b in zip(dev.weights_, host.weights_):
            assert col_err(a, b) <= (F32_TOL if f32 else 1e-12)


def test_grid_search_generic_route():
    from cca_zoo_amd.linear import CCA_EY
    from cca_zoo_amd.model_selection import GridSearchCV

    g = load_golden("ey_cca_c03")
    gs = GridSearchCV(CCA_EY(latent_dimensions=2, c=0.3, batch_size=100, max_iter=40, random_state=0),
                      {"learning_rate": [1e-3, 5e-3]}, cv=2).fit(case_views(g))
    assert gs.route_ == "generic"
    assert gs.best_params_["learning_rate"] in (1e-3, 5e-3)


# ---- a width beyond the Gram route ----------------------------------------------------------------------------------
def test_width_beyond_gram_route():
    """Two fp32 views of 40 000 features each (sum 80 000 > 65 535), n = 16 384, drawn on the device with
    ccz_randn_fill plus a planted rank-2 signal.  The first 5 steps match the float64 restatement on the gathered rows;
    a longer fit recovers the planted component on held-out rows."""
    import torch

    from cca_zoo_amd import _backend
    from cca_zoo_amd.linear import CCA_EY
    from cca_zoo_amd.linear.gradient._base import draw_batches

    n, n_test, p, k = 16384, 2048, 40000, 2
    h = _backend.default_handle()
    gen = torch.Generator(device="cuda").manual_seed(0)
    z = torch.randn(n + n_test, k, device="cuda", generator=gen)
    views = []
    for i in range(2):
        x = torch.empty(n + n_test, p, device="cuda", dtype=torch.float32)
        h.check(h.lib.ccz_randn_fill(h.raw, _backend.F32, C.c_void_p(x.data_ptr()), n + n_test, p, p, 1234 + i, 0, p,
                                     1.0, 0))
        a = torch.zeros(k, p, device="cuda")
        a[0, :200] = 0.25
        a[1, 200:400] = 0.15
        x += z @ a
        views.append(x)
    torch.cuda.synchronize()
    train = [v[:n] for v in views]
    test = [v[n:] for v in views]
    params = dict(latent_dimensions=k, c=0.5, batch_size=256, learning_rate=1e-4, tol=0.0, random_state=3)
    short = CCA_EY(max_iter=5, **params).fit(train)
    rng = np.random.default_rng(3)
    idx0 = rng.choice(n, 256, replace=False)
    [rng.standard_normal((p, k)) for _ in range(2)]
    draws = draw_batches(rng, n, 256, 5)
    rows = np.unique(np.concatenate([idx0, draws.reshape(-1)]))
    rowmap = np.full(n, -1)
    rowmap[rows] = np.arange(len(rows))
    ri = torch.as_tensor(rows, device="cuda")
    xs = [(t[ri] - torch.as_tensor(mu, device="cuda")).double().cpu().numpy() for t, mu in zip(train, short.means_)]
    W, steps = restate(xs, "cca", max_iter=5, n=n, rowmap=rowmap, **params)
    assert steps == 5 == short.n_iter_
    errs = [col_err(a, b) for a, b in zip(short.weights_, W)]
    print("wide: first 5 steps, per-column relative error vs float64", errs)
    assert max(errs) <= 1e-5, errs
    long = CCA_EY(max_iter=300, **params).fit(train)
    zt = long.transform(test)
    zt = [t.double().cpu().numpy() if hasattr(t, "cpu") else t for t in zt]
    corr = np.corrcoef(zt[0][:, 0], zt[1][:, 0])[0, 1]
    print("wide: held-out correlation of the first component", corr)
    assert abs(corr) >= 0.7, corr      # measured 0.83 (the planted correlation is 0.85-0.9 at this noise)
