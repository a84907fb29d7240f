"""GPU tests of the nonparametric module: the two HIP kernels (ccz_pairwise_kernel, ccz_kernel_project) against NumPy
float64, KCCA / KGCCA against the reference's goldens and properties, device tensors, loadings, and scale."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from test_kernel_cca_host import CASES, avg_corr, case_data, col_err, route, tolerance

pytestmark = pytest.mark.gpu

KINDS = {"linear": 0, "poly": 1, "rbf": 2, "sigmoid": 3, "cosine": 4}


def np_kernel(kind, A, B, gamma, degree, coef0, symmetric):
    A = A.astype(np.float64)
    B = B.astype(np.float64)
    G = A @ B.T
    na, nb = (A * A).sum(1), (B * B).sum(1)
    if kind == "linear":
        return G
    if kind == "poly":
        with np.errstate(invalid="ignore"):
            return np.power(gamma * G + coef0, degree)
    if kind == "rbf":
        D = np.maximum(na[:, None] + nb[None, :] - 2 * G, 0)
        if symmetric:
            np.fill_diagonal(D, 0)
        return np.exp(-gamma * D)
    if kind == "sigmoid":
        return np.tanh(gamma * G + coef0)
    s = np.sqrt(na)[:, None] * np.sqrt(nb)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(s > 0, G / np.where(s > 0, s, 1), 0.0)


def torch_mod():
    import torch

    assert torch.cuda.is_available()
    return torch


def dev_kernel(A, B, kind, gamma=0.3, degree=2.5, coef0=0.7, muA=None, muB=None, symmetric=False):
    from cca_zoo_amd import _backend

    torch = torch_mod()
    h = _backend.default_handle()
    At = torch.as_tensor(A, device="cuda")
    Bt = At if symmetric else torch.as_tensor(B, device="cuda")
    ma = None if muA is None else torch.as_tensor(muA, device="cuda")
    mb = ma if (symmetric and muB is muA) else (None if muB is None else torch.as_tensor(muB, device="cuda"))
    K = torch.full((A.shape[0], Bt.shape[0]), np.nan, dtype=torch.float64, device="cuda")
    dt = _backend.F32 if A.dtype == np.float32 else _backend.F64
    torch.cuda.synchronize()
    h.check(h.lib.ccz_pairwise_kernel(h.raw, dt, C.c_void_p(At.data_ptr()), A.shape[0], A.shape[1],
                                      None if ma is None else C.c_void_p(ma.data_ptr()), C.c_void_p(Bt.data_ptr()),
                                      Bt.shape[0], Bt.shape[1], None if mb is None else C.c_void_p(mb.data_ptr()),
                                      A.shape[1], KINDS[kind], gamma, degree, coef0, C.c_void_p(K.data_ptr()), K.shape[1]))
    h.sync()
    return K.cpu().numpy()


def check_close(K, R, tol=1e-13):
    assert K.shape == R.shape
    nan = np.isnan(R)
    assert np.array_equal(np.isnan(K), nan)
    err = np.abs(K - R)[~nan]
    scale = np.maximum(np.abs(R[~nan]), 1.0)
    assert (err / scale).max(initial=0.0) <= tol, (err / scale).max()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", list(KINDS))
def test_pairwise_kernel_all_kinds(kind, dtype):
    rng = np.random.default_rng(1)
    for na, nb, d in [(67, 45, 37), (130, 1, 1), (64, 128, 96), (5, 70, 33)]:
        A = rng.standard_normal((na, d)).astype(dtype)
        B = rng.standard_normal((nb, d)).astype(dtype)
        if kind == "cosine":
            A[3 % na] = 0
            B[0] = 0
        mu = rng.standard_normal(d) * 0.3
        nu = rng.standard_normal(d) * 0.3
        for muA, muB in [(None, None), (mu, None), (None, nu), (mu, nu)]:
            Ac = A.astype(np.float64) - (0 if muA is None else muA)
            Bc = B.astype(np.float64) - (0 if muB is None else muB)
            R = np_kernel(kind, Ac, Bc, 0.3 / d, 2.5, 0.7, False)
            check_close(dev_kernel(A, B, kind, 0.3 / d, 2.5, 0.7, muA, muB), R)
        for muA in (None, mu):
            Ac = A.astype(np.float64) - (0 if muA is None else muA)
            K = dev_kernel(A, A, kind, 0.3 / d, 2.5, 0.7, muA, muA, symmetric=True)
            check_close(K, np_kernel(kind, Ac, Ac, 0.3 / d, 2.5, 0.7, True))
            assert np.array_equal(K, K.T, equal_nan=True)
            if kind == "rbf":
                assert np.all(np.diag(K) == 1.0)


def test_poly_real_exponent_gives_nan_like_numpy():
    A = np.array([[1.0, -2.0], [0.5, 0.25], [-3.0, 1.0]])
    K = dev_kernel(A, A[::-1].copy(), "poly", 1.0, 1.5, -0.5)
    R = np_kernel("poly", A, A[::-1], 1.0, 1.5, -0.5, False)
    assert np.isnan(R).any()
    check_close(K, R)


@pytest.mark.parametrize("k", [1, 16, 64, 100])
@pytest.mark.parametrize("kind", ["rbf", "poly", "cosine"])
def test_kernel_project_matches_explicit_product(kind, k):
    from cca_zoo_amd import _backend

    torch = torch_mod()
    rng = np.random.default_rng(k)
    na, nb, d = 150, 203, 19
    A = rng.standard_normal((na, d))
    B = rng.standard_normal((nb, d))
    mu = rng.standard_normal(d) * 0.2
    W = rng.standard_normal((na, k))
    R = np_kernel(kind, A - mu, B, 0.1, 2.0, 1.0, False).T @ W
    h = _backend.default_handle()
    At, Bt, mt, Wt = (torch.as_tensor(x, device="cuda") for x in (A, B, mu, W))
    out = torch.zeros((nb, k), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    h.check(h.lib.ccz_kernel_project(h.raw, _backend.F64, C.c_void_p(At.data_ptr()), na, d, C.c_void_p(mt.data_ptr()),
                                     C.c_void_p(Bt.data_ptr()), nb, d, None, d, KINDS[kind], 0.1, 2.0, 1.0,
                                     C.c_void_p(Wt.data_ptr()), k, k, C.c_void_p(out.data_ptr()), k))
    h.sync()
    got = out.cpu().numpy()
    assert np.linalg.norm(got - R) <= 1e-12 * np.linalg.norm(R)


def fit_case(case, tensors=False):
    import cca_zoo_amd.nonparametric as npm

    g, p, train, test = case_data(case)
    kw = {k: v for k, v in p.items() if k != "estimator"}
    model = getattr(npm, p["estimator"])(**kw)
    if tensors:
        torch = torch_mod()
        train = [torch.as_tensor(v, device="cuda") for v in train]
        test = [torch.as_tensor(v, device="cuda") for v in test]
    return g, p, model.fit(train), train, test


@pytest.mark.parametrize("case", CASES)
def test_estimator_against_reference_goldens(case):
    import json

    g, p, model, train, test = fit_case(case)
    m = len(train)
    dt = json.loads(str(g["dtypes"]))
    zt, zs = model.transform(train), model.transform(test)
    assert str(zt[0].dtype) == dt["transform"] and str(model.weights_[0].dtype) == dt["weights"]
    assert str(model.means_[0].dtype) == dt["means"]
    tz, ts = tolerance(case)
    tz = max(tz, 1e-6)
    if case == "kcca_c10":
        # c = 10 makes B = 10 K - 9 K^2 indefinite: its floor eps = 1e-3 is reached as a difference of ~2e4-sized
        # eigenvalues of B, which amplifies the device eigensolver's ~1e-14 relative eigenvalue error to ~1e-7 here
        ts = 1e-6
    for i in range(m):
        assert model.weights_[i].shape == g[f"w{i}"].shape
        assert col_err(zt[i], g[f"transform_train{i}"]) < tz
        assert col_err(zs[i], g[f"transform_test{i}"]) < tz
    np.testing.assert_allclose(model.score(train), g["score_train"], atol=ts)
    np.testing.assert_allclose(model.score(test), g["score_test"], atol=max(ts, 1e-8))
    R = model.pairwise_correlations(train)
    assert np.abs(np.abs(R) - np.abs(g["pairwise_train"])).max() < max(ts, 1e-8) * 10
    if case == "kcca_f32":   # the fp64 route on the same fp32 inputs is far tighter than the fp32 reference
        W, _, kf = route(train, p)
        np.testing.assert_allclose(model.score(train), avg_corr([kf[i](train[i]).T @ W[i] for i in range(m)]), atol=1e-5)


def test_factor_loadings_match_reference_formula():
    g, p, model, train, test = fit_case("kcca_rbf")
    got = model.get_factor_loadings(test)
    for i, (v, z) in enumerate(zip(test, model.transform(test))):
        vc, zc = v - v.mean(0), z - z.mean(0)
        ref = (vc.T @ zc / (v.shape[0] - 1)) / np.outer(np.maximum(vc.std(0, ddof=1), 1e-12),
                                                         np.maximum(zc.std(0, ddof=1), 1e-12))
        np.testing.assert_allclose(got[i], ref, atol=1e-10)
    ref_l = [g[f"loadings{i}"] for i in range(len(train))]
    for a, b in zip(model.get_factor_loadings(train), ref_l):
        assert np.abs(np.abs(a) - np.abs(b)).max() < 1e-6


def test_device_tensors_in_tensors_out():
    torch = torch_mod()
    g, p, model, train, test = fit_case("kcca_rbf", tensors=True)
    zs = model.transform(test)
    assert all(isinstance(z, torch.Tensor) and z.is_cuda and z.dtype == torch.float64 for z in zs)
    for i, z in enumerate(zs):
        assert col_err(z.cpu().numpy(), g[f"transform_test{i}"]) < 1e-6
    np.testing.assert_allclose(model.score(test), g["score_test"], atol=1e-8)


def correlated(n=300, seed=0):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, 2))
    return [z @ rng.standard_normal((2, 6)) + 0.2 * rng.standard_normal((n, 6)),
            z @ rng.standard_normal((2, 5)) + 0.2 * rng.standard_normal((n, 5))]


def test_reference_properties():
    from cca_zoo_amd.linear import CCA
    from cca_zoo_amd.nonparametric import KCCA, KGCCA

    views = correlated()
    s_cca = CCA(latent_dimensions=2).fit(views).score(views)
    s_k = KCCA(latent_dimensions=2, kernel="linear", c=1e-4).fit(views).score(views)
    np.testing.assert_allclose(s_k, s_cca, atol=1e-3)
    assert np.all(KCCA(latent_dimensions=1, c=0.01, kernel="rbf").fit(views).score(views) > 0.8)
    lo = KCCA(kernel="linear", c=1e-4).fit(views).score(views)
    hi = KCCA(kernel="linear", c=10.0).fit(views).score(views)
    assert lo[0] >= hi[0] - 1e-6
    rng = np.random.default_rng(99)
    test = [rng.standard_normal((10, 6)), rng.standard_normal((10, 5))]
    three = views + [views[0][:, :3] + 0.1]
    for est in (KCCA, KGCCA):
        mdl = est(latent_dimensions=2).fit(views)
        assert [w.shape for w in mdl.weights_] == [(300, 2), (300, 2)]
        assert [z.shape for z in mdl.transform(test)] == [(10, 2), (10, 2)]
        assert mdl.score(views).shape == (2,)
        assert mdl.pairwise_correlations(views).shape == (2, 2, 2)
        assert [l.shape for l in mdl.get_factor_loadings(views)] == [(6, 2), (5, 2)]
        assert len(est(center=False).fit(views).transform(views)) == 2
        assert len(est(kernel=["linear", "rbf"]).fit(views).transform(views)) == 2
        assert len(est().fit(three).transform(three)) == 3
        a = est().fit_transform(views)
        b = est().fit(views).transform(views)
        for x, y in zip(a, b):
            np.testing.assert_allclose(np.abs(x), np.abs(y), atol=1e-10)


def test_kcca_n2048_matches_scipy_statement_of_the_reference():
    import scipy.linalg
    from sklearn.metrics import pairwise_kernels

    from cca_zoo_amd.nonparametric import KCCA

    rng = np.random.default_rng(5)
    n = 2048
    z = rng.standard_normal((n, 2))
    views = [np.tanh(z @ rng.standard_normal((2, 24))) + 0.5 * rng.standard_normal((n, 24)) for _ in range(2)]
    model = KCCA(latent_dimensions=3, kernel="rbf").fit(views)
    tc = [v - v.mean(0) for v in views]
    K = [pairwise_kernels(v, metric="rbf", gamma=1.0 / 24) for v in tc]
    A = np.cov(np.hstack(K), rowvar=False)
    A[:n, :n] = 0
    A[n:, n:] = 0
    A /= 2
    B = scipy.linalg.block_diag(*[0.1 * k + 0.9 * k @ k for k in K])
    lmin = np.linalg.eigvalsh(B).min()
    if lmin < 1e-3:
        B += (1e-3 - lmin) * np.eye(2 * n)
    B /= 2
    w, V = scipy.linalg.eigh(A, B, subset_by_index=[2 * n - 4, 2 * n - 1])
    w, V = w[::-1], V[:, ::-1]
    np.testing.assert_allclose(model.eigenvalues_, w[:3], rtol=1e-8, atol=1e-10)
    v = np.vstack(model.weights_)
    res = np.linalg.norm(A @ v - (B @ v) * model.eigenvalues_, axis=0) / (np.linalg.norm(A, 2) * np.linalg.norm(v, axis=0))
    assert res.max() <= 1e-8, res
    np.testing.assert_allclose(np.sum(v * (B @ v), axis=0), 1.0, atol=1e-8)
    # the canonical directions as a whole: the top-3 training-transform subspace of the device against scipy's
    zs = model.transform(views)
    for i in range(2):
        ref = K[i].T @ V[i * n:(i + 1) * n, :3]
        qa, qb = np.linalg.qr(zs[i])[0], np.linalg.qr(ref)[0]
        assert np.linalg.svd(qa.T @ qb, compute_uv=False).min() > 0.99


def test_kcca_n8192_generalised_residual_on_device():
    """||A v - lambda B v|| / (||A||_2 ||v||) <= 1e-10 at n = 8192, with A v and B v formed by ccz_gemm_f64.  ||A||_2 is
    sigma_max(C_12) / 2, estimated from below by power iteration (which only makes the bound stricter).  B is taken without
    a shift, and that is asserted: every eigenvalue of c K_i + (1 - c) K_i^2, from ccz_syevj of K_i, is >= 10 eps."""
    from cca_zoo_amd import _backend
    from cca_zoo_amd.nonparametric import KCCA
    from cca_zoo_amd.nonparametric._kernel_base import _DevView, pairwise_kernel

    torch = torch_mod()
    n, d, k, c, eps = 8192, 256, 4, 0.1, 1e-3
    g = torch.Generator(device="cuda").manual_seed(3)
    z = torch.randn((n, 2), device="cuda", dtype=torch.float64, generator=g)
    views = [torch.tanh(z @ torch.randn((2, d), device="cuda", dtype=torch.float64, generator=g))
             + torch.randn((n, d), device="cuda", dtype=torch.float64, generator=g) for _ in range(2)]
    model = KCCA(latent_dimensions=k, kernel="rbf", c=c, eps=eps).fit(views)
    h = _backend.handle_for(views)
    Ks = []
    for v in model.train_views_:
        K = torch.empty((n, n), dtype=torch.float64, device="cuda")
        dv = _DevView(h, v)
        pairwise_kernel(h, dv, dv, model._specs[0], K.data_ptr(), n)
        Ks.append(K)
    h.sync()
    for K in Ks:   # no shift: min eig(c K + (1 - c) K^2) well above eps
        Kw, lam = K.clone(), torch.empty(n, dtype=torch.float64, device="cuda")
        Vw = torch.empty((n, n), dtype=torch.float64, device="cuda")
        h.check(h.lib.ccz_syevj(h.raw, C.c_void_p(Kw.data_ptr()), n, C.c_void_p(lam.data_ptr()), C.c_void_p(Vw.data_ptr()),
                                None))
        h.sync()
        assert float((c * lam + (1 - c) * lam * lam).min()) >= 10 * eps
        del Kw, Vw
    Kc = [K - K.mean(dim=0, keepdim=True) for K in Ks]
    V = [torch.as_tensor(w, device="cuda") for w in model.weights_]
    lam = torch.as_tensor(model.eigenvalues_, device="cuda")

    def mm(X, Y, tA=False):
        out = torch.empty((X.shape[1] if tA else X.shape[0], Y.shape[1]), dtype=torch.float64, device="cuda")
        h.gemm(1 if tA else 0, 0, out.shape[0], out.shape[1], Y.shape[0], 1.0, X.data_ptr(), X.shape[1], Y.data_ptr(),
               Y.shape[1], 0.0, out.data_ptr(), out.shape[1])
        return out

    torch.cuda.synchronize()
    Av = [mm(Kc[0], mm(Kc[1], V[1]), tA=True) / (2 * (n - 1)), mm(Kc[1], mm(Kc[0], V[0]), tA=True) / (2 * (n - 1))]
    Bv = [(c * mm(Ks[i], V[i]) + (1 - c) * mm(Ks[i], mm(Ks[i], V[i]))) / 2 for i in range(2)]
    x = torch.ones((n, 1), dtype=torch.float64, device="cuda")
    for _ in range(40):   # power iteration on C_12' C_12 (C_12 = Kc_1' Kc_2 / (n - 1))
        y = mm(Kc[1], mm(Kc[0], mm(Kc[0], mm(Kc[1], x)), tA=True), tA=True)
        x = y / torch.linalg.norm(y)
    sigma = torch.linalg.norm(mm(Kc[0], mm(Kc[1], x), tA=True)) / (n - 1)
    h.sync()
    res = torch.linalg.norm(torch.cat([Av[i] - lam * Bv[i] for i in range(2)]), dim=0)
    nv = torch.linalg.norm(torch.cat(V), dim=0)
    assert float((res / (sigma / 2 * nv)).max()) <= 1e-10
    vBv = sum((V[i] * Bv[i]).sum(0) for i in range(2))
    assert torch.allclose(vBv, torch.ones_like(vBv), atol=1e-8)


@pytest.mark.parametrize("fit_dtype,test_dtype", [("float64", "float32"), ("float32", "float64"), ("float32", "float32")])
def test_transform_under_a_side_stream_with_dtype_conversion(fit_dtype, test_dtype):
    """Conversions of the training / test views happen on the caller's stream; the projection must wait for them, and
    they must stay alive until it is done, whatever stream the caller is on.  Mixed dtypes go through float64 on both
    sides (as sklearn's check_pairwise_arrays does), float32 pairs stay float32."""
    from cca_zoo_amd.nonparametric import KCCA

    torch = torch_mod()
    g, p, _, train, test = fit_case("kcca_rbf")
    f = {"float32": torch.float32, "float64": torch.float64}
    tr = [torch.as_tensor(v, device="cuda").to(f[fit_dtype]) for v in train]
    te = [torch.as_tensor(v, device="cuda").to(f[test_dtype]) for v in test]
    model = KCCA(latent_dimensions=3, kernel="rbf").fit(tr)
    ref = [model.transform([t.double() for t in te])[i].cpu().numpy() for i in range(2)] if fit_dtype == "float64" else None
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        big = torch.randn((4096, 4096), device="cuda", dtype=torch.float64)
        for _ in range(4):   # keep the side stream busy so that an unordered read would see unfinished copies
            big = big @ big / 64.0
        strided = [t.t().contiguous().t() for t in te]   # non-contiguous rows: transform makes a contiguous copy
        zs = model.transform(strided)
        del strided
        torch.cuda._sleep(1000000)
        zs = [z.clone() for z in zs]
    side.synchronize()
    exp_dt = np.float32 if (fit_dtype == "float32" and test_dtype == "float32") else np.float64
    for i, z in enumerate(zs):
        tr_i = model.train_views_[i].cpu().numpy().astype(exp_dt).astype(np.float64)
        te_i = te[i].cpu().numpy().astype(exp_dt).astype(np.float64)
        K = np_kernel("rbf", tr_i, te_i, model._specs[i][1], 1.0, 1.0, False)
        want = K.T @ model.weights_[i]
        assert np.linalg.norm(z.cpu().numpy() - want) <= 1e-10 * np.linalg.norm(want)
        if ref is not None and test_dtype == "float32":
            assert col_err(z.cpu().numpy(), ref[i]) < 1e-5
