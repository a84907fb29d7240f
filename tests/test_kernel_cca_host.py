"""CPU tests of the nonparametric module (KCCA / KGCCA): ABI surface, estimator contract, early errors, and a float64
NumPy restatement of the device route checked against the reference's goldens (tests/golden/kernel_cca_*.npz).

The restatement takes the kernel matrices from scikit-learn (as the reference does) and re-derives everything after
them the way csrc/kcca.cpp does: one eigendecomposition per kernel matrix, the two-view KCCA as a top-k SVD of the
whitened cross-covariance, more views as a dense EVD of the whitened A, KGCCA's Q through a factor of it and pinv(K_i)
in the eigenbasis.  It validates the maths of the route apart from the HIP kernels."""

from __future__ import annotations

import glob
import json
import os
import re

import numpy as np
import pytest
from sklearn.metrics import pairwise_kernels

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(os.path.basename(f)[len("kernel_cca_"):-len(".npz")]
               for f in glob.glob(os.path.join(ROOT, "tests", "golden", "kernel_cca_*.npz")))
NEW_SYMBOLS = {"ccz_pairwise_kernel", "ccz_kernel_project", "ccz_kcca_solve", "ccz_kgcca_solve"}


def kernel_fns(views, p):
    m = len(views)
    kern = p.get("kernel", "linear")
    kern = kern if isinstance(kern, list) else [kern] * m
    return [lambda Y, v=v, kn=kern[i]: np.asarray(
        pairwise_kernels(v, Y=Y, metric=kn, gamma=p.get("gamma"), degree=p.get("degree", 1.0), coef0=p.get("coef0", 1.0),
                         filter_params=True), dtype=np.float64) for i, v in enumerate(views)]


def route(train, p):
    """(weights, means, kernel functions of the centred training views) by the device route, in float64 NumPy."""
    m, n, k = len(train), train[0].shape[0], p.get("latent_dimensions", 1)
    center = p.get("center", True)
    means = [v.mean(0) if center else np.zeros(v.shape[1]) for v in train]
    tc = [v - mu for v, mu in zip(train, means)]
    kf = kernel_fns(tc, p)
    K = [kf[i](tc[i]) for i in range(m)]
    c = p.get("c", 0.1)
    c = c if isinstance(c, list) else [c] * m
    lam, U = zip(*[np.linalg.eigh(Ki) for Ki in K])
    b = [c[i] * lam[i] + (1 - c[i]) * lam[i] ** 2 for i in range(m)]
    if p["estimator"] == "KCCA":
        shift = max(0.0, p.get("eps", 1e-3) - min(bb.min() for bb in b))
        beta = [bb + shift for bb in b]
        P = [U[i] * (lam[i] / np.sqrt(beta[i])) for i in range(m)]
        P = [Pi - Pi.mean(0) for Pi in P]              # H U diag(l / sqrt(b)) = Kc B^-1/2 in the eigenbasis
        if m == 2:
            u, s, vt = np.linalg.svd(P[0].T @ P[1] / (n - 1))
            W = [U[0] @ (u[:, :k] / np.sqrt(beta[0])[:, None]), U[1] @ (vt[:k].T / np.sqrt(beta[1])[:, None])]
        else:
            T = np.zeros((m * n, m * n))
            for i in range(m):
                for j in range(m):
                    if i != j:
                        T[i * n:(i + 1) * n, j * n:(j + 1) * n] = P[i].T @ P[j] / (n - 1)
            V = np.linalg.eigh(T)[1][:, ::-1][:, :k]
            W = [np.sqrt(m) * U[i] @ (V[i * n:(i + 1) * n] / np.sqrt(beta[i])[:, None]) for i in range(m)]
    else:
        eps = p.get("eps", 1e-6)
        mu = p.get("view_weights") or [1.0] * m
        G = np.hstack([np.sqrt(mu[i]) * U[i] * (lam[i] / np.sqrt(b[i] + max(0.0, eps - b[i].min()))) for i in range(m)])
        T = np.linalg.svd(G, full_matrices=False)[0][:, :k]
        W = []
        for i in range(m):
            keep = np.abs(lam[i]) > 1e-15 * np.abs(lam[i]).max()
            pinv = np.where(keep, 1.0 / np.where(keep, lam[i], 1.0), 0.0)
            W.append(U[i] @ (pinv[:, None] * (U[i].T @ T)))
    return W, means, kf


def avg_corr(zs):
    m, k = len(zs), zs[0].shape[1]
    out = np.zeros(k)
    for i in range(m):
        for j in range(m):
            if i != j:
                out += [np.corrcoef(zs[i][:, t], zs[j][:, t])[0, 1] for t in range(k)]
    return out / (m * (m - 1))


def col_err(z, ref):
    s = np.sign(np.sum(z * ref, axis=0))
    s[s == 0] = 1.0
    return float((np.linalg.norm(z * s - ref, axis=0) / np.linalg.norm(ref, axis=0)).max())


def case_data(case):
    g = load_golden("kernel_cca_" + case)
    p = json.loads(str(g["params"]))
    m = sum(1 for key in g if re.fullmatch(r"train\d+", key))
    return g, p, [g[f"train{i}"] for i in range(m)], [g[f"test{i}"] for i in range(m)]


def tolerance(case):
    """1e-8, except where the reference's own answer is less precise than that:
    - fp32 inputs: the reference forms B = c K + (1 - c) K @ K in float32 (sklearn returns float32 kernels), ~1e-3;
    - KGCCA with rbf kernels: the reference inverts each B_i, whose smallest eigenvalue sits at the eps = 1e-6 floor
      (its transforms move by ~1e-7 under rounding-level perturbations);
    - KGCCA with a full-rank linear kernel: the reference's pinv(K) of an ill-conditioned K, ~2e-8."""
    if case == "kcca_f32":
        return 1e-2, 1e-3
    if case == "kgcca_linear_full":
        return 1e-7, 1e-8
    if case.startswith("kgcca"):
        return 1e-6, 1e-6
    return 1e-8, 1e-8


def test_new_entry_points_are_declared_and_bound():
    from cca_zoo_amd import _backend

    header = open(os.path.join(ROOT, "include", "ccz.h")).read()
    declared = set(re.findall(r"CCZ_API\s+(?:const\s+char\*|int64_t|int)\s+(ccz_\w+)\s*\(", header))
    assert NEW_SYMBOLS <= declared
    assert NEW_SYMBOLS <= set(_backend.SIGNATURES)
    assert declared == set(_backend.SIGNATURES)
    src = open(os.path.join(ROOT, "cca_zoo_amd", "csrc", "build.py")).read()
    assert '"kernel_matrix.hip"' in src and '"kcca.cpp"' in src


def test_build_lists_name_every_source_and_header():
    """build() takes staleness and the link line from these two lists: a file missing from them is not built, or not watched."""
    from cca_zoo_amd.csrc import build

    csrc = os.path.join(ROOT, "cca_zoo_amd", "csrc")
    names = [f for f in os.listdir(csrc) if os.path.isfile(os.path.join(csrc, f))]
    assert len(build.SOURCES) == len(set(build.SOURCES)) and len(build.HEADERS) == len(set(build.HEADERS))
    assert set(build.SOURCES) == {f for f in names if f.endswith((".hip", ".cpp"))}
    headers = {os.path.join(csrc, f) for f in names if f.endswith(".h")} | {os.path.join(ROOT, "include", "ccz.h")}
    assert {os.path.normpath(os.path.join(csrc, h)) for h in build.HEADERS} == headers


def test_solve_cpp_does_not_call_the_kernel_ops():
    """The host test double compiles solve.cpp alone: the KCCA drivers must live elsewhere."""
    src = open(os.path.join(ROOT, "cca_zoo_amd", "csrc", "solve.cpp")).read()
    for name in ("pairwise_kernel", "kernel_project", "kcca_solve", "kgcca_solve"):
        assert name not in src


@pytest.mark.parametrize("name", ["KCCA", "KGCCA"])
def test_sklearn_estimator_checks(name):
    from sklearn.utils.estimator_checks import (check_estimator_repr, check_get_params_invariance,
                                                check_no_attributes_set_in_init, check_set_params)

    import cca_zoo_amd.nonparametric as npm

    est = getattr(npm, name)()
    check_no_attributes_set_in_init(name, est)
    check_get_params_invariance(name, est)
    check_set_params(name, est)
    check_estimator_repr(name, est)


def test_defaults_match_the_reference():
    from cca_zoo_amd.nonparametric import KCCA, KGCCA

    a, b = KCCA().get_params(), KGCCA().get_params()
    assert a["eps"] == 1e-3 and b["eps"] == 1e-6
    for p in (a, b):
        assert p["c"] == 0.1 and p["kernel"] == "linear" and p["gamma"] is None
        assert p["degree"] == 1.0 and p["coef0"] == 1.0 and p["latent_dimensions"] == 1 and p["center"] is True
    assert b["view_weights"] is None
    import cca_zoo_amd

    assert "nonparametric" in cca_zoo_amd.__all__


@pytest.mark.parametrize("kernel", ["laplacian", "chi2", "additive_chi2", "precomputed", lambda a, b: 0.0])
@pytest.mark.parametrize("name", ["KCCA", "KGCCA"])
def test_unsupported_kernels_raise_before_device_work(name, kernel, monkeypatch):
    import cca_zoo_amd.nonparametric as npm
    from cca_zoo_amd import _backend

    def no_device(*a, **k):
        raise AssertionError("device touched")

    monkeypatch.setattr(_backend, "handle_for", no_device)
    monkeypatch.setattr(_backend, "default_handle", no_device)
    x = np.random.default_rng(0).standard_normal((20, 3))
    with pytest.raises(ValueError, match="supported kernels"):
        getattr(npm, name)(kernel=kernel).fit([x, x + 1])


def test_negative_view_weights_rejected(monkeypatch):
    from cca_zoo_amd import _backend
    from cca_zoo_amd.nonparametric import KGCCA

    monkeypatch.setattr(_backend, "handle_for", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device")))
    x = np.random.default_rng(0).standard_normal((20, 3))
    with pytest.raises(ValueError, match="non-negative"):
        KGCCA(view_weights=[1.0, -1.0]).fit([x, x])


def test_gamma_none_is_one_over_features():
    from cca_zoo_amd.nonparametric._kernel_base import kernel_specs

    specs = kernel_specs(["rbf", "poly", "linear"], None, 2.0, 0.5, None, 3, [4, 8, 5])
    assert specs == [(2, 0.25, 2.0, 0.5), (1, 0.125, 2.0, 0.5), (0, 0.0, 2.0, 0.5)]


def test_fit_inside_row_sharded_is_refused(monkeypatch):
    from cca_zoo_amd import _dist
    from cca_zoo_amd.nonparametric import KCCA

    monkeypatch.setattr(_dist, "is_sharded", lambda: True)
    x = np.zeros((10, 2))
    with pytest.raises(NotImplementedError, match="does not shard"):
        KCCA().fit([x, x])


def test_no_gpu_fails_loudly():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from cca_zoo_amd.nonparametric import KCCA, KGCCA

    x = np.random.default_rng(0).standard_normal((12, 3))
    for est in (KCCA(), KGCCA()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.fit([x, x + 1])


def test_goldens_cover_the_cases():
    assert {"kcca_linear", "kcca_poly", "kcca_rbf", "kcca_sigmoid", "kcca_cosine", "kcca_perview", "kcca_3views",
            "kcca_nocenter", "kcca_f32", "kcca_params", "kcca_c1e-4", "kcca_c10", "kgcca_rbf2", "kgcca_rbf3", "kgcca_vw",
            "kgcca_linear_full"} <= set(CASES)
    for case in CASES:
        g, p, train, _ = case_data(case)
        dt = json.loads(str(g["dtypes"]))
        assert dt["transform"] == "float64" and dt["weights"] == "float64"
        assert dt["means"] == ("float32" if train[0].dtype == np.float32 and p.get("center", True) else "float64")


@pytest.mark.parametrize("case", CASES)
def test_route_reproduces_the_reference(case):
    g, p, train, test = case_data(case)
    W, means, kf = route(train, p)
    m = len(train)
    tz, ts = tolerance(case)
    zt = [kf[i](train[i]).T @ W[i] for i in range(m)]
    zs = [kf[i](test[i]).T @ W[i] for i in range(m)]
    for i in range(m):
        assert col_err(zt[i], g[f"transform_train{i}"]) < tz
        assert col_err(zs[i], g[f"transform_test{i}"]) < tz
        np.testing.assert_allclose(means[i], g[f"mean{i}"], rtol=1e-6 if case == "kcca_f32" else 1e-12, atol=1e-12)
    np.testing.assert_allclose(avg_corr(zt), g["score_train"], atol=ts)
    np.testing.assert_allclose(avg_corr(zs), g["score_test"], atol=max(ts, 1e-8))
    if case in ("kcca_rbf", "kcca_poly", "kcca_params", "kcca_3views", "kcca_nocenter", "kcca_c1e-4", "kcca_sigmoid",
                "kcca_c10"):   # every K_i full rank: the weights themselves are determined
        for i in range(m):
            assert col_err(W[i], g[f"w{i}"]) < 1e-8
