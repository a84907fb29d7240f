"""CPU tests of TCCA / KTCCA: the public surface, the refusals that must fire before the device is touched, and the NumPy
restatement (tests/tcca_fit_restatement.py) against the reference's own arrays in the ``tccafit_*`` goldens
(tools/gen_golden_tcca_fit.py).  These tests run without a GPU: a refusal that reached the device would surface as a load
or runtime error instead of the asserted ``ValueError`` / ``TypeError``."""

import numpy as np
import pytest
from sklearn.base import clone

from conftest import load_golden
from tcca_fit_restatement import (TOL, align_signs, cp_als, cp_to_tensor, dense_error, khatri_rao, ktcca_fit, ktcca_transform,
                                  svd_init, tcca_fit)

#: tag -> what the golden tool passed to the model besides latent_dimensions (stored as ``k``)
CASES = {
    "three": {}, "k1": {}, "four": dict(c=0.1), "two": {}, "three17": dict(c=[0.0, 0.2, 0.05]), "k8": {}, "five": {},
    "narrowest": {}, "width1": {}, "nocenter": dict(center=False), "eps_shift": dict(eps=1e-2), "long": {}, "cap": {},
    "f32_three": {}, "f32_four": dict(c=0.1),
}
KCASES = {
    "k_rbf": dict(kernel="rbf"), "k_poly": dict(kernel="poly", degree=2.0, c=0.5, eps=0.1),
    "k_linear": dict(kernel="linear", c=[0.1, 0.3, 0.2], eps=0.1), "k_f32": dict(kernel="rbf"),
}
F32 = ("f32_three", "f32_four", "k_f32")

_cache = {}


def golden_case(tag):
    """(golden arrays, views as stored, restatement's fit of their float64 cast), computed once per case."""
    if tag not in _cache:
        g = load_golden(f"tccafit_{tag}")
        views = [g[f"x{i}"] for i in range(sum(k.startswith("x") for k in g))]
        k = int(g["k"])
        v64 = [v.astype(np.float64) for v in views]
        fit = ktcca_fit(v64, k, **KCASES[tag]) if tag in KCASES else tcca_fit(v64, k, **CASES[tag])
        _cache[tag] = (g, views, fit)
    return _cache[tag]


def col_gap(w, ref):
    return np.linalg.norm(w * align_signs(w, ref) - ref, axis=0) / np.linalg.norm(ref, axis=0)


# ---- surface ---------------------------------------------------------------------------------------------------------------
def test_exports_and_constructor_round_trip():
    from cca_zoo_amd.linear import TCCA
    from cca_zoo_amd.nonparametric import KTCCA
    import cca_zoo_amd.linear as lin
    import cca_zoo_amd.nonparametric as nonp

    assert "TCCA" in lin.__all__ and "KTCCA" in nonp.__all__
    t = TCCA(latent_dimensions=3, center=False, c=[0.1, 0.2, 0.3], eps=1e-4, random_state=5)
    assert t.get_params() == dict(latent_dimensions=3, center=False, c=[0.1, 0.2, 0.3], eps=1e-4, random_state=5)
    assert clone(t).get_params() == t.get_params()
    assert TCCA().get_params() == dict(latent_dimensions=1, center=True, c=0.0, eps=1e-6, random_state=None)
    kt = KTCCA(latent_dimensions=2, kernel=["rbf", "poly", "linear"], gamma=[0.5, None, None], degree=2.0, c=0.3)
    assert clone(kt).get_params() == kt.get_params()
    assert KTCCA().get_params() == dict(latent_dimensions=1, center=True, c=0.1, kernel="linear", gamma=None, degree=1.0, coef0=1.0,
                                        kernel_params=None, eps=1e-3, random_state=None)


def _views(n, widths, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, d)) for d in widths]


@pytest.mark.parametrize("params, widths, n", [
    (dict(latent_dimensions=33), (40, 40), 50),                 # above 32
    (dict(latent_dimensions=4), (5, 3, 6), 50),                 # above the narrowest view
    (dict(latent_dimensions=2), (5, 1, 6), 50),                 # a width of 1 with k = 2
    (dict(latent_dimensions=1), (2,) * 9, 50),                  # nine views
    (dict(latent_dimensions=1), (5,), 50),                      # one view
    (dict(latent_dimensions=1), (4097, 4096), 3),               # more than 2^24 tensor entries
    (dict(latent_dimensions=1), (5, 4), 1),                     # one sample
    (dict(latent_dimensions=1, c=[0.1, 0.2, 0.3]), (5, 4), 50),  # c per view, wrong length
    (dict(latent_dimensions=1, c=1.5), (5, 4), 50),
    (dict(latent_dimensions=1, eps=0.0), (5, 4), 50),
    (dict(latent_dimensions=0), (5, 4), 50),
    (dict(latent_dimensions=1, random_state=-1), (5, 4), 50),
])
def test_tcca_refuses_before_the_device_is_touched(params, widths, n):
    from cca_zoo_amd.linear import TCCA

    with pytest.raises(ValueError):
        TCCA(**params).fit(_views(n, widths))


def test_tcca_refuses_unequal_sample_counts():
    from cca_zoo_amd.linear import TCCA

    with pytest.raises(ValueError):
        TCCA().fit([np.zeros((10, 3)), np.zeros((11, 3))])


@pytest.mark.parametrize("params, widths, n, error", [
    (dict(kernel="laplacian"), (5, 4, 3), 20, ValueError),                        # not a device kernel
    (dict(kernel="rbf", kernel_params={"gamma": 0.5}), (5, 4, 3), 20, TypeError),  # repeats a constructor argument
    (dict(latent_dimensions=21), (5, 4, 3), 20, ValueError),                      # above the number of samples
    (dict(latent_dimensions=33), (5, 4), 50, ValueError),                         # above 32
    (dict(), (5, 4, 3), 257, ValueError),                                         # 257^3 > 2^24
    (dict(), (5, 4), 4097, ValueError),                                           # 4097^2 > 2^24
    (dict(), (2,) * 9, 4, ValueError),                                            # nine views
    (dict(c=[0.1, 0.2]), (5, 4, 3), 20, ValueError),                              # c per view, wrong length
    (dict(kernel=["rbf", "rbf"]), (5, 4, 3), 20, ValueError),
    (dict(), (5, 4, 3), 1, ValueError),
])
def test_ktcca_refuses_before_the_device_is_touched(params, widths, n, error):
    from cca_zoo_amd.nonparametric import KTCCA

    with pytest.raises(error):
        KTCCA(**params).fit(_views(n, widths))


def test_fit_inside_row_sharded_is_refused(monkeypatch):
    from cca_zoo_amd import _dist
    from cca_zoo_amd.linear import TCCA
    from cca_zoo_amd.nonparametric import KTCCA

    monkeypatch.setattr(_dist, "is_sharded", lambda: True)
    with pytest.raises(NotImplementedError, match="row_sharded"):
        TCCA().fit(_views(20, (5, 4, 3)))
    with pytest.raises(NotImplementedError, match="row_sharded"):
        KTCCA().fit(_views(20, (5, 4, 3)))


# ---- the restatement against the reference's own arrays ------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(CASES) + list(KCASES))
def test_restatement_reproduces_the_reference_arrays(tag):
    g, views, fit = golden_case(tag)
    M = g["M"]
    assert fit["M"].shape == M.shape
    assert np.abs(fit["M"] - M).max() <= 1e-10 * np.abs(M).max()
    for i in range(len(views)):
        F = g[f"invsqrt{i}"]
        assert np.abs(fit["invsqrt"][i] - F).max() <= 1e-10 * np.abs(F).max()
        assert col_gap(fit["weights"][i], g[f"w{i}"]).max() <= 1e-10
    assert fit["n_iter"] == int(g["n_iter"])
    assert np.abs(fit["trace"] - g["trace"]).max() <= 1e-12
    if tag in F32:
        assert all(v.dtype == np.float32 for v in views) and g["gap32"].shape == (len(views), int(g["k"]))
        assert int(g["n_iter32"]) == int(g["n_iter"])


@pytest.mark.parametrize("tag", list(KCASES))
def test_restatement_reproduces_the_reference_transform(tag):
    g, views, fit = golden_case(tag)
    held = [g[f"t{i}"].astype(np.float64) for i in range(len(views))]
    for z, ref in zip(ktcca_transform(fit, held), [g[f"z{i}"] for i in range(len(views))]):
        assert np.abs(z * align_signs(z, ref) - ref).max() <= 1e-10 * np.abs(ref).max()


def test_goldens_cover_what_they_are_meant_to():
    n_iter = {tag: int(golden_case(tag)[0]["n_iter"]) for tag in CASES}
    assert n_iter["cap"] == 100 and 16 < n_iter["long"] < 100
    orders = {golden_case(tag)[0]["M"].ndim for tag in CASES}
    assert {2, 3, 4, 5} <= orders
    assert int(golden_case("k1")[0]["k"]) == 1 and int(golden_case("k8")[0]["k"]) == 8
    assert int(golden_case("narrowest")[0]["k"]) == min(golden_case("narrowest")[0]["M"].shape)
    assert 1 in golden_case("width1")[0]["M"].shape
    x0 = golden_case("eps_shift")[1][0]
    lam = np.linalg.eigvalsh(np.cov(x0, rowvar=False)).min()
    assert 5e-5 < lam < 2e-4          # the eps = 1e-2 shift fires on this view


@pytest.mark.parametrize("tag", list(CASES) + list(KCASES))
def test_error_formula_and_trace(tag):
    """The iteration's error (from normM, the Grams and the last MTTKRP) is the dense ``||M - [[A]]|| / ||M||``; ALS never
    increases it (4 ulp of slack for a trace that has converged to rounding)."""
    g, views, fit = golden_case(tag)
    assert abs(fit["trace"][-1] - dense_error(fit["M"], fit["factors"])) <= 1e-10
    for n_iter in (1, 2, 3):
        A, tr = cp_als(fit["M"], int(g["k"]), n_iter_max=n_iter)
        assert abs(tr[-1] - dense_error(fit["M"], A)) <= 1e-10
    assert np.all(np.diff(g["trace"]) <= 4 * np.finfo(float).eps)


@pytest.mark.parametrize("dims, k", [((6, 5, 4), 2), ((7, 5), 3), ((4, 3, 3, 2), 2), ((12, 10, 9), 8), ((5, 1, 4), 1)])
def test_exact_rank_tensor_is_recovered(dims, k):
    rng = np.random.default_rng(sum(dims) + k)
    A = [np.linalg.qr(rng.standard_normal((d, k)))[0] for d in dims]
    M = (khatri_rao(A) * (1.5 ** -np.arange(k))).sum(axis=1).reshape(dims)
    got, trace = cp_als(M, k)
    assert dense_error(M, got) < 1e-6
    assert np.abs(cp_to_tensor(got) - M).max() < 1e-6 * np.abs(M).max()


def test_svd_init_sign_rule_and_rank_refusal():
    rng = np.random.default_rng(3)
    M = rng.standard_normal((5, 4, 3))
    for A in svd_init(M, 3):
        top = np.abs(A).argmax(axis=0)
        assert np.all(A[top, np.arange(3)] > 0)
        assert np.allclose(A.T @ A, np.eye(3), atol=1e-12)
    with pytest.raises(ValueError):
        svd_init(M, 4)
    assert TOL == 1e-8
