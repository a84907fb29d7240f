"""CPU tests of CCAR3: the estimator's surface and refusals (all raised before the device is touched: on a machine without
a GPU the first device call raises ``RuntimeError``, which none of these expects), and the NumPy restatement
(tests/ccar3_restatement.py) against the goldens captured from the reference (tools/gen_golden_ccar3.py)."""

import numpy as np
import pytest
from conftest import load_golden

import ccar3_restatement as R

TAGS = ("lowdim", "dense", "sparse", "p_gt_n", "nolw_nocenter", "lw_nocenter", "tight", "allzero", "k_gt_q", "q1", "wide_q",
        "rows517", "maxiter", "rankdef_y", "f32", "f32_p_gt_n")
PARAMS = ("latent_dimensions", "center", "lambda_", "highdim", "ledoit_wolf", "rho", "max_iter", "tol", "eps")
BAR = 1e-10

_cache = {}


def params_of(g):
    return {k: g[f"param_{k}"].item() for k in PARAMS}


def restated(tag):
    """(golden, restatement's fit on the float64 cast of its views), computed once per case."""
    if tag not in _cache:
        g = load_golden(f"ccar3_{tag}")
        par = params_of(g)
        par["ledoit_wolf_"] = par.pop("ledoit_wolf")
        _cache[tag] = (g, R.fit([g["x0"].astype(np.float64), g["x1"].astype(np.float64)], **par))
    return _cache[tag]


def test_export_params_and_clone():
    from sklearn.base import clone

    import cca_zoo_amd.linear as lin
    from cca_zoo_amd.linear import CCAR3

    assert "CCAR3" in lin.__all__
    est = CCAR3(2, lambda_=0.3, highdim=False, rho=2.0, tol=1e-6)
    assert est.get_params() == dict(latent_dimensions=2, center=True, lambda_=0.3, highdim=False, ledoit_wolf=True, rho=2.0,
                                    max_iter=10_000, tol=1e-6, eps=1e-8)
    assert clone(est).get_params() == est.get_params() and repr(clone(est)) == repr(est)
    assert CCAR3().get_params() == dict(latent_dimensions=1, center=True, lambda_=0.0, highdim=True, ledoit_wolf=True, rho=1.0,
                                        max_iter=10_000, tol=1e-4, eps=1e-8)


def test_refusals_fire_before_the_device_is_touched():
    from cca_zoo_amd.linear import CCAR3

    X, Y = np.zeros((6, 3)), np.zeros((6, 2))
    with pytest.raises(ValueError, match="CCAR3 requires exactly 2 views, got 3"):
        CCAR3().fit([X, Y, X])
    with pytest.raises(ValueError, match="same number of samples"):
        CCAR3().fit([X, np.zeros((5, 2))])
    with pytest.raises(ValueError, match="exceed the device path's limit of 16384"):
        CCAR3().fit([np.zeros((2, 16380)), np.zeros((2, 5))])
    with pytest.raises(ValueError, match="at most 1024"):
        CCAR3().fit([np.zeros((2, 3)), np.zeros((2, 1025))])


def test_a_fit_inside_row_sharded_is_refused(monkeypatch):
    from cca_zoo_amd import _dist
    from cca_zoo_amd.linear import CCAR3

    monkeypatch.setattr(_dist, "is_sharded", lambda: True)
    with pytest.raises(NotImplementedError, match="row_sharded"):
        CCAR3().fit([np.zeros((6, 3)), np.zeros((6, 2))])


def test_mixed_host_and_device_views_are_refused():
    from cca_zoo_amd.linear import CCAR3

    class FakeTensor:
        is_cuda = True
        shape = (6, 3)

        class dtype:
            is_floating_point = True

        def dim(self):
            return 2

        def element_size(self):
            return 8

    FakeTensor.__module__ = "torch.fake"
    with pytest.raises(ValueError, match="all host arrays or all CUDA tensors"):
        CCAR3().fit([FakeTensor(), np.zeros((6, 2))])


@pytest.mark.parametrize("bad", [dict(lambda_=-0.1), dict(lambda_="a"), dict(highdim="yes"), dict(ledoit_wolf=1), dict(rho=0.0),
                                 dict(rho=-1.0), dict(max_iter=0), dict(max_iter=2.5), dict(tol=0.0), dict(eps=0.0),
                                 dict(latent_dimensions=0), dict(center="no")])
def test_every_invalid_parameter_is_refused(bad):
    from sklearn.utils._param_validation import InvalidParameterError

    from cca_zoo_amd.linear import CCAR3

    with pytest.raises(InvalidParameterError):
        CCAR3(**bad).fit([np.zeros((6, 3)), np.zeros((6, 2))])


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_agrees_with_the_reference(tag):
    g, rs = restated(tag)
    gaps = R.col_gap(rs["weights"], [g["w0"], g["w1"]])
    b_err = np.linalg.norm(rs["B"] - g["B"]) / max(np.linalg.norm(g["B"]), 1e-300)
    print(tag, "columns", gaps.max(), "B", b_err, "n_iter", rs["n_iter"])
    assert rs["n_iter"] == int(g["n_iter"])
    assert np.array_equal(~np.any(rs["B"], axis=1), ~np.any(g["B"], axis=1))
    assert np.array_equal(~np.any(rs["weights"][0], axis=1), ~np.any(g["w0"], axis=1))
    assert gaps.max() <= BAR and b_err <= BAR
    if rs["n_iter"]:
        assert np.abs(rs["res"][-2:] - g["res_last2"]).max() <= 1e-12 * max(1.0, np.abs(g["res_last2"]).max())


@pytest.mark.parametrize("tag", TAGS)
def test_ledoit_wolf_moment_form_agrees_with_the_stored_covariance(tag):
    from cca_zoo_amd.linear._ccar3 import shrunk_covariance

    g, rs = restated(tag)
    assert np.abs(rs["Sy"] - g["Sy"]).max() <= BAR * np.abs(g["Sy"]).max()
    if bool(g["param_ledoit_wolf"]):
        m = R.moments(g["x0"], g["x1"], bool(g["param_center"]))
        Sy, shrinkage = shrunk_covariance(m["C"].copy(), m["fourth"], m["n"])      # the estimator's own host form
        assert np.abs(Sy - g["Sy"]).max() <= BAR * np.abs(g["Sy"]).max()
        assert 0.0 <= shrinkage <= 1.0 and shrinkage == rs["shrinkage"]


def test_the_cases_cover_what_they_are_there_for():
    zero = {t: int((~np.any(restated(t)[0]["B"], axis=1)).sum()) for t in TAGS}
    it = {t: int(restated(t)[0]["n_iter"]) for t in TAGS}
    assert zero["sparse"] > 0 and zero["p_gt_n"] >= 30 and zero["allzero"] == 20 and zero["dense"] == 0
    assert not np.any(restated("allzero")[0]["w0"]) and not np.any(restated("allzero")[0]["w1"])
    assert it["lowdim"] == 0 and it["maxiter"] == 5 and it["tight"] > 32 and it["allzero"] > 100
    g = restated("k_gt_q")[0]
    assert g["w0"].shape[1] == 5 and not np.any(g["w0"][:, 3:]) and not np.any(g["w1"][:, 3:])
    assert np.sum(restated("rankdef_y")[1]["lam"] <= R.CUT) == 1
    assert restated("f32")[0]["x0"].dtype == np.float32 and restated("f32")[0]["gap32"].shape == (2, 3)
