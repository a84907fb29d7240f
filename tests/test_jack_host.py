"""CPU tests of ``jackknife`` and of the BCa interval: the conditions of the inputs of tests/jack_cases.py (what the bars of
tests/test_gpu_jack.py rest on), the downdated moment form the device uses against the literal refits of
tests/jack_restatement.py at 1e-10, the restatement's ``bca_interval`` against ``scipy.stats.bootstrap`` at 1e-12, the package's
``bca_intervals`` against that loop at 1e-12 (ties, an observed value outside the bootstrap values, a constant jackknife), the
summaries on a toy, every refusal (none of which reaches a device) and the exports."""

import os
import re
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

import boot_restatement as br
import jack_cases as jc
import jack_restatement as jr
import test_gpu_boot as tb
from test_boot_host import column_error, make_views, no_device  # noqa: F401  (no_device is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANCHOR = 1e-10
BCA_ANCHOR = 1e-12


# ---- the groups, the cases and the form the device uses ------------------------------------------------------------------------
def test_groups_are_interleaved_and_balanced():
    from cca_zoo_amd.model_selection import _jackknife as jk

    for n, J in [(60, 60), (60, 7), (11, 2), (4101, 33)]:
        lit, got = jr.groups(n, J), jk.groups(n, J)
        assert len(lit) == len(got) == J
        for a, b in zip(lit, got):
            np.testing.assert_array_equal(a, b)
        sizes = [len(a) for a in lit]
        assert sum(sizes) == n and max(sizes) - min(sizes) <= 1 and max(sizes) == -(-n // J)
        np.testing.assert_array_equal(np.sort(np.concatenate(lit)), np.arange(n))
    assert [len(a) for a in jr.groups(60, 7)] == [9, 9, 9, 9, 8, 8, 8]
    assert [len(a) for a in jr.groups(4101, 2)] == [2051, 2050]
    assert jc.CASES[7][0][0] == tb._rows_per_split() + 5
    for J in (2, 25, 26, 60, 4101):
        s = jc.subset(J)
        assert len(s) == min(J, jc.SUBSET) and s[0] == 0 and s[-1] == J - 1 and np.all(np.diff(s) > 0)


@pytest.mark.parametrize("shape,c,center,J", jc.CASES)
def test_cases_meet_their_conditions_and_the_downdated_form(shape, c, center, J):
    X1, X2, reps, refs, ident, k = jc.case(shape, c, center, J)
    tb.assert_conditions(ident, k)
    e_sv = e_w = 0.0
    for g, f in zip(reps, refs):
        tb.assert_conditions(f, k)
        d = jc.downdated_fit(X1, X2, int(g), J, jc.ridge(c), center, k)
        e_sv = max(e_sv, float(np.max(np.abs(d.sv - f.sv)) / f.sv[0]))
        e_w = max(e_w, column_error(d.weights, f.weights))
    print(f"jack case n={shape[0]} ({shape[1]}, {shape[2]}) c={c} center={center} J={J}: {len(reps)} replicates, worst cond "
          f"{max(max(f.cond) for f in refs):.3g}; downdated form: sigma / sigma_1 {e_sv:.3g}, weights {e_w:.3g}")
    assert e_sv <= ANCHOR and e_w <= ANCHOR


def test_replicate_equals_the_zero_one_counts_resample():
    X1, X2 = make_views(45, 4, 3, seed=8)
    for J in (45, 6):
        counts = jc.loo_counts(45, J, np.arange(J))
        for g in (0, J // 2, J - 1):
            a = jr.fit_without(X1, X2, jr.groups(45, J)[g], 0.1, True, 2)
            b = br.fit_counts(X1, X2, counts[g], 0.1, True, 2)
            np.testing.assert_array_equal(a.sv, b.sv)
            assert counts[g].sum() == 45 - len(jr.groups(45, J)[g])


def test_summaries_on_a_toy():
    from cca_zoo_amd.model_selection._jackknife import summaries

    jack = np.array([[1.0, 5.0], [2.0, 5.0], [3.0, 5.0], [6.0, 5.0]])
    for fn in (summaries, jr.summaries):
        se, bias = fn(jack, np.array([2.5, 4.0]))
        np.testing.assert_allclose(se, [np.sqrt(0.75 * 14.0), 0.0], rtol=1e-15)       # mean 3: squares 4 + 1 + 0 + 9
        np.testing.assert_allclose(bias, [1.5, 3.0], rtol=1e-15)
    X1, X2 = make_views(40, 4, 3, seed=3)
    res = jr.jackknife([X1, X2], c=0.1, k=2, J=8)
    assert res.singular_values_jack.shape == (8, 3) and [w.shape for w in res.weights_jack] == [(8, 4, 2), (8, 3, 2)]
    assert res.singular_values_se.shape == (3,) and [w.shape for w in res.weights_bias] == [(4, 2), (3, 2)]
    for j in range(2):                                    # every replicate's column points the observed column's way
        dots = sum(np.einsum("bi,i->b", wb[:, :, j], w[:, j]) for wb, w in zip(res.weights_jack, res.weights))
        assert np.all(dots >= 0)


# ---- the BCa interval ---------------------------------------------------------------------------------------------------------
def test_bca_interval_equals_scipy():
    import scipy.stats

    n, B, cl = 40, 300, 0.9
    X1, X2 = make_views(n, 3, 2, seed=6)

    def stat(idx):
        idx = np.asarray(idx, dtype=np.int64)
        return br.fit_rows(X1[idx], X2[idx], 0.1, True, 1).sv

    rng = np.random.default_rng(2)
    boot = np.stack([stat(rng.integers(0, n, size=n)) for _ in range(B)])             # (B, 2)
    theta = stat(np.arange(n))
    jack = np.stack([stat(np.delete(np.arange(n), i)) for i in range(n)])
    ref = scipy.stats.bootstrap((np.arange(n, dtype=float),), stat, n_resamples=0, method="BCa", vectorized=False, confidence_level=cl,
                                bootstrap_result=SimpleNamespace(bootstrap_distribution=boot.T))
    want = np.stack([ref.confidence_interval.low, ref.confidence_interval.high])
    got = np.array([jr.bca_interval(theta[j], boot[:, j], jack[:, j], cl)[:2] for j in range(2)]).T
    worst = float(np.max(np.abs(got - want)))
    print(f"bca_interval against scipy.stats.bootstrap: {worst:.3g}")
    assert np.all(np.isfinite(want)) and worst <= BCA_ANCHOR
    from cca_zoo_amd.model_selection import bca_intervals

    assert float(np.max(np.abs(bca_intervals(theta, boot, jack, cl)[0] - want))) <= BCA_ANCHOR


def bca_arrays():
    """Random (B,) + (3, 4) and (J,) + (3, 4) arrays with ties, an observed value outside the range and a constant jackknife."""
    rng = np.random.default_rng(11)
    B, J, S = 200, 25, (3, 4)
    boot = rng.standard_normal((B,) + S) * rng.uniform(0.5, 2.0, S) + rng.standard_normal(S)
    jack = np.median(boot, axis=0) + 0.05 * rng.standard_normal((J,) + S) ** 3
    theta = np.quantile(boot, 0.4, axis=0)
    boot[:, 0, 1] = np.round(boot[:, 0, 1])               # ties, some of them with the observed value
    theta[0, 1] = 0.0
    theta[1, 2] = boot[:, 1, 2].max() + 1.0               # outside: z0 = +inf
    theta[2, 0] = boot[:, 2, 0].min() - 1.0               # outside: z0 = -inf
    jack[:, 2, 3] = 0.25                                  # constant: sum d^2 = 0
    theta[1, 1] = boot[:, 1, 1].max()                     # on the edge, not outside: finite
    return theta, boot, jack


@pytest.mark.parametrize("cl", [0.95, 0.5])
def test_bca_intervals_equal_the_loop(cl):
    from cca_zoo_amd.model_selection import bca_intervals

    theta, boot, jack = bca_arrays()
    want_ci, want_z0, want_a = jr.bca_all(theta, boot, jack, cl)
    with pytest.warns(RuntimeWarning, match="3 of 12 intervals are NaN") as rec:
        ci, z0, a = bca_intervals(theta, boot, jack, cl)
    assert len(rec) == 1
    assert ci.shape == (2, 3, 4) and z0.shape == a.shape == (3, 4)
    nan = np.zeros((3, 4), dtype=bool)
    nan[1, 2] = nan[2, 0] = nan[2, 3] = True
    np.testing.assert_array_equal(np.isnan(ci[0]), nan), np.testing.assert_array_equal(np.isnan(ci[1]), nan)
    np.testing.assert_array_equal(np.isnan(want_ci[0]), nan), np.testing.assert_array_equal(np.isnan(want_ci[1]), nan)
    assert z0[1, 2] == np.inf and z0[2, 0] == -np.inf and np.isnan(a[2, 3]) and np.isfinite(z0[1, 1])
    ok = ~nan
    worst = max(float(np.max(np.abs(ci[:, ok] - want_ci[:, ok]))), float(np.max(np.abs(z0[ok] - want_z0[ok]))),
                float(np.max(np.abs(a[ok] - want_a[ok]))))
    print(f"bca_intervals against the loop at {cl}: {worst:.3g}")
    assert worst <= BCA_ANCHOR
    assert np.all(ci[0, ok] <= ci[1, ok])
    with warnings.catch_warnings():                       # nothing degenerate: no warning; a scalar statistic works
        warnings.simplefilter("error")
        one = bca_intervals(theta[0, 0], boot[:, 0, 0], jack[:, 0, 0], cl)
    assert one[0].shape == (2,) and one[1].shape == ()
    assert np.max(np.abs(one[0] - ci[:, 0, 0])) <= BCA_ANCHOR   # (a strided mean may differ from a contiguous one in its last bit)
    with pytest.raises(ValueError, match=r"\(B,\) \+ S"):
        bca_intervals(theta, boot[:, :2], jack, cl)


# ---- limits, refusals, surface ---------------------------------------------------------------------------------------------
def test_import_surface():
    import dataclasses

    import cca_zoo_amd.model_selection as ms
    from cca_zoo_amd import _backend
    from cca_zoo_amd.model_selection import BCaBootstrapResult, BootstrapResult, JackknifeResult, bootstrap, jackknife
    from cca_zoo_amd.model_selection import _jackknife as jk

    assert {"jackknife", "JackknifeResult", "bca_intervals", "BCaBootstrapResult", "bootstrap", "BootstrapResult"} <= set(ms.__all__)
    assert [f.name for f in dataclasses.fields(JackknifeResult)] == [
        "singular_values", "weights", "singular_values_jack", "weights_jack", "singular_values_se", "weights_se",
        "singular_values_bias", "weights_bias", "n_groups", "estimator"]
    assert issubclass(BCaBootstrapResult, BootstrapResult)
    inherited = [f.name for f in dataclasses.fields(BootstrapResult)]
    own = [f.name for f in dataclasses.fields(BCaBootstrapResult)]
    assert own[:len(inherited)] == inherited              # the inherited field order is intact
    assert own[len(inherited):] == ["singular_values_ci_percentile", "weights_ci_percentile", "singular_values_jack", "weights_jack",
                                    "singular_values_z0", "weights_z0", "singular_values_acceleration", "weights_acceleration", "n_groups"]
    assert jk.DEFAULT_GROUPS == 4096
    doc = jackknife.__doc__
    assert "4096" in doc and "leave-one-out" in doc and "differ by one" in doc and "LinAlgError" in doc and "not a measured optimum" in doc
    assert "BCa" in bootstrap.__doc__ and "jackknife_groups" in bootstrap.__doc__
    assert "scipy.stats.bootstrap" in ms.bca_intervals.__doc__ and "RuntimeWarning" in ms.bca_intervals.__doc__
    res, args = _backend.SIGNATURES["ccz_jack_rcca"]
    assert len(args) == 16
    header = open(os.path.join(ROOT, "include", "ccz.h")).read()
    decl = re.search(r"CCZ_API int ccz_jack_rcca\(([^;]*)\);", header).group(1)
    assert len(decl.split(",")) == 16 and "int64_t ngroups, int64_t g0, int64_t ng" in " ".join(decl.split())
    assert "0/1 counts" in header


def test_limits_raise_value_errors(no_device):
    from cca_zoo_amd.linear import CCA, MCCA
    from cca_zoo_amd.model_selection import jackknife

    X = [np.zeros((20, 3)), np.zeros((20, 4))]
    for bad in (2.5, True, "4", 4.0):
        with pytest.raises(ValueError, match="n_groups must be None or an integer"):
            jackknife(CCA(), X, n_groups=bad)
    for bad in (1, 0, -3):
        with pytest.raises(ValueError, match="n_groups must be None or an integer >= 2"):
            jackknife(CCA(), X, n_groups=bad)
    with pytest.raises(ValueError, match="must not exceed the number of samples"):
        jackknife(CCA(), X, n_groups=21)
    with pytest.raises(ValueError, match="fewer than 2"):
        jackknife(CCA(), [np.zeros((3, 1)), np.zeros((3, 1))], n_groups=2)      # 3 - ceil(3 / 2) = 1
    with pytest.raises(ValueError, match="fewer than 2"):
        jackknife(CCA(), [np.zeros((2, 1)), np.zeros((2, 1))])                  # leave-one-out of two rows
    with pytest.raises(ValueError, match="at most 64 columns.*principal components"):
        jackknife(CCA(), [np.zeros((20, 65)), np.zeros((20, 4))])
    with pytest.raises(ValueError, match="at least 2 samples"):
        jackknife(CCA(), [np.zeros((1, 3)), np.zeros((1, 4))])
    with pytest.raises(ValueError, match="exactly 2 views"):
        jackknife(CCA(), X + [np.zeros((20, 2))])
    with pytest.raises(TypeError, match="CCA, rCCA or PLS"):
        jackknife(MCCA(), X)
    with pytest.raises(TypeError, match="half-precision"):
        jackknife(CCA(), [X[0].astype(np.float16), X[1]])
    with pytest.raises(TypeError, match="list of two"):
        jackknife(CCA(), X[0])
    est = CCA(latent_dimensions=2)
    with pytest.raises(ValueError):
        jackknife(est, X, n_groups=40)
    assert not hasattr(est, "weights_")


def test_row_sharded_is_refused(monkeypatch, no_device):
    from cca_zoo_amd import _dist
    from cca_zoo_amd.linear import PLS
    from cca_zoo_amd.model_selection import jackknife

    monkeypatch.setattr(_dist, "is_sharded", lambda: True)
    with pytest.raises(NotImplementedError, match="row_sharded"):
        jackknife(PLS(), [np.zeros((20, 3)), np.zeros((20, 4))])


def test_bootstrap_method_refusals(no_device):
    from cca_zoo_amd.linear import CCA
    from cca_zoo_amd.model_selection import bootstrap

    X = [np.zeros((20, 3)), np.zeros((20, 4))]
    for bad in ("bca", "basic", None, 1):
        with pytest.raises(ValueError, match="method must be one of"):
            bootstrap(CCA(), X, method=bad)
    with pytest.raises(ValueError, match="jackknife_groups needs method='BCa'"):
        bootstrap(CCA(), X, jackknife_groups=10)
    with pytest.raises(ValueError, match="jackknife_groups needs method='BCa'"):
        bootstrap(CCA(), X, method="percentile", jackknife_groups=10)
    for bad in (1, 2.5, True):
        with pytest.raises(ValueError, match="jackknife_groups must be None or an integer >= 2"):
            bootstrap(CCA(), X, method="BCa", jackknife_groups=bad)
    with pytest.raises(ValueError, match="jackknife_groups must not exceed"):
        bootstrap(CCA(), X, method="BCa", jackknife_groups=21)
    with pytest.raises(ValueError, match="n_resamples"):
        bootstrap(CCA(), X, method="BCa", n_resamples=1)


def test_percentile_method_never_calls_the_jackknife(monkeypatch):
    """``method="percentile"`` on a stand-in handle: the bootstrap's own device calls are recorded, the jackknife's raise."""
    from cca_zoo_amd import _backend
    from cca_zoo_amd.linear import rCCA
    from cca_zoo_amd.model_selection import BCaBootstrapResult, BootstrapResult, _bootstrap as bs, _jackknife as jk

    def forbidden(*a, **k):
        raise AssertionError("the jackknife ran")

    for name in ("run_replicates", "jack_rcca", "jackknife", "bca_intervals", "resolve_groups", "check_groups_type"):
        monkeypatch.setattr(jk, name, forbidden)
    n, p, B, k = 30, (4, 3), 5, 2
    rng = np.random.default_rng(0)
    X = [rng.standard_normal((n, d)) for d in p]
    calls = []

    class Buf:
        def __init__(self, nbytes):
            self.ptr, self.nbytes = 4096, nbytes

    class Handle:
        lib = raw = None

        def alloc(self, nbytes):
            return Buf(nbytes)

        def to_host(self, buf, shape, dtype=np.float64):
            if dtype == np.int32:
                return np.zeros(shape, dtype=np.int32)
            out = np.random.default_rng(int(np.prod(shape))).standard_normal(shape)
            return -np.sort(-np.abs(out), axis=1) if len(shape) == 2 else out

        def h2d(self, ptr, array):
            pass

    monkeypatch.setattr(_backend, "handle_for", lambda views: Handle())
    monkeypatch.setattr(bs._resample, "stage_f64", lambda h, views, on_device: ([], [4096, 4096]))
    monkeypatch.setattr(bs, "acquire", lambda h, views: None)
    monkeypatch.setattr(bs, "release", lambda h, sp: None)
    monkeypatch.setattr(bs, "_shifted", lambda h, xptr, n, d, center: None)
    monkeypatch.setattr(bs, "boot_rcca", lambda *a: calls.append(a[7]))
    monkeypatch.setattr(rCCA, "fit", lambda self, views: self)
    res = bs.bootstrap(rCCA(latent_dimensions=k, c=0.1), X, n_resamples=B, random_state=0)
    assert type(res) is BootstrapResult and not isinstance(res, BCaBootstrapResult)
    assert calls == [1, B] and res.singular_values_boot.shape == (B, 3)
    with pytest.raises(AssertionError, match="the jackknife ran"):
        bs.bootstrap(rCCA(latent_dimensions=k, c=0.1), X, n_resamples=B, random_state=0, method="BCa")
