"""CPU tests of ``bootstrap``: the float64 NumPy restatement (tests/boot_restatement.py, the comparator of
tests/test_gpu_boot.py) anchored at 1e-10 on goldens from the real reference (tests/golden/boot_rcca.npz, written by
tools/gen_golden_boot.py), on the multiplicity-weighted moment form the device uses and on a symmetric inverse-square-root
whitening route; the sign rules and summaries on hand-made arrays, the draw rule, the chunk producer, every refusal (none of
which reaches a device) and the exports."""

import os
import re

import numpy as np
import pytest

import boot_restatement as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANCHOR = 1e-10


def make_views(n, p1, p2, seed, shared=2, noise=1.0):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, shared))
    X1 = z @ rng.standard_normal((shared, p1)) + noise * rng.standard_normal((n, p1)) + rng.standard_normal(p1)
    X2 = z @ rng.standard_normal((shared, p2)) + noise * rng.standard_normal((n, p2)) + rng.standard_normal(p2)
    return X1, X2


def column_error(got, ref):
    """Worst error of the weight columns up to the coupled sign, per view relative to the reference column's largest entry."""
    worst = 0.0
    for j in range(ref[0].shape[1]):
        sign = 1.0 if sum(float(g[:, j] @ w[:, j]) for g, w in zip(got, ref)) >= 0 else -1.0
        for g, w in zip(got, ref):
            worst = max(worst, float(np.max(np.abs(sign * g[:, j] - w[:, j])) / np.max(np.abs(w[:, j]))))
    return worst


def inv_sqrt(R):
    w, V = np.linalg.eigh(R)
    return (V / np.sqrt(w)) @ V.T


def weighted_moment_form(X1, X2, m, c, center, k):
    """The device's route in NumPy: weighted sums over the rows in their stored order, no row is gathered."""
    c1, c2 = br.per_view(c)
    p1 = X1.shape[1]
    X = np.hstack([X1, X2])
    w = np.asarray(m, dtype=np.float64)
    N = float(np.sum(m))
    G, s = (X * w[:, None]).T @ X, w @ X
    Cm = (G - np.outer(s, s) / N if center else G) / (N - 1)
    R1 = (1 - c1) * Cm[:p1, :p1] + c1 * np.eye(p1)
    R2 = (1 - c2) * Cm[p1:, p1:] + c2 * np.eye(X2.shape[1])
    L1, L2 = np.linalg.cholesky(R1), np.linalg.cholesky(R2)
    T = np.linalg.solve(L1, Cm[:p1, p1:]) @ np.linalg.inv(L2).T
    U, S, Vt = np.linalg.svd(T, full_matrices=False)
    return S, [np.linalg.solve(L1.T, U[:, :k]), np.linalg.solve(L2.T, Vt[:k].T)]


def symmetric_whitening_form(X1, X2, rows, c, center, k):
    c1, c2 = br.per_view(c)
    A, B = X1[rows], X2[rows]
    N = len(rows)
    if center:
        A, B = A - A.mean(axis=0), B - B.mean(axis=0)
    H1 = inv_sqrt((1 - c1) * (A.T @ A) / (N - 1) + c1 * np.eye(A.shape[1]))
    H2 = inv_sqrt((1 - c2) * (B.T @ B) / (N - 1) + c2 * np.eye(B.shape[1]))
    U, S, Vt = np.linalg.svd(H1 @ (A.T @ B / (N - 1)) @ H2, full_matrices=False)
    return S, [H1 @ U[:, :k], H2 @ Vt[:k].T]


CONFIGS = [
    pytest.param(0.0, True, (6, 6), id="cca"),
    pytest.param(0.0, False, (5, 4), id="cca-uncentred"),
    pytest.param(1.0, True, (6, 4), id="pls"),
    pytest.param([0.1, 0.3], True, (5, 7), id="per-view-c"),
    pytest.param(0.2, False, (4, 6), id="uncentred"),
    pytest.param(1.0, False, (3, 9), id="pls-uncentred"),
]


# ---- anchors of the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,c", [("cca", 0.0), ("rcca", [0.1, 0.3]), ("pls", 1.0)])
def test_restatement_equals_the_reference_refits(name, c):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "boot_rcca.npz"))
    X1, X2, idx = gold["X1"], gold["X2"], gold["idx"]
    assert X1.shape == (60, 5) and X2.shape == (60, 3) and idx.shape == (8, 60)
    worst = 0.0
    for b, ix in enumerate(idx):
        fit = br.fit_rows(X1[ix], X2[ix], c, True, 3)
        worst = max(worst, column_error(fit.weights, [gold[f"{name}/w0"][b], gold[f"{name}/w1"][b]]))
        counted = br.fit_counts(X1, X2, np.bincount(ix, minlength=60), c, True, 3)
        worst = max(worst, column_error(counted.weights, [gold[f"{name}/w0"][b], gold[f"{name}/w1"][b]]))
        if name == "cca":                                 # the reference's per-dimension score of a CCA fit is the correlation
            worst = max(worst, float(np.max(np.abs(fit.sv - gold["cca/score"][b]))))
    print(f"restatement against the reference's {name}: {worst:.3g}")
    assert worst <= ANCHOR


@pytest.mark.parametrize("c,center,p", CONFIGS)
def test_restatement_equals_the_weighted_moment_form(c, center, p):
    X1, X2 = make_views(90, p[0], p[1], seed=1)
    k = min(p)
    rng = np.random.default_rng(4)
    for _ in range(4):
        m = np.bincount(rng.integers(0, 90, size=90), minlength=90)
        ref = br.fit_counts(X1, X2, m, c, center, k)
        S, W = weighted_moment_form(X1 - X1.mean(axis=0) if center else X1, X2 - X2.mean(axis=0) if center else X2, m, c, center, k)
        assert np.max(np.abs(S - ref.sv)) / ref.sv[0] <= ANCHOR
        assert column_error(W, ref.weights) <= ANCHOR
    half = (rng.random(90) < 0.5).astype(np.int64)       # 0/1 multiplicities: a subsample, N_b != n
    ref = br.fit_counts(X1, X2, half, c, center, k)
    S, W = weighted_moment_form(X1, X2, half, c, center, k)
    assert np.max(np.abs(S - ref.sv)) / ref.sv[0] <= ANCHOR and column_error(W, ref.weights) <= ANCHOR


@pytest.mark.parametrize("c,center,p", CONFIGS)
def test_restatement_equals_symmetric_whitening(c, center, p):
    X1, X2 = make_views(90, p[0], p[1], seed=2)
    k = min(p)
    res = br.restate([X1, X2], c=c, center=center, k=k, n_resamples=4, random_state=5)
    rng = np.random.default_rng(5)
    for b in range(4):
        ix = rng.integers(0, 90, size=90)
        np.testing.assert_array_equal(ix, res.idx[b])
        S, W = symmetric_whitening_form(X1, X2, ix, c, center, k)
        assert np.max(np.abs(S - res.singular_values_boot[b])) / S[0] <= ANCHOR
        assert column_error([w[b] for w in res.weights_boot], W) <= ANCHOR
    S, W = symmetric_whitening_form(X1, X2, np.arange(90), c, center, k)
    assert np.max(np.abs(S - res.singular_values)) / S[0] <= ANCHOR and column_error(res.weights, W) <= ANCHOR
    if c == 0.0 and center:
        assert np.all(res.singular_values < 1.0)           # canonical correlations


def test_restatement_shapes_and_summaries():
    X1, X2 = make_views(50, 4, 3, seed=3)
    res = br.restate([X1, X2], c=0.1, k=2, n_resamples=6, confidence_level=0.8, random_state=1)
    assert res.singular_values.shape == (3,) and res.singular_values_boot.shape == (6, 3)
    assert res.singular_values_se.shape == (3,) and res.singular_values_ci.shape == (2, 3)
    assert [w.shape for w in res.weights] == [(4, 2), (3, 2)] and [w.shape for w in res.weights_boot] == [(6, 4, 2), (6, 3, 2)]
    assert [w.shape for w in res.weights_se] == [(4, 2), (3, 2)] and [w.shape for w in res.weights_ci] == [(2, 4, 2), (2, 3, 2)]
    np.testing.assert_array_equal(res.singular_values_se, np.std(res.singular_values_boot, axis=0, ddof=1))
    np.testing.assert_array_equal(res.weights_ci[1], np.quantile(res.weights_boot[1], [(1 - 0.8) / 2, (1 + 0.8) / 2], axis=0))
    np.testing.assert_array_equal(res.bootstrap_ratio[0], res.weights[0] / res.weights_se[0])
    for j in range(2):                                    # every resampled column points the observed column's way
        dots = sum(np.einsum("bi,i->b", wb[:, :, j], w[:, j]) for wb, w in zip(res.weights_boot, res.weights))
        assert np.all(dots >= 0)


# ---- sign rules and summaries on hand-made arrays --------------------------------------------------------------------------
def test_observed_sign_rule():
    from cca_zoo_amd.model_selection._bootstrap import orient_observed

    W1 = np.array([[0.5, -2.0, 1.0], [-3.0, 1.0, -1.0]])
    W2 = np.array([[1.0, 1.5, -1.0]])
    want1 = np.array([[-0.5, 2.0, 1.0], [3.0, -1.0, -1.0]])   # column 0: -3 leads, flip; 1: -2 leads, flip; 2: the tie goes to the first (+1)
    want2 = np.array([[-1.0, -1.5, -1.0]])
    got = orient_observed(np.vstack([W1, W2]))
    np.testing.assert_array_equal(got, np.vstack([want1, want2]))
    r1, r2 = br.orient_observed(W1, W2)
    np.testing.assert_array_equal(r1, want1), np.testing.assert_array_equal(r2, want2)
    lead_in_view2 = orient_observed(np.array([[1.0], [0.5], [-4.0]]))
    np.testing.assert_array_equal(lead_in_view2, [[-1.0], [-0.5], [4.0]])   # the two views of a column flip together


def test_resampled_sign_rule():
    from cca_zoo_amd.model_selection._bootstrap import orient_to

    obs = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, -1.0]])                  # stacked (2 + 1) x 2
    boot = np.array([[[-1.0, 0.0], [0.0, 2.0], [-0.5, 1.0]],               # column 0: dot -1.5 -> flip; column 1: dot 1 -> keep
                     [[2.0, 1.0], [0.0, -1.0], [-2.0, 0.0]]])              # column 0: dot 0 -> keep;    column 1: dot -1 -> flip
    want = np.array([[[1.0, 0.0], [-0.0, 2.0], [0.5, 1.0]], [[2.0, -1.0], [0.0, 1.0], [-2.0, -0.0]]])
    np.testing.assert_array_equal(orient_to(boot, obs), want)
    for b in range(2):
        r1, r2 = br.orient_to(boot[b, :2], boot[b, 2:], obs[:2], obs[2:])
        np.testing.assert_array_equal(np.vstack([r1, r2]), want[b])


def test_summaries_on_a_toy():
    from cca_zoo_amd.model_selection._bootstrap import summaries

    boot = np.array([[1.0, 10.0], [2.0, 10.0], [3.0, 10.0], [4.0, 10.0], [5.0, 40.0]])
    for fn in (summaries, br.summaries):
        se, ci = fn(boot, 0.5)
        np.testing.assert_allclose(se, [np.sqrt(2.5), np.sqrt(180.0)], rtol=1e-15)
        np.testing.assert_array_equal(ci, [[2.0, 10.0], [4.0, 10.0]])      # the 25 % and 75 % quantiles
    se, ci = summaries(np.stack([boot, 2 * boot]).transpose(1, 0, 2), 0.5)
    assert se.shape == (2, 2) and ci.shape == (2, 2, 2)
    np.testing.assert_array_equal(ci[:, 1, :], [[4.0, 20.0], [8.0, 20.0]])


# ---- the draw rule and the chunk producer ----------------------------------------------------------------------------------
def test_draw_rule_is_the_integers_stream():
    from cca_zoo_amd.model_selection._bootstrap import draw_counts

    n, B = 41, 9
    got = draw_counts(np.random.default_rng(9), n, B)
    assert got.dtype == np.int32 and got.shape == (B, n) and got.flags.c_contiguous
    np.testing.assert_array_equal(got.sum(axis=1), np.full(B, n))
    rng = np.random.default_rng(9)
    np.testing.assert_array_equal(got, np.stack([np.bincount(rng.integers(0, n, size=n), minlength=n) for _ in range(B)]))
    np.testing.assert_array_equal(got, np.stack([np.bincount(ix, minlength=n) for ix in br.draw_indices(9, n, B)]))


@pytest.mark.parametrize("chunk", [1, 7, 23])
def test_chunk_producer_is_the_same_stream(chunk):
    from cca_zoo_amd.model_selection._bootstrap import count_chunks, draw_counts

    n, B = 41, 23
    got = list(count_chunks(np.random.default_rng(9), n, B, chunk))
    assert [g.shape[0] for g in got] == [chunk] * (B // chunk) + ([B % chunk] if B % chunk else [])
    assert all(g.dtype == np.int32 and g.flags.c_contiguous for g in got)
    np.testing.assert_array_equal(np.concatenate(got), draw_counts(np.random.default_rng(9), n, B))


def test_chunk_length_and_constants_match_the_header(monkeypatch):
    from cca_zoo_amd.model_selection import _bootstrap as bs

    header = open(os.path.join(ROOT, "include", "ccz.h")).read()
    assert int(re.search(r"#define CCZ_PERM_ROWS (\d+)", header).group(1)) == bs.ROWS_PER_SPLIT
    assert int(re.search(r"#define CCZ_PERM_MAXP (\d+)", header).group(1)) == bs.MAX_WIDTH
    codes = {name: int(v) for name, v in re.findall(r"#define CCZ_BOOT_INFO_(\w+) (\d+)", header)}
    assert codes == {"R1": 1, "R2": 2, "N": 3, "JACOBI": 4} and set(bs.INFO_CAUSES) == set(codes.values())
    assert "c > 0" in bs.INFO_CAUSES[1] and "c > 0" in bs.INFO_CAUSES[2]
    assert bs.chunk_length(100) == bs.CHUNK_RESAMPLES and bs.chunk_length(2 ** 30) == 1
    monkeypatch.setattr(bs, "CHUNK_RESAMPLES", 7)
    assert bs.chunk_length(100) == 7


def test_info_becomes_a_linalg_error():
    from cca_zoo_amd.model_selection._bootstrap import raise_for_info

    raise_for_info(np.zeros(5, dtype=np.int32))
    with pytest.raises(np.linalg.LinAlgError, match=r"resample 2: R_2 .*c > 0"):
        raise_for_info(np.array([0, 0, 0, 2, 1], dtype=np.int32))
    with pytest.raises(np.linalg.LinAlgError, match=r"the observed sample: R_1 .*c > 0"):
        raise_for_info(np.array([1, 0], dtype=np.int32))
    with pytest.raises(np.linalg.LinAlgError, match="resample 0: .*fewer than 2 rows"):
        raise_for_info(np.array([0, 3], dtype=np.int32))
    with pytest.raises(np.linalg.LinAlgError, match="resample 1: .*did not settle"):
        raise_for_info(np.array([0, 0, 4], dtype=np.int32))


# ---- refusals: all before the device is touched ---------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    from cca_zoo_amd import _backend

    def touched(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_backend, "handle_for", touched)
    monkeypatch.setattr(_backend, "default_handle", touched)


def _device_like(n, d, dtype):
    import torch

    class OnDevice(torch.Tensor):
        @property
        def is_cuda(self):
            return True

    OnDevice.__module__ = "torch._stand_in"
    return torch.zeros((n, d), dtype=dtype).as_subclass(OnDevice)


def test_import_surface():
    import cca_zoo_amd.model_selection as ms
    from cca_zoo_amd.model_selection import BootstrapResult, bootstrap

    assert {"GridSearchCV", "permutation_test", "PermutationTestResult", "bootstrap", "BootstrapResult"} <= set(ms.__all__)
    assert callable(bootstrap)
    assert list(BootstrapResult.__dataclass_fields__) == ["singular_values", "singular_values_boot", "singular_values_se",
                                                          "singular_values_ci", "weights", "weights_boot", "weights_se", "weights_ci",
                                                          "bootstrap_ratio", "estimator"]
    doc = bootstrap.__doc__
    assert "64" in doc and "principal components" in doc and "LinAlgError" in doc


def test_estimator_type_is_checked(no_device):
    from cca_zoo_amd.linear import MCCA, PLS_ALS
    from cca_zoo_amd.model_selection import bootstrap

    X = [np.zeros((20, 3)), np.zeros((20, 4))]
    for bad in (MCCA(), PLS_ALS(), object(), None):
        with pytest.raises(TypeError, match="CCA, rCCA or PLS"):
            bootstrap(bad, X)


def test_unsupported_views_raise_type_errors(no_device):
    import scipy.sparse
    import torch

    from cca_zoo_amd.linear import CCA, rCCA
    from cca_zoo_amd.model_selection import bootstrap

    dense = np.zeros((20, 3))
    with pytest.raises(TypeError, match="sparse"):
        bootstrap(CCA(), [scipy.sparse.csr_matrix(np.eye(20, 4)), dense])
    with pytest.raises(TypeError, match="half-precision"):
        bootstrap(CCA(), [dense.astype(np.float16), dense])
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match="half-precision"):
            bootstrap(rCCA(c=0.1), [_device_like(20, 3, dt), _device_like(20, 4, dt)])
        with pytest.raises(TypeError, match="half-precision"):
            bootstrap(rCCA(c=0.1), [torch.zeros((20, 3), dtype=dt), dense])
    with pytest.raises(TypeError, match="list of two"):
        bootstrap(CCA(), dense)


def test_row_sharded_is_refused(monkeypatch, no_device):
    from cca_zoo_amd import _dist
    from cca_zoo_amd.linear import PLS
    from cca_zoo_amd.model_selection import bootstrap

    monkeypatch.setattr(_dist, "is_sharded", lambda: True)
    with pytest.raises(NotImplementedError, match="row_sharded"):
        bootstrap(PLS(), [np.zeros((20, 3)), np.zeros((20, 4))])


def test_limits_raise_value_errors(monkeypatch, no_device):
    from cca_zoo_amd.linear import CCA, rCCA
    from cca_zoo_amd.model_selection import _resample
    from cca_zoo_amd.model_selection import bootstrap

    X = [np.zeros((20, 3)), np.zeros((20, 4))]
    with pytest.raises(ValueError, match="at most 64 columns.*principal components"):
        bootstrap(CCA(), [np.zeros((20, 65)), np.zeros((20, 4))])
    with pytest.raises(ValueError, match="at most 64 columns"):
        bootstrap(CCA(), [np.zeros((20, 4)), np.zeros((20, 200))])
    for bad in (0, 1, -3, 2.5, True, None):
        with pytest.raises(ValueError, match="n_resamples"):
            bootstrap(CCA(), X, n_resamples=bad)
    for bad in (0.0, 1.0, -0.5, 95, True, None, "0.9"):
        with pytest.raises(ValueError, match="confidence_level"):
            bootstrap(CCA(), X, confidence_level=bad)
    with pytest.raises(ValueError, match="at least 2 samples"):
        bootstrap(CCA(), [np.zeros((1, 3)), np.zeros((1, 4))])
    with pytest.raises(ValueError, match="exactly 2 views"):
        bootstrap(CCA(), X + [np.zeros((20, 2))])
    with pytest.raises(ValueError, match="At least 2 views"):
        bootstrap(CCA(), X[:1])
    with pytest.raises(ValueError, match="same number of samples"):
        bootstrap(CCA(), [np.zeros((20, 3)), np.zeros((19, 4))])
    with pytest.raises(ValueError):
        bootstrap(rCCA(c=1.5), X)
    with pytest.raises(ValueError, match="length 2"):
        bootstrap(rCCA(c=[0.1, 0.2, 0.3]), X)
    with pytest.raises(ValueError, match="all host arrays or all CUDA tensors"):
        import torch

        bootstrap(CCA(), [_device_like(20, 3, torch.float32), np.zeros((20, 4))])

    class Tall:                                             # 2^31 rows without the memory
        dtype = np.dtype(np.float64)

        def __init__(self, d):
            self.shape = (2 ** 31, d)

    monkeypatch.setattr(_resample, "validate_views", lambda views, **kw: list(views))
    with pytest.raises(ValueError, match="2\\^31"):
        bootstrap(CCA(), [Tall(3), Tall(4)])


def test_the_estimator_passed_in_is_not_fitted_by_a_refused_call(no_device):
    from cca_zoo_amd.linear import CCA
    from cca_zoo_amd.model_selection import bootstrap

    est = CCA(latent_dimensions=2)
    with pytest.raises(ValueError):
        bootstrap(est, [np.zeros((20, 65)), np.zeros((20, 4))])
    assert not hasattr(est, "weights_")
