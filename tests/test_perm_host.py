"""CPU tests of ``permutation_test``: the float64 NumPy restatement (tests/perm_restatement.py, the comparator of
tests/test_gpu_perm.py) anchored on the closed form and on brute-force refits, the counting rule, the tails, every refusal
(none of which reaches a device) and the chunked index producer."""

import os
import re

import numpy as np
import pytest
import scipy.linalg

import perm_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_views(n, p1, p2, seed, shared=2, noise=1.0):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, shared))
    X1 = z @ rng.standard_normal((shared, p1)) + noise * rng.standard_normal((n, p1)) + rng.standard_normal(p1)
    X2 = z @ rng.standard_normal((shared, p2)) + noise * rng.standard_normal((n, p2)) + rng.standard_normal(p2)
    return X1, X2


def inv_sqrt(R):
    w, V = np.linalg.eigh(R)
    return (V / np.sqrt(w)) @ V.T


def closed_form(X1, X2, c, center):
    """Singular values of ``R_1^-1/2 C_12 R_2^-1/2`` (symmetric whitening: another route than the Cholesky factors), from scratch."""
    n = X1.shape[0]
    c1, c2 = pr.per_view(c)
    A = X1 - X1.mean(axis=0) if center else X1
    Bm = X2 - X2.mean(axis=0) if center else X2
    R1 = (1 - c1) * (A.T @ A) / (n - 1) + c1 * np.eye(A.shape[1])
    R2 = (1 - c2) * (Bm.T @ Bm) / (n - 1) + c2 * np.eye(Bm.shape[1])
    return scipy.linalg.svd(inv_sqrt(R1) @ (A.T @ Bm / (n - 1)) @ inv_sqrt(R2), compute_uv=False)


CONFIGS = [
    pytest.param(0.0, True, (6, 6), id="cca"),
    pytest.param(1.0, True, (6, 4), id="pls"),
    pytest.param([0.1, 0.3], True, (5, 7), id="per-view-c"),
    pytest.param(0.2, False, (4, 6), id="uncentred"),
    pytest.param(0.0, True, (3, 9), id="p1-ne-p2"),
]


@pytest.mark.parametrize("c,center,p", CONFIGS)
def test_identity_equals_closed_form(c, center, p):
    X1, X2 = make_views(90, p[0], p[1], seed=1)
    res = pr.restate([X1, X2], c=c, center=center, n_permutations=1, random_state=0)
    ref = closed_form(X1, X2, c, center)
    assert res.statistic.shape == (min(p),)
    assert np.all(np.diff(res.statistic) <= 0)
    assert np.max(np.abs(res.statistic - ref)) < 1e-12
    if c == 0.0:
        assert np.all(res.statistic < 1.0)               # canonical correlations


@pytest.mark.parametrize("c,center,p", CONFIGS)
def test_permuted_row_equals_brute_force_refit(c, center, p):
    """The invariance the design rests on: means and covariances of [X1, X2[pi]] recomputed from scratch change nothing."""
    X1, X2 = make_views(90, p[0], p[1], seed=2)
    res = pr.restate([X1, X2], c=c, center=center, n_permutations=4, random_state=5)
    rng = np.random.default_rng(5)
    for b in range(4):
        pi = rng.permutation(90)
        np.testing.assert_array_equal(pi, res.perms[b])
        assert np.max(np.abs(res.null[b] - closed_form(X1, X2[pi], c, center))) < 1e-12


def test_counting_rule_on_a_toy():
    from cca_zoo_amd.model_selection._permutation import count_pvalues

    statistic = np.array([0.5, 0.2])
    null = np.array([[0.6, 0.1], [0.5, 0.3], [0.4, 0.19]])
    for fn in (count_pvalues, pr.count_pvalues):
        np.testing.assert_array_equal(fn(statistic, null), [3 / 4, 2 / 4])       # ties count against the observed value
    np.testing.assert_array_equal(count_pvalues(np.array([2.0]), np.array([[1.0], [1.5], [0.5]])), [1 / 4])


def test_tails():
    from cca_zoo_amd.model_selection._permutation import tails

    s = np.array([0.9, 0.5, 0.1])
    want = np.cumsum((s ** 2)[::-1])[::-1]
    np.testing.assert_array_equal(tails(s), want)
    np.testing.assert_array_equal(pr.tails(s), want)
    batch = np.stack([s, 2 * s])
    np.testing.assert_array_equal(tails(batch), np.stack([want, 4 * want]))
    assert tails(s)[0] == pytest.approx(np.sum(s ** 2))


def test_restatement_pvalues_and_tails_are_consistent():
    X1, X2 = make_views(60, 4, 3, seed=3)
    res = pr.restate([X1, X2], c=0.0, n_permutations=3, random_state=1)
    for j in range(3):
        assert res.pvalues[j] == (1 + int(np.sum(res.null[:, j] >= res.statistic[j]))) / 4
        assert res.tail_pvalues[j] == (1 + int(np.sum(res.tail_null[:, j] >= res.tail[j]))) / 4
    np.testing.assert_allclose(res.tail, np.cumsum((res.statistic ** 2)[::-1])[::-1], rtol=0, atol=0)


# ---- the index producer ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 7, 23])
def test_index_producer_is_the_rng_sequence(chunk):
    from cca_zoo_amd.model_selection._permutation import permutation_chunks

    n, B = 41, 23
    got = list(permutation_chunks(np.random.default_rng(9), n, B, chunk))
    assert [g.shape[0] for g in got] == [chunk] * (B // chunk) + ([B % chunk] if B % chunk else [])
    assert all(g.dtype == np.int32 and g.flags.c_contiguous for g in got)
    rng = np.random.default_rng(9)
    np.testing.assert_array_equal(np.concatenate(got), np.stack([rng.permutation(n) for _ in range(B)]))


def test_constants_match_the_header():
    from cca_zoo_amd.model_selection import _permutation as pm

    header = open(os.path.join(ROOT, "include", "ccz.h")).read()
    assert int(re.search(r"#define CCZ_PERM_ROWS (\d+)", header).group(1)) == pm.ROWS_PER_SPLIT
    assert int(re.search(r"#define CCZ_PERM_MAXP (\d+)", header).group(1)) == pm.MAX_WIDTH
    assert isinstance(pm.CHUNK_PERMS, int) and pm.CHUNK_PERMS >= 1


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
    from cca_zoo_amd.model_selection import PermutationTestResult, permutation_test

    assert {"GridSearchCV", "permutation_test", "PermutationTestResult"} <= set(ms.__all__)
    assert callable(permutation_test) and PermutationTestResult.__dataclass_fields__.keys() >= {"statistic", "null", "pvalues", "tail",
                                                                                                 "tail_null", "tail_pvalues", "estimator"}
    doc = permutation_test.__doc__
    assert "64" in doc and "stepwise" in doc and "omnibus" in doc


def test_estimator_type_is_checked(no_device):
    from cca_zoo_amd.linear import MCCA, PLS_ALS
    from cca_zoo_amd.model_selection import permutation_test

    X = [np.zeros((20, 3)), np.zeros((20, 4))]
    for bad in (MCCA(), PLS_ALS(), object(), None):
        with pytest.raises(TypeError, match="CCA, rCCA or PLS"):
            permutation_test(bad, X)


def test_unsupported_views_raise_type_errors(no_device):
    import scipy.sparse
    import torch

    from cca_zoo_amd.linear import CCA, rCCA
    from cca_zoo_amd.model_selection import permutation_test

    dense = np.zeros((20, 3))
    with pytest.raises(TypeError, match="sparse"):
        permutation_test(CCA(), [scipy.sparse.csr_matrix(np.eye(20, 4)), dense])
    with pytest.raises(TypeError, match="half-precision"):
        permutation_test(CCA(), [dense.astype(np.float16), dense])
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match="half-precision"):
            permutation_test(rCCA(c=0.1), [_device_like(20, 3, dt), _device_like(20, 4, dt)])
        with pytest.raises(TypeError, match="half-precision"):
            permutation_test(rCCA(c=0.1), [torch.zeros((20, 3), dtype=dt), dense])


def test_row_sharded_is_refused(monkeypatch, no_device):
    from cca_zoo_amd import _dist
    from cca_zoo_amd.linear import PLS
    from cca_zoo_amd.model_selection import permutation_test

    monkeypatch.setattr(_dist, "is_sharded", lambda: True)
    with pytest.raises(NotImplementedError, match="row_sharded"):
        permutation_test(PLS(), [np.zeros((20, 3)), np.zeros((20, 4))])


def test_limits_raise_value_errors(monkeypatch, no_device):
    from cca_zoo_amd.linear import CCA, rCCA
    from cca_zoo_amd.model_selection import _resample
    from cca_zoo_amd.model_selection import permutation_test

    X = [np.zeros((20, 3)), np.zeros((20, 4))]
    with pytest.raises(ValueError, match="at most 64 columns"):
        permutation_test(CCA(), [np.zeros((20, 65)), np.zeros((20, 4))])
    with pytest.raises(ValueError, match="at most 64 columns"):
        permutation_test(CCA(), [np.zeros((20, 4)), np.zeros((20, 200))])
    for bad in (0, -3, 2.5, True, None):
        with pytest.raises(ValueError, match="n_permutations"):
            permutation_test(CCA(), X, n_permutations=bad)
    with pytest.raises(ValueError, match="at least 2 samples"):
        permutation_test(CCA(), [np.zeros((1, 3)), np.zeros((1, 4))])
    with pytest.raises(ValueError, match="exactly 2 views"):
        permutation_test(CCA(), X + [np.zeros((20, 2))])
    with pytest.raises(ValueError, match="At least 2 views"):
        permutation_test(CCA(), X[:1])
    with pytest.raises(ValueError, match="same number of samples"):
        permutation_test(CCA(), [np.zeros((20, 3)), np.zeros((19, 4))])
    with pytest.raises(ValueError):
        permutation_test(rCCA(c=1.5), X)
    with pytest.raises(ValueError, match="length 2"):
        permutation_test(rCCA(c=[0.1, 0.2, 0.3]), X)
    with pytest.raises(ValueError, match="all host arrays or all CUDA tensors"):
        import torch

        permutation_test(CCA(), [_device_like(20, 3, torch.float32), np.zeros((20, 4))])

    class Tall:                                             # 2^31 rows without the memory
        dtype = np.dtype(np.float64)

        def __init__(self, d):
            self.shape = (2 ** 31, d)

    monkeypatch.setattr(_resample, "validate_views", lambda views, **kw: list(views))
    with pytest.raises(ValueError, match="2\\^31"):
        permutation_test(CCA(), [Tall(3), Tall(4)])


def test_the_estimator_passed_in_is_not_fitted_by_a_refused_call(no_device):
    from cca_zoo_amd.linear import CCA
    from cca_zoo_amd.model_selection import permutation_test

    est = CCA(latent_dimensions=2)
    with pytest.raises(ValueError):
        permutation_test(est, [np.zeros((20, 65)), np.zeros((20, 4))])
    assert not hasattr(est, "weights_")
