"""GPU tests of PLS_ALS / SCCA_PMD / ParkhomenkoCCA / SCCA_Span on ``scipy.sparse`` views: every fit against the same
estimator on ``toarray()`` float64 host arrays and against the CPU restatement (tests/test_als_host.py::restate) at the
family's device bar, with equal sweep counts and identical supports; transform / score of held-out sparse views; mixed
sparse / dense fits; float32 values; the methods' contracts."""

import functools

import numpy as np
import pytest
import scipy.sparse as sp

from test_als_host import col_err, restate, support
from test_sparse_views_host import planted_sparse

pytestmark = pytest.mark.gpu

W_TOL = 1e-8          # the family's device bar: largest per-column relative error
MAX_ITER = 40

# seed, n, dims, density
SHAPES = {"2views": (1, 70, (300, 190), 0.08), "3views": (2, 41, (1030, 517, 66), 0.03)}
# Thresholding parameters chosen on the restatement so that every column of every view has a support strictly between 1
# and p entries (asserted below): the rule bites, a fit cannot pass by never thresholding.
PARAMS = {
    "2views": {"PLS_ALS": {}, "SCCA_PMD": {"tau": [0.5, 0.5]}, "ParkhomenkoCCA": {"tau": [0.6, 0.6]}, "SCCA_Span": {"span": [50, 31]}},
    "3views": {"PLS_ALS": {}, "SCCA_PMD": {"tau": [0.5, 0.5, 0.9]}, "ParkhomenkoCCA": {"tau": [0.3, 0.3, 0.05]},
               "SCCA_Span": {"span": [171, 86, 11]}},
}
MODELS = ("PLS_ALS", "SCCA_PMD", "ParkhomenkoCCA", "SCCA_Span")


def _cls(name):
    import cca_zoo_amd.linear as lin

    return getattr(lin, name)


@functools.lru_cache(maxsize=None)
def _views(shape, seed_shift=0):
    seed, n, dims, density = SHAPES[shape]
    return tuple(planted_sparse(seed + 100 * seed_shift, n, dims, density))


def _params(shape, model, center, k):
    return dict(latent_dimensions=k, center=center, max_iter=MAX_ITER, tol=1e-6, random_state=3, **PARAMS[shape][model])


@functools.lru_cache(maxsize=None)
def _restated(shape, model, center, k):
    dense = [v.toarray() for v in _views(shape)]
    return restate(dense, model, **_params(shape, model, center, k))


@functools.lru_cache(maxsize=None)
def _dense_fit(shape, model, center, k):
    return _cls(model)(**_params(shape, model, center, k)).fit([v.toarray() for v in _views(shape)])


def _formats(views):
    """The same matrices in a mix of scipy formats."""
    conv = ("tocsr", "tocsc", "tocoo")
    return [getattr(v, conv[i % 3])() for i, v in enumerate(views)]


def _agree(model, ref_weights, ref_iters, what):
    worst = 0.0
    assert model.n_iter_ == list(ref_iters), (what, model.n_iter_, ref_iters)
    for i, (w, r) in enumerate(zip(model.weights_, ref_weights)):
        assert w.dtype == np.float64
        for a, b in zip(support(w), support(r)):
            np.testing.assert_array_equal(a, b)
        err = col_err(w, r)
        worst = max(worst, err)
        assert err <= W_TOL, (what, i, err)
    return worst


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("center", [True, False], ids=["centred", "uncentred"])
@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_sparse_fit_matches_the_dense_float64_fit_and_the_restatement(shape, name, center, k):
    views = _views(shape)
    W, sweeps, _ = _restated(shape, name, center, k)
    if name != "PLS_ALS":
        for w, v in zip(W, views):
            nnz = [int(np.count_nonzero(w[:, d])) for d in range(k)]
            assert all(1 < c < v.shape[1] for c in nnz), (name, nnz)
    dense = _dense_fit(shape, name, center, k)
    model = _cls(name)(**_params(shape, name, center, k)).fit(_formats(views))
    a = _agree(model, dense.weights_, dense.n_iter_, "dense float64 fit")
    b = _agree(model, W, sweeps, "restatement")
    print(f"sparse {shape} {name} centre={center} k={k}: worst col err vs dense fit {a:.2e}, vs restatement {b:.2e}, sweeps {sweeps}")
    n = views[0].shape[0]
    for v, mu in zip(views, model.means_):
        assert mu.dtype == np.float64 and mu.shape == (v.shape[1],)
        want = np.asarray(v.sum(axis=0)).ravel() / n if center else np.zeros(v.shape[1])
        assert np.max(np.abs(mu - want)) <= 1e-12 * max(np.max(np.abs(want)), 1.0)
    # held-out sparse views against the dense fit's outputs
    held = _views(shape, 1)
    zs, zd = model.transform(_formats(held)), dense.transform([v.toarray() for v in held])
    for x, y in zip(zs, zd):
        assert isinstance(x, np.ndarray) and x.dtype == np.float64 and x.shape == y.shape
        assert col_err(x, y) <= W_TOL
    np.testing.assert_allclose(model.score(list(held)), dense.score([v.toarray() for v in held]), rtol=0, atol=W_TOL)


@pytest.mark.parametrize("name", MODELS)
def test_float32_values_give_the_bits_of_float64_values(name):
    """The generator's numbers are float32-representable: the same fit, bit for bit, and float64 means."""
    views = _views("3views")
    p = _params("3views", name, True, 3)
    a = _cls(name)(**p).fit(list(views))
    b = _cls(name)(**p).fit([v.astype(np.float32) for v in views])
    assert a.n_iter_ == b.n_iter_
    for x, y in zip(a.weights_ + a.means_, b.weights_ + b.means_):
        assert y.dtype == np.float64
        np.testing.assert_array_equal(x, y)
    for x, y in zip(a.transform(list(views)), b.transform([v.astype(np.float32) for v in views])):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("which", [(0,), (1, 2)], ids=["first_sparse", "last_two_sparse"])
def test_mixed_sparse_and_dense_views(name, which):
    views = _views("3views")
    dense = _dense_fit("3views", name, True, 3)
    mixed = [v if i in which else v.toarray() for i, v in enumerate(views)]
    model = _cls(name)(**_params("3views", name, True, 3)).fit(mixed)
    worst = _agree(model, dense.weights_, dense.n_iter_, "dense float64 fit")
    print(f"mixed {name} sparse views {which}: worst col err {worst:.2e}")
    held = _views("3views", 1)
    hm = [v if i in which else v.toarray() for i, v in enumerate(held)]
    for x, y in zip(model.transform(hm), dense.transform([v.toarray() for v in held])):
        assert col_err(x, y) <= W_TOL
    np.testing.assert_allclose(model.average_pairwise_correlations(hm),
                               dense.average_pairwise_correlations([v.toarray() for v in held]), rtol=0, atol=W_TOL)


def test_mixed_float32_dense_view_keeps_its_own_means_dtype():
    from cca_zoo_amd.linear import PLS_ALS

    views = _views("2views")
    d32 = views[1].toarray().astype(np.float32)
    model = PLS_ALS(max_iter=5, random_state=0).fit([views[0].astype(np.float32), d32])
    assert [m.dtype for m in model.means_] == [np.float64, np.float32]
    np.testing.assert_array_equal(model.means_[1], d32.mean(axis=0))
    assert all(w.dtype == np.float64 for w in model.weights_)


def test_two_sparse_fits_are_bit_identical():
    from cca_zoo_amd.linear import SCCA_PMD

    views = _views("3views")
    p = _params("3views", "SCCA_PMD", True, 3)
    a, b = SCCA_PMD(**p).fit(list(views)), SCCA_PMD(**p).fit(_formats(views))
    assert a.n_iter_ == b.n_iter_
    for x, y in zip(a.weights_, b.weights_):
        np.testing.assert_array_equal(x, y)


def test_methods_of_a_model_fitted_on_sparse_views():
    from cca_zoo_amd.linear import ParkhomenkoCCA

    views = list(_views("2views"))
    p = _params("2views", "ParkhomenkoCCA", True, 3)
    model = ParkhomenkoCCA(**p)
    z = model.fit_transform(views)
    for a, b in zip(z, model.transform(views)):
        np.testing.assert_array_equal(a, b)
    R = model.pairwise_correlations(views)
    assert R.shape == (2, 2, 3) and np.all(np.isfinite(R))
    np.testing.assert_allclose(model.score(views), model.average_pairwise_correlations(views))
    with pytest.raises(ValueError, match="get_factor_loadings"):
        model.get_factor_loadings(views)
    loadings = model.get_factor_loadings([v.toarray() for v in views])          # dense views still work
    assert [x.shape for x in loadings] == [(300, 3), (190, 3)]
    with pytest.raises(ValueError, match="columns"):
        model.transform([views[0][:, :10], views[1]])
    # the caller's matrices are left as they were
    for v, w in zip(views, _views("2views")):
        assert (v != w).nnz == 0
    # a dense view with a non-finite value next to a sparse one
    bad = views[1].toarray()
    bad[3, 4] = np.inf
    with pytest.raises(ValueError, match="Input contains NaN or infinity."):
        ParkhomenkoCCA(**p).fit([views[0], bad])


def test_zero_sparse_view_exercises_the_guards():
    """A view without stored entries: zeros throughout, as the dense fit gives, and no NaN."""
    from cca_zoo_amd.linear import PLS_ALS, ParkhomenkoCCA

    X = _views("2views")[0]
    Z = sp.csr_matrix((X.shape[0], 5))
    for cls in (PLS_ALS, ParkhomenkoCCA):
        model = cls(latent_dimensions=2, max_iter=5, random_state=0).fit([X, Z])
        W, sweeps, _ = restate([X.toarray(), Z.toarray()], cls.__name__, latent_dimensions=2, max_iter=5, random_state=0)
        assert model.n_iter_ == sweeps
        for w, r in zip(model.weights_, W):
            assert np.all(np.isfinite(w))
            np.testing.assert_allclose(w, r, atol=1e-12)
        assert np.all(model.weights_[0] == 0)
