"""CPU tests of sparse views, everything that happens before the device is touched: the ``allow_sparse`` flag of
``validate_views``, the canonical CSR / CSC pair every scipy format ends as, scipy's full format check, the lanes-per-line
rule of the kernels, and the refusals that stay (every model but PLS_ALS / SCCA_PMD / ParkhomenkoCCA / SCCA_Span)."""

import importlib
import inspect
import pkgutil

import numpy as np
import pytest
import scipy.sparse as sp

SPARSE_MODELS = ("PLS_ALS", "SCCA_PMD", "ParkhomenkoCCA", "SCCA_Span")
GRAM_MODELS = ("SCCA_ADMM", "SCCA_IPLS", "ElasticCCA")


def planted_sparse(seed, n, dims, density, latent=3):
    """Planted sparse non-negative views, float64 CSR holding float32-representable numbers: ``|z A + noise| + 0.25``
    where a Bernoulli mask is set, with one empty row (n // 3) and one empty column (d // 2) per view."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, latent))
    views = []
    for d in dims:
        a = np.abs(z @ rng.standard_normal((latent, d)) + 0.5 * rng.standard_normal((n, d))) + 0.25
        a = np.where(rng.random((n, d)) < density, a, 0.0)
        a[n // 3] = 0.0
        a[:, d // 2] = 0.0
        views.append(sp.csr_matrix(a.astype(np.float32).astype(np.float64)))
    return views


def _pair():
    return planted_sparse(0, 20, (9, 6), 0.4)


# ---- the flag -------------------------------------------------------------------------------------------------------
def test_sparse_views_are_refused_without_the_flag():
    from cca_zoo_amd._utils import validate_views

    with pytest.raises(TypeError, match="[Ss]parse"):
        validate_views(_pair())
    with pytest.raises(TypeError, match="[Ss]parse"):
        validate_views(_pair(), check_finite=False, allow_bf16=True)


def test_the_flag_lets_every_format_pass_as_it_is():
    from cca_zoo_amd._utils import validate_views

    a, b = _pair()
    for conv in ("tocsr", "tocsc", "tocoo", "tolil", "todok", "tobsr", "todia"):
        x = getattr(a, conv)()
        out = validate_views([x, b.toarray()], allow_sparse=True)
        assert out[0] is x and isinstance(out[1], np.ndarray)
    out = validate_views([sp.csc_array(a), sp.coo_array(b)], allow_sparse=True)
    assert out[0].format == "csc" and out[1].format == "coo"


def test_checks_of_a_sparse_view():
    from cca_zoo_amd._utils import validate_views

    a, b = _pair()
    # dtypes: float32 stays, anything else real becomes float64, complex is refused
    out = validate_views([a.astype(np.float32), (b > 0).astype(np.int8), sp.csr_matrix(a > 0)], allow_sparse=True)
    assert [v.dtype for v in out] == [np.float32, np.float64, np.float64]
    with pytest.raises(ValueError, match="numeric"):
        validate_views([a.astype(np.complex128), b], allow_sparse=True)
    # rows
    with pytest.raises(ValueError, match="same number of samples"):
        validate_views([a, b[:-1]], allow_sparse=True)
    with pytest.raises(ValueError, match="same number of samples"):
        validate_views([a, b.toarray()[:-1]], allow_sparse=True)
    with pytest.raises(ValueError, match="2D"):
        validate_views([a, sp.coo_array(np.ones(20))], allow_sparse=True)
    # NaN / infinity among the stored entries, whatever check_finite says and whatever the format
    for bad in (np.nan, np.inf):
        for conv in ("tocsr", "tocoo", "tolil"):
            x = a.copy()
            x.data[3] = bad
            with pytest.raises(ValueError, match="Input contains NaN or infinity."):
                validate_views([getattr(x, conv)(), b], check_finite=False, allow_sparse=True)


# ---- canonical forms ------------------------------------------------------------------------------------------------
def _same_pair(x, y):
    for f, g in zip(x, y):
        assert f.shape == g.shape
        for name in ("data", "indices", "indptr"):
            np.testing.assert_array_equal(getattr(f, name), getattr(g, name))
            assert getattr(f, name).dtype == getattr(g, name).dtype


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_format_gives_the_same_canonical_pair(dtype):
    from cca_zoo_amd._utils._resident import canonical_forms

    a = _pair()[0]
    want = canonical_forms(a, dtype)
    csr, csc = want
    assert csr.format == "csr" and csc.format == "csc"
    assert csr.data.dtype == csc.data.dtype == dtype
    assert csr.indices.dtype == csc.indices.dtype == np.int32 and csr.indptr.dtype == csc.indptr.dtype == np.int64
    assert csr.has_canonical_format and csc.has_canonical_format
    np.testing.assert_array_equal(csr.toarray(), a.toarray().astype(dtype))
    np.testing.assert_array_equal(csc.toarray(), a.toarray().astype(dtype))
    for j in range(a.shape[1]):          # ascending rows within a column: the summation order of the means
        rows = csc.indices[csc.indptr[j]:csc.indptr[j + 1]]
        assert np.all(np.diff(rows) > 0)
    coo = a.tocoo()
    # duplicates: every entry split in two halves (exact in binary), in shuffled order
    perm = np.random.default_rng(1).permutation(2 * coo.nnz)
    dup = sp.coo_matrix((np.tile(coo.data / 2, 2)[perm], (np.tile(coo.row, 2)[perm], np.tile(coo.col, 2)[perm])), shape=a.shape)
    # unsorted indices within the rows
    uns = a.copy()
    for r in range(uns.shape[0]):
        s, e = uns.indptr[r], uns.indptr[r + 1]
        uns.indices[s:e], uns.data[s:e] = uns.indices[s:e][::-1].copy(), uns.data[s:e][::-1].copy()
    uns.has_sorted_indices = False
    # int64 indices
    wide = a.copy()          # (the constructor would narrow them again)
    wide.indices, wide.indptr = wide.indices.astype(np.int64), wide.indptr.astype(np.int64)
    assert wide.indices.dtype == np.int64
    # explicit stored zeros
    zr, zc = np.nonzero(a.toarray() == 0)
    zeros = sp.coo_matrix((np.concatenate([coo.data, np.zeros(5)]), (np.concatenate([coo.row, zr[:5]]),
                                                                      np.concatenate([coo.col, zc[:5]]))), shape=a.shape).tocsr()
    assert zeros.nnz == a.nnz + 5
    variants = {"csr_matrix": sp.csr_matrix(a), "csc_array": sp.csc_array(a), "coo_duplicates": dup, "unsorted": uns,
                "int64": wide, "stored_zeros": zeros, "lil": a.tolil(), "dok": a.todok(), "bsr": a.tobsr(), "dia": a.todia(),
                "coo_array": sp.coo_array(a)}
    for name, v in variants.items():
        before = v.copy()
        _same_pair(canonical_forms(v, dtype), want)
        assert (before != v).nnz == 0 and before.format == v.format, name      # the caller's matrix is left alone
    assert canonical_forms(a, dtype, csc=False)[1] is None


def test_a_malformed_matrix_raises_before_the_device_is_touched():
    from cca_zoo_amd._utils._resident import MEANS_COLMEANS, ResidentViews, canonical_forms
    from cca_zoo_amd.linear import PLS_ALS

    a, b = _pair()
    bad = a.copy()
    bad.indices[2] = a.shape[1]                       # an index >= p put in by hand
    neg = a.copy()
    neg.indices[2] = -1
    ptr = a.copy()
    ptr.indptr[-1] += 3                               # the last pointer past the stored entries
    col = a.tocsc()
    col.indices[0] = a.shape[0]
    coo = a.tocoo()
    coo.col[1] = a.shape[1] + 4
    for m in (bad, neg, ptr, col, coo):
        with pytest.raises(ValueError):
            canonical_forms(m, np.float64)
        with pytest.raises(ValueError):
            ResidentViews([m, b], True, MEANS_COLMEANS, allow_sparse=True)
        with pytest.raises(ValueError):               # no GPU is needed to get here
            PLS_ALS().fit([m, b])
    nan = a.copy()
    nan.data[0] = np.nan
    with pytest.raises(ValueError, match="Input contains NaN or infinity."):
        PLS_ALS().fit([nan, b])


def test_resident_views_know_their_formats_and_dtype():
    from cca_zoo_amd import _backend
    from cca_zoo_amd._utils._resident import MEANS_COLMEANS, ResidentViews

    a, b = _pair()
    d32 = np.ones((20, 4), dtype=np.float32)
    r = ResidentViews([a.astype(np.float32), d32, b.astype(np.float32).tocoo()], True, MEANS_COLMEANS, allow_sparse=True)
    assert r.sparse == [True, False, True] and r.f32 and r.code == _backend.F32 and r.p == [9, 4, 6] and r.n == 20
    r = ResidentViews([a, d32], True, MEANS_COLMEANS, allow_sparse=True)            # one 8-byte view: a float64 fit
    assert r.sparse == [True, False] and not r.f32 and r.code == _backend.F64
    r = ResidentViews([a.astype(np.float32), np.ones((20, 4))], False, MEANS_COLMEANS, allow_sparse=True)
    assert not r.f32
    r = ResidentViews([sp.csr_matrix(a > 0), d32], True, MEANS_COLMEANS, allow_sparse=True)   # bool values become float64
    assert not r.f32
    with pytest.raises(TypeError):
        ResidentViews([a, d32], True, MEANS_COLMEANS)


# ---- the lanes per line ----------------------------------------------------------------------------------------------
def test_group_width_is_a_function_of_the_mean_line_length():
    """G: the smallest power of two not below nnz / lines, within [4, 64] (include/ccz.h: ccz_sparse_group)."""
    from cca_zoo_amd._utils._resident import sparse_group

    lines = 1000
    for mean, want in [(0, 4), (0.3, 4), (1, 4), (4, 4), (4.001, 8), (8, 8), (8.5, 16), (16, 16), (17, 32), (32, 32),
                       (32.001, 64), (41, 64), (64, 64), (65, 64), (2621, 64)]:
        assert sparse_group(int(round(mean * lines)), lines) == want, mean
    assert sparse_group(9, 2) == 8 and sparse_group(8, 2) == 4        # 4.5 and 4 entries per line
    # README shape: n = 4096, p = 262144 at 1 %
    nnz = int(4096 * 262144 * 0.01)
    assert sparse_group(nnz, 4096) == 64 and sparse_group(nnz, 262144) == 64
    from cca_zoo_amd import _backend

    assert _backend.library().ccz_sparse_group(-1, 5) < 0 and _backend.library().ccz_sparse_group(5, 0) < 0


# ---- the refusals that stay -----------------------------------------------------------------------------------------
def _estimators():
    import cca_zoo_amd
    from cca_zoo_amd._base import BaseModel

    found = {}
    for info in pkgutil.iter_modules(cca_zoo_amd.__path__):
        if info.name.startswith("_") or info.name in ("csrc", "lib", "deep", "datasets", "model_selection"):
            continue
        mod = importlib.import_module(f"cca_zoo_amd.{info.name}")
        for name in getattr(mod, "__all__", []):
            c = getattr(mod, name)
            if inspect.isclass(c) and issubclass(c, BaseModel) and not inspect.isabstract(c):
                found[name] = c
    return found


def test_every_other_family_refuses_sparse_views_as_before():
    est = _estimators()
    assert set(SPARSE_MODELS) | set(GRAM_MODELS) <= set(est) and len(est) >= 20
    a, b = _pair()
    for name, cls in est.items():
        if name in SPARSE_MODELS or name in GRAM_MODELS:
            continue
        assert not cls._sparse_views
        kw = {"partials": np.ones((20, 2))} if name == "PartialCCA" else {}
        with pytest.raises(TypeError, match="[Ss]parse"):
            cls().fit([a, b], **kw)
        with pytest.raises(TypeError, match="[Ss]parse"):
            cls().fit([a.toarray(), b], **kw)


@pytest.mark.parametrize("name", GRAM_MODELS)
def test_gram_based_als_models_refuse_sparse_views_by_name(name):
    cls = _estimators()[name]
    a, b = _pair()
    with pytest.raises(ValueError, match=f"{name} needs the Gram"):
        cls().fit([a, b])
    with pytest.raises(ValueError, match=f"{name} needs the Gram"):
        cls().fit([a.toarray(), b])


@pytest.mark.filterwarnings("ignore:Sparse CSR tensor support")
@pytest.mark.parametrize("name", SPARSE_MODELS)
def test_row_sharded_torch_sparse_and_loadings_are_refused(name):
    import torch

    from cca_zoo_amd import _dist

    cls = _estimators()[name]
    assert cls._sparse_views
    a, b = _pair()
    prev = _dist.is_sharded
    _dist.is_sharded = lambda: True
    try:
        with pytest.raises(NotImplementedError, match="row_sharded"):
            cls().fit([a, b])
    finally:
        _dist.is_sharded = prev
    ts = [torch.tensor(a.toarray()).to_sparse(), torch.tensor(b.toarray()).to_sparse()]
    with pytest.raises(TypeError, match="[Ss]parse"):
        cls().fit(ts)
    with pytest.raises(TypeError, match="[Ss]parse"):
        cls().fit([ts[0].to_sparse_csr(), ts[1].to_sparse_csr()])
    # a fitted model (attributes set by hand: no device here) refuses the loadings of a sparse view
    model = cls()
    model.weights_ = [np.ones((9, 1)), np.ones((6, 1))]
    model.means_ = [np.zeros(9), np.zeros(6)]
    with pytest.raises(ValueError, match="get_factor_loadings"):
        model.get_factor_loadings([a, b])
    with pytest.raises(ValueError, match="get_factor_loadings"):
        model.get_factor_loadings([a.toarray(), b])


def test_store_keeps_float64_means_for_sparse_views():
    from cca_zoo_amd.linear import PLS_ALS

    m = PLS_ALS()
    m._store([np.ones((3, 1)), np.ones((2, 1))], [np.zeros(3, dtype=np.float32), np.zeros(2)], "f32", False, sparse=[False, True])
    assert [x.dtype for x in m.means_] == [np.float32, np.float64] and all(w.dtype == np.float64 for w in m.weights_)
    m._store([np.ones((3, 1))], [np.zeros(3, dtype=np.float32)], "f32", False)
    assert m.means_[0].dtype == np.float32
