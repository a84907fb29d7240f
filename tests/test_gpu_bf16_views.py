"""GPU: bfloat16 device views in the closed-form estimators (rCCA / CCA / PLS, MCCA, GCCA, PartialCCA, GRCCA, GridSearchCV over
them, deep.score_representations) and the projection that serves them, ``ccz_transform_wide``.

The kernel (cca_zoo_amd/csrc/project_bf16.hip) is held to the float32 projection's own bar of tests/test_gpu_ops.py against
float64 on the bf16-rounded rows, and to twice the error of the float32 kernel on the same (widened) rows -- three float32
accumulations per k-step instead of one, at most sqrt(3) in a random-walk sum.  The estimators are held to the float32 bar of
tests/test_gpu_edge_cases.py::test_device_tensor_slices_and_dtypes (1e-3 per column of the weights) against the same estimator
fitted on the host on the views' exact float64 images.
"""

import ctypes as C
import functools

import numpy as np
import pytest
from conftest import col_rel_err

pytestmark = pytest.mark.gpu

ROUTE_KERNEL, ROUTE_ADAPTER = 1, 2
CCZ_EINVAL, CCZ_EUNSUP = -1, -6


@pytest.fixture(scope="module")
def H():
    from cca_zoo_amd import _backend

    return _backend.default_handle(0)


# ---------------------------------------------------------------------------------------------------------------------
# ccz_transform_wide through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _project(H, name, code, x, mean, W, out):
    """One projection call on torch tensors (x: n x d view with its own row stride; out: n x ldo float32); returns the raw code."""
    import torch

    sp = int(torch.cuda.current_stream().cuda_stream)
    H.acquire(sp)
    rc = getattr(H.lib, name)(H.raw, code, C.c_void_p(x.data_ptr()), x.shape[0], x.shape[1], x.stride(0),
                              C.c_void_p(mean.data_ptr()) if mean is not None else None, C.c_void_p(W.data_ptr()), W.shape[1],
                              C.c_void_p(out.data_ptr()), out.stride(0))
    H.release(sp)
    return rc


def _last_route(H):
    r = C.c_int(-1)
    H.check(H.lib.ccz_transform_last_route(H.raw, C.byref(r)))
    return r.value


def _rows(n, d, ld, tdt, elem_offset=0, seed=None):
    """randn + 0.3 rounded to the 2-byte type, as columns [0, d) of an (n, ld) buffer that starts `elem_offset` elements into its
    allocation; the padding columns hold other random numbers (nothing may read them)."""
    import torch

    rng = np.random.default_rng(n + d + ld if seed is None else seed)
    full = torch.from_numpy(rng.standard_normal((n, ld)) + 0.3).to(tdt)
    flat = torch.zeros(n * ld + 16, dtype=tdt, device="cuda")
    buf = flat[elem_offset:elem_offset + n * ld].view(n, ld)
    buf.copy_(full)
    return buf[:, :d]


def _case(H, n, d, k, ld_extra, ldo_extra, with_mean, elem_offset=0, tdt=None, seed=None):
    """Runs ccz_transform_wide and, on the widened rows, ccz_transform(CCZ_F32).  Returns (err_new, err_f32, bar, route, out)."""
    import torch

    from cca_zoo_amd import _backend

    tdt = tdt or torch.bfloat16
    rng = np.random.default_rng((n * 131 + d * 17 + k) if seed is None else seed)
    x = _rows(n, d, d + ld_extra, tdt, elem_offset, seed)
    mean_h, W_h = rng.standard_normal(d), rng.standard_normal((d, k))
    mean = torch.from_numpy(mean_h).cuda() if with_mean else None
    W = torch.from_numpy(W_h).cuda()
    ldo = k + ldo_extra
    out = torch.full((n, ldo), 7.0, dtype=torch.float32, device="cuda")
    H.check(_project(H, "ccz_transform_wide", _backend.dtype_code(tdt), x, mean, W, out))
    route = _last_route(H)
    xf = torch.zeros((n, d + ld_extra), dtype=torch.float32, device="cuda")[:, :d]
    xf.copy_(x)
    out32 = torch.full((n, ldo), 7.0, dtype=torch.float32, device="cuda")
    H.check(_project(H, "ccz_transform", _backend.F32, xf, mean, W, out32))
    ref = (x.double().cpu().numpy() - (mean_h if with_mean else 0.0)) @ W_h
    got, got32 = out.cpu().numpy(), out32.cpu().numpy()
    if ldo_extra:
        assert np.all(got[:, k:] == 7.0)                  # padding columns untouched
    scale = np.abs(ref).max()
    return np.abs(got[:, :k] - ref).max(), np.abs(got32[:, :k] - ref).max(), 2e-5 * scale * np.sqrt(d), route, out


KERNEL_SHAPES = [
    (1, 16, 1, 0, 0, 0),          # one row, one k-step: shorter than the ring
    (63, 48, 31, 8, 0, 0),        # fewer k-steps than ring slots
    (65, 80, 33, 0, 3, 0),        # a second column tile, d no multiple of the slot, padded output
    (257, 64, 64, 0, 0, 0),       # exactly one slot
    (300, 1040, 5, 8, 1, 0),      # many ring periods plus a ragged period
    (8193, 320, 17, 0, 0, 0),     # a ragged last workgroup
    (300, 64, 32, 0, 0, 8),       # the base pointer 8 elements into an allocation: still 16-byte aligned
]


@pytest.mark.parametrize("with_mean", [True, False])
@pytest.mark.parametrize("n,d,k,ld_extra,ldo_extra,elem_offset", KERNEL_SHAPES)
def test_kernel_against_float64_and_the_float32_kernel(H, n, d, k, ld_extra, ldo_extra, elem_offset, with_mean):
    err, err32, bar, route, _ = _case(H, n, d, k, ld_extra, ldo_extra, with_mean, elem_offset)
    print(f"bf16 kernel ({n}, {d}, {k}, {ld_extra}, {ldo_extra}) mean={with_mean}: err {err:.3e}, float32 kernel {err32:.3e}, "
          f"ratio {err / max(err32, 1e-300):.3f}, bar {bar:.3e}, route {route}")
    assert route == ROUTE_KERNEL
    assert err < bar
    assert err <= 2.0 * err32


@pytest.mark.parametrize("what,n,d,k,ld_extra,elem_offset", [
    ("d = 40", 300, 40, 5, 0, 0),
    ("ld - d = 4", 300, 48, 5, 4, 0),
    ("base pointer one element off", 300, 64, 5, 0, 1),
    ("k = 65", 300, 64, 65, 0, 0),
])
def test_ineligible_shapes_take_the_adapter(H, what, n, d, k, ld_extra, elem_offset):
    err, err32, bar, route, _ = _case(H, n, d, k, ld_extra, 0, True, elem_offset)
    print(f"adapter, {what}: err {err:.3e}, float32 kernel {err32:.3e}, bar {bar:.3e}, route {route}")
    assert route == ROUTE_ADAPTER
    assert err < bar


def test_float16_rows_take_the_adapter(H):
    import torch

    err, err32, bar, route, _ = _case(H, 300, 64, 8, 0, 0, True, tdt=torch.float16)
    assert route == ROUTE_ADAPTER
    assert err < bar


def test_switch_sends_eligible_rows_to_the_adapter(H, monkeypatch):
    monkeypatch.setenv("CCZ_PROJECT_BF16", "0")
    err, err32, bar, route, _ = _case(H, 300, 64, 8, 0, 0, True)
    assert route == ROUTE_ADAPTER
    assert err < bar
    monkeypatch.delenv("CCZ_PROJECT_BF16")
    assert _case(H, 300, 64, 8, 0, 0, True)[3] == ROUTE_KERNEL


def test_two_calls_give_the_same_bits(H):
    import torch

    a = _case(H, 1000, 336, 40, 8, 0, True, seed=11)
    b = _case(H, 1000, 336, 40, 8, 0, True, seed=11)
    assert a[3] == b[3] == ROUTE_KERNEL
    assert torch.equal(a[4], b[4])


def test_an_inf_and_a_nan_stay_in_their_rows(H):
    import torch

    from cca_zoo_amd import _backend

    n, d, k = 130, 64, 8
    x = _rows(n, d, d, torch.bfloat16)
    rng = np.random.default_rng(5)
    mean, W = torch.from_numpy(rng.standard_normal(d)).cuda(), torch.from_numpy(rng.standard_normal((d, k))).cuda()
    clean = torch.zeros((n, k), dtype=torch.float32, device="cuda")
    H.check(_project(H, "ccz_transform_wide", _backend.BF16, x, mean, W, clean))
    x[5, 3] = float("inf")
    x[70, 20] = float("nan")
    out = torch.zeros((n, k), dtype=torch.float32, device="cuda")
    H.check(_project(H, "ccz_transform_wide", _backend.BF16, x, mean, W, out))
    assert _last_route(H) == ROUTE_KERNEL
    bad = ~torch.isfinite(out).all(dim=1).cpu().numpy()
    assert list(np.flatnonzero(bad)) == [5, 70]
    assert not torch.isfinite(out[5]).any() and torch.isnan(out[70]).all()
    keep = torch.as_tensor(~bad, device="cuda")
    assert torch.equal(out[keep], clean[keep])


def test_argument_checks(H):
    import torch

    from cca_zoo_amd import _backend

    x = _rows(20, 16, 16, torch.bfloat16)
    W = torch.zeros((16, 2), dtype=torch.float64, device="cuda")
    out = torch.zeros((20, 2), dtype=torch.float32, device="cuda")
    assert _project(H, "ccz_transform_wide", _backend.F32, x, None, W, out) == CCZ_EUNSUP
    assert _project(H, "ccz_transform_wide", _backend.F64, x, None, W, out) == CCZ_EUNSUP
    f = H.lib.ccz_transform_wide
    ok = (C.c_void_p(x.data_ptr()), 20, 16, 16, None, C.c_void_p(W.data_ptr()), 2, C.c_void_p(out.data_ptr()), 2)
    assert f(H.raw, _backend.BF16, None, *ok[1:]) == CCZ_EINVAL
    assert f(H.raw, _backend.BF16, *ok[:5], None, *ok[6:]) == CCZ_EINVAL
    assert f(H.raw, _backend.BF16, *ok[:7], None, 2) == CCZ_EINVAL
    assert f(H.raw, _backend.BF16, ok[0], 20, 16, 15, *ok[4:]) == CCZ_EINVAL            # ld < d
    assert f(H.raw, _backend.BF16, *ok[:8], 1) == CCZ_EINVAL                             # ldo < k
    assert f(H.raw, _backend.BF16, *ok) == 0
    H.sync()


# ---------------------------------------------------------------------------------------------------------------------
# the estimators
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planted(n, widths):
    """The planted data of test_device_tensor_slices_and_dtypes at these widths with offsets +0.3 / -0.2 / +0.1, rounded to bfloat16
    (CUDA tensors) and the exact float64 images of those roundings (host arrays).  Checked on the host: at n = 2000, widths 48
    and 32 and c = 0.05 the top singular values are 1.0465, 1.0239, 0.9542 against 0.248; at n = 32773, widths 64 and 48 they are
    1.047, 1.032, 0.973 against 0.079 -- gaps >= 0.02, so the comparison per column is well posed."""
    import torch

    rng = np.random.default_rng(2)
    z = rng.standard_normal((n, 3)) * np.array([2.0, 1.0, 0.5])
    dev, host = [], []
    for w, off in zip(widths, (0.3, -0.2, 0.1)):
        v = torch.from_numpy(z @ rng.standard_normal((3, w)) + rng.standard_normal((n, w)) + off).to(torch.bfloat16).cuda()
        dev.append(v)
        host.append(v.double().cpu().numpy())
    return dev, host


def _check_fit(m, ref, dev, host, wdt):
    import torch

    for a, b in zip(m.weights_, ref.weights_):
        assert a.dtype == wdt
        assert col_rel_err(a, b) < 1e-3, col_rel_err(a, b)
    if m.center:
        assert all(mu.dtype == np.float32 for mu in m.means_)
    np.testing.assert_allclose(m.score(dev), ref.score(host), atol=1e-3)
    zs = m.transform(dev)
    assert all(z.is_cuda and z.dtype == torch.float32 for z in zs)
    return zs


def _make(name):
    from cca_zoo_amd import linear

    kw = {"rCCA": {"c": 0.05}, "CCA": {}, "PLS": {}, "MCCA": {"c": 0.05}, "GCCA": {"c": 0.05}}[name]
    return getattr(linear, name)(latent_dimensions=3, **kw)


# name -> (number of views, dtype of weights_): the dtype flow of float32 views
MODELS = {"rCCA": (2, np.float32), "CCA": (2, np.float32), "PLS": (2, np.float32), "MCCA": (2, np.float64), "GCCA": (3, np.float64)}


@pytest.mark.parametrize("name", list(MODELS))
def test_estimators_on_bf16_views(H, name):
    import torch

    from cca_zoo_amd import _backend

    nv, wdt = MODELS[name]
    dev, host = _planted(2000, (48, 32, 40))
    dev, host = dev[:nv], host[:nv]
    ref = _make(name).fit(host)
    m = _make(name).fit(dev)
    zs = _check_fit(m, ref, dev, host, wdt)
    # transform is the ABI call: float32 variates of the bf16 rows -- the kernel for widths 48 and 32, the adapter for 40 (no
    # multiple of 16)
    for v, mu, w, z in zip(dev, m.means_, m.weights_, zs):
        out = torch.zeros_like(z)
        H.check(_project(H, "ccz_transform_wide", _backend.BF16, v, torch.from_numpy(np.asarray(mu, dtype=np.float64)).cuda(),
                         torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).cuda(), out))
        assert _last_route(H) == (ROUTE_KERNEL if v.shape[1] % 16 == 0 else ROUTE_ADAPTER)
        assert torch.equal(out, z)
    for a, b in zip(m.get_factor_loadings(dev), ref.get_factor_loadings(host)):
        s = np.sign(np.sum(a * b, axis=0))
        np.testing.assert_allclose(a * s, b, atol=1e-3)
    R, Rr = m.pairwise_correlations(dev), ref.pairwise_correlations(host)
    np.testing.assert_allclose(R, Rr, atol=1e-3)


def test_center_false_strided_and_non_contiguous_views():
    import torch

    from cca_zoo_amd.linear import rCCA

    dev, host = _planted(2000, (48, 32))
    ref = rCCA(latent_dimensions=3, c=0.05, center=False).fit(host)
    m = rCCA(latent_dimensions=3, c=0.05, center=False).fit(dev)
    for a, b in zip(m.weights_, ref.weights_):
        assert a.dtype == np.float32 and col_rel_err(a, b) < 1e-3
    assert all(mu.dtype == np.float64 and not mu.any() for mu in m.means_)
    np.testing.assert_allclose(m.score(dev), ref.score(host), atol=1e-3)
    # a view with ld > d, sliced from a wider bf16 tensor (8 elements in: still on 16 bytes), and a non-contiguous column slice
    ref = rCCA(latent_dimensions=3, c=0.05).fit(host)
    big = torch.zeros((2000, 64), dtype=torch.bfloat16, device="cuda")
    big[:, 8:56] = dev[0]
    inter = torch.zeros((2000, 64), dtype=torch.bfloat16, device="cuda")
    inter[:, ::2] = dev[1]
    for views in ([big[:, 8:56], dev[1]], [dev[0], inter[:, ::2]]):
        assert views[0].stride(0) == 64 or views[1].stride(1) == 2
        m = rCCA(latent_dimensions=3, c=0.05).fit(views)
        for a, b in zip(m.weights_, ref.weights_):
            assert col_rel_err(a, b) < 1e-3
        np.testing.assert_allclose(m.score(views), ref.score(host), atol=1e-3)
        plain = rCCA(latent_dimensions=3, c=0.05).fit(dev)
        for z, zp in zip(m.transform(views), plain.transform(dev)):
            assert z.dtype == torch.float32
            np.testing.assert_allclose(z.cpu().numpy(), zp.cpu().numpy(), atol=1e-3)


def test_partial_and_group_estimators():
    import torch

    from cca_zoo_amd.linear import GRCCA, PartialCCA

    dev, host = _planted(2000, (48, 32))
    rng = np.random.default_rng(7)
    partials = rng.standard_normal((2000, 3))
    ref = PartialCCA(latent_dimensions=3, c=0.05).fit(host, partials=partials)
    m = PartialCCA(latent_dimensions=3, c=0.05).fit(dev, partials=torch.from_numpy(partials).cuda())
    for a, b in zip(m.weights_, ref.weights_):
        assert a.dtype == np.float64 and col_rel_err(a, b) < 1e-3, col_rel_err(a, b)
    zs = m.transform(dev, partials=torch.from_numpy(partials).cuda())
    zr = ref.transform(host, partials=partials)
    for z, r in zip(zs, zr):
        assert z.is_cuda and z.dtype == torch.float32
        s = np.sign(np.sum(z.cpu().numpy() * r, axis=0))
        np.testing.assert_allclose(z.cpu().numpy() * s, r, atol=1e-3 * np.abs(r).max())
    # bfloat16 confounds are read as they lie, by K1 and by the residual projection
    pb = torch.from_numpy(partials).to(torch.bfloat16).cuda()
    refb = PartialCCA(latent_dimensions=3, c=0.05).fit(host, partials=pb.double().cpu().numpy())
    mb = PartialCCA(latent_dimensions=3, c=0.05).fit(dev, partials=pb)
    for a, b in zip(mb.weights_, refb.weights_):
        assert col_rel_err(a, b) < 1e-3
    assert all(z.dtype == torch.float32 for z in mb.transform(dev, partials=pb))
    groups = [np.arange(48) % 4, np.arange(32) % 3]
    ref = GRCCA(latent_dimensions=3, c=0.05, mu=0.1).fit(host, feature_groups=groups)
    m = GRCCA(latent_dimensions=3, c=0.05, mu=0.1).fit(dev, feature_groups=groups)
    for a, b in zip(m.weights_, ref.weights_):
        assert a.dtype == np.float64 and col_rel_err(a, b) < 1e-3, col_rel_err(a, b)
    np.testing.assert_allclose(m.score(dev), ref.score(host), atol=1e-3)


def test_split_route_reads_bf16_rows(H):
    from cca_zoo_amd.linear import rCCA

    dev, host = _planted(32773, (64, 48))
    ref = rCCA(latent_dimensions=3, c=0.05).fit(host)
    prev = H.k1_route("bf16x2")
    try:
        m = rCCA(latent_dimensions=3, c=0.05).fit(dev)
        assert H.moments_last_route()[0] == "bf16x2"
        assert m.timings_["k1_route"] == "bf16x2"
    finally:
        H.k1_route(prev)
    for a, b in zip(m.weights_, ref.weights_):
        assert a.dtype == np.float32 and col_rel_err(a, b) < 1e-3, col_rel_err(a, b)
    np.testing.assert_allclose(m.score(dev), ref.score(host), atol=1e-3)


def test_mixed_bf16_and_float32_views_are_the_float32_fit():
    from cca_zoo_amd.linear import MCCA, rCCA

    dev, _ = _planted(2000, (48, 32))
    other = dev[1].float() + 0.001                          # (a float32 view that is no bf16 image)
    for make in (lambda: rCCA(latent_dimensions=3, c=0.05), lambda: MCCA(latent_dimensions=3, c=0.05)):
        a = make().fit([dev[0], other])
        b = make().fit([dev[0].float(), other])
        for wa, wb in zip(a.weights_, b.weights_):
            assert wa.dtype == wb.dtype and np.array_equal(wa, wb)


def test_grid_search_on_bf16_views():
    from cca_zoo_amd.linear import rCCA
    from cca_zoo_amd.model_selection import GridSearchCV

    dev, _ = _planted(600, (48, 32))
    grid = {"c": [0.01, 0.1]}
    gb = GridSearchCV(rCCA(latent_dimensions=3), grid, cv=3).fit(dev)
    gf = GridSearchCV(rCCA(latent_dimensions=3), grid, cv=3).fit([v.float() for v in dev])
    assert gb.route_ == gf.route_ == "shared-moments"
    assert gb.best_params_ == gf.best_params_
    np.testing.assert_allclose(gb.cv_results_["mean_test_score"], gf.cv_results_["mean_test_score"], atol=1e-3)
    assert gb.best_estimator_.weights_[0].dtype == np.float32


def test_row_sharded_at_world_size_one():
    import torch.distributed as dist

    from cca_zoo_amd import row_sharded
    from cca_zoo_amd.linear import MCCA, rCCA

    dev, _ = _planted(2000, (48, 32))
    started = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29689", rank=0, world_size=1)
        started = True
    try:
        for make in (lambda: rCCA(latent_dimensions=3, c=0.05), lambda: MCCA(latent_dimensions=3, c=0.05)):
            plain = make().fit(dev)
            with row_sharded():
                sharded = make().fit(dev)
                score = sharded.score(dev)
            for a, b in zip(sharded.weights_, plain.weights_):
                assert col_rel_err(a, b) < 1e-10
            np.testing.assert_allclose(score, plain.score(dev), atol=1e-10)
    finally:
        if started:
            dist.destroy_process_group()


def test_score_representations_on_bf16():
    from cca_zoo_amd.deep import score_representations

    dev, _ = _planted(2000, (48, 32))
    np.testing.assert_allclose(score_representations(dev, 3), score_representations([v.float() for v in dev], 3), atol=1e-3)


# ---------------------------------------------------------------------------------------------------------------------
# refusals: raised before the device is touched
# ---------------------------------------------------------------------------------------------------------------------
def test_float16_device_views_are_still_refused():
    import torch

    from cca_zoo_amd.linear import MCCA, rCCA

    v = torch.zeros((20, 4), dtype=torch.float16, device="cuda")
    for est in (MCCA(), rCCA()):
        with pytest.raises(ValueError, match="float32 or float64"):
            est.fit([v, v])


def test_other_families_refuse_bf16_views_as_before():
    import torch

    from cca_zoo_amd.linear import CCA_EY, CCAR3, PLS_ALS, SCCA_IPLS, TCCA
    from cca_zoo_amd.nonparametric import KCCA
    from cca_zoo_amd.probabilistic import GFA, ProbabilisticCCA, VariationalBayesCCA
    from cca_zoo_amd.tree import TreeCCA

    dev, _ = _planted(600, (48, 32))
    for est in (CCA_EY(), PLS_ALS(), SCCA_IPLS(), GFA(), VariationalBayesCCA(), ProbabilisticCCA(), KCCA(), TCCA(), CCAR3(), TreeCCA()):
        with pytest.raises(ValueError, match="float32 or float64"):
            est.fit(dev)
    assert all(v.dtype == torch.bfloat16 for v in dev)


def test_mixed_host_and_device_views_raise_as_before():
    from cca_zoo_amd.linear import MCCA

    dev, host = _planted(600, (48, 32))
    with pytest.raises(ValueError, match="all host arrays or all CUDA"):
        MCCA().fit([host[0], dev[1]])
