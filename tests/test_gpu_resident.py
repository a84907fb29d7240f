"""GPU tests of the shared view stager (``cca_zoo_amd/_utils/_resident.py``): what it hands libccz for strided CUDA
tensors, and that a refused fit gives the caller's stream back."""

import numpy as np
import pytest

from test_ey_host import col_err

pytestmark = pytest.mark.gpu


def _two_views(seed=5, n=64, dims=(8, 8)):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, 2))
    return [z @ rng.standard_normal((2, d)) + 0.5 * rng.standard_normal((n, d)) + 0.25 for d in dims]


def _refused_ey():
    """17 views pass every Python check and are refused by ``ccz_ey_create``, after the stream was acquired."""
    import torch

    from cca_zoo_amd.linear import CCA_EY

    views = [torch.as_tensor(v, device="cuda") for v in _two_views(seed=6, dims=(4,) * 17)]
    with pytest.raises(ValueError, match="1 to 16 views"):
        CCA_EY(latent_dimensions=1, max_iter=3, random_state=0).fit(views)


def _refused_als():
    import torch

    from cca_zoo_amd.linear import PLS_ALS

    with pytest.raises(ValueError, match="at most 32"):
        PLS_ALS(latent_dimensions=33).fit([torch.as_tensor(v, device="cuda") for v in _two_views()])


@pytest.mark.parametrize("family", ["ey", "als"])
def test_refused_fit_releases_the_callers_stream(family):
    """After a refused fit of CUDA tensors, a fit of CUDA tensors on the same handle and stream equals the fit of the
    same data from host arrays (the tolerance of test_gpu_ey.py::test_device_tensors_match_host_arrays, float64)."""
    import torch

    from cca_zoo_amd.linear import CCA_EY, PLS_ALS

    def make():
        if family == "ey":
            return CCA_EY(latent_dimensions=2, c=0.3, batch_size=16, max_iter=30, learning_rate=0.01, tol=0.0,
                          random_state=0)
        return PLS_ALS(latent_dimensions=2, max_iter=50, random_state=0)

    views = _two_views()
    host = make().fit(views)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _refused_ey() if family == "ey" else _refused_als()
        dev = make().fit([torch.as_tensor(v, device="cuda") for v in views])
    side.synchronize()
    assert dev.n_iter_ == host.n_iter_
    for a, b in zip(dev.weights_, host.weights_):
        assert np.all(np.isfinite(a))
        assert col_err(a, b) <= 1e-12, col_err(a, b)


@pytest.mark.parametrize("means", ["torch", "colmeans"])
@pytest.mark.parametrize("layout", ["row_strided", "column_strided"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_strided_cuda_tensors_as_libccz_sees_them(dtype, layout, means):
    """A row stride of cols + 3 is handed through (ld = cols + 3, same pointer); a column-strided tensor is copied
    (ld = cols).  The rows behind ``varr`` and the means behind ``marr``, read back with ccz_memcpy_d2h, are the input's."""
    import torch

    from cca_zoo_amd._utils._resident import ResidentViews

    n, dims = 33, (5, 12)
    rng = np.random.default_rng(3)
    hosts = [(rng.standard_normal((n, d)) + 1.5).astype(dtype) for d in dims]
    tens = []
    for x in hosts:
        d = x.shape[1]
        if layout == "row_strided":
            big = torch.zeros((n, d + 3), dtype=torch.as_tensor(x).dtype, device="cuda")
            big[:, :d] = torch.as_tensor(x, device="cuda")
            t = big[:, :d]
            assert t.stride() == (d + 3, 1)
        else:
            t = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda").T
            assert t.stride() == (1, n)
        tens.append(t)
    with ResidentViews(tens, True, means) as res:
        h = res.handle
        assert (res.n, res.p, res.f32) == (n, list(dims), dtype == np.float32)
        for i, (x, t) in enumerate(zip(hosts, tens)):
            d = x.shape[1]
            ld = d + 3 if layout == "row_strided" else d
            assert (res.varr[i].cols, res.varr[i].ld) == (d, ld)
            assert (res.varr[i].data == t.data_ptr()) == (layout == "row_strided")
            flat = h.to_host(int(res.varr[i].data), ((n - 1) * ld + d,), dtype=dtype)
            rows = np.lib.stride_tricks.as_strided(flat, (n, d), (ld * flat.itemsize, flat.itemsize))
            np.testing.assert_array_equal(rows, x)
            mu = h.to_host(int(res.marr[i]), (d,), dtype=dtype)
            if means == "colmeans":
                np.testing.assert_array_equal(mu, x.mean(axis=0))
            else:
                staged = t if layout == "row_strided" else t.contiguous()      # what the stager takes the mean of
                np.testing.assert_array_equal(mu, staged.mean(dim=0).cpu().numpy())
    for mu, x in zip(res.means_host(), hosts):
        assert mu.dtype == dtype
        np.testing.assert_allclose(mu, x.mean(axis=0), rtol=1e-6 if dtype == np.float32 else 1e-14)
