"""CPU tests of the shared view stager (``cca_zoo_amd/_utils/_resident.py``) on NumPy inputs with a fake handle."""

import numpy as np
import pytest

from cca_zoo_amd import _backend
from cca_zoo_amd._utils._resident import MEANS_COLMEANS, MEANS_TORCH, ResidentViews


class FakeBuffer:
    def __init__(self, ptr):
        self.ptr = ptr


class FakeHandle:
    """Records what ``to_device`` is given; hands out distinct fake addresses."""

    def __init__(self):
        self.uploads = []

    def to_device(self, arr):
        self.uploads.append(np.array(arr, copy=True))
        return FakeBuffer(0x1000 * len(self.uploads))


def _views(dtypes, n=6, p=(3, 5)):
    rng = np.random.default_rng(0)
    return [(10 * rng.standard_normal((n, pi))).astype(dt) for pi, dt in zip(p, dtypes)]


@pytest.mark.parametrize("means", [MEANS_TORCH, MEANS_COLMEANS])
def test_int_view_becomes_float64_and_view_array_is_filled(means):
    views = _views([np.int64, np.float32])
    h = FakeHandle()
    res = ResidentViews(views, True, means, handle=h)
    assert (res.n, res.p, res.f32, res.code) == (6, [3, 5], False, _backend.F64)
    with res as r:
        assert r is res and res.handle is h
        # two views, then two means, all float64 (the float32 view is widened: one dtype per fit)
        assert [u.dtype for u in h.uploads] == [np.float64] * 4
        np.testing.assert_array_equal(h.uploads[0], views[0].astype(np.float64))
        np.testing.assert_array_equal(h.uploads[1], views[1].astype(np.float64))
        for i in range(2):
            np.testing.assert_array_equal(h.uploads[2 + i], views[i].astype(np.float64).mean(axis=0))
            assert (res.varr[i].data, res.varr[i].cols, res.varr[i].ld) == (0x1000 * (i + 1), res.p[i], res.p[i])
            assert res.marr[i] == 0x1000 * (i + 3)
    for mu, v in zip(res.means_host(), views):
        np.testing.assert_array_equal(mu, v.astype(np.float64).mean(axis=0))


def test_f32_only_when_every_view_is_float32():
    assert ResidentViews(_views([np.float32, np.float32]), True, MEANS_TORCH).f32
    assert ResidentViews(_views([np.float32, np.float32]), True, MEANS_TORCH).code == _backend.F32
    assert not ResidentViews(_views([np.float32, np.float64]), True, MEANS_TORCH).f32
    assert not ResidentViews(_views([np.float32, np.int32]), True, MEANS_TORCH).f32
    h = FakeHandle()
    views = _views([np.float32, np.float32])
    with ResidentViews(views, True, MEANS_TORCH, handle=h) as res:
        assert [u.dtype for u in h.uploads] == [np.float32] * 4
    assert [mu.dtype for mu in res.means_host()] == [np.float32] * 2
    np.testing.assert_array_equal(res.means_host()[1], views[1].mean(axis=0))


def test_non_finite_host_view_raises_before_any_upload():
    views = _views([np.float64, np.float64])
    views[1][2, 1] = np.inf
    h = FakeHandle()
    with pytest.raises(ValueError, match=r"^Input contains NaN or infinity\.$"):
        with ResidentViews(views, True, MEANS_COLMEANS, handle=h):
            pass
    assert h.uploads == []


def test_mixed_views_raise_the_existing_text(monkeypatch):
    from cca_zoo_amd._utils import _resident

    class FakeTensor:
        shape = (6, 4)

    real = _resident.is_device_tensor
    monkeypatch.setattr(_resident, "is_device_tensor", lambda v: isinstance(v, FakeTensor) or real(v))
    monkeypatch.setattr(_resident, "validate_views", lambda views, **kw: list(views))
    with pytest.raises(ValueError, match="^views must be all host arrays or all CUDA tensors$"):
        ResidentViews([np.zeros((6, 3)), FakeTensor()], True, MEANS_TORCH, handle=FakeHandle())


def test_no_means_without_centring():
    h = FakeHandle()
    with ResidentViews(_views([np.float64, np.float64]), False, MEANS_COLMEANS, handle=h) as res:
        assert res.marr is None
        assert len(h.uploads) == 2
    mus = res.means_host()
    assert [mu.shape for mu in mus] == [(3,), (5,)] and not any(mu.any() for mu in mus)


def test_unknown_means_policy_is_refused():
    with pytest.raises(ValueError, match="unknown means policy"):
        ResidentViews(_views([np.float64, np.float64]), True, "numpy")
