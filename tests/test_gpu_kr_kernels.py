"""ccz_kr_moment / ccz_kr_apply through ctypes against np.einsum, elementwise, at the rounding bound of both sides:
``2 (n + V) 2^-53 scale sum_s prod_i |H_i[s, r_i]|`` for the moment (each side sums n terms of V-fold products: at most
(n + V) roundings per side), the same contraction of absolute values with ``|T|`` for the apply.  The apply's sum has
``prod d / d_mode`` terms per sample instead of n: where that is fewer than n, the smaller count sets the factor."""

import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GOLDEN_SHAPES = [(96, (5, 4, 3)), (64, (6, 4)), (80, (3, 2, 4, 3)), (200, (17, 16, 9)), (70, (33, 2, 5)), (33, (4, 1, 3)),
                 (120, (2, 3, 40)), (4100, (3, 2, 2))]
EXTRA_SHAPES = [(257, (16, 16, 16)), (64, (65, 4)), (5, (3, 3, 3))]
LETTERS = "abcdefgh"


def _handle():
    from cca_zoo_amd import _backend

    return _backend.default_handle(0), _backend


def _views(_backend, ts):
    v = (_backend.View * len(ts))()
    for i, t in enumerate(ts):
        v[i].data, v[i].cols, v[i].ld = t.data_ptr(), int(t.shape[1]), int(t.stride(0))
    return v


def _make(n, dims, seed, pad=0):
    """float64 device views (column slices of wider tensors when ``pad``: a non-contiguous ld) and their host copies."""
    rng = np.random.default_rng(seed)
    host = [rng.standard_normal((n, d)) for d in dims]
    dev = []
    for x in host:
        wide = torch.full((n, x.shape[1] + 2 * pad), 7.0, dtype=torch.float64, device="cuda")
        wide[:, pad:pad + x.shape[1]] = torch.tensor(x)
        dev.append(wide[:, pad:pad + x.shape[1]])
    return host, dev


def _moment_expr(V):
    return ",".join("s" + LETTERS[i] for i in range(V)) + "->" + LETTERS[:V]


def _apply_expr(V, mode):
    return LETTERS[:V] + "," + ",".join("s" + LETTERS[i] for i in range(V) if i != mode) + "->s" + LETTERS[mode]


def _moment(h, _backend, dev, n, scale):
    M = torch.full([int(t.shape[1]) for t in dev], float("nan"), dtype=torch.float64, device="cuda")
    h.check(h.lib.ccz_kr_moment(h.raw, _views(_backend, dev), len(dev), n, scale, C.c_void_p(M.data_ptr())))
    h.sync()
    return M.cpu().numpy()


def _apply(h, _backend, dev, n, T, mode, scale, ldo_pad=0):
    dj = int(dev[mode].shape[1])
    out = torch.full((n, dj + ldo_pad), float("nan"), dtype=torch.float64, device="cuda")
    h.check(h.lib.ccz_kr_apply(h.raw, _views(_backend, dev), len(dev), n, C.c_void_p(T.data_ptr()), mode, scale,
                               C.c_void_p(out.data_ptr()), dj + ldo_pad))
    h.sync()
    got = out.cpu().numpy()
    assert np.isnan(got[:, dj:]).all()                      # nothing written past the d_mode columns
    return got[:, :dj]


@pytest.mark.parametrize("n,dims", GOLDEN_SHAPES + EXTRA_SHAPES)
@pytest.mark.parametrize("pad,scale", [(0, 1.0), (3, 0.37)])
def test_kr_moment_matches_einsum(n, dims, pad, scale):
    h, _backend = _handle()
    host, dev = _make(n, dims, 11 + len(dims) + n, pad)
    V = len(dims)
    got = _moment(h, _backend, dev, n, scale)
    want = scale * np.einsum(_moment_expr(V), *host)
    bound = 2 * (n + V) * U * abs(scale) * np.einsum(_moment_expr(V), *[np.abs(x) for x in host])
    assert np.isfinite(got).all()
    assert (np.abs(got - want) <= bound).all(), float((np.abs(got - want) / bound).max())


@pytest.mark.parametrize("n,dims", GOLDEN_SHAPES + EXTRA_SHAPES)
@pytest.mark.parametrize("pad,scale", [(0, 1.0), (3, 0.37)])
def test_kr_apply_matches_einsum_for_every_mode(n, dims, pad, scale):
    h, _backend = _handle()
    host, dev = _make(n, dims, 23 + len(dims) + n, pad)
    V = len(dims)
    Th = np.random.default_rng(5).standard_normal(dims)
    T = torch.tensor(Th, device="cuda")
    for mode in range(V):
        got = _apply(h, _backend, dev, n, T, mode, scale, ldo_pad=pad)
        others = [x for i, x in enumerate(host) if i != mode]
        want = scale * np.einsum(_apply_expr(V, mode), Th, *others)
        terms = int(np.prod(dims)) // dims[mode]
        bound = 2 * (min(n, terms) + V) * U * abs(scale) * np.einsum(_apply_expr(V, mode), np.abs(Th), *[np.abs(x) for x in others])
        assert np.isfinite(got).all()
        assert (np.abs(got - want) <= bound).all(), (mode, float((np.abs(got - want) / bound).max()))


def test_two_calls_give_equal_bits():
    h, _backend = _handle()
    for n, dims in [(4100, (3, 2, 2)), (257, (16, 16, 16))]:
        host, dev = _make(n, dims, 3)
        a, b = _moment(h, _backend, dev, n, 1.0 / n), _moment(h, _backend, dev, n, 1.0 / n)
        assert a.tobytes() == b.tobytes()
        T = torch.tensor(a, device="cuda")
        for mode in range(len(dims)):
            x, y = _apply(h, _backend, dev, n, T, mode, 1.0 / n), _apply(h, _backend, dev, n, T, mode, 1.0 / n)
            assert x.tobytes() == y.tobytes()


def test_argument_errors_are_einval_with_a_message():
    h, _backend = _handle()
    _, dev = _make(8, (2, 2, 2, 2, 2, 2, 2, 2, 2), 1)
    M = torch.zeros(512, dtype=torch.float64, device="cuda")
    out = torch.zeros((8, 4096), dtype=torch.float64, device="cuda")
    msg = lambda: h.lib.ccz_last_error(h.raw).decode()
    assert h.lib.ccz_kr_moment(h.raw, _views(_backend, dev), 9, 8, 1.0, C.c_void_p(M.data_ptr())) == -1 and "n_views" in msg()
    assert h.lib.ccz_kr_moment(h.raw, _views(_backend, dev[:1]), 1, 8, 1.0, C.c_void_p(M.data_ptr())) == -1 and "n_views" in msg()
    assert h.lib.ccz_kr_apply(h.raw, _views(_backend, dev[:3]), 3, 8, C.c_void_p(M.data_ptr()), 3, 1.0, C.c_void_p(out.data_ptr()), 2) == -1
    assert "mode" in msg()
    assert h.lib.ccz_kr_apply(h.raw, _views(_backend, dev[:3]), 3, 8, C.c_void_p(M.data_ptr()), -1, 1.0, C.c_void_p(out.data_ptr()), 2) == -1
    assert "mode" in msg()
    big = [torch.zeros((8, 4096), dtype=torch.float64, device="cuda") for _ in range(2)] + [dev[0]]      # 2^25 entries
    assert h.lib.ccz_kr_moment(h.raw, _views(_backend, big), 3, 8, 1.0, C.c_void_p(M.data_ptr())) == -1 and "2^24" in msg()
    assert h.lib.ccz_kr_apply(h.raw, _views(_backend, big), 3, 8, C.c_void_p(M.data_ptr()), 0, 1.0, C.c_void_p(out.data_ptr()), 4096) == -1
    assert "2^24" in msg()
    with pytest.raises(ValueError, match="n_views"):
        h.check(h.lib.ccz_kr_moment(h.raw, _views(_backend, dev), 9, 8, 1.0, C.c_void_p(M.data_ptr())))
