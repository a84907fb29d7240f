"""The split-bf16 K1 route (csrc/gram_split.hip, the split branch of gram.hip::launch_moments) on STRUCTURED float32 views, through
the C ABI, against the host statement of its arithmetic (tests/split_emulation.py) -- tests/test_gpu_k1_split.py draws Gaussian
rows only, and for those the route's premise (every dropped product is zero-mean and averages out over the rows) holds by itself.

(a) Exact cases.  0/1 features, one-hot blocks, Poisson counts, integers 300 +- 3, 7-bit pixel values: with the coarse pilot of
    float32 views (k_pilot_coarse) x - p stays on the rows' grid, mid = 0, and every product and every float32 chunk sum (256-row
    chunks) is an exactly representable number -- the device's moments EQUAL the float64 X'X, no tolerance.  With the plain sample
    mean as the pilot, which the route used before, this group fails at 2e-6 ... 3e-6 (0/1, one-hot).  Sparse signed integers of 9 and 10 bits put
    the mid plane to the same test: the reference is the designed result in integers, which lacks the off-diagonal mid * mid.
    (Magnitudes up to 2047 cannot meet the validity bound below: one entry v alone contributes v^2 >= 2^22 to a window's
    sum |terms| on the diagonal.  The bound stays; the magnitudes are [256, 1023] on 1/512 of the entries.)
    Before any GPU call each case asserts on the host that the window maximum of sum |terms| is below 2^22 u_i u_j and that the
    pilot does not depend on the order of the sample's sums (split_emulation.settle_pilot moves single entries of sampled rows
    until no column sits on a rounding boundary: among hundreds of grid-valued columns a plain seed always leaves one there).
    The coarse pilot is taken by the columns whose sampled values lie on a grid (k_sample_grid); every other float32 column keeps
    the sample mean and the bits its moments always had -- ReLU outputs among them, whose 2e-6 ... 3e-6 is therefore pinned in (b).
(b) Faithful-to-design cases, 256-row chunks: Gaussian (the control), ReLU, float32 up-cast from bfloat16, mean = 1000 sigma, and
    the four inputs whose error is pinned, not fixed -- columns duplicated across views (the cross-view copy of a diagonal entry
    lacks sum mid^2: k_split_reduce adds it where i == j in G only), one row at 1e4 sigma, Student-t rows with 2.5 degrees of
    freedom, a period-16 input whose phase 0 is shifted by 20 sigma (at 33000 rows the pilot sample's stride is 16: it sees phase 0
    only).  a_ref = rel(moments_f32_chunks(256), G_emul) is the host model's float32 accumulation error; the device must stay
    within 4 a_ref of the emulation (the matrix pipe's summation order inside a chunk against the BLAS one, the maximum over D^2
    entries) and its total error within the design's own plus 4 a_ref.
(c) The same at the default chunk length (a_ref from 16384-row chunks).
(d) rCCA on two identical views: canonical correlations against the oracle's float64 generalised eigenproblem on the emulated moments.

Measured (MI355X; rel = tests/test_gpu_k1_split.py::_rel; ratio = rel(G_gpu, G_emul) / a_ref):

    case (256-row chunks)          rel(G_emul,G64)  a_ref      rel(G_gpu,G_emul)  ratio  rel(G_gpu,G64)
    gaussian 4099                  3.94e-07         6.09e-07   1.73e-07           0.28   4.29e-07
    gaussian 5000                  4.20e-07         5.67e-07   1.34e-07           0.24   4.29e-07
    gaussian 33000                 1.38e-07         5.04e-07   6.67e-08           0.13   1.55e-07
    relu 4099                      2.23e-06         2.88e-06   1.09e-07           0.04   2.23e-06
    relu 5000                      2.75e-06         3.10e-06   9.92e-08           0.03   2.76e-06
    relu 33000                     3.02e-06         2.80e-06   4.91e-08           0.02   3.03e-06
    from_bf16 4099                 1.29e-07         4.42e-07   1.06e-07           0.24   1.24e-07
    from_bf16 5000                 1.19e-07         4.38e-07   1.19e-07           0.27   1.29e-07
    from_bf16 33000                4.46e-08         4.59e-07   8.68e-08           0.19   8.68e-08
    mean1000 4099                  2.25e-13         5.82e-13   1.42e-13           0.24   2.49e-13
    mean1000 5000                  2.19e-13         4.70e-13   1.65e-13           0.35   2.33e-13
    mean1000 33000                 9.18e-14         3.32e-13   6.11e-14           0.18   1.00e-13
    duplicate 4099                 3.13e-06         6.11e-07   1.30e-07           0.21   3.14e-06
    duplicate 5000                 3.13e-06         6.03e-07   1.66e-07           0.28   3.11e-06
    duplicate 33000                2.85e-06         5.01e-07   6.37e-08           0.13   2.87e-06
    outlier_row 4099               9.76e-06         1.21e-06   6.35e-07           0.52   9.87e-06
    outlier_row 5000               1.23e-05         1.19e-06   6.37e-07           0.54   1.21e-05
    outlier_row 33000              1.55e-05         2.36e-07   2.75e-07           1.16   1.55e-05
    student_t 4099                 6.28e-06         6.32e-07   2.46e-07           0.39   6.29e-06
    student_t 5000                 8.42e-06         7.95e-07   3.75e-07           0.47   8.36e-06
    student_t 33000                6.05e-06         5.18e-07   2.16e-07           0.42   6.06e-06
    period16 4099                  9.50e-07         1.20e-06   1.44e-07           0.12   9.63e-07
    period16 5000                  9.66e-07         1.19e-06   1.74e-07           0.15   1.03e-06
    period16 33000                 1.68e-06         1.98e-06   8.83e-07           0.45   1.88e-06
    relu 33000 (long chunks)       3.02e-06         2.46e-06   2.33e-07           0.10   3.00e-06
    identical views (rCCA, k = 4)  1 - sigma_ref = 2.553e-06 2.562e-06 2.573e-06 2.582e-06;  measured 1 - sigma = 2.553e-06 2.562e-06 2.573e-06 2.582e-06
    (|sigma - sigma_ref| <= 1.4e-10)
    exact group, every case and the auto case: rel(G_gpu, G_ref) = 0 (bit for bit).  The same group against the build before
    k_pilot_coarse (mean pilot), run once: binary 2.92e-06 / 3.06e-06 / 3.09e-06 (4099 / 5000 / 33000 rows), 3.06e-06 on auto;
    one-hot 2.00e-06 / 2.02e-06 / 1.96e-06; counts 4.7e-07 ... 4.9e-07; int300 1.3e-10; pixels7 1.34e-06 ... 1.60e-06;
    sparse integers 6.50e-06 / 6.73e-06 / 3.06e-06 -- all 19 cases failed there.
"""

import functools
import os

import numpy as np
import pytest

import split_emulation as E

pytestmark = pytest.mark.gpu

SHAPES = [(4099, [257, 63]),            # one-column panel remainder, 3 rows in the last k-step, unaligned rows
          (5000, [300, 520]),           # ragged multi-panel, cross-view tiles, a diagonal and an off-diagonal tile per view
          (33000, [128, 384, 200])]     # three views, more than two row chunks
EXACT = ["binary", "onehot", "counts", "int300", "pixels7"]
FAITHFUL = ["gaussian", "relu", "from_bf16", "mean1000", "duplicate", "outlier_row", "student_t", "period16"]
KINDS = EXACT + ["sparse_int"] + FAITHFUL
WINDOW_BOUND = 2.0 ** 22                # two bits under float32's 24


@pytest.fixture(scope="module")
def H():
    from cca_zoo_amd import _backend

    h = _backend.default_handle(0)
    yield h
    h.k1_route("auto")


def _moments(H, views, route):
    """Device-resident float32 views through ``H.moments`` with the handle's route set (and restored): G, s, the route taken."""
    from cca_zoo_amd import _backend

    n = views[0].shape[0]
    D = sum(v.shape[1] for v in views)
    mom = H.alloc((D * D + D) * 8)
    bufs = [H.to_device(np.ascontiguousarray(v)) for v in views]
    prev = H.k1_route(route)
    try:
        H.moments([(b.ptr, v.shape[1], v.shape[1]) for b, v in zip(bufs, views)], n, _backend.F32, True, mom.ptr)
        taken = H.moments_last_route()[0]
    finally:
        H.k1_route(prev)
    flat = H.to_host(mom, (D * D + D,))
    return flat[: D * D].reshape(D, D), flat[D * D:], taken


def _seed(kind, n):
    return 1000 * (1 + [s[0] for s in SHAPES].index(n)) + 10 * KINDS.index(kind) if n != 32768 else 4000


def _upper_equal(G, Gr):
    iu = np.triu_indices(G.shape[0])
    return np.array_equal(G[iu], Gr[iu])


def _exact_reference(kind, n, dims):
    """Views, pilot and the designed moments in integers, with the host-side validity conditions of an exact comparison."""
    views = E.make_views(kind, n, dims, _seed(kind, n), settle=True)
    assert E.pilot_is_order_robust(views)
    p = E.pilot(views)
    G_int, s_ref, u, window = E.exact_int(views, p)
    assert window < WINDOW_BOUND, np.log2(window)
    return views, G_int, s_ref


def _check_exact(H, monkeypatch, views, G_ref, s_ref, route, tag):
    monkeypatch.setenv("CCZ_SPLIT_ROWS", "256")                      # a workgroup accumulates at most 16 k-steps in float32
    G, s, taken = _moments(H, views, route)
    assert taken == "bf16x2"
    print("K1S exact %-28s rel(G_gpu, G_ref) = %.3e" % (tag, E.rel(G, G_ref)))
    assert np.array_equal(s, s_ref)
    assert _upper_equal(G, G_ref), E.rel(G, G_ref)


@pytest.mark.parametrize("n,dims", SHAPES)
@pytest.mark.parametrize("kind", EXACT)
def test_grid_valued_views_are_exact(H, monkeypatch, kind, n, dims):
    views, G_int, s_ref = _exact_reference(kind, n, dims)
    G_ref, s64 = E.float64_moments(views)
    assert np.array_equal(G_int, G_ref) and np.array_equal(s_ref, s64)         # mid = 0: the designed result IS X'X
    _check_exact(H, monkeypatch, views, G_ref, s_ref, "bf16x2", "%s %d" % (kind, n))


@pytest.mark.parametrize("n,dims", SHAPES)
def test_sparse_integers_through_the_mid_plane_are_exact(H, monkeypatch, n, dims):
    views, G_ref, s_ref = _exact_reference("sparse_int", n, dims)
    G64, _ = E.float64_moments(views)
    off = ~np.eye(G64.shape[0], dtype=bool)
    assert np.any(G_ref[off] != G64[off])                            # the designed result lacks the off-diagonal mid * mid ...
    assert np.array_equal(np.diag(G_ref), np.diag(G64))              # ... and has the diagonal one (sum mid^2)
    _check_exact(H, monkeypatch, views, G_ref, s_ref, "bf16x2", "sparse_int %d" % n)


def test_auto_route_keeps_binary_features_exact(H, monkeypatch):
    """What ``auto`` does to moments the fp32 kernel gets exactly, from 32768 rows on."""
    if os.environ.get("CCZ_K1_ROUTE"):
        pytest.skip("CCZ_K1_ROUTE overrides the automatic choice in this process")
    monkeypatch.setenv("CCZ_SPLIT_MIN_FLOP", "1e9")
    views, G_int, s_ref = _exact_reference("binary", 32768, [256, 256])
    G_ref, _ = E.float64_moments(views)
    assert np.array_equal(G_int, G_ref)
    _check_exact(H, monkeypatch, views, G_ref, s_ref, "auto", "binary 32768 (auto)")


@functools.lru_cache(maxsize=2)
def _faithful_reference(kind, n, dims, rows):
    views = E.make_views(kind, n, list(dims), _seed(kind, n))
    p = E.pilot(views)
    G_emul, s_ref = E.moments(views, p)
    G64, _ = E.float64_moments(views)
    a_ref = E.rel(E.moments_f32_chunks(views, p, rows)[0], G_emul)
    for a in views + [G_emul, G64, s_ref]:
        a.setflags(write=False)
    return views, G_emul, G64, s_ref, a_ref


def _check_faithful(H, kind, n, dims, rows, tag):
    views, G_emul, G64, s_ref, a_ref = _faithful_reference(kind, n, tuple(dims), rows)
    G, s, taken = _moments(H, views, "bf16x2")
    assert taken == "bf16x2"
    e_design, e_gpu, e_total = E.rel(G_emul, G64), E.rel(G, G_emul), E.rel(G, G64)
    print("K1S faithful %-22s rel(G_emul, G64) = %.3e  a_ref = %.3e  rel(G_gpu, G_emul) = %.3e  ratio = %.3f  rel(G_gpu, G64) = %.3e"
          % (tag, e_design, a_ref, e_gpu, e_gpu / a_ref, e_total))
    np.testing.assert_allclose(s, s_ref, rtol=1e-12, atol=1e-7)
    assert e_gpu <= 4.0 * a_ref, (e_gpu, a_ref)
    assert e_total <= e_design + 4.0 * a_ref, (e_total, e_design, a_ref)


@pytest.mark.parametrize("n,dims", SHAPES)
@pytest.mark.parametrize("kind", FAITHFUL)
def test_route_is_faithful_to_its_design(H, monkeypatch, kind, n, dims):
    monkeypatch.setenv("CCZ_SPLIT_ROWS", "256")
    _check_faithful(H, kind, n, dims, 256, "%s %d" % (kind, n))


def test_route_is_faithful_to_its_design_with_long_chunks(H, monkeypatch):
    monkeypatch.delenv("CCZ_SPLIT_ROWS", raising=False)
    n, dims = SHAPES[2]
    _check_faithful(H, "relu", n, dims, 16384, "relu %d (long chunks)" % n)


def test_identical_views_keep_their_canonical_correlations(H):
    """rCCA(c = 0) on [X, X]: the cross-view copy of every diagonal entry lacks sum mid^2, so the route's canonical correlations
    are 1 - O(1e-6), not 1 -- pinned to what the oracle's float64 generalised eigenproblem gives on the emulated moments
    (the reference's own invariant for identical views is 1e-6: cca_zoo tests/linear/test_eigendecomposition.py:330-336)."""
    import torch

    from cca_zoo_amd.linear import rCCA
    from oracle import reference_form as rf

    n, d, k = 32768, 64, 4
    X = np.random.default_rng(64).standard_normal((n, d)).astype(np.float32)
    G_emul, s = E.moments([X, X], E.pilot([X, X]))
    C = (G_emul - np.outer(s, s) / n) / (n - 1)
    A, B = np.zeros_like(C), np.zeros_like(C)
    A[:d, d:], A[d:, :d] = C[:d, d:], C[:d, d:].T
    B[:d, :d], B[d:, d:] = C[:d, :d], C[d:, d:]
    sigma_ref, _ = rf.top_eigenpairs(A, B, k)
    t = torch.from_numpy(X).cuda()
    prev = H.k1_route("bf16x2")
    try:
        model = rCCA(latent_dimensions=k, c=0).fit([t, t.clone()])
        assert H.moments_last_route()[0] == "bf16x2"
    finally:
        H.k1_route(prev)
    sigma = np.asarray(model.singular_values_, dtype=np.float64)
    print("K1S identical views: 1 - sigma_ref =", 1.0 - sigma_ref, " 1 - sigma =", 1.0 - sigma)
    assert np.all(np.abs(sigma - sigma_ref) <= 2.0 * np.abs(1.0 - sigma_ref) + 1e-7), (sigma, sigma_ref)
    assert np.all(np.abs(1.0 - sigma) <= 1e-5), sigma
