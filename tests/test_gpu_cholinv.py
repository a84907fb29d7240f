"""GPU tests of ccz_cholinv (csrc/cholinv.hip): batched Cholesky factor + triangular inverse.  By default one
persistent launch serves the whole batch (k_cholinv_chain); the launch-per-link kernels behind CCZ_CHOLINV_CHAIN=0 are
covered by test_gpu_round5.py::test_switches_in_a_child_process.  Reference: numpy.linalg.cholesky / inv in fp64."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from cca_zoo_amd import _backend

    return _backend.default_handle()


def _spd_down(rng, d, cond=1e3):
    """Spectrum 1 down to 1 / cond."""
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    lam = np.geomspace(1.0, 1.0 / cond, d)
    return (q * lam) @ q.T


def _spd_up(rng, d, cond=1e3):
    """Spectrum 1 up to cond."""
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    w = np.exp(np.linspace(0.0, np.log(cond), d))
    return (q * w) @ q.T


def _cholinv(H, mats, want_x=True):
    """[(L, X)] per matrix; L starts as NaN and X as zeros, so untouched entries show."""
    bufs, pa, pl, px = [], [], [], []
    for A in mats:
        d = A.shape[0]
        a, l, x = H.to_device(A), H.to_device(np.full((d, d), np.nan)), H.to_device(np.zeros((d, d)))
        bufs.append((a, l, x))
        pa.append(a.ptr), pl.append(l.ptr), px.append(x.ptr)
    n = len(mats)
    arr = lambda p: (C.c_void_p * n)(*p)
    dd = (C.c_int64 * n)(*[m.shape[0] for m in mats])
    H.check(H.lib.ccz_cholinv(H.raw, n, arr(pa), dd, arr(pl), arr(px) if want_x else None))
    return [(H.to_host(l, A.shape), H.to_host(x, A.shape)) for (a, l, x), A in zip(bufs, mats)]


@pytest.mark.parametrize("d", [1, 5, 63, 64, 65, 128, 200, 512, 1000])
def test_cholinv_single(H, d):
    rng = np.random.default_rng(d)
    A = _spd_down(rng, d)
    (L, X), = _cholinv(H, [A])
    Lr = np.linalg.cholesky(A)
    assert np.abs(np.tril(L) - Lr).max() < 1e-11 * np.abs(Lr).max()
    assert np.all(np.isnan(L[np.triu_indices(d, 1)]))            # strictly-upper part untouched
    Xl = np.tril(X)
    assert np.abs(Xl @ Lr - np.eye(d)).max() < 1e-9
    # blocks strictly above the block diagonal were left at the zeros we put there
    for bi in range(0, d, 64):
        assert np.all(X[bi:bi + 64, bi + 64:] == 0.0)


def test_cholinv_batched_mixed_sizes_and_failure(H):
    rng = np.random.default_rng(7)
    mats = [_spd_down(rng, d, 1e4) for d in (512, 70, 512, 1, 333, 64, 129, 200)]
    for (L, X), A in zip(_cholinv(H, mats), mats):
        Lr = np.linalg.cholesky(A)
        assert np.abs(np.tril(L) - Lr).max() < 1e-10 * np.abs(Lr).max()
        assert np.abs(np.tril(X) @ Lr - np.eye(A.shape[0])).max() < 1e-8
    # factor only
    (L, X), = _cholinv(H, [mats[0]], want_x=False)
    assert np.abs(np.tril(L) - np.linalg.cholesky(mats[0])).max() < 1e-10 and np.all(X == 0.0)
    # an indefinite matrix is reported, with the others in the batch unaffected up to that point
    bad = mats[4].copy()
    bad[150, 150] = -1.0
    with pytest.raises(np.linalg.LinAlgError, match="not positive definite"):
        _cholinv(H, [mats[1], bad])


# ---------------------------------------------------------------------------------------------
# the chain kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 65, 127, 128, 192, 448, 512, 513, 1024, 1500, 2048])
def test_chain_single_matrix(H, d):
    rng = np.random.default_rng(1000 + d)
    A = _spd_up(rng, d, 1e5)
    (L, X), = _cholinv(H, [A])
    Lr = np.linalg.cholesky(A)
    assert np.abs(np.tril(L) - Lr).max() < 2e-11 * np.abs(Lr).max()
    assert np.all(np.isnan(L[np.triu_indices(d, 1)]))            # strictly-upper part untouched
    Xr = np.linalg.inv(Lr)
    assert np.abs(np.tril(X) - Xr).max() < 1e-9 * np.abs(Xr).max()
    for bi in range(0, d, 64):                                    # blocks above the block diagonal: left alone
        assert np.all(X[bi:bi + 64, bi + 64:] == 0.0)


def test_chain_repeated_launches_leave_the_sync_block_clean(H):
    """The last workgroup of a launch clears the progress counters: twenty launches in a row (different shapes in
    between) must all be right."""
    rng = np.random.default_rng(5)
    for it in range(20):
        ds = [512, 512] if it % 3 else [200, 64, 700]
        mats = [_spd_up(rng, d, 1e4) for d in ds]
        for (L, X), A in zip(_cholinv(H, mats), mats):
            Lr = np.linalg.cholesky(A)
            assert np.abs(np.tril(L) - Lr).max() < 1e-10 * np.abs(Lr).max()
            assert np.abs(np.tril(X) @ Lr - np.eye(A.shape[0])).max() < 1e-8


def test_chain_eight_matrices_and_failure(H):
    rng = np.random.default_rng(9)
    mats = [_spd_up(rng, d, 1e4) for d in (512, 512, 512, 512, 333, 512, 129, 512)]
    for (L, X), A in zip(_cholinv(H, mats), mats):
        Lr = np.linalg.cholesky(A)
        assert np.abs(np.tril(L) - Lr).max() < 1e-10 * np.abs(Lr).max()
        assert np.abs(np.tril(X) @ Lr - np.eye(A.shape[0])).max() < 1e-8
    (L, X), = _cholinv(H, [mats[0]], want_x=False)
    assert np.abs(np.tril(L) - np.linalg.cholesky(mats[0])).max() < 1e-10 and np.all(X == 0.0)
    bad = mats[4].copy()
    bad[150, 150] = -1.0
    with pytest.raises(np.linalg.LinAlgError, match="not positive definite"):
        _cholinv(H, [mats[1], bad])
    # ... and the launch after a failed one is clean again
    (L, X), = _cholinv(H, [mats[6]])
    assert np.abs(np.tril(L) - np.linalg.cholesky(mats[6])).max() < 1e-10
