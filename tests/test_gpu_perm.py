"""``ccz_perm_singular_values`` and ``permutation_test`` on the device against tests/perm_restatement.py (float64 NumPy).

The bar is the family's device bar, 1e-8, absolute on ``sigma / sigma_1``.  Conditioning is a condition of the inputs, not a
measurement: every reference singular value compared is asserted to be at least ``1e-3 sigma_1``.  The singular values of a
fully permuted SQUARE problem have a hard edge at zero (3 - 5 % of all permutations of the (16, 16) and (64, 64) shapes
fall below that ratio), so no seed gives 300 such permutations in a row: the permutations of a case are the first ones of
one fixed ``rng.permutation`` stream whose reference meets the condition (with a factor 2 to spare) -- inputs chosen on the
NumPy side, every one of them compared, none left out.  Each test prints the worst error it measured; on an MI355X: kernels
2.3e-14 (n = 130, (64, 64), the batch of 300), public function 2.2e-15, null rows against refits 2.1e-15.
"""

import ctypes as C
import functools

import numpy as np
import pytest

import perm_restatement as pr

pytestmark = pytest.mark.gpu

BAR = 1e-8
COND = 1e-3
NBATCH = 300


def _rows_per_split():
    from cca_zoo_amd.model_selection import _permutation as pm

    return pm.ROWS_PER_SPLIT


def _shapes():
    return [(37, 5, 3), (130, 64, 64), (131, 17, 64), (131, 64, 1), (_rows_per_split() + 5, 16, 16)]


def _handle():
    from cca_zoo_amd import _backend

    return _backend.default_handle(0)


def whitened_pair(n, p1, p2, seed, noise=0.3):
    """Planted low-rank plus noise, centred, columns orthonormalised (``Z' Z / (n - 1) = I``)."""
    rng = np.random.default_rng(seed)
    k = min(p1, p2, 3)
    z = rng.standard_normal((n, k))
    out = []
    for p in (p1, p2):
        X = z @ rng.standard_normal((k, p)) + noise * rng.standard_normal((n, p))
        q, _ = np.linalg.qr(X - X.mean(axis=0))
        out.append(np.ascontiguousarray(q * np.sqrt(n - 1)))
    return out


@functools.lru_cache(maxsize=None)
def case(n, p1, p2):
    """Inputs and NumPy reference of one shape, computed once: Z_1, Z_2, the identity's values, NBATCH permutations (int32) whose
    references meet the conditioning bar, and those references."""
    Z1, Z2 = whitened_pair(n, p1, p2, seed=1000 + n + p1)
    rng = np.random.default_rng(n + p2)
    perms, refs, drawn = [], [], 0
    while len(perms) < NBATCH:
        pi = rng.permutation(n)
        drawn += 1
        assert drawn <= 2 * NBATCH, "the generator does not give conditioned problems"
        s = pr.singular_values(Z1, Z2, pi)
        if s[-1] >= 2 * COND * s[0]:
            perms.append(pi.astype(np.int32))
            refs.append(s)
    for a in (Z1, Z2):
        a.setflags(write=False)
    perms, refs = np.stack(perms), np.stack(refs)
    perms.setflags(write=False), refs.setflags(write=False)
    return Z1, Z2, pr.singular_values(Z1, Z2), perms, refs


class Device:
    """Z_1, Z_2 of one shape in HBM and calls of the entry point on them."""

    def __init__(self, n, p1, p2):
        self.h = _handle()
        self.n, self.p1, self.p2, self.r = n, p1, p2, min(p1, p2)
        Z1, Z2 = case(n, p1, p2)[:2]
        self.z1, self.z2 = self.h.to_device(Z1), self.h.to_device(Z2)

    def run(self, perms):
        """Singular values (nperm x r) of ``perms`` (nperm x n int32, or None = the identity) in ONE call."""
        h, vp = self.h, C.c_void_p
        nperm = 1 if perms is None else int(perms.shape[0])
        pd = None if perms is None else h.to_device(np.ascontiguousarray(perms, dtype=np.int32))
        sv = h.to_device(np.full((nperm, self.r), np.nan))
        h.check(h.lib.ccz_perm_singular_values(h.raw, self.n, self.p1, self.p2, vp(self.z1.ptr), vp(self.z2.ptr),
                                               vp(pd.ptr) if pd is not None else None, nperm, 1.0 / (self.n - 1), vp(sv.ptr)))
        return h.to_host(sv, (nperm, self.r))


def worst_error(got, ref):
    ref = np.atleast_2d(ref)
    assert np.all(ref[:, -1] >= COND * ref[:, 0]), "broken test: a reference singular value is below 1e-3 sigma_1"
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    assert np.all(np.diff(got, axis=1) <= 0)                # descending
    return float(np.max(np.abs(got - ref) / ref[:, :1]))


@pytest.mark.parametrize("n,p1,p2", _shapes())
def test_kernels_match_numpy(n, p1, p2):
    Z1, Z2, ident, perms, refs = case(n, p1, p2)
    dev = Device(n, p1, p2)
    errs = {"identity": worst_error(dev.run(None), ident),
            "one": worst_error(dev.run(perms[:1]), refs[:1]),
            "batch": worst_error(dev.run(perms), refs)}
    print(f"perm kernels n={n} ({p1}, {p2}): worst |sigma - ref| / sigma_1 = {errs}")
    assert max(errs.values()) <= BAR, errs


@pytest.mark.parametrize("n,p1,p2", _shapes())
def test_bit_identity(n, p1, p2):
    perms = case(n, p1, p2)[3]
    dev = Device(n, p1, p2)
    whole = dev.run(perms)
    np.testing.assert_array_equal(dev.run(perms), whole)                                           # the same call twice
    by64 = np.concatenate([dev.run(perms[b:b + 64]) for b in range(0, NBATCH, 64)])
    np.testing.assert_array_equal(by64, whole)
    by1 = np.concatenate([dev.run(perms[b:b + 1]) for b in range(NBATCH)])                         # permutation b alone
    np.testing.assert_array_equal(by1, whole)
    ident = np.arange(n, dtype=np.int32)[None, :]
    np.testing.assert_array_equal(dev.run(ident), dev.run(None))                                   # NULL is the identity


def test_entry_point_refuses_shapes_outside_the_limits():
    dev = Device(37, 5, 3)
    h, vp = dev.h, C.c_void_p
    f = h.lib.ccz_perm_singular_values
    ok = (vp(dev.z1.ptr), vp(dev.z2.ptr))
    sv = h.alloc(64 * 8)
    assert f(h.raw, 37, 65, 3, *ok, None, 1, 1.0, vp(sv.ptr)) == -6          # CCZ_EUNSUP
    assert f(h.raw, 2 ** 31, 5, 3, *ok, None, 1, 1.0, vp(sv.ptr)) == -6
    assert f(h.raw, 37, 5, 3, *ok, None, 2, 1.0, vp(sv.ptr)) == -1           # CCZ_EINVAL: the identity is one permutation
    assert f(h.raw, 37, 5, 0, *ok, None, 1, 1.0, vp(sv.ptr)) == -1
    assert f(h.raw, 37, 5, 3, *ok, None, 0, 1.0, vp(sv.ptr)) == -1
    assert f(h.raw, 37, 5, 3, None, vp(dev.z2.ptr), None, 1, 1.0, vp(sv.ptr)) == -1


# ---- the public function --------------------------------------------------------------------------------------------------
PUB_N, PUB_P, PUB_B, PUB_SEED = 70, (12, 7), 50, 3
ESTIMATORS = {
    "cca": (lambda ld: _linear().CCA(latent_dimensions=ld), 0.0, True),
    "rcca": (lambda ld: _linear().rCCA(latent_dimensions=ld, c=[0.1, 0.3]), [0.1, 0.3], True),
    "pls": (lambda ld: _linear().PLS(latent_dimensions=ld), 1.0, True),
    "uncentred": (lambda ld: _linear().rCCA(latent_dimensions=ld, c=0.2, center=False), 0.2, False),
}


def _linear():
    import cca_zoo_amd.linear as lin

    return lin


@functools.lru_cache(maxsize=None)
def public_views(dtype):
    rng = np.random.default_rng(21)
    z = rng.standard_normal((PUB_N, 2))
    views = [z @ rng.standard_normal((2, p)) + rng.standard_normal((PUB_N, p)) + rng.standard_normal(p) for p in PUB_P]
    views = [np.ascontiguousarray(v, dtype=dtype) for v in views]
    for v in views:
        v.setflags(write=False)
    return views


@functools.lru_cache(maxsize=None)
def public_reference(name, dtype):
    _, c, center = ESTIMATORS[name]
    ref = pr.restate(public_views(dtype), c=c, center=center, n_permutations=PUB_B, random_state=PUB_SEED)    # float32: widened first
    # the p-values are counts: no compared pair may lie within 1e-6 of a tie
    assert np.min(np.abs(ref.null - ref.statistic[None, :])) > 1e-6
    assert np.min(np.abs(ref.tail_null - ref.tail[None, :])) > 1e-6
    assert np.all(ref.null[:, -1] >= COND * ref.null[:, 0]) and ref.statistic[-1] >= COND * ref.statistic[0]
    return ref


@pytest.mark.parametrize("where", ["host", "cuda"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(ESTIMATORS))
def test_permutation_test_matches_restatement(name, dtype, where):
    import torch

    from cca_zoo_amd.model_selection import permutation_test

    k = 3
    ref = public_reference(name, dtype)
    views = [np.array(v) for v in public_views(dtype)]
    if where == "cuda":
        views = [torch.tensor(v, device="cuda") for v in views]
    est = ESTIMATORS[name][0](k)
    res = permutation_test(est, views, n_permutations=PUB_B, random_state=PUB_SEED)
    assert not hasattr(est, "weights_")
    assert res.statistic.shape == (7,) and res.null.shape == (PUB_B, 7) and res.tail_null.shape == (PUB_B, 7)
    e_stat = float(np.max(np.abs(res.statistic - ref.statistic)) / ref.statistic[0])
    e_null = float(np.max(np.abs(res.null - ref.null) / ref.null[:, :1]))
    sv_fit = np.asarray(res.estimator.singular_values_, dtype=np.float64)
    e_fit = float(np.max(np.abs(sv_fit[:k] - res.statistic[:k])) / res.statistic[0])
    print(f"permutation_test {name} {np.dtype(dtype).name} {where}: statistic {e_stat:.3g}, null {e_null:.3g}, fitted estimator {e_fit:.3g}")
    assert e_stat <= BAR and e_null <= BAR
    np.testing.assert_array_equal(res.pvalues, ref.pvalues)
    np.testing.assert_array_equal(res.tail_pvalues, ref.tail_pvalues)
    np.testing.assert_allclose(res.tail, ref.tail, rtol=0, atol=4 * BAR * ref.tail[0])
    assert sv_fit.shape == (k,) and len(res.estimator.weights_) == 2
    # the ordinary fit of float32 views runs K1 on the float32 matrix pipe (unit roundoff 6e-8): the bar applies to float64 views
    assert e_fit <= (BAR if dtype == np.float64 else 1e-5)


def test_chunk_length_does_not_change_a_bit(monkeypatch):
    from cca_zoo_amd.linear import rCCA
    from cca_zoo_amd.model_selection import _permutation as pm
    from cca_zoo_amd.model_selection import permutation_test

    views = [np.array(v) for v in public_views(np.float64)]
    base = permutation_test(rCCA(c=[0.1, 0.3]), views, n_permutations=PUB_B, random_state=PUB_SEED)
    for chunk in (1, 7, PUB_B):
        monkeypatch.setattr(pm, "CHUNK_PERMS", chunk)
        res = permutation_test(rCCA(c=[0.1, 0.3]), views, n_permutations=PUB_B, random_state=PUB_SEED)
        np.testing.assert_array_equal(res.null, base.null)
        np.testing.assert_array_equal(res.statistic, base.statistic)


@pytest.mark.parametrize("name", ["cca", "rcca"])
def test_null_rows_equal_refits_by_the_existing_solver(name):
    """A different route to the same numbers, by code that predates the permutation test: refit on [X1, X2[pi]]."""
    from cca_zoo_amd.model_selection import permutation_test

    views = [np.array(v) for v in public_views(np.float64)]
    res = permutation_test(ESTIMATORS[name][0](1), views, n_permutations=5, random_state=PUB_SEED)
    rng = np.random.default_rng(PUB_SEED)
    worst = 0.0
    for b in range(5):
        pi = rng.permutation(PUB_N)
        sv = ESTIMATORS[name][0](7).fit([views[0], views[1][pi]]).singular_values_
        assert res.null[b, -1] >= COND * res.null[b, 0]
        worst = max(worst, float(np.max(np.abs(sv - res.null[b])) / res.null[b, 0]))
    print(f"permutation_test {name} against refits: {worst:.3g}")
    assert worst <= BAR


def test_planted_and_independent_views():
    from cca_zoo_amd.linear import CCA
    from cca_zoo_amd.model_selection import permutation_test

    rng = np.random.default_rng(8)
    n = 200
    z = rng.standard_normal((n, 1))
    planted = [z @ rng.standard_normal((1, 6)) + rng.standard_normal((n, 6)), z @ rng.standard_normal((1, 4)) + rng.standard_normal((n, 4))]
    res = permutation_test(CCA(), planted, n_permutations=99, random_state=0)
    assert res.pvalues[0] == 0.01 and res.tail_pvalues[0] == 0.01
    independent = [rng.standard_normal((n, 6)), rng.standard_normal((n, 4))]
    ref = pr.restate(independent, c=0.0, n_permutations=99, random_state=0)
    assert np.min(np.abs(ref.null - ref.statistic[None, :])) > 1e-6
    res = permutation_test(CCA(), independent, n_permutations=99, random_state=0)
    np.testing.assert_array_equal(res.pvalues, ref.pvalues)
    assert res.pvalues[0] == ref.pvalues[0]
