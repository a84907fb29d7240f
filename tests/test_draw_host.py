"""CPU tests of the device draws' specification (tests/draw_restatement.py; the kernels are held to it bit for bit in
tests/test_gpu_draw.py) and of what ``draws=`` refuses before a device is touched.

Uniformity is tested on five fixed seeds, every one of which must pass; each chi-square is bounded by its 1 - 1e-6 quantile,
computed here.  The statistics measured when the seeds were fixed (seed: n = 4 orderings, df 23 | n = 64 table, df 3969 |
multiplicities, df 7 | zeros, in standard errors | lag-1 correlation, in standard errors):

    1: 45.2 | 4027.0 | 2.5 | -1.29 | +0.76          2: 24.3 | 3914.9 | 8.2 | +0.17 | -1.29          3: 25.6 | 3813.7 | 7.1 | -0.80 | +0.17
    20261021: 18.1 | 3952.7 | 3.3 | -0.13 | -0.58            0xDEADBEEFCAFEF00D: 15.2 | 3770.6 | 2.5 | -0.85 | -0.02

All five passed on the first run and none was replaced.  The 45.2 of seed 1 (the bound is 70.5) is the 0.4 % point of its
chi-square, the largest of the 25 figures; at 240 000 permutations the same seed gives 26.9.
"""

import os
import re

import numpy as np
import pytest
import scipy.stats

import draw_restatement as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (1, 2, 3, 20261021, 0xDEADBEEFCAFEF00D)
TAIL = 1e-6


def test_splitmix64_by_hand_and_against_the_existing_restatement():
    from oracle.rng import splitmix64 as oracle_splitmix64

    # the first three outputs of the published SplitMix64 from state 0: its state after k steps is k * golden gamma
    gamma = 0x9E3779B97F4A7C15
    inputs = np.array([0, gamma, (2 * gamma) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    want = np.array([0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F], dtype=np.uint64)
    np.testing.assert_array_equal(oracle_splitmix64(inputs), want)
    np.testing.assert_array_equal(dr.splitmix64(inputs), want)
    x = 0
    x = (x + gamma) & 0xFFFFFFFFFFFFFFFF                      # the first one once more, in Python integers
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    assert x ^ (x >> 31) == int(want[0])


def test_stream_is_the_convention_of_the_svi_and_nuts_restatements():
    import vbcca_restatement as vr

    for seed, b, site in ((0, 0, 0), (7, 3, dr.SITE_PERM), (2 ** 64 - 1, 2 ** 40, dr.SITE_BOOT)):
        assert int(dr.stream(seed, b, site)) == vr.stream(seed, b, site)
    got = dr.key(5, np.arange(3)[:, None], dr.SITE_PERM, np.arange(4)[None, :])
    for b in range(3):
        np.testing.assert_array_equal(got[b], dr.key(5, b, dr.SITE_PERM, np.arange(4)))


def test_mulhi_is_the_high_word_of_the_128_bit_product():
    rng = np.random.default_rng(0)
    a = rng.integers(0, 2 ** 64, size=200, dtype=np.uint64)
    a[:3] = [0, 2 ** 64 - 1, 2 ** 32]
    for n in (1, 2, 3, 4096, 70001, 2 ** 31 - 1):
        np.testing.assert_array_equal(dr.mulhi(a, n), np.array([(int(x) * n) >> 64 for x in a], dtype=np.uint64))


def test_header_constants_are_those_of_the_restatement():
    header = open(os.path.join(ROOT, "include", "ccz.h")).read()
    assert int(re.search(r"#define CCZ_DRAW_SITE_PERM (0x[0-9A-Fa-f]+)ull", header).group(1), 16) == dr.SITE_PERM
    assert int(re.search(r"#define CCZ_DRAW_SITE_BOOT (0x[0-9A-Fa-f]+)ull", header).group(1), 16) == dr.SITE_BOOT
    assert dr.SITE_PERM != dr.SITE_BOOT
    rows, cap = (int(re.search(r"#define %s (\d+)" % name, header).group(1)) for name in ("CCZ_DRAW_BUCKET_ROWS", "CCZ_DRAW_SORT_CAP"))
    assert rows < cap          # a bucket's load is rows +- sqrt(rows): the default never reaches the oversize path


@pytest.mark.parametrize("n", [1, 2, 5, 64, 1000, 4097])
def test_permutations_are_permutations_and_counts_sum_to_n(n):
    for seed in SEEDS:
        for b in (0, 1, 77):
            np.testing.assert_array_equal(np.sort(dr.permutation(seed, b, n)), np.arange(n))
            m = dr.counts(seed, b, n)
            assert m.shape == (n,) and m.min() >= 0 and m.sum() == n
    k = dr.key(SEEDS[0], 0, dr.SITE_PERM, np.arange(n))
    assert len(np.unique(k)) == n                            # splitmix64 is a bijection: no two places share a key


def test_streams_differ():
    n, seed = 50, SEEDS[0]
    perms = [tuple(dr.permutation(seed, b, n)) for b in range(20)]
    assert len(set(perms)) == 20
    assert tuple(dr.permutation(seed + 1, 0, n)) != perms[0]
    for b in range(3):
        kp, kb = dr.key(seed, b, dr.SITE_PERM, np.arange(n)), dr.key(seed, b, dr.SITE_BOOT, np.arange(n))
        assert not np.any(kp == kb)
        assert tuple(np.argsort(kb)) != perms[b]
    assert not np.array_equal(dr.counts(seed, 0, n), dr.counts(seed, 1, n))


def _many_permutations(seed, n, B):
    return np.argsort(dr.key(seed, np.arange(B)[:, None], dr.SITE_PERM, np.arange(n)[None, :]), axis=1, kind="stable")


@pytest.mark.parametrize("seed", SEEDS)
def test_all_orderings_of_four_rows_are_equally_likely(seed):
    B = 24000
    perms = _many_permutations(seed, 4, B)
    code = perms @ np.array([64, 16, 4, 1])
    seen = np.unique(code, return_counts=True)[1]
    assert len(seen) == 24
    stat = float(np.sum((seen - B / 24) ** 2 / (B / 24)))
    print(f"seed {seed:#x}: chi-square of the 24 orderings {stat:.1f} (df 23)")
    assert stat <= scipy.stats.chi2.ppf(1 - TAIL, 23)


@pytest.mark.parametrize("seed", SEEDS)
def test_every_value_is_equally_likely_at_every_position(seed):
    """The table O[position, value] of B permutations of n rows has covariance B / (n - 1) times the projector on the
    (n - 1)^2-dimensional space of tables with zero margins (the covariance of a uniform permutation matrix), so
    sum (O - B / n)^2 / (B / n) is n / (n - 1) times a chi-square of (n - 1)^2 degrees of freedom."""
    n, B = 64, 4000
    perms = _many_permutations(seed, n, B)
    table = np.zeros((n, n))
    np.add.at(table, (np.broadcast_to(np.arange(n), perms.shape), perms), 1.0)
    stat = float(np.sum((table - B / n) ** 2 / (B / n))) * (n - 1) / n
    print(f"seed {seed:#x}: chi-square of the position-by-value table {stat:.1f} (df {(n - 1) ** 2})")
    assert stat <= scipy.stats.chi2.ppf(1 - TAIL, (n - 1) ** 2)


@pytest.mark.parametrize("seed", SEEDS)
def test_multiplicities_are_those_of_n_uniform_draws(seed):
    n, B = 4096, 200
    m = np.stack([dr.counts(seed, b, n) for b in range(B)])
    # the histogram of all B n multiplicities against Binomial(n, 1 / n), 7 and more in one cell.  The cells of one resample
    # sum to n, which lowers the variance of the histogram below the independent case: the chi-square bound is on the safe side
    hist = np.bincount(np.minimum(m.ravel(), 7), minlength=8).astype(np.float64)
    pmf = scipy.stats.binom.pmf(np.arange(7), n, 1.0 / n)
    expect = B * n * np.append(pmf, 1.0 - pmf.sum())
    stat = float(np.sum((hist - expect) ** 2 / expect))
    assert stat <= scipy.stats.chi2.ppf(1 - TAIL, 7)
    # rows never drawn: the occupancy problem's exact mean and variance of the number of empty cells
    q1, q2 = (1.0 - 1.0 / n) ** n, (1.0 - 2.0 / n) ** n
    var = n * (n - 1) * q2 + n * q1 - (n * q1) ** 2
    zeros = (m == 0).sum(axis=1)
    z_zero = float((zeros.mean() - n * q1) / np.sqrt(var / B))
    assert abs(z_zero) <= 5.0
    # neighbouring rows are not related: the mean lag-1 correlation of B sequences of n values has standard error 1 / sqrt(B n)
    c = m - m.mean(axis=1, keepdims=True)
    r1 = np.sum(c[:, :-1] * c[:, 1:], axis=1) / np.sum(c * c, axis=1)
    z_lag = float(r1.mean() * np.sqrt(B * n))
    print(f"seed {seed:#x}: multiplicity chi-square {stat:.1f} (df 7), zeros {z_zero:+.2f} se, lag-1 correlation {z_lag:+.2f} se")
    assert abs(z_lag) <= 5.0


# ---- what needs no device ---------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    from cca_zoo_amd import _backend

    def touched(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_backend, "handle_for", touched)
    monkeypatch.setattr(_backend, "default_handle", touched)


@pytest.mark.parametrize("bad", ["gpu", "Device", "", None, 1])
def test_unknown_draws_raise_value_error(no_device, bad):
    from cca_zoo_amd.linear import CCA
    from cca_zoo_amd.model_selection import bootstrap, permutation_test

    X = [np.zeros((20, 3)), np.zeros((20, 4))]
    with pytest.raises(ValueError, match="draws"):
        permutation_test(CCA(), X, n_permutations=5, draws=bad)
    with pytest.raises(ValueError, match="draws"):
        bootstrap(CCA(), X, n_resamples=5, draws=bad)


def test_draws_is_refused_after_the_type_checks_and_is_keyword_only(no_device):
    from cca_zoo_amd.linear import CCA
    from cca_zoo_amd.model_selection import bootstrap, permutation_test

    X = [np.zeros((20, 3)), np.zeros((20, 4))]
    with pytest.raises(TypeError, match="estimator"):
        permutation_test(object(), X, draws="gpu")
    with pytest.raises(TypeError, match="half-precision"):
        bootstrap(CCA(), [np.zeros((20, 3), dtype=np.float16), np.zeros((20, 4))], draws="gpu")
    with pytest.raises(ValueError, match="draws"):          # before the counts and the shapes
        permutation_test(CCA(), X, n_permutations=0, draws="gpu")
    with pytest.raises(TypeError):
        permutation_test(CCA(), X, 5, 0, "device")
    with pytest.raises(TypeError):
        bootstrap(CCA(), X, 5, 0.9, 0, "device")


def test_seed_rule():
    from cca_zoo_amd.model_selection import _resample

    a, b, c = _resample.device_seed(3), _resample.device_seed(3), _resample.device_seed(4)
    assert a == b and a != c and isinstance(a, int) and 0 <= a < 2 ** 64
    assert a == dr.seed_of(3)
    assert _resample.device_seed(np.random.SeedSequence(3)) == a
    assert _resample.device_seed(np.random.default_rng(3)) == a
    assert _resample.device_seed(None) != _resample.device_seed(None)
    assert _resample.DRAWS == ("numpy", "device")
