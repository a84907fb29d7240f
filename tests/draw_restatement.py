"""The specification of the device draws (``include/ccz.h``: ``ccz_draw_permutations`` / ``ccz_draw_counts``, ``csrc/draw.hip``) in
NumPy ``uint64`` (imported by tests/test_draw_host.py and tests/test_gpu_draw.py).  All arithmetic wraps at 64 bits:

    stream(seed, b, site) = splitmix64(splitmix64(splitmix64(seed) + b) + site)
    key(seed, b, site, j) = splitmix64(stream(seed, b, site) ^ splitmix64(j))
    permutation(seed, b, n) = argsort_j key(seed, b, SITE_PERM, j)                  (the keys of a stream are distinct)
    counts(seed, b, n)[s]   = #{j < n : (key(seed, b, SITE_BOOT, j) * n) >> 64 = s}

``seed_of(random_state)`` is the public functions' rule for the seed.
"""

import numpy as np

SITE_PERM = 0x5045524D      # CCZ_DRAW_SITE_PERM
SITE_BOOT = 0x424F4F54      # CCZ_DRAW_SITE_BOOT
M32 = np.uint64(0xFFFFFFFF)


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def stream(seed, b, site):
    """``b``: one index or an array of them (the result has its shape)."""
    with np.errstate(over="ignore"):
        s = splitmix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)) + np.asarray(b, dtype=np.uint64)
        return splitmix64(splitmix64(s) + np.uint64(int(site)))


def key(seed, b, site, j):
    """The keys of the places ``j`` (any integer array) of stream ``(seed, b, site)``; arrays ``b`` and ``j`` broadcast."""
    return splitmix64(stream(seed, b, site) ^ splitmix64(np.asarray(j, dtype=np.uint64)))


def mulhi(a, n):
    """``(a * n) >> 64`` for a ``uint64`` array ``a`` and an integer ``0 < n < 2^32``, from 32-bit halves: with
    ``a = hi 2^32 + lo``, ``a n = (hi n) 2^32 + lo n`` and both products are below 2^64."""
    n = int(n)
    assert 0 < n < 2 ** 32
    a = np.asarray(a, dtype=np.uint64)
    hi, lo = a >> np.uint64(32), a & M32
    return (hi * np.uint64(n) + ((lo * np.uint64(n)) >> np.uint64(32))) >> np.uint64(32)   # < 2^64: hi n <= (2^32 - 1)^2, the carry < 2^32


def permutation(seed, b, n):
    """``pi[rank] = j``: the places 0 .. n - 1 in ascending order of their keys (int64)."""
    return np.argsort(key(seed, b, SITE_PERM, np.arange(n)), kind="stable")


def indices(seed, b, n):
    """The ``n`` rows that resample ``b`` draws, in the order of the draws (int64)."""
    return mulhi(key(seed, b, SITE_BOOT, np.arange(n)), n).astype(np.int64)


def counts(seed, b, n):
    """The multiplicity vector of resample ``b`` (int64, sums to ``n``)."""
    return np.bincount(indices(seed, b, n), minlength=n)


def seed_of(random_state):
    return int(np.random.default_rng(random_state).integers(0, 2 ** 64, dtype=np.uint64))
