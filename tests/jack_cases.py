"""Inputs and float64 references of the jackknife tests (tests/test_jack_host.py on the CPU, tests/test_gpu_jack.py on the device).
Pure NumPy, not a test.  The views are ``planted_views`` of tests/test_gpu_boot.py with its seed rule ``1000 + n + p1``; the bars
and the conditions they rest on (``cond(R_i) <= 1e4``, every compared ``sigma_j`` at least ``5e-3 sigma_1`` from its neighbours) are
that module's, imported.  The conditions are a requirement on the inputs: tests/test_jack_host.py asserts them on ``subset(J)``
of every case, at most SUBSET evenly spaced replicates (the literal refit of every replicate of (2000, 64, 64) takes most of a
minute).
"""

import functools

import numpy as np

import boot_restatement as br
import jack_restatement as jr
import test_gpu_boot as tb

SUBSET = 25

# (n, p1, p2), c, center, J
CASES = [
    ((60, 5, 3), 0.0, True, 60),
    ((60, 5, 3), 0.0, True, 7),                          # groups of 9 and 8
    ((300, 64, 1), 0.0, True, 300),
    ((1000, 17, 64), (0.1, 0.3), True, 1000),
    ((1000, 17, 64), 0.0, True, 33),
    ((2000, 64, 64), 0.2, False, 128),
    ((2000, 64, 64), 0.0, True, 2000),
    ((4101, 16, 16), 0.0, True, 4101),                   # two row splits
    ((4101, 16, 16), 0.0, True, 2),                      # groups of 2051 and 2050
]
assert CASES[7][0][0] == 4096 + 5                        # ROWS_PER_SPLIT + 5 (asserted against the package in test_jack_host.py)

GROUPS_CASE = ((41920, 5, 3), 0.0, True, 41920)          # leave-one-out past the 41890 replicates of one launch group


def subset(J):
    """At most SUBSET evenly spaced replicates of ``J``, the first and the last among them."""
    return np.unique(np.round(np.linspace(0, J - 1, min(J, SUBSET))).astype(np.int64))


def views(shape):
    n, p1, p2 = shape
    return tb.planted_views(n, p1, p2, seed=1000 + n + p1)


def ridge(c):
    return list(c) if isinstance(c, tuple) else c


@functools.lru_cache(maxsize=None)
def case(shape, c, center, J):
    """``X1, X2, replicates, refs, ident, k``: the literal refits (``br.fit_rows`` on the rows kept) of ``subset(J)``."""
    X1, X2 = views(shape)
    k = min(shape[1], shape[2], 2)
    reps = subset(J)
    refs = [jr.fit_without(X1, X2, np.arange(g, shape[0], J), ridge(c), center, k) for g in reps]   # group g of jr.groups(n, J)
    ident = br.fit_rows(X1, X2, ridge(c), center, k)
    return X1, X2, reps, refs, ident, k


def loo_counts(n, J, replicates):
    """The 0/1 multiplicities of the replicates: ``counts[i, s] = (s % J != replicates[i])`` (int32)."""
    s = np.arange(n, dtype=np.int64) % J
    return (s[None, :] != np.asarray(replicates, dtype=np.int64)[:, None]).astype(np.int32)


def downdated_fit(X1, X2, g, J, c, center, k):
    """The device's route in NumPy: the moments of all rows (of the views shifted by their full-sample means when centring)
    minus those of group ``g``, into the solve of tests/boot_restatement.py."""
    c1, c2 = br.per_view(c)
    p1, p2 = X1.shape[1], X2.shape[1]
    X = np.hstack([X1 - X1.mean(axis=0), X2 - X2.mean(axis=0)]) if center else np.hstack([X1, X2])
    D = X[g::J]
    N = X.shape[0] - D.shape[0]
    G, s = X.T @ X - D.T @ D, X.sum(axis=0) - D.sum(axis=0)
    Cm = (G - np.outer(s, s) / N if center else G) / (N - 1)
    R1 = (1 - c1) * Cm[:p1, :p1] + c1 * np.eye(p1)
    R2 = (1 - c2) * Cm[p1:, p1:] + c2 * np.eye(p2)
    L1, L2 = np.linalg.cholesky(R1), np.linalg.cholesky(R2)
    T = np.linalg.solve(L1, Cm[:p1, p1:]) @ np.linalg.inv(L2).T
    U, S, Vt = np.linalg.svd(T, full_matrices=False)
    return br.SimpleNamespace(sv=S, weights=[np.linalg.solve(L1.T, U[:, :k]), np.linalg.solve(L2.T, Vt[:k].T)])
