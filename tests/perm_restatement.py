"""The specification of ``cca_zoo_amd.model_selection.permutation_test`` in float64 NumPy (imported by tests/test_perm_host.py
and tests/test_gpu_perm.py).

    R_i = (1 - c_i) C_ii + c_i I = L_i L_i',   Z_i = (X_i - 1 mu_i') L_i^-T,   sv(pi) = svd(Z_1' Z_2[pi] / (n - 1))

with ``C_ii`` the covariance (``center=False``: the uncentred second moment over ``n - 1``, ``mu_i = 0``, as ``rCCA`` does).
Permutation ``b`` is the ``b``-th ``np.random.default_rng(random_state).permutation(n)``.
"""

from types import SimpleNamespace

import numpy as np
import scipy.linalg


def per_view(c):
    return list(c) if isinstance(c, (list, tuple)) else [c, c]


def whiten(X, c, center=True):
    """``(X - 1 mu') L^-T`` with ``L`` the Cholesky factor of ``(1 - c) C + c I``."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    Xc = X - X.mean(axis=0) if center else X
    R = (1.0 - c) * (Xc.T @ Xc) / (n - 1) + c * np.eye(d)
    L = np.linalg.cholesky(R)
    return scipy.linalg.solve_triangular(L, Xc.T, lower=True).T


def singular_values(Z1, Z2, perm=None):
    n = Z1.shape[0]
    Zp = Z2 if perm is None else Z2[perm]
    return np.linalg.svd(Z1.T @ Zp / (n - 1), compute_uv=False)


def tails(sv):
    sq = np.asarray(sv, dtype=np.float64) ** 2
    return np.cumsum(sq[..., ::-1], axis=-1)[..., ::-1]


def count_pvalues(statistic, null):
    B = null.shape[0]
    return np.array([(1 + sum(1 for b in range(B) if null[b, j] >= statistic[j])) / (B + 1) for j in range(len(statistic))])


def restate(views, c=0.0, center=True, n_permutations=1000, random_state=None, perms=None):
    """Everything ``permutation_test`` returns but the estimator.  ``perms`` (B x n) replaces the drawn permutations."""
    X1, X2 = (np.asarray(v, dtype=np.float64) for v in views)
    c1, c2 = per_view(c)
    Z1, Z2 = whiten(X1, c1, center), whiten(X2, c2, center)
    n = X1.shape[0]
    if perms is None:
        rng = np.random.default_rng(random_state)
        perms = [rng.permutation(n) for _ in range(n_permutations)]
    statistic = singular_values(Z1, Z2)
    null = np.stack([singular_values(Z1, Z2, np.asarray(pi)) for pi in perms])
    tail, tail_null = tails(statistic), tails(null)
    return SimpleNamespace(statistic=statistic, null=null, pvalues=count_pvalues(statistic, null), tail=tail, tail_null=tail_null,
                           tail_pvalues=count_pvalues(tail, tail_null), perms=np.asarray(perms), Z=(Z1, Z2))
