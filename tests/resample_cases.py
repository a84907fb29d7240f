"""Inputs and float64 references for the paths of the resampling core (csrc/resample_dev.h, perm.hip, boot.hip) that the five
shapes of tests/test_gpu_perm.py and tests/test_gpu_boot.py leave out: every tile layout, bootstrap at full ``k``, counts that
skip chunks, calls of more than one launch group, and matrices that show what the one-sided Jacobi promises.  Pure NumPy, not a
test: tests/test_resample_cases_host.py asserts on the CPU every condition stated here, tests/test_gpu_resample_core.py runs the
device on these inputs.  The generators, bars and conditions are those of the two GPU modules, imported, not restated.
"""

import functools
import os

import numpy as np

import boot_restatement as br
import perm_restatement as pr
import test_gpu_boot as tb
import test_gpu_perm as tp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_graded.npz")

WIDTHS = (9, 24, 40, 57)                                # 1, 2, 3 and 4 tiles of 16, each with a ragged last tile
PERM_SWEEP_N, BOOT_SWEEP_N = 131, 600                   # 131 = four chunks of 32 and a 3-row tail
SWEEP_PERMS, SWEEP_BOOT = 64, 24
# (n, p1, p2), k: two full passes of the back substitution; a second pass of two jobs either way round; 17 of 64; exactly one pass
FULL_K = [((2000, 64, 64), 64), ((600, 40, 33), 33), ((500, 33, 48), 33), ((1000, 17, 64), 17), ((700, 48, 48), 32)]
FULL_K_BOOT = 20


def rows_per_split():
    return tp._rows_per_split()


def perm_sweep_shapes():
    """All of WIDTHS x WIDTHS but (9, 9): there the identity's smallest value is below COND, and (1, 1) tiles are covered."""
    return [(PERM_SWEEP_N, p1, p2) for p1 in WIDTHS for p2 in WIDTHS if (p1, p2) != (9, 9)]


def boot_sweep_shapes():
    return [(BOOT_SWEEP_N, p1, p2) for p1 in WIDTHS for p2 in WIDTHS]


def perm_row_shapes():
    """Exactly one split, three splits, and fewer rows than one staged chunk."""
    R = rows_per_split()
    return [(R, 24, 40), (2 * R + 1, 24, 40), (6, 3, 2)]


def boot_row_cases():
    """(shape, c): as perm_row_shapes; 7 rows repeat within a resample, so that case carries a ridge."""
    R = rows_per_split()
    return [((R, 24, 40), 0.0), ((2 * R + 1, 24, 40), 0.0), ((7, 3, 2), 0.5)]


# ---- bootstrap cases ------------------------------------------------------------------------------------------------------
def draw_counts(rng, n, count):
    return np.stack([np.bincount(rng.integers(0, n, size=n), minlength=n) for _ in range(count)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def boot_case(shape, c=0.0, nboot=SWEEP_BOOT, k=None):
    """The first ``nboot`` resamples of ``tb.case(shape, c, True, False)`` -- its views, its draw stream -- at the cost of
    ``nboot`` refits, not NBOOT; ``k``: the weight columns (default: that case's).  The gaps are asserted for the columns that
    are compared one by one, the first two."""
    n, p1, p2 = shape
    X1, X2 = tb.planted_views(n, p1, p2, seed=1000 + n + p1)
    counts = draw_counts(np.random.default_rng(n + p2), n, nboot)
    k = min(p1, p2, 2) if k is None else k
    refs = [br.fit_counts(X1, X2, m, c, True, k) for m in counts]
    ident = br.fit_rows(X1, X2, c, True, k)
    for f in refs + [ident]:
        tb.assert_conditions(f, min(k, 2))
    counts.setflags(write=False)
    return X1, X2, counts, refs, ident, k


def resample_moments(X1, X2, m):
    """R_1, R_2, C_12 (c = 0, centred) of the resample with multiplicities ``m``, from its repeated rows."""
    rows = np.repeat(np.arange(len(m)), np.asarray(m, dtype=np.int64))
    A, B = np.asarray(X1)[rows], np.asarray(X2)[rows]
    A, B = A - A.mean(axis=0), B - B.mean(axis=0)
    d = len(rows) - 1
    return A.T @ A / d, B.T @ B / d, A.T @ B / d


def identity_residuals(X1, X2, m, sv, W1, W2):
    """max |W_1' R_1 W_1 - I|, max |W_2' R_2 W_2 - I|, max |W_1' C_12 W_2 - diag(sv[:k])|: what the weights of a CCA fit
    satisfy whatever the spectral gaps are."""
    R1, R2, C12 = resample_moments(X1, X2, m)
    k = W1.shape[1]
    eye = np.eye(k)
    return (float(np.max(np.abs(W1.T @ R1 @ W1 - eye))), float(np.max(np.abs(W2.T @ R2 @ W2 - eye))),
            float(np.max(np.abs(W1.T @ C12 @ W2 - np.diag(np.asarray(sv)[:k])))))


@functools.lru_cache(maxsize=None)
def skip_case():
    """(shape, X1, X2, counts, refs, k): three splits; 8 resamples drawn only from the rows outside [64, 200) and outside the
    whole second split, two of them with 50 added to five multiplicities (N_b != n there)."""
    R = rows_per_split()
    n, p1, p2 = shape = (2 * R + 5, 24, 40)
    X1, X2 = tb.planted_views(n, p1, p2, seed=1000 + n + p1)
    allowed = np.concatenate([np.arange(0, 64), np.arange(200, R), np.arange(2 * R, n)])
    rng = np.random.default_rng(n + p2)
    counts = np.stack([np.bincount(allowed[rng.integers(0, len(allowed), size=n)], minlength=n) for _ in range(8)]).astype(np.int32)
    for b in (2, 5):
        counts[b, rng.choice(allowed, size=5, replace=False)] += 50
    k = 2
    refs = [br.fit_counts(X1, X2, m, 0.0, True, k) for m in counts]
    for f in refs:
        tb.assert_conditions(f, k)
    counts.setflags(write=False)
    return shape, X1, X2, counts, refs, k


def zero_chunks(counts):
    """Per resample, how many aligned chunks of 32 rows hold no drawn row (a split starts at a multiple of 32)."""
    n = counts.shape[1]
    return np.array([sum(1 for s in range(0, n, 32) if not m[s:s + 32].any()) for m in counts])


# ---- calls of more than one launch group ----------------------------------------------------------------------------------
def conditioned_perms(Z1, Z2, rng, count):
    """``count`` fresh permutations whose reference meets the conditioning bar as ``tp.case`` asks it, and those references."""
    n = Z1.shape[0]
    perms, refs, drawn = [], [], 0
    while len(perms) < count:
        pi = rng.permutation(n)
        drawn += 1
        assert drawn <= 2 * count + 20, "the generator does not give conditioned problems"
        s = pr.singular_values(Z1, Z2, pi)
        if s[-1] >= 2 * tp.COND * s[0]:
            perms.append(pi.astype(np.int32))
            refs.append(s)
    return np.stack(perms), np.stack(refs)


def perm_group_case(shape, cap, ntail):
    """``cap + ntail`` permutations: the first ``cap`` tile the case's own NBATCH, the tail is fresh.  Returns them and the
    tail's references."""
    Z1, Z2, _, perms, _ = tp.case(*shape)
    tail, refs = conditioned_perms(Z1, Z2, np.random.default_rng(77 + shape[0]), ntail)
    return np.concatenate([perms[np.arange(cap) % len(perms)], tail]), refs


def boot_group_case(shape, cap, ntail, nbase=SWEEP_BOOT):
    """(X1, X2, counts, nbase, tail references, k): ``cap + ntail`` resamples, the first ``cap`` tiling ``boot_case``'s
    ``nbase``, the tail fresh."""
    n, p1, p2 = shape
    X1, X2, base, _, _, k = boot_case(shape, 0.0, nbase)
    tail = draw_counts(np.random.default_rng(77 + n), n, ntail)
    refs = [br.fit_counts(X1, X2, m, 0.0, True, k) for m in tail]
    for f in refs:
        tb.assert_conditions(f, k)
    return X1, X2, np.concatenate([base[np.arange(cap) % nbase], tail]), nbase, refs, k


# ---- what the Jacobi promises: matrices laid out on marked rows ---------------------------------------------------------------
def marked_rows(T0, nperm, seed, transposed=False):
    """Z_1, Z_2 (n = ROWS_PER_SPLIT + 5 rows, all zero but 64 each), permutations and their ``sigma`` such that every entry of
    ``Z_1' Z_2[pi]`` is ONE product x * 1: with ``T0`` m x r, Z_1[pos1[i]] = e_i and Z_2[pos2[i]] = T0[i], and pi carries
    pos1[i] to pos2[sigma[i]], so T = T0[sigma] exactly.  transposed: the roles swapped, T = T0[argsort(sigma)]' (r x m).
    Both position sets reach into the second split."""
    T0 = np.asarray(T0, dtype=np.float64)
    m = T0.shape[0]
    n = rows_per_split() + 5
    rng = np.random.default_rng(seed)
    pos1 = np.concatenate([rng.choice(n - 5, size=m - 2, replace=False), [n - 4, n - 1]])
    pos2 = np.concatenate([rng.choice(n - 5, size=m - 2, replace=False), [n - 5, n - 2]])
    rng.shuffle(pos1), rng.shuffle(pos2)
    E, Z = np.zeros((n, m)), np.zeros((n, T0.shape[1]))
    E[pos2 if transposed else pos1] = np.eye(m)
    Z[pos1 if transposed else pos2] = T0
    rest1, rest2 = np.setdiff1d(np.arange(n), pos1), np.setdiff1d(np.arange(n), pos2)
    perms, sigmas = [], []
    for _ in range(nperm):
        sigma = rng.permutation(m)
        pi = np.empty(n, dtype=np.int32)
        pi[pos1] = pos2[sigma]
        pi[rest1] = rng.permutation(rest2)
        assert np.array_equal(np.sort(pi), np.arange(n))
        perms.append(pi), sigmas.append(sigma)
    Z1, Z2 = (Z, E) if transposed else (E, Z)
    return np.ascontiguousarray(Z1), np.ascontiguousarray(Z2), np.stack(perms), np.stack(sigmas)


def marked_product(T0, sigma, transposed=False):
    """What ``Z_1' Z_2[pi]`` is, entry for entry."""
    return T0[np.argsort(sigma)].T if transposed else T0[sigma]


def graded_matrix():
    """B (Gaussian, 64 x 33), D (a shuffled 2^(-2j), j = 0 .. 32: span 5e-20) and T0 = B D; the scaling is exact."""
    rng = np.random.default_rng(33)
    B = rng.standard_normal((64, 33))
    D = 2.0 ** (-2.0 * rng.permutation(33))
    return B, D, B * D


def graded_reference():
    """The singular values of T0 by ``mpmath.svd_r`` at 60 digits, descending, rounded to float64."""
    import mpmath

    with mpmath.workdps(60):
        s = mpmath.svd_r(mpmath.matrix(graded_matrix()[2].tolist()), compute_uv=False)
        return np.array(sorted((float(x) for x in s), reverse=True))


def graded_fixture():
    """(T0, sv) as stored under tests/golden (written by tools/gen_golden_resample.py)."""
    with np.load(GOLDEN) as f:
        return f["T0"], f["sv"]


def hestenes_singular_values(A, max_sweeps=30):
    """One-sided Jacobi in plain NumPy, cyclic by rows, with the kernel's test of a pair (4 eps sqrt(a_pp a_qq))."""
    A = np.array(A, dtype=np.float64)
    r = A.shape[1]
    tol = 4.0 * np.finfo(np.float64).eps
    for _ in range(max_sweeps):
        moved = False
        for p in range(r - 1):
            for q in range(p + 1, r):
                x, y = A[:, p].copy(), A[:, q].copy()
                hpp, hqq, hpq = x @ x, y @ y, x @ y
                if abs(hpq) > tol * np.sqrt(hpp * hqq):
                    zeta = (hqq - hpp) / (2.0 * hpq)
                    t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + np.hypot(1.0, zeta))
                    cs = 1.0 / np.hypot(1.0, t)
                    sn = cs * t
                    A[:, p], A[:, q] = cs * x - sn * y, sn * x + cs * y
                    moved = True
        if not moved:
            return np.sort(np.linalg.norm(A, axis=0))[::-1]
    raise AssertionError("the Hestenes loop did not settle")


def hadamard16():
    H = np.ones((1, 1))
    for _ in range(4):
        H = np.block([[H, H], [H, -H]])
    return H


# (n, p1, p2, the view whose column is zeroed, the column): the zero column is a Jacobi column either way round
ZERO_COLUMN = [(131, 24, 9, 2, 4), (131, 9, 24, 1, 6)]


def zero_column_case(n, p1, p2, view, col, nperm=8):
    """A whitened pair with one column set to 0, ``nperm`` permutations and the NumPy values (identity first)."""
    Z1, Z2 = tp.whitened_pair(n, p1, p2, seed=500 + p1)
    (Z1 if view == 1 else Z2)[:, col] = 0.0
    rng = np.random.default_rng(600 + p2)
    perms = np.stack([rng.permutation(n) for _ in range(nperm)]).astype(np.int32)
    refs = np.stack([pr.singular_values(Z1, Z2)] + [pr.singular_values(Z1, Z2, pi) for pi in perms])
    return Z1, Z2, perms, refs
