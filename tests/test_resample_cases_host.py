"""CPU tests of tests/resample_cases.py: every condition that tests/test_gpu_resample_core.py rests on is asserted here on the
NumPy side, so a broken input or reference shows without a GPU -- the generators' conditioning and gaps at every sweep shape,
the restatement's own identity residuals, the zero chunks and the zero split, the exactness of the marked-row construction,
the graded reference against mpmath, and a plain Hestenes loop meeting a bar a hundred times tighter than the device's."""

import numpy as np
import pytest

import boot_restatement as br
import resample_cases as rc
import test_gpu_boot as tb
import test_gpu_perm as tp


# ---- the sweeps -------------------------------------------------------------------------------------------------------------
def test_sweep_shapes_reach_every_layout():
    perm, boot = rc.perm_sweep_shapes(), rc.boot_sweep_shapes()
    assert len(perm) == 15 and len(boot) == 16 and (131, 9, 9) not in perm
    tiles = lambda p: (p + 15) // 16                                                  # noqa: E731
    assert {(tiles(p1), tiles(p2)) for _, p1, p2 in boot} == {(a, b) for a in range(1, 5) for b in range(1, 5)}
    assert {(tiles(p1), tiles(p2)) for _, p1, p2 in perm} == {(a, b) for a in range(1, 5) for b in range(1, 5)} - {(1, 1)}
    assert all(p % 16 for p in rc.WIDTHS) and rc.PERM_SWEEP_N % 32 == 3
    R = rc.rows_per_split()
    assert [s[0] for s in rc.perm_row_shapes()] == [R, 2 * R + 1, 6] and [s[0][0] for s in rc.boot_row_cases()] == [R, 2 * R + 1, 7]


@pytest.mark.parametrize("n,p1,p2", rc.perm_sweep_shapes() + rc.perm_row_shapes())
def test_perm_generator_meets_its_condition(n, p1, p2):
    _, _, ident, perms, refs = tp.case(n, p1, p2)          # (the case itself asserts 2 COND on every permutation)
    ratio = min(float(ident[-1] / ident[0]), float(np.min(refs[:rc.SWEEP_PERMS, -1] / refs[:rc.SWEEP_PERMS, 0])))
    print(f"perm n={n} ({p1}, {p2}): smallest sigma_r / sigma_1 = {ratio:.3g}")
    assert ratio >= tp.COND and perms.shape == (tp.NBATCH, n)


@pytest.mark.parametrize("shape,c", [(s, 0.0) for s in rc.boot_sweep_shapes()] + rc.boot_row_cases())
def test_boot_generator_meets_its_conditions(shape, c):
    _, _, counts, refs, ident, k = rc.boot_case(shape, c)   # (the case itself asserts the gaps)
    cond = max(max(f.cond) for f in refs + [ident])
    print(f"boot n={shape[0]} ({shape[1]}, {shape[2]}) c={c}: worst cond(R_i) = {cond:.3g}")
    assert cond <= tb.COND and counts.shape == (rc.SWEEP_BOOT, shape[0]) and k == min(shape[1], shape[2], 2)
    assert np.all(counts.sum(axis=1) == shape[0])
    if shape[0] == 7:
        assert counts.max() >= 2                           # rows do repeat: the ridge is what keeps R_i conditioned


def test_boot_case_is_the_head_of_the_existing_case():
    shape = (60, 5, 3)
    X1, X2, counts, refs, ident, k = tb.case(shape, 0.0, True, False)
    Y1, Y2, head, hrefs, hident, hk = rc.boot_case(shape)
    np.testing.assert_array_equal(Y1, X1), np.testing.assert_array_equal(Y2, X2)
    np.testing.assert_array_equal(head, counts[:rc.SWEEP_BOOT])
    np.testing.assert_array_equal(hrefs[-1].sv, refs[rc.SWEEP_BOOT - 1].sv)
    np.testing.assert_array_equal(hident.weights[0], ident.weights[0])
    assert hk == k


# ---- full k ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,k", rc.FULL_K)
def test_restatement_meets_the_identities_at_full_k(shape, k):
    X1, X2, counts, refs, ident, kk = rc.boot_case(shape, 0.0, rc.FULL_K_BOOT, k)
    assert kk == k <= min(shape[1:]) and len(refs) == rc.FULL_K_BOOT
    worst = max(max(rc.identity_residuals(X1, X2, m, f.sv, *f.weights)) for m, f in zip(counts, refs))
    worst = max(worst, max(rc.identity_residuals(X1, X2, np.ones(shape[0], dtype=np.int32), ident.sv, *ident.weights)))
    cond = max(max(f.cond) for f in refs + [ident])
    print(f"full k n={shape[0]} ({shape[1]}, {shape[2]}) k={k}: restatement's identity residual {worst:.3g}, cond {cond:.3g}")
    assert worst <= 1e-12 and cond <= tb.COND
    assert refs[0].weights[0].shape == (shape[1], k) and refs[0].weights[1].shape == (shape[2], k)


def test_full_k_reaches_the_second_pass():
    jobs = [2 * k for _, k in rc.FULL_K]                   # the back substitution takes 64 (view, column) jobs per pass
    assert jobs == [128, 66, 66, 34, 64]
    assert [(s[1] < s[2]) for s, _ in rc.FULL_K[1:3]] == [False, True]


# ---- counts that skip chunks -----------------------------------------------------------------------------------------------
def test_skip_case_has_zero_chunks_and_a_zero_split():
    shape, X1, X2, counts, refs, k = rc.skip_case()
    R = rc.rows_per_split()
    assert shape == (2 * R + 5, 24, 40) and counts.shape == (8, shape[0])
    assert not counts[:, 64:200].any() and not counts[:, R:2 * R].any()
    assert np.all(counts[:, 2 * R:].sum(axis=1) > 0)       # the third split's five rows are drawn
    assert np.all(rc.zero_chunks(counts) >= 4 + R // 32)   # [64, 192) and the second split, whole chunks
    big = counts.max(axis=1)
    assert sorted(np.flatnonzero(big >= 50)) == [2, 5] and np.all(counts.sum(axis=1)[[2, 5]] == shape[0] + 250)
    cond = max(max(f.cond) for f in refs)
    print(f"skip case: largest multiplicity {big.max()}, worst cond(R_i) = {cond:.3g}")
    assert cond <= tb.COND


# ---- the marked-row construction and the graded matrix ------------------------------------------------------------------------
@pytest.mark.parametrize("transposed", [False, True])
def test_marked_rows_give_the_permuted_matrix_exactly(transposed):
    T0 = rc.graded_matrix()[2]
    Z1, Z2, perms, sigmas = rc.marked_rows(T0, 8, seed=9, transposed=transposed)
    n = rc.rows_per_split() + 5
    assert Z1.shape == (n, 33 if transposed else 64) and Z2.shape == (n, 64 if transposed else 33) and perms.dtype == np.int32
    for Z in (Z1, Z2):
        marked = np.flatnonzero(Z.any(axis=1))
        assert len(marked) == 64 and marked.min() < rc.rows_per_split() <= marked.max()     # both splits
    for pi, sigma in zip(perms, sigmas):
        np.testing.assert_array_equal(Z1.T @ Z2[pi], rc.marked_product(T0, sigma, transposed))
    assert len({tuple(s) for s in sigmas}) == 8
    H = rc.hadamard16()
    np.testing.assert_array_equal(H.T @ H, 16.0 * np.eye(16))
    Z1, Z2, perms, sigmas = rc.marked_rows(H, 4, seed=10)
    np.testing.assert_array_equal(Z1.T @ Z2[perms[3]], H[sigmas[3]])


def test_graded_matrix_is_what_the_bar_assumes():
    B, D, T0 = rc.graded_matrix()
    assert np.linalg.cond(B) <= 10
    np.testing.assert_array_equal(np.sort(D)[::-1], 2.0 ** (-2.0 * np.arange(33)))
    np.testing.assert_array_equal(T0 / D, B)               # the scaling is exact
    fT0, fsv = rc.graded_fixture()
    np.testing.assert_array_equal(fT0, T0)                 # the fixture is this matrix's
    assert fsv.shape == (33,) and np.all(np.diff(fsv) < 0) and fsv[-1] / fsv[0] < 1e-18


def test_graded_fixture_equals_mpmath():
    pytest.importorskip("mpmath")
    np.testing.assert_array_equal(rc.graded_reference(), rc.graded_fixture()[1])


def test_hestenes_loop_reaches_the_bar_and_the_other_routes_do_not():
    T0, ref = rc.graded_fixture()
    rel = lambda s: float(np.max(np.abs(np.asarray(s) - ref) / ref))                  # noqa: E731
    jac = max(rel(rc.hestenes_singular_values(T0)), rel(rc.hestenes_singular_values(T0[::-1])))
    lapack = rel(np.linalg.svd(T0, compute_uv=False))
    gram = rel(np.sqrt(np.abs(np.linalg.eigvalsh(T0.T @ T0)[::-1])))
    print(f"graded case, relative error: Hestenes {jac:.3g}, LAPACK {lapack:.3g}, Gram {gram:.3g}")
    assert jac <= 1e-12                                    # the device's bar, 1e-10, is reachable by the algorithm it claims to be
    assert lapack > 1e-10 and gram > 1e-10                 # and a change of route would not pass it


def test_zero_column_cases():
    for n, p1, p2, view, col in rc.ZERO_COLUMN:
        Z1, Z2, perms, refs = rc.zero_column_case(n, p1, p2, view, col)
        assert not (Z1 if view == 1 else Z2)[:, col].any() and (p1 < p2) == (view == 1)
        assert refs.shape == (9, min(p1, p2)) and np.all(refs[:, -1] <= 1e-12 * refs[:, 0]) and np.all(refs[:, -2] >= tp.COND * refs[:, 0])
