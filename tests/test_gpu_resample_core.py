"""The resampling core (csrc/resample_dev.h) through ``ccz_perm_singular_values`` and ``ccz_boot_rcca`` on the paths that the five
shapes of tests/test_gpu_perm.py and tests/test_gpu_boot.py leave out: every tile layout (1 to 4 tiles of 16 on either side, each
ragged), row counts at the edges of a chunk and of a split, bootstrap weights at full ``k``, counts that skip chunks and a whole
split, calls of more than one launch group, and what the one-sided Jacobi promises: small singular values to RELATIVE accuracy,
ties, an exact zero, and a NaN row that is written, not left.

Inputs, references and the conditions they meet are those of tests/resample_cases.py (asserted on the CPU by
tests/test_resample_cases_host.py); helpers and bars are those of the two GPU modules.  The bars: 1e-8 on ``sigma / sigma_1``
and on the gap-free identities ``W_i' R_i W_i = I``, ``W_1' C_12 W_2 = diag(sigma)`` (a backward-stable solve leaves
``p eps cond(R) <= 64 * 2.2e-16 * 1e4 = 1.4e-10``, and ``cond <= 1e4`` is asserted); ``1e-8 / GAP`` on the weight columns that
have an asserted gap; 1e-10 RELATIVE on every singular value of the graded matrix (one-sided Jacobi: ``r eps cond(B) <=
1.5e-13``; LAPACK's bidiagonal route gives 4e-2 there and the Gram route 1e11).  Each test prints the worst error it measured;
on an MI355X they are listed in DESIGN.md sections 4r and 4s.
"""

import ctypes as C

import numpy as np
import pytest

import resample_cases as rc
import test_gpu_boot as tb
import test_gpu_perm as tp
from test_gpu_boot import WBAR, errors
from test_gpu_perm import BAR, worst_error

pytestmark = pytest.mark.gpu

RS_SCRATCH = 1 << 25                                    # csrc/resample_dev.h: RS_SCRATCH = 2^25 doubles of partials per launch group
RS_MAXBATCH = 65535                                     # csrc/resample_dev.h: RS_MAXBATCH = 65535, gridDim.y
GRADED_BAR = 1e-10


def tiles(p):
    return (p + 15) // 16


def launch_cap(per_item):
    """The items of one launch group, as ``for_batches`` computes it."""
    return max(1, min(RS_SCRATCH // per_item, RS_MAXBATCH))


def perm_per_item(n, p1, p2):
    return -(-n // rc.rows_per_split()) * 256 * tiles(p1) * tiles(p2)


def boot_per_item(n, p1, p2):
    P1, P2 = 16 * tiles(p1), 16 * tiles(p2)
    return -(-n // rc.rows_per_split()) * (P1 * P1 + P1 * P2 + P2 * P2 + P1 + P2 + 1)


class Raw(tp.Device):
    """Any Z_1, Z_2 in HBM; ``run`` with the scale and the prefill of ``sv`` chosen by the caller."""

    def __init__(self, Z1, Z2):
        self.h = tp._handle()
        self.n, self.p1, self.p2 = Z1.shape[0], Z1.shape[1], Z2.shape[1]
        self.r = min(self.p1, self.p2)
        self.z1, self.z2 = self.h.to_device(np.ascontiguousarray(Z1)), self.h.to_device(np.ascontiguousarray(Z2))

    def run(self, perms, scale=None, prefill=-7.0):
        h, vp = self.h, C.c_void_p
        nperm = 1 if perms is None else int(perms.shape[0])
        pd = None if perms is None else h.to_device(np.ascontiguousarray(perms, dtype=np.int32))
        sv = h.to_device(np.full((nperm, self.r), prefill))
        h.check(h.lib.ccz_perm_singular_values(h.raw, self.n, self.p1, self.p2, vp(self.z1.ptr), vp(self.z2.ptr),
                                               vp(pd.ptr) if pd is not None else None, nperm,
                                               1.0 / (self.n - 1) if scale is None else scale, vp(sv.ptr)))
        return h.to_host(sv, (nperm, self.r))


# ---- 1. every tile layout, and the row counts at the edges ------------------------------------------------------------------
@pytest.mark.parametrize("n,p1,p2", rc.perm_sweep_shapes() + rc.perm_row_shapes())
def test_perm_layouts_match_numpy(n, p1, p2):
    _, _, ident, perms, refs = tp.case(n, p1, p2)
    dev = tp.Device(n, p1, p2)
    errs = {"identity": worst_error(dev.run(None), ident),
            "batch": worst_error(dev.run(perms[:rc.SWEEP_PERMS]), refs[:rc.SWEEP_PERMS])}
    print(f"perm layout n={n} ({p1}, {p2}) tiles ({tiles(p1)}, {tiles(p2)}): worst |sigma - ref| / sigma_1 = {errs}")
    assert max(errs.values()) <= BAR, errs


@pytest.mark.parametrize("shape,c", [(s, 0.0) for s in rc.boot_sweep_shapes()] + rc.boot_row_cases())
def test_boot_layouts_match_numpy(shape, c):
    X1, X2, counts, refs, ident, k = rc.boot_case(shape, c)
    assert max(max(f.cond) for f in refs + [ident]) <= tb.COND
    dev = tb.Device(shape, c, True, X1, X2)
    sv, W, info = dev.run(counts, k)
    assert not info.any()
    batch = errors(sv, W, refs, shape[1])
    sv1, W1, info1 = dev.run(None, k)
    assert not info1.any()
    one = errors(sv1, W1, [ident], shape[1])
    print(f"boot layout n={shape[0]} ({shape[1]}, {shape[2]}) tiles ({tiles(shape[1])}, {tiles(shape[2])}) c={c}: "
          f"worst |sigma - ref| / sigma_1 = {max(batch[0], one[0]):.3g}, worst weight error = {max(batch[1], one[1]):.3g}")
    assert max(batch[0], one[0]) <= BAR and max(batch[1], one[1]) <= WBAR


# ---- 2. bootstrap at full k -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,k", rc.FULL_K)
def test_boot_full_k_meets_the_identities(shape, k):
    """On an MI355X the worst identity residual over the five shapes is 4.5e-14 (``W_2' R_2 W_2`` at (64, 64), k = 64)."""
    X1, X2, counts, refs, ident, _ = rc.boot_case(shape, 0.0, rc.FULL_K_BOOT, k)
    assert max(max(f.cond) for f in refs + [ident]) <= tb.COND
    dev = tb.Device(shape, 0.0, True, X1, X2)
    p1 = shape[1]
    sv, W, info = dev.run(counts, k)
    sv1, W1, info1 = dev.run(None, k)
    assert not info.any() and not info1.any() and W.shape == (rc.FULL_K_BOOT, p1 + shape[2], k)
    ones = np.ones(shape[0], dtype=np.int32)
    resid = [rc.identity_residuals(X1, X2, m, s, w[:p1], w[p1:]) for m, s, w in zip(counts, sv, W)]
    resid.append(rc.identity_residuals(X1, X2, ones, sv1[0], W1[0, :p1], W1[0, p1:]))
    e_id = np.max(np.array(resid), axis=0)
    first = [type(f)(sv=f.sv, weights=[w[:, :2] for w in f.weights]) for f in refs + [ident]]   # the columns with an asserted gap
    e_sv, e_w = errors(np.concatenate([sv, sv1]), np.concatenate([W, W1])[:, :, :2], first, p1)
    print(f"boot full k n={shape[0]} ({p1}, {shape[2]}) k={k}: |W1' R1 W1 - I| {e_id[0]:.3g}, |W2' R2 W2 - I| {e_id[1]:.3g}, "
          f"|W1' C12 W2 - diag(sigma)| {e_id[2]:.3g}, worst |sigma - ref| / sigma_1 = {e_sv:.3g}, columns 0, 1: {e_w:.3g}")
    assert e_id.max() <= BAR and e_sv <= BAR and e_w <= WBAR


# ---- 3. counts that skip chunks ------------------------------------------------------------------------------------------------
def test_boot_counts_that_skip_chunks():
    shape, X1, X2, counts, refs, k = rc.skip_case()
    R = rc.rows_per_split()
    assert np.all(rc.zero_chunks(counts) >= 1) and not counts[:, R:2 * R].any() and counts.max() >= 50
    assert max(max(f.cond) for f in refs) <= tb.COND
    dev = tb.Device(shape, 0.0, True, X1, X2)
    whole = dev.run(counts, k)
    assert not whole[2].any()
    e_sv, e_w = errors(whole[0], whole[1], refs, shape[1])
    print(f"boot skipped chunks n={shape[0]} ({shape[1]}, {shape[2]}): worst |sigma - ref| / sigma_1 = {e_sv:.3g}, worst weight error = {e_w:.3g}")
    assert e_sv <= BAR and e_w <= WBAR
    alone = [dev.run(counts[b:b + 1], k) for b in range(len(counts))]
    for got, want in zip((np.concatenate(x) for x in zip(*alone)), whole):
        np.testing.assert_array_equal(got, want)


# ---- 4. more than one launch group -------------------------------------------------------------------------------------------
def _perm_groups():
    R = rc.rows_per_split()
    return [((37, 5, 3), RS_MAXBATCH, 70), ((R + 5, 57, 57), 4096, 40)]


@pytest.mark.parametrize("shape,cap,ntail", _perm_groups())
def test_perm_launch_groups(shape, cap, ntail):
    assert launch_cap(perm_per_item(*shape)) == cap
    perms, tail_refs = rc.perm_group_case(shape, cap, ntail)
    count = cap + ntail
    assert perms.shape == (count, shape[0]) and count > cap
    dev = tp.Device(*shape)
    got = dev.run(perms)
    np.testing.assert_array_equal(got[cap:], dev.run(perms[cap:]))                   # the second group alone
    e = worst_error(got[cap:], tail_refs)
    print(f"perm launch groups n={shape[0]} ({shape[1]}, {shape[2]}) {count} permutations, cap {cap}: tail worst |sigma - ref| / sigma_1 = {e:.3g}")
    assert e <= BAR
    base = dev.run(tp.case(*shape)[3])
    rows = np.arange(0, cap, 1000)
    np.testing.assert_array_equal(got[rows], base[rows % tp.NBATCH])


def _boot_groups():
    R = rc.rows_per_split()
    return [((60, 5, 3), 41890, 30), ((R + 5, 64, 64), 1351, 20)]


@pytest.mark.parametrize("shape,cap,ntail", _boot_groups())
def test_boot_launch_groups(shape, cap, ntail):
    assert launch_cap(boot_per_item(*shape)) == cap
    X1, X2, counts, nbase, tail_refs, k = rc.boot_group_case(shape, cap, ntail)
    count = cap + ntail
    assert counts.shape == (count, shape[0]) and count > cap
    dev = tb.Device(shape, 0.0, True, X1, X2)
    got = dev.run(counts, k)
    assert not got[2].any()
    for a, b in zip(got, dev.run(counts[cap:], k)):                                  # the second group alone
        np.testing.assert_array_equal(a[cap:], b)
    e_sv, e_w = errors(got[0][cap:], got[1][cap:], tail_refs, shape[1])
    print(f"boot launch groups n={shape[0]} ({shape[1]}, {shape[2]}) {count} resamples, cap {cap}: tail worst |sigma - ref| / sigma_1 = {e_sv:.3g}, "
          f"worst weight error = {e_w:.3g}")
    assert e_sv <= BAR and e_w <= WBAR
    base = dev.run(counts[:nbase], k)
    rows = np.arange(0, cap, 1000)
    for a, b in zip(got, base):
        np.testing.assert_array_equal(a[rows], b[rows % nbase])


# ---- 5. what the Jacobi promises (scale = 1) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("transposed", [False, True])
def test_graded_singular_values_to_relative_accuracy(transposed):
    """Every singular value of T0 = B D (sigma_r / sigma_1 = 4e-20) to 1e-10 of ITSELF.  On an MI355X: 4.4e-15 at (64, 33), 4.7e-15 at
    (33, 64)."""
    T0, ref = rc.graded_fixture()
    np.testing.assert_array_equal(T0, rc.graded_matrix()[2])
    Z1, Z2, perms, _ = rc.marked_rows(T0, 8, seed=9, transposed=transposed)
    dev = Raw(Z1, Z2)
    batch = dev.run(perms, scale=1.0)
    assert np.all(np.isfinite(batch)) and np.all(np.diff(batch, axis=1) < 0)
    alone = np.concatenate([dev.run(perms[b:b + 1], scale=1.0) for b in range(len(perms))])
    np.testing.assert_array_equal(alone, batch)
    rel = float(np.max(np.abs(batch - ref) / ref))
    print(f"graded matrix ({Z1.shape[1]}, {Z2.shape[1]}): worst |sigma_j - ref_j| / ref_j = {rel:.3g}")
    assert rel <= GRADED_BAR


def test_equal_singular_values_fill_every_slot():
    Z1, Z2, perms, _ = rc.marked_rows(rc.hadamard16(), 6, seed=10)
    got = Raw(Z1, Z2).run(perms, scale=1.0, prefill=-7.0)
    np.testing.assert_array_equal(got, np.full((6, 16), 4.0))


@pytest.mark.parametrize("n,p1,p2,view,col", rc.ZERO_COLUMN)
def test_zero_column_gives_an_exact_zero(n, p1, p2, view, col):
    Z1, Z2, perms, refs = rc.zero_column_case(n, p1, p2, view, col)
    dev = Raw(Z1, Z2)
    got = np.concatenate([dev.run(None), dev.run(perms)])
    assert np.all(np.isfinite(got)) and np.all(np.diff(got, axis=1) <= 0)
    np.testing.assert_array_equal(got[:, -1], np.zeros(len(got)))
    e = float(np.max(np.abs(got - refs) / refs[:, :1]))
    print(f"zero column n={n} ({p1}, {p2}), column {col} of view {view}: worst |sigma - ref| / sigma_1 = {e:.3g}")
    assert e <= BAR


@pytest.mark.parametrize("n,p1,p2", [(37, 5, 3), (37, 3, 5), (131, 40, 24), (131, 24, 40)])
def test_nan_row_is_written(n, p1, p2):
    """With p1 < p2 the Jacobi columns are the rows of T and a NaN in Z_1 reaches one of them only: ranking the finite norms
    beside it once wrote a slot twice and left the last slot of the row at its prefill."""
    Z1, Z2, _, perms, refs = tp.case(n, p1, p2)
    bad = np.array(Z1)
    bad[n // 2, 1] = np.nan
    dev = Raw(bad, Z2)
    for got in (dev.run(None), dev.run(perms[:5])):
        assert np.all(np.isnan(got)), got                  # every slot of every row: nothing is left at the prefill
    clean = tp.Device(n, p1, p2)                           # the same handle afterwards
    e = worst_error(clean.run(perms[:5]), refs[:5])
    print(f"after a NaN call n={n} ({p1}, {p2}): worst |sigma - ref| / sigma_1 = {e:.3g}")
    assert e <= BAR
