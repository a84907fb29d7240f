"""tests/split_emulation.py -- the host statement of the split-bf16 K1 route and of its pilot rule -- held to its own claims, without
a GPU: what the DESIGN of the route gives on Gaussian and on grid-valued float32 inputs (n = 32768, two views of 24 columns, fixed
seeds; the measure is tests/test_gpu_k1_split.py::_rel on the raw and on the centred moments).  The device is held to this
emulation in tests/test_gpu_k1_split_structured.py."""

import numpy as np
import pytest

import split_emulation as E

N, DIMS = 32768, [24, 24]
KINDS = ["gaussian", "binary", "onehot", "pixels8", "pixels7", "counts", "int300", "sparse_int", "relu", "from_bf16", "mean1000",
         "duplicate", "outlier_row", "student_t", "period16"]
EXACT = ["binary", "onehot", "pixels8", "counts", "int300"]                  # exact with the coarse pilot: mid = 0 everywhere
ON_A_GRID = EXACT + ["pixels7", "sparse_int"]                                # d / u are integers: exact_int applies


def _views(kind):
    return E.make_views(kind, N, DIMS, seed=100 + KINDS.index(kind))


def _errors(views, rule):
    Gr, s = E.float64_moments(views)
    G, s_emul = E.moments(views, E.pilot(views, rule))
    assert np.array_equal(s_emul, s)
    return E.rel(G, Gr), E.rel(E.centred(G, s, N), E.centred(Gr, s, N))


def test_bf16_rounding_is_round_to_nearest_even_on_the_bit_pattern():
    import torch

    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32)
    ties = (rng.integers(0, 2 ** 16, size=4096, dtype=np.uint64).astype(np.uint32) << np.uint32(16)) | np.uint32(0x8000)    # exact halves
    x = np.concatenate([bits, ties]).view(np.float32)
    x = x[np.isfinite(x)]
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    got = E.bf16_round(x)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.all(got.view(np.uint32) & np.uint32(0xFFFF) == 0)


def test_gaussian_rows_meet_the_designs_error():
    views = _views("gaussian")
    assert np.array_equal(E.pilot(views), E.pilot(views, "mean"))    # generic float32 columns keep the mean pilot, bit for bit
    for rule in ("coarse", "mean", "coarse_all"):                    # (a coarse pilot would be neutral on them)
        raw, cen = _errors(_views("gaussian"), rule)
        assert raw <= 5e-7 and cen <= 5e-7, (rule, raw, cen)


@pytest.mark.parametrize("kind", EXACT)
def test_grid_valued_inputs_are_exact_with_the_coarse_pilot(kind):
    views = _views(kind)
    Gr, s = E.float64_moments(views)
    p = E.pilot(views)
    G, _ = E.moments(views, p)
    assert np.array_equal(G, Gr)
    assert _errors(views, "coarse") == (0.0, 0.0)
    assert not np.any(E.planes(views, p)[1])                         # because mid = 0: hi holds x - p


@pytest.mark.parametrize("kind", ON_A_GRID)
def test_exact_int_equals_moments_bit_for_bit(kind):
    views = _views(kind)
    p = E.pilot(views)
    G, s = E.moments(views, p)
    Gi, si, u, window = E.exact_int(views, p)
    assert np.array_equal(Gi, G) and np.array_equal(si, s)
    assert window < 2.0 ** 22
    d = E.stack(views) - p[None, :]
    assert np.array_equal(d / u, np.rint(d / u)) and np.all(np.abs(d / u).max(axis=0) >= 1.0)


def test_sparse_integers_exercise_the_mid_plane():
    """The designed result lacks the off-diagonal mid * mid and keeps the diagonal one."""
    views = _views("sparse_int")
    p = E.pilot(views)
    assert np.any(E.planes(views, p)[1])
    G, _ = E.moments(views, p)
    Gr, _ = E.float64_moments(views)
    off = ~np.eye(G.shape[0], dtype=bool)
    assert np.any(G[off] != Gr[off])
    assert np.array_equal(np.diag(G), np.diag(Gr))


def test_mean_pilot_against_coarse_pilot_on_binary_features():
    """Why the rule exists: with the sample mean as the pilot, mid is the same number on every row that holds the same value and
    sum_k mid_ki mid_kj adds up coherently -- an error that does not fall with the row count; the coarse pilot keeps the grid."""
    views = _views("binary")
    raw_mean, cen_mean = _errors(views, "mean")
    assert raw_mean > 1e-6 and cen_mean > 1e-6, (raw_mean, cen_mean)
    assert _errors(views, "coarse") == (0.0, 0.0)
    short = [v[:4096] for v in views]                               # ... flat in n
    Gr, _ = E.float64_moments(short)
    assert E.rel(E.moments(short, E.pilot(short, "mean"))[0], Gr) > 1e-6


GENERIC = ["gaussian", "relu", "mean1000", "duplicate", "outlier_row", "student_t", "period16"]


def test_coarse_pilot_helps_values_up_cast_from_bfloat16():
    views = _views("from_bf16")
    (raw_c, cen_c), (raw_m, cen_m) = _errors(views, "coarse"), _errors(views, "mean")
    assert raw_c * 10.0 <= raw_m and cen_c * 10.0 <= cen_m, (raw_c, raw_m, cen_c, cen_m)
    assert raw_c <= 5e-7 and cen_c <= 5e-7


def test_relu_outputs_keep_the_mean_pilot_and_its_error():
    """Exact zeros among generic values are no grid: the column keeps the mean pilot (and the bits of its moments); what a coarse
    pilot for every column would have gained is on record here."""
    views = _views("relu")
    assert np.array_equal(E.pilot(views), E.pilot(views, "mean"))
    raw, cen = _errors(views, "coarse")
    assert 1e-6 < raw < 4e-6 and 1e-6 < cen < 5e-6, (raw, cen)
    raw_all, cen_all = _errors(views, "coarse_all")
    assert raw_all * 10.0 <= raw and cen_all * 10.0 <= cen


def test_which_columns_take_the_coarse_pilot_and_how_far_it_moves():
    """Grid-valued kinds: every column, |p - mean| <= sd / 8, u in (sd / 16, sd / 8].  Generic kinds: none, the pilot is the mean's
    bits; on columns whose mean is 1000 sigma the centred error stays what it was."""
    for kind in KINDS:
        views = _views(kind)
        mean, sd, u = E.pilot_stats(views)
        p = E.pilot(views).astype(np.float64)
        assert np.all(np.abs(p - mean) <= sd / 8.0 + np.abs(mean) * 2.0 ** -24), kind
        if kind in GENERIC:
            assert not np.any(u) and np.array_equal(E.pilot(views), E.pilot(views, "mean")), kind
        else:
            assert np.all((u > 0.0) & (u <= sd / 8.0) & (u > sd / 16.0)), kind
            assert np.array_equal(E.pilot(views), E.pilot(views, "coarse_all")), kind
    for rule in ("coarse", "coarse_all"):
        raw, cen = _errors(_views("mean1000"), rule)
        assert cen <= 1e-7 and raw <= 1e-12, (rule, raw, cen)


def test_pilot_of_mixed_columns():
    rng = np.random.default_rng(5)
    v = rng.standard_normal((5000, 4)).astype(np.float32)
    v[:, 1] = 2.7                                                    # sd == 0: the mean
    v[:, 2] = rng.poisson(3.0, 5000)                                 # counts: coarse
    v[:, 3] = 0.0                                                    # nothing to see
    p = E.pilot([v])
    S = E.pilot_sample([v])
    assert S.shape == (2048, 4) and np.array_equal(S[3], v[3 * 2].astype(np.float64))
    assert p[0] == np.float32(S[:, 0].sum() / 2048.0) and p[1] == np.float32(2.7) and p[3] == 0.0
    assert float(p[2]) * 8.0 == round(float(p[2]) * 8.0) and abs(float(p[2]) - S[:, 2].mean()) <= S[:, 2].std() / 8.0


def test_float32_chunks_model_stays_near_the_float64_accumulation():
    views = _views("gaussian")
    p = E.pilot(views)
    G, _ = E.moments(views, p)
    a256, a16k = E.rel(E.moments_f32_chunks(views, p, 256)[0], G), E.rel(E.moments_f32_chunks(views, p, 16384)[0], G)
    assert 0.0 < a256 < 2e-6 and 0.0 < a16k < 2e-6, (a256, a16k)


def test_pinned_effects_of_the_design():
    """What the rule does not fix: the cross-view copy of a diagonal entry lacks sum mid^2 (duplicated columns), heavy tails."""
    raw, _ = _errors(_views("duplicate"), "coarse")
    assert 1e-6 < raw < 6e-6, raw
    for kind in ("outlier_row", "student_t"):
        raw, _ = _errors(_views(kind), "coarse")
        assert 5e-7 < raw < 5e-5, (kind, raw)
