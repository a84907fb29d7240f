"""``ccz_draw_permutations`` / ``ccz_draw_counts`` (csrc/draw.hip) against tests/draw_restatement.py, bit for bit, and
``permutation_test`` / ``bootstrap`` with ``draws="device"`` against the float64 restatements of the two functions run on the
restated draws of the same seed.

The draws are integers, so every comparison of them is ``assert_array_equal``.  The public functions keep the bars and the
conditions of tests/test_gpu_perm.py and tests/test_gpu_boot.py, whose helpers are imported: 1e-8 on ``sigma / sigma_1``, 2e-6
on the weights, asserted conditioning of every reference that is compared.
"""

import ctypes as C
import functools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import boot_restatement as br
import draw_restatement as dr
import perm_restatement as pr
import test_gpu_boot as tb
import test_gpu_perm as tp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0xC0FFEE1234567891                                   # all 64 bits must reach the kernel
EINVAL, EUNSUP = -1, -6
SENTINEL = -7
NS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 70001]
BIG_N = 1100003                                             # more than 1024 buckets at the default bucket size
MAXB = 65


def _header(name):
    header = open(os.path.join(ROOT, "include", "ccz.h")).read()
    return int(re.search(r"#define %s (\d+)" % name, header).group(1))


@functools.lru_cache(maxsize=None)
def restated_permutations(n, count=MAXB):
    out = np.stack([dr.permutation(SEED, b, n) for b in range(count)]).astype(np.int32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated_counts(n, count=MAXB):
    out = np.stack([dr.counts(SEED, b, n) for b in range(count)]).astype(np.int32)
    out.setflags(write=False)
    return out


def draw(what, n, count, seed=SEED, first=0, bucket_rows=0, expect=0):
    """Rows ``[first, first + count)`` from the entry point in ONE call, into a buffer of ``count x n`` sentinels (a call that
    is expected to be refused gets a small buffer, which must come back as it was)."""
    h, vp = tp._handle(), C.c_void_p
    out = h.to_device(np.full((4, 64) if expect else (count, n), SENTINEL, dtype=np.int32))
    if what == "permutations":
        rc = h.lib.ccz_draw_permutations(h.raw, n, count, seed, first, bucket_rows, vp(out.ptr))
    else:
        rc = h.lib.ccz_draw_counts(h.raw, n, count, seed, first, vp(out.ptr))
    assert rc == expect, (rc, h.lib.ccz_last_error(h.raw))
    return h.to_host(out, out.shape, dtype=np.int32)


@pytest.mark.parametrize("count", [1, 3, MAXB])
@pytest.mark.parametrize("n", NS)
def test_permutations_equal_the_restatement(n, count):
    np.testing.assert_array_equal(draw("permutations", n, count), restated_permutations(n)[:count])


@pytest.mark.parametrize("count", [1, 3, MAXB])
@pytest.mark.parametrize("n", NS)
def test_counts_equal_the_restatement(n, count):
    np.testing.assert_array_equal(draw("counts", n, count), restated_counts(n)[:count])


def test_more_than_1024_buckets_at_the_default_bucket_size():
    assert -(-BIG_N // _header("CCZ_DRAW_BUCKET_ROWS")) > 1024
    np.testing.assert_array_equal(draw("permutations", BIG_N, 2), restated_permutations(BIG_N, 2))
    np.testing.assert_array_equal(draw("counts", BIG_N, 2), restated_counts(BIG_N, 2))


def bucket_loads(n, b, bucket_rows):
    nb = -(-n // bucket_rows)
    return np.bincount(dr.mulhi(dr.key(SEED, b, dr.SITE_PERM, np.arange(n)), nb).astype(np.int64), minlength=nb)


def test_bucket_rows_does_not_change_a_bit():
    n, count, cap = 70001, 3, _header("CCZ_DRAW_SORT_CAP")
    want = restated_permutations(n)[:count]
    # 16: 4376 buckets, more than one tile of the scan and more than a workgroup's LDS histogram holds; 1024: every bucket
    # sorted in LDS; 4096: every bucket larger than the sort pass's LDS capacity, ranked by counting
    assert -(-n // 16) == 4376
    assert all(bucket_loads(n, b, 1024).max() <= cap for b in range(count))
    assert all(bucket_loads(n, b, 4096).min() > cap for b in range(count))
    for rows in (16, 1024, 4096):
        np.testing.assert_array_equal(draw("permutations", n, count, bucket_rows=rows), want, err_msg=f"bucket_rows = {rows}")
    np.testing.assert_array_equal(draw("permutations", n, count, bucket_rows=_header("CCZ_DRAW_BUCKET_ROWS")), draw("permutations", n, count))


def test_one_oversize_bucket_and_buckets_of_one_row():
    """n = 4097 in ONE bucket: the oversize path with a third, ragged tile of keys.  n = 1025 in 1025 buckets: empty ones too."""
    np.testing.assert_array_equal(draw("permutations", 4097, 3, bucket_rows=8192), restated_permutations(4097)[:3])
    np.testing.assert_array_equal(draw("permutations", 1025, 3, bucket_rows=1), restated_permutations(1025)[:3])


@pytest.mark.parametrize("what,ref", [("permutations", restated_permutations), ("counts", restated_counts)])
def test_splits_and_repeats_give_the_same_rows(what, ref):
    n = 4097
    whole = draw(what, n, 10)
    np.testing.assert_array_equal(whole, ref(n)[:10])
    np.testing.assert_array_equal(draw(what, n, 10), whole)                                        # the same call twice
    np.testing.assert_array_equal(np.concatenate([draw(what, n, 3, first=0), draw(what, n, 7, first=3)]), whole)
    np.testing.assert_array_equal(draw(what, n, 1, first=64), ref(n)[64:65])
    assert not np.array_equal(draw(what, n, 1, seed=SEED + 1), whole[:1])


def test_entry_points_refuse_and_write_nothing():
    h, vp = tp._handle(), C.c_void_p
    for what in ("permutations", "counts"):
        for kw in (dict(n=0, count=2), dict(n=37, count=0), dict(n=37, count=-1), dict(n=-5, count=2), dict(n=37, count=2, first=-1)):
            got = draw(what, kw["n"], kw["count"], first=kw.get("first", 0), expect=EINVAL)
            assert np.all(got == SENTINEL), (what, kw)
        got = draw(what, 2 ** 31, 1, expect=EUNSUP)
        assert np.all(got == SENTINEL), what
        assert b"2^31" in h.lib.ccz_last_error(h.raw)
    got = draw("permutations", 37, 2, bucket_rows=-1, expect=EINVAL)
    assert np.all(got == SENTINEL)
    assert h.lib.ccz_draw_permutations(h.raw, 37, 2, SEED, 0, 0, None) == EINVAL
    assert h.lib.ccz_draw_counts(h.raw, 37, 2, SEED, 0, None) == EINVAL
    assert h.lib.ccz_draw_permutations(h.raw, 2 ** 31, 0, SEED, 0, 0, None) == EINVAL            # the counts come first
    np.testing.assert_array_equal(draw("permutations", 37, 2), restated_permutations(37)[:2])     # and the handle still works


# ---- permutation_test(draws="device") ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def perm_reference(name, dtype):
    _, c, center = tp.ESTIMATORS[name]
    seed = dr.seed_of(tp.PUB_SEED)
    perms = [dr.permutation(seed, b, tp.PUB_N) for b in range(tp.PUB_B)]
    ref = pr.restate(tp.public_views(dtype), c=c, center=center, perms=perms)
    # the conditions of tests/test_gpu_perm.py's public reference, on these permutations
    assert np.min(np.abs(ref.null - ref.statistic[None, :])) > 1e-6
    assert np.min(np.abs(ref.tail_null - ref.tail[None, :])) > 1e-6
    assert np.all(ref.null[:, -1] >= tp.COND * ref.null[:, 0]) and ref.statistic[-1] >= tp.COND * ref.statistic[0]
    return ref


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(tp.ESTIMATORS))
def test_permutation_test_with_device_draws_matches_restatement(name, dtype):
    from cca_zoo_amd.model_selection import permutation_test

    ref = perm_reference(name, dtype)
    views = [np.array(v) for v in tp.public_views(dtype)]
    res = permutation_test(tp.ESTIMATORS[name][0](3), views, n_permutations=tp.PUB_B, random_state=tp.PUB_SEED, draws="device")
    host = permutation_test(tp.ESTIMATORS[name][0](3), views, n_permutations=tp.PUB_B, random_state=tp.PUB_SEED, draws="numpy")
    assert res.null.shape == (tp.PUB_B, 7)
    e_stat = float(np.max(np.abs(res.statistic - ref.statistic)) / ref.statistic[0])
    e_null = float(np.max(np.abs(res.null - ref.null) / ref.null[:, :1]))
    print(f"permutation_test device draws {name} {np.dtype(dtype).name}: statistic {e_stat:.3g}, null {e_null:.3g}")
    assert e_stat <= tp.BAR and e_null <= tp.BAR
    np.testing.assert_array_equal(res.pvalues, ref.pvalues)
    np.testing.assert_array_equal(res.tail_pvalues, ref.tail_pvalues)
    np.testing.assert_array_equal(res.statistic, host.statistic)                                   # the draws do not touch it
    assert not np.array_equal(res.null, host.null)                                                 # other, equally valid draws


def test_permutation_chunks_and_view_placement_do_not_change_a_bit(monkeypatch):
    import torch

    from cca_zoo_amd.linear import rCCA
    from cca_zoo_amd.model_selection import _permutation as pm

    def host_draw(*a, **k):
        raise AssertionError("draws='device' drew on the host")

    monkeypatch.setattr(pm, "draw_permutations", host_draw)
    views = [np.array(v) for v in tp.public_views(np.float64)]
    run = lambda v: pm.permutation_test(rCCA(c=[0.1, 0.3]), v, n_permutations=tp.PUB_B, random_state=tp.PUB_SEED, draws="device")
    base = run(views)
    for chunk in (1, 7, tp.PUB_B):
        monkeypatch.setattr(pm, "CHUNK_PERMS", chunk)
        res = run(views)
        np.testing.assert_array_equal(res.null, base.null)
        np.testing.assert_array_equal(res.statistic, base.statistic)
    res = run([torch.tensor(v, device="cuda") for v in views])
    np.testing.assert_array_equal(res.null, base.null)
    np.testing.assert_array_equal(res.pvalues, base.pvalues)


def test_both_draws_answer_the_same_question():
    """The views of tests/test_gpu_perm.py::test_planted_and_independent_views."""
    from cca_zoo_amd.linear import CCA
    from cca_zoo_amd.model_selection import permutation_test

    rng = np.random.default_rng(8)
    n = 200
    z = rng.standard_normal((n, 1))
    planted = [z @ rng.standard_normal((1, 6)) + rng.standard_normal((n, 6)), z @ rng.standard_normal((1, 4)) + rng.standard_normal((n, 4))]
    independent = [rng.standard_normal((n, 6)), rng.standard_normal((n, 4))]
    p = {(kind, draws): permutation_test(CCA(), views, n_permutations=999, random_state=0, draws=draws).tail_pvalues[0]
         for kind, views in (("planted", planted), ("independent", independent)) for draws in ("numpy", "device")}
    print(f"omnibus p-values: {p}")
    assert p["planted", "numpy"] == p["planted", "device"] == 1.0 / 1000.0
    assert p["independent", "numpy"] > 0.05 and p["independent", "device"] > 0.05


# ---- bootstrap(draws="device") ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def boot_reference(name, dtype):
    """``boot_restatement.restate`` with the restated multiplicities of the same seed in place of its own draws."""
    _, c, center = tb.ESTIMATORS[name]
    X1, X2 = (np.asarray(v, dtype=np.float64) for v in tb.public_views(dtype))
    seed, k = dr.seed_of(tb.PUB_SEED), tb.PUB_K
    obs = br.fit_rows(X1, X2, c, center, k)
    tb.assert_conditions(obs, k)
    O1, O2 = br.orient_observed(*obs.weights)
    sv_boot, w_boot = [], [[], []]
    for b in range(tb.PUB_B):
        m = dr.counts(seed, b, tb.PUB_N)
        assert m.sum() == tb.PUB_N
        f = br.fit_counts(X1, X2, m, c, center, k)
        tb.assert_conditions(f, k)
        W1, W2 = br.orient_to(f.weights[0], f.weights[1], O1, O2)
        sv_boot.append(f.sv), w_boot[0].append(W1), w_boot[1].append(W2)
    sv_boot, w_boot = np.stack(sv_boot), [np.stack(w) for w in w_boot]
    sv_se, sv_ci = br.summaries(sv_boot, 0.95)
    w_sum = [br.summaries(w, 0.95) for w in w_boot]
    return SimpleNamespace(singular_values=obs.sv, singular_values_boot=sv_boot, singular_values_se=sv_se, singular_values_ci=sv_ci,
                           weights=[O1, O2], weights_boot=w_boot, weights_se=[s[0] for s in w_sum], weights_ci=[s[1] for s in w_sum])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(tb.ESTIMATORS))
def test_bootstrap_with_device_draws_matches_restatement(name, dtype):
    from cca_zoo_amd.model_selection import bootstrap

    ref = boot_reference(name, dtype)
    views = [np.array(v) for v in tb.public_views(dtype)]
    res = bootstrap(tb.ESTIMATORS[name][0](tb.PUB_K), views, n_resamples=tb.PUB_B, random_state=tb.PUB_SEED, draws="device")
    host = bootstrap(tb.ESTIMATORS[name][0](tb.PUB_K), views, n_resamples=tb.PUB_B, random_state=tb.PUB_SEED)
    e = tb.public_errors(res, ref)
    print(f"bootstrap device draws {name} {np.dtype(dtype).name}: {', '.join(f'{a} {b:.3g}' for a, b in e.items())}")
    assert e["sv"] <= tb.BAR and e["sv_boot"] <= tb.BAR and e["w"] <= tb.WBAR and e["w_boot"] <= tb.WBAR
    assert e["sv_se"] <= 4 * tb.BAR and e["sv_ci"] <= 4 * tb.BAR and e["w_se"] <= 4 * tb.WBAR and e["w_ci"] <= 4 * tb.WBAR
    np.testing.assert_array_equal(res.singular_values, host.singular_values)
    for i in range(2):
        np.testing.assert_array_equal(res.weights[i], host.weights[i])
        np.testing.assert_array_equal(res.bootstrap_ratio[i], res.weights[i] / res.weights_se[i])
    assert not np.array_equal(res.singular_values_boot, host.singular_values_boot)


def test_bootstrap_chunks_and_view_placement_do_not_change_a_bit(monkeypatch):
    import torch

    from cca_zoo_amd.linear import rCCA
    from cca_zoo_amd.model_selection import _bootstrap as bs

    def host_draw(*a, **k):
        raise AssertionError("draws='device' drew on the host")

    monkeypatch.setattr(bs, "draw_counts", host_draw)
    views = [np.array(v) for v in tb.public_views(np.float64)]
    run = lambda v: bs.bootstrap(rCCA(latent_dimensions=2, c=[0.1, 0.3]), v, n_resamples=tb.PUB_B, random_state=tb.PUB_SEED, draws="device")
    base = run(views)
    for chunk in (1, 7, tb.PUB_B):
        monkeypatch.setattr(bs, "CHUNK_RESAMPLES", chunk)
        res = run(views)
        np.testing.assert_array_equal(res.singular_values_boot, base.singular_values_boot)
        for i in range(2):
            np.testing.assert_array_equal(res.weights_boot[i], base.weights_boot[i])
            np.testing.assert_array_equal(res.weights_ci[i], base.weights_ci[i])
    res = run([torch.tensor(v, device="cuda") for v in views])
    np.testing.assert_array_equal(res.singular_values_boot, base.singular_values_boot)
    for i in range(2):
        np.testing.assert_array_equal(res.weights_boot[i], base.weights_boot[i])
