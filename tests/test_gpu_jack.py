"""``ccz_jack_rcca``, ``jackknife`` and ``bootstrap(method="BCa")`` on the device.

The bars are the family's (tests/test_gpu_boot.py): 1e-8 absolute on ``sigma / sigma_1`` and ``1e-8 / 5e-3 = 2e-6`` per weight
column up to the coupled sign, relative to the reference column's largest entry; the conditions they rest on are asserted on the
CPU by tests/test_jack_host.py for the inputs of tests/jack_cases.py.  Every replicate of every case is compared with
``ccz_boot_rcca`` on the 0/1 counts ``counts[s] = (s % J != g)`` in the same process -- the verified path, which the downdated
moments must equal in exact arithmetic -- and ``jack_cases.subset(J)`` of them with the literal NumPy refits.  The host half of
BCa (``bca_intervals``) is held to the loop of tests/jack_restatement.py on the very arrays the call returned, at 1e-12; no
end-to-end interval bar is fixed beyond that: the interval is a quantile at a level that depends on the acceleration, so its
sensitivity is the bootstrap density.  Each test prints the worst error it measured; on an MI355X they are listed in DESIGN.md
section 4s.
"""

import ctypes as C
import functools
import warnings

import numpy as np
import pytest

import boot_restatement as br
import jack_cases as jc
import jack_restatement as jr
import test_gpu_boot as tb
from test_gpu_boot import BAR, COND, WBAR, assert_conditions, errors

pytestmark = pytest.mark.gpu

RS_SCRATCH = 1 << 25                                    # csrc/resample_dev.h: RS_SCRATCH = 2^25 doubles of partials per launch group
RS_MAXBATCH = 65535                                     # csrc/resample_dev.h: RS_MAXBATCH = 65535, gridDim.y
BCA_ANCHOR = 1e-12
SE_BAR = 1e-8
EINVAL, EUNSUP = -1, -6


def launch_cap(per_item):
    """The items of one launch group, as ``for_batches`` computes it."""
    return max(1, min(RS_SCRATCH // per_item, RS_MAXBATCH))


def jack_per_item(p1, p2):
    """One folded partial per replicate, whatever ``n``: the row splits are folded once, before the downdates."""
    P1, P2 = 16 * ((p1 + 15) // 16), 16 * ((p2 + 15) // 16)
    return P1 * P1 + P1 * P2 + P2 * P2 + P1 + P2 + 1


class Device(tb.Device):
    """The (shifted) views of one case in HBM; ``jack``: one call of the entry point on them."""

    def jack(self, J, g0, ng, k):
        """(sv ng x r, W ng x (p1 + p2) x k, info ng) of replicates [g0, g0 + ng) in ONE call."""
        h, vp = self.h, C.c_void_p
        pt = self.p1 + self.p2
        sv = h.to_device(np.full((ng, self.r), -7.0))
        W = h.to_device(np.full((ng, pt, k), -7.0))
        info = h.to_device(np.full(ng, -7, dtype=np.int32))
        h.check(h.lib.ccz_jack_rcca(h.raw, self.n, self.p1, self.p2, vp(self.x1.ptr), vp(self.x2.ptr), J, g0, ng, self.c[0], self.c[1],
                                    int(self.center), k, vp(sv.ptr), vp(W.ptr), vp(info.ptr)))
        return h.to_host(sv, (ng, self.r)), h.to_host(W, (ng, pt, k)), h.to_host(info, (ng,), dtype=np.int32)


def batch_errors(sv, W, sv_ref, W_ref, p1):
    """(worst |sigma - ref| / sigma_1, worst weight-column error up to the coupled sign) of every replicate against arrays of the
    same shapes: ``errors`` of tests/test_gpu_boot.py without the loop."""
    assert np.all(np.isfinite(sv)) and np.all(np.isfinite(W)) and np.all(np.isfinite(sv_ref)) and np.all(np.isfinite(W_ref))
    assert np.all(np.diff(sv, axis=1) <= 0)
    e_sv = float(np.max(np.abs(sv - sv_ref) / sv_ref[:, :1]))
    sign = np.where(np.einsum("bij,bij->bj", W, W_ref) >= 0, 1.0, -1.0)[:, None, :]
    e_w = 0.0
    for s in (slice(0, p1), slice(p1, None)):
        e_w = max(e_w, float(np.max(np.abs(sign * W[:, s] - W_ref[:, s]) / np.max(np.abs(W_ref[:, s]), axis=1, keepdims=True))))
    return e_sv, e_w


# ---- the kernel through the C ABI ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,c,center,J", jc.CASES)
def test_replicates_match_the_counts_route_and_numpy(shape, c, center, J):
    X1, X2, reps, refs, ident, k = jc.case(shape, c, center, J)
    dev = Device(shape, c, center, X1, X2)
    sv, W, info = dev.jack(J, 0, J, k)
    assert not info.any()
    sv_c, W_c, info_c = dev.run(jc.loo_counts(shape[0], J, np.arange(J)), k)
    assert not info_c.any()
    against_counts = batch_errors(sv, W, sv_c, W_c, shape[1])
    against_numpy = errors(sv[reps], W[reps], refs, shape[1])
    print(f"jack kernels n={shape[0]} ({shape[1]}, {shape[2]}) c={c} center={center} J={J}: against the counts route (all {J}) "
          f"sigma / sigma_1 {against_counts[0]:.3g}, weights {against_counts[1]:.3g}; against NumPy ({len(reps)}) "
          f"sigma / sigma_1 {against_numpy[0]:.3g}, weights {against_numpy[1]:.3g}")
    assert against_counts[0] <= BAR and against_counts[1] <= WBAR
    assert against_numpy[0] <= BAR and against_numpy[1] <= WBAR


@pytest.mark.parametrize("shape,c,center,J", [jc.CASES[0], jc.CASES[4]])
def test_bits_do_not_depend_on_the_call(shape, c, center, J):
    X1, X2, _, _, _, k = jc.case(shape, c, center, J)
    dev = Device(shape, c, center, X1, X2)
    whole = dev.jack(J, 0, J, k)

    def same(parts):
        for got, want in zip((np.concatenate(x) for x in zip(*parts)), whole):
            np.testing.assert_array_equal(got, want)

    same([dev.jack(J, 0, J, k)])                                                     # the same call twice
    same([dev.jack(J, g, 1, k) for g in range(J)])                                   # replicate g alone
    same([dev.jack(J, g, min(7, J - g), k) for g in range(0, J, 7)])
    same([dev.jack(J, 0, J // 2, k), dev.jack(J, J // 2, J - J // 2, k)])


def test_launch_groups():
    shape, c, center, J = jc.GROUPS_CASE
    cap = launch_cap(jack_per_item(shape[1], shape[2]))
    assert cap == 41890 and J > cap
    X1, X2 = jc.views(shape)
    k = 2
    dev = Device(shape, c, center, X1, X2)
    sv, W, info = dev.jack(J, 0, J, k)
    assert not info.any() and np.all(np.isfinite(sv)) and np.all(np.isfinite(W))
    rows = np.concatenate([np.arange(0, J, 1000), [cap, J - 1]])                      # cap: the first replicate of the second group
    sv_c, W_c, info_c = dev.run(jc.loo_counts(shape[0], J, rows), k)
    assert not info_c.any()
    e_sv, e_w = batch_errors(sv[rows], W[rows], sv_c, W_c, shape[1])
    for got, want in zip(dev.jack(J, cap, J - cap, k), (sv, W, info)):                # the second group alone
        np.testing.assert_array_equal(got, want[cap:])
    ref = jr.fit_without(X1, X2, np.array([cap]), c, center, k)
    assert_conditions(ref, k)
    n_sv, n_w = errors(sv[cap:cap + 1], W[cap:cap + 1], [ref], shape[1])
    print(f"jack launch groups n={shape[0]} ({shape[1]}, {shape[2]}) {J} replicates, cap {cap}: against the counts route ({len(rows)}) "
          f"sigma / sigma_1 {e_sv:.3g}, weights {e_w:.3g}; replicate {cap} against NumPy {n_sv:.3g}, {n_w:.3g}")
    assert e_sv <= BAR and e_w <= WBAR and n_sv <= BAR and n_w <= WBAR


def test_info_codes_and_nan_rows():
    from cca_zoo_amd.linear import CCA, rCCA
    from cca_zoo_amd.model_selection import jackknife

    shape = (60, 5, 3)
    X1, X2 = (np.array(v) for v in jc.views(shape))
    X1[:, 2] = 0.0                                        # an exact zero column: the pivot of R_1 (c = 0) is exactly 0 in every replicate
    dev = Device(shape, 0.0, True, X1, X2)
    for J in (60, 7):
        sv, W, info = dev.jack(J, 0, J, 2)
        assert np.all((info == 1) | (info == 2)) and np.all(np.isnan(sv)) and np.all(np.isnan(W))
    with pytest.raises(np.linalg.LinAlgError, match=r"R_[12] .*c > 0"):
        jackknife(CCA(latent_dimensions=2), [X1, X2])
    res = jackknife(rCCA(latent_dimensions=2, c=0.5), [X1, X2])                      # the remedy: c > 0
    assert np.all(np.isfinite(res.singular_values_jack)) and res.n_groups == 60


def test_jackknife_names_the_replicate(monkeypatch):
    from cca_zoo_amd.linear import CCA
    from cca_zoo_amd.model_selection import _jackknife as jk

    X1, X2 = jc.views((60, 5, 3))
    run = jk.run_replicates

    def spoiled(*a):
        sv, W, info = run(*a)
        info[4] = 2
        return sv, W, info

    monkeypatch.setattr(jk, "run_replicates", spoiled)
    with pytest.raises(np.linalg.LinAlgError, match=r"jackknife: replicate 4: R_2 .*c > 0"):
        jk.jackknife(CCA(), [np.array(X1), np.array(X2)], n_groups=10)


def test_entry_point_refuses_what_it_cannot_do():
    X1, X2 = jc.views((60, 5, 3))
    dev = Device((60, 5, 3), 0.0, True, X1, X2)
    h, vp = dev.h, C.c_void_p
    f = h.lib.ccz_jack_rcca
    x = (vp(dev.x1.ptr), vp(dev.x2.ptr))
    sv, W, info = h.alloc(64 * 64 * 8), h.alloc(64 * 128 * 64 * 8), h.alloc(64 * 4)
    out = (vp(sv.ptr), vp(W.ptr), vp(info.ptr))
    tail = (0.0, 0.0, 1, 2)                                # c1, c2, center, k
    assert f(h.raw, 60, 5, 3, *x, 60, 0, 60, *tail, *out) == 0
    assert f(h.raw, 60, 5, 3, *x, 7, 5, 2, *tail, *out) == 0
    assert f(h.raw, 60, 65, 3, *x, 60, 0, 1, *tail, *out) == EUNSUP
    assert f(h.raw, 60, 5, 65, *x, 60, 0, 1, *tail, *out) == EUNSUP
    assert f(h.raw, 2 ** 31, 5, 3, *x, 60, 0, 1, *tail, *out) == EUNSUP
    assert f(h.raw, 0, 5, 3, *x, 60, 0, 1, *tail, *out) == EINVAL
    assert f(h.raw, 60, 0, 3, *x, 60, 0, 1, *tail, *out) == EINVAL
    assert f(h.raw, 60, 5, 0, *x, 60, 0, 1, *tail, *out) == EINVAL
    assert f(h.raw, 60, 5, 3, *x, 1, 0, 1, *tail, *out) == EINVAL                  # ngroups < 2
    assert f(h.raw, 60, 5, 3, *x, 61, 0, 1, *tail, *out) == EINVAL                 # ngroups > n
    assert f(h.raw, 60, 5, 3, *x, 60, -1, 1, *tail, *out) == EINVAL                # g0 < 0
    assert f(h.raw, 60, 5, 3, *x, 60, 0, 0, *tail, *out) == EINVAL                 # ng < 1
    assert f(h.raw, 60, 5, 3, *x, 60, 58, 3, *tail, *out) == EINVAL                # g0 + ng > ngroups
    assert f(h.raw, 60, 5, 3, *x, 60, 60, 1, *tail, *out) == EINVAL
    assert f(h.raw, 60, 5, 3, *x, 60, 0, 1, 0.0, 0.0, 1, 0, *out) == EINVAL        # k < 1
    assert f(h.raw, 60, 5, 3, *x, 60, 0, 1, 0.0, 0.0, 1, 4, *out) == EINVAL        # k > r
    assert f(h.raw, 60, 5, 3, None, x[1], 60, 0, 1, *tail, *out) == EINVAL
    assert f(h.raw, 60, 5, 3, x[0], None, 60, 0, 1, *tail, *out) == EINVAL
    assert f(h.raw, 60, 5, 3, *x, 60, 0, 1, *tail, None, out[1], out[2]) == EINVAL
    assert f(h.raw, 60, 5, 3, *x, 60, 0, 1, *tail, out[0], None, out[2]) == EINVAL
    assert f(h.raw, 60, 5, 3, *x, 60, 0, 1, *tail, out[0], out[1], None) == EINVAL
    h.sync()


# ---- the public functions -----------------------------------------------------------------------------------------------------
PUB_N, PUB_P, PUB_B, PUB_K, PUB_SEED = tb.PUB_N, tb.PUB_P, tb.PUB_B, tb.PUB_K, tb.PUB_SEED
ESTIMATORS = tb.ESTIMATORS
JACK_FIELDS = ["sv", "sv_jack", "w", "w_jack"]


def check_conditions(ref):
    assert np.max(ref.cond) <= COND
    rows = [ref.singular_values] + list(ref.singular_values_jack) + list(getattr(ref, "singular_values_boot", []))
    for sv in rows:
        assert_conditions(br.SimpleNamespace(sv=sv, cond=(1.0, 1.0)), PUB_K)


@functools.lru_cache(maxsize=None)
def jack_reference(name, dtype, J):
    _, c, center = ESTIMATORS[name]
    ref = jr.jackknife(tb.public_views(dtype), c=c, center=center, k=PUB_K, J=J)   # float32: widened first
    check_conditions(ref)
    return ref


@functools.lru_cache(maxsize=None)
def bca_reference(name, dtype, J):
    _, c, center = ESTIMATORS[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ref = jr.restate_bca(tb.public_views(dtype), c=c, center=center, k=PUB_K, n_resamples=PUB_B, random_state=PUB_SEED, J=J)
    check_conditions(ref)
    return ref


def value_errors(res, ref):
    """The observed and the jackknife values against the restatement, each at its bar's scale."""
    s1 = ref.singular_values[0]
    scale = [np.max(np.abs(w), axis=0) for w in ref.weights]
    return {"sv": float(np.max(np.abs(res.singular_values - ref.singular_values)) / s1),
            "sv_jack": float(np.max(np.abs(res.singular_values_jack - ref.singular_values_jack) / ref.singular_values_jack[:, :1])),
            "w": max(float(np.max(np.abs(a - b) / s)) for a, b, s in zip(res.weights, ref.weights, scale)),
            "w_jack": max(float(np.max(np.abs(a - b) / np.max(np.abs(b), axis=1, keepdims=True)))
                          for a, b in zip(res.weights_jack, ref.weights_jack))}


def assert_values(e):
    assert e["sv"] <= BAR and e["sv_jack"] <= BAR and e["w"] <= WBAR and e["w_jack"] <= WBAR, e


def as_views(dtype, where):
    import torch

    views = [np.array(v) for v in tb.public_views(dtype)]
    return [torch.tensor(v, device="cuda") for v in views] if where == "cuda" else views


@pytest.mark.parametrize("J", [PUB_N, 16])
@pytest.mark.parametrize("where", ["host", "cuda"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(ESTIMATORS))
def test_jackknife_matches_restatement(name, dtype, where, J):
    from cca_zoo_amd.model_selection import JackknifeResult, jackknife

    ref = jack_reference(name, dtype, J)
    est = ESTIMATORS[name][0](PUB_K)
    res = jackknife(est, as_views(dtype, where), n_groups=J)
    assert isinstance(res, JackknifeResult) and not hasattr(est, "weights_") and res.n_groups == J
    r, k = min(PUB_P), PUB_K
    assert res.singular_values.shape == (r,) and res.singular_values_jack.shape == (J, r)
    assert res.singular_values_se.shape == (r,) and res.singular_values_bias.shape == (r,)
    for i, p in enumerate(PUB_P):
        assert res.weights[i].shape == (p, k) and res.weights_jack[i].shape == (J, p, k)
        assert res.weights_se[i].shape == (p, k) and res.weights_bias[i].shape == (p, k)
    e = value_errors(res, ref)
    e["sv_se"] = float(np.max(np.abs(res.singular_values_se - ref.singular_values_se) / ref.singular_values_se))
    e["sv_bias"] = float(np.max(np.abs(res.singular_values_bias - ref.singular_values_bias) / ref.singular_values_se))
    e["w_se"] = max(float(np.max(np.abs(a - b) / b)) for a, b in zip(res.weights_se, ref.weights_se))
    e["w_bias"] = max(float(np.max(np.abs(a - b) / s)) for a, b, s in zip(res.weights_bias, ref.weights_bias, ref.weights_se))
    sv_fit = np.asarray(res.estimator.singular_values_, dtype=np.float64)
    print(f"jackknife {name} {np.dtype(dtype).name} {where} J={J}: {', '.join(f'{a} {b:.3g}' for a, b in e.items())}")
    assert_values(e)
    assert max(e["sv_se"], e["sv_bias"], e["w_se"], e["w_bias"]) <= SE_BAR, e
    assert sv_fit.shape == (k,) and len(res.estimator.weights_) == 2


def test_default_groups():
    from cca_zoo_amd.linear import rCCA
    from cca_zoo_amd.model_selection import jackknife

    views = as_views(np.float64, "host")
    res = jackknife(rCCA(latent_dimensions=PUB_K, c=[0.1, 0.3]), views)              # None: min(n, 4096) = n, leave-one-out
    same = jackknife(rCCA(latent_dimensions=PUB_K, c=[0.1, 0.3]), views, n_groups=PUB_N)
    assert res.n_groups == PUB_N
    np.testing.assert_array_equal(res.singular_values_jack, same.singular_values_jack)
    np.testing.assert_array_equal(res.weights_jack[1], same.weights_jack[1])


INHERITED = ["singular_values", "singular_values_boot", "singular_values_se", "weights", "weights_boot", "weights_se", "bootstrap_ratio"]


def assert_same(a, b):
    if isinstance(a, list):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    else:
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("draws,J", [("numpy", None), ("device", None), ("numpy", 16)])
@pytest.mark.parametrize("where", ["host", "cuda"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(ESTIMATORS))
def test_bca_bootstrap(name, dtype, where, draws, J):
    from cca_zoo_amd.model_selection import BCaBootstrapResult, BootstrapResult, bca_intervals, bootstrap

    groups = PUB_N if J is None else J
    views = as_views(dtype, where)
    with warnings.catch_warnings():                       # (with B = 50 an observed weight may lie outside its bootstrap values)
        warnings.simplefilter("ignore", RuntimeWarning)
        res = bootstrap(ESTIMATORS[name][0](PUB_K), views, n_resamples=PUB_B, random_state=PUB_SEED, draws=draws, method="BCa",
                        jackknife_groups=J)
    plain = bootstrap(ESTIMATORS[name][0](PUB_K), views, n_resamples=PUB_B, random_state=PUB_SEED, draws=draws)
    assert isinstance(res, BCaBootstrapResult) and isinstance(res, BootstrapResult) and type(plain) is BootstrapResult
    assert res.n_groups == groups and res.singular_values_jack.shape == (groups, min(PUB_P))
    # the percentile call's fields, bit for bit
    for f in INHERITED:
        assert_same(getattr(res, f), getattr(plain, f))
    assert_same(res.singular_values_ci_percentile, plain.singular_values_ci)
    assert_same(res.weights_ci_percentile, plain.weights_ci)
    # the device's arrays against the restatement (the resamples of draws="device" are the device's own: the jackknife only)
    ref = bca_reference(name, dtype, groups) if draws == "numpy" else jack_reference(name, dtype, groups)
    e = value_errors(res, ref)
    if draws == "numpy":
        e.update({f: v for f, v in tb.public_errors(res, ref).items() if f in ("sv_boot", "w_boot")})
        assert e["sv_boot"] <= BAR and e["w_boot"] <= WBAR, e
    assert_values(e)
    # the host half on the very arrays that were returned: exactly the package's function, and the loop at 1e-12
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = [(res.singular_values_ci, res.singular_values_z0, res.singular_values_acceleration)]
        got += list(zip(res.weights_ci, res.weights_z0, res.weights_acceleration))
        args = [(res.singular_values, res.singular_values_boot, res.singular_values_jack)]
        args += list(zip(res.weights, res.weights_boot, res.weights_jack))
        worst = 0.0
        for (ci, z0, a), (theta, boot, jack) in zip(got, args):
            again = bca_intervals(theta, boot, jack, 0.95)
            for x, y in zip((ci, z0, a), again):
                np.testing.assert_array_equal(x, y)        # (NaN equals NaN here)
            loop = jr.bca_all(theta, boot, jack, 0.95)
            np.testing.assert_array_equal(np.isnan(ci), np.isnan(loop[0]))
            ok = ~np.isnan(ci)
            if ok.any():
                worst = max(worst, float(np.max(np.abs(ci[ok] - loop[0][ok]))))
            fin = np.isfinite(z0) & np.isfinite(a)
            worst = max(worst, float(np.max(np.abs(z0[fin] - loop[1][fin]))), float(np.max(np.abs(a[fin] - loop[2][fin]))))
    assert np.all(np.isfinite(res.singular_values_ci[:, :PUB_K]))
    print(f"bootstrap BCa {name} {np.dtype(dtype).name} {where} draws={draws} J={groups}: {', '.join(f'{a} {b:.3g}' for a, b in e.items())}, "
          f"intervals against the loop {worst:.3g}")
    assert worst <= BCA_ANCHOR


# ---- what BCa is for ----------------------------------------------------------------------------------------------------------
def test_bca_corrects_the_upward_bias_of_the_first_correlation():
    """The sample canonical correlation is biased upward, so its bootstrap values sit above it more often than below
    (z0 < 0) and the BCa interval reaches further down than the percentile interval."""
    from cca_zoo_amd.linear import CCA
    from cca_zoo_amd.model_selection import bootstrap

    X1, X2 = tb.stat_views()

    def properties(r):
        lo, hi = r.singular_values_ci[:, 0]
        plo, phi = r.singular_values_ci_percentile[:, 0]
        return bool(lo <= r.singular_values[0] <= hi), bool(plo <= r.singular_values[0] <= phi), bool(lo < plo)

    ref = jr.restate_bca([X1, X2], c=0.0, k=1, n_resamples=1000, random_state=0)
    assert properties(ref) == (True, True, True), "broken test: the restatement itself does not show the property"
    res = bootstrap(CCA(latent_dimensions=1), [X1, X2], n_resamples=1000, random_state=0, method="BCa")
    print(f"planted pair: sigma_1 {res.singular_values[0]:.4f}, BCa {res.singular_values_ci[:, 0]}, percentile "
          f"{res.singular_values_ci_percentile[:, 0]}, z0 {res.singular_values_z0[0]:.3f}, a {res.singular_values_acceleration[0]:.4f}")
    assert properties(res) == (True, True, True)
    assert res.n_groups == 400
