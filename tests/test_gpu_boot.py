"""``ccz_boot_rcca`` and ``bootstrap`` on the device against tests/boot_restatement.py (float64 NumPy).

Singular values: the family's device bar, 1e-8, absolute on ``sigma / sigma_1``.  Weights: per column up to the coupled sign,
relative to the largest entry of the reference column in that view, at ``1e-8 / GAP = 2e-6`` with ``GAP = 5e-3``: a singular
vector's error is the matrix error divided by the gap.  Conditioning is a condition of the inputs, not a measurement: the NumPy
side asserts ``cond(R_i^b) <= 1e4`` for every resample and that every compared ``sigma_j`` (``j <= k``, including against
``sigma_{k+1}``) is at least ``GAP sigma_1`` away from its neighbours.  Every resample of a case is compared.  The generator:
two planted pairs with population correlations (0.95, 0.75) on the first two columns of unit-Gaussian noise, each view mixed by
``M = (Q linspace(1, 3, p)) Q'`` with a random orthogonal ``Q``, plus a random column offset.  Each test prints the worst error
it measured; on an MI355X they are listed in DESIGN.md section 4s.
"""

import ctypes as C
import functools

import numpy as np
import pytest

import boot_restatement as br

pytestmark = pytest.mark.gpu

BAR = 1e-8
GAP = 5e-3
WBAR = BAR / GAP
COND = 1e4
NBOOT = 100


def _rows_per_split():
    from cca_zoo_amd.model_selection import _bootstrap as bs

    return bs.ROWS_PER_SPLIT


def _shapes():
    return [(60, 5, 3), (2000, 64, 64), (1000, 17, 64), (300, 64, 1), (_rows_per_split() + 5, 16, 16)]


def _handle():
    from cca_zoo_amd import _backend

    return _backend.default_handle(0)


def planted_views(n, p1, p2, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, 2))
    X1, X2 = rng.standard_normal((n, p1)), rng.standard_normal((n, p2))
    for j, rho in enumerate((0.95, 0.75)[: min(2, p1, p2)]):
        X2[:, j] = rho * z[:, j] + np.sqrt(1.0 - rho * rho) * X2[:, j]
        X1[:, j] = z[:, j]
    out = []
    for X in (X1, X2):
        p = X.shape[1]
        Q, _ = np.linalg.qr(rng.standard_normal((p, p)))
        out.append(np.ascontiguousarray(X @ ((Q * np.linspace(1.0, 3.0, p)) @ Q.T) + rng.standard_normal(p)))
    for a in out:
        a.setflags(write=False)
    return out


def assert_conditions(fit, k):
    """What the bars rest on, asserted on the NumPy reference of one resample."""
    assert max(fit.cond) <= COND, f"broken test: cond(R_i) = {fit.cond}"
    sv = fit.sv
    for j in range(k):
        for nb in (j - 1, j + 1):
            if 0 <= nb < len(sv):
                assert abs(sv[j] - sv[nb]) >= GAP * sv[0], f"broken test: sigma_{j} and sigma_{nb} are closer than GAP sigma_1: {sv}"


# (shape, c, center, 0/1 multiplicities)
PLAIN = [(s, 0.0, True, False) for s in _shapes()]
EXTRA = [((1000, 17, 64), (0.1, 0.3), True, False), ((2000, 64, 64), 0.2, False, False), ((2000, 64, 64), 0.0, True, True)]


@functools.lru_cache(maxsize=None)
def case(shape, c, center, subsample):
    """Inputs and NumPy references of one case, computed once: the views, NBOOT multiplicity vectors (int32) and the refits."""
    n, p1, p2 = shape
    X1, X2 = planted_views(n, p1, p2, seed=1000 + n + p1)
    rng = np.random.default_rng(n + p2)
    if subsample:
        counts = (rng.random((NBOOT, n)) < 0.5).astype(np.int32)
    else:
        counts = np.stack([np.bincount(rng.integers(0, n, size=n), minlength=n) for _ in range(NBOOT)]).astype(np.int32)
    k = min(p1, p2, 2)
    cc = list(c) if isinstance(c, tuple) else c
    refs = [br.fit_counts(X1, X2, m, cc, center, k) for m in counts]
    for f in refs:
        assert_conditions(f, k)
    ident = br.fit_rows(X1, X2, cc, center, k)
    assert_conditions(ident, k)
    counts.setflags(write=False)
    return X1, X2, counts, refs, ident, k


class Device:
    """The (shifted) views of one case in HBM and calls of the entry point on them."""

    def __init__(self, shape, c, center, X1, X2):
        self.h = _handle()
        self.n, self.p1, self.p2 = shape
        self.r = min(self.p1, self.p2)
        self.c = list(c) if isinstance(c, tuple) else [c, c]
        self.center = center
        # what the Python side passes: X_i - 1 mu_i' with the full-sample mean when centring, the views as they are otherwise
        self.x1 = self.h.to_device(X1 - X1.mean(axis=0) if center else X1)
        self.x2 = self.h.to_device(X2 - X2.mean(axis=0) if center else X2)

    def run(self, counts, k):
        """(sv nboot x r, W nboot x (p1 + p2) x k, info nboot) of ``counts`` (nboot x n int32, or None = all ones) in ONE call."""
        h, vp = self.h, C.c_void_p
        nboot = 1 if counts is None else int(counts.shape[0])
        cd = None if counts is None else h.to_device(np.ascontiguousarray(counts, dtype=np.int32))
        pt = self.p1 + self.p2
        sv = h.to_device(np.full((nboot, self.r), -7.0))
        W = h.to_device(np.full((nboot, pt, k), -7.0))
        info = h.to_device(np.full(nboot, -7, dtype=np.int32))
        h.check(h.lib.ccz_boot_rcca(h.raw, self.n, self.p1, self.p2, vp(self.x1.ptr), vp(self.x2.ptr),
                                    vp(cd.ptr) if cd is not None else None, nboot, self.c[0], self.c[1], int(self.center), k,
                                    vp(sv.ptr), vp(W.ptr), vp(info.ptr)))
        return h.to_host(sv, (nboot, self.r)), h.to_host(W, (nboot, pt, k)), h.to_host(info, (nboot,), dtype=np.int32)


def errors(sv, W, refs, p1):
    """(worst |sigma - ref| / sigma_1, worst weight-column error up to the coupled sign) over all resamples."""
    e_sv = e_w = 0.0
    assert np.all(np.isfinite(sv)) and np.all(np.isfinite(W))
    assert np.all(np.diff(sv, axis=1) <= 0)                # descending
    for b, f in enumerate(refs):
        e_sv = max(e_sv, float(np.max(np.abs(sv[b] - f.sv)) / f.sv[0]))
        e_w = max(e_w, weight_error([W[b, :p1], W[b, p1:]], f.weights))
    return e_sv, e_w


def weight_error(got, ref):
    worst = 0.0
    for j in range(ref[0].shape[1]):
        sign = 1.0 if sum(float(g[:, j] @ w[:, j]) for g, w in zip(got, ref)) >= 0 else -1.0
        for g, w in zip(got, ref):
            worst = max(worst, float(np.max(np.abs(sign * g[:, j] - w[:, j])) / np.max(np.abs(w[:, j]))))
    return worst


@pytest.mark.parametrize("shape,c,center,subsample", PLAIN + EXTRA)
def test_kernels_match_numpy(shape, c, center, subsample):
    X1, X2, counts, refs, ident, k = case(shape, c, center, subsample)
    dev = Device(shape, c, center, X1, X2)
    sv, W, info = dev.run(counts, k)
    assert not info.any()
    if subsample:
        assert np.all(counts.sum(axis=1) != shape[0])      # N_b != n: the divisor is the resample's
    batch = errors(sv, W, refs, shape[1])
    sv1, W1, info1 = dev.run(None, k)
    assert not info1.any()
    one = errors(sv1, W1, [ident], shape[1])
    print(f"boot kernels n={shape[0]} ({shape[1]}, {shape[2]}) c={c} center={center} subsample={subsample}: "
          f"worst |sigma - ref| / sigma_1 = {max(batch[0], one[0]):.3g}, worst weight error = {max(batch[1], one[1]):.3g}")
    assert max(batch[0], one[0]) <= BAR and max(batch[1], one[1]) <= WBAR


@pytest.mark.parametrize("shape", _shapes())
def test_bit_identity(shape):
    X1, X2, counts, _, _, k = case(shape, 0.0, True, False)
    dev = Device(shape, 0.0, True, X1, X2)
    whole = dev.run(counts, k)

    def same(parts):
        for got, want in zip((np.concatenate(x) for x in zip(*parts)), whole):
            np.testing.assert_array_equal(got, want)

    same([dev.run(counts, k)])                                                      # the same call twice
    same([dev.run(counts[b:b + 64], k) for b in range(0, NBOOT, 64)])
    same([dev.run(counts[b:b + 1], k) for b in range(NBOOT)])                       # resample b alone
    ones = np.ones((1, shape[0]), dtype=np.int32)
    for got, want in zip(dev.run(ones, k), dev.run(None, k)):                       # NULL is all ones
        np.testing.assert_array_equal(got, want)


def test_entry_point_refuses_shapes_outside_the_limits():
    X1, X2 = planted_views(60, 5, 3, seed=1)
    dev = Device((60, 5, 3), 0.0, True, X1, X2)
    h, vp = dev.h, C.c_void_p
    f = h.lib.ccz_boot_rcca
    x = (vp(dev.x1.ptr), vp(dev.x2.ptr))
    sv, W, info = h.alloc(64 * 8), h.alloc(128 * 64 * 8), h.alloc(64)
    out = (vp(sv.ptr), vp(W.ptr), vp(info.ptr))
    assert f(h.raw, 60, 5, 3, *x, None, 1, 0.0, 0.0, 1, 2, *out) == 0
    assert f(h.raw, 60, 65, 3, *x, None, 1, 0.0, 0.0, 1, 2, *out) == -6          # CCZ_EUNSUP
    assert f(h.raw, 60, 5, 65, *x, None, 1, 0.0, 0.0, 1, 2, *out) == -6
    assert f(h.raw, 2 ** 31, 5, 3, *x, None, 1, 0.0, 0.0, 1, 2, *out) == -6
    assert f(h.raw, 60, 5, 3, *x, None, 2, 0.0, 0.0, 1, 2, *out) == -1           # CCZ_EINVAL: all ones is one resample
    assert f(h.raw, 60, 5, 0, *x, None, 1, 0.0, 0.0, 1, 2, *out) == -1
    assert f(h.raw, 0, 5, 3, *x, None, 1, 0.0, 0.0, 1, 2, *out) == -1
    assert f(h.raw, 60, 5, 3, *x, None, 0, 0.0, 0.0, 1, 2, *out) == -1
    assert f(h.raw, 60, 5, 3, *x, None, 1, 0.0, 0.0, 1, 0, *out) == -1
    assert f(h.raw, 60, 5, 3, *x, None, 1, 0.0, 0.0, 1, 4, *out) == -1           # k > r
    assert f(h.raw, 60, 5, 3, None, x[1], None, 1, 0.0, 0.0, 1, 2, *out) == -1
    assert f(h.raw, 60, 5, 3, *x, None, 1, 0.0, 0.0, 1, 2, out[0], None, out[2]) == -1
    assert f(h.raw, 60, 5, 3, *x, None, 1, 0.0, 0.0, 1, 2, out[0], out[1], None) == -1
    h.sync()


def degenerate_counts(n):
    """Fewer distinct rows than columns, and an exact zero: 64 copies of row 0 alone.  Scaling by 64 is exact, so
    ``G - s s' / N`` is exactly zero and the first pivot of ``R_1`` (c = 0) is exactly 0 -- a numerical outcome, nothing faults."""
    m = np.zeros((1, n), dtype=np.int32)
    m[0, 0] = 64
    return m


def test_info_codes_and_nan_rows():
    shape = (60, 5, 3)
    X1, X2, counts, refs, _, k = case(shape, 0.0, True, False)
    dev = Device(shape, 0.0, True, X1, X2)
    mixed = np.concatenate([counts[:1], degenerate_counts(60), counts[1:2], np.eye(1, 60, 3, dtype=np.int32)])
    sv, W, info = dev.run(mixed, k)
    assert info[0] == 0 and info[2] == 0 and info[1] in (1, 2) and info[3] == 3      # one row drawn once: N_b < 2
    for b in (1, 3):
        assert np.all(np.isnan(sv[b])) and np.all(np.isnan(W[b]))
    e = errors(sv[[0, 2]], W[[0, 2]], refs[:2], 5)                                   # the neighbours of a refused resample are whole
    assert e[0] <= BAR and e[1] <= WBAR
    ridge = Device(shape, 0.5, True, X1, X2)                                         # the remedy: c > 0
    assert ridge.run(degenerate_counts(60), k)[2][0] == 0


def test_bootstrap_turns_info_into_linalg_error(monkeypatch):
    from cca_zoo_amd.linear import CCA, rCCA
    from cca_zoo_amd.model_selection import _bootstrap as bs

    X1, X2 = (np.array(v) for v in case((60, 5, 3), 0.0, True, False)[:2])

    def draw(rng, n, count):
        out = bs_draw(rng, n, count)
        out[-1] = degenerate_counts(n)[0]
        return out

    bs_draw = bs.draw_counts
    monkeypatch.setattr(bs, "draw_counts", draw)
    monkeypatch.setattr(bs, "CHUNK_RESAMPLES", 4)
    with pytest.raises(np.linalg.LinAlgError, match=r"resample 3: R_[12] .*c > 0"):
        bs.bootstrap(CCA(), [X1, X2], n_resamples=6, random_state=0)
    res = bs.bootstrap(rCCA(c=0.5), [X1, X2], n_resamples=6, random_state=0)
    assert np.all(np.isfinite(res.singular_values_boot))


# ---- the public function --------------------------------------------------------------------------------------------------
PUB_N, PUB_P, PUB_B, PUB_K, PUB_SEED = 200, (12, 7), 50, 2, 3
ESTIMATORS = {
    "cca": (lambda ld: _linear().CCA(latent_dimensions=ld), 0.0, True),
    "rcca": (lambda ld: _linear().rCCA(latent_dimensions=ld, c=[0.1, 0.3]), [0.1, 0.3], True),
    "pls": (lambda ld: _linear().PLS(latent_dimensions=ld), 1.0, True),
    "uncentred": (lambda ld: _linear().rCCA(latent_dimensions=ld, c=0.2, center=False), 0.2, False),
}


def _linear():
    import cca_zoo_amd.linear as lin

    return lin


@functools.lru_cache(maxsize=None)
def public_views(dtype):
    views = [np.ascontiguousarray(v, dtype=dtype) for v in planted_views(PUB_N, PUB_P[0], PUB_P[1], seed=21)]
    for v in views:
        v.setflags(write=False)
    return views


@functools.lru_cache(maxsize=None)
def public_reference(name, dtype):
    _, c, center = ESTIMATORS[name]
    views = public_views(dtype)                             # float32: widened first
    ref = br.restate(views, c=c, center=center, k=PUB_K, n_resamples=PUB_B, random_state=PUB_SEED)
    assert np.max(ref.cond) <= COND
    for sv in [ref.singular_values] + list(ref.singular_values_boot):
        assert_conditions(br.SimpleNamespace(sv=sv, cond=(1.0, 1.0)), PUB_K)
    return ref


def public_errors(res, ref):
    s1 = ref.singular_values[0]
    scale = [np.max(np.abs(w), axis=0) for w in ref.weights]                          # per view and column
    e = {"sv": float(np.max(np.abs(res.singular_values - ref.singular_values)) / s1),
         "sv_boot": float(np.max(np.abs(res.singular_values_boot - ref.singular_values_boot) / ref.singular_values_boot[:, :1])),
         "sv_se": float(np.max(np.abs(res.singular_values_se - ref.singular_values_se)) / s1),
         "sv_ci": float(np.max(np.abs(res.singular_values_ci - ref.singular_values_ci)) / s1),
         "w": max(float(np.max(np.abs(a - b) / s)) for a, b, s in zip(res.weights, ref.weights, scale)),
         "w_boot": max(float(np.max(np.abs(a - b) / np.max(np.abs(b), axis=1, keepdims=True)))
                       for a, b in zip(res.weights_boot, ref.weights_boot)),
         "w_se": max(float(np.max(np.abs(a - b) / s)) for a, b, s in zip(res.weights_se, ref.weights_se, scale)),
         "w_ci": max(float(np.max(np.abs(a - b) / s)) for a, b, s in zip(res.weights_ci, ref.weights_ci, scale))}
    return e


@pytest.mark.parametrize("where", ["host", "cuda"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(ESTIMATORS))
def test_bootstrap_matches_restatement(name, dtype, where):
    import torch

    from cca_zoo_amd.model_selection import BootstrapResult, bootstrap

    ref = public_reference(name, dtype)
    views = [np.array(v) for v in public_views(dtype)]
    if where == "cuda":
        views = [torch.tensor(v, device="cuda") for v in views]
    est = ESTIMATORS[name][0](PUB_K)
    res = bootstrap(est, views, n_resamples=PUB_B, random_state=PUB_SEED)
    assert isinstance(res, BootstrapResult) and not hasattr(est, "weights_")
    r, k, B = min(PUB_P), PUB_K, PUB_B
    assert res.singular_values.shape == (r,) and res.singular_values_boot.shape == (B, r)
    assert res.singular_values_se.shape == (r,) and res.singular_values_ci.shape == (2, r)
    for i, p in enumerate(PUB_P):
        assert res.weights[i].shape == (p, k) and res.weights_boot[i].shape == (B, p, k) and res.weights_se[i].shape == (p, k)
        assert res.weights_ci[i].shape == (2, p, k) and res.bootstrap_ratio[i].shape == (p, k)
        np.testing.assert_array_equal(res.bootstrap_ratio[i], res.weights[i] / res.weights_se[i])
    e = public_errors(res, ref)
    sv_fit = np.asarray(res.estimator.singular_values_, dtype=np.float64)
    e_fit = float(np.max(np.abs(sv_fit[:k] - res.singular_values[:k])) / res.singular_values[0])
    print(f"bootstrap {name} {np.dtype(dtype).name} {where}: {', '.join(f'{a} {b:.3g}' for a, b in e.items())}, fitted estimator {e_fit:.3g}")
    assert e["sv"] <= BAR and e["sv_boot"] <= BAR and e["w"] <= WBAR and e["w_boot"] <= WBAR
    assert e["sv_se"] <= 4 * BAR and e["sv_ci"] <= 4 * BAR and e["w_se"] <= 4 * WBAR and e["w_ci"] <= 4 * WBAR
    assert sv_fit.shape == (k,) and len(res.estimator.weights_) == 2
    # the ordinary fit of float32 views runs K1 on the float32 matrix pipe (unit roundoff 6e-8): the bar applies to float64 views
    assert e_fit <= (BAR if dtype == np.float64 else 1e-5)


def test_chunk_length_does_not_change_a_bit(monkeypatch):
    from cca_zoo_amd.linear import rCCA
    from cca_zoo_amd.model_selection import _bootstrap as bs

    views = [np.array(v) for v in public_views(np.float64)]
    base = bs.bootstrap(rCCA(latent_dimensions=2, c=[0.1, 0.3]), views, n_resamples=PUB_B, random_state=PUB_SEED)
    for chunk in (1, 7, PUB_B):
        monkeypatch.setattr(bs, "CHUNK_RESAMPLES", chunk)
        res = bs.bootstrap(rCCA(latent_dimensions=2, c=[0.1, 0.3]), views, n_resamples=PUB_B, random_state=PUB_SEED)
        np.testing.assert_array_equal(res.singular_values_boot, base.singular_values_boot)
        np.testing.assert_array_equal(res.singular_values, base.singular_values)
        for i in range(2):
            np.testing.assert_array_equal(res.weights_boot[i], base.weights_boot[i])
            np.testing.assert_array_equal(res.weights[i], base.weights[i])
            np.testing.assert_array_equal(res.weights_ci[i], base.weights_ci[i])


@pytest.mark.parametrize("name", ["cca", "rcca"])
def test_resamples_equal_refits_by_the_existing_solver(name):
    """Another route to the same numbers, by code that predates the bootstrap: refit on [X1[idx], X2[idx]]."""
    from cca_zoo_amd.model_selection import bootstrap

    views = [np.array(v) for v in public_views(np.float64)]
    ref = public_reference(name, np.float64)                # (its conditions hold for these very resamples)
    res = bootstrap(ESTIMATORS[name][0](PUB_K), views, n_resamples=5, random_state=PUB_SEED)
    rng = np.random.default_rng(PUB_SEED)
    e_sv = e_w = 0.0
    for b in range(5):
        ix = rng.integers(0, PUB_N, size=PUB_N)
        np.testing.assert_array_equal(ix, ref.idx[b])
        fit = ESTIMATORS[name][0](PUB_K).fit([views[0][ix], views[1][ix]])
        sv = np.asarray(fit.singular_values_, dtype=np.float64)
        e_sv = max(e_sv, float(np.max(np.abs(sv - res.singular_values_boot[b, :PUB_K])) / res.singular_values_boot[b, 0]))
        W = br.orient_to(np.asarray(fit.weights_[0], dtype=np.float64), np.asarray(fit.weights_[1], dtype=np.float64), *res.weights)
        e_w = max(e_w, weight_error(W, [w[b] for w in res.weights_boot]))
        for got, want in zip(W, [w[b] for w in res.weights_boot]):                    # sign-aligned: no sign left to choose
            assert np.max(np.abs(got - want) / np.max(np.abs(want), axis=0)) <= WBAR
    print(f"bootstrap {name} against refits: singular values {e_sv:.3g}, weights {e_w:.3g}")
    assert e_sv <= BAR and e_w <= WBAR


STAT_SEED = 5


def stat_views():
    """One strong component on the first column of each view, the other columns pure noise."""
    rng = np.random.default_rng(STAT_SEED)
    n = 400
    z = rng.standard_normal(n)
    X1, X2 = rng.standard_normal((n, 6)), rng.standard_normal((n, 4))
    X1[:, 0] = z + 0.3 * X1[:, 0]
    X2[:, 0] = z + 0.3 * X2[:, 0]
    return X1, X2


def stat_properties(res):
    lo, hi = res.singular_values_ci[:, 0]
    inside = lo <= res.singular_values[0] <= hi
    planted = min(abs(res.bootstrap_ratio[0][0, 0]), abs(res.bootstrap_ratio[1][0, 0]))
    noise = np.median(np.abs(np.concatenate([res.bootstrap_ratio[0][1:, 0], res.bootstrap_ratio[1][1:, 0]])))
    return bool(inside), float(planted), float(noise)


def test_planted_component_is_stable():
    from cca_zoo_amd.linear import CCA
    from cca_zoo_amd.model_selection import bootstrap

    X1, X2 = stat_views()
    ref = br.restate([X1, X2], c=0.0, k=1, n_resamples=200, random_state=0)
    inside, planted, noise = stat_properties(ref)
    assert inside and planted > noise, "broken test: the restatement itself does not show the property"
    res = bootstrap(CCA(latent_dimensions=1), [X1, X2], n_resamples=200, random_state=0)
    inside, planted, noise = stat_properties(res)
    print(f"planted component: |bootstrap ratio| planted {planted:.1f}, noise median {noise:.2f}, "
          f"interval {res.singular_values_ci[:, 0]} around {res.singular_values[0]:.4f}")
    assert inside and planted > noise
    assert res.singular_values_ci[0, 0] < res.singular_values_ci[1, 0] <= 1.0
