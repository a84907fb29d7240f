"""GPU tests of GFA: every kernel against NumPy float64 through the C ABI (one iteration from a peeked state, term by
term), every golden case through the estimator (host arrays and CUDA tensors), determinism, chunking and guards."""

import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from test_gfa_host import CASES, PRIOR, case_params, case_views, col_err, initial_state, rel, sample_errors

pytestmark = pytest.mark.gpu

W_TOL = 1e-8          # the family's device bar (tests/test_gpu_als.py): per-column relative error of weights_, fp64 AND fp32 views
EPS = 2.0 ** -52
PEEK = {"z": 0, "w": 1, "xw": 2, "cov_z": 3, "cov_w": 4, "ww": 5, "zz": 6, "alpha": 7, "tau": 8, "b_tau": 9, "b_ard": 10, "setup": 11}


class _Fit:
    """A raw fit state on rows uploaded to the device.  ``pad``: extra elements per row (ld = p + pad) filled with
    ``pad_value``; ``offset``: the view starts this many elements into its buffer (base pointer 4 or 8 bytes off a
    16-byte boundary); ``means``: "auto", None (``means_dev == NULL``) or a list whose None entries become NULL entries."""

    def __init__(self, views, k, tol=1e-4, max_iter=10000, drop_k=True, chunk=8, pad=0, offset=0, means="auto", pad_value=1e30):
        from cca_zoo_amd import _backend

        self.h = h = _backend.default_handle()
        self.m, self.k = len(views), k
        self.p = [v.shape[1] for v in views]
        self.n = views[0].shape[0]
        f32 = views[0].dtype == np.float32
        if isinstance(means, str):
            means = [v.mean(axis=0).astype(v.dtype) for v in views]
        self.bufs, self.mbufs = [], []
        self.varr = (_backend.View * self.m)()
        for i, v in enumerate(views):
            ld = v.shape[1] + pad
            padded = np.full((v.shape[0], ld), pad_value, dtype=v.dtype)
            padded[:, : v.shape[1]] = v
            flat = np.concatenate([np.full(offset, pad_value, dtype=v.dtype), padded.reshape(-1)])
            b = h.to_device(flat)
            self.bufs.append(b)
            self.varr[i].data, self.varr[i].cols, self.varr[i].ld = b.ptr + offset * v.dtype.itemsize, v.shape[1], ld
            if means is not None:
                self.mbufs.append(None if means[i] is None else h.to_device(np.asarray(means[i], dtype=v.dtype)))
        self.marr = (C.c_void_p * self.m)(*[None if b is None else b.ptr for b in self.mbufs]) if means is not None else None
        self.state = C.c_void_p()
        h.check(h.lib.ccz_gfa_create(h.raw, _backend.F32 if f32 else _backend.F64, self.m, (C.c_int64 * self.m)(*self.p),
                                     self.n, k, tol, max_iter, int(drop_k), chunk, C.byref(self.state)))
        # the rows the device multiplies: fl(x - mu) in the views' dtype, as float64
        self.xs = [(v if means is None or means[i] is None else v - np.asarray(means[i], dtype=v.dtype)).astype(np.float64)
                   for i, v in enumerate(views)]

    def setup(self, z0):
        a = np.ascontiguousarray(z0, dtype=np.float64)
        assert a.shape == (self.n, self.k)
        self.h.check(self.h.lib.ccz_gfa_set_init(self.h.raw, self.state, a.ctypes.data_as(C.POINTER(C.c_double))))
        self.h.check(self.h.lib.ccz_gfa_setup(self.h.raw, self.state, self.varr, self.marr))

    def iterations(self, s):
        a, b = C.c_int64(0), C.c_int(0)
        self.h.check(self.h.lib.ccz_gfa_iterations(self.h.raw, self.state, self.varr, self.marr, s, C.byref(a), C.byref(b)))
        return a.value, b.value

    def status(self):
        it, st, ka, stable, npr, rc = C.c_int64(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.0)
        pi, pk = (C.c_int64 * 32)(), (C.c_int * 32)()
        self.h.check(self.h.lib.ccz_gfa_status(self.h.raw, self.state, C.byref(it), C.byref(st), C.byref(ka), C.byref(stable),
                                               C.byref(rc), C.byref(npr), pi, pk))
        return dict(iters=it.value, stopped=st.value, k=ka.value, stable=stable.value, rel_change=rc.value,
                    prunes=[int(pi[i]) for i in range(npr.value)], prune_k=[int(pk[i]) for i in range(npr.value)])

    def peek(self, what, view=0):
        ka = self.status()["k"]
        shape = {"z": (self.n, ka), "w": (self.p[view], ka), "xw": (self.n, ka), "cov_z": (ka, ka), "cov_w": (ka, ka),
                 "ww": (ka, ka), "zz": (ka, ka), "alpha": (ka,), "b_ard": (ka,), "tau": (self.m,), "b_tau": (self.m,),
                 "setup": (2,)}[what]
        out = np.empty(shape)
        self.h.check(self.h.lib.ccz_gfa_peek(self.h.raw, self.state, PEEK[what], view, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def snapshot(self):
        """The whole state in the layout of ``test_gfa_host.initial_state``."""
        r = range(self.m)
        setup = [self.peek("setup", i) for i in r]
        return dict(z=self.peek("z"), cov_z=self.peek("cov_z"), zz=self.peek("zz"), tau=self.peek("tau"), b_tau=self.peek("b_tau"),
                    w=[self.peek("w", i) for i in r], cov_w=[self.peek("cov_w", i) for i in r], ww=[self.peek("ww", i) for i in r],
                    alpha=[self.peek("alpha", i) for i in r], b_ard=[self.peek("b_ard", i) for i in r],
                    xw=[self.peek("xw", i) for i in r], y_const=np.array([s[0] for s in setup]),
                    datavar=np.array([s[1] for s in setup]))

    def close(self):
        self.h.check(self.h.lib.ccz_gfa_destroy(self.h.raw, self.state))


def check_one_iteration(fit, before, after, tag):
    """Every term of one iteration, each recomputed in NumPy float64 from the DEVICE's own inputs to that term.  Bars:
    1e-12 for sums of products of O(n p) terms; the two Cholesky inverses are held through their residual to
    ``8 k eps cond`` (the textbook bound of an inverse formed from a Cholesky factor is a small multiple of
    ``k eps cond``); b_tau, whose three terms cancel (``y_const / (2 b_tau) <= 100`` is the generator's rule; here the
    ratio is measured), to 1e-13 times that ratio."""
    xs, m, n = fit.xs, fit.m, fit.n
    k = after["z"].shape[1]
    assert before["z"].shape[1] == k
    worst = {}

    def note(name, err, bar):
        worst[name] = max(worst.get(name, 0.0), err)
        assert err <= bar, (tag, name, err, bar)

    for i in range(m):
        t = 1.0 / np.sqrt(before["alpha"][i])
        inner = np.outer(t, t) * before["zz"] + np.eye(k) / before["tau"][i]
        scale = (1.0 / before["tau"][i]) * np.outer(t, t)
        inv = after["cov_w"][i] / scale
        note("cov_w", float(np.max(np.abs(inv @ inner - np.eye(k)))), 8 * k * EPS * np.linalg.cond(inner))
        note("w", rel(after["w"][i], (xs[i].T @ before["z"]) @ after["cov_w"][i] * before["tau"][i]), 1e-12)
        note("ww", rel(after["ww"][i], after["w"][i].T @ after["w"][i] + xs[i].shape[1] * after["cov_w"][i]), 1e-12)
        note("xw", rel(after["xw"][i], xs[i] @ after["w"][i]), 1e-12)
    prec = np.eye(k)
    for i in range(m):
        prec = prec + before["tau"][i] * after["ww"][i]
    note("cov_z", float(np.max(np.abs(after["cov_z"] @ prec - np.eye(k)))), 8 * k * EPS * np.linalg.cond(prec))
    rhs = sum(after["xw"][i] * before["tau"][i] for i in range(m))
    note("z", rel(after["z"], rhs @ after["cov_z"]), 1e-12)
    note("zz", rel(after["zz"], after["z"].T @ after["z"] + n * after["cov_z"]), 1e-12)
    for i in range(m):
        d = xs[i].shape[1]
        b_ard = PRIOR + np.diag(after["ww"][i]) / 2.0
        note("b_ard", rel(after["b_ard"][i], b_ard), 1e-14)
        note("alpha", rel(after["alpha"][i], (PRIOR + d / 2.0) / b_ard), 1e-14)
        b_tau = PRIOR + (before["y_const"][i] + np.sum(after["ww"][i] * after["zz"]) - 2.0 * np.sum(after["z"] * after["xw"][i])) / 2.0
        ratio = max(before["y_const"][i] / (2.0 * b_tau), 1.0)
        note("b_tau", abs(after["b_tau"][i] - b_tau) / b_tau, 1e-13 * ratio)
        note("tau", abs(after["tau"][i] - (PRIOR + n * d / 2.0) / after["b_tau"][i]) / after["tau"][i], 1e-14)
    print(tag, " ".join(f"{a}={b:.1e}" for a, b in worst.items()))


# dims, n, k, pad, offset, means: p not a multiple of 4, of the 64-feature MFMA strip, of the 256- / 1024-column workgroup
# strips; ld > p with poisoned padding; base pointers off a 16-byte boundary; NULL means and NULL entries; n not a
# multiple of 4, 8, 16 or 64; k = 1 and 3 (plain FMA kernels), 16, 17 and 32 (the MFMA tile edges); 37 x 9001 takes two
# column splits of the X w kernel; 67 rows two row blocks of it
SHAPES = [
    ((5, 3), 9, 1, 0, 0, "auto"),
    ((37, 21), 50, 3, 3, 0, "auto"),
    ((1030, 517), 41, 16, 2, 0, "auto"),
    ((1024, 2049, 70), 67, 17, 0, 0, "one_null"),
    ((130, 64), 33, 32, 1, 1, "auto"),
    ((131, 66), 35, 3, 0, 2, "none"),
    ((9001, 300), 37, 17, 3, 0, "auto"),
    ((9000, 4100), 18, 1, 0, 1, "one_null"),
]


def _shape_fit(shape, dtype):
    dims, n, k, pad, offset, meanmode = shape
    rng = np.random.default_rng(len(dims) * 1000 + n)
    zt = rng.standard_normal((n, 2))
    views = [(zt @ rng.standard_normal((2, d)) + rng.standard_normal((n, d)) + 0.5).astype(dtype) for d in dims]
    means = "auto"
    if meanmode == "none":
        means = None
    elif meanmode == "one_null":
        means = [v.mean(axis=0).astype(dtype) for v in views]
        means[len(dims) // 2] = None
    fit = _Fit(views, k, max_iter=50, pad=pad, offset=offset, means=means)
    return fit, rng.standard_normal((n, k))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{'x'.join(map(str, s[0]))}_n{s[1]}_k{s[2]}" for s in SHAPES])
def test_setup_and_iteration_kernels(shape, dtype):
    fit, z0 = _shape_fit(shape, dtype)
    try:
        fit.setup(z0)
        s0 = fit.snapshot()
        ref = initial_state(fit.xs, z0)
        assert rel(s0["y_const"], ref["y_const"]) <= 1e-13 and rel(s0["datavar"], ref["datavar"]) <= 1e-12
        np.testing.assert_array_equal(s0["z"], z0)
        assert rel(s0["zz"], ref["zz"]) <= 1e-13
        for i in range(fit.m):
            assert rel(s0["alpha"][i], ref["alpha"][i]) <= 2e-12      # datavar's bar, and the division
            np.testing.assert_array_equal(s0["ww"][i], ref["ww"][i])
            np.testing.assert_array_equal(s0["cov_w"][i], np.eye(fit.k))
            assert np.all(s0["w"][i] == 0) and np.all(s0["b_ard"][i] == PRIOR)
        assert np.all(s0["tau"] == 1e3) and np.all(s0["b_tau"] == PRIOR)
        # the first iteration starts from w = 0 and tau = 1e3, the second from a state with every term in play
        fit.iterations(1)
        s1 = fit.snapshot()
        check_one_iteration(fit, s0, s1, f"{np.dtype(dtype).name} {shape[0]} it1")
        fit.iterations(1)
        s2 = fit.snapshot()
        check_one_iteration(fit, s1, s2, f"{np.dtype(dtype).name} {shape[0]} it2")
        st = fit.status()
        assert (st["iters"], st["stopped"], st["k"], st["prunes"]) == (2, 0, fit.k, [])
        assert abs(st["rel_change"] - np.linalg.norm(s2["z"] - s1["z"]) / np.linalg.norm(s1["z"])) <= 1e-12 * st["rel_change"]
    finally:
        fit.close()


@pytest.mark.parametrize("case,its", [("two_maxiter", 8), ("wide17", 40)])
def test_iteration_kernels_after_a_prune(case, its):
    """A state whose active k is below the allocated one (plain kernels: 4 -> 3; MFMA kernels: 17 -> 16): the prune is
    the one the reference makes, and the next iteration is checked term by term on the kept columns."""
    g = load_golden(f"gfa_{case}")
    par = case_params(g)
    views = case_views(g)
    k = par["latent_dimensions"]
    fit = _Fit(views, k, max_iter=par["max_iter"], chunk=8, pad_value=0.0)
    try:
        fit.setup(np.random.default_rng(par["random_state"]).standard_normal((views[0].shape[0], k)))
        for _ in range(its // 8):
            fit.iterations(8)
        st = fit.status()
        want = [int(i) for i in g["prune_iterations"] if i <= its]
        assert st["iters"] == its and st["prunes"] == want and 0 < st["k"] < k and st["stable"] <= its - want[-1]
        s0 = fit.snapshot()
        assert s0["z"].shape[1] == st["k"] and s0["w"][0].shape[1] == st["k"]
        # the compacted state is a consistent one: zz and ww are those of the kept columns
        assert rel(s0["zz"], s0["z"].T @ s0["z"] + fit.n * s0["cov_z"]) <= 1e-12
        fit.iterations(1)
        check_one_iteration(fit, s0, fit.snapshot(), f"{case} after the prune")
    finally:
        fit.close()


def test_iterations_after_the_stop_are_no_ops():
    g = load_golden("gfa_k1")
    par = case_params(g)
    views = case_views(g)
    fit = _Fit(views, 1, max_iter=par["max_iter"], chunk=64, pad_value=0.0)
    try:
        fit.setup(np.random.default_rng(par["random_state"]).standard_normal((views[0].shape[0], 1)))
        fit.iterations(64)
        fit.iterations(64)          # the stop (max_iter = 100) arrives 36 iterations into this chunk
        a = fit.snapshot()
        fit.iterations(64)
        known, stopped = fit.iterations(0)
        assert (known, stopped) == (100, 1) and fit.status()["iters"] == 100
        b = fit.snapshot()
        for key in ("z", "tau", "zz"):
            np.testing.assert_array_equal(a[key], b[key])
        np.testing.assert_array_equal(a["w"][0], b["w"][0])
    finally:
        fit.close()


# ---- the reference's fits ------------------------------------------------------------------------------------------
def _model(g, **over):
    from cca_zoo_amd.probabilistic import GFA

    p = case_params(g)
    p.update(over)
    return GFA(**p)


@pytest.fixture(scope="module")
def host_fits():
    """One fit per golden from host arrays, shared by the tests that compare against it (never modified)."""
    cache = {}

    def get(case):
        if case not in cache:
            g = load_golden(f"gfa_{case}")
            cache[case] = _model(g).fit(case_views(g))
        return cache[case]

    return get


def _check_against_golden(model, g, tag):
    f32 = case_views(g)[0].dtype == np.float32
    assert model.n_iter_ == int(g["n_iter"])
    assert model.n_components_ == int(g["n_components"])
    assert model.prune_iterations_ == [int(i) for i in g["prune_iterations"]]
    for i, w in enumerate(model.weights_):
        assert w.dtype == np.float64 and model.means_[i].dtype == g[f"mean{i}"].dtype
        np.testing.assert_array_equal(model.means_[i], g[f"mean{i}"])
        err = col_err(w, g[f"W{i}"])
        print(f"golden {tag} view {i}: weights col err {err:.2e}")
        assert err <= W_TOL, (i, err)
    err = rel(model.view_relevance_, g["view_relevance"])
    serr = sample_errors(model.posterior_samples_, g)
    print(f"golden {tag}: view_relevance {err:.2e} samples {max(serr.values()):.2e}")
    assert err <= W_TOL and max(serr.values()) <= W_TOL, (err, serr)
    assert set(model.posterior_samples_) == {k[2:] for k in g if k.startswith("S_")}
    assert model.posterior_samples_["z"].shape == (int(g["num_posterior_samples"]), model.n_samples_, model.n_components_)
    # held-out outputs at the bars tests/test_gpu_als.py uses for its own
    bar = 1e-3 if f32 else 1e-7
    test = case_views(g, "T")
    np.testing.assert_allclose(model.score(test), g["score_test"], atol=bar)
    zt = model.transform(test)
    assert len(zt) == 1 and col_err(np.asarray(zt[0]), g["Zt"]) <= bar
    ll = model.log_likelihood(test)
    print(f"golden {tag}: held-out log-likelihood {ll:.12g} reference {float(g['loglik_test']):.12g}")
    assert abs(ll - float(g["loglik_test"])) <= bar * abs(float(g["loglik_test"]))


@pytest.mark.parametrize("case", CASES)
def test_golden_case_from_host_arrays(case, host_fits):
    _check_against_golden(host_fits(case), load_golden(f"gfa_{case}"), f"{case} (host)")


@pytest.mark.parametrize("case", CASES)
def test_golden_case_from_cuda_tensors(case, host_fits):
    import torch

    g = load_golden(f"gfa_{case}")
    tens = [torch.as_tensor(v, device="cuda") for v in case_views(g)]
    before = [t.clone() for t in tens]
    model = _model(g).fit(tens)
    for a, b in zip(tens, before):
        assert torch.equal(a, b)
    _check_against_golden(model, g, f"{case} (cuda)")
    # the same rows and the same means give the same bits as the fit from host arrays
    for a, b in zip(model.weights_, host_fits(case).weights_):
        np.testing.assert_array_equal(a, b)
    held = [torch.as_tensor(v, device="cuda") for v in case_views(g, "T")]
    zt = model.transform(held)
    assert len(zt) == 1 and zt[0].is_cuda and col_err(zt[0].cpu().numpy(), g["Zt"]) <= (1e-3 if tens[0].dtype == torch.float32 else 1e-7)
    bar = 1e-3 if tens[0].dtype == torch.float32 else 1e-7
    assert abs(model.log_likelihood(held) - float(g["loglik_test"])) <= bar * abs(float(g["loglik_test"]))


def _same_fit(a, b):
    assert (a.n_iter_, a.n_components_, a.prune_iterations_) == (b.n_iter_, b.n_components_, b.prune_iterations_)
    for x, y in zip(a.weights_, b.weights_):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a.view_relevance_, b.view_relevance_)
    for key in a.posterior_samples_:      # functions of z, cov_z, cov_w, b_ard, b_tau: the whole final state
        np.testing.assert_array_equal(a.posterior_samples_[key], b.posterior_samples_[key])


@pytest.mark.parametrize("case", ["three_wide_f32", "wide17"])
def test_two_fits_are_bit_identical(case, host_fits):
    g = load_golden(f"gfa_{case}")
    _same_fit(_model(g).fit(case_views(g)), host_fits(case))


@pytest.mark.parametrize("case", ["two_maxiter", "wide17", "tolstop_k8"])
def test_chunk_length_does_not_change_the_result(case, host_fits, monkeypatch):
    """Chunks of 1 against the default 64: the prunes of two_maxiter (iterations 7, 16) and wide17 (39 .. 58) and the stop
    of tolstop_k8 (iteration 3696 = 57 x 64 + 48) all arrive inside a chunk of 64."""
    from cca_zoo_amd.probabilistic import _gfa

    g = load_golden(f"gfa_{case}")
    assert _gfa.CHUNK_ITERS == 64 and int(g["n_iter"]) % 64 != 0
    monkeypatch.setattr(_gfa, "CHUNK_ITERS", 1)
    _same_fit(_model(g).fit(case_views(g)), host_fits(case))


def test_drop_k_false_keeps_every_dimension(host_fits):
    m = host_fits("nodrop_f32")
    assert m.n_components_ == 3 and m.prune_iterations_ == [] and m.weights_[0].shape[1] == 3


def test_factor_loadings_use_the_per_view_projections(host_fits):
    g = load_golden("gfa_two_maxiter")
    m, views = host_fits("two_maxiter"), case_views(g, "T")
    for v, w, mu, got in zip(views, m.weights_, m.means_, m.get_factor_loadings(views)):
        t = (v - mu) @ w
        vc, tc = v - v.mean(axis=0), t - t.mean(axis=0)
        want = (vc.T @ tc / (len(v) - 1)) / np.outer(vc.std(axis=0, ddof=1), tc.std(axis=0, ddof=1))
        np.testing.assert_allclose(got, want, atol=1e-9)


# ---- guards ---------------------------------------------------------------------------------------------------------
def test_guards():
    from cca_zoo_amd import _backend
    from cca_zoo_amd.probabilistic import GFA
    from cca_zoo_amd.probabilistic._gfa import MAX_SAMPLE_BYTES

    rng = np.random.default_rng(0)
    X = [rng.standard_normal((40, 5)), rng.standard_normal((40, 4))]
    with pytest.raises(ValueError, match="at most 32"):
        GFA(latent_dimensions=33).fit(X)
    with pytest.raises(ValueError, match="at most 8 views"):
        GFA().fit([X[0]] * 9)
    with pytest.raises(ValueError, match="lower num_posterior_samples"):
        GFA(latent_dimensions=2, num_posterior_samples=MAX_SAMPLE_BYTES // (40 * 2 * 8) + 1).fit(X)
    # the C ABI refuses the same limits
    h = _backend.default_handle()
    state = C.c_void_p()
    for m, k in ((2, 33), (9, 2)):
        rc = h.lib.ccz_gfa_create(h.raw, _backend.F64, m, (C.c_int64 * m)(*[5] * m), 40, k, 1e-4, 10, 1, 8, C.byref(state))
        assert rc != 0 and not state.value


def test_fit_inside_row_sharded_is_refused(monkeypatch):
    from cca_zoo_amd import _dist
    from cca_zoo_amd.probabilistic import GFA

    monkeypatch.setattr(_dist, "is_sharded", lambda: True)
    rng = np.random.default_rng(0)
    with pytest.raises(NotImplementedError, match="row_sharded"):
        GFA().fit([rng.standard_normal((40, 5)), rng.standard_normal((40, 4))])
