"""GPU tests of VariationalBayesCCA: every kernel against NumPy float64 through the C ABI (one step from a peeked state, term
by term, each from the device's own inputs to that term), 100-step trajectories against the restatement
(``tests/vbcca_restatement.py``), then the estimator end to end: host arrays and CUDA tensors, determinism, chunking,
held-out outputs, guards and the non-finite stop."""

import ctypes as C
import math

import numpy as np
import pytest

import vbcca_restatement as R
from test_vbcca_host import TRAJ_CASES, TRAJ_LR, TRAJ_STEPS, col_err, nonfinite_case, nonfinite_run, traj_case, traj_run

pytestmark = pytest.mark.gpu

W_TOL = 1e-8          # the family's device bar (tests/test_gpu_als.py, tests/test_gpu_gfa.py)
PEEK = {"loc": 0, "rho": 1, "m1": 2, "v1": 3, "m2": 4, "v2": 5, "theta": 6, "eps": 7, "grad": 8, "loss": 9, "plan": 10}
STATE = ("loc", "rho", "m1", "v1", "m2", "v2")
SEED, LR = 77, 1e-2


def rel(a, b):
    """Largest error of a against b in units of the largest entry of b."""
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), 1e-300))


class _Fit:
    """A raw SVI fit state on rows uploaded to the device.  ``pad``: extra elements per row (ld = p + pad) filled with
    ``pad_value``; ``offset``: the view starts this many elements into its buffer (base pointer 4 or 8 bytes off a
    16-byte boundary); ``means``: "auto", None (``means_dev == NULL``) or a list whose None entries become NULL entries."""

    def __init__(self, views, k, num_steps=4, lr=LR, seed=SEED, chunk=2, pad=0, offset=0, means="auto", pad_value=1e30):
        from cca_zoo_amd import _backend

        self.h = h = _backend.default_handle()
        self.m, self.k = len(views), k
        self.p = [v.shape[1] for v in views]
        self.n = views[0].shape[0]
        self.lay = R.Layout(self.p, self.n, k)
        self.num_steps, self.lr, self.seed = num_steps, lr, seed
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
        h.check(h.lib.ccz_svi_create(h.raw, _backend.F32 if f32 else _backend.F64, self.m, (C.c_int64 * self.m)(*self.p),
                                     self.n, k, num_steps, lr, seed, chunk, C.byref(self.state)))
        # the rows the device subtracts from: fl(x - mu) in the views' dtype, as float64
        self.xs = [(v if means is None or means[i] is None else v - np.asarray(means[i], dtype=v.dtype)).astype(np.float64)
                   for i, v in enumerate(views)]

    def set_init(self, loc0):
        a = np.ascontiguousarray(loc0, dtype=np.float64)
        assert a.shape == (self.lay.N,)
        self.h.check(self.h.lib.ccz_svi_set_init(self.h.raw, self.state, a.ctypes.data_as(C.POINTER(C.c_double))))

    def steps(self, s):
        a, b = C.c_int64(0), C.c_int(0)
        self.h.check(self.h.lib.ccz_svi_steps(self.h.raw, self.state, self.varr, self.marr, s, C.byref(a), C.byref(b)))
        return a.value, b.value

    def status(self):
        done, stop, bad = C.c_int64(0), C.c_int(0), C.c_int64(0)
        self.h.check(self.h.lib.ccz_svi_status(self.h.raw, self.state, C.byref(done), C.byref(stop), C.byref(bad)))
        return dict(steps=done.value, stopped=stop.value, bad_step=bad.value)

    def peek(self, what):
        size = {"loss": self.num_steps, "plan": 3 + self.m}.get(what, self.lay.N)
        out = np.empty(size)
        self.h.check(self.h.lib.ccz_svi_peek(self.h.raw, self.state, PEEK[what], out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def plan(self):
        pl = self.peek("plan")
        return dict(nchunk=int(pl[0]), rc=int(pl[1]), strips=[int(x) for x in pl[3:]])

    def snapshot(self):
        return {key: self.peek(key) for key in STATE}

    def close(self):
        self.h.check(self.h.lib.ccz_svi_destroy(self.h.raw, self.state))


def check_one_step(fit, before, t, tag):
    """Every term of step t, each recomputed in NumPy float64 from the DEVICE's own inputs to that term.  Bars: 1e-12 for
    the sums of products (as tests/test_gpu_gfa.py), in units of the largest entry of the site; eps is held to 1e-12
    absolute, the accuracy of log / cos on either side."""
    lay, after = fit.lay, fit.snapshot()
    theta, eps, grad, loss = fit.peek("theta"), fit.peek("eps"), fit.peek("grad"), fit.peek("loss")[t]
    worst = {}

    def note(name, err, bar):
        worst[name] = max(worst.get(name, 0.0), err)
        assert err <= bar, (tag, name, err, bar)

    note("eps", float(np.max(np.abs(eps - R.draw_eps(lay, fit.seed, t)))), 1e-12)
    scale = R.softplus(before["rho"])
    note("theta", rel(theta, before["loc"] + scale * eps), 1e-14)
    lp, g = R.log_joint_and_grad(lay, theta, fit.xs)
    names = ["da"] + [x for i in range(lay.m) for x in (f"dW{i}", f"ds{i}")] + ["dZ"]
    for name, (_, view) in zip(names, lay.sites()):
        note(name, rel(view(grad), view(g)), 1e-12)
    log_q = np.sum(-0.5 * math.log(2.0 * math.pi) - np.log(scale) - 0.5 * eps * eps)
    note("loss", abs(loss - (-(lp - log_q))) / abs(loss), 1e-12)
    # Adam from the device's own gradient, eps and moments
    gr = (grad * eps + 1.0 / scale) * R.sigmoid(before["rho"])
    loc, m1, v1 = R.adam(before["loc"], before["m1"], before["v1"], -grad, fit.lr, t)
    rho, m2, v2 = R.adam(before["rho"], before["m2"], before["v2"], -gr, fit.lr, t)
    for key, want in (("loc", loc), ("rho", rho), ("m1", m1), ("v1", v1), ("m2", m2), ("v2", v2)):
        note(key, rel(after[key], want), 1e-12)
    print(tag, " ".join(f"{a}={b:.1e}" for a, b in worst.items()))
    return after


# p per view, n, k: p not a multiple of 4, of the 64-feature wave strip of the MFMA kernel, of the 256-column strip; n not a
# multiple of 16 (the MFMA row block) or of the rows of a chunk; k = 1, 3, 4 (plain FMA kernel), 5, 16, 17 and 32 (the MFMA
# tile edges).  2050 x 5 takes nine strips of the plain kernel, 1030 x 517 five of the MFMA kernel; 37 x 21 (n = 50) takes
# four row chunks of the plain kernel, 1030 x 517 (n = 41) two of the MFMA kernel, the second a partial 16-row block.
SHAPES = [
    ((5, 3), 9, 1),
    ((37, 21), 50, 3),
    ((66, 131), 35, 4),
    ((2050, 5), 19, 2),
    ((1030, 517), 41, 5),
    ((130, 64), 33, 16),
    ((1024, 2049, 70), 67, 17),
    ((300, 9001), 37, 32),
]
SHAPE_IDS = [f"{'x'.join(map(str, s[0]))}_n{s[1]}_k{s[2]}" for s in SHAPES]
# ld > p with poisoned padding and a base pointer 4 (fp32) or 8 bytes off a 16-byte boundary; NULL means; one NULL entry
LAYOUTS = [(3, 1, "auto"), (1, 2, "none"), (0, 0, "one_null")]


def _shape_views(shape, dtype):
    dims, n, _ = shape
    rng = np.random.default_rng(len(dims) * 1000 + n)
    zt = rng.standard_normal((n, 2))
    return [(zt @ rng.standard_normal((2, d)) + rng.standard_normal((n, d)) + 0.5).astype(dtype) for d in dims], rng


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_step_kernels(shape, dtype):
    views, rng = _shape_views(shape, dtype)
    for pad, offset, meanmode in LAYOUTS:
        means = "auto"
        if meanmode == "none":
            means = None
        elif meanmode == "one_null":
            means = [v.mean(axis=0).astype(dtype) for v in views]
            means[len(views) // 2] = None
        fit = _Fit(views, shape[2], pad=pad, offset=offset, means=means)
        try:
            loc0 = R.init_loc(rng, fit.lay)
            fit.set_init(loc0)
            s0 = fit.snapshot()
            np.testing.assert_array_equal(s0["loc"], loc0)
            assert rel(R.softplus(s0["rho"]), np.full(fit.lay.N, R.INIT_SCALE)) <= 1e-15
            assert all(np.all(s0[key] == 0) for key in ("m1", "v1", "m2", "v2"))
            tag = f"{np.dtype(dtype).name} {shape[0]} pad{pad} off{offset} {meanmode}"
            fit.steps(1)
            s1 = check_one_step(fit, s0, 0, tag + " step0")
            fit.steps(1)           # the second step starts from non-zero moments
            check_one_step(fit, s1, 1, tag + " step1")
            st = fit.status()
            assert (st["steps"], st["stopped"], st["bad_step"]) == (2, 0, -1)
        finally:
            fit.close()


def test_table_reaches_two_strips_and_two_row_chunks_of_both_kernels():
    """From the planned launch: the plain (k <= 4) and the MFMA kernel each meet a shape with at least two strips
    (column splits) of one view and a shape with at least two row chunks."""
    seen = {(path, what): False for path in ("plain", "mfma") for what in ("strips", "chunks")}
    for shape in SHAPES:
        views, _ = _shape_views(shape, np.float32)
        fit = _Fit(views, shape[2])
        try:
            fit.set_init(np.zeros(fit.lay.N))
            pl = fit.plan()
        finally:
            fit.close()
        path = "plain" if shape[2] <= 4 else "mfma"
        assert pl["strips"] == [(p + 255) // 256 for p in shape[0]] and pl["rc"] % 16 == 0 and pl["nchunk"] == -(-shape[1] // pl["rc"])
        seen[(path, "strips")] |= max(pl["strips"]) >= 2
        seen[(path, "chunks")] |= pl["nchunk"] >= 2
    assert all(seen.values()), seen


def test_steps_after_the_stop_are_no_ops_and_more_than_num_steps_is_refused():
    views, rng = _shape_views(SHAPES[1], np.float64)
    fit = _Fit(views, 3, num_steps=3, chunk=2)
    try:
        fit.set_init(R.init_loc(rng, fit.lay))
        fit.steps(2)
        fit.steps(1)
        a = fit.snapshot()
        assert fit.status() == dict(steps=3, stopped=1, bad_step=-1)
        with pytest.raises(ValueError, match="more steps"):
            fit.steps(1)
        fit.steps(0)
        for key in STATE:
            np.testing.assert_array_equal(a[key], fit.peek(key))
    finally:
        fit.close()


# ---- trajectories against the restatement ---------------------------------------------------------------------------------
def _model(k, **over):
    from cca_zoo_amd.probabilistic import VariationalBayesCCA

    par = dict(latent_dimensions=k, num_steps=TRAJ_STEPS, learning_rate=TRAJ_LR, num_posterior_samples=3, random_state=5)
    par.update(over)
    return VariationalBayesCCA(**par)


@pytest.fixture(scope="module")
def traj_fits():
    """One fit per trajectory case from host arrays, shared by the tests that compare against it (never modified)."""
    cache = {}

    def get(name):
        if name not in cache:
            views, k, center = traj_case(name)
            cache[name] = _model(k, center=center).fit(views)
        return cache[name]

    return get


@pytest.mark.parametrize("name", sorted(TRAJ_CASES))
def test_trajectory_matches_the_restatement(name, traj_fits):
    """100 steps: loc of every W_i to 1e-8 per column and every loss to 1e-8 relative (the cases are conditioned to 1e-10:
    tests/test_vbcca_host.py::test_trajectory_cases_are_well_conditioned)."""
    model, ref = traj_fits(name), traj_run(name)
    lay = ref["layout"]
    assert model.n_iter_ == TRAJ_STEPS and model.losses_.shape == (TRAJ_STEPS,) and model.losses_.dtype == np.float64
    errs = [col_err(model.variational_params_[f"W_{i}"]["loc"], lay.W(ref["loc"], i)) for i in range(lay.m)]
    lerr = float(np.max(np.abs(model.losses_ - ref["losses"]) / np.abs(ref["losses"])))
    print(f"trajectory {name}: W loc col err {max(errs):.2e} losses {lerr:.2e}")
    assert max(errs) <= W_TOL and lerr <= W_TOL


# ---- the estimator ---------------------------------------------------------------------------------------------------
#: weights_, ard_relevance_ and the draws are loc + scale x (the same normals): the 1e-8 device bar on loc and scale times
#: 1 + the largest |normal| of the draws (below 5), with a factor 2
FIT_TOL = 1e-7


@pytest.mark.parametrize("name", ["two_f64", "wide_f32_k5"])
def test_estimator_matches_the_restatement_driven_expectation(name, traj_fits):
    views, k, center = traj_case(name)
    model = traj_fits(name)
    ref = R.fit_expectation(views, k, TRAJ_STEPS, TRAJ_LR, 5, 3, center=center)
    assert set(model.posterior_samples_) == set(ref["samples"])
    for key, want in ref["samples"].items():
        assert model.posterior_samples_[key].shape == want.shape and rel(model.posterior_samples_[key], want) <= FIT_TOL, key
    for i, w in enumerate(model.weights_):
        assert w.dtype == np.float64 and w.shape == (views[i].shape[1], k) and rel(w, ref["weights"][i]) <= FIT_TOL
        assert model.means_[i].dtype == views[i].dtype
        np.testing.assert_array_equal(model.means_[i], ref["means"][i])
    assert rel(model.ard_relevance_, ref["ard_relevance"]) <= FIT_TOL
    assert set(model.variational_params_) == {"log_alpha", "z"} | {f"{s}_{i}" for s in ("W", "log_psi") for i in range(len(views))}
    assert rel(model.variational_params_["z"]["scale"], ref["layout"].Z(ref["scale"])) <= FIT_TOL


def _same_fit(a, b):
    np.testing.assert_array_equal(a.losses_, b.losses_)
    np.testing.assert_array_equal(a.ard_relevance_, b.ard_relevance_)
    for x, y in zip(a.weights_, b.weights_):
        np.testing.assert_array_equal(x, y)
    for key in a.posterior_samples_:
        np.testing.assert_array_equal(a.posterior_samples_[key], b.posterior_samples_[key])
    for key in a.variational_params_:
        np.testing.assert_array_equal(a.variational_params_[key]["loc"], b.variational_params_[key]["loc"])
        np.testing.assert_array_equal(a.variational_params_[key]["scale"], b.variational_params_[key]["scale"])


@pytest.mark.parametrize("name", ["three_f32", "wide_f32_k5"])
def test_two_fits_are_bit_identical(name, traj_fits):
    views, k, center = traj_case(name)
    _same_fit(_model(k, center=center).fit(views), traj_fits(name))


@pytest.mark.parametrize("name", ["two_f64", "wide_f32_k5"])
def test_chunk_length_does_not_change_the_result(name, traj_fits, monkeypatch):
    from cca_zoo_amd.probabilistic import _vbcca

    views, k, center = traj_case(name)
    assert _vbcca.CHUNK_STEPS == 64 and TRAJ_STEPS % 64 != 0
    monkeypatch.setattr(_vbcca, "CHUNK_STEPS", 1)
    _same_fit(_model(k, center=center).fit(views), traj_fits(name))


@pytest.mark.parametrize("name", ["two_f64", "three_f32"])
def test_cuda_tensors_give_the_same_bits_and_stay_unchanged(name, traj_fits):
    import torch

    views, k, center = traj_case(name)
    tens = [torch.as_tensor(v, device="cuda") for v in views]
    before = [t.clone() for t in tens]
    model = _model(k, center=center).fit(tens)
    for a, b in zip(tens, before):
        assert torch.equal(a, b)
    host = traj_fits(name)
    for a, b in zip(model.means_, host.means_):      # ccz_als_colmeans sums in NumPy's order
        np.testing.assert_array_equal(a, b)
    _same_fit(model, host)                           # the same rows and the same means give the same bits


def _held_out(name):
    seed, n, p, _, dtype, _ = TRAJ_CASES[name]
    rng = np.random.default_rng(seed + 100)
    return [rng.standard_normal((15, pi)).astype(dtype) for pi in p]


@pytest.mark.parametrize("name", ["two_f64", "three_f32", "two_f64_nocenter"])
def test_held_out_outputs_match_the_mixin_formulas(name, traj_fits):
    """transform / score / log_likelihood against cca_zoo/probabilistic/_utils.py:11-109, :217-291 written out in NumPy, at
    the bars tests/test_gpu_gfa.py uses (1e-7 for fp64 views, 1e-3 for fp32 views)."""
    import torch

    model, test = traj_fits(name), _held_out(name)
    bar = 1e-3 if test[0].dtype == np.float32 else 1e-7
    cent = [np.asarray(v, dtype=np.float64) - np.asarray(mu, dtype=np.float64) for v, mu in zip(test, model.means_)]
    psi = [np.exp(model.posterior_samples_[f"log_psi_{i}"]).mean(axis=0) for i in range(len(test))]
    k = model.latent_dimensions
    prec, info = np.eye(k), np.zeros((15, k))
    for x, w, ps in zip(cent, model.weights_, psi):
        pinv = 1.0 / np.maximum(ps, 1e-8)
        prec = prec + w.T @ (w * pinv[:, None])
        info = info + (x * pinv) @ w
    zt = model.transform(test)
    assert len(zt) == 1 and zt[0].dtype == np.float64 and col_err(zt[0], info @ np.linalg.inv(prec)) <= bar
    proj = np.stack([x @ w for x, w in zip(cent, model.weights_)])
    proj = proj - proj.mean(axis=1, keepdims=True)
    nrm = np.sqrt((proj ** 2).sum(axis=1, keepdims=True))
    tn = proj / np.where(nrm > 1e-12, nrm, 1.0)
    corr = np.einsum("isd,jsd->ijd", tn, tn)
    m = len(test)
    want_score = (corr.sum(axis=(0, 1)) - sum(corr[i, i] for i in range(m))) / (m * (m - 1))
    np.testing.assert_allclose(model.score(test), want_score, atol=bar)
    w_full, psi_full, x_full = np.concatenate(model.weights_), np.concatenate(psi), np.concatenate(cent, axis=1)
    pinv = 1.0 / np.maximum(psi_full, 1e-8)
    mm = np.eye(k) + (w_full.T * pinv) @ w_full
    logdet = np.sum(np.log(np.maximum(psi_full, 1e-300))) + np.linalg.slogdet(mm)[1]
    xs = x_full * pinv
    pj = xs @ w_full
    quad = np.einsum("np,np->n", x_full, xs) - np.einsum("nk,kj,nj->n", pj, np.linalg.inv(mm), pj)
    want_ll = float(np.mean(-0.5 * (x_full.shape[1] * np.log(2 * np.pi) + logdet + quad)))
    ll = model.log_likelihood(test)
    print(f"held-out {name}: log-likelihood {ll:.12g} NumPy {want_ll:.12g}")
    assert abs(ll - want_ll) <= bar * abs(want_ll)
    held = [torch.as_tensor(v, device="cuda") for v in test]
    zc = model.transform(held)
    assert len(zc) == 1 and zc[0].is_cuda and col_err(zc[0].cpu().numpy(), info @ np.linalg.inv(prec)) <= bar
    assert abs(model.log_likelihood(held) - want_ll) <= bar * abs(want_ll)


def test_non_finite_loss_raises_with_the_restatements_step():
    ref = nonfinite_run()
    with pytest.raises(FloatingPointError, match=f"step {ref['bad_step']} "):
        _model(2, num_steps=20, learning_rate=1e6, num_posterior_samples=2, random_state=0).fit(nonfinite_case())


# ---- guards ---------------------------------------------------------------------------------------------------------
def test_guards():
    from cca_zoo_amd import _backend
    from cca_zoo_amd.probabilistic import VariationalBayesCCA
    from cca_zoo_amd.probabilistic._vbcca import MAX_SAMPLE_BYTES

    rng = np.random.default_rng(0)
    X = [rng.standard_normal((40, 5)), rng.standard_normal((40, 4))]
    with pytest.raises(ValueError, match="at most 32"):
        VariationalBayesCCA(latent_dimensions=33).fit(X)
    with pytest.raises(ValueError, match="at most 8 views"):
        VariationalBayesCCA().fit([X[0]] * 9)
    with pytest.raises(ValueError, match="lower num_posterior_samples"):
        VariationalBayesCCA(latent_dimensions=2, num_posterior_samples=MAX_SAMPLE_BYTES // (40 * 2 * 8) + 1).fit(X)
    # the C ABI refuses the same limits, and a single view, a single row and an empty view
    h = _backend.default_handle()
    state = C.c_void_p()
    for p, n, k in (([5, 5], 40, 33), ([5] * 9, 40, 2), ([5], 40, 2), ([5, 5], 1, 2), ([5, 0], 40, 2)):
        m = len(p)
        rc = h.lib.ccz_svi_create(h.raw, _backend.F64, m, (C.c_int64 * m)(*p), n, k, 10, 1e-2, 0, 8, C.byref(state))
        assert rc != 0 and not state.value, (p, n, k)


def test_fit_inside_row_sharded_is_refused(monkeypatch):
    from cca_zoo_amd import _dist
    from cca_zoo_amd.probabilistic import VariationalBayesCCA

    monkeypatch.setattr(_dist, "is_sharded", lambda: True)
    rng = np.random.default_rng(0)
    with pytest.raises(NotImplementedError, match="row_sharded"):
        VariationalBayesCCA().fit([rng.standard_normal((40, 5)), rng.standard_normal((40, 4))])
