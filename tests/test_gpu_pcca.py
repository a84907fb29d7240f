"""GPU tests of ProbabilisticCCA: every kernel against NumPy float64 through the C ABI (leapfrog steps from a set state, term
by term, each from the device's own inputs to that term), the Welford update and a window end, whole transitions from a
set state and conditioned trajectories against the restatement (``tests/pcca_restatement.py``), then the estimator end
to end: determinism, CUDA tensors, held-out outputs, guards, the non-finite initial potential and one statistical case."""

import ctypes as C
import math

import numpy as np
import pytest

import pcca_restatement as P
from test_pcca_host import (TRAJ_CASES, TRAJ_DEPTH, TRAJ_SAMPLES, TRAJ_WARMUP, TRANSITION_STEP, col_err, planted,
                            traj_case, traj_run, transition_case)

pytestmark = pytest.mark.gpu

W_TOL = 1e-8          # the family's device bar (tests/test_gpu_vbcca.py, tests/test_gpu_als.py); measured worst 5.5e-13 (W), 8.3e-14 (U)
TERM_TOL = 1e-12      # sums of products, in units of the site's largest entry (tests/test_gpu_vbcca.py, tests/test_gpu_gfa.py);
                      # measured worst 2.0e-15 (a leapfrog's dz), 3.6e-16 (Welford and the window end)
SLOT = {"left_q": 0, "left_p": 1, "left_g": 2, "right_q": 3, "right_p": 4, "right_g": 5, "q": 6, "g": 7, "sub_q": 8, "sub_g": 9,
        "rho": 10, "rsum": 11, "minv": 12, "wmean": 13, "wm2": 14, "ckpt": 15}
PLAN, RECORD, SCALARS = 100, 101, 102
TOP = 20              # record index of the whole tree's two products
SEED = 77


def rel(a, b):
    """Largest error of a against b in units of the largest entry of b."""
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), 1e-300))


class _Fit:
    """A raw NUTS fit state on rows uploaded to the device; ``pad`` / ``offset`` / ``means`` as in tests/test_gpu_vbcca.py."""

    def __init__(self, views, k, num_warmup=0, num_samples=4, depth=5, target=0.8, seed=SEED, pad=0, offset=0, means="auto",
                 pad_value=1e30):
        from cca_zoo_amd import _backend

        self.h = h = _backend.default_handle()
        self.m, self.k = len(views), k
        self.p = [v.shape[1] for v in views]
        self.n = views[0].shape[0]
        self.lay = P.Layout(self.p, self.n, k)
        self.seed, self.num_warmup, self.num_samples = seed, num_warmup, num_samples
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
        h.check(h.lib.ccz_nuts_create(h.raw, _backend.F32 if f32 else _backend.F64, self.m, (C.c_int64 * self.m)(*self.p), self.n, k,
                                      num_warmup, num_samples, depth, target, seed, C.byref(self.state)))
        # the rows the device subtracts from: fl(x - mu) in the views' dtype, as float64
        self.xs = [(v if means is None or means[i] is None else v - np.asarray(means[i], dtype=v.dtype)).astype(np.float64)
                   for i, v in enumerate(views)]
        self.pg = P.model_pg(self.lay, self.xs)

    def _pd(self, a):
        return a.ctypes.data_as(C.POINTER(C.c_double))

    def set_init(self, q0):
        a = np.ascontiguousarray(q0, dtype=np.float64)
        assert a.shape == (self.lay.N,)
        u = C.c_double(0.0)
        self.h.check(self.h.lib.ccz_nuts_set_init(self.h.raw, self.state, self.varr, self.marr, self._pd(a), C.byref(u)))
        return u.value

    def set_adapt(self, eps, minv=None):
        a = None if minv is None else np.ascontiguousarray(minv, dtype=np.float64)
        self.h.check(self.h.lib.ccz_nuts_set_adapt(self.h.raw, self.state, eps, None if a is None else self._pd(a)))

    def leapfrog(self, t, begin, direction, leaf, depth):
        rec = np.zeros(27)
        self.h.check(self.h.lib.ccz_nuts_leapfrog(self.h.raw, self.state, self.varr, self.marr, t, begin, direction, leaf, depth,
                                                  self._pd(rec)))
        return rec

    def run(self, count, draws=None):
        self.h.check(self.h.lib.ccz_nuts_run(self.h.raw, self.state, self.varr, self.marr, count, None if draws is None else self._pd(draws)))

    def status(self):
        done, stop, bad = C.c_int64(0), C.c_int(0), C.c_int64(0)
        self.h.check(self.h.lib.ccz_nuts_status(self.h.raw, self.state, C.byref(done), C.byref(stop), C.byref(bad)))
        return dict(transitions=done.value, stopped=stop.value, bad=bad.value)

    def peek(self, what, c=0):
        code = {"plan": PLAN, "record": RECORD, "scalars": SCALARS}.get(what)
        if code is None:
            code = SLOT["ckpt"] + 2 * c if what == "ckpt_p" else SLOT["ckpt"] + 2 * c + 1 if what == "ckpt_sum" else SLOT[what]
        out = np.empty({PLAN: 5 + self.m, RECORD: 26, SCALARS: 4}.get(code, self.lay.N))
        self.h.check(self.h.lib.ccz_nuts_peek(self.h.raw, self.state, code, self._pd(out)))
        return out

    def plan(self):
        pl = self.peek("plan")
        return dict(nchunk=int(pl[0]), rc=int(pl[1]), workgroups=int(pl[3]), slots=int(pl[4]), strips=[int(x) for x in pl[5:]])

    def stats(self, count):
        out, step, minv = np.empty((6, count)), C.c_double(0.0), np.empty(self.lay.N)
        self.h.check(self.h.lib.ccz_nuts_get_stats(self.h.raw, self.state, self._pd(out), C.byref(step), self._pd(minv)))
        names = ("tree_depth", "n_leapfrog", "accept_prob", "diverging", "potential_energy", "step_size")
        return {name: out[a] for a, name in enumerate(names)}, step.value, minv

    def close(self):
        self.h.check(self.h.lib.ccz_nuts_destroy(self.h.raw, self.state))


class _Worst:
    def __init__(self, tag):
        self.tag, self.worst = tag, {}

    def note(self, name, err, bar):
        self.worst[name] = max(self.worst.get(name, 0.0), err)
        assert err <= bar, (self.tag, name, err, bar)

    def show(self):
        print(self.tag, " ".join(f"{a}={b:.1e}" for a, b in self.worst.items()))


def _dots_err(dev, minv, p_a, p_b, rho):
    """Error of the device's two products in units of the sum of the magnitudes of their terms (a sum's rounding error is
    bounded relative to that, not to the possibly cancelling sum)."""
    c = rho - 0.5 * (p_a + p_b)
    want = P.turn_dots(minv, p_a, p_b, rho)
    scale = max(float(np.sum(np.abs(minv * p_a * c))), float(np.sum(np.abs(minv * p_b * c))), 1e-300)
    return max(abs(dev[0] - want[0]), abs(dev[1] - want[1])) / scale


def check_leaf(fit, w, end, eps, before, rec, minv, name):
    """One leapfrog of the end ``end`` ("left" / "right") from ``before = (q, p, g)`` as the device held them."""
    lay = fit.lay
    q0, p0, g0 = before
    q1, p1, g1 = (fit.peek(f"{end}_{x}") for x in "qpg")
    p_half = p0 - (0.5 * eps) * g0
    w.note(name + ".q", rel(q1, q0 + eps * (minv * p_half)), 1e-14)
    u, g = fit.pg(q1)                                        # from the device's own q'
    sites = lay.site_slices()
    for sname, sl in zip(lay.names(), sites):
        w.note(f"{name}.d{sname}", rel(g1[sl], g[sl]), TERM_TOL)
    w.note(name + ".p", rel(p1, p_half - (0.5 * eps) * g1), 1e-14)
    w.note(name + ".U", abs(rec[0] - u) / abs(u), TERM_TOL)
    w.note(name + ".kinetic", abs(rec[1] - P.kinetic(p1, minv)) / P.kinetic(p1, minv), TERM_TOL)
    assert rec[2] == rec[0] + rec[1] and rec[25] == 1.0
    return q1, p1, g1


def check_leapfrogs(fit, q0, eps, minv, tag):
    """set_init, the momentum draw of transition 3, a doubling at depth 1 to the right (leaf 0: a checkpoint; leaf 1: closes
    it and the whole tree), then a doubling at depth 0 to the left."""
    lay, w = fit.lay, _Worst(tag)
    u_dev = fit.set_init(q0)
    u0, g0 = fit.pg(q0)
    np.testing.assert_array_equal(fit.peek("q"), q0)
    w.note("init.U", abs(u_dev - u0) / abs(u0), TERM_TOL)
    for sname, sl in zip(lay.names(), lay.site_slices()):
        w.note(f"init.d{sname}", rel(fit.peek("g")[sl], g0[sl]), TERM_TOL)
    np.testing.assert_array_equal(fit.peek("minv"), np.ones(lay.N))
    fit.set_adapt(eps, minv)
    g_dev = fit.peek("g")
    rec = fit.leapfrog(3, 1, 1, 0, 1)
    # the draw: the left end still holds it
    p0 = fit.peek("left_p")
    w.note("momentum", float(np.max(np.abs(p0 * np.sqrt(minv) - P.draw_momentum(lay.site_slices(), fit.seed, 3, np.ones(lay.N))))), 1e-12)
    np.testing.assert_array_equal(fit.peek("left_q"), q0)
    np.testing.assert_array_equal(fit.peek("left_g"), g_dev)
    np.testing.assert_array_equal(fit.peek("rho"), p0)
    w.note("kinetic0", abs(rec[26] - P.kinetic(p0, minv)) / P.kinetic(p0, minv), TERM_TOL)
    q1, p1, g1 = check_leaf(fit, w, "right", eps, (q0, p0, g_dev), rec, minv, "leaf0")
    np.testing.assert_array_equal(fit.peek("rsum"), p1)
    np.testing.assert_array_equal(fit.peek("ckpt_p"), p1)
    np.testing.assert_array_equal(fit.peek("ckpt_sum"), p1)
    assert not np.any(rec[3:25])                              # an even leaf below the top closes nothing
    rec = fit.leapfrog(3, 0, 1, 1, 1)
    q2, p2, g2 = check_leaf(fit, w, "right", eps, (q1, p1, g1), rec, minv, "leaf1")
    rsum = fit.peek("rsum")
    w.note("rsum", rel(rsum, p1 + p2), 1e-15)
    w.note("subtree dots", _dots_err(rec[3:5], minv, p1, p2, (rsum - p1) + p1), TERM_TOL)
    w.note("tree dots", _dots_err(rec[3 + TOP: 5 + TOP], minv, p0, p2, p0 + rsum), TERM_TOL)
    assert not np.any(rec[5: 3 + TOP])
    np.testing.assert_array_equal(fit.peek("left_p"), p0)      # the other end has not moved
    rec = fit.leapfrog(3, 0, -1, 0, 0)
    _, pl, _ = check_leaf(fit, w, "left", -eps, (q0, p0, g_dev), rec, minv, "back")
    np.testing.assert_array_equal(fit.peek("rsum"), pl)
    w.note("back tree dots", _dots_err(rec[3 + TOP: 5 + TOP], minv, p2, pl, p0 + pl), TERM_TOL)
    np.testing.assert_array_equal(fit.peek("right_p"), p2)
    w.show()


# p per view, n, k: the smallest shapes that reach the plain kernel with several row chunks (37 x 21, n = 50), the MFMA kernel
# with two chunks and a partial 16-row block (1030 x 517, n = 41), two and more strips of one view (2050 x 5; 1030 x 517), and
# ptot both above (2050 x 5, 300 x 9001) and below (5 x 3 with k = 1 .. equal; 130 x 64 with k = 16) n k in the fold kernel
SHAPES = [
    ((5, 3), 9, 1),
    ((37, 21), 50, 3),
    ((2050, 5), 19, 2),
    ((1030, 517), 41, 5),
    ((130, 64), 33, 16),
    ((1024, 2049, 70), 67, 17),
    ((300, 9001), 37, 32),
]
SHAPE_IDS = [f"{'x'.join(map(str, s[0]))}_n{s[1]}_k{s[2]}" for s in SHAPES]
# ld > p with poisoned padding and a base pointer 4 (fp32) or 8 bytes off a 16-byte boundary; NULL means; one NULL entry
LAYOUTS = [(3, 1, "auto"), (1, 2, "none"), (0, 0, "one_null")]
LAYOUT_SHAPES = (SHAPES[1], SHAPES[3])


def _shape_views(shape, dtype):
    dims, n, _ = shape
    rng = np.random.default_rng(len(dims) * 1000 + n)
    zt = rng.standard_normal((n, 2))
    return [(zt @ rng.standard_normal((2, d)) + rng.standard_normal((n, d)) + 0.5).astype(dtype) for d in dims], rng


def _set_state(rng, lay):
    """A moderate point (uniform(-2, 2) on W and z would put |R| in the hundreds for the wide shapes), a small step and an
    uneven inverse mass."""
    q0 = 0.5 * P.init_point(rng, lay)
    return q0, 0.01, rng.uniform(0.5, 2.0, size=lay.N)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_leapfrog_kernels(shape, dtype):
    views, rng = _shape_views(shape, dtype)
    layouts = LAYOUTS if shape in LAYOUT_SHAPES else [(0, 0, "auto")]
    for pad, offset, meanmode in layouts:
        means = "auto"
        if meanmode == "none":
            means = None
        elif meanmode == "one_null":
            means = [v.mean(axis=0).astype(dtype) for v in views]
            means[len(views) // 2] = None
        fit = _Fit(views, shape[2], pad=pad, offset=offset, means=means)
        try:
            q0, eps, minv = _set_state(rng, fit.lay)
            check_leapfrogs(fit, q0, eps, minv, f"{np.dtype(dtype).name} {shape[0]} pad{pad} off{offset} {meanmode}")
            assert fit.status() == dict(transitions=0, stopped=0, bad=-1)
        finally:
            fit.close()


def test_table_reaches_both_kernels_strips_chunks_and_both_fold_regimes():
    seen = {(path, what): False for path in ("plain", "mfma") for what in ("strips", "chunks")}
    fold = {"ptot_above_nk": False, "ptot_below_nk": False}
    for shape in SHAPES:
        views, _ = _shape_views(shape, np.float32)
        fit = _Fit(views, shape[2])
        try:
            pl = fit.plan()
        finally:
            fit.close()
        path = "plain" if shape[2] <= 4 else "mfma"
        assert pl["strips"] == [(p + 255) // 256 for p in shape[0]] and pl["rc"] % 16 == 0 and pl["nchunk"] == -(-shape[1] // pl["rc"])
        assert pl["slots"] == 15 + 2 * 5
        seen[(path, "strips")] |= max(pl["strips"]) >= 2
        seen[(path, "chunks")] |= pl["nchunk"] >= 2
        fold["ptot_above_nk" if sum(shape[0]) > shape[1] * shape[2] else "ptot_below_nk"] = True
    assert all(seen.values()) and all(fold.values()), (seen, fold)


# ---- the Welford update and a window end ------------------------------------------------------------------------------------
def test_welford_updates_and_window_end_match_numpy():
    """20 warm-up transitions one at a time: after each transition of the middle window (3 .. 17) the Welford mean and M2
    against NumPy on the device's own points; at its end minv against np.var and the shrinkage formula, the state reset."""
    views, k, center, random_state = traj_case("two_f64")
    fit = _Fit(views, k, num_warmup=20, num_samples=1, depth=TRAJ_DEPTH, seed=random_state, means="auto" if center else None)
    try:
        fit.set_init(P.init_point(np.random.default_rng(random_state), fit.lay))
        points, worst = [], 0.0
        for t in range(20):
            fit.run(1)
            q = fit.peek("q")
            count = fit.peek("scalars")[2]
            if 3 <= t < 17:
                points.append(q)
                x = np.array(points)
                assert count == len(points)
                worst = max(worst, rel(fit.peek("wmean"), x.mean(axis=0)), rel(fit.peek("wm2"), ((x - x.mean(axis=0)) ** 2).sum(axis=0)) if t > 3 else 0.0)
            elif t == 17:
                x = np.array(points + [q])
                c = 15.0
                want = (c / (c + 5.0)) * np.var(x, axis=0, ddof=1) + 1e-3 * (5.0 / (c + 5.0))
                worst = max(worst, rel(fit.peek("minv"), want))
                assert count == 0 and not fit.peek("wmean").any() and not fit.peek("wm2").any()
            else:
                assert count == 0
                if t < 3:
                    np.testing.assert_array_equal(fit.peek("minv"), np.ones(fit.lay.N))
        print(f"welford / window end worst {worst:.1e}")
        assert worst <= TERM_TOL
    finally:
        fit.close()


# ---- whole transitions from a set state ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TRAJ_CASES))
def test_transitions_from_a_set_state_match_the_restatement(name):
    """Two transitions of depth 5 (31 leapfrogs each, every checkpoint level): the record equal, q, accept_prob and U within
    1e-10 (conditioned to 1e-12 on the host).  Measured worst: q 1.8e-15, accept_prob 2.7e-14."""
    views, k, center, random_state = traj_case(name)
    end, want = traj_run(name), transition_case(name)
    fit = _Fit(views, k, num_warmup=0, num_samples=2, depth=5, seed=random_state, means="auto" if center else None)
    try:
        fit.set_init(end["q"])
        fit.set_adapt(TRANSITION_STEP * end["step_size"], end["minv"])
        draws = np.empty((2, fit.lay.N))
        fit.run(2, draws)
        stats, _, _ = fit.stats(2)
        for t, (q, u, rec) in enumerate(want):
            assert (stats["tree_depth"][t], stats["n_leapfrog"][t], stats["diverging"][t]) == (rec["tree_depth"], rec["n_leapfrog"], rec["diverging"])
            err = float(np.max(np.abs(draws[t] - q)))
            print(f"transition {name} {t}: q {err:.1e} accept {abs(stats['accept_prob'][t] - rec['accept_prob']):.1e}")
            assert err <= 1e-10 and abs(stats["accept_prob"][t] - rec["accept_prob"]) <= 1e-10
            assert abs(stats["potential_energy"][t] - u) <= 1e-10 * abs(u)
        assert fit.status() == dict(transitions=2, stopped=0, bad=-1)
        with pytest.raises(ValueError, match="more transitions"):
            fit.run(1)
    finally:
        fit.close()


# ---- conditioned trajectories against the restatement ---------------------------------------------------------------------------
def _model(k, **over):
    from cca_zoo_amd.probabilistic import ProbabilisticCCA

    par = dict(latent_dimensions=k, num_warmup=TRAJ_WARMUP, num_samples=TRAJ_SAMPLES, max_tree_depth=TRAJ_DEPTH)
    par.update(over)
    return ProbabilisticCCA(**par)


@pytest.fixture(scope="module")
def traj_fits():
    """One fit per trajectory case from host arrays, shared by the tests that compare against it (never modified)."""
    cache = {}

    def get(name):
        if name not in cache:
            views, k, center, random_state = traj_case(name)
            cache[name] = _model(k, center=center, random_state=random_state).fit(views)
        return cache[name]

    return get


@pytest.mark.parametrize("name", sorted(TRAJ_CASES))
def test_trajectory_matches_the_restatement(name):
    """20 warm-up and 5 kept transitions through the C ABI: the discrete record equal, every W_i column of every kept draw
    and every U within 1e-8 (the cases are conditioned to 1e-10: tests/test_pcca_host.py)."""
    views, k, center, random_state = traj_case(name)
    ref = traj_run(name)
    lay = ref["layout"]
    total = TRAJ_WARMUP + TRAJ_SAMPLES
    fit = _Fit(views, k, num_warmup=TRAJ_WARMUP, num_samples=TRAJ_SAMPLES, depth=TRAJ_DEPTH, seed=random_state,
               means="auto" if center else None)
    try:
        fit.set_init(P.init_point(np.random.default_rng(random_state), lay))
        draws = np.empty((TRAJ_SAMPLES, lay.N))
        fit.run(total, draws)
        stats, step, minv = fit.stats(total)
    finally:
        fit.close()
    for key in ("tree_depth", "n_leapfrog", "diverging"):
        np.testing.assert_array_equal(stats[key], ref["stats"][key])
    werr = max(col_err(lay.W(draws[d], i), lay.W(ref["draws"][d], i)) for d in range(TRAJ_SAMPLES) for i in range(lay.m))
    uerr = float(np.max(np.abs(stats["potential_energy"] - ref["stats"]["potential_energy"]) / np.abs(ref["stats"]["potential_energy"])))
    serr = float(np.max(np.abs(stats["step_size"] - ref["stats"]["step_size"]) / ref["stats"]["step_size"]))
    print(f"trajectory {name}: W col err {werr:.2e} U {uerr:.2e} step sizes {serr:.2e} minv {rel(minv, ref['minv']):.2e}")
    assert werr <= W_TOL and uerr <= W_TOL and serr <= W_TOL and rel(minv, ref["minv"]) <= W_TOL
    assert abs(step - ref["step_size"]) <= W_TOL * ref["step_size"]


# ---- the estimator ---------------------------------------------------------------------------------------------------------
#: the aligned draws are the raw ones (1e-8) times a rotation that is the polar factor of a k x k sum over the draws: a
#: factor 10 for its conditioning
FIT_TOL = 1e-7


@pytest.mark.parametrize("name", ["two_f64", "wide_f32_k5"])
def test_estimator_matches_the_restatement_driven_expectation(name, traj_fits):
    from cca_zoo_amd.probabilistic._posterior import align_posterior_rotation

    views, k, center, random_state = traj_case(name)
    model = traj_fits(name)
    ref = P.fit_expectation(views, k, random_state, TRAJ_WARMUP, TRAJ_SAMPLES, TRAJ_DEPTH, center=center)
    lay = ref["layout"]
    for key in ("tree_depth", "n_leapfrog", "diverging"):
        np.testing.assert_array_equal(model.sample_stats_[key], ref["stats"][key])
    assert model.sample_stats_["tree_depth"].dtype == np.int64 and model.sample_stats_["diverging"].dtype == bool
    assert model.n_divergent_ == int(ref["stats"]["diverging"][TRAJ_WARMUP:].sum()) and model.n_components_ == k
    assert abs(model.step_size_ - ref["step_size"]) <= W_TOL * ref["step_size"]
    raw_w = ref["draws"][:, : lay.oS].reshape(TRAJ_SAMPLES, lay.ptot, k)
    aligned, rotations = align_posterior_rotation(raw_w)
    assert set(model.posterior_samples_) == set(lay.names()) == set(model.inverse_mass_matrix_)
    for i in range(lay.m):
        want = aligned[:, lay.off[i]: lay.off[i + 1]]
        assert model.posterior_samples_[f"W_{i}"].shape == want.shape and rel(model.posterior_samples_[f"W_{i}"], want) <= FIT_TOL
        assert rel(model.posterior_samples_[f"log_psi_{i}"], ref["draws"][:, lay.s_slice(i)]) <= W_TOL
        assert rel(model.inverse_mass_matrix_[f"W_{i}"], lay.W(ref["minv"], i)) <= W_TOL
        w = model.weights_[i]
        assert w.dtype == np.float64 and w.shape == (views[i].shape[1], k) and rel(w, want.mean(axis=0)) <= FIT_TOL
        assert model.means_[i].dtype == views[i].dtype
        np.testing.assert_array_equal(model.means_[i], ref["means"][i])
    z = np.einsum("snk,skj->snj", ref["draws"][:, lay.z_slice()].reshape(TRAJ_SAMPLES, lay.n, k), rotations)
    assert rel(model.posterior_samples_["z"], z) <= FIT_TOL


def _same_fit(a, b):
    for x, y in zip(a.weights_, b.weights_):
        np.testing.assert_array_equal(x, y)
    for key in a.posterior_samples_:
        np.testing.assert_array_equal(a.posterior_samples_[key], b.posterior_samples_[key])
    for key in a.sample_stats_:
        np.testing.assert_array_equal(a.sample_stats_[key], b.sample_stats_[key])
    for key in a.inverse_mass_matrix_:
        np.testing.assert_array_equal(a.inverse_mass_matrix_[key], b.inverse_mass_matrix_[key])
    assert a.step_size_ == b.step_size_


@pytest.mark.parametrize("name", ["three_f32", "wide_f32_k5"])
def test_two_fits_are_bit_identical(name, traj_fits):
    views, k, center, random_state = traj_case(name)
    _same_fit(_model(k, center=center, random_state=random_state).fit(views), traj_fits(name))


@pytest.mark.parametrize("name", ["two_f64", "three_f32"])
def test_cuda_tensors_give_the_same_bits_and_stay_unchanged(name, traj_fits):
    import torch

    views, k, center, random_state = traj_case(name)
    tens = [torch.as_tensor(v, device="cuda") for v in views]
    before = [t.clone() for t in tens]
    model = _model(k, center=center, random_state=random_state).fit(tens)
    for a, b in zip(tens, before):
        assert torch.equal(a, b)
    host = traj_fits(name)
    for a, b in zip(model.means_, host.means_):
        np.testing.assert_array_equal(a, b)
    _same_fit(model, host)


@pytest.mark.parametrize("name", ["two_f64", "three_f32", "two_f64_nocenter"])
def test_held_out_outputs_match_the_mixin_formulas(name, traj_fits):
    """transform / score / log_likelihood against cca_zoo/probabilistic/_utils.py:11-109, :217-291 written out in NumPy, at
    the bars tests/test_gpu_vbcca.py uses (1e-7 for fp64 views, 1e-3 for fp32 views)."""
    import torch

    model = traj_fits(name)
    seed, n, p, _, dtype, _, _ = TRAJ_CASES[name]
    rng = np.random.default_rng(seed + 100)
    test = [rng.standard_normal((15, pi)).astype(dtype) for pi in p]
    bar = 1e-3 if dtype == np.float32 else 1e-7
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


def test_non_finite_initial_potential_raises():
    from cca_zoo_amd.probabilistic import ProbabilisticCCA

    rng = np.random.default_rng(0)
    X = [1e200 * rng.standard_normal((12, 5)), rng.standard_normal((12, 4))]
    with pytest.raises(FloatingPointError, match="initial point"):
        ProbabilisticCCA(num_warmup=3, num_samples=2).fit(X)
    # the C ABI: the fit is stopped, every kernel a no-op, run refuses
    fit = _Fit(X, 1, num_warmup=0, num_samples=2)
    try:
        assert math.isnan(fit.set_init(np.ones(fit.lay.N)))
        assert fit.status() == dict(transitions=0, stopped=1, bad=0)
        with pytest.raises(ValueError, match="stopped"):
            fit.run(1)
    finally:
        fit.close()


def test_guards():
    from cca_zoo_amd import _backend

    # the C ABI refuses the limits, a single view, a single row, an empty view, a tree depth out of range, and slots that
    # would not fit (35 slots of more than 2^35 doubles), all before any device work
    h = _backend.default_handle()
    state = C.c_void_p()
    for p, n, k, depth in (([5, 5], 40, 33, 5), ([5] * 9, 40, 2, 5), ([5], 40, 2, 5), ([5, 5], 1, 2, 5), ([5, 0], 40, 2, 5),
                           ([5, 5], 40, 2, 0), ([5, 5], 40, 2, 11), ([2 ** 30, 5], 2 ** 30, 32, 10)):
        m = len(p)
        rc = h.lib.ccz_nuts_create(h.raw, _backend.F64, m, (C.c_int64 * m)(*p), n, k, 10, 10, depth, 0.8, 0, C.byref(state))
        assert rc != 0 and not state.value, (p, n, k, depth)


# ---- one statistical case ---------------------------------------------------------------------------------------------------
#: the restatement's CPU run of this configuration over random_state 0 .. 4 gives the cosine of the largest principal angle
#: 0.9963, 0.9964, 0.9962, 0.9964, 0.9964: the bound is its minimum less 0.05
PLANTED_BOUND = 0.9962 - 0.05


def test_planted_two_factor_loadings_are_recovered():
    """Measured on the device: 0.9962, no divergence after warm-up, 8596 leapfrogs."""
    from cca_zoo_amd.probabilistic import ProbabilisticCCA

    views, loadings = planted(21, 60, (6, 5), 2, np.float64)
    model = ProbabilisticCCA(latent_dimensions=2, num_warmup=150, num_samples=100, max_tree_depth=6, random_state=0).fit(views)
    qa, qb = np.linalg.qr(np.concatenate(model.weights_))[0], np.linalg.qr(np.concatenate(loadings))[0]
    cosine = float(np.linalg.svd(qa.T @ qb, compute_uv=False).min())
    print(f"planted: cosine of the largest principal angle {cosine:.4f} (bound {PLANTED_BOUND:.4f}), divergent {model.n_divergent_}, "
          f"leapfrogs {int(model.sample_stats_['n_leapfrog'].sum())}, step {model.step_size_:.3f}")
    assert cosine >= PLANTED_BOUND and model.n_divergent_ == 0
