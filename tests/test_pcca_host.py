"""CPU tests of ProbabilisticCCA: no reference run is possible (numpyro is not installed), so the NumPy restatement of the
sampler (``tests/pcca_restatement.py``) is anchored here -- its potential against ``scipy.stats``, its gradient against
central differences, the leapfrog's reversibility and order, dual averaging by hand, the windows against hand-listed ones, the
window-end variance against ``np.var``, the whole sampler on a toy Gaussian -- the alignment is held to goldens of the
reference's own function, and the estimator's surface and guards are checked as far as they go without a device.  The cases
of the device trajectories (``tests/test_gpu_pcca.py``) are defined here and checked for conditioning."""

import math
import os

import numpy as np
import pytest

import pcca_restatement as P
from test_vbcca_host import col_err, planted  # noqa: F401  (col_err is re-exported to the GPU tests)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
#: the trajectory cases must be conditioned two orders below the 1e-8 device bar (as test_vbcca_host.RESTATE_TOL)
RESTATE_TOL = 1e-10
TRAJ_WARMUP, TRAJ_SAMPLES, TRAJ_DEPTH = 20, 5, 3

#: name -> (views seed, n, p, k, dtype, center, random_state): 2 and 3 views, fp64 and fp32, center=False, p > n with k = 5
#: (the MFMA kernel).  20 warm-up transitions have the windows (0, 2), (3, 17), (18, 19): the middle one ends inside the
#: run, so minv is updated at transition 17 (below 20 there is a single window and, as in numpyro, no mass adaptation).
TRAJ_CASES = {
    "two_f64": (11, 12, (7, 5), 2, np.float64, True, 7),
    "three_f32": (12, 10, (6, 4, 5), 3, np.float32, True, 5),
    "two_f64_nocenter": (13, 11, (9, 4), 2, np.float64, False, 6),
    "wide_f32_k5": (14, 8, (20, 17), 5, np.float32, True, 7),
}
TRANSITION_STEP = 0.25
DISCRETE = ("tree_depth", "n_leapfrog", "diverging", "chosen")


def traj_case(name):
    seed, n, p, k, dtype, center, random_state = TRAJ_CASES[name]
    views, _ = planted(seed, n, p, 2, dtype)
    return views, k, center, random_state


_TRAJ = {}


def traj_run(name, perturb=False):
    """The restatement's run of a case (cached, never modified); ``perturb`` scales every gradient entry by
    1 +- 1e-13 (alternating signs)."""
    if (name, perturb) not in _TRAJ:
        views, k, center, random_state = traj_case(name)
        means = [v.mean(axis=0) for v in views] if center else None
        lay = P.Layout([v.shape[1] for v in views], views[0].shape[0], k)
        q0 = P.init_point(np.random.default_rng(random_state), lay)
        sign = np.where(np.arange(lay.N) % 2 == 0, 1.0, -1.0)
        wrap = (lambda g: g * (1.0 + 1e-13 * sign)) if perturb else None
        _TRAJ[(name, perturb)] = P.run_model(views, means, k, q0, random_state, TRAJ_WARMUP, TRAJ_SAMPLES, TRAJ_DEPTH, wrap=wrap)
    return _TRAJ[(name, perturb)]


def transition_case(name, perturb=False):
    """Two transitions from the END of a case's restatement run (a point of the typical set, a quarter of the adapted step
    size -- at which the trees reach depth 5 without a divergence, so every checkpoint level is used -- and the adapted
    minv), as ``ccz_nuts_run`` takes them on a fresh state with no warm-up: the list of ``(q, U, record)``."""
    views, k, center, random_state = traj_case(name)
    end = traj_run(name)
    lay = end["layout"]
    xc = P.centred(views, [v.mean(axis=0) for v in views] if center else None)
    sign = np.where(np.arange(lay.N) % 2 == 0, 1.0, -1.0)
    pg = P.model_pg(lay, xc, (lambda g: g * (1.0 + 1e-13 * sign)) if perturb else None)
    q = end["q"]
    u, g = pg(q)
    out = []
    for t in range(2):
        p0 = P.draw_momentum(lay.site_slices(), random_state, t, end["minv"])
        q, u, g, rec = P.transition(pg, q, u, g, TRANSITION_STEP * end["step_size"], end["minv"], p0, P.stream(random_state, t, len(lay.site_slices())), 5)
        out.append((q, u, rec))
    return out


def small_problem(m, k, seed=0):
    p = (5, 4, 3)[:m]
    views, _ = planted(seed, 6, p, 2)
    xc = P.centred(views, [v.mean(axis=0) for v in views])
    lay = P.Layout(p, 6, k)
    q = P.init_point(np.random.default_rng(seed + 1), lay)
    return lay, xc, q


# ---- (a), (b): the potential and its gradient ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,k", [(2, 1), (2, 3), (3, 1), (3, 3)])
def test_potential_matches_scipy(m, k):
    from scipy import stats

    lay, xc, q = small_problem(m, k)
    u, _ = P.potential_and_grad(lay, q, xc)
    z = lay.Z(q)
    lp = np.sum(stats.norm.logpdf(z))
    for i in range(m):
        w, s = lay.W(q, i), lay.s(q, i)
        lp += np.sum(stats.norm.logpdf(w)) + np.sum(stats.norm.logpdf(s))
        lp += np.sum(stats.norm.logpdf(xc[i], z @ w.T, np.exp(s)))         # exp(log_psi) is the standard deviation
    assert abs(u + lp) <= 1e-10 * abs(u)


@pytest.mark.parametrize("m,k", [(2, 1), (2, 3), (3, 1), (3, 3)])
def test_gradient_matches_central_differences(m, k):
    lay, xc, q = small_problem(m, k)
    _, g = P.potential_and_grad(lay, q, xc)
    fd = np.empty(lay.N)
    for e in range(lay.N):
        h = 1e-6 * max(1.0, abs(q[e]))
        d = np.zeros(lay.N)
        d[e] = h
        fd[e] = (P.potential_and_grad(lay, q + d, xc)[0] - P.potential_and_grad(lay, q - d, xc)[0]) / (2 * h)
    for sl in lay.site_slices():
        assert np.max(np.abs(g[sl] - fd[sl])) <= 1e-6 * np.max(np.abs(g[sl]))


# ---- (c): the leapfrog ------------------------------------------------------------------------------------------------
def test_leapfrog_is_reversible_and_second_order():
    lay, xc, q = small_problem(2, 2)
    pg = P.model_pg(lay, xc)
    rng = np.random.default_rng(3)
    minv = rng.uniform(0.5, 2.0, size=lay.N)
    p = rng.standard_normal(lay.N) / np.sqrt(minv)
    q = 0.3 * q                                 # a moderate point: the energy error is then in its asymptotic regime
    u0, g0 = pg(q)
    q1, p1, g1, _ = P.leapfrog(pg, q, p, g0, 1e-3, minv)
    q2, p2, _, _ = P.leapfrog(pg, q1, p1, g1, -1e-3, minv)
    assert np.max(np.abs(q2 - q)) <= 1e-13 * np.max(np.abs(q)) and np.max(np.abs(p2 - p)) <= 1e-12 * np.max(np.abs(p))
    h0 = u0 + P.kinetic(p, minv)

    def energy_error(eps, steps):
        qq, pp, gg = q, p, g0
        for _ in range(steps):
            qq, pp, gg, uu = P.leapfrog(pg, qq, pp, gg, eps, minv)
        return abs(uu + P.kinetic(pp, minv) - h0)

    ratio = energy_error(2e-3, 8) / energy_error(1e-3, 16)       # the same time span: a second-order integrator
    print(f"leapfrog energy-error ratio on halving eps: {ratio:.3f}")
    assert 3.5 <= ratio <= 4.5


# ---- (d), (e), (f): the warm-up -------------------------------------------------------------------------------------------
def test_dual_averaging_two_steps_by_hand():
    da = P.DualAverage(math.log(10.0))
    da.update(0.8 - 0.3)
    g1 = 0.5 / 11.0
    x1 = math.log(10.0) - 1.0 / 0.05 * g1
    assert da.g_avg == pytest.approx(g1, rel=1e-15) and da.x == pytest.approx(x1, rel=1e-15)
    assert da.x_avg == pytest.approx(x1, rel=1e-15)              # weight 1^-0.75 = 1
    da.update(0.8 - 1.0)
    g2 = (1.0 - 1.0 / 12.0) * g1 + (-0.2) / 12.0
    x2 = math.log(10.0) - math.sqrt(2.0) / 0.05 * g2
    w = 2.0 ** -0.75
    assert da.g_avg == pytest.approx(g2, rel=1e-14) and da.x == pytest.approx(x2, rel=1e-14)
    assert da.x_avg == pytest.approx((1.0 - w) * x1 + w * x2, rel=1e-14)


def test_window_schedule_against_hand_listed_windows():
    assert P.window_schedule(8) == [(0, 7)]
    assert P.window_schedule(19) == [(0, 18)]
    assert P.window_schedule(20) == [(0, 2), (3, 17), (18, 19)]
    assert P.window_schedule(100) == [(0, 14), (15, 89), (90, 99)]
    assert P.window_schedule(150) == [(0, 74), (75, 99), (100, 149)]
    assert P.window_schedule(500) == [(0, 74), (75, 99), (100, 149), (150, 249), (250, 449), (450, 499)]


def test_window_end_variance_against_numpy():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((15, 6)) * np.array([0.1, 0.5, 1.0, 2.0, 5.0, 10.0]) + 3.0
    wf = P.Welford(6)
    for row in x:
        wf.update(row)
    c = 15.0
    want = (c / (c + 5.0)) * np.var(x, axis=0, ddof=1) + 1e-3 * (5.0 / (c + 5.0))
    np.testing.assert_allclose(wf.mean, x.mean(axis=0), rtol=1e-13)
    np.testing.assert_allclose(wf.regularised_variance(), want, rtol=1e-12)


# ---- (g): the sampler on a toy target --------------------------------------------------------------------------------------
def test_sampler_on_a_diagonal_gaussian():
    """A 5-dimensional diagonal Gaussian whose variances span 100x, 500 warm-up transitions and 2000 draws.  Mean and
    variance of every coordinate within 4 Monte-Carlo standard errors (batch means, 20 batches of 100).  Measured z-scores
    with this seed: see the comment at the assertion."""
    var = np.array([0.1, 0.3, 1.0, 3.0, 10.0])
    mean = np.array([1.0, -2.0, 0.5, 0.0, 3.0])

    def pg(q):
        d = q - mean
        return 0.5 * float(np.sum(d * d / var)), d / var

    res = P.sample(pg, np.zeros(5), [slice(0, 5)], 11, 500, 2000)
    draws = res["draws"]
    assert not res["stats"]["diverging"][500:].any()
    z = []
    for series, truth in ((draws, mean), ((draws - mean) ** 2, var)):
        batches = series.reshape(20, 100, 5).mean(axis=1)
        se = batches.std(axis=0, ddof=1) / math.sqrt(20.0)
        z.append((series.mean(axis=0) - truth) / se)
    print("toy z-scores mean", np.round(z[0], 2), "variance", np.round(z[1], 2), "minv", np.round(res["minv"], 3),
          "step", round(res["step_size"], 3))
    # measured: mean [-0.35 -1.43 -0.43  0.94 -0.  ], variance [-1.05 -1.07 -0.73  1.01 -1.89]: the worst is 1.89 of the 4 allowed;
    # minv [0.093 0.319 1.118 2.373 9.19 ] against the variances [0.1 0.3 1 3 10]
    assert np.max(np.abs(z)) <= 4.0
    assert np.all(np.diff(res["minv"]) > 0)                      # the adapted inverse mass is ordered like the variances
    assert np.all(np.abs(np.log(res["minv"] / var)) <= math.log(2.0))


# ---- (h): the alignment against the reference's own function ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["pcca_align_k3", "pcca_align_k1"])
def test_alignment_matches_the_reference_goldens(name):
    from cca_zoo_amd.probabilistic._posterior import align_posterior_rotation

    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    aligned, rotations = align_posterior_rotation(g["w_samples"])
    assert aligned.shape == g["aligned"].shape and rotations.shape == g["rotations"].shape
    err_a = float(np.max(np.abs(aligned - g["aligned"])))
    err_r = float(np.max(np.abs(rotations - g["rotations"])))
    print(f"alignment {name}: aligned {err_a:.1e} rotations {err_r:.1e}")
    assert err_a <= 1e-12 and err_r <= 1e-12
    if name.endswith("k1"):
        assert set(np.round(rotations.reshape(-1)).astype(int)) == {-1, 1}          # the sign-flip case has both signs


# ---- (i): surface, parameters, guards --------------------------------------------------------------------------------------
def test_surface_and_get_params():
    import cca_zoo_amd.probabilistic as prob
    from cca_zoo_amd.probabilistic import ProbabilisticCCA
    from cca_zoo_amd.probabilistic._posterior import PosteriorMeanMixin
    from sklearn.base import clone

    assert prob.__all__ == ["GFA"]
    m = ProbabilisticCCA()
    assert m.get_params() == dict(latent_dimensions=1, center=True, num_warmup=500, num_samples=1000, random_state=0,
                                  max_tree_depth=10, target_accept_prob=0.8)
    assert clone(ProbabilisticCCA(2, num_warmup=5)).get_params() == ProbabilisticCCA(2, num_warmup=5).get_params()
    assert isinstance(m, PosteriorMeanMixin)
    assert ProbabilisticCCA.log_likelihood is PosteriorMeanMixin.log_likelihood          # shared, not copied
    assert prob.VariationalBayesCCA.log_likelihood is PosteriorMeanMixin.log_likelihood


def test_parameter_validation_and_guards_without_a_device():
    from sklearn.utils._param_validation import InvalidParameterError

    from cca_zoo_amd.probabilistic import ProbabilisticCCA
    from cca_zoo_amd.probabilistic._pcca import MAX_SAMPLE_BYTES

    rng = np.random.default_rng(0)
    X = [rng.standard_normal((40, 5)), rng.standard_normal((40, 4))]
    for bad in (dict(num_warmup=-1), dict(num_samples=0), dict(max_tree_depth=0), dict(max_tree_depth=11),
                dict(target_accept_prob=1.0), dict(target_accept_prob=0.0), dict(random_state=-1), dict(latent_dimensions=0)):
        with pytest.raises(InvalidParameterError):
            ProbabilisticCCA(**bad).fit(X)
    with pytest.raises(ValueError, match="at most 32"):
        ProbabilisticCCA(latent_dimensions=33).fit(X)
    with pytest.raises(ValueError, match="at most 8 views"):
        ProbabilisticCCA().fit([X[0]] * 9)
    size = 9 * 2 + 9 + 40 * 2
    with pytest.raises(ValueError, match="lower num_samples"):
        ProbabilisticCCA(latent_dimensions=2, num_samples=MAX_SAMPLE_BYTES // (size * 8) + 1).fit(X)


def test_fit_inside_row_sharded_is_refused(monkeypatch):
    from cca_zoo_amd import _dist
    from cca_zoo_amd.probabilistic import ProbabilisticCCA

    monkeypatch.setattr(_dist, "is_sharded", lambda: True)
    rng = np.random.default_rng(0)
    with pytest.raises(NotImplementedError, match="row_sharded"):
        ProbabilisticCCA().fit([rng.standard_normal((40, 5)), rng.standard_normal((40, 4))])


def test_sites_cover_the_flat_layout_in_model_order():
    from cca_zoo_amd.probabilistic import ProbabilisticCCA

    lay = P.Layout((4, 3, 2), 5, 2)
    sites = ProbabilisticCCA._sites([4, 3, 2], 5, 2)
    assert [s[0] for s in sites] == lay.names()
    assert [s[2] for s in sites] == lay.site_slices()
    assert sum(int(np.prod(s[1])) for s in sites) == lay.N


# ---- (j): the device trajectories' cases are conditioned ---------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TRAJ_CASES))
def test_trajectory_cases_are_well_conditioned(name):
    """With every gradient perturbed by a relative 1e-13 the run has the same discrete record and the same positions to
    1e-10: a condition on the inputs, not on the device.  Measured: two_f64 9.9e-13, three_f32 9.6e-13, two_f64_nocenter
    1.4e-11, wide_f32_k5 7.3e-13."""
    a, b = traj_run(name), traj_run(name, perturb=True)
    for key in DISCRETE:
        np.testing.assert_array_equal(a["stats"][key], b["stats"][key])
    err = float(np.max(np.abs(a["draws"] - b["draws"])))
    print(f"conditioning {name}: positions {err:.1e} depths {a['stats']['tree_depth']}")
    assert err <= RESTATE_TOL
    assert len(a["stats"]["tree_depth"]) == TRAJ_WARMUP + TRAJ_SAMPLES and TRAJ_WARMUP >= 8 and TRAJ_SAMPLES >= 5
    assert a["stats"]["tree_depth"].max() >= 3
    assert np.ptp(a["minv"]) > 0                 # the middle window ended inside the run: minv was updated


@pytest.mark.parametrize("name", sorted(TRAJ_CASES))
def test_transition_cases_are_well_conditioned(name):
    """The two set-state transitions of the device test: the same record and the same point to 1e-12 under the perturbation."""
    for (qa, ua, ra), (qb, ub, rb) in zip(transition_case(name), transition_case(name, perturb=True)):
        assert all(ra[key] == rb[key] for key in DISCRETE)
        err = float(np.max(np.abs(qa - qb)))
        print(f"transition conditioning {name}: {err:.1e} depth {ra['tree_depth']}")
        assert err <= 1e-12 and ra["tree_depth"] == 5 and not ra["diverging"]


def test_trajectory_cases_cover_the_required_ground():
    cases = TRAJ_CASES.values()
    assert {len(c[2]) for c in cases} == {2, 3} and {c[4] for c in cases} == {np.float32, np.float64}
    assert any(not c[5] for c in cases) and any(sum(c[2]) > c[1] and c[3] == 5 for c in cases)
