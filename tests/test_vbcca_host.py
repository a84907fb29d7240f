"""CPU tests of VariationalBayesCCA: no reference run is possible (numpyro is not installed), so the NumPy restatement
(``tests/vbcca_restatement.py``) is anchored here -- its loss against ``scipy.stats``, its gradient against central
differences, its Adam step against a hand computation, a planted case -- and the estimator's surface and guards are checked
as far as they go without a device.  The cases of the device trajectories (``tests/test_gpu_vbcca.py``) are defined here and
checked for conditioning."""

import math

import numpy as np
import pytest

import vbcca_restatement as R

#: the trajectory cases must be conditioned two orders below the 1e-8 device bar (as test_gfa_host.RESTATE_TOL)
RESTATE_TOL = 1e-10
TRAJ_STEPS, TRAJ_LR = 100, 1e-2


def planted(seed, n, p, k_true, dtype=np.float64, noise=0.3):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, k_true))
    loadings = [rng.standard_normal((pi, k_true)) for pi in p]
    views = [(z @ w.T + noise * rng.standard_normal((n, pi))).astype(dtype) for w, pi in zip(loadings, p)]
    return views, loadings


#: name -> (views seed, n, p, k, dtype, center): 2 and 3 views, fp64 and fp32, center=False, p > n (k = 5 takes the MFMA kernel)
TRAJ_CASES = {
    "two_f64": (11, 12, (7, 5), 2, np.float64, True),
    "three_f32": (12, 10, (6, 4, 5), 3, np.float32, True),
    "two_f64_nocenter": (13, 11, (9, 4), 2, np.float64, False),
    "wide_f32_k5": (14, 8, (20, 17), 5, np.float32, True),
}


def traj_case(name):
    seed, n, p, k, dtype, center = TRAJ_CASES[name]
    views, _ = planted(seed, n, p, 2, dtype)
    return views, k, center


def traj_run(name, perturb=False):
    views, k, center = traj_case(name)
    means = [v.mean(axis=0) for v in views] if center else None
    lay = R.Layout([v.shape[1] for v in views], views[0].shape[0], k)
    loc0 = R.init_loc(np.random.default_rng(5), lay)
    return R.run(views, means, k, TRAJ_STEPS, TRAJ_LR, 5, loc0, perturb=perturb)


def col_err(a, b):
    """Largest per-column relative error of a against b."""
    return float(np.max(np.linalg.norm(a - b, axis=0) / np.maximum(np.linalg.norm(b, axis=0), 1e-300)))


def small_problem(m, k, seed=0):
    p = (5, 4, 3)[:m]
    views, _ = planted(seed, 6, p, 2)
    xc = R.centred(views, [v.mean(axis=0) for v in views])
    lay = R.Layout(p, 6, k)
    rng = np.random.default_rng(seed + 1)
    loc = R.init_loc(rng, lay)
    rho = rng.uniform(-3.0, 0.5, size=lay.N)
    eps = R.draw_eps(lay, 7, 0)
    return lay, xc, loc, rho, eps


@pytest.mark.parametrize("m,k", [(2, 1), (2, 3), (3, 1), (3, 3)])
def test_loss_matches_scipy(m, k):
    """(a) the loss equals ``-(log p - log q)`` evaluated with scipy.stats at the same theta, every constant included."""
    from scipy import stats

    lay, xc, loc, rho, eps = small_problem(m, k)
    loss, _, _, theta = R.loss_and_grads(lay, loc, rho, eps, xc)
    a, z = lay.a(theta), lay.Z(theta)
    alpha = np.exp(a)
    lp = np.sum(stats.gamma.logpdf(alpha, a=R.A0, scale=1.0 / R.B0)) + np.sum(a)      # the Jacobian of alpha = exp(a)
    lp += np.sum(stats.norm.logpdf(z))
    for i in range(m):
        w, s = lay.W(theta, i), lay.s(theta, i)
        lp += np.sum(stats.norm.logpdf(w, 0.0, 1.0 / np.sqrt(alpha)))
        lp += np.sum(stats.norm.logpdf(s))
        lp += np.sum(stats.norm.logpdf(xc[i], z @ w.T, np.exp(s)))                      # exp(log_psi) is the standard deviation
    lq = np.sum(stats.norm.logpdf(theta, loc, R.softplus(rho)))
    assert abs(loss - (-(lp - lq))) <= 1e-10 * abs(loss)


@pytest.mark.parametrize("m,k", [(2, 1), (2, 3), (3, 1), (3, 3)])
def test_gradient_matches_central_differences(m, k):
    """(b) d loss / d loc and d loss / d rho of every site against central differences with eps held fixed."""
    lay, xc, loc, rho, eps = small_problem(m, k)
    _, gl, gr, _ = R.loss_and_grads(lay, loc, rho, eps, xc)

    def loss(l, r):
        return R.loss_and_grads(lay, l, r, eps, xc)[0]

    fd_l, fd_r = np.empty(lay.N), np.empty(lay.N)
    for e in range(lay.N):
        h = 1e-6 * max(1.0, abs(loc[e]))
        d = np.zeros(lay.N)
        d[e] = h
        fd_l[e] = (loss(loc + d, rho) - loss(loc - d, rho)) / (2 * h)
        fd_r[e] = (loss(loc, rho + d) - loss(loc, rho - d)) / (2 * h)
    for _, view in lay.sites():
        for an, fd in ((-gl, fd_l), (-gr, fd_r)):
            a, f = view(an), view(fd)
            assert np.max(np.abs(a - f)) <= 1e-6 * np.max(np.abs(a))


def test_adam_step_by_hand():
    """(c) the first step moves every parameter by lr g / (|g| + eps); the second uses the corrected moments."""
    g0, g1, lr = np.array([0.3, -2.0, 1e-9]), np.array([-0.1, 0.5, 2e-9]), 0.01
    x, m, v = R.adam(np.zeros(3), np.zeros(3), np.zeros(3), g0, lr, 0)
    assert np.allclose(x, -lr * g0 / (np.abs(g0) + 1e-8), rtol=1e-13, atol=0)
    x2, m2, v2 = R.adam(x, m, v, g1, lr, 1)
    mh = (0.9 * 0.1 * g0 + 0.1 * g1) / (1 - 0.81)
    vh = (0.999 * 0.001 * g0 ** 2 + 0.001 * g1 ** 2) / (1 - 0.999 ** 2)
    assert np.allclose(x2, x - lr * mh / (np.sqrt(vh) + 1e-8), rtol=1e-13, atol=0)


def test_streams_and_normals():
    """The stream derivation separates steps and sites, and hash_normal is a standard normal."""
    seen = {R.stream(3, t, s) for t in range(50) for s in range(6)}
    assert len(seen) == 300
    x = R.hash_normal(R.stream(3, 0, 0), np.arange(200000, dtype=np.uint64))
    assert abs(x.mean()) < 0.01 and abs(x.std() - 1.0) < 0.01


#: (d) measured over random_state 0..4 with the restatement (n = 80, p = (10, 8), two planted factors, latent_dimensions = 4,
#: PLANTED_STEPS steps at learning_rate 0.02); the thresholds carry a factor 2 of margin
#: measured (ratio of the third-smallest to the second-smallest ard_relevance_, largest principal angle in degrees):
#:   random_state 0: 31.5, 2.6   1: 3.48, 7.0   2: 5.34, 7.4   3: 13.6, 6.0   4: 78.1, 2.5
PLANTED_STEPS = 1500
PLANTED_RATIO_MIN = 3.48 / 2
PLANTED_ANGLE_MAX = 7.4 * 2


def planted_fit(random_state):
    views, loadings = planted(100, 80, (10, 8), 2)
    res = R.fit_expectation(views, 4, PLANTED_STEPS, 0.02, random_state, 200)
    ard = np.sort(res["ard_relevance"])
    ratio = ard[2] / ard[1]                          # the two relevant dimensions against the two shrunk ones
    w = np.concatenate(res["weights"], axis=0)
    keep = np.argsort(res["ard_relevance"])[:2]
    q, _ = np.linalg.qr(w[:, keep])
    t, _ = np.linalg.qr(np.concatenate(loadings, axis=0))
    cosines = np.linalg.svd(q.T @ t, compute_uv=False)
    return ratio, float(np.degrees(np.arccos(np.clip(cosines.min(), -1.0, 1.0))))


@pytest.mark.parametrize("random_state", range(5))
def test_planted_factors_are_found(random_state):
    """(d) two shared factors under latent_dimensions = 4: exactly two ARD precisions stay below the other two, and the
    loadings of those two dimensions span the planted ones."""
    ratio, angle = planted_fit(random_state)
    print(random_state, f"ratio {ratio:.2f} angle {angle:.1f}")
    assert ratio >= PLANTED_RATIO_MIN and angle <= PLANTED_ANGLE_MAX


# measured gaps (W per column, losses relative), 100 steps: two_f64 1.9e-16 4.8e-16; three_f32 1.9e-16 3.1e-16;
# two_f64_nocenter 1.4e-16 3.9e-16; wide_f32_k5 2.1e-16 3.5e-16
@pytest.mark.parametrize("name", sorted(TRAJ_CASES))
def test_trajectory_cases_are_well_conditioned(name):
    """The restatement with every contraction summed in reversed order moves by at most RESTATE_TOL over the steps the
    device tests run: the 1e-8 device bar then measures the device, not the case."""
    a, b = traj_run(name), traj_run(name, perturb=True)
    lay = a["layout"]
    gap_w = max(col_err(lay.W(a["loc"], i), lay.W(b["loc"], i)) for i in range(lay.m))
    gap_l = float(np.max(np.abs(a["losses"] - b["losses"]) / np.abs(b["losses"])))
    print(name, f"W {gap_w:.1e} losses {gap_l:.1e}")
    assert a["bad_step"] == -1 and gap_w <= RESTATE_TOL and gap_l <= RESTATE_TOL


def test_non_finite_loss_step():
    """learning_rate = 1e6 drives the restatement to a non-finite loss at a definite step (the device must name the same)."""
    res = nonfinite_run()
    assert res["bad_step"] >= 1 and not np.isfinite(res["losses"][res["bad_step"]])
    assert np.all(np.isfinite(res["losses"][: res["bad_step"]]))


def nonfinite_case():
    return planted(21, 9, (6, 5), 2)[0]


def nonfinite_run():
    views = nonfinite_case()
    return R.fit_expectation(views, 2, 20, 1e6, 0, 2)


# -- (e) surface, validation, guards -------------------------------------------------------------------------------------
def test_import_surface():
    import cca_zoo_amd.probabilistic as P
    from cca_zoo_amd.probabilistic import GFA, VariationalBayesCCA

    assert P.VariationalBayesCCA is VariationalBayesCCA
    m = VariationalBayesCCA()
    assert m.get_params() == dict(latent_dimensions=1, center=True, num_steps=2000, learning_rate=1e-2, num_posterior_samples=1000,
                                  random_state=0)
    assert isinstance(GFA(), object)


@pytest.mark.parametrize("bad", [dict(num_steps=0), dict(learning_rate=0.0), dict(learning_rate=-1.0), dict(num_posterior_samples=0),
                                 dict(latent_dimensions=0), dict(random_state=-1), dict(random_state=1.5), dict(center="yes")])
def test_parameter_validation(bad):
    from sklearn.utils._param_validation import InvalidParameterError

    from cca_zoo_amd.probabilistic import VariationalBayesCCA

    views = planted(0, 6, (3, 2), 1)[0]
    with pytest.raises(InvalidParameterError):
        VariationalBayesCCA(**bad).fit(views)


def test_guards_before_any_device_work():
    from cca_zoo_amd.probabilistic import VariationalBayesCCA

    views = planted(0, 6, (3, 2), 1)[0]
    with pytest.raises(ValueError, match="at most 32"):
        VariationalBayesCCA(latent_dimensions=33).fit(views)
    with pytest.raises(ValueError, match="at most 8 views"):
        VariationalBayesCCA().fit([views[0]] * 9)
    with pytest.raises(ValueError, match="lower num_posterior_samples"):
        VariationalBayesCCA(latent_dimensions=32, num_posterior_samples=2 ** 22).fit(views)
    with pytest.raises(ValueError, match="at least 2 samples"):
        VariationalBayesCCA().fit([v[:1] for v in views])


def test_site_table_matches_the_restatement_layout():
    from cca_zoo_amd.probabilistic import VariationalBayesCCA

    p, n, k = [4, 3, 5], 6, 2
    lay = R.Layout(p, n, k)
    flat = np.arange(lay.N, dtype=np.float64)
    sites = VariationalBayesCCA._sites(p, n, k)
    assert [s[0] for s in sites] == ["log_alpha", "W_0", "log_psi_0", "W_1", "log_psi_1", "W_2", "log_psi_2", "z"]
    for (name, shape, sl), (_, view) in zip(sites, lay.sites()):
        assert np.array_equal(flat[sl].reshape(shape), view(flat))
    assert sites[-1][2].stop == lay.N
