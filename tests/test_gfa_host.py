"""CPU tests of GFA: import surface, parameters and limits, and a float64 NumPy restatement of the fit in the form the
device uses (``fl(x - mu)`` rows read where they lie, the updates of ``csrc/gfa.hip`` in its order), checked against every
golden (the comparator of tests/test_gpu_gfa.py)."""

import glob
import os

import numpy as np
import pytest

from conftest import load_golden

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "gfa_*.npz")))

#: the restatement against the goldens (measured worst 0: the same NumPy operations on the same values give the
#: reference's bits): two orders under the device tolerance of tests/test_gpu_gfa.py, as
#: tests/test_als_host.py sets its bar
RESTATE_TOL = 1e-10

PRIOR, INIT_TAU, DROP_TOL, PATIENCE = 1e-14, 1e3, 1e-7, 1000


def case_params(g):
    import ast

    return dict(ast.literal_eval(str(g["params"])))


def case_views(g, prefix="X"):
    return [g[f"{prefix}{i}"] for i in range(int(g["n_views"]))]


def col_err(w, ref):
    """Largest per-column relative error."""
    num = np.linalg.norm(w - ref, axis=0)
    den = np.maximum(np.linalg.norm(ref, axis=0), 1e-300)
    return float(np.max(num / den))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def spd_inverse(a):
    """inv(a) through the Cholesky factor, as the reference and the device form it."""
    c = np.linalg.cholesky(a)
    return np.linalg.solve(c.T, np.linalg.solve(c, np.eye(a.shape[0])))


def centred(views, center):
    """The rows the device multiplies: ``v - v.mean(0)`` in the views' dtype, then float64; and the means."""
    xs = [np.asarray(v) for v in views]
    xs = [x if x.dtype in (np.float32, np.float64) else x.astype(np.float64) for x in xs]
    means = [x.mean(axis=0) if center else np.zeros(x.shape[1]) for x in xs]
    return [(x - mu if center else x).astype(np.float64) for x, mu in zip(xs, means)], means


def initial_state(xs, z0):
    """The state after ``ccz_gfa_setup`` (``_gfa.py:184-204``)."""
    m, (n, k) = len(xs), z0.shape
    d = [x.shape[1] for x in xs]
    datavar = [np.var(x, axis=0, ddof=1).sum() for x in xs]
    return dict(
        z=z0.copy(), cov_z=np.eye(k), w=[np.zeros((di, k)) for di in d], cov_w=[np.eye(k) for _ in d],
        tau=np.full(m, INIT_TAU), alpha=[np.full(k, k * di / max(dv - 1.0 / INIT_TAU, 1e-8)) for di, dv in zip(d, datavar)],
        y_const=np.array([np.sum(x ** 2) for x in xs]), datavar=np.array(datavar),
        ww=[di * np.eye(k) for di in d], zz=z0.T @ z0 + n * np.eye(k),
        b_ard=[np.full(k, PRIOR) for _ in d], b_tau=np.full(m, PRIOR), xw=[np.zeros((n, k)) for _ in d],
    )


def iterate(xs, s, drop_k=True):
    """One iteration in place, in the order of ``csrc/gfa.hip``; returns (kept columns or None, mean z^2 per column,
    |z - z_prev|_F, |z_prev|_F)."""
    m, n = len(xs), xs[0].shape[0]
    d = [x.shape[1] for x in xs]
    k = s["z"].shape[1]
    for i in range(m):
        t = 1.0 / np.sqrt(s["alpha"][i])
        inner = np.outer(t, t) * s["zz"] + np.eye(k) / s["tau"][i]
        s["cov_w"][i] = (1.0 / s["tau"][i]) * np.outer(t, t) * spd_inverse(inner)
        s["w"][i] = (xs[i].T @ s["z"]) @ s["cov_w"][i] * s["tau"][i]
        s["ww"][i] = s["w"][i].T @ s["w"][i] + d[i] * s["cov_w"][i]
    prec = np.eye(k)
    for i in range(m):
        prec = prec + s["tau"][i] * s["ww"][i]
    s["cov_z"] = spd_inverse(prec)
    s["xw"] = [xs[i] @ s["w"][i] for i in range(m)]
    rhs = np.zeros((n, k))
    for i in range(m):
        rhs = rhs + s["xw"][i] * s["tau"][i]
    prev = s["z"]
    s["z"] = rhs @ s["cov_z"]
    z2 = np.sum(s["z"] ** 2, axis=0) / n
    dz, pz = np.linalg.norm(s["z"] - prev), np.linalg.norm(prev)
    s["zz"] = s["z"].T @ s["z"] + n * s["cov_z"]
    for i in range(m):
        s["b_ard"][i] = PRIOR + np.diag(s["ww"][i]) / 2.0
        s["alpha"][i] = (PRIOR + d[i] / 2.0) / s["b_ard"][i]
        s["b_tau"][i] = PRIOR + (s["y_const"][i] + np.sum(s["ww"][i] * s["zz"]) - 2.0 * np.sum(s["z"] * s["xw"][i])) / 2.0
        s["tau"][i] = (PRIOR + n * d[i] / 2.0) / s["b_tau"][i]
    keep = np.where(z2 > DROP_TOL)[0] if drop_k else np.arange(k)
    if not 0 < len(keep) != k:
        return None, z2, dz, pz
    ix = np.ix_(keep, keep)
    s["z"], s["cov_z"], s["zz"] = s["z"][:, keep], s["cov_z"][ix], s["zz"][ix]
    for i in range(m):
        s["w"][i], s["cov_w"][i], s["ww"][i] = s["w"][i][:, keep], s["cov_w"][i][ix], s["ww"][i][ix]
        s["alpha"][i], s["b_ard"][i] = s["alpha"][i][keep], s["b_ard"][i][keep]
    return keep, z2, dz, pz


def restate(views, latent_dimensions=1, center=True, max_iter=10000, tol=1e-4, drop_k=True, num_posterior_samples=1000,
            random_state=0, trace=None):
    """The fit and the posterior draws in float64 NumPy.  ``trace`` (a list) receives per iteration
    (mean z^2 per column, rel_change or None, y_const / (2 b_tau)).  Returns a dict of the fitted attributes."""
    xs, means = centred(views, center)
    n, p = xs[0].shape[0], [x.shape[1] for x in xs]
    rng = np.random.default_rng(random_state)
    s = initial_state(xs, rng.standard_normal((n, latent_dimensions)))
    stable, n_iter, prunes = 0, max_iter, []
    for it in range(1, max_iter + 1):
        keep, z2, dz, pz = iterate(xs, s, drop_k)
        rc = None
        if keep is not None:
            prunes.append(it)
            stable = 0
        elif it > 1:
            rc = dz / max(pz, 1e-300)
            stable = stable + 1 if rc < tol else 0
        if trace is not None:
            trace.append((z2, rc, s["y_const"] / (2.0 * s["b_tau"])))
        if stable >= PATIENCE:
            n_iter = it
            break
    k, m, ns = s["z"].shape[1], len(xs), num_posterior_samples
    a_ard, a_tau = PRIOR + np.array(p) / 2.0, PRIOR + n * np.array(p) / 2.0
    samples = {"z": s["z"][None] + rng.standard_normal((ns, n, k)) @ np.linalg.cholesky(s["cov_z"]).T}
    taus = np.stack([rng.gamma(a_tau[i], 1.0 / s["b_tau"][i], size=ns) for i in range(m)], axis=1)
    samples["alpha"] = np.stack([rng.gamma(a_ard[i], 1.0 / s["b_ard"][i], size=(ns, k)) for i in range(m)], axis=1)
    for i in range(m):
        samples[f"W_{i}"] = s["w"][i][None] + rng.standard_normal((ns, p[i], k)) @ np.linalg.cholesky(s["cov_w"][i]).T
        samples[f"log_psi_{i}"] = np.log(1.0 / taus[:, i])[:, None] * np.ones((1, p[i]))
    return dict(weights=s["w"], means=means, view_relevance=np.array(s["alpha"]), tau=s["tau"].copy(), n_iter=n_iter,
                n_components=k, prune_iterations=prunes, samples=samples, state=s)


def sample_errors(samples, g):
    """Relative errors of the stored part of the draws (the goldens keep the first rows of the z and W draws)."""
    out = {}
    for key in [k for k in g if k.startswith("S_")]:
        ref, got = g[key], samples[key[2:]]
        out[key[2:]] = rel(got[:, : ref.shape[1]], ref)
    return out


# ---- import surface, parameters, limits -------------------------------------------------------------------------------
def test_import_surface_and_parameters():
    from sklearn.base import clone
    from sklearn.exceptions import NotFittedError
    from sklearn.utils._param_validation import InvalidParameterError

    import cca_zoo_amd.probabilistic as prob
    from cca_zoo_amd.probabilistic import GFA

    assert prob.__all__ == ["GFA"]
    est = GFA()
    assert est.get_params() == dict(latent_dimensions=1, center=True, max_iter=10000, tol=1e-4, drop_k=True,
                                    num_posterior_samples=1000, random_state=0)
    assert clone(GFA(3, tol=1e-3)).get_params() == GFA(3, tol=1e-3).get_params()
    X = [np.zeros((6, 2)), np.zeros((6, 3))]
    with pytest.raises(NotFittedError):
        est.transform(X)
    with pytest.raises(NotFittedError):
        est.log_likelihood(X)
    for bad in (GFA(latent_dimensions=0), GFA(center="yes"), GFA(max_iter=0), GFA(tol=-1.0), GFA(drop_k="no"),
                GFA(num_posterior_samples=0), GFA(random_state=1.5)):
        with pytest.raises(InvalidParameterError):
            bad.fit(X)


def test_limits_are_checked_before_any_device_work():
    from cca_zoo_amd.probabilistic import GFA
    from cca_zoo_amd.probabilistic._gfa import MAX_SAMPLE_BYTES

    X = [np.zeros((6, 2)), np.zeros((6, 3))]
    with pytest.raises(ValueError, match="at most 32"):
        GFA(latent_dimensions=33).fit(X)
    with pytest.raises(ValueError, match="at most 8 views"):
        GFA().fit([np.zeros((6, 2))] * 9)
    with pytest.raises(ValueError, match="lower num_posterior_samples"):
        GFA(latent_dimensions=2, num_posterior_samples=MAX_SAMPLE_BYTES // (6 * 2 * 8) + 1).fit(X)
    with pytest.raises(ValueError, match="At least 2 views"):
        GFA().fit([np.zeros((6, 2))])


def test_fit_inside_row_sharded_is_refused(monkeypatch):
    from cca_zoo_amd import _dist
    from cca_zoo_amd.probabilistic import GFA

    monkeypatch.setattr(_dist, "is_sharded", lambda: True)
    with pytest.raises(NotImplementedError, match="row_sharded"):
        GFA().fit([np.zeros((6, 2)), np.zeros((6, 3))])


# ---- the restatement against the reference's fits ---------------------------------------------------------------------
def test_the_goldens_cover_what_they_should():
    assert len(CASES) >= 6
    gs = [load_golden(f"gfa_{c}") for c in CASES]
    par = [case_params(g) for g in gs]
    assert {int(g["n_views"]) for g in gs} >= {2, 3}
    assert {case_views(g)[0].dtype for g in gs} == {np.dtype(np.float32), np.dtype(np.float64)}
    assert any(q.get("center") is False for q in par) and any(q.get("drop_k") is False for q in par)
    assert any(q["latent_dimensions"] == 1 for q in par)
    assert any(v.shape[1] > v.shape[0] for g in gs for v in case_views(g))
    assert any(len(set(g["prune_iterations"].tolist())) >= 2 for g in gs)
    assert any(1000 < int(g["n_iter"]) < q.get("max_iter", 10000) for g, q in zip(gs, par))
    assert any(int(g["n_iter"]) == q.get("max_iter", 10000) for g, q in zip(gs, par))
    for g in gs:
        assert case_views(g)[0].shape[0] <= 200 and sum(v.shape[1] for v in case_views(g)) <= 350
        assert int(g["num_posterior_samples"]) <= 8


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_the_reference(case):
    g = load_golden(f"gfa_{case}")
    r = restate(case_views(g), **case_params(g))
    assert r["n_iter"] == int(g["n_iter"])
    assert r["n_components"] == int(g["n_components"])
    assert r["prune_iterations"] == [int(i) for i in g["prune_iterations"]]
    worst = 0.0
    for i, w in enumerate(r["weights"]):
        worst = max(worst, col_err(w, g[f"W{i}"]))
        np.testing.assert_array_equal(r["means"][i], g[f"mean{i}"])
    worst = max(worst, rel(r["view_relevance"], g["view_relevance"]), rel(r["tau"], g["tau"]))
    worst = max([worst] + list(sample_errors(r["samples"], g).values()))
    print(f"restatement {case}: worst error {worst:.2e}")
    assert worst <= RESTATE_TOL


def test_cholesky_inverse_is_the_inverse():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((40, 9))
    a = a.T @ a + np.eye(9)
    np.testing.assert_allclose(spd_inverse(a) @ a, np.eye(9), atol=1e-12)
