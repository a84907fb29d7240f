#!/usr/bin/env python3
"""Capture golden vectors of the reference's GFA (``cca_zoo/probabilistic/_gfa.py``).

Same shims as ``tools/gen_golden_als.py`` (importing it installs them).  Every case stores its inputs and parameters, the
reference's ``weights_``, ``means_``, ``view_relevance_``, ``tau`` (from the ``b_tau`` it hands to its posterior draws),
``n_iter_``, ``n_components_``, the ``log_psi_*`` and ``alpha`` draws whole and the first rows of the ``z`` / ``W`` draws,
and held-out ``transform`` / ``score`` / ``log_likelihood``, in ``tests/golden/gfa_<case>.npz``.  The iterations of the
prunes come from the float64 restatement of ``tests/test_gfa_host.py`` (the reference does not record them), which must
first agree with the reference on the counts and to 1e-10 on the weights.  Three rules reject a case, all on that trace:

* drop margin: an iteration in which a column's ``mean(z^2)`` lies within a relative 1e-6 of ``1e-7``;
* stop margin: a ``rel_change`` within a relative 1e-6 of ``tol``;
* cancellation: ``y_const / (2 b_tau)`` above 100 in any iteration (the tau update would cancel more than two digits).

    python tools/gen_golden_gfa.py
"""

from __future__ import annotations

import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_als as base  # noqa: E402  (the shims, ``views``, ``Reject``, ``OUT``)

from cca_zoo.probabilistic._gfa import GFA as RefGFA  # noqa: E402
from conftest import save_npz_parts  # noqa: E402
from test_gfa_host import col_err, restate  # noqa: E402

STORED_ROWS = 5      # rows of every z / W draw that a golden keeps

# name, params, dims, n, dtype, data options
CASES = [
    ("two_maxiter", dict(latent_dimensions=4, max_iter=200, num_posterior_samples=8, random_state=0), (7, 5), 60,
     np.float64, {}),
    ("three_wide_f32", dict(latent_dimensions=6, max_iter=300, num_posterior_samples=6, random_state=1), (40, 9, 6), 37,
     np.float32, {}),
    ("tolstop_k8", dict(latent_dimensions=8, num_posterior_samples=4, random_state=0), (12, 10), 200, np.float64, {}),
    ("nocenter", dict(latent_dimensions=3, center=False, max_iter=150, num_posterior_samples=8, random_state=2), (9, 6), 50,
     np.float64, {}),
    ("nodrop_f32", dict(latent_dimensions=3, drop_k=False, max_iter=120, num_posterior_samples=8, random_state=3), (8, 11), 45,
     np.float32, {}),
    ("k1", dict(latent_dimensions=1, max_iter=100, num_posterior_samples=8, random_state=4), (6, 9), 40, np.float64, {}),
    ("wide17", dict(latent_dimensions=17, max_iter=60, num_posterior_samples=3, random_state=5), (150, 130, 50), 48,
     np.float32, dict(latent=3)),
]


def fit_reference(params, train):
    est = RefGFA(**params)
    seen = {}
    orig = est._draw_posterior_samples

    def draw(rng, z, cov_z, w, cov_w, a_ard, b_ard, a_tau, b_tau, d):
        seen["tau"] = np.asarray(a_tau) / np.asarray(b_tau)
        return orig(rng, z, cov_z, w, cov_w, a_ard, b_ard, a_tau, b_tau, d)

    est._draw_posterior_samples = draw
    est.fit(train)
    del est._draw_posterior_samples
    return est, seen["tau"]


def check_rules(name, params, train, est):
    trace = []
    r = restate(train, trace=trace, **params)
    if r["n_iter"] != est.n_iter_ or r["n_components"] != est.n_components_:
        raise base.Reject(f"{name}: the restatement took {r['n_iter']} iterations / {r['n_components']} components, "
                          f"the reference {est.n_iter_} / {est.n_components_}")
    err = max(col_err(w, ref) for w, ref in zip(r["weights"], est.weights_))
    if err > 1e-10:
        raise base.Reject(f"{name}: the restatement's weights differ from the reference's by {err:.2e}")
    tol = float(params.get("tol", 1e-4))
    worst_ratio = 0.0
    for it, (z2, rc, ratio) in enumerate(trace, 1):
        if params.get("drop_k", True) and np.any(np.abs(z2 - 1e-7) <= 1e-6 * 1e-7):
            raise base.Reject(f"{name}: mean z^2 within 1e-6 of the drop level at iteration {it}")
        if rc is not None and abs(rc - tol) <= 1e-6 * tol:
            raise base.Reject(f"{name}: rel_change within 1e-6 of tol at iteration {it}")
        worst_ratio = max(worst_ratio, float(np.max(ratio)))
    if worst_ratio > 100.0:
        raise base.Reject(f"{name}: y_const / (2 b_tau) reaches {worst_ratio:.1f}")
    return r["prune_iterations"], worst_ratio


def save_case(name, params, est, tau, train, test, prunes, ratio):
    out = {f"X{i}": v for i, v in enumerate(train)}
    out.update({f"T{i}": v for i, v in enumerate(test)})
    out.update({f"W{i}": w for i, w in enumerate(est.weights_)})
    out.update({f"mean{i}": mu for i, mu in enumerate(est.means_)})
    out["view_relevance"] = np.asarray(est.view_relevance_)
    out["tau"] = tau
    out["n_iter"] = np.int64(est.n_iter_)
    out["n_components"] = np.int64(est.n_components_)
    out["prune_iterations"] = np.asarray(prunes, dtype=np.int64)
    for key, v in est.posterior_samples_.items():
        v = np.asarray(v)
        out[f"S_{key}"] = v[:, :STORED_ROWS] if key == "z" or key.startswith("W_") else v
    out["Zt"] = est.transform(test)[0]
    out["score_test"] = np.asarray(est.score(test))
    out["loglik_test"] = np.float64(est.log_likelihood(test))
    out["loglik_train"] = np.float64(est.log_likelihood(train))
    out["params"] = np.array(repr(sorted(params.items())))
    out["num_posterior_samples"] = np.int64(params["num_posterior_samples"])
    out["n_views"] = np.int64(len(train))
    files = save_npz_parts(os.path.join(base.OUT, f"gfa_{name}.npz"), out)
    assert files == [os.path.join(base.OUT, f"gfa_{name}.npz")], "a GFA golden must fit one file"
    print(f"{name}: n_iter={est.n_iter_} components={est.n_components_} prunes at {prunes} "
          f"max y_const/(2 b_tau)={ratio:.1f} bytes={os.path.getsize(files[0])}")


def run_case(name, params, dims, n, dtype, opts, seed_shift=0):
    data = base.views(sum(name.encode()) + 29 + 1000 * seed_shift, n + 30, dims, dtype=dtype, **opts)
    train = [v[:n] for v in data]
    test = [v[n:] for v in data]
    est, tau = fit_reference(params, train)
    prunes, ratio = check_rules(name, params, train, est)
    save_case(name, params, est, tau, train, test, prunes, ratio)


def main():
    for case in CASES:
        for shift in range(20):
            try:
                run_case(*case, seed_shift=shift)
                break
            except base.Reject as e:
                print("rejected:", e, "-- moving the data seed")
        else:
            raise SystemExit(f"{case[0]}: every data seed was rejected")


if __name__ == "__main__":
    main()
