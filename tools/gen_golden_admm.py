#!/usr/bin/env python3
"""Capture golden vectors of the reference's SCCA_ADMM (``cca_zoo/linear/_iterative.py:388-514``).

Built like ``tools/gen_golden_als.py`` (whose shims and data generator it imports): the reference runs in-process, every
case stores its inputs, the reference's ``weights_`` and ``means_``, held-out ``transform`` / ``score`` and the iterations
taken per latent dimension (``_target_score`` calls / views) in ``tests/golden/admm_<case>.npz``.  The reference's
``_fit_single`` is one loop, so the two rejection rules read the trajectory of the float64 restatement
(``tests/test_admm_host.py::restate``), which must first reproduce the reference's iteration counts and supports:

* stop margin: an iteration whose delta lies within 1 % of ``tol``;
* support: at a dimension's last iteration, an entry with ``||w' + eta| - tau / mu| / max|w' + eta| < 1e-9``, or a
  norm of the thresholded vector within 1e-9 of 1 (where the projection onto the unit ball switches on).

What the searches behind the cases found (``max_iter <= 200`` throughout):

* on data of ordinary scale the iterates end every iteration on the unit sphere and flip sign from one iteration to the
  next (delta = 2), so ``tol`` never stops a non-zero fit; ``collapse`` and ``half_collapse`` are the cases in which
  ``tol`` stops a dimension there (all weights, or one view's, become exactly zero);
* on data scaled down by 20 to 50 the projection is inactive at the end (``inactive_ball``: columns of norm 0.68 to
  0.98) and non-zero fits do reach a looser ``tol`` (``tolstop``: tol = 1e-4, the second dimension stops after 53
  iterations); at ``tol = 1e-6`` no non-zero fit stopped within 200 iterations.

The last line printed is the worst per-column error between the reference and the restatement over the float32 cases:
the reference multiplies ``X'X`` in float32 at the first dimension, the restatement (and the device) in float64.
``tests/test_admm_host.py::F32_MEASURED`` and DESIGN.md quote it.

    python tools/gen_golden_admm.py
"""

from __future__ import annotations

import os
import sys

import numpy as np

from gen_golden_als import OUT, Reject, ref_it, save_npz_parts, views  # noqa: E402  (also sets the import shims up)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from test_admm_host import restate  # noqa: E402
from test_als_host import col_err  # noqa: E402


def fit_counted(params, train):
    """The reference's fit and its iterations per dimension: ``_target_score`` runs once per view and iteration."""
    est = ref_it.SCCA_ADMM(**params)
    counts = []
    orig_single, orig_target = est._fit_single, ref_it._target_score

    def single(vs, w, d):
        counts.append(0)
        return orig_single(vs, w, d)

    def target(vs, ws, i):
        counts[-1] += 1
        return orig_target(vs, ws, i)

    est._fit_single, ref_it._target_score = single, target
    try:
        with np.errstate(all="ignore"):
            est.fit(train)
    finally:
        ref_it._target_score = orig_target
        del est._fit_single
    assert all(c % len(train) == 0 for c in counts)
    return est, [c // len(train) for c in counts]


def check_rules(name, params, est, iters, train):
    trace = []
    W, its, deltas = restate(train, trace=trace, **params)
    if its != iters:
        raise Reject(f"{name}: the restatement takes {its} iterations, the reference {iters}")
    for w, r in zip(W, est.weights_):
        if not np.array_equal(w != 0, r != 0):
            raise Reject(f"{name}: the restatement's support differs from the reference's")
    tol = float(params.get("tol", 1e-6))
    for rec in trace:
        for d in rec["deltas"]:
            if tol > 0 and np.isfinite(d) and abs(d - tol) < 0.01 * tol:
                raise Reject(f"{name}: a stop margin {d} is within 1% of tol {tol}")
        for i, u in enumerate(rec["last"]):
            a = np.abs(u["v"])
            if a.max() > 0 and np.min(np.abs(a - u["thr"])) / a.max() < 1e-9:
                raise Reject(f"{name}: an entry lies within 1e-9 of the threshold at the last iteration of view {i}")
            if abs(u["znorm"] - 1.0) < 1e-9:
                raise Reject(f"{name}: the thresholded vector of view {i} has norm within 1e-9 of 1")
    return max(col_err(w, r) for w, r in zip(W, est.weights_)), deltas


def save_case(name, params, est, train, test, iters, deltas):
    out = {f"X{i}": v for i, v in enumerate(train)}
    out.update({f"T{i}": v for i, v in enumerate(test)})
    out.update({f"W{i}": w for i, w in enumerate(est.weights_)})
    out.update({f"mean{i}": mu for i, mu in enumerate(est.means_)})
    out.update({f"Zt{i}": z for i, z in enumerate(est.transform(test))})
    out["score_test"] = np.asarray(est.score(test))
    out["n_iter"] = np.asarray(iters, dtype=np.int64)
    out["model"] = np.array("SCCA_ADMM")
    out["params"] = np.array(repr(sorted(params.items())))
    out["n_views"] = np.int64(len(train))
    files = save_npz_parts(os.path.join(OUT, f"admm_{name}.npz"), out)
    assert files == [os.path.join(OUT, f"admm_{name}.npz")], "an ADMM golden must fit one file"
    nnz = [[int(np.count_nonzero(w[:, d])) for d in range(w.shape[1])] for w in est.weights_]
    nrm = [[round(float(np.linalg.norm(w[:, d])), 4) for d in range(w.shape[1])] for w in est.weights_]
    print(f"{name}: iterations={iters} last delta={[f'{d:.2e}' for d in deltas]} support sizes={nnz} norms={nrm} "
          f"bytes={os.path.getsize(files[0])}")


# name, params, dims, n, dtype, data options
CASES = [
    ("tall2", dict(latent_dimensions=2, tau=1.0, mu=1.0, max_iter=100, random_state=1), (10, 8), 60, np.float64, {}),
    ("wide2", dict(latent_dimensions=2, tau=1.0, mu=10.0, max_iter=100, random_state=2), (300, 200), 40, np.float64, {}),
    ("three", dict(latent_dimensions=2, tau=1.0, mu=2.0, max_iter=100, random_state=3), (12, 9, 7), 50, np.float64,
     dict(latent=3)),
    ("nocenter", dict(latent_dimensions=2, center=False, tau=1.0, mu=1.0, max_iter=100, random_state=4), (10, 8), 60,
     np.float64, {}),
    ("perview", dict(latent_dimensions=2, tau=[0.5, 1.5], mu=2.0, max_iter=100, random_state=5), (14, 9), 60, np.float64, {}),
    ("tall_f32", dict(latent_dimensions=2, tau=1.0, mu=1.0, max_iter=100, random_state=6), (11, 6), 70, np.float32, {}),
    ("wide_f32", dict(latent_dimensions=2, tau=1.0, mu=10.0, max_iter=100, random_state=7), (300, 200), 40, np.float32, {}),
    ("collapse", dict(latent_dimensions=2, tau=1.0, mu=1.0, max_iter=100, random_state=8), (300, 200), 40, np.float64, {}),
    ("half_collapse", dict(latent_dimensions=2, tau=2.0, mu=5.0, max_iter=100, random_state=9), (300, 200), 40, np.float64, {}),
    ("inactive_ball", dict(latent_dimensions=2, tau=0.2, mu=5.0, max_iter=150, tol=1e-4, random_state=10), (10, 8), 60,
     np.float64, dict(scale=0.05)),
    ("tolstop", dict(latent_dimensions=2, tau=0.01, mu=1.0, max_iter=150, tol=1e-4, random_state=10), (10, 8), 60,
     np.float64, dict(scale=0.02)),
]


def run_case(name, params, dims, n, dtype, opts, seed_shift=0):
    data = views(sum(name.encode()) + 29 + 1000 * seed_shift, n + 30, dims, dtype=dtype, **opts)
    train = [v[:n] for v in data]
    test = [v[n:] for v in data]
    est, iters = fit_counted(params, train)
    err, deltas = check_rules(name, params, est, iters, train)
    save_case(name, params, est, train, test, iters, deltas)
    return err


def main():
    worst = {np.float32: 0.0, np.float64: 0.0}
    for case in CASES:
        for shift in range(20):
            try:
                err = run_case(*case, seed_shift=shift)
                worst[case[4]] = max(worst[case[4]], err)
                break
            except Reject as e:
                print("rejected:", e, "-- moving the data seed")
        else:
            raise SystemExit(f"{case[0]}: every data seed was rejected")
    print(f"float64 cases: worst reference-to-restatement column error {worst[np.float64]:.2e}")
    print(f"float32 cases: worst reference-to-restatement column error {worst[np.float32]:.2e}")


if __name__ == "__main__":
    main()
