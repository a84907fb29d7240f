#!/usr/bin/env python3
"""Golden vectors for ``CCAR3`` (cca_zoo/linear/_ccar3.py), captured from the REAL reference in the build container ->
tests/golden/ccar3_<tag>.npz.  Same metadata shim as tools/gen_golden.py; the reference source never travels.

Per case: the views, the parameters, the reference's ``weights_`` and ``score`` on the training views, ``B`` from the
reference's own ``_admm_row_sparse_rrr`` (its ``np.linalg.solve`` lines for ``highdim=False``), ``Sy`` as the reference forms
it, ``n_iter`` and the residuals of the last two iterations.  The reference returns neither of the last two, so:

- ``n_iter`` is the restatement's count (tests/ccar3_restatement.py), PROVED on the reference: its ADMM called with
  ``max_iter = n_iter`` returns the very array that the case's own ``max_iter`` returns, and with ``max_iter = n_iter - 1``
  a different one (``allzero``: B is zero at every iteration, so there the count is the restatement's alone)
- ``res_last2`` are the restatement's (primal, dual) residuals of iterations ``n_iter - 1`` and ``n_iter``

Float32 cases store float32 views; the reference runs on their float64 cast (what is stored) and on the float32 arrays
themselves, and ``gap32`` is the per-column gap (per view, one sign per column for both views) of the second to the first.

Admission checks; a draw that fails any of them gets the next seed (the seed that passed is stored and printed):

1. the stopping residual and the one before it each differ from ``tol`` by more than 0.1 % of ``tol``
2. at the final iterate every row norm of ``B + U`` differs from ``lambda_ / rho`` by more than 1e-6 relative
3. no eigenvalue of ``Sy`` within 1e-6 relative of the 1e-4 cut
4. the leading ``r_eff + 1`` singular values of ``B`` have relative gaps >= 1e-3 (the Cholesky whitening is not
   rotation-invariant: per-column parity needs separated singular values)
5. both Cholesky factorisations succeed
and the restatement agrees with the reference within 1e-10 per column (float64), with identical zero rows of ``B``.

    python tools/gen_golden_ccar3.py
"""
import importlib.metadata as md
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
REF = "/root/reference"
if not os.path.isdir(REF):
    sys.exit("reference not mounted; goldens can only be regenerated in the build container")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ccar3_restatement as R  # noqa: E402
from conftest import save_npz_parts  # noqa: E402

sys.path.insert(0, REF)
_orig_version = md.version
md.version = lambda name: "0.0.0+oracle" if name == "cca_zoo" else _orig_version(name)
_tl = types.ModuleType("tensorly")          # cca_zoo.linear imports TCCA, which imports tensorly; nothing here calls it
_tl.set_backend = lambda *a, **k: None
_dec = types.ModuleType("tensorly.decomposition")
_dec.parafac = None
_tl.decomposition = _dec
sys.modules["tensorly"] = _tl
sys.modules["tensorly.decomposition"] = _dec

from sklearn.covariance import LedoitWolf  # noqa: E402

from cca_zoo.linear import _ccar3 as ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
PARAMS = ("latent_dimensions", "center", "lambda_", "highdim", "ledoit_wolf", "rho", "max_iter", "tol", "eps")
DEFAULTS = dict(latent_dimensions=1, center=True, lambda_=0.0, highdim=True, ledoit_wolf=True, rho=1.0, max_iter=10_000, tol=1e-4,
                eps=1e-8)

#: tag -> shape (n, p, q), the constructor's arguments, and how the views are drawn: "latents" shared latent variables
#: of scales linspace(2, 0.7, latents), "signal" = the number of leading X features that carry them (all by default),
#: "noise"; "iters" = (least, most) iterations the case is there for
CASES = {
    "lowdim": dict(shape=(200, 24, 10), latent_dimensions=3, highdim=False),
    "dense": dict(shape=(300, 40, 12), latent_dimensions=3, lambda_=0.0),
    "sparse": dict(shape=(300, 40, 12), latent_dimensions=3, lambda_=0.1, signal=6, zero_rows=(5, 39)),
    "p_gt_n": dict(shape=(60, 150, 9), latent_dimensions=2, lambda_=0.15, signal=8, zero_rows=(30, 120)),
    "nolw_nocenter": dict(shape=(257, 33, 7), latent_dimensions=2, lambda_=0.05, ledoit_wolf=False, center=False, signal=9),
    "lw_nocenter": dict(shape=(150, 20, 6), latent_dimensions=2, lambda_=0.05, center=False, signal=8),
    "tight": dict(shape=(200, 30, 8), latent_dimensions=2, lambda_=0.05, tol=1e-8, rho=2.0, signal=8, iters=(33, 200)),
    "allzero": dict(shape=(100, 20, 5), latent_dimensions=2, lambda_=50.0, iters=(100, 2000), zero_rows=(20, 20)),
    "k_gt_q": dict(shape=(120, 30, 3), latent_dimensions=5, lambda_=0.05, signal=8),
    "q1": dict(shape=(150, 25, 1), latent_dimensions=1, lambda_=0.05, signal=6),
    "wide_q": dict(shape=(300, 90, 70), latent_dimensions=3, lambda_=0.05, latents=4, signal=12),
    "rows517": dict(shape=(200, 517, 12), latent_dimensions=2, lambda_=0.1, signal=10, zero_rows=(100, 510)),
    "maxiter": dict(shape=(200, 30, 8), latent_dimensions=2, lambda_=0.05, max_iter=5, signal=8),
    "rankdef_y": dict(shape=(200, 30, 6), latent_dimensions=2, lambda_=0.05, ledoit_wolf=False, signal=8, dup_y=True),
    "f32": dict(shape=(300, 40, 12), latent_dimensions=3, lambda_=0.1, signal=6, dtype=np.float32),
    "f32_p_gt_n": dict(shape=(60, 150, 9), latent_dimensions=2, lambda_=0.15, signal=8, dtype=np.float32),
}


def params_of(spec):
    return {k: spec.get(k, DEFAULTS[k]) for k in PARAMS}


def draw(spec, seed):
    rng = np.random.default_rng(seed)
    n, p, q = spec["shape"]
    k = spec.get("latents", 3)
    lat = rng.standard_normal((n, k)) * np.linspace(2.0, 0.7, k)
    wx, wy = rng.standard_normal((k, p)), rng.standard_normal((k, q))
    wx[:, spec.get("signal", p):] = 0.0
    noise = spec.get("noise", 1.0)
    X = lat @ wx + noise * rng.standard_normal((n, p)) + rng.choice([-1.0, 1.0], p) * rng.uniform(2.0, 3.0, p)
    Y = lat @ wy + noise * rng.standard_normal((n, q)) + rng.choice([-1.0, 1.0], q) * rng.uniform(2.0, 3.0, q)
    if spec.get("dup_y"):
        Y[:, -1] = Y[:, 0]
    dt = spec.get("dtype", np.float64)
    return [X.astype(dt), Y.astype(dt)]


def reference_parts(par, views):
    """Sy, B and the ADMM's own inputs as the reference's ``fit`` forms them (its own functions, line by line)."""
    model = ref.CCAR3(**par)
    X, Y = model._setup_fit([v.copy() for v in views])
    n = X.shape[0]
    Sy = LedoitWolf().fit(Y).covariance_ if par["ledoit_wolf"] else Y.T @ Y / n
    root = ref._sqrt_inv_psd(Sy)
    Yt = Y @ root
    if par["highdim"]:
        def admm(max_iter):
            return ref._admm_row_sparse_rrr(X, Yt, lambda_=par["lambda_"], rho=par["rho"], max_iter=max_iter, tol=par["tol"],
                                            ridge=par["eps"])
        return Sy, admm(par["max_iter"]), admm
    return Sy, np.linalg.solve(X.T @ X / n + par["eps"] * np.eye(X.shape[1]), X.T @ Yt / n), None


def admit(spec, par, rs, B_ref, admm):
    """The admission checks on the restatement's figures; returns (ok, figures)."""
    fig = {"n_iter": rs["n_iter"]}
    ok = True
    if par["highdim"]:
        res = rs["res"].max(axis=1)[-2:]
        fig["margin"] = float(np.min(np.abs(res - par["tol"])) / par["tol"])
        thr = par["lambda_"] / par["rho"]
        fig["row_margin"] = float(np.min(np.abs(rs["norms"] - thr) / thr)) if thr > 0 else np.inf
        ok = fig["margin"] > 1e-3 and fig["row_margin"] > 1e-6
        # n_iter, proved on the reference itself
        it = rs["n_iter"]
        # (an all-zero B is zero at every iteration and proves nothing: there the count is the restatement's alone)
        ok = ok and np.array_equal(admm(it), B_ref) and (it == 1 or not np.any(B_ref) or not np.array_equal(admm(it - 1), B_ref))
        lo, hi = spec.get("iters", (1, par["max_iter"]))
        ok = ok and lo <= it <= hi
    fig["cut_margin"] = float(np.min(np.abs(rs["lam"] - R.CUT) / R.CUT))
    ok = ok and fig["cut_margin"] > 1e-6
    r = min(par["latent_dimensions"], *B_ref.shape)
    s = rs["sv"][:r + 1]
    fig["sv_gap"] = float(np.min(-np.diff(s) / s[:-1])) if s.size > 1 else np.inf
    ok = ok and fig["sv_gap"] >= 1e-3 and rs["chol_ok"]
    zero = ~np.any(B_ref, axis=1)
    fig["zero_rows"] = int(zero.sum())
    lo, hi = spec.get("zero_rows", (0, B_ref.shape[0]))
    ok = ok and lo <= fig["zero_rows"] <= hi and np.array_equal(zero, ~np.any(rs["B"], axis=1))
    return bool(ok), fig


def main():
    os.makedirs(OUT, exist_ok=True)
    for row, (tag, spec) in enumerate(CASES.items()):
        par = params_of(spec)
        for attempt in range(200):
            seed = 7000 + 100 * row + attempt
            views = draw(spec, seed)
            v64 = [v.astype(np.float64) for v in views]
            model = ref.CCAR3(**par).fit([v.copy() for v in v64])
            Sy, B_ref, admm = reference_parts(par, v64)
            rs = R.fit(v64, **{("ledoit_wolf_" if k == "ledoit_wolf" else k): v for k, v in par.items()})
            ok, fig = admit(spec, par, rs, B_ref, admm)
            w_ref = [np.asarray(w, dtype=np.float64) for w in model.weights_]
            worst = max(float(R.col_gap(rs["weights"], w_ref).max()), float(np.abs(rs["Sy"] - Sy).max() / np.abs(Sy).max()),
                        float(np.linalg.norm(rs["B"] - B_ref) / max(np.linalg.norm(B_ref), 1e-300)))
            if ok and worst < 1e-10:
                break
        else:
            sys.exit(f"{tag}: no seed passed the admission checks (last figures {fig}, restatement {worst:.1e})")
        store = {"seed": np.int64(seed), "x0": views[0], "x1": views[1], "w0": w_ref[0], "w1": w_ref[1],
                 "score": np.asarray(model.score([v.copy() for v in v64]), dtype=np.float64), "B": np.asarray(B_ref, dtype=np.float64),
                 "Sy": np.asarray(Sy, dtype=np.float64), "n_iter": np.int64(rs["n_iter"]),
                 "res_last2": rs["res"][-2:].copy()}
        for k, v in par.items():
            store[f"param_{k}"] = np.asarray(v)
        note = ""
        if spec.get("dtype") is np.float32:
            m32 = ref.CCAR3(**par).fit([v.copy() for v in views])
            store["gap32"] = R.col_gap([np.asarray(w, dtype=np.float64) for w in m32.weights_], w_ref)
            store["score32"] = np.asarray(m32.score([v.copy() for v in views]), dtype=np.float64)
            note = f"  gap32 {store['gap32'].max():.1e}"
        path = os.path.join(OUT, f"ccar3_{tag}.npz")
        files = save_npz_parts(path, store)
        assert all(os.path.getsize(f) < (1 << 20) for f in files)
        print(f"ccar3_{tag}: seed {seed}  " + "  ".join(f"{k} {v:.3g}" for k, v in fig.items())
              + f"  restatement {worst:.1e}{note}  {sum(os.path.getsize(f) for f in files)} bytes")


if __name__ == "__main__":
    main()
