"""Float64 NumPy restatement of SCCA_IPLS / ElasticCCA as ``csrc/als.hip`` runs them: implicit deflation, the Gram form of
the elastic-net solve with blocked cyclic coordinate descent, scikit-learn's stop rule.  It is the reference of the CPU and
GPU tests (``test_enet_host.py``, ``test_gpu_enet.py``) and of ``tools/gen_golden_enet.py``, which compares it with the real
reference (``cca_zoo/linear/_iterative.py:522-623``, ``:730-831``, ``:938-982``) on every golden.

The blocked sweep visits the coordinates in index order and applies the same updates as one coordinate at a time; only
the residual outside the running block is brought up to date per block instead of per coordinate.
"""

from __future__ import annotations

import numpy as np

BW = 64        # coordinates per block (ENET_BW)
CAP = 1000     # CD sweeps per solve (scikit-learn's max_iter)

#: every golden, by class of the numeric bar: tol <= 1e-10, the default tol, float32 views
CASES = {
    "tight": ["ipls2_tight", "en2_tight", "ipls_lasso_tall", "ipls_perview_ridge", "en_perview", "ipls_nocenter"],
    "default": ["ipls2", "en2", "ipls3", "en3", "ipls_wide", "en_maxiter"],
    "f32": ["ipls_f32", "en_f32"],
}
ALL_CASES = [c for cs in CASES.values() for c in cs]


def case_class(case):
    return next(k for k, v in CASES.items() if case in v)


def soft(z, a):
    return np.sign(z) * max(abs(z) - a, 0.0)


def cd_sweep(G, r, c, a, b):
    """One blocked cyclic sweep in place on (r, c); returns (max |delta|, max |c|, per-block max |delta|)."""
    p = len(c)
    dmax, blocks = 0.0, []
    for j0 in range(0, p, BW):
        j1 = min(p, j0 + BW)
        T = G[j0:j1, j0:j1]
        rb, cb = r[j0:j1].copy(), c[j0:j1].copy()
        dl = np.zeros(j1 - j0)
        for j in range(j1 - j0):
            g = T[j, j]
            if g == 0.0:
                continue
            new = soft(rb[j] + g * cb[j], a) / (g + b)
            d = new - cb[j]
            if d != 0.0:
                rb -= d * T[j]
                cb[j] = new
                dl[j] = d
        if np.any(dl != 0.0):
            r -= G[j0:j1].T @ dl
        r[j0:j1] = rb
        c[j0:j1] = cb
        blocks.append(float(np.abs(dl).max()))
        dmax = max(dmax, blocks[-1])
    return dmax, float(np.abs(c).max()), blocks


def duality_gap(q, r, c, tt, a, b):
    """scikit-learn's duality gap of the elastic net in Gram form (R'R = t't - c'q - c'r, R't = t't - c'q, X'R = r)."""
    cq, cr = float(c @ q), float(c @ r)
    rr, rt = tt - cq - cr, tt - cq
    dual = float(np.abs(r - b * c).max())
    if dual > a:
        cst = a / dual
        gap = 0.5 * (rr + rr * cst * cst)
    else:
        cst, gap = 1.0, rr
    return gap + a * float(np.abs(c).sum()) - cst * rt + 0.5 * b * (1.0 + cst * cst) * float(c @ c)


def enet_solve(G, q, tt, c0, a, b, ridge, tol):
    """The solve from coefficients ``c0``: (c, r, CD sweeps, capped, last gap)."""
    c = np.array(c0, dtype=np.float64)
    r = q - G @ c
    gap = np.nan
    for sweep in range(1, CAP + 1):
        dmax, cmax, _ = cd_sweep(G, r, c, a, b)
        crit = cmax == 0.0 or dmax / cmax < tol
        cap = sweep >= CAP
        if ridge:
            if crit or cap:
                return c, r, sweep, not crit, gap
        elif crit or cap:
            gap = duality_gap(q, r, c, tt, a, b)
            if gap < tol * tt or cap:
                return c, r, sweep, not gap < tol * tt, gap
    raise AssertionError("unreachable")


def initial_vectors(random_state, p, k):
    rng = np.random.default_rng(random_state)
    out = []
    for _ in range(k):
        w = [rng.standard_normal(pi) for pi in p]
        out.append([x / np.linalg.norm(x) for x in w])
    return out


def restate(views, model, latent_dimensions, alpha, l1_ratio, center=True, max_iter=500, tol=1e-6, random_state=None):
    """``model``: "SCCA_IPLS" or "ElasticCCA"; ``alpha`` / ``l1_ratio``: one number per view.
    Returns (weights, sweeps per dimension, CD sweeps per dimension, capped solves)."""
    m, n, k = len(views), views[0].shape[0], int(latent_dimensions)
    X = [np.asarray(v - v.mean(axis=0) if center else v).astype(np.float64) for v in views]
    p = [x.shape[1] for x in X]
    ridge = [l == 0.0 for l in l1_ratio]
    a = [0.0 if rg else n * al * l for al, l, rg in zip(alpha, l1_ratio, ridge)]
    b = [al if rg else n * al * (1.0 - l) for al, l, rg in zip(alpha, l1_ratio, ridge)]
    G = [x.T @ x for x in X]
    Q = [np.zeros((n, 0)) for _ in X]
    W = [np.zeros((pi, k)) for pi in p]
    w0 = initial_vectors(random_state, p, k)
    iters, inner, capped = [], [], 0

    def score(j, w):
        s = X[j] @ w[j]
        return s - Q[j] @ (Q[j].T @ s)

    for d in range(k):
        w = [x.copy() for x in w0[d]]
        coef = [np.zeros(pi) for pi in p]
        s = [score(j, w) for j in range(m)]
        inner.append(0)
        for it in range(int(max_iter)):
            prev = [x.copy() for x in w]
            for i in range(m):
                t = sum(s[j] for j in range(m) if model == "ElasticCCA" or j != i)
                t = np.zeros(n) if np.isscalar(t) else t
                nt = np.linalg.norm(t)
                if nt > 1e-12:
                    t = t / nt
                tt = float(t @ t)
                q = X[i].T @ (t - Q[i] @ (Q[i].T @ t))
                c, _, sweeps, cap, _ = enet_solve(G[i], q, tt, coef[i], a[i], b[i], ridge[i], tol)
                coef[i] = c
                inner[-1] += sweeps
                capped += int(cap)
                w[i] = c.copy()
                s[i] = score(i, w)
                if model == "SCCA_IPLS":
                    sd = s[i].std()
                    if sd > 1e-12:
                        w[i] = c / sd
                        s[i] = s[i] / sd
            delta = max(np.linalg.norm(w[i] - prev[i]) for i in range(m))
            if delta < tol:
                break
        iters.append(it + 1)
        for i in range(m):
            W[i][:, d] = w[i]
            ns = float(s[i] @ s[i])
            qn = s[i] / np.sqrt(ns) if ns > 1e-12 else np.zeros(n)
            Q[i] = np.column_stack([Q[i], qn])
            ad = X[i].T @ qn
            G[i] = G[i] - np.outer(ad, ad)
    return W, iters, inner, capped


def case_views(g):
    return [g[f"X{i}"] for i in range(int(g["n_views"]))]


def case_params(g):
    """The constructor arguments of a golden (per-view lists)."""
    return dict(latent_dimensions=int(g["latent_dimensions"]), center=bool(g["center"]),
                alpha=[float(x) for x in g["alpha"]], l1_ratio=[float(x) for x in g["l1_ratio"]],
                max_iter=int(g["max_iter"]), tol=float(g["tol"]), random_state=int(g["random_state"]))


def restate_case(g):
    return restate(case_views(g), str(g["model"]), **case_params(g))


def col_err(w, ref):
    """Largest per-column relative error (the update map has no sign freedom)."""
    w, ref = np.asarray(w, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.linalg.norm(w - ref, axis=0) / np.maximum(np.linalg.norm(ref, axis=0), 1e-300)).max())
