"""NumPy restatement of CCAR3 (cca_zoo/linear/_ccar3.py) in moment form: what ``cca_zoo_amd.linear.CCAR3`` and
``csrc/rrr.hip`` are held to.  Written in this project's own words, not copied from the reference.

Everything except one scalar is a function of the second moments of ``[X Y]``:

- ``Sxx, Sxy, Syy = X'X/n, X'Y/n, Y'Y/n`` (division by n; the views centred when ``center``)
- Ledoit-Wolf (sklearn's ``LedoitWolf().fit(Y)``, which always centres): ``C = Yc'Yc/n``, ``mu = tr(C)/q``,
  ``delta_ = sum C^2``, ``beta_ = (1/n) sum_i |y_i - ybar|^4`` (the one quantity the moments do not hold),
  ``beta = (beta_ - delta_)/(q n)``, ``delta = (delta_ - 2 mu tr(C) + q mu^2)/q``, ``shrinkage = min(beta, delta)/delta``
  (0 when ``beta == 0``), ``Sy = (1 - shrinkage) C + shrinkage mu I``
- ``R = Sy^-1/2`` with the eigenvalues <= 1e-4 set to zero, ``P = Sxy R``
- ``highdim=False``: ``B = (Sxx + eps I)^-1 P``.  ``highdim=True``: ADMM from ``Z = U = 0`` with the explicit inverse
  ``M = (Sxx + (rho + eps) I)^-1`` (the reference solves with the Cholesky factor every iteration; the matrix's condition
  number is at most ``(lambda_max + rho)/rho``)
- the SVD of B, the two Cholesky whitenings from ``U0' Sxx U0`` and ``V0' Syy V0``, signs, order, padding
"""

import numpy as np

CUT = 1e-4            # eigenvalues of Sy up to this are zeroed in R


def moments(X, Y, center=True):
    """n, the column means (zeros without centring), Sxx, Sxy, Syy of the (centred) views, the always-centred covariance of
    Y and ``sum_i |y_i - ybar|^4``; everything in float64."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    n = X.shape[0]
    mx, my = X.mean(axis=0), Y.mean(axis=0)
    Yc = Y - my
    if center:
        X, Y = X - mx, Yc
    else:
        mx, my = np.zeros(X.shape[1]), np.zeros(Y.shape[1])
    return dict(n=n, means=[mx, my], Sxx=X.T @ X / n, Sxy=X.T @ Y / n, Syy=Y.T @ Y / n, C=Yc.T @ Yc / n,
                fourth=float(np.sum(np.sum(Yc * Yc, axis=1) ** 2)))


def ledoit_wolf(C, fourth, n):
    """(Sy, shrinkage) from the centred covariance C (division by n) and ``fourth = sum_i |y_i - ybar|^4``."""
    q = C.shape[0]
    tr = np.trace(C)
    mu = tr / q
    delta_ = np.sum(C * C)
    beta_ = fourth / n
    beta = (beta_ - delta_) / (q * n)
    delta = (delta_ - 2.0 * mu * tr + q * mu * mu) / q
    beta = min(beta, delta)
    shrinkage = 0.0 if beta == 0 else beta / delta
    Sy = (1.0 - shrinkage) * C
    Sy[np.diag_indices(q)] += shrinkage * mu
    return Sy, float(shrinkage)


def inv_sqrt_cut(Sy):
    """(R, eigenvalues): ``R = V diag(lam^-1/2 where lam > CUT, else 0) V'``."""
    lam, V = np.linalg.eigh(0.5 * (Sy + Sy.T))
    f = np.zeros_like(lam)
    keep = lam > CUT
    f[keep] = 1.0 / np.sqrt(lam[keep])
    return (V * f) @ V.T, lam


def admm_loop(M, P, lambda_, rho, tol, max_iter):
    """The ADMM iterations on ``M = (Sxx + (rho + eps) I)^-1`` and ``P``.  Returns Z (exact zero rows), the iteration
    count, the (primal, dual) residuals of every iteration and the row norms of ``B + U`` at the last one."""
    p = P.shape[0]
    Z, U = np.zeros_like(P), np.zeros_like(P)
    thr = lambda_ / rho
    res, norms = [], np.zeros(p)
    for _ in range(int(max_iter)):
        B = M @ (P + rho * (Z - U))
        Z_old = Z
        T = B + U
        norms = np.sqrt(np.sum(T * T, axis=1))
        scale = np.zeros(p)
        nz = norms > 0
        scale[nz] = np.maximum(0.0, 1.0 - thr / norms[nz])
        Z = T * scale[:, None]
        U = T - Z
        res.append((np.sqrt(np.sum((Z - B) ** 2)) / np.sqrt(p), np.sqrt(np.sum((Z_old - Z) ** 2)) / np.sqrt(p)))
        if max(res[-1]) < tol:
            break
    return Z, len(res), np.array(res).reshape(-1, 2), norms


def whiten_factor(G, eps):
    """W with ``W' G W = I``: the inverse transposed Cholesky factor of ``sym(G) + eps I``; when that fails, the symmetric
    inverse square root with the eigenvalues raised to eps.  Returns (W, whether the Cholesky factorisation succeeded)."""
    G = 0.5 * (G + G.T) + eps * np.eye(G.shape[0])
    try:
        return np.linalg.inv(np.linalg.cholesky(G)).T, True
    except np.linalg.LinAlgError:
        lam, V = np.linalg.eigh(G)
        return (V / np.sqrt(np.maximum(lam, eps))) @ V.T, False


def finish(U0, V0, Sxx, Sxy, Syy, k, eps, p, q):
    """The weights from the leading singular vectors U0 (p x r_eff) of B and ``V0 = R Vt[:r_eff]'``: whitening, sign,
    order, zero padding to k columns.  Returns (U, V, whether both Cholesky factorisations succeeded)."""
    Wx, okx = whiten_factor(U0.T @ Sxx @ U0, eps)
    Wy, oky = whiten_factor(V0.T @ Syy @ V0, eps)
    U, V = U0 @ Wx, V0 @ Wy
    cor = np.diag(U.T @ Sxy @ V).copy()
    neg = cor < 0
    V[:, neg] *= -1.0
    cor[neg] *= -1.0
    order = np.argsort(-cor)
    U, V = U[:, order], V[:, order]
    r = U.shape[1]
    if r < k:
        U, V = np.hstack([U, np.zeros((p, k - r))]), np.hstack([V, np.zeros((q, k - r))])
    return U, V, okx and oky


def postprocess(B, R, Sxx, Sxy, Syy, k, eps):
    p, q = B.shape
    if not np.any(B):
        return np.zeros((p, k)), np.zeros((q, k)), True, np.zeros(0)
    r = min(k, p, q)
    U0, s, Vt = np.linalg.svd(B, full_matrices=False)
    U, V, ok = finish(U0[:, :r], R @ Vt[:r].T, Sxx, Sxy, Syy, k, eps, p, q)
    return U, V, ok, s


def fit(views, latent_dimensions=1, center=True, lambda_=0.0, highdim=True, ledoit_wolf_=True, rho=1.0, max_iter=10_000,
        tol=1e-4, eps=1e-8):
    """The whole fit.  Returns a dict: weights, means, B, n_iter, res (per-iteration residuals), norms (row norms of B + U
    at the last iteration), Sy, shrinkage, lam (eigenvalues of Sy), sv (singular values of B), chol_ok, M, P."""
    X, Y = views
    m = moments(X, Y, center)
    p, q = m["Sxx"].shape[0], m["Syy"].shape[0]
    Sy, shrinkage = ledoit_wolf(m["C"], m["fourth"], m["n"]) if ledoit_wolf_ else (m["Syy"].copy(), 0.0)
    R, lam = inv_sqrt_cut(Sy)
    P = m["Sxy"] @ R
    out = dict(means=m["means"], Sy=Sy, shrinkage=shrinkage, lam=lam, P=P, R=R)
    if highdim:
        M = np.linalg.inv(m["Sxx"] + (rho + eps) * np.eye(p))
        M = 0.5 * (M + M.T)
        B, n_iter, res, norms = admm_loop(M, P, lambda_, rho, tol, max_iter)
        out.update(M=M, n_iter=n_iter, res=res, norms=norms)
    else:
        B = np.linalg.solve(m["Sxx"] + eps * np.eye(p), P)
        out.update(n_iter=0, res=np.zeros((0, 2)), norms=np.zeros(p))
    U, V, ok, sv = postprocess(B, R, m["Sxx"], m["Sxy"], m["Syy"], int(latent_dimensions), eps)
    out.update(B=B, weights=[U, V], chol_ok=ok, sv=sv)
    return out


def col_gap(got, ref):
    """Per-column ``|s got - ref| / |ref|`` of BOTH views with ONE sign s per column (the SVD fixes the pair of singular
    vectors only up to a common sign); a zero reference column asks for a zero column.  ``got``, ``ref``: [U, V]."""
    s = np.sign(sum(np.sum(a * b, axis=0) for a, b in zip(got, ref)))
    s[s == 0] = 1.0
    gaps = []
    for a, b in zip(got, ref):
        den = np.linalg.norm(b, axis=0)
        num = np.linalg.norm(a * s - b, axis=0)
        gaps.append(np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0)))
    return np.stack(gaps)
