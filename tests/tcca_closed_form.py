"""NumPy closed form of the tensor CCA loss and its input gradients (float64) -- the specification that
``cca_zoo_amd.deep.TCCALoss`` implements, checked against the reference's autograd in the ``tcca_*`` goldens.

Per view: ``Z_c = Z - mean``, ``S = Z_c'Z_c / (n - 1) + eps I = V diag(lam) V'``, ``f = max(lam, eps)^-1/2``,
``F = V diag(f) V'``, ``H = Z_c F``.  ``M = (1 / n) sum_s H_1[s] (x) .. (x) H_V[s]`` is a Khatri-Rao product times a matrix,
the loss is ``-||M||_F``.  Backward: ``T = -M / ||M||``; ``GH_j = (1 / n) T_(j) (Khatri-Rao of the other views)``;
``dF = Z_c' GH_j``; ``dS = V ((V' sym(dF) V) o K) V'`` with the Daleckii-Krein matrix ``K_ab = (f_a - f_b) / (lam_a - lam_b)``
(``f'`` on the diagonal and between equal eigenvalues, 0 where the clamp is active); ``dZ_c = GH_j F + 2 Z_c dS / (n - 1)``,
column-centred.
"""

import numpy as np

CASES = ("three", "two", "four", "three17", "odd", "one_col", "wide_last", "tall")


def kr_rows(mats):
    """Row-wise Khatri-Rao product: (n, prod d_i), the last matrix's index fastest."""
    out = mats[0]
    for m in mats[1:]:
        out = (out[:, :, None] * m[:, None, :]).reshape(out.shape[0], -1)
    return out


def dk_matrix(lam, f, eps):
    fp = np.where(lam > eps, -0.5 * f ** 3, 0.0)
    dl = lam[:, None] - lam[None, :]
    close = np.abs(dl) <= 1e-12 * max(np.abs(lam).max(), 1e-300)
    return np.where(close, 0.5 * (fp[:, None] + fp[None, :]), (f[:, None] - f[None, :]) / np.where(close, 1.0, dl))


def tcca_loss_closed_form(views, eps):
    """(loss, [dloss/dZ_i]) in float64."""
    zs = [np.asarray(z, dtype=np.float64) for z in views]
    n = zs[0].shape[0]
    zc, lam, vec, f, F, H = [], [], [], [], [], []
    for z in zs:
        c = z - z.mean(axis=0)
        S = c.T @ c / (n - 1) + eps * np.eye(z.shape[1])
        w, V = np.linalg.eigh(S)
        fi = 1.0 / np.sqrt(np.maximum(w, eps))
        Fi = (V * fi) @ V.T
        zc.append(c), lam.append(w), vec.append(V), f.append(fi), F.append(Fi), H.append(c @ Fi)
    dims = [h.shape[1] for h in H]
    M = (kr_rows(H[:-1]).T @ H[-1] / n).reshape(dims)
    norm = np.sqrt(np.sum(M * M))
    T = -M / norm if norm > 0 else np.zeros_like(M)
    grads = []
    for j in range(len(H)):
        others = [H[i] for i in range(len(H)) if i != j]
        Tj = np.moveaxis(T, j, -1).reshape(-1, dims[j])
        GH = kr_rows(others) @ Tj / n
        dF = zc[j].T @ GH
        V = vec[j]
        dS = V @ ((V.T @ (0.5 * (dF + dF.T)) @ V) * dk_matrix(lam[j], f[j], eps)) @ V.T
        g = GH @ F[j] + zc[j] @ (2.0 / (n - 1) * dS)
        grads.append(g - g.mean(axis=0))
    return -norm, grads
