"""NumPy closed forms (float64) of the four moment-map losses and their input gradients -- the specification that
``cca_zoo_amd.deep.EYLoss`` / ``BarlowTwinsLoss`` / ``VICRegLoss`` / ``SDLLoss`` implement, checked against the reference's
autograd in the ``ssl_*`` goldens (tools/gen_golden_ssl.py).

Notation: n rows, m views of common width d, ``Z = [z_1 .. z_m]``, mu the column mean, ``zc = Z - 1 mu'``,
``S_ab = zc_a' zc_b / (n - 1)``.  Every gradient is ``dZ = zc Gamma_c + Z Gamma_r`` with block ``(b, a)`` of a Gamma acting
from view b into the gradient of view a (DESIGN.md 4j lists them); the functions below return the terms and the gradients.

EY       ``V = mean_a S_aa``, ``C = (1 / m) sum_ab S_ab``; ``-2 tr C + tr(V V_ind)`` (``V_ind = V`` without an independent batch)
Barlow   ``C = z_1' z_2 / n`` (raw); ``sum_i (1 - C_ii)^2 + lam sum_{i != j} C_ij^2``
VICReg   ``sim_coeff mean((z_1 - z_2)^2) + std_coeff sum_a mean_j relu(1 - sqrt((S_aa)_jj + 1e-4)) + cov_coeff sum_a sum_{i != j} (S_aa)_ij^2 / d``
SDL      ``mean((z_1 - z_2)^2) + lam sum_a mean |offdiag S_aa|``
"""

import numpy as np

#: tag -> (kind, n, m, d, params, flavour[, n_ind]); flavours: "plain" (latent mix + 0.3 i offsets), "bn" (batch-normalised
#: columns), "offset" (column offsets of order 1), "cancel" (z_2 = z_1 + 1e-3 noise), "scaled" (column spreads on both sides of 1)
CASES = {
    "ey_small": ("ey", 64, 2, 4, (), "plain"),
    "ey_four17": ("ey", 96, 4, 17, (), "plain"),
    "ey_one_col": ("ey", 33, 2, 1, (), "plain"),
    "ey_three": ("ey", 80, 3, 5, (), "plain"),
    "ey_wide": ("ey", 150, 2, 70, (), "plain"),
    "ey_tall": ("ey", 4100, 2, 3, (), "plain"),
    "ey_ind": ("ey", 96, 2, 5, (), "plain", 80),
    "bt_small": ("barlow", 64, 2, 4, (5e-3,), "bn"),
    "bt_odd": ("barlow", 33, 2, 17, (5e-3,), "bn"),
    "bt_40": ("barlow", 120, 2, 40, (2e-2,), "bn"),
    "bt_wide": ("barlow", 150, 2, 70, (5e-3,), "bn"),
    "bt_offset": ("barlow", 96, 2, 17, (5e-3,), "offset"),
    "bt_tall": ("barlow", 4100, 2, 3, (5e-3,), "bn"),
    "vic_small": ("vicreg", 64, 2, 4, (25.0, 25.0, 1.0), "scaled"),
    "vic_one_col": ("vicreg", 33, 2, 1, (25.0, 25.0, 1.0), "scaled"),
    "vic_40": ("vicreg", 120, 2, 40, (10.0, 5.0, 2.0), "scaled"),
    "vic_wide": ("vicreg", 150, 2, 70, (25.0, 25.0, 1.0), "scaled"),
    "vic_cancel": ("vicreg", 96, 2, 8, (25.0, 25.0, 1.0), "cancel"),
    "vic_offset": ("vicreg", 80, 2, 17, (25.0, 25.0, 1.0), "offset"),
    "vic_tall": ("vicreg", 4100, 2, 3, (25.0, 25.0, 1.0), "scaled"),
    "sdl_small": ("sdl", 64, 2, 4, (0.5,), "plain"),
    "sdl_three": ("sdl", 80, 3, 5, (0.5,), "plain"),
    "sdl_four17": ("sdl", 96, 4, 17, (0.5,), "plain"),
    "sdl_odd": ("sdl", 33, 2, 6, (0.2,), "plain"),
    "sdl_40": ("sdl", 120, 2, 40, (0.5,), "plain"),
    "sdl_cancel": ("sdl", 96, 2, 8, (0.5,), "cancel"),
}

TERM_KEYS = {
    "ey": ("rewards", "penalties"),
    "barlow": ("invariance", "redundancy"),
    "vicreg": ("sim_loss", "var_loss", "cov_loss"),
    "sdl": ("l2", "sdl"),
}

VICREG_EPS = 1e-4


def _centred(views):
    zs = [np.asarray(z, dtype=np.float64) for z in views]
    return zs, [z - z.mean(axis=0) for z in zs]


def _ey_v(zc):
    n = zc[0].shape[0]
    return sum(c.T @ c for c in zc) / ((n - 1) * len(zc))


def ey(views, independent=None):
    """``(terms, grads, grads_independent)``; ``grads_independent`` is None without an independent batch."""
    zs, zc = _centred(views)
    n, m = zs[0].shape[0], len(zs)
    V = _ey_v(zc)
    total = sum(zc)
    rewards = 2.0 * np.sum(total * total) / (m * (n - 1))
    gi = None
    if independent is None:
        Vo, coef = V, 4.0
    else:
        _, ic = _centred(independent)
        Vo, coef = _ey_v(ic), 2.0
        gi = [c @ (2.0 * V) / (len(ic) * (ic[0].shape[0] - 1)) for c in ic]
    penalties = float(np.sum(V * Vo))
    grads = [(-4.0 * total + coef * c @ Vo) / (m * (n - 1)) for c in zc]
    return {"objective": -rewards + penalties, "rewards": rewards, "penalties": penalties}, grads, gi


def barlow(views, lam):
    zs, _ = _centred(views)
    if len(zs) != 2:
        raise ValueError("exactly 2 views")
    n = zs[0].shape[0]
    C = zs[0].T @ zs[1] / n
    dg = np.diag(C)
    invariance = float(np.sum((1.0 - dg) ** 2))
    redundancy = float(np.sum(C * C) - np.sum(dg * dg))
    E = 2.0 * lam * C
    E[np.diag_indices_from(E)] = -2.0 * (1.0 - dg)
    grads = [zs[1] @ E.T / n, zs[0] @ E / n]
    return {"objective": invariance + lam * redundancy, "invariance": invariance, "redundancy": redundancy}, grads, None


def _offdiag(S):
    return S - np.diag(np.diag(S))


def vicreg(views, sim_coeff, std_coeff, cov_coeff):
    zs, zc = _centred(views)
    if len(zs) != 2:
        raise ValueError("exactly 2 views")
    n, d = zs[0].shape
    diff = zs[0] - zs[1]
    sim = float(np.mean(diff * diff))
    var = cov = 0.0
    grads = []
    for a, c in enumerate(zc):
        S = c.T @ c / (n - 1)
        sig = np.sqrt(np.diag(S) + VICREG_EPS)
        var += float(np.mean(np.maximum(1.0 - sig, 0.0)))
        off = _offdiag(S)
        cov += float(np.sum(off * off) / d)
        gam = (cov_coeff * 4.0 * off / d - std_coeff * np.diag((sig < 1.0) / (sig * d))) / (n - 1)
        grads.append(c @ gam + (1.0 if a == 0 else -1.0) * sim_coeff * 2.0 * diff / (n * d))
    obj = sim_coeff * sim + std_coeff * var + cov_coeff * cov
    return {"objective": obj, "sim_loss": sim, "var_loss": var, "cov_loss": cov}, grads, None


def sdl(views, lam):
    zs, zc = _centred(views)
    n, d = zs[0].shape
    if d < 2:
        raise ValueError("d >= 2")
    diff = zs[0] - zs[1]
    l2 = float(np.mean(diff * diff))
    total = 0.0
    grads = []
    for a, c in enumerate(zc):
        off = _offdiag(c.T @ c / (n - 1))
        total += float(np.sum(np.abs(off)) / (d * (d - 1)))
        g = c @ (lam * 2.0 * np.sign(off) / (d * (d - 1) * (n - 1)))
        if a < 2:
            g = g + (1.0 if a == 0 else -1.0) * 2.0 * diff / (n * d)
        grads.append(g)
    return {"objective": l2 + lam * total, "l2": l2, "sdl": total}, grads, None


def closed_form(kind, views, params, independent=None):
    if kind == "ey":
        return ey(views, independent)
    return {"barlow": barlow, "vicreg": vicreg, "sdl": sdl}[kind](views, *params)
