"""NumPy float64 restatement of the SVI algorithm of ``VariationalBayesCCA`` (``include/ccz.h``, the ``ccz_svi_*`` section;
``cca_zoo_amd/csrc/svi.hip``).

TEST INFRASTRUCTURE ONLY.  The reference (``cca_zoo/probabilistic/_vbcca.py``) runs numpyro's ``AutoNormal`` /
``Trace_ELBO`` / ``Adam``, which cannot be run here; this file writes the same algorithm out with numpyro's documented
defaults.  These are NOT numpyro's bits (its PRNG differs).  ``tests/test_vbcca_host.py`` anchors it: the loss against
``scipy.stats``, the gradient against central differences, one Adam step against a hand computation.

Flat layout of every parameter-shaped vector (``N = k + P k + P + n k``, ``P = sum p_i``)::

    [ a (k) | W_0 .. W_{M-1} (each p_i x k row-major, back to back) | s_0 .. s_{M-1} | Z (n x k row-major) ]

Sites are numbered 0: a, 1 + 2 i: W_i, 2 + 2 i: s_i, 1 + 2 M: Z.  The host draws (initial ``loc``, posterior samples) go
through the sites in MODEL order: a, W_0, s_0, W_1, s_1, .., Z.
"""

from __future__ import annotations

import math

import numpy as np

from oracle.rng import splitmix64

A0 = B0 = 1e-3
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8
INIT_SCALE = 0.1
_U64 = 0xFFFFFFFFFFFFFFFF


class Layout:
    def __init__(self, p, n, k):
        self.p, self.n, self.k, self.m = [int(x) for x in p], int(n), int(k), len(p)
        self.ptot = sum(self.p)
        self.off = np.concatenate([[0], np.cumsum(self.p)]).astype(int)
        self.oW, self.oS = self.k, self.k + self.ptot * self.k
        self.oZ = self.oS + self.ptot
        self.N = self.oZ + self.n * self.k

    def a(self, x):
        return x[: self.k]

    def W(self, x, i):
        return x[self.oW + self.off[i] * self.k: self.oW + self.off[i + 1] * self.k].reshape(self.p[i], self.k)

    def s(self, x, i):
        return x[self.oS + self.off[i]: self.oS + self.off[i + 1]]

    def Z(self, x):
        return x[self.oZ:].reshape(self.n, self.k)

    def sites(self):
        """(site number, view of the flat vector -> array) in MODEL order."""
        out = [(0, lambda x: self.a(x))]
        for i in range(self.m):
            out.append((1 + 2 * i, lambda x, i=i: self.W(x, i)))
            out.append((2 + 2 * i, lambda x, i=i: self.s(x, i)))
        out.append((1 + 2 * self.m, lambda x: self.Z(x)))
        return out


def stream(seed, t, site):
    """``splitmix64(splitmix64(splitmix64(seed) + t) + site)`` with 64-bit wrap-around."""
    a = int(splitmix64(np.uint64(int(seed) & _U64)))
    b = int(splitmix64(np.uint64((a + int(t)) & _U64)))
    return int(splitmix64(np.uint64((b + int(site)) & _U64)))


def hash_normal(seed, index):
    """``cca_zoo_amd/csrc/rng_hash.h::hash_normal``: one normal per (seed, index), Box-Muller's cosine branch."""
    index = np.asarray(index, dtype=np.uint64)
    s = np.uint64(int(seed) & _U64)
    with np.errstate(over="ignore"):
        a = splitmix64(s ^ splitmix64(np.uint64(2) * index))
        b = splitmix64(s ^ splitmix64(np.uint64(2) * index + np.uint64(1)))
    u1 = ((a >> np.uint64(11)).astype(np.float64) + 1.0) * (1.0 / 9007199254740993.0)
    u2 = (b >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def draw_eps(lay, seed, t):
    eps = np.empty(lay.N)
    for site, view in lay.sites():
        v = view(eps)
        v[...] = hash_normal(stream(seed, t, site), np.arange(v.size, dtype=np.uint64)).reshape(v.shape)
    return eps


def init_loc(rng, lay):
    """Uniform in (-2, 2), drawn site by site in model order from ``rng``."""
    loc = np.empty(lay.N)
    for _, view in lay.sites():
        v = view(loc)
        v[...] = rng.uniform(-2.0, 2.0, size=v.shape)
    return loc


def softplus(r):
    return np.where(r > 0, r + np.log1p(np.exp(-np.abs(r))), np.log1p(np.exp(-np.abs(r))))


def sigmoid(r):
    return 1.0 / (1.0 + np.exp(-r))


def centred(views, means):
    """``fl(x - mean)`` in the views' common dtype (float32 only if every view is), widened to float64."""
    f32 = all(np.asarray(v).dtype == np.float32 for v in views)
    dt = np.float32 if f32 else np.float64
    out = []
    for i, v in enumerate(views):
        x = np.asarray(v, dtype=dt)
        if means is not None and means[i] is not None:
            x = x - np.asarray(means[i], dtype=dt)
        out.append(np.asarray(x, dtype=np.float64))
    return out


def _dot(a, b, perturb):
    """``a @ b``; ``perturb`` reverses the order of the contraction (the conditioning probe of the trajectory tests)."""
    return a[:, ::-1] @ b[::-1, :] if perturb else a @ b


def log_joint_and_grad(lay, theta, xc, perturb=False):
    """``log p(x, theta) + sum a`` with every normalising constant, and its gradient with respect to theta (flat)."""
    k, n, P = lay.k, lay.n, lay.ptot
    a, Z = lay.a(theta), lay.Z(theta)
    alpha = np.exp(a)
    g = np.zeros(lay.N)
    l2pi = math.log(2.0 * math.pi)
    lp = k * (A0 * math.log(B0) - math.lgamma(A0)) + np.sum((A0 - 1.0) * a - B0 * alpha) + np.sum(a)
    lp += np.sum(-0.5 * l2pi - 0.5 * Z * Z)
    gz = -Z.copy()
    w2 = np.zeros(k)
    for i in range(lay.m):
        W, s = lay.W(theta, i), lay.s(theta, i)
        R = xc[i] - _dot(Z, W.T, perturb)
        e2 = np.exp(-2.0 * s)
        D = R * e2
        s2 = (R[::-1] * D[::-1]).sum(axis=0) if perturb else (R * D).sum(axis=0)
        lp += np.sum(-0.5 * s2 - n * s) - 0.5 * l2pi * n * lay.p[i]
        lp += np.sum(-0.5 * l2pi - 0.5 * s * s)
        lp += np.sum(-0.5 * l2pi + 0.5 * a - 0.5 * alpha * W * W)
        lay.W(g, i)[...] = _dot(D.T, Z, perturb) - alpha * W
        lay.s(g, i)[...] = s2 - n - s
        gz += _dot(D, W, perturb)
        w2 += (W * W).sum(axis=0)
    lay.Z(g)[...] = gz
    lay.a(g)[...] = A0 - B0 * alpha + 0.5 * P - 0.5 * alpha * w2
    return float(lp), g


def loss_and_grads(lay, loc, rho, eps, xc, perturb=False):
    """One-particle ``loss = -(log p(x, theta) + sum a - log q(theta))`` and d ELBO / d loc, d ELBO / d rho, theta."""
    scale = softplus(rho)
    theta = loc + scale * eps
    lp, g = log_joint_and_grad(lay, theta, xc, perturb)
    log_q = np.sum(-0.5 * math.log(2.0 * math.pi) - np.log(scale) - 0.5 * eps * eps)
    return -(lp - log_q), g, (g * eps + 1.0 / scale) * sigmoid(rho), theta


def adam(x, m, v, grad_loss, lr, t):
    m = B1 * m + (1.0 - B1) * grad_loss
    v = B2 * v + (1.0 - B2) * grad_loss * grad_loss
    x = x - lr * (m / (1.0 - B1 ** (t + 1))) / (np.sqrt(v / (1.0 - B2 ** (t + 1))) + ADAM_EPS)
    return x, m, v


def new_state(loc0):
    z = np.zeros_like(loc0)
    return dict(loc=loc0.copy(), rho=np.full_like(loc0, math.log(math.expm1(INIT_SCALE))), m1=z.copy(), v1=z.copy(), m2=z.copy(),
                v2=z.copy())


def step(lay, st, xc, seed, lr, t, perturb=False):
    """Step t in place; returns (loss, theta, eps, d theta)."""
    eps = draw_eps(lay, seed, t)
    loss, gl, gr, theta = loss_and_grads(lay, st["loc"], st["rho"], eps, xc, perturb)
    st["loc"], st["m1"], st["v1"] = adam(st["loc"], st["m1"], st["v1"], -gl, lr, t)
    st["rho"], st["m2"], st["v2"] = adam(st["rho"], st["m2"], st["v2"], -gr, lr, t)
    return loss, theta, eps, gl


def run(views, means, k, num_steps, lr, seed, loc0, perturb=False):
    """The whole fit: ``dict(loc, rho, losses, bad_step)``; stops after the first step whose loss is not finite."""
    xc = centred(views, means)
    lay = Layout([x.shape[1] for x in xc], xc[0].shape[0], k)
    st = new_state(loc0)
    losses, bad = np.zeros(num_steps), -1
    with np.errstate(all="ignore"):
        for t in range(num_steps):
            losses[t] = step(lay, st, xc, seed, lr, t, perturb)[0]
            if not np.isfinite(losses[t]):
                bad = t
                break
    return dict(loc=st["loc"], rho=st["rho"], losses=losses, bad_step=bad, layout=lay)


def posterior_samples(rng, lay, loc, scale, num_samples):
    """``num_samples`` draws from q, site by site in model order, from ``rng`` (after the initial draws)."""
    out = {}
    names = ["alpha"] + [x for i in range(lay.m) for x in (f"W_{i}", f"log_psi_{i}")] + ["z"]
    for name, (_, view) in zip(names, lay.sites()):
        mu, sd = view(loc), view(scale)
        d = mu[np.newaxis] + sd[np.newaxis] * rng.standard_normal((num_samples, *mu.shape))
        out[name] = np.exp(d) if name == "alpha" else d
    return out


def fit_expectation(views, k, num_steps, lr, random_state, num_samples, center=True):
    """What ``VariationalBayesCCA.fit`` must give on host arrays: the same generator, in the same order."""
    f32 = all(np.asarray(v).dtype == np.float32 for v in views)
    dt = np.float32 if f32 else np.float64
    xs = [np.asarray(v, dtype=dt) for v in views]
    means = [x.mean(axis=0) for x in xs] if center else None
    rng = np.random.default_rng(random_state)
    lay = Layout([x.shape[1] for x in xs], xs[0].shape[0], k)
    loc0 = init_loc(rng, lay)
    res = run(xs, means, k, num_steps, lr, random_state, loc0)
    scale = softplus(res["rho"])
    samples = posterior_samples(rng, lay, res["loc"], scale, num_samples)
    res.update(samples=samples, weights=[samples[f"W_{i}"].mean(axis=0) for i in range(lay.m)],
               ard_relevance=samples["alpha"].mean(axis=0), scale=scale, means=means)
    return res
