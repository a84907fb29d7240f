"""The specification of ``cca_zoo_amd.model_selection.jackknife`` and of the BCa interval of ``bootstrap(method="BCa")`` in
float64 NumPy, written the slow literal way (imported by tests/test_jack_host.py and tests/test_gpu_jack.py).

Replicate ``g`` of ``J`` is the refit of tests/boot_restatement.py on the rows that are NOT in group ``g``; group ``g`` holds the
rows ``s`` with ``s % J == g``.  ``se = sqrt((J - 1) / J * sum_g (theta_g - mean)^2)``, ``bias = (J - 1) (mean - observed)``.
The BCa interval of one scalar (Efron 1987, as ``scipy.stats.bootstrap`` computes it):

    z0 = Phi^-1((#{boot < theta} + #{boot <= theta}) / (2 B)),   a = sum d^3 / (6 (sum d^2)^(3/2)),  d = mean(jack) - jack,
    alpha_-+ = Phi(z0 + (z0 -+ z) / (1 - a (z0 -+ z))),  z = Phi^-1((1 + cl) / 2),   ci = quantile(boot, [alpha_-, alpha_+]);

NaN where ``z0`` is infinite or ``sum d^2 = 0``.  Phi and its inverse are those of ``statistics.NormalDist``.
"""

import math
from statistics import NormalDist
from types import SimpleNamespace

import numpy as np

import boot_restatement as br

NORMAL = NormalDist()


def groups(n, J):
    """The rows each replicate leaves out."""
    return [np.array([s for s in range(n) if s % J == g], dtype=np.int64) for g in range(J)]


def fit_without(X1, X2, left_out, c, center, k):
    keep = np.ones(X1.shape[0], dtype=bool)
    keep[left_out] = False
    return br.fit_rows(X1[keep], X2[keep], c, center, k)


def summaries(jack, observed):
    jack = np.asarray(jack, dtype=np.float64)
    J = jack.shape[0]
    mean = jack.sum(axis=0) / J
    return np.sqrt((J - 1) / J * ((jack - mean) ** 2).sum(axis=0)), (J - 1) * (mean - observed)


def jackknife(views, c=0.0, center=True, k=1, J=None, only=None):
    """Everything ``jackknife`` returns but the estimator, plus the per-fit ``cond`` (observed first); ``only``: the replicates
    to refit (default all; the summaries are left out then)."""
    X1, X2 = (np.asarray(v, dtype=np.float64) for v in views)
    n = X1.shape[0]
    J = min(n, 4096) if J is None else J
    k = min(k, X1.shape[1], X2.shape[1])
    obs = br.fit_rows(X1, X2, c, center, k)
    O1, O2 = br.orient_observed(*obs.weights)
    grp = groups(n, J)
    which = range(J) if only is None else only
    sv, w, cond = [], [[], []], [obs.cond]
    for g in which:
        f = fit_without(X1, X2, grp[g], c, center, k)
        W1, W2 = br.orient_to(f.weights[0], f.weights[1], O1, O2)
        sv.append(f.sv), w[0].append(W1), w[1].append(W2), cond.append(f.cond)
    sv, w = np.stack(sv), [np.stack(x) for x in w]
    out = SimpleNamespace(singular_values=obs.sv, weights=[O1, O2], singular_values_jack=sv, weights_jack=w, n_groups=J,
                          replicates=list(which), cond=np.asarray(cond))
    if only is None:
        out.singular_values_se, out.singular_values_bias = summaries(sv, obs.sv)
        s = [summaries(a, o) for a, o in zip(w, out.weights)]
        out.weights_se, out.weights_bias = [x[0] for x in s], [x[1] for x in s]
    return out


def inv_phi(q):
    if q <= 0.0:
        return -math.inf
    if q >= 1.0:
        return math.inf
    return NORMAL.inv_cdf(q)


def bca_interval(theta, boot, jack, confidence_level):
    """``(lo, hi, z0, a)`` of one scalar statistic, with loops."""
    B, J = len(boot), len(jack)
    below = sum(1 for b in boot if b < theta) + sum(1 for b in boot if b <= theta)
    z0 = inv_phi(below / (2.0 * B))
    mean = sum(float(x) for x in jack) / J
    d2 = sum((mean - float(x)) ** 2 for x in jack)
    d3 = sum((mean - float(x)) ** 3 for x in jack)
    a = d3 / (6.0 * d2 ** 1.5) if d2 > 0.0 else math.nan
    if math.isinf(z0) or math.isnan(a):
        return math.nan, math.nan, z0, a
    z = NORMAL.inv_cdf((1.0 + confidence_level) / 2.0)
    ends = []
    for sz in (-z, z):
        den = 1.0 - a * (z0 + sz)
        arg = z0 + (z0 + sz) / den if den != 0.0 else math.copysign(math.inf, z0 + sz)
        alpha = 0.0 if arg == -math.inf else 1.0 if arg == math.inf else NORMAL.cdf(arg)
        ends.append(float(np.quantile(np.asarray(boot, dtype=np.float64), alpha)))
    return ends[0], ends[1], z0, a


def bca_all(theta, boot, jack, confidence_level):
    """:func:`bca_interval` entry by entry: ``(ci (2,) + S, z0 S, a S)``."""
    theta, boot, jack = np.asarray(theta, dtype=np.float64), np.asarray(boot, dtype=np.float64), np.asarray(jack, dtype=np.float64)
    ci, z0, a = np.empty((2,) + theta.shape), np.empty(theta.shape), np.empty(theta.shape)
    for e in np.ndindex(*theta.shape):
        lo, hi, z0[e], a[e] = bca_interval(float(theta[e]), boot[(slice(None),) + e], jack[(slice(None),) + e], confidence_level)
        ci[(0,) + e], ci[(1,) + e] = lo, hi
    return ci, z0, a


def restate_bca(views, c=0.0, center=True, k=1, n_resamples=1000, confidence_level=0.95, random_state=None, J=None):
    """``bootstrap(method="BCa")``: the percentile restatement, the jackknife above and the intervals entry by entry."""
    boot = br.restate(views, c=c, center=center, k=k, n_resamples=n_resamples, confidence_level=confidence_level, random_state=random_state)
    jack = jackknife(views, c=c, center=center, k=k, J=J)
    out = SimpleNamespace(**vars(boot))
    out.singular_values_ci_percentile, out.weights_ci_percentile = boot.singular_values_ci, boot.weights_ci
    out.singular_values_jack, out.weights_jack, out.n_groups = jack.singular_values_jack, jack.weights_jack, jack.n_groups
    out.singular_values_ci, out.singular_values_z0, out.singular_values_acceleration = bca_all(
        boot.singular_values, boot.singular_values_boot, jack.singular_values_jack, confidence_level)
    w = [bca_all(o, b, j, confidence_level) for o, b, j in zip(boot.weights, boot.weights_boot, jack.weights_jack)]
    out.weights_ci, out.weights_z0, out.weights_acceleration = [x[0] for x in w], [x[1] for x in w], [x[2] for x in w]
    out.cond = np.concatenate([boot.cond, jack.cond[1:]])
    return out
