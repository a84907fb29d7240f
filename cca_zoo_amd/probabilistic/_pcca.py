"""ProbabilisticCCA: Bayesian CCA sampled with the No-U-Turn sampler, every leapfrog step on the device.

Reference: ``cca_zoo/probabilistic/_pcca.py`` (the model, ``:90-131``; the fit, ``:137-189``) and
``cca_zoo/probabilistic/_utils.py`` (``align_posterior_rotation``, ``:112-164``; ``PosteriorMeanTransformMixin``,
``:167-359``).  The reference hands the model to numpyro (``NUTS``, ``MCMC`` with their defaults); here the same sampler is
written out in libccz (``include/ccz.h``, the ``ccz_nuts_*`` section; ``csrc/nuts.hip``) and restated in NumPy in
``tests/pcca_restatement.py``, which is the specification.  These are NOT numpyro's bits: the random numbers are this
library's.  The host draws the initial point from ``default_rng(random_state)``; the device takes whole leapfrog steps
(one read of every view each); the tree and the adaptation scalars are host C++ inside libccz, which reads one small record
per leapfrog.
"""

from __future__ import annotations

import ctypes as C
from numbers import Integral, Real
from typing import Any, ClassVar

import numpy as np
from sklearn.utils._param_validation import Interval

from cca_zoo_amd._base import BaseModel
from cca_zoo_amd._utils._resident import MEANS_COLMEANS, ResidentViews, check_limits, fit_state, refuse_row_sharded
from cca_zoo_amd.probabilistic._posterior import PosteriorMeanMixin, align_posterior_rotation

#: limits of the device path (``csrc/nuts.hip``)
MAX_DIMS, MAX_VIEWS, MAX_TREE_DEPTH = 32, 8, 10
#: largest ``posterior_samples_`` (``num_samples`` draws of every site, float64) that ``fit`` fetches
MAX_SAMPLE_BYTES = 2 << 30
#: transitions per ``ccz_nuts_run`` call (the result does not depend on it)
CHUNK_TRANSITIONS = 50
_STATS = ("tree_depth", "n_leapfrog", "accept_prob", "diverging", "potential_energy", "step_size")


class ProbabilisticCCA(PosteriorMeanMixin, BaseModel):
    r"""Probabilistic CCA with full Bayesian inference by NUTS.

    $$
    W_i \sim \mathcal N(0, I),\quad \log\psi_i \sim \mathcal N(0, I),\quad z \sim \mathcal N(0, I_K),\quad
    x_i \mid z \sim \mathcal N(W_i z, \Psi_i)
    $$

    with, as in the reference's model, $\exp(\log\psi_i)$ entering the likelihood as its standard deviation.  ``num_warmup``
    transitions adapt the step size (dual averaging towards ``target_accept_prob``) and a diagonal mass matrix (Stan's
    windows), ``num_samples`` transitions are kept.  The momenta and the tree's random choices of transition ``t`` come
    from a counter-based generator keyed by ``(random_state, t, site)``, so a fit is a pure function of its inputs: two
    fits give the same bits.  The draws are then aligned by generalised Procrustes (three passes): the model does not
    change under a rotation of the latent space shared by all views, and unaligned draws would average towards zero.

    Fitted attributes: ``weights_`` (float64, ``p_i x k``: the mean of the aligned draws of ``W_i``), ``means_`` (input
    dtype), ``posterior_samples_`` (``W_i``, ``log_psi_i``, ``z``; ``W_i`` and ``z`` aligned), ``sample_stats_`` (per
    transition, warm-up first: ``tree_depth``, ``n_leapfrog``, ``accept_prob``, ``diverging``, ``potential_energy``,
    ``step_size``), ``step_size_`` (after warm-up), ``inverse_mass_matrix_`` (the diagonal, one array per site),
    ``n_divergent_`` (divergent transitions after warm-up), ``n_components_``.

    ``transform`` returns a ONE-element list, the posterior mean of the shared ``z``; ``score`` and the correlations use
    each view's own projection ``(X_i - mean_i) W_i``.

    Differences from the reference, on purpose:

    - Not numpyro's bits: the sampler is the one its call describes, the random numbers are this library's.
    - ``sample_stats_``, ``step_size_``, ``inverse_mass_matrix_`` and ``n_divergent_`` stand in for the reference's
      numpyro object ``mcmc_``.
    - At most 32 latent dimensions, 2 to 8 views, ``max_tree_depth`` at most 10; the sampler's device vectors
      (``15 + 2 max_tree_depth`` of the state's length) may not exceed 64 GiB.
    - All draws together (``num_samples`` times the state's length, float64) may not exceed 2 GiB: ``fit`` raises
      ``ValueError`` and asks for fewer samples.
    - A non-finite potential at the initial point raises ``FloatingPointError``.
    - ``fit`` inside :func:`cca_zoo_amd.row_sharded` raises ``NotImplementedError``.
    - The views are never copied: the rows are read where they lie (float32 views as float32) and device tensors are
      left bit-unchanged.

    Args:
        latent_dimensions: Number of latent components. Default is 1.
        center: Whether to subtract column means. Default True.
        num_warmup: Number of warm-up transitions. Default is 500.
        num_samples: Number of kept draws. Default is 1000.
        random_state: Seed of the initial point and of every transition (``None``: fresh entropy). Default is 0.
        max_tree_depth: Most doublings of a transition's tree (numpyro's default 10).
        target_accept_prob: Target of the step-size adaptation (numpyro's default 0.8).
    """

    _parameter_constraints: ClassVar[dict[str, list[Any]]] = {
        **BaseModel._parameter_constraints,
        "num_warmup": [Interval(Integral, 0, None, closed="left")],
        "num_samples": [Interval(Integral, 1, None, closed="left")],
        "random_state": [Interval(Integral, 0, None, closed="left"), None],
        "max_tree_depth": [Interval(Integral, 1, MAX_TREE_DEPTH, closed="both")],
        "target_accept_prob": [Interval(Real, 0, 1, closed="neither")],
    }

    def __init__(
        self,
        latent_dimensions: int = 1,
        center: bool = True,
        num_warmup: int = 500,
        num_samples: int = 1000,
        random_state: int = 0,
        max_tree_depth: int = 10,
        target_accept_prob: float = 0.8,
    ) -> None:
        super().__init__(latent_dimensions=latent_dimensions, center=center)
        self.num_warmup = num_warmup
        self.num_samples = num_samples
        self.random_state = random_state
        self.max_tree_depth = max_tree_depth
        self.target_accept_prob = target_accept_prob

    @staticmethod
    def _sites(p, n, k):
        """``(name, shape, slice of the flat layout)`` of every site in MODEL order (``W_i`` and ``log_psi_i`` per view,
        then ``z``); the flat layout is ``[W_0 .. | log_psi_0 .. | z]`` (``include/ccz.h``)."""
        ptot, off = sum(p), np.concatenate([[0], np.cumsum(p)]).astype(int)
        o_s = ptot * k
        o_z = o_s + ptot
        out = []
        for i, pi in enumerate(p):
            out.append((f"W_{i}", (pi, k), slice(off[i] * k, off[i + 1] * k)))
            out.append((f"log_psi_{i}", (pi,), slice(o_s + off[i], o_s + off[i + 1])))
        out.append(("z", (n, k), slice(o_z, o_z + n * k)))
        return out

    def fit(self, views, y=None):
        """Fit to a list of (n_samples, n_features_i) host arrays or CUDA tensors."""
        refuse_row_sharded("ProbabilisticCCA moves whole loading matrices and the shared latent variable in every leapfrog "
                           "step, which this build does not shard by rows")
        self._validate_params()
        res = ResidentViews(views, self.center, MEANS_COLMEANS)
        m, n, p = len(res.p), res.n, res.p
        k = int(self.latent_dimensions)
        warm, keep = int(self.num_warmup), int(self.num_samples)
        check_limits(k, m, MAX_DIMS, MAX_VIEWS)
        if m < 2:
            raise ValueError("at least 2 views are required")
        if n < 2:
            raise ValueError("at least 2 samples are required")
        sites = self._sites(p, n, k)
        size = sum(int(np.prod(shape)) for _, shape, _ in sites)
        if keep * size * 8 > MAX_SAMPLE_BYTES:
            raise ValueError(
                f"num_samples={keep}: posterior_samples_ would hold {keep} x {size} float64 values "
                f"({keep * size * 8 / 2 ** 30:.1f} GiB, the limit is {MAX_SAMPLE_BYTES >> 30} GiB); lower num_samples"
            )
        self.n_views_, self.n_features_in_, self.n_samples_ = m, p, n
        rng = np.random.default_rng(self.random_state)
        seed = int(rng.integers(0, 2 ** 63)) if self.random_state is None else int(self.random_state) & (2 ** 64 - 1)
        q0 = np.empty(size)
        for _, shape, sl in sites:        # model order; each site lands in its place of the device's flat layout
            q0[sl] = rng.uniform(-2.0, 2.0, size=shape).reshape(-1)
        pd = C.POINTER(C.c_double)
        total = warm + keep
        draws, stats, minv = np.empty((keep, size)), np.empty((len(_STATS), total)), np.empty(size)
        step, u0 = C.c_double(0.0), C.c_double(0.0)
        with res:
            h = res.handle
            with fit_state(h, "nuts", res.code, m, (C.c_int64 * m)(*p), n, k, warm, keep, int(self.max_tree_depth),
                           float(self.target_accept_prob), C.c_uint64(seed)) as state:
                h.check(h.lib.ccz_nuts_set_init(h.raw, state, res.varr, res.marr, q0.ctypes.data_as(pd), C.byref(u0)))
                if not np.isfinite(u0.value):
                    raise FloatingPointError("ProbabilisticCCA: the potential at the initial point is not finite; rescale the "
                                             "views")
                done = 0
                while done < total:
                    chunk = min(int(CHUNK_TRANSITIONS), total - done)
                    h.check(h.lib.ccz_nuts_run(h.raw, state, res.varr, res.marr, chunk, draws.ctypes.data_as(pd)))
                    done += chunk
                h.check(h.lib.ccz_nuts_get_stats(h.raw, state, stats.ctypes.data_as(pd), C.byref(step), minv.ctypes.data_as(pd)))
        samples = {name: draws[:, sl].reshape(keep, *shape).copy() for name, shape, sl in sites}
        # the model's rotational symmetry: align the stacked loadings of every draw, rotate that draw's z with them
        aligned, rotations = align_posterior_rotation(np.concatenate([samples[f"W_{i}"] for i in range(m)], axis=1))
        off = np.concatenate([[0], np.cumsum(p)]).astype(int)
        for i in range(m):
            samples[f"W_{i}"] = aligned[:, off[i]: off[i + 1]].copy()
        samples["z"] = np.einsum("snk,skj->snj", samples["z"], rotations)
        self.posterior_samples_ = samples
        self.n_components_ = k
        self.sample_stats_ = {name: stats[a].copy() for a, name in enumerate(_STATS)}
        for name in ("tree_depth", "n_leapfrog"):
            self.sample_stats_[name] = self.sample_stats_[name].astype(np.int64)
        self.sample_stats_["diverging"] = self.sample_stats_["diverging"] != 0
        self.step_size_ = float(step.value)
        self.inverse_mass_matrix_ = {name: minv[sl].reshape(shape).copy() for name, shape, sl in sites}
        self.n_divergent_ = int(np.sum(self.sample_stats_["diverging"][warm:]))
        weights = [samples[f"W_{i}"].mean(axis=0) for i in range(m)]
        self._store(weights, res.means_host(), "f32" if res.f32 else "f64", weights_like_input=False)
        return self
