"""VariationalBayesCCA: Bayesian CCA with a shared ARD prior, fitted by mean-field SVI, every step on the device.

Reference: ``cca_zoo/probabilistic/_vbcca.py`` (the model, ``:108-159``; the fit, ``:165-213``) and
``cca_zoo/probabilistic/_utils.py`` (``PosteriorMeanTransformMixin``, ``:167-359``).  The reference hands the model to
numpyro (``AutoNormal``, ``Trace_ELBO``, ``Adam``, ``svi.run``); here the same algorithm is written out in libccz
(``include/ccz.h``, the ``ccz_svi_*`` section; ``csrc/svi.hip``) and restated in NumPy in ``tests/vbcca_restatement.py``.
These are NOT numpyro's bits: its PRNG differs.  The host draws the initial ``loc`` from ``default_rng(random_state)``,
enqueues steps in chunks behind a device stop word, and draws the posterior samples from the same generator afterwards.
"""

from __future__ import annotations

import ctypes as C
from numbers import Integral, Real
from typing import Any, ClassVar

import numpy as np
from sklearn.utils._param_validation import Interval

from cca_zoo_amd._base import BaseModel
from cca_zoo_amd._utils._resident import (MEANS_COLMEANS, ResidentViews, check_limits, fit_state, refuse_row_sharded,
                                           run_chunks)
from cca_zoo_amd.probabilistic._posterior import PosteriorMeanMixin

#: steps per ``ccz_svi_steps`` call: one host wait (for the chunk two calls back) per chunk; the result does not depend on it
CHUNK_STEPS = 64
#: limits of the device path (``csrc/svi.hip``)
MAX_DIMS, MAX_VIEWS = 32, 8
#: largest ``posterior_samples_["z"]`` (``num_posterior_samples x n x k`` float64) that ``fit`` draws
MAX_SAMPLE_BYTES = 2 << 30
#: initial scale of every guide normal (numpyro's ``AutoNormal(init_scale=0.1)``)
_INIT_SCALE = 0.1


def _softplus(r):
    return np.where(r > 0, r + np.log1p(np.exp(-np.abs(r))), np.log1p(np.exp(-np.abs(r))))


class VariationalBayesCCA(PosteriorMeanMixin, BaseModel):
    r"""Variational Bayesian CCA with automatic relevance determination shared across the views.

    $$
    \alpha_k \sim \mathrm{Gamma}(a_0, b_0),\quad W_i[:, k] \sim \mathcal N(0, \alpha_k^{-1} I),\quad
    z \sim \mathcal N(0, I_K),\quad \log\psi_i \sim \mathcal N(0, I),\quad x_i \mid z \sim \mathcal N(W_i z, \Psi_i)
    $$

    with $a_0 = b_0 = 10^{-3}$ and, as in the reference's model, $\exp(\log\psi_i)$ entering the likelihood as its standard
    deviation.  The posterior is approximated by independent normals (``loc``, ``scale = softplus(rho)``; ``scale`` starts at
    0.1, ``loc`` uniform in (-2, 2)) and fitted by ``num_steps`` Adam steps on the one-particle reparameterised ELBO.  The
    noise of step ``t`` comes from a counter-based generator keyed by ``(random_state, t, site)``, so a fit is a pure
    function of its inputs: two fits give the same bits.

    Fitted attributes: ``weights_`` (float64, ``p_i x k``: the mean of the posterior draws of ``W_i``), ``means_`` (input
    dtype), ``ard_relevance_`` (the mean of the draws of $\alpha$; large means shrunk away), ``losses_`` (float64, one per
    step, every normalising constant included), ``posterior_samples_`` (``alpha``, ``W_i``, ``log_psi_i``, ``z``),
    ``variational_params_`` (``loc`` / ``scale`` of every site: ``log_alpha``, ``W_i``, ``log_psi_i``, ``z``; it stands in
    for the reference's numpyro objects ``svi_result_`` / ``guide_``), ``n_iter_``.

    ``transform`` returns a ONE-element list, the posterior mean of the shared ``z``; ``score`` and the correlations use
    each view's own projection ``(X_i - mean_i) W_i``.

    Differences from the reference, on purpose:

    - Not numpyro's bits: the algorithm is the one its call describes, the random numbers are this library's.
    - A step whose loss is not finite ends the fit: ``fit`` raises ``FloatingPointError`` naming the step (the reference
      would return NaNs).
    - ``fit`` inside :func:`cca_zoo_amd.row_sharded` raises ``NotImplementedError``.
    - At most 32 latent dimensions and 2 to 8 views.
    - ``num_posterior_samples * n * latent_dimensions * 8`` bytes may not exceed 2 GiB: ``fit`` raises ``ValueError`` and
      asks for fewer samples.
    - The views are never copied: the rows are read where they lie (float32 views as float32) and device tensors are
      left bit-unchanged.

    Args:
        latent_dimensions: Number of latent components; set it generously and read ``ard_relevance_``. Default is 1.
        center: Whether to subtract column means. Default True.
        num_steps: Number of SVI steps. Default is 2000.
        learning_rate: Adam's learning rate. Default is 1e-2.
        num_posterior_samples: Draws in ``posterior_samples_``. Default is 1000.
        random_state: Seed of the initial ``loc``, of the noise of every step and of the posterior draws (``None``:
            fresh entropy). Default is 0.
    """

    _parameter_constraints: ClassVar[dict[str, list[Any]]] = {
        **BaseModel._parameter_constraints,
        "num_steps": [Interval(Integral, 1, None, closed="left")],
        "learning_rate": [Interval(Real, 0, None, closed="neither")],
        "num_posterior_samples": [Interval(Integral, 1, None, closed="left")],
        "random_state": [Interval(Integral, 0, None, closed="left"), None],
    }

    def __init__(
        self,
        latent_dimensions: int = 1,
        center: bool = True,
        num_steps: int = 2000,
        learning_rate: float = 1e-2,
        num_posterior_samples: int = 1000,
        random_state: int = 0,
    ) -> None:
        super().__init__(latent_dimensions=latent_dimensions, center=center)
        self.num_steps = num_steps
        self.learning_rate = learning_rate
        self.num_posterior_samples = num_posterior_samples
        self.random_state = random_state

    # -- fit -------------------------------------------------------------------------------------------------------
    def fit(self, views, y=None):
        """Fit to a list of (n_samples, n_features_i) host arrays or CUDA tensors."""
        refuse_row_sharded("VariationalBayesCCA updates whole loading matrices and the shared latent variable in every step, "
                           "which this build does not shard by rows")
        self._validate_params()
        res = ResidentViews(views, self.center, MEANS_COLMEANS)
        m, n, p = len(res.p), res.n, res.p
        k = int(self.latent_dimensions)
        s = int(self.num_posterior_samples)
        check_limits(k, m, MAX_DIMS, MAX_VIEWS)
        if m < 2:
            raise ValueError("at least 2 views are required")
        if n < 2:
            raise ValueError("at least 2 samples are required")
        if s * n * k * 8 > MAX_SAMPLE_BYTES:
            raise ValueError(
                f"num_posterior_samples={s}: posterior_samples_['z'] would hold {s} x {n} x {k} float64 values "
                f"({s * n * k * 8 / 2 ** 30:.1f} GiB, the limit is {MAX_SAMPLE_BYTES >> 30} GiB); lower num_posterior_samples"
            )
        self.n_views_, self.n_features_in_, self.n_samples_ = m, p, n
        total = int(self.num_steps)
        chunk = max(1, min(int(CHUNK_STEPS), total))
        rng = np.random.default_rng(self.random_state)
        seed = int(rng.integers(0, 2 ** 63)) if self.random_state is None else int(self.random_state) & (2 ** 64 - 1)
        sites = self._sites(p, n, k)
        size = sum(int(np.prod(shape)) for _, shape, _ in sites)
        loc0 = np.empty(size)
        for _, shape, sl in sites:        # model order; each site lands in its place of the device's flat layout
            loc0[sl] = rng.uniform(-2.0, 2.0, size=shape).reshape(-1)
        pd = C.POINTER(C.c_double)
        loc, rho, losses = np.empty(size), np.empty(size), np.empty(total)
        with res:
            h = res.handle
            with fit_state(h, "svi", res.code, m, (C.c_int64 * m)(*p), n, k, total, float(self.learning_rate), C.c_uint64(seed),
                           chunk) as state:
                h.check(h.lib.ccz_svi_set_init(h.raw, state, loc0.ctypes.data_as(pd)))
                known, stopped = C.c_int64(-1), C.c_int(0)

                def steps(step):
                    h.check(h.lib.ccz_svi_steps(h.raw, state, res.varr, res.marr, step, C.byref(known), C.byref(stopped)))
                    return stopped.value

                run_chunks(total, chunk, steps)
                done, stop, bad = C.c_int64(0), C.c_int(0), C.c_int64(-1)
                h.check(h.lib.ccz_svi_status(h.raw, state, C.byref(done), C.byref(stop), C.byref(bad)))
                if bad.value >= 0:
                    raise FloatingPointError(f"VariationalBayesCCA: the loss of step {bad.value} is not finite; lower learning_rate "
                                             "or rescale the views")
                if not stop.value:
                    raise RuntimeError(f"VariationalBayesCCA fit ended after {done.value} of {total} steps")   # cannot happen
                h.check(h.lib.ccz_svi_get_result(h.raw, state, loc.ctypes.data_as(pd), rho.ctypes.data_as(pd),
                                                 losses.ctypes.data_as(pd)))
        scale = _softplus(rho)
        self.n_iter_ = int(done.value)
        self.n_components_ = k
        self.losses_ = losses
        self.variational_params_ = {name: {"loc": loc[sl].reshape(shape).copy(), "scale": scale[sl].reshape(shape).copy()}
                                    for name, shape, sl in sites}
        samples = {}
        for name, shape, sl in sites:     # after the initial draws, from the same generator, in model order
            d = loc[sl].reshape(shape)[np.newaxis] + scale[sl].reshape(shape)[np.newaxis] * rng.standard_normal((s, *shape))
            if name == "log_alpha":
                samples["alpha"] = np.exp(d)
            else:
                samples[name] = d
        self.posterior_samples_ = samples
        weights = [samples[f"W_{i}"].mean(axis=0) for i in range(m)]
        self._store(weights, res.means_host(), "f32" if res.f32 else "f64", weights_like_input=False)
        self.ard_relevance_ = samples["alpha"].mean(axis=0)
        return self

    @staticmethod
    def _sites(p, n, k):
        """``(name, shape, slice of the flat layout)`` of every site in MODEL order (``log_alpha``, then ``W_i`` and
        ``log_psi_i`` per view, then ``z``); the flat layout is ``[a | W_0 .. | log_psi_0 .. | z]`` (``include/ccz.h``)."""
        ptot, off = sum(p), np.concatenate([[0], np.cumsum(p)]).astype(int)
        o_w, o_s = k, k + ptot * k
        o_z = o_s + ptot
        out = [("log_alpha", (k,), slice(0, k))]
        for i, pi in enumerate(p):
            out.append((f"W_{i}", (pi, k), slice(o_w + off[i] * k, o_w + off[i + 1] * k)))
            out.append((f"log_psi_{i}", (pi,), slice(o_s + off[i], o_s + off[i + 1])))
        out.append(("z", (n, k), slice(o_z, o_z + n * k)))
        return out

    # -- after the fit: transform, the correlations' variates and log_likelihood come from PosteriorMeanMixin
