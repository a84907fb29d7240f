"""Shared mini-batch momentum-SGD loop of the Eckart-Young (EY) models, run on the device.

Reference: ``cca_zoo/linear/gradient/_base.py:101-130`` (the loop), ``cca_zoo/_utils/_ey.py:98-127`` (PLS_EY's
initial weights) and ``:129-185`` (CCA_EY's).  Every gradient step runs in libccz (``csrc/ey.hip``, four launches per
step); the host draws the mini-batch indices with NumPy itself, in the reference's order, one chunk of steps ahead of
the device, and does the two one-off QR factorisations of the initialisation.
"""

from __future__ import annotations

import ctypes as C
from typing import Any, ClassVar

import numpy as np

from cca_zoo_amd._base import BaseModel
from cca_zoo_amd._utils._resident import MEANS_TORCH, ResidentViews, fit_state, refuse_row_sharded, run_chunks

#: steps per ``ccz_ey_steps`` call: one host wait (for the chunk two calls back) and one index upload per chunk
CHUNK_STEPS = 64


def draw_batches(rng, n, bs, steps):
    """``steps`` x ``bs`` row indices, one ``rng.choice(n, bs, replace=False)`` per step, as the reference draws them
    (``_base.py:118``)."""
    return np.stack([rng.choice(n, bs, replace=False) for _ in range(steps)]).astype(np.int64, copy=False)


def initial_weights(kind, p, k, n, bs, rng, project):
    """The reference's initial weights with its RNG draw order.  ``kind`` "pls": ``qr(N(p_i, k)).Q`` per view
    (``_ey.py:120-126``).  ``kind`` "cca": one ``choice(n, bs)`` and then, per view, ``w0 = qr(N(p_i, k)).Q``,
    ``z0 = X_i[idx] w0`` (``project(idx, w0s)``, on the device), ``R = qr(z0).R`` on the host -- LAPACK's signs decide
    the result -- and ``w0 R^-1`` (``_ey.py:177-184``)."""
    if kind == "pls":
        return [np.linalg.qr(rng.standard_normal((pi, k)))[0] for pi in p]
    idx = rng.choice(n, bs, replace=False)
    w0s = [np.linalg.qr(rng.standard_normal((pi, k)))[0] for pi in p]
    z0s = project(idx, w0s)
    out = []
    for w0, z0 in zip(w0s, z0s):
        _, r = np.linalg.qr(z0)
        out.append(w0 @ np.linalg.solve(r, np.eye(k)))
    return out


class BaseGradientModel(BaseModel):
    """Mini-batch momentum SGD of the EY models on the device (see module docstring).

    ``n_iter_`` (not in the reference) is the number of gradient steps applied: ``max_iter``, or the step after which
    ``|prev - obj| < tol`` stopped the loop.
    """

    _parameter_constraints: ClassVar[dict[str, list[Any]]] = {
        **BaseModel._parameter_constraints,
    }
    _init_kind = "cca"

    def __init__(
        self,
        latent_dimensions: int = 1,
        center: bool = True,
        learning_rate: float = 1e-2,
        max_iter: int = 1000,
        batch_size: int | None = None,
        tol: float = 1e-6,
        momentum: float = 0.9,
        random_state: int | None = None,
    ) -> None:
        super().__init__(latent_dimensions=latent_dimensions, center=center)
        self.learning_rate = learning_rate
        self.max_iter = max_iter
        self.batch_size = batch_size
        self.tol = tol
        self.momentum = momentum
        self.random_state = random_state

    def _ridge(self) -> float:
        return float(self.c)

    def fit(self, views, y=None):
        refuse_row_sharded(f"{type(self).__name__} takes a global mini-batch per step, which does not shard by rows")
        self._validate_params()
        # the reference's _setup_fit: v.mean(axis=0) in the input dtype (torch's mean for device rows)
        res = ResidentViews(views, self.center, MEANS_TORCH)
        m, n, p = len(res.p), res.n, res.p
        k = int(self.latent_dimensions)
        if k > min(p):
            raise ValueError(f"latent_dimensions={k} exceeds the smallest view width ({min(p)})")
        if k > 128:
            raise ValueError(f"latent_dimensions={k}: the device path supports at most 128")
        if n < 1:
            raise ValueError("at least 1 sample is required")
        self.n_views_, self.n_features_in_, self.n_samples_ = m, p, n
        bs = n if self.batch_size is None else min(int(self.batch_size), n)
        full = bs == n
        chunk = max(1, min(CHUNK_STEPS, int(self.max_iter)))
        with res:
            h, varr, marr = res.handle, res.varr, res.marr
            with fit_state(h, "ey", res.code, m, (C.c_int64 * m)(*p), k, bs, chunk, self._ridge(), float(self.learning_rate),
                           float(self.momentum), float(self.tol)) as state:
                rng = np.random.default_rng(self.random_state)

                def project(idx, w0s):
                    h.check(h.lib.ccz_ey_set_weights(h.raw, state, _dp(_wblocks(w0s))))
                    z = np.empty((m, bs, k))
                    ia = np.ascontiguousarray(idx, dtype=np.int64)
                    h.check(h.lib.ccz_ey_project(h.raw, state, varr, marr, n, ia.ctypes.data_as(C.POINTER(C.c_int64)),
                                                 z.ctypes.data_as(C.POINTER(C.c_double))))
                    return [z[i] for i in range(m)]

                W0 = initial_weights(self._init_kind, p, k, n, bs, rng, project)
                h.check(h.lib.ccz_ey_set_weights(h.raw, state, _dp(_wblocks(W0))))
                known, stopped = C.c_int64(-1), C.c_int(0)

                def steps_chunk(s):
                    idx = None if full else draw_batches(rng, n, bs, s)
                    ip = None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_int64))
                    h.check(h.lib.ccz_ey_steps(h.raw, state, varr, marr, n, ip, s, C.byref(known), C.byref(stopped)))
                    return stopped.value

                run_chunks(int(self.max_iter), chunk, steps_chunk)
                steps, stop, obj = C.c_int64(0), C.c_int(0), C.c_double(0.0)
                h.check(h.lib.ccz_ey_status(h.raw, state, C.byref(steps), C.byref(stop), C.byref(obj)))
                wflat = np.empty(sum(p) * k)
                h.check(h.lib.ccz_ey_get_weights(h.raw, state, wflat.ctypes.data_as(C.POINTER(C.c_double))))
        self.n_iter_ = int(steps.value)
        weights = np.split(wflat.reshape(-1, k), np.cumsum(p)[:-1])
        self._store(weights, res.means_host(), "f32" if res.f32 else "f64", weights_like_input=False)
        return self


def _wblocks(ws):
    """The W blocks of ``ccz_ey_set_weights``: every view's (p_i x k) weights, row-major, back to back."""
    return np.ascontiguousarray(np.concatenate([np.asarray(w, dtype=np.float64).reshape(-1) for w in ws]))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))

