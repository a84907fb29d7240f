"""The eigen-free objectives of the reference's self-supervised models as ``nn.Module`` callables backed by libccz.

Reference: ``DCCA_EY.loss`` (cca_zoo/deep/_dcca_ey.py:10-111), ``BarlowTwins.loss`` (_barlowtwins.py:83-112), ``VICReg.loss``
(_vicreg.py:12-67, :142-169) and ``DCCA_SDL.loss`` (_dcca_sdl.py:12-26, :100-121).  Contract kept: ``forward(list[Tensor (batch x
d)]) -> 0-dim Tensor`` on the inputs' device / dtype, differentiable w.r.t. every input, stateless modules; ``terms(...)`` returns
the reference's whole dictionary (``objective`` and the loss's own terms) as detached 0-dim tensors, under no-grad.

What runs underneath (``ccz_moment_loss_forward``, csrc/ssl_loss.hip): every one of these losses is a function of the batch second
moments of ``[z_1 .. z_m]`` -- ONE K1 pass, the matrix ``CCALoss`` already builds --, a small map on the D x D moments that
writes the terms, the objective and ``Gamma``, and (VICReg, SDL) one streaming pass for ``mean((z_1 - z_2)^2)``; every gradient is
the sample-side product ``Z Gamma - 1 (mean' Gamma_c)`` of ``ccz_pair_loss_backward`` with the upstream gradient applied inside.
No centred copies, no n x d x d products per term, no boolean masks, no autograd through any of it; enqueue-only in torch's
current stream.

``torch.bfloat16`` / ``torch.float16`` views are accepted as a format (see ``objectives.py``): the objective and the terms are then
float32 0-dim tensors and every gradient is rounded once into its input's dtype.

Differences from the reference, on purpose:

* all views of a list must have the same width (the reference fails or broadcasts in ``torch`` depending on the loss);
* ``VICRegLoss`` with more than two views is an error (the reference silently ignores views beyond the second);
* ``SDLLoss`` with one column per view is an error (the reference returns NaN: the mean of an empty off-diagonal);
* under ``row_sharded()`` these modules raise, as ``TCCALoss`` does: they are not sharded.
"""

from __future__ import annotations

import ctypes as C

import torch
from torch.autograd.function import once_differentiable
import torch.nn as nn

from cca_zoo_amd import _backend
from cca_zoo_amd.deep.objectives import _loss_dtype, _require_cuda, _stream_ptr, _view_of, _views_of

__all__ = ["EYLoss", "BarlowTwinsLoss", "VICRegLoss", "SDLLoss"]

_EY, _BARLOW, _VICREG, _SDL = 0, 1, 2, 3          # include/ccz.h: CCZ_MOMENT_*
_MAX_VIEWS = 8
_TERM_KEYS = {
    _EY: ("rewards", "penalties"),
    _BARLOW: ("invariance", "redundancy"),
    _VICREG: ("sim_loss", "var_loss", "cov_loss"),
    _SDL: ("l2", "sdl"),
}


def _validate(what: str, kind: int, reps, label: str = "representations", like=None) -> list[torch.Tensor]:
    """The checks that need no device, in a fixed order: view count, (batch, d) tensors, equal batch size, equal widths, SDL's
    two columns.  The CUDA / dtype checks follow in ``_MomentLoss._check`` once every list has passed these."""
    zs = list(reps)
    if kind in (_BARLOW, _VICREG):
        if len(zs) != 2:
            raise ValueError(f"{what} expects exactly 2 {label}, got {len(zs)}.")
    elif not 2 <= len(zs) <= _MAX_VIEWS:
        raise ValueError(f"{what} expects 2 to {_MAX_VIEWS} {label}, got {len(zs)}.")
    if like is not None and len(zs) != len(like):
        raise ValueError(f"{what} expects as many {label} as representations ({len(like)}), got {len(zs)}.")
    for z in zs:
        if not isinstance(z, torch.Tensor) or z.dim() != 2:
            raise ValueError(f"{what} expects (batch, d_i) tensors")
    for z in zs:
        if z.shape[0] != zs[0].shape[0]:
            raise ValueError(f"{what} expects (batch, d_i) tensors with equal batch size")
    widths = [int(z.shape[1]) for z in zs] + ([int(like[0].shape[1])] if like is not None else [])
    if len(set(widths)) != 1 or widths[0] < 1:
        raise ValueError(f"{what}: every view must have the same width, got widths {widths[:len(zs)]}"
                         + (f" against {widths[-1]} of the representations" if like is not None else ""))
    if kind == _SDL and widths[0] < 2:
        raise ValueError(f"{what} needs at least 2 columns per view, got {widths[0]} (the mean of an empty off-diagonal is undefined)")
    return zs


def _evaluate(kind: int, params, vs, vis, want_state: bool, want_state_ind: bool, want_terms: bool):
    """One device pass: ``(objective (0-dim, the views' dtype), terms (3 float64 on the device) or None, state, state_ind)``."""
    dt, dev = vs[0].dtype, vs[0].device
    m, n, d = len(vs), int(vs[0].shape[0]), int(vs[0].shape[1])
    h = _backend.handle_for(vs)
    code = _backend.dtype_code(dt)
    loss = torch.empty((), dtype=_loss_dtype(dt), device=dev)       # half views: a float32 element
    terms = torch.empty(3, dtype=torch.float64, device=dev) if want_terms else None

    def new_state():
        nbytes = int(h.lib.ccz_moment_loss_state_bytes(code, d, m))
        if nbytes <= 0:
            raise ValueError("unsupported views")
        return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)

    state = new_state() if want_state else None
    state_ind = new_state() if (want_state_ind and vis is not None) else None
    par = (C.c_double * 3)(*(list(params) + [0.0] * (3 - len(params))))
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None    # noqa: E731
    sp = _stream_ptr(vs[0])
    h.adopt(sp)                                             # the loss's kernels go INTO torch's current stream
    try:
        h.check(h.lib.ccz_moment_loss_forward(h.raw, code, kind, par, _views_of(vs), m, n, _views_of(vis) if vis is not None else None,
                                              int(vis[0].shape[0]) if vis is not None else 0, ptr(loss), ptr(terms), ptr(state),
                                              ptr(state_ind)))
    finally:
        h.acquire(sp)                                       # the handle goes home, ordered behind the caller's stream
    return loss, terms, state, state_ind


def _prepare(zs, dt):
    return [_view_of(z if z.dtype == dt else z.to(dt)) for z in zs]


class _MomentLossFn(torch.autograd.Function):
    """One of the four moment-map losses as a two-phase autograd node: ``ccz_moment_loss_forward`` (K1, the map, the objective on
    the device, ``Gamma`` left in a state tensor with the layout of the pairwise CCA loss) and ``ccz_pair_loss_backward`` (every
    view's gradient from the views where they lie, the upstream gradient applied inside the product).  ``zs`` holds the ``m``
    representations followed by EY's independent ones (``n_ind`` of them: 0 or ``m``); gradients flow into both."""

    @staticmethod
    def forward(ctx, kind: int, params: tuple, n_ind: int, *zs: torch.Tensor) -> torch.Tensor:
        m = len(zs) - n_ind
        dt = zs[0].dtype
        vs = _prepare(zs[:m], dt)
        vis = _prepare(zs[m:], dt) if n_ind else None
        need = list(ctx.needs_input_grad[3:])
        loss, _, state, state_ind = _evaluate(kind, params, vs, vis, any(need[:m]), any(need[m:]), False)
        if state is not None or state_ind is not None:
            ctx.save_for_backward(*[t for t in (state, state_ind) if t is not None], *vs, *(vis or []))
            ctx.have = (state is not None, state_ind is not None)
            ctx.m, ctx.n_ind = m, n_ind
            ctx.dtypes = [z.dtype for z in zs]
            ctx.wanted = need
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        saved = list(ctx.saved_tensors)
        state = saved.pop(0) if ctx.have[0] else None
        state_ind = saved.pop(0) if ctx.have[1] else None
        m = ctx.m
        groups = [(saved[:m], state, ctx.wanted[:m]), (saved[m:], state_ind, ctx.wanted[m:])]
        dt = saved[0].dtype
        h = _backend.handle_for(saved[:m])
        go = grad_out.detach().to(device=saved[0].device, dtype=_loss_dtype(dt)).reshape(()).contiguous()
        code = _backend.dtype_code(dt)
        out = []
        sp = _stream_ptr(saved[0])
        for vs, st, wanted in groups:
            if st is None:
                out += [None] * len(vs)
                continue
            k = len(vs)
            grads = [torch.empty_like(v, memory_format=torch.contiguous_format) if w else None for v, w in zip(vs, wanted)]
            gp = (C.c_void_p * k)(*[g.data_ptr() if g is not None else None for g in grads])
            ldg = (C.c_int64 * k)(*[int(g.stride(0)) if g is not None else 0 for g in grads])
            h.adopt(sp)
            try:
                h.check(h.lib.ccz_pair_loss_backward(h.raw, code, _views_of(vs), k, int(vs[0].shape[0]), C.c_void_p(st.data_ptr()),
                                                     C.c_void_p(go.data_ptr()), gp, ldg))
            finally:
                h.acquire(sp)
            out += grads
        return (None, None, None, *[g if g is None else g.to(t) for g, t in zip(out, ctx.dtypes)])


class _MomentLoss(nn.Module):
    _kind = -1

    def _params(self) -> tuple:
        return ()

    def _check(self, representations, independent_representations=None):
        what = type(self).__name__
        zs = _validate(what, self._kind, representations)
        zi = None
        if independent_representations is not None:
            zi = _validate(what, self._kind, independent_representations, "independent representations", like=zs)
        for z in zs + (zi or []):
            _require_cuda(z, what)
        from cca_zoo_amd import _dist

        if _dist.is_sharded():
            raise RuntimeError(f"{what} under row_sharded() is not supported: the loss needs the moments of the whole batch")
        return zs, zi

    def _forward(self, zs, zi) -> torch.Tensor:
        return _MomentLossFn.apply(self._kind, self._params(), len(zi) if zi else 0, *zs, *(zi or []))

    def _terms(self, zs, zi) -> dict[str, torch.Tensor]:
        with torch.no_grad():
            dt = zs[0].dtype
            loss, terms, _, _ = _evaluate(self._kind, self._params(), _prepare(zs, dt), _prepare(zi, dt) if zi else None, False, False, True)
            out = {"objective": loss}
            for i, k in enumerate(_TERM_KEYS[self._kind]):
                out[k] = terms[i].to(_loss_dtype(dt))
        return out


class EYLoss(_MomentLoss):
    r"""Eckart-Young (EigenGame) objective ``-2 tr C + tr(V V_ind)`` for 2 to 8 views of one width: ``C`` the mean of ALL pairwise
    batch cross-covariances (the a = b terms included, as the reference's double loop does), ``V`` the mean within-view covariance,
    ``V_ind`` that of ``independent_representations`` (``V`` itself when none is given).  Gradients flow into both lists."""

    _kind = _EY

    def forward(self, representations: list[torch.Tensor], independent_representations: list[torch.Tensor] | None = None) -> torch.Tensor:
        return self._forward(*self._check(representations, independent_representations))

    def terms(self, representations: list[torch.Tensor], independent_representations: list[torch.Tensor] | None = None) -> dict[str, torch.Tensor]:
        """``objective``, ``rewards`` (= 2 tr C) and ``penalties`` (= tr(V V_ind))."""
        return self._terms(*self._check(representations, independent_representations))


class BarlowTwinsLoss(_MomentLoss):
    r"""Barlow Twins: ``sum_i (1 - C_ii)^2 + lam sum_{i != j} C_ij^2`` with ``C = z_1' z_2 / n`` of exactly two (batch-normalised)
    views -- raw moments, nothing is centred, as in the reference.

    Args:
        lam: weight of the redundancy term (default 5e-3).
    """

    _kind = _BARLOW

    def __init__(self, lam: float = 5e-3) -> None:
        super().__init__()
        self.lam = lam

    def _params(self) -> tuple:
        return (float(self.lam),)

    def forward(self, representations: list[torch.Tensor]) -> torch.Tensor:
        return self._forward(*self._check(representations))

    def terms(self, representations: list[torch.Tensor]) -> dict[str, torch.Tensor]:
        """``objective``, ``invariance`` and ``redundancy``."""
        return self._terms(*self._check(representations))


class VICRegLoss(_MomentLoss):
    r"""VICReg for exactly two views: ``sim_coeff mean((z_1 - z_2)^2) + std_coeff sum_a mean_j relu(1 - sqrt(var_aj + 1e-4)) +
    cov_coeff sum_a sum_{i != j} cov_a,ij^2 / d``.  More than two views are an error (the reference ignores them silently).

    Args:
        sim_coeff, std_coeff, cov_coeff: weights of the three terms (defaults 25, 25, 1).
    """

    _kind = _VICREG

    def __init__(self, sim_coeff: float = 25.0, std_coeff: float = 25.0, cov_coeff: float = 1.0) -> None:
        super().__init__()
        self.sim_coeff = sim_coeff
        self.std_coeff = std_coeff
        self.cov_coeff = cov_coeff

    def _params(self) -> tuple:
        return (float(self.sim_coeff), float(self.std_coeff), float(self.cov_coeff))

    def forward(self, representations: list[torch.Tensor]) -> torch.Tensor:
        return self._forward(*self._check(representations))

    def terms(self, representations: list[torch.Tensor]) -> dict[str, torch.Tensor]:
        """``objective``, ``sim_loss``, ``var_loss`` and ``cov_loss``."""
        return self._terms(*self._check(representations))


class SDLLoss(_MomentLoss):
    r"""Stochastic decorrelation loss for 2 to 8 views of one width d >= 2: ``mean((z_1 - z_2)^2) + lam sum_a mean |offdiag
    cov_a|`` -- the squared difference is taken between the first two views only, as in the reference.  One column per view is an
    error here (the reference returns NaN from the mean of an empty off-diagonal).

    Args:
        lam: weight of the decorrelation term (default 0.5).
    """

    _kind = _SDL

    def __init__(self, lam: float = 0.5) -> None:
        super().__init__()
        self.lam = lam

    def _params(self) -> tuple:
        return (float(self.lam),)

    def forward(self, representations: list[torch.Tensor]) -> torch.Tensor:
        return self._forward(*self._check(representations))

    def terms(self, representations: list[torch.Tensor]) -> dict[str, torch.Tensor]:
        """``objective``, ``l2`` and ``sdl``."""
        return self._terms(*self._check(representations))
