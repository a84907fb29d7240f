"""Views kept in HBM for the length of an iterative fit (:class:`ResidentViews`: the EY, ALS / ADMM and GFA models), the
host side of such a fit (its refusals, the fit state's bracket, the chunk loop), and the coercion, dtype probes and stream
bracket that the kernel models share with it."""

from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from cca_zoo_amd import _backend
from cca_zoo_amd._utils._validation import is_device_tensor, validate_views

#: the column means of CUDA tensors (host arrays always take NumPy's ``v.mean(axis=0)``): ``x.mean(dim=0)`` with torch on
#: the caller's stream (EY), or ``ccz_als_colmeans`` on the handle's stream in NumPy's order of summation (ALS)
MEANS_TORCH, MEANS_COLMEANS = "torch", "colmeans"


def as_float(v):
    """Floating views: float32 / float64 stay, anything else becomes float64 (as ``v - mean`` does in the reference)."""
    if is_device_tensor(v):
        return v
    return v if v.dtype in (np.float32, np.float64) else v.astype(np.float64)


def is_f32(v):
    return v.element_size() == 4 if is_device_tensor(v) else v.dtype == np.float32


def as_dtype(v, code):
    if is_device_tensor(v):
        import torch

        return v.to(torch.float32 if code == _backend.F32 else torch.float64)
    return np.asarray(v, dtype=np.float32 if code == _backend.F32 else np.float64)


def acquire(h, views):
    """Device tensors: the handle's stream waits for the caller's current stream (no host wait).  Returns what
    :func:`release` takes (``None`` for host arrays)."""
    if views and is_device_tensor(views[0]):
        import torch

        sp = int(torch.cuda.current_stream(views[0].device).cuda_stream)
        h.acquire(sp)
        return sp
    return None


def release(h, sp):
    if sp is not None:
        h.release(sp)


def refuse_row_sharded(why):
    """Raise inside ``row_sharded()``; ``why`` names the model and what keeps it from sharding by rows."""
    from cca_zoo_amd import _dist

    if _dist.is_sharded():
        raise NotImplementedError(f"{why}: fit it outside row_sharded()")


def check_limits(k, m, max_dims, max_views):
    if k > max_dims:
        raise ValueError(f"latent_dimensions={k}: the device path supports at most {max_dims}")
    if m > max_views:
        raise ValueError(f"{m} views: the device path supports at most {max_views} views")


@contextlib.contextmanager
def fit_state(h, family, *args):
    """The fit state of ``family`` ("ey", "als", "gfa") for the length of a ``with`` block: ``ccz_<family>_create(handle,
    *args, &state)`` makes it (a refused create raises and leaves nothing behind), ``ccz_<family>_destroy`` frees it on
    every path."""
    state = C.c_void_p()
    h.check(getattr(h.lib, f"ccz_{family}_create")(h.raw, *args, C.byref(state)))
    try:
        yield state
    finally:
        getattr(h.lib, f"ccz_{family}_destroy")(h.raw, state)


def run_chunks(total, chunk, call):
    """Enqueue ``total`` steps in chunks of at most ``chunk``.  ``call(step)`` enqueues one chunk and returns the stop flag
    it was told (that of the chunk two calls back); no chunk follows a reported stop."""
    done, stopped = 0, False
    while done < total and not stopped:
        step = min(chunk, total - done)
        stopped = bool(call(step))
        done += step


class ResidentViews:
    """The views of one fit as libccz reads them, in one dtype, for the length of a ``with`` block.

    The constructor validates (no device work): non-float host arrays become float64, mixed host / CUDA views are
    refused, and ``n``, ``p``, ``f32`` (only if every view is 4-byte) and ``code`` are known.  Entering makes the rows
    contiguous (a row stride above the width is kept), checks host arrays for non-finite values and uploads them, forms
    the means when ``center`` and fills ``varr`` (a ``View`` per view) and ``marr`` (means pointers; ``None`` without
    centring).  For CUDA tensors the handle's stream is acquired last, after every conversion is enqueued on the
    caller's; leaving releases it on every path.  Every tensor and buffer stays referenced as long as this object does.
    """

    def __init__(self, views, center, device_means, handle=None):
        if device_means not in (MEANS_TORCH, MEANS_COLMEANS):
            raise ValueError(f"unknown means policy {device_means!r}")
        self.views = [as_float(v) for v in validate_views(views, check_finite=False)]
        dev = [is_device_tensor(v) for v in self.views]
        if any(dev) and not all(dev):
            raise ValueError("views must be all host arrays or all CUDA tensors")
        self.on_device, self.center, self.device_means, self.handle = all(dev), bool(center), device_means, handle
        self.n = int(self.views[0].shape[0])
        self.p = [int(v.shape[1]) for v in self.views]
        self.f32 = all(is_f32(v) for v in self.views)
        self.code = _backend.F32 if self.f32 else _backend.F64
        self.varr = self.marr = self._keep = self._sp = None
        self._mus = []

    def __enter__(self):
        h = self.handle = self.handle if self.handle is not None else _backend.handle_for(self.views)
        m = len(self.views)
        xs = [as_dtype(v, self.code) for v in self.views]
        if self.on_device:
            import torch

            xs = [x if (x.stride(1) == 1 and x.stride(0) >= x.shape[1]) else x.contiguous() for x in xs]
            if self.center and self.device_means == MEANS_TORCH:
                self._mus = [x.mean(dim=0) for x in xs]
            elif self.center:
                self._mus = [torch.empty(pi, dtype=x.dtype, device=x.device) for x, pi in zip(xs, self.p)]
            self._keep = xs
            ptrs = [(int(x.data_ptr()), int(x.stride(0))) for x in xs]
            mptrs = [int(mu.data_ptr()) for mu in self._mus]
        else:
            xs = [np.ascontiguousarray(x) for x in xs]
            if not all(np.all(np.isfinite(x)) for x in xs):
                raise ValueError("Input contains NaN or infinity.")
            if self.center:     # the reference's _setup_fit: v.mean(axis=0) in the input dtype
                self._mus = [x.mean(axis=0) for x in xs]
            self._keep = [h.to_device(a) for a in xs + self._mus]
            ptrs = [(int(b.ptr), pi) for b, pi in zip(self._keep, self.p)]
            mptrs = [int(b.ptr) for b in self._keep[m:]]
        self.varr = (_backend.View * m)()
        for i, ((ptr, ld), pi) in enumerate(zip(ptrs, self.p)):
            self.varr[i].data, self.varr[i].cols, self.varr[i].ld = ptr, pi, ld
        self.marr = (C.c_void_p * m)(*mptrs) if self.center else None
        self._sp = acquire(h, self.views)
        if self._sp is not None and self.center and self.device_means == MEANS_COLMEANS:
            try:
                for v, mp in zip(self.varr, mptrs):
                    h.check(h.lib.ccz_als_colmeans(h.raw, self.code, C.byref(v), self.n, C.c_void_p(mp)))
            except BaseException:
                self.__exit__()
                raise
        return self

    def __exit__(self, *exc):
        sp, self._sp = self._sp, None
        release(self.handle, sp)

    def means_host(self):
        """The means as host arrays in the views' dtype (float64 zeros without centring), after the block: means formed
        on the handle's stream are ordered before the caller's stream only once it is released."""
        if self._sp is not None:
            raise RuntimeError("means_host() inside the block: the handle's stream still holds the means")
        if not self.center:
            return [np.zeros(pi) for pi in self.p]
        return [mu.detach().cpu().numpy() for mu in self._mus] if self.on_device else list(self._mus)
