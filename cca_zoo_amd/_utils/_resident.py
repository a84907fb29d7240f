"""Views kept in HBM for the length of an iterative fit (:class:`ResidentViews`: the EY, ALS / ADMM and GFA models), the
host side of such a fit (its refusals, the fit state's bracket, the chunk loop), and the coercion, dtype probes and stream
bracket that the kernel models share with it."""

from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from cca_zoo_amd import _backend
from cca_zoo_amd._utils._validation import is_device_tensor, is_sparse_view, validate_views

#: the column means of CUDA tensors (host arrays always take NumPy's ``v.mean(axis=0)``): ``x.mean(dim=0)`` with torch on
#: the caller's stream (EY), or ``ccz_als_colmeans`` on the handle's stream in NumPy's order of summation (ALS)
MEANS_TORCH, MEANS_COLMEANS = "torch", "colmeans"


def as_float(v):
    """Floating views: float32 / float64 stay, anything else becomes float64 (as ``v - mean`` does in the reference)."""
    if is_device_tensor(v):
        return v
    return v if v.dtype in (np.float32, np.float64) else v.astype(np.float64)


def canonical_forms(v, dtype, csc=True):
    """The CSR and CSC forms of a ``scipy.sparse`` view as libccz reads them (``ccz_sparse_view``): values of ``dtype``,
    ``int32`` minor indices, ``int64`` pointers, both canonical -- indices sorted, duplicates summed, stored zeros dropped
    -- so every scipy format of the same matrix gives the same pair, and the entries of a CSC column are in ascending
    row order.  scipy's full format check (O(nnz)) runs on what the caller passed before anything is rearranged: the
    kernels trust the indices, so a malformed matrix raises ``ValueError`` here, before the device is touched.
    ``csc=False`` (the projection reads rows only) returns ``None`` for that form."""
    if v.format in ("csr", "csc", "bsr"):
        v.check_format(full_check=True)
    elif v.format == "coo" and v.nnz:
        n, p = v.shape
        if min(v.row.min(), v.col.min()) < 0 or v.row.max() >= n or v.col.max() >= p:
            raise ValueError("sparse view: a COO index is out of range")
    csr = v.tocsr()
    csr.check_format(full_check=True)
    csr = csr.astype(dtype, copy=True)       # never the caller's own arrays: the next three calls work in place
    csr.sum_duplicates()
    csr.eliminate_zeros()
    csr.sort_indices()
    if max(csr.shape) >= 2 ** 31 or csr.nnz >= 2 ** 31:
        raise ValueError("sparse views are limited to fewer than 2^31 rows, columns and stored entries")
    forms = [csr]
    if csc:
        forms.append(csr.tocsc())
        forms[1].sort_indices()
    for f in forms:
        f.indices = np.ascontiguousarray(f.indices, dtype=np.int32)
        f.indptr = np.ascontiguousarray(f.indptr, dtype=np.int64)
    return csr, (forms[1] if csc else None)


def sparse_group(nnz, lines):
    """Lanes per line of the sparse kernels (``ccz_sparse_group``): the smallest power of two that is not below the mean
    number of stored entries per line, within [4, 64]."""
    return int(_backend.library().ccz_sparse_group(int(nnz), int(lines)))


class DeviceSparse:
    """Both forms of one sparse view in HBM for as long as this object lives; ``view`` is its ``ccz_sparse_view``."""

    def __init__(self, h, csr, csc=None):
        forms = [csr] + ([csc] if csc is not None else [])
        self._keep = [[h.to_device(a) for a in (f.data, f.indices, f.indptr)] for f in forms]
        self.view = sv = _backend.SparseView()
        sv.csr_val, sv.csr_col, sv.csr_ptr = (b.ptr for b in self._keep[0])
        if csc is not None:
            sv.csc_val, sv.csc_row, sv.csc_ptr = (b.ptr for b in self._keep[1])
        sv.rows, sv.cols, sv.nnz = int(csr.shape[0]), int(csr.shape[1]), int(csr.nnz)


def is_f32(v):
    return v.element_size() == 4 if is_device_tensor(v) else v.dtype == np.float32     # host arrays and sparse views


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

    With ``allow_sparse`` (the four plain ALS models) any subset of HOST views may be ``scipy.sparse`` matrices or arrays:
    ``sparse[i]`` says which, ``sarr[i]`` holds such a view's two device forms after entering, its means are float64
    (``ccz_sparse_colmeans``) and ``f32`` counts its values like a dense view's elements.

    The constructor validates (no device work): non-float host arrays become float64, mixed host / CUDA views are
    refused, and ``n``, ``p``, ``f32`` (only if every view is 4-byte) and ``code`` are known.  Entering makes the rows
    contiguous (a row stride above the width is kept), checks host arrays for non-finite values and uploads them, forms
    the means when ``center`` and fills ``varr`` (a ``View`` per view) and ``marr`` (means pointers; ``None`` without
    centring).  For CUDA tensors the handle's stream is acquired last, after every conversion is enqueued on the
    caller's; leaving releases it on every path.  Every tensor and buffer stays referenced as long as this object does.
    """

    def __init__(self, views, center, device_means, handle=None, allow_sparse=False):
        if device_means not in (MEANS_TORCH, MEANS_COLMEANS):
            raise ValueError(f"unknown means policy {device_means!r}")
        self.views = [as_float(v) for v in validate_views(views, check_finite=False, allow_sparse=allow_sparse)]
        dev = [is_device_tensor(v) for v in self.views]
        if any(dev) and not all(dev):
            raise ValueError("views must be all host arrays or all CUDA tensors")
        self.on_device, self.center, self.device_means, self.handle = all(dev), bool(center), device_means, handle
        self.n = int(self.views[0].shape[0])
        self.p = [int(v.shape[1]) for v in self.views]
        self.f32 = all(is_f32(v) for v in self.views)
        self.code = _backend.F32 if self.f32 else _backend.F64
        self.sparse = [is_sparse_view(v) for v in self.views]
        self.sarr = [None] * len(self.views)
        vdt = np.float32 if self.f32 else np.float64
        # canonical forms and scipy's full format check now: a malformed matrix raises before the device is touched
        self._forms = [canonical_forms(v, vdt) if s else None for v, s in zip(self.views, self.sparse)]
        self.varr = self.marr = self._keep = self._sp = self._mbufs = None
        self._mus = []

    def __enter__(self):
        h = self.handle = self.handle if self.handle is not None else _backend.handle_for(self.views)
        m = len(self.views)
        xs = [v if s else as_dtype(v, self.code) for v, s in zip(self.views, self.sparse)]
        if any(self.sparse):
            return self._enter_sparse(h, xs)
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

    def _enter_sparse(self, h, xs):
        """Host views of which some are sparse: a dense view as in the all-dense case (its means NumPy's, in its own
        dtype); a sparse view as both canonical forms (:class:`DeviceSparse`), its means float64 from
        ``ccz_sparse_colmeans``, its ``varr`` entry without data."""
        m = len(xs)
        xs = [x if s else np.ascontiguousarray(x) for x, s in zip(xs, self.sparse)]
        if not all(np.all(np.isfinite(x)) for x, s in zip(xs, self.sparse) if not s):
            raise ValueError("Input contains NaN or infinity.")
        self.sarr = [DeviceSparse(h, *f) if s else None for f, s in zip(self._forms, self.sparse)]
        self._forms = None                       # the host copies of the two forms have served
        bufs = [None if s else h.to_device(x) for x, s in zip(xs, self.sparse)]
        self._mus, mbufs = [None] * m, [None] * m
        if self.center:
            for i, (x, s) in enumerate(zip(xs, self.sparse)):
                if s:
                    mbufs[i] = h.alloc(self.p[i] * 8)
                    h.check(h.lib.ccz_sparse_colmeans(h.raw, self.code, C.byref(self.sarr[i].view), C.c_void_p(mbufs[i].ptr)))
                else:
                    self._mus[i] = x.mean(axis=0)
                    mbufs[i] = h.to_device(self._mus[i])
        self._keep, self._mbufs = bufs, mbufs
        self.varr = (_backend.View * m)()
        for i, pi in enumerate(self.p):
            self.varr[i].data, self.varr[i].cols, self.varr[i].ld = (None if self.sparse[i] else int(bufs[i].ptr)), pi, pi
        self.marr = (C.c_void_p * m)(*[int(b.ptr) for b in mbufs]) if self.center else None
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
        if any(self.sparse):
            return [self.handle.to_host(b, (pi,)) if s else mu
                    for b, mu, s, pi in zip(self._mbufs, self._mus, self.sparse, self.p)]
        return [mu.detach().cpu().numpy() for mu in self._mus] if self.on_device else list(self._mus)
