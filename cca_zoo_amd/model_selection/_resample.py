"""The host half of what :func:`permutation_test` and :func:`bootstrap` share (the device half is ``csrc/resample_dev.h``): the
checks before the device is touched, the float64 staging, and the loop that draws one chunk of resamples ahead of the device,
the arrangement of the EY models' mini-batch indices (``linear/gradient/_base.py``) -- or, with ``draws="device"``, has the
device draw each chunk itself (``csrc/draw.hip``), in the same loop.
"""

from __future__ import annotations

import numpy as np

from cca_zoo_amd._utils._resident import as_float, refuse_row_sharded
from cca_zoo_amd._utils._validation import is_device_tensor, is_sparse_view, perview_parameter, validate_views

#: limits of the device path (``include/ccz.h``: CCZ_PERM_MAXP, CCZ_PERM_ROWS).  ``ROWS_PER_SPLIT`` rows of one resample go to
#: one workgroup of the block product: the row split is a function of ``n`` alone
MAX_WIDTH = 64
ROWS_PER_SPLIT = 4096
MAX_ROWS = 2 ** 31
#: where a resample is drawn: by NumPy on the host, one chunk ahead of the device, or by ``csrc/draw.hip`` in the slot itself
DRAWS = ("numpy", "device")


def is_half(v):
    if type(v).__module__.startswith("torch"):
        return bool(v.dtype.is_floating_point) and v.element_size() == 2
    return getattr(getattr(v, "dtype", None), "itemsize", 0) == 2 and getattr(v.dtype, "kind", "") == "f"


def check_shape(name, n, p, advice=""):
    """``ValueError`` for the widths and row counts the device path excludes; ``advice`` ends the sentence on wider views."""
    if max(p) > MAX_WIDTH:
        raise ValueError(f"{name}: views of at most {MAX_WIDTH} columns are supported, got {list(p)}; reduce wider "
                         f"views first (e.g. to their leading principal components){advice}")
    if n >= MAX_ROWS:
        raise ValueError(f"{name}: fewer than 2^31 rows are supported, got {n}")
    if n - 1 <= 0:
        raise ValueError("at least 2 samples are required")


def device_seed(random_state):
    """The 64-bit seed of the device draws: one rule for ``None``, ints, ``SeedSequence`` s and ``Generator`` s."""
    return int(np.random.default_rng(random_state).integers(0, 2 ** 64, dtype=np.uint64))


def prepare(name, one_device, estimator, views, check, draws="numpy"):
    """Every refusal that needs no device, in a fixed order; ``check(n, p)`` is the caller's own (its counts and levels, then
    :func:`check_shape`).  Returns ``est, views_, n, p, c_, center, on_device``: ``est`` is a validated clone."""
    from sklearn.base import clone

    from cca_zoo_amd.linear import rCCA

    if not isinstance(estimator, rCCA):
        raise TypeError(f"{name} takes a CCA, rCCA or PLS estimator, got {type(estimator).__name__}")
    refuse_row_sharded(f"{name} {one_device}, which this build does not shard by rows")
    if not isinstance(views, (list, tuple)):
        raise TypeError("views must be a list of two arrays or CUDA tensors")
    for v in views:
        if is_sparse_view(v):
            raise TypeError(f"{name}: sparse views are not supported; pass dense arrays")
        if is_half(v):
            raise TypeError(f"{name}: half-precision views are not supported; pass float32 or float64")
    if not (isinstance(draws, str) and draws in DRAWS):
        raise ValueError(f"{name}: draws must be one of {list(DRAWS)}, got {draws!r}")
    est = clone(estimator)
    est._validate_params()
    views_ = [as_float(v) for v in validate_views(list(views), check_finite=False)]
    if len(views_) != 2:
        raise ValueError(f"{name} requires exactly 2 views, got {len(views_)}")
    n, p = int(views_[0].shape[0]), [int(v.shape[1]) for v in views_]
    check(n, p)
    dev = [is_device_tensor(v) for v in views_]
    if any(dev) and not all(dev):
        raise ValueError("views must be all host arrays or all CUDA tensors")
    c_ = [float(v) for v in perview_parameter("c", est.c, 0.0, 2)]
    return est, views_, n, p, c_, bool(est.center), all(dev)


def stage_f64(h, views_, on_device):
    """``(owners, pointers)`` of float64 device copies of the views, made before the handle's stream takes over (CUDA: on the
    caller's stream)."""
    if on_device:
        import torch

        x64 = [v.to(torch.float64).contiguous() for v in views_]
        return x64, [int(x.data_ptr()) for x in x64]
    x64 = [h.to_device(np.ascontiguousarray(v, dtype=np.float64)) for v in views_]
    return x64, [int(b.ptr) for b in x64]


def chunk_length(n, per_call, byte_cap):
    """Resamples per upload: ``per_call``, fewer when their ``n`` int32 each would exceed ``byte_cap``."""
    return max(1, min(int(per_call), byte_cap // (4 * n)))


def chunks(draw, rng, n, total, chunk):
    """The ``total`` resamples of ``draw(rng, n, count)`` in chunks of at most ``chunk``, drawn as they are asked for."""
    done = 0
    while done < total:
        step = min(int(chunk), total - done)
        yield draw(rng, n, step)
        done += step


def device_chunks(h, what, n, seed, total, chunk):
    """The ``total`` resamples of ``csrc/draw.hip`` in chunks of at most ``chunk``, as device producers ``(count, write)``:
    ``write(ptr)`` enqueues the draw of resamples ``[done, done + count)`` into ``ptr``.  ``what``: ``"permutations"`` (row
    ``b`` = the argsort of stream ``b``'s keys) or ``"counts"`` (row ``b`` = the multiplicities of stream ``b``'s ``n`` draws);
    a row is a function of ``(seed, b, n)`` only, so the chunk length does not change a bit."""
    import ctypes as C

    def write(ptr, count, first):
        if what == "permutations":
            h.check(h.lib.ccz_draw_permutations(h.raw, int(n), count, seed, first, 0, C.c_void_p(int(ptr))))
        else:
            h.check(h.lib.ccz_draw_counts(h.raw, int(n), count, seed, first, C.c_void_p(int(ptr))))

    done = 0
    while done < total:
        step = min(int(chunk), total - done)
        yield step, (lambda ptr, step=step, done=done: write(ptr, step, done))
        done += step


def run_chunks(h, chunks, slot_bytes, call):
    """``call(ptr, count, done)`` for every chunk, in one of two slots of ``slot_bytes``.  A host chunk (an array of
    :func:`chunks`) is uploaded: the next one is drawn while the device works on this one, and its upload is ordered behind that
    work on the handle's stream.  A device chunk (``(count, write)`` of :func:`device_chunks`) is drawn into the slot by
    ``write(ptr)``, in stream order, and nothing is built or uploaded by the host.  Returns the slots, which the caller keeps
    until it has read the results."""
    slots = [h.alloc(slot_bytes) for _ in range(2)]
    done = 0
    for i, block in enumerate(chunks):
        slot = slots[i & 1]
        if isinstance(block, np.ndarray):
            count = block.shape[0]
            h.h2d(slot.ptr, block)
        else:
            count, write = block
            write(slot.ptr)
        call(slot.ptr, count, done)
        done += count
    return slots
