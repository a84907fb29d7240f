"""View validation -- the boundary semantics of cca_zoo/_utils/_validation.py:14-75.

Besides array-likes (validated with sklearn ``check_array(dtype="numeric")``, which
preserves float32 exactly like the reference), views may be **torch CUDA tensors**:
those stay in HBM and are handed to libccz by pointer (no host round trip).
"""

from __future__ import annotations

from typing import Any

import numpy as np
from sklearn.utils.validation import check_array


def is_device_tensor(v: Any) -> bool:
    return type(v).__module__.startswith("torch") and hasattr(v, "is_cuda") and bool(v.is_cuda)


def _n_rows(v) -> int:
    return int(v.shape[0])


def is_bf16_tensor(v: Any) -> bool:
    """A CUDA tensor of ``torch.bfloat16`` (the only 2-byte view format the closed-form estimators take)."""
    return is_device_tensor(v) and str(v.dtype) == "torch.bfloat16"


def is_sparse_view(v: Any) -> bool:
    """A ``scipy.sparse`` matrix or array of any format (never a torch sparse tensor)."""
    return type(v).__module__.startswith("scipy.sparse") and hasattr(v, "tocsr")


def _stored_values(v) -> np.ndarray:
    """The stored entries of a sparse view as one array (formats without a flat ``data`` go through COO)."""
    return v.data if v.format in ("csr", "csc", "coo", "bsr", "dia") else v.tocoo().data


def _validate_sparse(v):
    """The host-side checks of one sparse view, format untouched: 2-D, a real numeric dtype (anything but float32 /
    float64 becomes float64), no NaN or infinity among the stored entries."""
    if v.ndim != 2:
        raise ValueError(f"Expected 2D sparse view, got {v.ndim}D instead.")
    if v.dtype.kind not in "buif":
        raise ValueError(f"sparse views must have a real numeric dtype, got {v.dtype}")
    if v.dtype not in (np.float32, np.float64):
        v = v.astype(np.float64)
    if not np.all(np.isfinite(_stored_values(v))):
        raise ValueError("Input contains NaN or infinity.")
    return v


def validate_views(views, min_views: int = 2, check_finite: bool = True, allow_bf16: bool = False,
                   allow_sparse: bool = False) -> list:
    """Return the views as 2-D numpy arrays (or untouched 2-D CUDA tensors).

    ``allow_sparse`` (the four plain ALS models only: PLS_ALS, SCCA_PMD, ParkhomenkoCCA, SCCA_Span, and ``transform`` of
    a model fitted on sparse views) lets ``scipy.sparse`` matrices and arrays of any format pass in their own format;
    their stored entries are always checked for NaN / infinity (a pass over nnz numbers).  Without it they fail as any
    other unsupported input does (sklearn's ``TypeError``).

    ``allow_bf16`` (the closed-form family only: rCCA / CCA / PLS, MCCA, GCCA, PartialCCA, GRCCA and the grid search over
    them) lets 2-D ``torch.bfloat16`` CUDA tensors pass as they lie; ``float16`` device views are refused either way.

    ``check_finite=False`` skips sklearn's host-side NaN/inf scan (a single-threaded pass over the
    whole input, 0.2 s per 4 GB): ``fit`` detects non-finite inputs for free from the column sums of
    the moments pass and ``transform`` from its n x k output, raising the same ``ValueError``.

    Raises:
        ValueError: fewer than ``min_views`` views, or unequal numbers of samples.
    """
    if len(views) < min_views:
        raise ValueError(f"At least {min_views} views are required, got {len(views)}.")
    out = []
    for v in views:
        if is_device_tensor(v):
            if v.dim() != 2:
                raise ValueError(f"Expected 2D tensor, got {v.dim()}D tensor instead.")
            if allow_bf16 and is_bf16_tensor(v):
                pass
            elif not v.dtype.is_floating_point or v.element_size() not in (4, 8):
                raise ValueError("device views must be float32 or float64 tensors" + (" (or bfloat16)" if allow_bf16 else ""))
            out.append(v)
        elif allow_sparse and is_sparse_view(v):
            out.append(_validate_sparse(v))
        else:
            if type(v).__module__.startswith("torch"):
                v = v.detach().cpu().numpy()
            out.append(check_array(v, ensure_2d=True, allow_nd=False, dtype="numeric", ensure_all_finite=check_finite))
    n = _n_rows(out[0])
    if not all(_n_rows(v) == n for v in out):
        raise ValueError(
            "All views must have the same number of samples. "
            f"Got shapes: {[tuple(v.shape) for v in out]}."
        )
    return out


def perview_parameter(name: str, value, default, n_views: int) -> list:
    """One value per view: a list is taken as is (its length must be ``n_views``), a scalar is repeated and
    ``None`` stands for ``default`` (semantics and message of cca_zoo/_utils/_validation.py:45-75)."""
    if not isinstance(value, list):
        fill = default if value is None else value
        return [fill for _ in range(n_views)]
    if len(value) == n_views:
        return value
    raise ValueError(f"Parameter '{name}' must be a scalar or a list of length {n_views}, got length {len(value)}.")
