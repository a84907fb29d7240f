"""TreeCCA -- gradient-boosted-tree CCA: the reference's outer loop around a built-in histogram booster, whole rounds on the
device.

Reference: ``cca_zoo/tree/_treecca.py``.  The reference boosts with xgboost or lightgbm; neither is a dependency here.  The
booster is this project's own (``backend="hist"``, ``csrc/tree.hip``): xgboost's documented ``tree_method="hist"`` regression
tree for the parameters the reference passes, specified in ``tests/treecca_restatement.py`` -- 256 quantile bins per feature,
gradients in fixed point so that every node sum is an exact integer, the gain in float64 with every operation rounded once,
ties to the lowest feature and then the lowest bin.  A tree is therefore a deterministic function of its inputs; it is not
xgboost's tree.  Row and feature samples are pure functions of a splitmix64 hash of ``(random_state, round, view, index)``.

The host draws the random-orthogonal start (``np.random.default_rng(random_state)`` and a QR, ``p x k``), the cut sample
and the feature lists; bins, base margin, the EY gradient, the rescale, tree growth and the embedding update run on the
device as one chain of launches per round, enqueued in chunks behind a device status word.
"""

from __future__ import annotations

import ctypes as C
from numbers import Integral, Real
from typing import Any, ClassVar

import numpy as np
from sklearn.utils._param_validation import Interval
from sklearn.utils.validation import check_is_fitted

from cca_zoo_amd import _backend
from cca_zoo_amd._base import BaseModel
from cca_zoo_amd._utils._param_constraints import POSITIVE_EPS, POSITIVE_INT
from cca_zoo_amd._utils._resident import MEANS_COLMEANS, ResidentViews, fit_state, refuse_row_sharded, run_chunks
from cca_zoo_amd._utils._validation import is_device_tensor, validate_views

#: rounds per ``ccz_tree_rounds`` call
CHUNK_ROUNDS = 4
#: limits of the device path (``csrc/tree.hip``): uint8 node ids, one workgroup's tables, the grid's second dimension
MAX_DEPTH, MAX_DIMS, MAX_VIEWS, MAX_FEATURES, MAX_ROWS = 8, 32, 8, 32768, (1 << 31) - 1
#: the histogram workspace of one level (bytes): the features of a level are tiled to stay inside it
HIST_BYTES = 64 << 20
CUT_SAMPLE = 8192
_CUT_TAG = 1 << 63
_M64 = (1 << 64) - 1


def _splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def hash_keys(seed, tag, count):
    """``splitmix64(splitmix64(seed ^ splitmix64(tag)) ^ splitmix64(i))`` for i < count (``csrc/rng_hash.h``)."""
    stream = _splitmix64(np.uint64(int(seed) & _M64) ^ _splitmix64(np.uint64(int(tag) & _M64)))
    return _splitmix64(stream ^ _splitmix64(np.arange(count, dtype=np.uint64)))


def cut_sample_rows(n, seed):
    """The rows the cut points are taken from: all up to 8192, else those with the 8192 smallest keys."""
    if n <= CUT_SAMPLE:
        return np.arange(n, dtype=np.int64)
    return np.sort(np.argsort(hash_keys(seed, _CUT_TAG, n), kind="stable")[:CUT_SAMPLE]).astype(np.int64)


def feature_list(seed, rnd, view, p, colsample):
    """The ascending features of the trees of (round, view): the ``max(1, floor(colsample p))`` smallest keys."""
    nsel = max(1, int(np.floor(float(colsample) * p)))
    return np.sort(np.argsort(hash_keys(seed, 2 * (64 * rnd + view) + 1, p), kind="stable")[:nsel]).astype(np.int32)


def check_limits(n, dims, k, depth):
    """``ValueError`` for what the device path excludes, before the device is touched."""
    if depth > MAX_DEPTH:
        raise ValueError(f"TreeCCA: max_depth={depth} exceeds the device path's limit of {MAX_DEPTH} (uint8 node ids)")
    if k > min(dims):
        raise ValueError(f"TreeCCA: latent_dimensions={k} exceeds the {min(dims)} features of the narrowest view")
    if k > MAX_DIMS:
        raise ValueError(f"TreeCCA: latent_dimensions={k}: the device path supports at most {MAX_DIMS}")
    if len(dims) > MAX_VIEWS:
        raise ValueError(f"TreeCCA: {len(dims)} views: the device path supports at most {MAX_VIEWS}")
    if max(dims) > MAX_FEATURES:
        raise ValueError(f"TreeCCA: a view has {max(dims)} features, the device path supports at most {MAX_FEATURES}")
    if n < 2 or n > MAX_ROWS:
        raise ValueError(f"TreeCCA: {n} rows: the device path supports 2 to {MAX_ROWS}")
    # the histogram of one feature at the deepest level must fit the workspace (it does for every k and depth allowed
    # above: 32 * 128 * 256 * 12 B = 12 MiB; kept as a check because the two limits are set independently)
    if k * (1 << (depth - 1)) * 256 * 12 > HIST_BYTES:
        raise ValueError("TreeCCA: one feature's histogram of the deepest level exceeds the 64 MiB workspace")


def _device_args(h, v, mean):
    """(dtype code, View, mean pointer or None, what to keep alive) of one view and its mean in their common dtype."""
    f32 = (v.element_size() == 4 if is_device_tensor(v) else v.dtype == np.float32) and (mean is None or mean.dtype == np.float32)
    view = _backend.View()
    keep = []
    if is_device_tensor(v):
        import torch

        x = v.to(torch.float32 if f32 else torch.float64)
        if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
            x = x.contiguous()
        view.data, view.cols, view.ld = x.data_ptr(), int(x.shape[1]), int(x.stride(0))
        keep.append(x)
        mptr = None
        if mean is not None:
            md = torch.as_tensor(np.ascontiguousarray(mean, dtype=np.float32 if f32 else np.float64), device=v.device)
            keep.append(md)
            mptr = md.data_ptr()
    else:
        x = np.ascontiguousarray(v, dtype=np.float32 if f32 else np.float64)
        xb = h.to_device(x)
        view.data, view.cols, view.ld = xb.ptr, int(x.shape[1]), int(x.shape[1])
        keep.append(xb)
        mptr = None
        if mean is not None:
            mb = h.to_device(np.ascontiguousarray(mean, dtype=x.dtype))
            keep.append(mb)
            mptr = mb.ptr
    return (_backend.F32 if f32 else _backend.F64), view, mptr, keep


def predict_device(v, mean, proj, feature, threshold, leaf, max_depth):
    """``(v - mean) @ proj`` (``proj`` None: 0) plus the float32 leaves of the trees (``[n_trees][k][nodes]`` host arrays)
    summed in tree order, float64 ``n x k``: a NumPy array for a host view, a CUDA tensor for a CUDA tensor."""
    n_trees, k = int(feature.shape[0]), int(feature.shape[1])
    n = int(v.shape[0])
    h = _backend.handle_for([v])
    on_device = is_device_tensor(v)
    sp = None
    if on_device:
        import torch

        out = torch.empty((n, k), dtype=torch.float64, device=v.device)
        code, view, mptr, keep = _device_args(h, v, mean)
        sp = int(torch.cuda.current_stream(v.device).cuda_stream)
        h.acquire(sp)
        optr = out.data_ptr()
    else:
        code, view, mptr, keep = _device_args(h, v, mean)
        ob = h.alloc(max(n * k * 8, 8))
        optr = ob.ptr
    try:
        fd = h.to_device(np.ascontiguousarray(feature, dtype=np.int32))
        td = h.to_device(np.ascontiguousarray(threshold, dtype=np.float32))
        ld = h.to_device(np.ascontiguousarray(leaf, dtype=np.float32))
        pd = h.to_device(np.ascontiguousarray(proj, dtype=np.float64)) if proj is not None else None
        vp = C.c_void_p
        h.check(h.lib.ccz_tree_predict(h.raw, code, C.byref(view), n, vp(mptr) if mptr else None, vp(pd.ptr) if pd is not None else None, k,
                                       n_trees, int(max_depth), vp(fd.ptr), vp(td.ptr), vp(ld.ptr), vp(optr), k))
        if on_device:
            h.sync()               # the tree tables uploaded above are freed on return
            return out
        z = h.to_host(ob, (n, k))
    finally:
        if sp is not None:
            h.release(sp)
        del keep
    if not np.all(np.isfinite(z)):
        raise ValueError("Input contains NaN or infinity.")
    return z


class TreeBooster:
    """The trees of one latent component of one view, in the order the rounds added them: host arrays of shape
    ``(n_trees, 2^(max_depth + 1) - 1)`` in heap order (children of node i: 2 i + 1 and 2 i + 2) -- ``feature`` (-1: not a
    split), ``bin``, ``threshold`` (float32), ``leaf`` (float32; 0 on a split) and ``gain`` (float64; 0 on a leaf)."""

    def __init__(self, feature, bin, threshold, leaf, gain, max_depth, n_features):
        self.feature = np.ascontiguousarray(feature, dtype=np.int32)
        self.bin = np.ascontiguousarray(bin, dtype=np.int32)
        self.threshold = np.ascontiguousarray(threshold, dtype=np.float32)
        self.leaf = np.ascontiguousarray(leaf, dtype=np.float32)
        self.gain = np.ascontiguousarray(gain, dtype=np.float64)
        self.max_depth = int(max_depth)
        self.n_features = int(n_features)

    @property
    def n_trees(self):
        return int(self.feature.shape[0])

    def predict(self, X):
        """The raw sum of the tree outputs (float32, no base margin) for the rows of ``X`` as the trees were grown on them
        (centred, if the model centres): a traversal on the device, left iff ``float32(x) < threshold``."""
        X = validate_views([X], min_views=1, check_finite=False)[0]
        if int(X.shape[1]) != self.n_features:
            raise ValueError(f"X has {int(X.shape[1])} features, the booster was grown on {self.n_features}")
        z = predict_device(X, None, None, self.feature[:, None, :], self.threshold[:, None, :], self.leaf[:, None, :], self.max_depth)
        if is_device_tensor(z):
            import torch

            return z[:, 0].to(torch.float32)
        return z[:, 0].astype(np.float32)

    def get_score(self, importance_type="weight"):
        """xgboost's feature importances from the stored per-split gains: ``"weight"`` (number of splits on the feature),
        ``"total_gain"`` and ``"gain"`` (its mean per split), keyed ``f<index>``; features never split on are absent."""
        if importance_type not in ("weight", "gain", "total_gain"):
            raise ValueError(f"importance_type must be 'weight', 'gain' or 'total_gain' (cover statistics are not stored), "
                             f"got {importance_type!r}")
        split = self.feature >= 0
        feats = self.feature[split]
        count = np.bincount(feats, minlength=self.n_features)
        total = np.bincount(feats, weights=self.gain[split], minlength=self.n_features)
        out = {}
        for f in np.nonzero(count)[0]:
            if importance_type == "weight":
                out[f"f{f}"] = int(count[f])
            elif importance_type == "total_gain":
                out[f"f{f}"] = float(total[f])
            else:
                out[f"f{f}"] = float(total[f] / count[f])
        return out

    def __repr__(self):
        return f"TreeBooster(n_trees={self.n_trees}, max_depth={self.max_depth}, n_features={self.n_features})"


class TreeCCA(BaseModel):
    r"""Nonlinear multiview CCA with gradient-boosted-tree encoders (Chapman 2026, arXiv:2607.27027).

    One boosted-tree ensemble per view and latent dimension is fit to the Eckart-Young objective
    :math:`-2 \operatorname{tr}(C) + \operatorname{tr}(V V)` by alternating gradient boosting: every round, for every view in
    turn, one tree is added to each of its ``latent_dimensions`` boosters on the EY gradient of the embeddings (rescaled to
    standard deviation 0.1 with one scalar shared by the views), and with ``gauss_seidel=True`` the gradient is recomputed
    from the freshest embeddings before the next view.  Training starts from a random-orthogonal unit-variance embedding.

    Fitted attributes: ``boosters_[view][component]`` (:class:`TreeBooster`), ``means_``, ``embeddings_`` (not in the
    reference: the training embeddings the fit ended with, float64 host arrays), ``n_views_``, ``n_features_in_``,
    ``n_samples_``.

    Differences from the reference, on purpose:

    - ``backend="hist"`` (the default and the only one) is this project's device booster, specified in
      ``tests/treecca_restatement.py``.  It follows xgboost's documented ``tree_method="hist"`` algorithm with
      ``reg_lambda=1``, ``gamma=0``, ``max_bin=256``, but its trees are not xgboost's: cut points, row and feature samples are
      its own.  ``backend="xgboost"`` and ``"lightgbm"`` raise ``ValueError``.
    - The gradient is evaluated in float64 from embeddings that hold float32 values (xgboost would hand back float32).
    - ``max_depth <= 8``, ``latent_dimensions <= 32`` (and, as in the reference, at most the narrowest view's width), at most
      8 views and 32768 features per view (``ValueError`` otherwise); ``fit`` inside :func:`cca_zoo_amd.row_sharded` raises
      ``NotImplementedError``.
    - Views may be host arrays or CUDA tensors (not a mixture); views of mixed precision are widened to float64.

    Args:
        latent_dimensions: Number of latent components. Default is 1.
        center: Whether to subtract per-view column means before fitting. Default is True.
        backend: ``"hist"``, the built-in device booster.
        n_estimators: Number of boosting rounds. Default is 50.
        max_depth: Maximum depth of each tree (at most 8). Default is 5.
        learning_rate: Boosting learning rate. Default is 0.1.
        subsample: Row subsampling ratio per round. Default is 0.8.
        colsample_bytree: Column subsampling ratio per tree. Default is 0.8.
        min_child_weight: Minimum number of sampled rows in a child. Default is 5.
        gauss_seidel: Recompute the gradient after each view's update (default) or once per round (Jacobi).
        random_state: Seed of the row / feature samples and of the random-orthogonal start. Default is 0.
    """

    _parameter_constraints: ClassVar[dict[str, list[Any]]] = {
        **BaseModel._parameter_constraints,
        "backend": [str],
        "n_estimators": POSITIVE_INT,
        "max_depth": POSITIVE_INT,
        "learning_rate": POSITIVE_EPS,
        "subsample": [Interval(Real, 0, 1, closed="right")],
        "colsample_bytree": [Interval(Real, 0, 1, closed="right")],
        "min_child_weight": [Interval(Real, 0, None, closed="left")],
        "gauss_seidel": ["boolean"],
        "random_state": [Interval(Integral, 0, None, closed="left")],
    }

    def __init__(self, latent_dimensions: int = 1, center: bool = True, backend: str = "hist", n_estimators: int = 50,
                 max_depth: int = 5, learning_rate: float = 0.1, subsample: float = 0.8, colsample_bytree: float = 0.8,
                 min_child_weight: float = 5, gauss_seidel: bool = True, random_state: int = 0) -> None:
        super().__init__(latent_dimensions=latent_dimensions, center=center)
        self.backend = backend
        self.n_estimators = n_estimators
        self.max_depth = max_depth
        self.learning_rate = learning_rate
        self.subsample = subsample
        self.colsample_bytree = colsample_bytree
        self.min_child_weight = min_child_weight
        self.gauss_seidel = gauss_seidel
        self.random_state = random_state

    def _check_backend(self):
        if self.backend in ("xgboost", "lightgbm"):
            raise ValueError(f"backend={self.backend!r} is not available: cca_zoo_amd grows its trees on the device with its own "
                             "histogram booster, backend='hist' (the only backend)")
        if isinstance(self.backend, str) and self.backend != "hist":      # anything but a string is left to _validate_params
            raise ValueError(f"backend must be 'xgboost' or 'lightgbm', got {self.backend!r}.")

    def fit(self, views, y=None):
        """Fit to a list of 2 or more (n_samples, n_features_i) host arrays or CUDA tensors."""
        self._check_backend()
        refuse_row_sharded("TreeCCA boosts on the gradient of all rows, which this build does not all-reduce")
        views_ = self._setup_fit(views)
        n, dims, M = self.n_samples_, self.n_features_in_, self.n_views_
        k, depth, rounds = int(self.latent_dimensions), int(self.max_depth), int(self.n_estimators)
        check_limits(n, dims, k, depth)
        seed = int(self.random_state) & _M64
        rng = np.random.default_rng(self.random_state)
        W = [np.linalg.qr(rng.standard_normal((p, k)))[0] for p in dims]
        rows = cut_sample_rows(n, seed)
        lists = [np.concatenate([feature_list(seed, t, v, p, self.colsample_bytree) for t in range(rounds)]) for v, p in enumerate(dims)]
        nsel = [len(l) // rounds for l in lists]
        NN = (2 << depth) - 1
        rv = ResidentViews(views_, self.center, MEANS_COLMEANS)
        with rv:
            h = rv.handle
            parr = (C.c_int64 * M)(*dims)
            with fit_state(h, "tree", M, parr, n, k, depth, rounds, float(self.learning_rate), float(self.min_child_weight),
                           1 if self.gauss_seidel else 0, float(self.subsample), seed, CHUNK_ROUNDS) as st:
                h.check(h.lib.ccz_tree_setup(h.raw, st, rv.code, rv.varr, rv.marr, rows.ctypes.data_as(C.POINTER(C.c_int64)), len(rows)))
                wcat = np.ascontiguousarray(np.concatenate([w.ravel() for w in W]), dtype=np.float64)
                sumsq = np.zeros(M * k)
                h.check(h.lib.ccz_tree_project(h.raw, st, rv.code, rv.varr, rv.marr, wcat.ctypes.data_as(C.POINTER(C.c_double)),
                                               sumsq.ctypes.data_as(C.POINTER(C.c_double))))
                if not np.all(np.isfinite(sumsq)):
                    raise ValueError("Input contains NaN or infinity.")
                scale = np.sqrt(sumsq) / np.sqrt(n - 1)
                h.check(h.lib.ccz_tree_set_margin(h.raw, st, scale.ctypes.data_as(C.POINTER(C.c_double))))
                lcat = np.ascontiguousarray(np.concatenate(lists), dtype=np.int32)
                h.check(h.lib.ccz_tree_set_features(h.raw, st, (C.c_int * M)(*nsel), lcat.ctypes.data_as(C.POINTER(C.c_int))))
                known, stopped = C.c_int64(-1), C.c_int(0)

                def enqueue(step):
                    h.check(h.lib.ccz_tree_rounds(h.raw, st, step, C.byref(known), C.byref(stopped)))
                    return 0          # the number of rounds is fixed: nothing stops a fit early

                run_chunks(rounds, CHUNK_ROUNDS, enqueue)
                done, stop = C.c_int64(0), C.c_int(0)
                h.check(h.lib.ccz_tree_status(h.raw, st, C.byref(done), C.byref(stop)))
                if done.value != rounds or not stop.value:
                    raise RuntimeError(f"TreeCCA: the device ran {done.value} of {rounds} rounds")   # cannot happen
                trees, emb = [], []
                for v in range(M):
                    arr = {"feature": np.empty((rounds, k, NN), np.int32), "bin": np.empty((rounds, k, NN), np.int32),
                           "threshold": np.empty((rounds, k, NN), np.float32), "leaf": np.empty((rounds, k, NN), np.float32),
                           "gain": np.empty((rounds, k, NN), np.float64)}
                    h.check(h.lib.ccz_tree_get_trees(h.raw, st, v, *[arr[a].ctypes.data_as(C.c_void_p)
                                                                     for a in ("feature", "bin", "threshold", "leaf", "gain")]))
                    z = np.empty((n, k))
                    h.check(h.lib.ccz_tree_get_embedding(h.raw, st, v, z.ctypes.data_as(C.c_void_p), None))
                    trees.append(arr)
                    emb.append(z)
        if not all(np.all(np.isfinite(z)) for z in emb):
            raise ValueError("Input contains NaN or infinity.")
        scale = scale.reshape(M, k)
        self._projections_ = [(w / scale[v]).astype(np.float32) for v, w in enumerate(W)]
        self._trees_ = trees
        mdt = np.float32 if (rv.f32 and self.center) else np.float64
        self.means_ = [np.ascontiguousarray(m, dtype=mdt) for m in rv.means_host()]
        self.embeddings_ = emb
        self.boosters_ = [[TreeBooster(*[t[a][:, c, :] for a in ("feature", "bin", "threshold", "leaf", "gain")], depth, p)
                           for c in range(k)] for t, p in zip(trees, dims)]
        return self

    def transform(self, views) -> list:
        """Base-margin projection plus tree sums per view, float64.  Host arrays in -> NumPy out; CUDA tensors in -> CUDA
        tensors out."""
        check_is_fitted(self)
        validated = validate_views(views, check_finite=False)
        if len(validated) != self.n_views_:
            raise ValueError(f"Expected {self.n_views_} views, got {len(validated)}.")
        out = []
        for v, m, proj, t, p in zip(validated, self.means_, self._projections_, self._trees_, self.n_features_in_):
            if int(v.shape[1]) != p:
                raise ValueError(f"a view has {int(v.shape[1])} features, the model was fit on {p}")
            if not is_device_tensor(v) and v.dtype not in (np.float32, np.float64):
                v = v.astype(np.float64)
            out.append(predict_device(v, m, proj, t["feature"], t["threshold"], t["leaf"], int(self.max_depth)))
        return out

    @property
    def weights(self) -> list:
        check_is_fitted(self)
        raise NotImplementedError(
            "TreeCCA has no linear weight matrices; its encoders are gradient-boosted-tree ensembles. Use the `boosters_` "
            'attribute instead for per-component feature importance, e.g. model.boosters_[view][component].get_score('
            'importance_type="gain").')

    def get_factor_loadings(self, views) -> list:
        """Pearson correlation of every input feature with every variate of its view: one float64 K1 pass over
        ``[X_i | Z_i]`` per view, the correlations read off the cross block of its second moments."""
        from cca_zoo_amd._moments import compute_moments

        check_is_fitted(self)
        validated = validate_views(views, check_finite=False)
        zs = self.transform(validated)
        out = []
        for v, z in zip(validated, zs):
            if is_device_tensor(v):
                import torch

                v = v.to(torch.float64)
            else:
                v = np.ascontiguousarray(v, dtype=np.float64)
            h = _backend.handle_for([v])
            mom, keep, n, dims, _ = compute_moments([v, z], h)
            p, k = int(dims[0]), int(dims[1])
            D = p + k
            h.moments_symmetrize(mom, D)
            flat = h.to_host(mom, (D * D + D,))
            del keep
            G, s = flat[: D * D].reshape(D, D), flat[D * D:]
            S = (G - np.outer(s, s) / n) / (n - 1)
            # a constant column: its centred sum of squares is the rounding residue of G - s s' / n (a few ulp of G), where
            # the reference's centred column is exactly zero and its loadings with it
            flat_col = np.diag(S) * (n - 1) <= 1e-12 * np.diag(G)
            S[flat_col, :] = 0.0
            S[:, flat_col] = 0.0
            std = np.maximum(np.sqrt(np.maximum(np.diag(S), 0.0)), 1e-12)
            out.append(S[:p, p:] / np.outer(std[:p], std[p:]))
        return out
