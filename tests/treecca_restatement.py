"""Integer / float64 NumPy restatement of TreeCCA as ``csrc/tree.hip`` runs it: the reference's outer loop
(``cca_zoo/tree/_treecca.py:329-360``) around a histogram booster that this file specifies.  It is the contract of the CPU
and GPU tests (``test_treecca_host.py``, ``test_gpu_tree_kernels.py``, ``test_gpu_treecca.py``) and the booster behind the
``xgboost`` shim of ``tools/gen_golden_treecca.py``, which runs the real reference's ``TreeCCA`` around it.

The booster restates xgboost's documented ``tree_method="hist"`` regression tree for the parameters the reference passes,
with ``reg_lambda = 1``, ``gamma = 0``, ``max_bin = 256``, ``base_score = 0``, depth-wise growth and the hessian 1 of the
reference's objective.  No parity with xgboost's own trees is claimed.

Bins.  The (centred) view is cast to float32.  Per feature the cut points are the values at ranks ``j S / 256`` (j = 1..255)
of the sorted column of a row sample of ``S = min(n, 8192)`` rows (all rows up to 8192, else the rows with the S smallest
hash keys, ties to the lower index); equal cuts are merged and cuts equal to the sample's minimum dropped.  ``bin(x)`` is the
number of cuts ``<= x`` (uint8).  A constant feature has one bin and no candidate split.

Sampling.  ``key(seed, tag, i) = splitmix64(splitmix64(seed ^ splitmix64(tag)) ^ splitmix64(i))``.  Row r is in the sample of
round t iff ``key(seed, 2 t, r) < subsample 2^64`` (all views and components of a round share it); the features of the
trees of (round t, view v) are the ``max(1, floor(colsample_bytree p))`` features with the smallest ``key(seed, 2 (64 t + v)
+ 1, f)``, ties to the lower index, in ascending feature order; the cut sample uses the tag ``2^63``.

Gradients in fixed point.  A float32 gradient column g becomes ``q = rint(g 2^S)``, ``S = 30 - frexp_exponent(max |g|)``
(S = 0 for a zero column): |q| <= 2^30, node sums are exact integers whatever the order of summation.

Split.  Candidate (feature, bin b) sends ``bin <= b`` left; admissible iff both children hold at least ``min_child_weight``
sampled rows; with the sums scaled by ``2^-S``: ``gain = GL^2 / (HL + 1) + GR^2 / (HR + 1) - G^2 / (H + 1)``, float64, every
operation rounded once, evaluated as ``((GL GL) / (HL + 1) + (GR GR) / (HR + 1)) - (G G) / (H + 1)``.  A node splits iff its
best gain is > 0; ties go to the lowest feature index, then the lowest bin.  Leaf: ``float32((-lr (G 2^-S)) / (H + 1))``.
Rows outside the sample are routed too.  The stored threshold is cut b; ``predict`` goes left iff ``float32(x) < threshold``.

Trees are stored as heaps of ``2^(depth + 1) - 1`` nodes (children of i: 2 i + 1, 2 i + 2): ``feature`` (-1: not a split),
``bin``, ``threshold``, ``leaf`` (the value of a leaf, else 0), ``gain`` (of a split, else 0).  ``pos`` is a row's position
in the last level with a leaf above it continued to the left (``pos -> 2 pos``), as the device's uint8 node ids are.
"""

from __future__ import annotations

import numpy as np

MAX_BIN = 256
CUT_SAMPLE = 8192
LAMBDA = 1.0
TARGET_STD = 0.1
CUT_TAG = 1 << 63

#: every golden of tools/gen_golden_treecca.py
ALL_CASES = ["two", "three", "k1", "rows517", "tall", "stump", "deep", "no_split", "full_sample", "sparse_sample", "jacobi",
             "nocenter", "f32", "lowcard", "p1"]
GAP = 1e-6     # least relative gap between the best gain and the best different one at every split decision of a golden


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def hash_keys(seed, tag, count):
    stream = splitmix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ splitmix64(np.uint64(int(tag) & 0xFFFFFFFFFFFFFFFF)))
    return splitmix64(stream ^ splitmix64(np.arange(count, dtype=np.uint64)))


def cut_sample_rows(n, seed):
    if n <= CUT_SAMPLE:
        return np.arange(n, dtype=np.int64)
    order = np.argsort(hash_keys(seed, CUT_TAG, n), kind="stable")[:CUT_SAMPLE]
    return np.sort(order).astype(np.int64)


def row_mask(seed, rnd, n, subsample):
    thr = int(float(subsample) * 2.0 ** 64)
    if thr >= 1 << 64:
        return np.ones(n, dtype=bool)
    return hash_keys(seed, 2 * rnd, n) < np.uint64(thr)


def feature_list(seed, rnd, view, p, colsample):
    nsel = max(1, int(np.floor(float(colsample) * p)))
    order = np.argsort(hash_keys(seed, 2 * (64 * rnd + view) + 1, p), kind="stable")[:nsel]
    return np.sort(order).astype(np.int32)


def make_cuts(column):
    """Cut points (float32, ascending, at most 255) of one sampled float32 column."""
    s = np.sort(np.asarray(column, dtype=np.float32))
    S = len(s)
    cand = s[(np.arange(1, MAX_BIN) * S) // MAX_BIN]
    cuts = np.unique(cand)
    return cuts[cuts != s[0]].astype(np.float32)


def make_bins(X32, rows):
    """(bins uint8 n x p, list of cut arrays) of a float32 view with the cut sample ``rows``."""
    X32 = np.asarray(X32, dtype=np.float32)
    cuts = [make_cuts(X32[rows, f]) for f in range(X32.shape[1])]
    bins = np.stack([np.searchsorted(c, X32[:, f], side="right") for f, c in enumerate(cuts)], axis=1).astype(np.uint8)
    return bins, cuts


def quantise(g32):
    """(q int64, S) of a float32 gradient column."""
    g32 = np.asarray(g32, dtype=np.float32)
    m = float(np.max(np.abs(g32))) if g32.size else 0.0
    if m == 0.0:
        return np.zeros(g32.shape, dtype=np.int64), 0
    S = 30 - int(np.frexp(m)[1])
    return np.rint(np.ldexp(g32.astype(np.float64), S)).astype(np.int64), S


def _gain(GL, HL, G, H, S):
    sc = np.ldexp(1.0, -S)
    gl, gr, g = GL.astype(np.float64) * sc, (G - GL).astype(np.float64) * sc, np.float64(G) * sc
    hl, hr, h = HL.astype(np.float64), (H - HL).astype(np.float64), np.float64(H)
    return ((gl * gl) / (hl + LAMBDA) + (gr * gr) / (hr + LAMBDA)) - (g * g) / (h + LAMBDA)


def grow_tree(bins, cuts, q, S, mask, feats, depth, lr, mcw):
    """One tree.  ``bins`` n x p uint8, ``cuts`` per feature, ``q`` int64 per row, ``mask`` the sampled rows, ``feats`` the
    ascending candidate features.  Returns a dict: the heap arrays, ``pos`` (uint8 per row) and ``gaps`` (one per decision)."""
    n = bins.shape[0]
    NN = (1 << (depth + 1)) - 1
    tree = {"feature": np.full(NN, -1, np.int32), "bin": np.zeros(NN, np.int32), "threshold": np.zeros(NN, np.float32),
            "leaf": np.zeros(NN, np.float32), "gain": np.zeros(NN, np.float64)}
    q = np.asarray(q, dtype=np.int64)
    pos = np.zeros(n, dtype=np.int64)
    exists = {0: (int(q[mask].sum()), int(mask.sum()))}       # heap node -> (G, H) of the nodes still open
    leaves, gaps = {}, []
    for d in range(depth):
        base = (1 << d) - 1
        nxt = {}
        split = np.zeros(1 << d, dtype=bool)
        sf, sb = np.zeros(1 << d, np.int64), np.zeros(1 << d, np.int64)
        for node, (G, H) in sorted(exists.items()):
            j = node - base
            rows = mask & (pos == j)
            best, bf, bb, bGL, bHL, allg = -np.inf, -1, -1, 0, 0, []
            for f in feats:
                nb = len(cuts[f]) + 1
                if nb < 2:
                    continue
                hg = np.zeros(nb, np.int64)
                np.add.at(hg, bins[rows, f], q[rows])
                hh = np.bincount(bins[rows, f], minlength=nb).astype(np.int64)
                GL, HL = np.cumsum(hg)[:-1], np.cumsum(hh)[:-1]
                ok = (HL.astype(np.float64) >= mcw) & ((H - HL).astype(np.float64) >= mcw)
                if not ok.any():
                    continue
                gain = np.where(ok, _gain(GL, HL, G, H, S), -np.inf)
                allg.append(gain[ok])
                b = int(np.argmax(gain))
                if gain[b] > best:
                    best, bf, bb, bGL, bHL = float(gain[b]), int(f), b, int(GL[b]), int(HL[b])
            if allg:
                allg = np.concatenate(allg)
                if best > 0:
                    other = allg[allg != best]
                    gaps.append(float((best - other.max()) / best) if other.size else np.inf)
                else:
                    gs = np.float64(G) * np.ldexp(1.0, -S)
                    ref = float((gs * gs) / (np.float64(H) + LAMBDA))
                    if ref > 0:
                        gaps.append(abs(best) / ref)
            if best > 0:
                tree["feature"][node], tree["bin"][node] = bf, bb
                tree["threshold"][node], tree["gain"][node] = cuts[bf][bb], best
                nxt[2 * node + 1], nxt[2 * node + 2] = (bGL, bHL), (G - bGL, H - bHL)
                split[j], sf[j], sb[j] = True, bf, bb
            else:
                leaves[node] = (G, H)
        right = split[pos] & (bins[np.arange(n), sf[pos]] > sb[pos])
        pos = 2 * pos + right
        exists = nxt
    leaves.update(exists)
    sc = np.ldexp(1.0, -S)
    for node, (G, H) in leaves.items():
        tree["leaf"][node] = np.float32((-float(lr) * (np.float64(G) * sc)) / (np.float64(H) + LAMBDA))
    tree["pos"] = pos.astype(np.uint8)
    tree["gaps"] = gaps
    return tree


def leaf_of_pos(tree, depth):
    """The leaf value under every position of the last level (a leaf above it covers the positions on its left spine)."""
    out = np.zeros(1 << depth, np.float32)
    for j in range(1 << depth):
        for d in range(depth + 1):
            node = (1 << d) - 1 + (j >> (depth - d))
            if tree["feature"][node] < 0:
                out[j] = tree["leaf"][node]
                break
    return out


def predict_tree(tree, X32):
    """float32 leaf value per row of raw float32 data: left iff x < threshold."""
    X32 = np.asarray(X32, dtype=np.float32)
    node = np.zeros(X32.shape[0], dtype=np.int64)
    while True:
        f = tree["feature"][node]
        live = f >= 0
        if not live.any():
            break
        r = np.nonzero(live)[0]
        go_right = X32[r, f[r]] >= tree["threshold"][node[r]]
        node[r] = 2 * node[r] + 1 + go_right
    return tree["leaf"][node]


class Booster:
    """The trees of one component of one view, in the order they were added."""

    def __init__(self, trees=()):
        self.trees = list(trees)

    def predict_raw(self, X32):
        out = np.zeros(np.asarray(X32).shape[0], dtype=np.float32)
        for t in self.trees:
            out = out + predict_tree(t, X32)          # float32, in tree order
        return out


class Binned:
    """A float32 view with its bins (made on first use)."""

    def __init__(self, X, seed=0):
        self.X32 = np.ascontiguousarray(np.asarray(X), dtype=np.float32)
        self.seed = seed
        self._bins = None

    def bins(self):
        if self._bins is None:
            self._bins = make_bins(self.X32, cut_sample_rows(self.X32.shape[0], self.seed))
        return self._bins


def boost_one(data, g32, rnd, view, params):
    """The tree that round ``rnd`` adds to one component of view ``view`` for the float32 gradient column ``g32``."""
    bins, cuts = data.bins()
    n, p = bins.shape
    seed = int(params["seed"])
    q, S = quantise(g32)
    tree = grow_tree(bins, cuts, q, S, row_mask(seed, rnd, n, params["subsample"]),
                     feature_list(seed, rnd, view, p, params["colsample_bytree"]), int(params["max_depth"]),
                     float(params["learning_rate"]), float(params["min_child_weight"]))
    tree["shift"] = S
    return tree


def ey_grad_z(reps):
    """cca_zoo/_utils/_ey.py:187-212, operation for operation."""
    n, m = reps[0].shape[0], len(reps)
    centred = [z - z.mean(axis=0) for z in reps]
    total = sum(centred)
    k = centred[0].shape[1]
    V = np.zeros((k, k))
    for zi in centred:
        V += zi.T @ zi / (n - 1)
    V = V / m
    scale = 4.0 / (m * (n - 1))
    return [scale * (zc @ V - total) for zc in centred]


def rescale(grads):
    scale = max(max(float(g.std()) for g in grads), 1e-6)
    return [(g / scale * TARGET_STD).astype(np.float32) for g in grads]


def base_margin(Xc, k, rng):
    n, p = Xc.shape
    W, _ = np.linalg.qr(rng.standard_normal((p, k)))
    Z = Xc @ W
    scale = np.linalg.norm(Z, axis=0, keepdims=True) / np.sqrt(n - 1)
    return (Z / scale).astype(np.float32), (W / scale).astype(np.float32)


def fit(views, latent_dimensions=1, center=True, n_estimators=50, max_depth=5, learning_rate=0.1, subsample=0.8,
        colsample_bytree=0.8, min_child_weight=5, gauss_seidel=True, random_state=0):
    """The whole fit.  Returns a dict: ``means``, ``projections``, ``trees[view][component]`` (lists of tree dicts) and
    ``embeddings`` (float64 arrays holding float32 base margin + float32 tree sum)."""
    views = [np.asarray(v) for v in views]
    views = [v if v.dtype in (np.float32, np.float64) else v.astype(np.float64) for v in views]
    k, M = int(latent_dimensions), len(views)
    if center:
        means = [v.mean(axis=0) for v in views]
        views = [v - m for v, m in zip(views, means)]
    else:
        means = [np.zeros(v.shape[1]) for v in views]
    rng = np.random.default_rng(random_state)
    bms, projs = zip(*[base_margin(X, k, rng) for X in views])
    params = {"seed": int(random_state), "subsample": subsample, "colsample_bytree": colsample_bytree, "max_depth": max_depth,
              "learning_rate": learning_rate, "min_child_weight": min_child_weight}
    data = [Binned(X, int(random_state)) for X in views]
    n = views[0].shape[0]
    trees = [[[] for _ in range(k)] for _ in range(M)]
    sums = [np.zeros((n, k), dtype=np.float32) for _ in range(M)]

    def reps():
        return [bm + s.astype(np.float64) for bm, s in zip(bms, sums)]

    for rnd in range(int(n_estimators)):
        cur = reps()
        grads = rescale(ey_grad_z(cur))
        for v in range(M):
            for c in range(k):
                t = boost_one(data[v], grads[v][:, c].copy(), rnd, v, params)
                trees[v][c].append(t)
                sums[v][:, c] = sums[v][:, c] + leaf_of_pos(t, int(max_depth))[t["pos"]]
            if gauss_seidel and v < M - 1:
                cur[v] = bms[v] + sums[v].astype(np.float64)
                grads = rescale(ey_grad_z(cur))
    return {"means": means, "projections": list(projs), "trees": trees, "embeddings": reps()}


def transform(model, views):
    out = []
    for v, m, proj, trees in zip(views, model["means"], model["projections"], model["trees"]):
        vc = np.asarray(v) - m
        x32 = vc.astype(np.float32)
        pred = np.column_stack([Booster(t).predict_raw(x32) for t in trees])
        out.append(vc @ proj + pred.astype(np.float64))
    return out


def score(zs):
    """BaseModel.average_pairwise_correlations on the variates ``zs``."""
    m, k = len(zs), zs[0].shape[1]
    zc = [z - z.mean(axis=0) for z in zs]
    nrm = [np.sqrt((z * z).sum(axis=0)) for z in zc]
    nrm = [np.where(x > 1e-12, x, 1.0) for x in nrm]
    tot = np.zeros(k)
    for i in range(m):
        for j in range(m):
            if i != j:
                tot += (zc[i] * zc[j]).sum(axis=0) / (nrm[i] * nrm[j])
    return tot / (m * (m - 1))
