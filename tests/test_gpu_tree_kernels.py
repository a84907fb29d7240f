"""GPU tests of csrc/tree.hip through the C ABI, inputs from NumPy, against tests/treecca_restatement.py: cut points and bins
(``ccz_tree_setup`` / ``ccz_tree_get_bins``), the growth of the k trees of one view through the test seam ``ccz_tree_grow``,
and the traversal ``ccz_tree_predict``.

Every comparison is an equality: node sums are integers (exact in any order of the atomics) and the gain is one float64
expression with every operation rounded once on both sides, so feature / bin / threshold / leaf / gain arrays and node ids
must agree bit for bit; the leaf value is one rounding of a float64 quotient to float32."""

import ctypes as C

import numpy as np
import pytest

import treecca_restatement as R

pytestmark = pytest.mark.gpu

VP = C.c_void_p
NAMES = ("feature", "bin", "threshold", "leaf", "gain")


def handle():
    from cca_zoo_amd import _backend

    return _backend.default_handle()


def ptr(a):
    return a.ctypes.data_as(VP)


# ---- cuts and bins -------------------------------------------------------------------------------------------------------
def device_bins(X, mean, n_views=2):
    """(bins n x p, cuts p x 256, ncuts) of view 0 of a fit state whose views are all ``X`` (dtype of ``X``)."""
    from cca_zoo_amd import _backend

    h = handle()
    n, p = X.shape
    code = _backend.F32 if X.dtype == np.float32 else _backend.F64
    xb = h.to_device(X)
    mb = h.to_device(mean.astype(X.dtype)) if mean is not None else None
    views = (_backend.View * n_views)()
    for v in views:
        v.data, v.cols, v.ld = xb.ptr, p, p
    means = (VP * n_views)(*[mb.ptr] * n_views) if mb is not None else None
    rows = R.cut_sample_rows(n, 3)
    st = VP()
    parr = (C.c_int64 * n_views)(*[p] * n_views)
    h.check(h.lib.ccz_tree_create(h.raw, n_views, parr, n, 1, 2, 1, 0.1, 5.0, 1, 0.8, 3, 4, C.byref(st)))
    try:
        h.check(h.lib.ccz_tree_setup(h.raw, st, code, views, means, rows.ctypes.data_as(C.POINTER(C.c_int64)), len(rows)))
        bins, cuts, nc = np.empty((p, n), np.uint8), np.empty((p, 256), np.float32), np.empty(p, np.int32)
        h.check(h.lib.ccz_tree_get_bins(h.raw, st, 0, ptr(bins), ptr(cuts), ptr(nc)))
    finally:
        h.lib.ccz_tree_destroy(h.raw, st)
    return bins.T.copy(), cuts, nc, rows


def draw_view(n, p, seed, special=False):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) * rng.uniform(0.5, 3.0, p) + rng.uniform(-2, 2, p)
    if special and p >= 3:
        X[:, 0] = np.floor(3 * rng.random(n))          # three levels
        X[:, 1] = -0.75                                # constant
        X[:, 2] = np.round(X[:, 2])                    # many repeated values
    return X


@pytest.mark.parametrize("n,p,dtype,center,special", [(517, 7, np.float64, True, False), (300, 5, np.float64, False, True),
                                                      (300, 5, np.float32, True, True), (64, 1, np.float32, False, False),
                                                      (2, 3, np.float64, True, False), (9000, 3, np.float64, True, True),
                                                      (8192, 2, np.float32, True, False), (8193, 2, np.float64, False, False)])
def test_cuts_and_bins_equal_the_restatement(n, p, dtype, center, special):
    X = draw_view(n, p, 100 + n + p, special).astype(dtype)
    mean = X.mean(axis=0) if center else None
    bins, cuts, nc, rows = device_bins(X, mean)
    X32 = (X - mean if center else X).astype(np.float32)
    rb, rc = R.make_bins(X32, rows)
    assert np.array_equal(nc, [len(c) for c in rc])
    for f in range(p):
        assert np.array_equal(cuts[f, :nc[f]], rc[f]), f
        assert np.all(np.isinf(cuts[f, nc[f]:]))
    assert np.array_equal(bins, rb)
    if special:
        assert nc[1] == 0 and not bins[:, 1].any() and nc[0] == 2
    if n > 8192:
        assert len(rows) == 8192 and len(np.unique(rows)) == 8192


# ---- growth --------------------------------------------------------------------------------------------------------------
def problem(n, p, k, seed, mask_keep=None, special=False):
    """Bins of a random view, k quantised gradient columns correlated with a few features, a row mask."""
    rng = np.random.default_rng(seed)
    X32 = draw_view(n, p, seed, special).astype(np.float32)
    bins, cuts = R.make_bins(X32, R.cut_sample_rows(n, 0))
    g = (X32[:, rng.integers(0, p, k)] * rng.uniform(0.5, 1.5, k) + np.sin(3 * X32[:, rng.integers(0, p, k)])
         + 0.3 * rng.standard_normal((n, k))).astype(np.float32)
    g = (g - g.mean(axis=0)).astype(np.float32) * np.float32(0.05)
    qs, shifts = zip(*[R.quantise(g[:, c]) for c in range(k)])
    if mask_keep is None:
        mask = R.row_mask(seed, 0, n, 0.8)
    else:
        mask = np.zeros(n, bool)
        mask[rng.choice(n, mask_keep, replace=False)] = True
    return X32, bins, cuts, np.stack(qs), np.array(shifts, np.int32), mask


def device_grow(bins, cuts, q, shifts, mask, feats, depth, lr, mcw, hist_bytes=0):
    h = handle()
    n, p = bins.shape
    k = q.shape[0]
    NN = (2 << depth) - 1
    cpad = np.full((p, 256), np.inf, np.float32)
    for f, c in enumerate(cuts):
        cpad[f, :len(c)] = c
    nc = np.array([len(c) for c in cuts], np.int32)
    bt = np.ascontiguousarray(bins.T)
    q32 = np.ascontiguousarray(q, dtype=np.int32)
    assert np.array_equal(q32, q)
    m8 = np.ascontiguousarray(mask, dtype=np.uint8)
    fl = np.ascontiguousarray(feats, dtype=np.int32)
    out = {"feature": np.empty((k, NN), np.int32), "bin": np.empty((k, NN), np.int32), "threshold": np.empty((k, NN), np.float32),
           "leaf": np.empty((k, NN), np.float32), "gain": np.empty((k, NN), np.float64), "pos": np.empty((k, n), np.uint8)}
    rc = h.lib.ccz_tree_grow(h.raw, n, p, k, depth, ptr(bt), ptr(cpad), ptr(nc), ptr(q32), ptr(np.ascontiguousarray(shifts, np.int32)),
                             ptr(m8), ptr(fl), len(fl), float(lr), float(mcw), int(hist_bytes), ptr(out["feature"]), ptr(out["bin"]),
                             ptr(out["threshold"]), ptr(out["leaf"]), ptr(out["gain"]), ptr(out["pos"]))
    h.check(rc)
    return out


def check_grow(n, p, k, depth, seed, mcw=5.0, mask_keep=None, feats=None, hist_bytes=0, special=False):
    X32, bins, cuts, q, shifts, mask = problem(n, p, k, seed, mask_keep, special)
    feats = R.feature_list(seed, 0, 0, p, 0.8) if feats is None else np.asarray(feats, np.int32)
    dev = device_grow(bins, cuts, q, shifts, mask, feats, depth, 0.1, mcw, hist_bytes)
    splits = 0
    for c in range(k):
        ref = R.grow_tree(bins, cuts, q[c], int(shifts[c]), mask, feats, depth, 0.1, mcw)
        for name in NAMES:
            assert np.array_equal(dev[name][c], ref[name]), (name, c)
        assert dev["leaf"][c].tobytes() == ref["leaf"].tobytes() and dev["gain"][c].tobytes() == ref["gain"].tobytes()
        assert np.array_equal(dev["pos"][c], ref["pos"]), c
        splits += int((ref["feature"] >= 0).sum())
    return dev, splits, (X32, bins, cuts, q, shifts, mask, feats)


#: n in {1, 63, 64, 65, 517, 4100}, p in {1, 7, 70}, k in {1, 3}, depth in {1, 3, 6, 8} (n = 200 at depth 8)
SHAPES = [(1, 1, 1, 1, 1.0), (63, 7, 1, 3, 2.0), (64, 7, 3, 3, 2.0), (65, 1, 3, 1, 2.0), (65, 70, 1, 6, 1.0), (517, 7, 3, 6, 5.0),
          (517, 70, 3, 3, 5.0), (517, 1, 1, 8, 1.0), (4100, 7, 3, 3, 5.0), (4100, 70, 1, 6, 5.0), (4100, 1, 3, 1, 5.0),
          (200, 7, 3, 8, 1.0), (200, 70, 1, 8, 1.0)]


@pytest.mark.parametrize("n,p,k,depth,mcw", SHAPES)
def test_grown_trees_equal_the_restatement(n, p, k, depth, mcw):
    _, splits, _ = check_grow(n, p, k, depth, 1000 + n + 7 * p + k + depth, mcw)
    print(n, p, k, depth, "splits", splits)
    assert splits > 0 or n == 1


def test_low_cardinality_constant_and_duplicate_features_follow_the_tie_rule():
    X32, bins, cuts, q, shifts, mask = problem(517, 7, 3, 77, special=True)
    bins[:, 5], cuts[5] = bins[:, 3], cuts[3]            # two features inducing one partition
    feats = np.arange(7, dtype=np.int32)
    dev = device_grow(bins, cuts, q, shifts, mask, feats, 4, 0.1, 5.0)
    for c in range(3):
        ref = R.grow_tree(bins, cuts, q[c], int(shifts[c]), mask, feats, 4, 0.1, 5.0)
        for name in NAMES:
            assert np.array_equal(dev[name][c], ref[name]), (name, c)
        assert np.array_equal(dev["pos"][c], ref["pos"])
    assert not np.isin(dev["feature"], (1, 5)).any()       # the constant never splits, the duplicate never wins


def test_all_rows_masked_out_but_min_child_weight_many():
    # 5 sampled rows, min_child_weight 5: no admissible split, every tree is its root leaf; with 10 rows and a tie-free
    # gradient exactly one split is admissible per feature
    dev, splits, _ = check_grow(517, 7, 3, 3, 5, mcw=5.0, mask_keep=5)
    assert splits == 0 and np.all(dev["feature"] == -1) and np.all(dev["leaf"][:, 0] != 0) and not dev["pos"].any()
    dev, splits, _ = check_grow(517, 7, 3, 3, 6, mcw=5.0, mask_keep=10)
    assert np.all((dev["feature"] >= 0).sum(axis=1) <= 1)


def test_a_feature_list_of_one_and_a_last_feature():
    dev, splits, _ = check_grow(517, 70, 3, 3, 9, feats=[69])
    assert splits > 0 and set(np.unique(dev["feature"])) <= {-1, 69}


def test_feature_tiling_gives_the_same_trees():
    # 56 candidate features through a workspace of one, three and all features per tile: the running best crosses tiles
    one = 3 * 4 * 256 * 12
    a, splits, _ = check_grow(517, 70, 3, 3, 11, hist_bytes=one)
    b, _, _ = check_grow(517, 70, 3, 3, 11, hist_bytes=3 * one)
    c, _, _ = check_grow(517, 70, 3, 3, 11)
    assert splits > 0
    for name in NAMES + ("pos",):
        assert a[name].tobytes() == b[name].tobytes() == c[name].tobytes()


def test_the_same_call_twice_gives_identical_bytes():
    a, _, _ = check_grow(4100, 7, 3, 6, 13)
    b, _, _ = check_grow(4100, 7, 3, 6, 13)
    for name in NAMES + ("pos",):
        assert a[name].tobytes() == b[name].tobytes()


# ---- predict -------------------------------------------------------------------------------------------------------------
def device_predict(X, mean, proj, trees, depth):
    """trees: list (in tree order) of dicts of k x nodes arrays."""
    from cca_zoo_amd.tree._treecca import predict_device

    stack = {name: np.stack([t[name] for t in trees]) for name in ("feature", "threshold", "leaf")}
    return predict_device(X, mean, proj, stack["feature"], stack["threshold"], stack["leaf"], depth)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_predict_on_the_training_rows_reproduces_the_node_id_route(dtype):
    depth, k = 4, 3
    trees, X32 = [], None
    for t in range(3):
        dev, _, (X32, bins, cuts, q, shifts, mask, feats) = check_grow(517, 7, k, depth, 21, mcw=3.0 + t)
        trees.append(dev)
    X = X32.astype(dtype)
    out = device_predict(X, None, None, trees, depth)
    want = np.zeros((517, k), np.float32)
    for t in trees:
        for c in range(k):
            one = {name: t[name][c] for name in NAMES}
            by_pos = R.leaf_of_pos(one, depth)[t["pos"][c]]
            assert np.array_equal(by_pos, R.predict_tree(one, X32))
            want[:, c] = want[:, c] + by_pos                 # float32, in tree order
    assert out.dtype == np.float64 and np.array_equal(out, want.astype(np.float64))
    # with a mean and a projection: (X - mean) P in float64 plus the same sums
    rng = np.random.default_rng(3)
    mean = rng.standard_normal(7).astype(dtype)
    P = rng.standard_normal((7, k))
    shifted = (X + mean).astype(dtype)
    out2 = device_predict(shifted, mean, P, trees, depth)
    xc = (shifted - mean)
    want2 = np.zeros((517, k), np.float32)
    for t in trees:
        for c in range(k):
            want2[:, c] = want2[:, c] + R.predict_tree({name: t[name][c] for name in NAMES}, xc.astype(np.float32))
    bm = xc.astype(np.float64) @ P
    assert np.abs(out2 - (bm + want2)).max() <= 1e-12 * max(1.0, np.abs(bm).max())


def test_a_row_equal_to_a_threshold_goes_right():
    dev, splits, (X32, bins, cuts, q, shifts, mask, feats) = check_grow(517, 7, 1, 1, 31)
    assert splits == 1
    f, thr = int(dev["feature"][0, 0]), dev["threshold"][0, 0]
    rows = np.zeros((3, 7), np.float32)
    rows[:, f] = [np.nextafter(thr, np.float32(-np.inf)), thr, np.nextafter(thr, np.float32(np.inf))]
    out = device_predict(rows, None, None, [dev], 1)[:, 0]
    assert np.array_equal(out, np.array([dev["leaf"][0, 1], dev["leaf"][0, 2], dev["leaf"][0, 2]], np.float64))
    assert dev["leaf"][0, 1] != dev["leaf"][0, 2]


# ---- misuse --------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused_with_einval():
    h = handle()
    L = h.lib
    known, stopped = C.c_int64(0), C.c_int(0)
    assert L.ccz_tree_rounds(h.raw, None, 1, C.byref(known), C.byref(stopped)) == -1
    assert L.ccz_tree_status(h.raw, None, None, None) == -1
    assert L.ccz_tree_get_bins(h.raw, None, 0, None, None, None) == -1
    assert L.ccz_tree_create(h.raw, 2, (C.c_int64 * 2)(3, 2), 10, 1, 2, 1, 0.1, 5.0, 1, 0.8, 0, 4, None) == -1
    st = VP()
    parr = (C.c_int64 * 2)(3, 2)
    for bad in (dict(k=3), dict(depth=9), dict(depth=0), dict(rounds=0), dict(sub=0.0), dict(sub=1.5), dict(n=1)):
        a = dict(n=10, k=1, depth=2, rounds=1, sub=0.8)
        a.update(bad)
        assert L.ccz_tree_create(h.raw, 2, parr, a["n"], a["k"], a["depth"], a["rounds"], 0.1, 5.0, 1, a["sub"], 0, 4, C.byref(st)) < 0, bad
        assert not st.value
    h.check(L.ccz_tree_create(h.raw, 2, parr, 10, 1, 2, 1, 0.1, 5.0, 1, 0.8, 0, 4, C.byref(st)))
    try:
        assert L.ccz_tree_rounds(h.raw, st, 1, C.byref(known), C.byref(stopped)) == -1        # before setup
        assert L.ccz_tree_get_bins(h.raw, st, 0, None, None, None) == -1
        assert L.ccz_tree_status(h.raw, st, None, None) == -1
        assert L.ccz_tree_get_trees(h.raw, st, 0, None, None, None, None, None) == -1
        assert L.ccz_tree_get_embedding(h.raw, st, 5, None, None) == -1
        assert L.ccz_tree_setup(h.raw, st, 1, None, None, None, 10) == -1
        assert L.ccz_tree_set_margin(h.raw, st, None) == -1
        assert L.ccz_tree_set_features(h.raw, st, None, None) == -1
    finally:
        L.ccz_tree_destroy(h.raw, st)
    assert L.ccz_tree_destroy(h.raw, None) == 0
    assert L.ccz_tree_grow(h.raw, 10, 3, 1, 2, *([None] * 7), 1, 0.1, 5.0, 0, *([None] * 6)) == -1
    assert L.ccz_tree_predict(h.raw, 1, None, 10, None, None, 1, 0, 2, None, None, None, None, 1) == -1
    # a feature list that does not ascend, a feature out of range
    X32, bins, cuts, q, shifts, mask = problem(65, 7, 1, 1)
    for feats in ([3, 2], [0, 7], [-1]):
        with pytest.raises(ValueError):
            device_grow(bins, cuts, q, shifts, mask, feats, 2, 0.1, 1.0)
