"""CPU tests of TreeCCA: the estimator's surface and refusals (all raised before the device is touched: on a machine without
a GPU the first device call raises ``RuntimeError``, which none of these expects), the NumPy restatement
(tests/treecca_restatement.py) against the goldens that the real reference's outer loop produced around it
(tools/gen_golden_treecca.py), the gap condition on the goldens, and ``TreeBooster.get_score`` on a hand-built tree."""

import numpy as np
import pytest
from conftest import load_golden

import treecca_restatement as R

PARAMS = ("latent_dimensions", "center", "n_estimators", "max_depth", "learning_rate", "subsample", "colsample_bytree",
          "min_child_weight", "gauss_seidel", "random_state")
NAMES = ("feature", "bin", "threshold", "leaf", "gain")

_cache = {}


def params_of(g):
    return {k: g[f"par_{k}"].item() for k in PARAMS}


def views_of(g, prefix="x"):
    dt = np.float32 if bool(g["f32"]) else np.float64
    return [g[f"{prefix}{v}"].astype(dt) for v in range(int(g["n_views"]))]


def restated(tag):
    """(golden, the restatement's fit of its views), computed once per case."""
    if tag not in _cache:
        g = load_golden(f"treecca_{tag}")
        _cache[tag] = (g, R.fit(views_of(g), **params_of(g)))
    return _cache[tag]


def stacked(trees, name):
    """rounds x k x nodes of one view's trees[component][round]."""
    return np.stack([np.stack([trees[c][t][name] for c in range(len(trees))]) for t in range(len(trees[0]))])


def test_export_params_and_clone():
    from sklearn.base import clone

    import cca_zoo_amd
    import cca_zoo_amd.tree as tree
    from cca_zoo_amd.tree import TreeCCA

    assert "tree" in cca_zoo_amd.__all__ and "TreeCCA" in tree.__all__
    default = dict(latent_dimensions=1, center=True, backend="hist", n_estimators=50, max_depth=5, learning_rate=0.1, subsample=0.8,
                   colsample_bytree=0.8, min_child_weight=5, gauss_seidel=True, random_state=0)
    assert TreeCCA().get_params() == default
    assert list(TreeCCA().get_params(deep=False)) == sorted(default)
    import inspect

    assert list(inspect.signature(TreeCCA.__init__).parameters)[1:] == list(default)       # the reference's order
    est = TreeCCA(2, n_estimators=7, max_depth=3, subsample=0.5, gauss_seidel=False, random_state=4)
    assert clone(est).get_params() == est.get_params() and repr(clone(est)) == repr(est)
    assert "n_estimators=7" in repr(est)


def test_refusals_fire_before_the_device_is_touched():
    from cca_zoo_amd.tree import TreeCCA

    X, Y = np.zeros((6, 3)), np.zeros((6, 2))
    for name in ("xgboost", "lightgbm"):
        with pytest.raises(ValueError, match="backend='hist'"):
            TreeCCA(backend=name).fit([X, Y])
    with pytest.raises(ValueError, match="backend must be 'xgboost' or 'lightgbm', got 'catboost'"):
        TreeCCA(backend="catboost").fit([X, Y])
    with pytest.raises(ValueError, match="At least 2 views"):
        TreeCCA().fit([X])
    with pytest.raises(ValueError, match="same number of samples"):
        TreeCCA().fit([X, np.zeros((5, 2))])
    with pytest.raises(ValueError, match="max_depth=9 exceeds"):
        TreeCCA(max_depth=9).fit([X, Y])
    with pytest.raises(ValueError, match="latent_dimensions=3 exceeds the 2 features"):
        TreeCCA(latent_dimensions=3).fit([X, Y])
    with pytest.raises(ValueError, match="at most 32"):
        TreeCCA(latent_dimensions=33).fit([np.zeros((6, 40)), np.zeros((6, 33))])
    with pytest.raises(ValueError, match="at most 8"):
        TreeCCA().fit([X] * 9)
    with pytest.raises(ValueError, match="at most 32768"):
        TreeCCA().fit([np.zeros((2, 32769)), Y[:2]])
    with pytest.raises(ValueError, match="2 to"):
        TreeCCA().fit([X[:1], Y[:1]])


def test_a_fit_inside_row_sharded_is_refused(monkeypatch):
    from cca_zoo_amd import _dist
    from cca_zoo_amd.tree import TreeCCA

    monkeypatch.setattr(_dist, "is_sharded", lambda: True)
    with pytest.raises(NotImplementedError, match="row_sharded"):
        TreeCCA().fit([np.zeros((6, 3)), np.zeros((6, 2))])


@pytest.mark.parametrize("bad", [dict(n_estimators=0), dict(n_estimators=2.5), dict(max_depth=0), dict(learning_rate=0.0),
                                 dict(subsample=0.0), dict(subsample=1.5), dict(colsample_bytree=0.0), dict(colsample_bytree=2),
                                 dict(min_child_weight=-1), dict(gauss_seidel="yes"), dict(random_state=-1), dict(random_state=0.5),
                                 dict(backend=3), dict(latent_dimensions=0), dict(center="no")])
def test_every_invalid_parameter_is_refused(bad):
    from sklearn.utils._param_validation import InvalidParameterError

    from cca_zoo_amd.tree import TreeCCA

    with pytest.raises(InvalidParameterError):
        TreeCCA(**bad).fit([np.zeros((6, 3)), np.zeros((6, 2))])


def test_unfitted_model_raises_not_fitted():
    from sklearn.exceptions import NotFittedError

    from cca_zoo_amd.tree import TreeCCA

    with pytest.raises(NotFittedError):
        TreeCCA().weights
    with pytest.raises(NotFittedError):
        TreeCCA().transform([np.zeros((6, 3)), np.zeros((6, 2))])


def test_the_estimators_host_sampling_is_the_restatements():
    from cca_zoo_amd.tree import _treecca as T

    for seed in (0, 7, 2 ** 40 + 3):
        assert np.array_equal(T.cut_sample_rows(9000, seed), R.cut_sample_rows(9000, seed))
        assert np.array_equal(T.cut_sample_rows(300, seed), np.arange(300))
        for rnd, view, p, cs in ((0, 0, 8, 0.8), (3, 1, 6, 0.5), (49, 2, 1, 0.8), (5, 0, 70, 1.0)):
            assert np.array_equal(T.feature_list(seed, rnd, view, p, cs), R.feature_list(seed, rnd, view, p, cs))
    assert len(R.cut_sample_rows(9000, 0)) == 8192 and len(R.feature_list(0, 0, 0, 1, 0.5)) == 1
    assert R.row_mask(0, 0, 1000, 1.0).all() and 700 < R.row_mask(0, 0, 1000, 0.8).sum() < 900
    assert not np.array_equal(R.row_mask(0, 0, 1000, 0.8), R.row_mask(0, 1, 1000, 0.8))


@pytest.mark.parametrize("tag", R.ALL_CASES)
def test_restatement_reproduces_the_golden(tag):
    g, rs = restated(tag)
    k = int(g["par_latent_dimensions"])
    for v in range(int(g["n_views"])):
        assert len(rs["trees"][v]) == k
        for name in NAMES:
            assert np.array_equal(stacked(rs["trees"][v], name), g[f"{name}{v}"]), (tag, v, name)
        assert np.array_equal(rs["embeddings"][v], g[f"z{v}"]), (tag, v)                   # bit-equal
        assert np.array_equal(rs["projections"][v], g[f"proj{v}"])
    held = R.transform(rs, views_of(g, "h"))
    for v, t in enumerate(held):
        assert np.array_equal(t, g[f"t{v}"])
    assert np.abs(R.score(rs["embeddings"]) - g["score"]).max() < 1e-6       # score is of transform(train): the base margin's rounding


@pytest.mark.parametrize("tag", R.ALL_CASES)
def test_every_split_decision_of_a_golden_has_a_gap(tag):
    g, rs = restated(tag)
    gaps = [x for trees in rs["trees"] for comp in trees for t in comp for x in t["gaps"]]
    least = min(gaps) if gaps else np.inf
    print(tag, "decisions", len(gaps), "least gap", least)
    assert least >= R.GAP
    assert least == float(g["mingap"])


def test_the_cases_cover_what_they_are_there_for():
    feat = {t: np.concatenate([restated(t)[0][f"feature{v}"].ravel() for v in range(int(restated(t)[0]["n_views"]))]) for t in R.ALL_CASES}
    assert int(restated("three")[0]["n_views"]) == 3 and restated("k1")[0]["z0"].shape[1] == 1
    assert restated("rows517")[0]["x0"].shape[0] == 517 and restated("tall")[0]["x0"].shape[0] == 4100
    assert restated("stump")[0]["feature0"].shape[2] == 3 and restated("deep")[0]["feature0"].shape[2] == 127
    assert not (feat["no_split"] >= 0).any() and np.any(restated("no_split")[0]["leaf0"][:, :, 0] != 0)
    assert (feat["two"] >= 0).any() and (feat["deep"] >= 0).any()
    d = restated("deep")[0]["feature0"]          # leaves above the last level (the children of a split, below depth 6, that do not split)
    inner = np.arange(1, 63)
    early = (d[:, :, (inner - 1) // 2] >= 0) & (d[:, :, inner] < 0)
    print("deep: leaves above the last level in view 0:", int(early.sum()))
    assert early.sum() > 20
    assert restated("f32")[1]["means"][0].dtype == np.float32 and not np.any(restated("nocenter")[1]["means"][0])
    x = restated("lowcard")[0]["x0"]
    assert len(np.unique(x[:, 1])) == 3 and len(np.unique(x[:, 2])) == 1 and np.array_equal(x[:, 0], x[:, 5])
    f0 = restated("lowcard")[0]["feature0"]
    assert not np.isin(f0, (2, 5, 6)).any()      # the constant feature never splits; of equal columns the lowest index wins
    assert restated("p1")[0]["x0"].shape[1] == 1
    assert not bool(restated("jacobi")[0]["par_gauss_seidel"]) and float(restated("sparse_sample")[0]["par_subsample"]) == 0.5


def test_bins_follow_the_definition():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((1000, 4)).astype(np.float32)
    X[:, 1] = np.floor(3 * rng.random(1000))
    X[:, 2] = -2.0
    bins, cuts = R.make_bins(X, np.arange(1000))
    assert len(cuts[0]) == 255 and len(cuts[1]) == 2 and len(cuts[2]) == 0
    assert np.array_equal(cuts[1], np.array([1.0, 2.0], np.float32)) and not bins[:, 2].any()
    for f in range(4):
        assert np.array_equal(bins[:, f], (cuts[f][None, :] <= X[:, f][:, None]).sum(axis=1))
    # thresholds route raw values as the bins route the rows: left iff x < cut[b] iff bin <= b
    for b in (0, 100, 254):
        assert np.array_equal(X[:, 0] < cuts[0][b], bins[:, 0] <= b)


def test_quantise_and_tie_rule():
    q, S = R.quantise(np.array([0.3, -0.7, 0.0], np.float32))
    assert S == 30 and q.dtype == np.int64 and np.abs(q).max() <= 2 ** 30 and q[2] == 0
    assert np.array_equal(R.quantise(np.zeros(3, np.float32))[0], np.zeros(3, np.int64))
    # two equal columns: the lower feature index wins; an empty bin inside a node ties with its neighbour: the lower bin wins
    col = np.array([0, 0, 0, 2, 2, 2], np.uint8)
    bins = np.stack([col, col], axis=1)
    cuts = [np.array([1.0, 2.0], np.float32)] * 2
    q = np.array([5, 5, 5, -5, -5, -5], np.int64) << 20
    t = R.grow_tree(bins, cuts, q, 30, np.ones(6, bool), np.array([0, 1], np.int32), 1, 0.1, 1)
    assert t["feature"][0] == 0 and t["bin"][0] == 0 and t["threshold"][0] == 1.0
    assert np.array_equal(t["pos"], [0, 0, 0, 1, 1, 1]) and t["leaf"][1] < 0 < t["leaf"][2] and t["leaf"][0] == 0


def test_get_score_on_a_hand_built_tree():
    from cca_zoo_amd.tree import TreeBooster

    # two trees of depth 2 on 4 features: splits on f1 (gain 3), f1 (gain 1), f3 (gain 2); the second tree is one leaf
    feature = np.array([[1, 1, 3, -1, -1, -1, -1], [-1] * 7], np.int32)
    gain = np.array([[3.0, 1.0, 2.0, 0, 0, 0, 0], [0.0] * 7])
    b = TreeBooster(feature, np.zeros((2, 7), np.int32), np.zeros((2, 7), np.float32), np.zeros((2, 7), np.float32), gain, 2, 4)
    assert b.n_trees == 2
    assert b.get_score() == {"f1": 2, "f3": 1} and b.get_score(importance_type="weight") == {"f1": 2, "f3": 1}
    assert b.get_score(importance_type="total_gain") == {"f1": 4.0, "f3": 2.0}
    assert b.get_score(importance_type="gain") == {"f1": 2.0, "f3": 2.0}
    with pytest.raises(ValueError, match="importance_type"):
        b.get_score(importance_type="cover")
