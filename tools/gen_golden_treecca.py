#!/usr/bin/env python3
"""Golden vectors for ``TreeCCA`` -> tests/golden/treecca_<tag>.npz.  Same import shims as tools/gen_golden_tcca.py, plus a
shim module ``xgboost`` (``DMatrix``, ``train``, ``Booster.predict``) backed by the booster of tests/treecca_restatement.py:
the REAL ``cca_zoo.tree.TreeCCA.fit / transform / score`` runs around it.  ``predict`` returns float64 arrays holding float32
values, so the reference's ``ey_grad_z`` evaluates in float64.

Stored per case: the views (``x<i>``), 10 held-out rows (``h<i>``), the parameters, every tree (``feature<i>``, ``bin<i>``,
``threshold<i>``, ``leaf<i>``, ``gain<i>``: rounds x k x nodes; ``shift<i>``: rounds x k), the training embeddings
(``z<i>``), ``transform`` of the held-out rows (``t<i>``), ``score`` of the training rows and ``mingap``.  The script asserts
that the restatement's own outer loop reproduces the run exactly (same trees, bit-equal embeddings) and that the least
relative gap at a split decision is at least 1e-6; a case that misses the gap takes the next seed and says so.
``treecca_property.npz`` holds the views of the property test (n 300, p (8, 6), k 2, depth 3, 50 rounds): the first seed on
which the restatement scores above 0.5 in every dimension, and that score.

    python tools/gen_golden_treecca.py
"""
import importlib.machinery
import importlib.metadata as md
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
REF = "/root/reference"
if not os.path.isdir(REF):
    sys.exit("reference not mounted; goldens can only be regenerated in the build container")
sys.path.insert(0, REF)
_orig_version = md.version
md.version = lambda name: "0.0.0+oracle" if name == "cca_zoo" else _orig_version(name)
_tl = types.ModuleType("tensorly")
_tl.set_backend = lambda *a, **k: None
_dec = types.ModuleType("tensorly.decomposition")
_dec.parafac = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("tensorly stub"))
_tl.decomposition = _dec
sys.modules["tensorly"] = _tl
sys.modules["tensorly.decomposition"] = _dec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import treecca_restatement as R  # noqa: E402

# ---- the xgboost shim ---------------------------------------------------------------------------------------------------
_xgb = types.ModuleType("xgboost")
_xgb.__spec__ = importlib.machinery.ModuleSpec("xgboost", None)      # cca_zoo/tree/__init__.py asks find_spec
_xgb.views_made = 0
_xgb.as_f32 = False       # True: predict returns float32, as xgboost itself would (the information-only run)


class DMatrix:
    def __init__(self, X):
        self.data = R.Binned(X, 0)
        self.view = _xgb.views_made       # the encoders are made in view order; a fit makes exactly one DMatrix per view
        _xgb.views_made += 1


class ShimBooster:
    def __init__(self, trees=(), train=None, pred=None):
        self.trees, self._train, self._pred = list(trees), train, pred

    def predict(self, dm, output_margin=True):
        if dm is self._train and self._pred is not None:
            return self._pred.astype(np.float32 if _xgb.as_f32 else np.float64)
        return R.Booster(self.trees).predict_raw(dm.data.X32).astype(np.float32 if _xgb.as_f32 else np.float64)


def train(params, dtrain, num_boost_round=0, obj=None, xgb_model=None):
    if num_boost_round == 0:
        return ShimBooster([], dtrain, np.zeros(dtrain.data.X32.shape[0], dtype=np.float32))
    assert num_boost_round == 1 and obj is not None and xgb_model is not None
    assert params["tree_method"] == "hist" and params["base_score"] == 0.0
    g, h = obj(xgb_model.predict(dtrain), dtrain)
    assert g.dtype == np.float32 and np.all(h == 1)
    dtrain.data.seed = int(params["seed"])
    t = R.boost_one(dtrain.data, g, len(xgb_model.trees), dtrain.view, params)
    pred = xgb_model._pred + R.leaf_of_pos(t, int(params["max_depth"]))[t["pos"]]
    return ShimBooster(xgb_model.trees + [t], dtrain, pred)


_xgb.DMatrix, _xgb.train, _xgb.Booster = DMatrix, train, ShimBooster
sys.modules["xgboost"] = _xgb

from cca_zoo.tree import TreeCCA  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
BASE = dict(latent_dimensions=2, center=True, n_estimators=8, max_depth=3, learning_rate=0.1, subsample=0.8, colsample_bytree=0.8,
            min_child_weight=5, gauss_seidel=True, random_state=0)
# tag, n, dims, dtype, parameter changes
CASES = (
    ("two", 300, (8, 6), np.float64, {}),
    ("three", 300, (8, 6, 5), np.float64, {"n_estimators": 6}),
    ("k1", 300, (8, 6), np.float64, {"latent_dimensions": 1}),
    ("rows517", 517, (8, 6), np.float64, {"n_estimators": 6}),
    ("tall", 4100, (3, 2), np.float64, {"max_depth": 2, "n_estimators": 3}),
    ("stump", 300, (8, 6), np.float64, {"max_depth": 1}),
    ("deep", 200, (8, 6), np.float64, {"max_depth": 6, "n_estimators": 5}),
    ("no_split", 300, (8, 6), np.float64, {"min_child_weight": 1000, "n_estimators": 3}),
    ("full_sample", 300, (8, 6), np.float64, {"subsample": 1.0, "colsample_bytree": 1.0}),
    ("sparse_sample", 300, (8, 6), np.float64, {"subsample": 0.5, "colsample_bytree": 0.5}),
    ("jacobi", 300, (8, 6), np.float64, {"gauss_seidel": False}),
    ("nocenter", 300, (8, 6), np.float64, {"center": False}),
    ("f32", 300, (8, 6), np.float32, {}),
    ("lowcard", 300, (8, 6), np.float64, {"colsample_bytree": 1.0}),
    ("p1", 300, (1, 6), np.float64, {"latent_dimensions": 1}),
)


def draw(seed, n, dims, dtype, tag):
    rng = np.random.default_rng(seed)
    lat = rng.standard_normal((n + 10, 2))
    xs = [(lat @ rng.standard_normal((2, d)) + 0.6 * rng.standard_normal((n + 10, d)) + 0.3 * i) for i, d in enumerate(dims)]
    if tag == "lowcard":
        xs[0][:, 1] = np.floor(3 * rng.random(n + 10))      # three levels
        xs[0][:, 2] = 1.5                                   # constant
        xs[0][:, 5] = xs[0][:, 0]                           # duplicated columns: equal partitions, the tie rule decides
        xs[0][:, 6] = xs[0][:, 0]
    xs = [np.ascontiguousarray(x, dtype=np.float32).astype(dtype) for x in xs]     # float32 values: stored as float32
    return [x[:n] for x in xs], [x[n:] for x in xs]


def pack(boosters, depth):
    """rounds x k x nodes arrays of one view's boosters."""
    out = {}
    for name in ("feature", "bin", "threshold", "leaf", "gain"):
        out[name] = np.stack([np.stack([b.trees[t][name] for b in boosters]) for t in range(len(boosters[0].trees))])
    out["shift"] = np.array([[b.trees[t]["shift"] for b in boosters] for t in range(len(boosters[0].trees))], dtype=np.int32)
    return out


def run(views, held, par):
    _xgb.views_made = 0
    model = TreeCCA(backend="xgboost", **par).fit(views)
    _xgb.views_made = 0      # the transform's DMatrix objects are never trained on
    z = model.transform(views)
    t = model.transform(held)
    s = model.score(views)
    gaps = [g for bs in model.boosters_ for b in bs for tr in b.trees for g in tr["gaps"]]
    return model, z, t, s, (min(gaps) if gaps else np.inf)


def main():
    for row, (tag, n, dims, dtype, change) in enumerate(CASES):
        par = dict(BASE, **change)
        seed, skipped = 8000 + 100 * row, []
        while True:
            views, held = draw(seed, n, dims, dtype, tag)
            model, z, t, s, gap = run(views, held, par)
            if gap >= R.GAP:
                break
            skipped.append(seed)
            seed += 1
        _xgb.as_f32 = True
        s32 = run(views, held, par)[3]
        _xgb.as_f32 = False
        own = R.fit(views, **par)
        for v, bs in enumerate(model.boosters_):
            for c, b in enumerate(bs):
                for a, o in zip(b.trees, own["trees"][v][c]):
                    for name in ("feature", "bin", "threshold", "leaf", "gain", "pos"):
                        assert np.array_equal(a[name], o[name]), (tag, v, c, name)
        # the training embeddings the fit ended with (bit-equal between the two outer loops)
        emb = [bm.astype(np.float64) for bm in own["embeddings"]]
        ref_emb = []
        for v, bs in enumerate(model.boosters_):
            ref_emb.append(np.column_stack([b._pred.astype(np.float64) for b in bs]))
        for v in range(len(views)):
            base = emb[v] - ref_emb[v]       # what remains is the base margin: float32 values
            assert np.array_equal(base.astype(np.float32).astype(np.float64), base), (tag, v)
        own_t = R.transform(own, held)
        for a, o in zip(t, own_t):
            assert np.array_equal(a, o), (tag, "transform")
        for a, o in zip(model._projections_, own["projections"]):
            assert np.array_equal(a, o), (tag, "projection")
        store = {"n_views": np.int64(len(views)), "f32": np.bool_(dtype == np.float32), "score": np.asarray(s), "mingap": np.float64(gap), "seed": np.int64(seed)}
        for name, val in par.items():
            store[f"par_{name}"] = np.asarray(val)
        for v in range(len(views)):
            store[f"x{v}"], store[f"h{v}"] = views[v].astype(np.float32), held[v].astype(np.float32)
            assert np.array_equal(store[f"x{v}"].astype(dtype), views[v])
            store[f"z{v}"], store[f"t{v}"] = own["embeddings"][v], t[v]
            store[f"proj{v}"] = model._projections_[v]
            for name, val in pack(model.boosters_[v], par["max_depth"]).items():
                store[f"{name}{v}"] = val
        # the fit's own embeddings against the reference's transform of the training rows: they differ by the base margin's
        # float32 rounding only
        worst = max(float(np.abs(a - b).max()) for a, b in zip(z, own["embeddings"]))
        path = os.path.join(OUT, f"treecca_{tag}.npz")
        np.savez_compressed(path, **store)
        print(f"treecca_{tag}: seed {seed} (skipped {skipped})  score {np.round(s, 4)}  min gap {gap:.2e}  float32-predict trajectory: score differs by {np.abs(s32 - s).max():.1e}  "
              f"transform(train) - embeddings {worst:.1e}  {os.path.getsize(path)} bytes")
    # the property test's views
    par = dict(BASE, n_estimators=50)
    for seed in range(100):
        views, _ = draw(9000 + seed, 300, (8, 6), np.float64, "property")
        own = R.fit(views, **par)
        sc = R.score(own["embeddings"])
        print(f"property seed {9000 + seed}: restatement score {np.round(sc, 4)}")
        if np.all(sc > 0.5):
            break
    else:
        sys.exit("no seed passed")
    store = {"score": sc, "seed": np.int64(9000 + seed), "x0": views[0].astype(np.float32), "x1": views[1].astype(np.float32)}
    for name, val in par.items():
        store[f"par_{name}"] = np.asarray(val)
    np.savez_compressed(os.path.join(OUT, "treecca_property.npz"), **store)


if __name__ == "__main__":
    main()
