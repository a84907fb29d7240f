#!/usr/bin/env python3
"""Capture golden vectors of the reference's gradient (Eckart-Young) models: CCA_EY, PLS_EY, MCCA_EY.

Same shims as ``tools/gen_golden_kernel.py``.  Every case stores its inputs, the reference's ``weights_`` and
``means_``, training and held-out ``transform`` / ``score``, factor loadings, the number of gradient steps it took
(``_objective`` calls), ``|prev - obj|`` at the last two steps and the first three mini-batch index draws, in
``tests/golden/ey_<case>.npz``.  A case whose stop margin lies within 1 % of ``tol`` is rejected: a rounding
difference could move its stop by a step.

    python tools/gen_golden_ey.py
"""

from __future__ import annotations

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


def _nope(*a, **k):
    raise RuntimeError("tensorly stub")


_dec.parafac = _nope
_tl.decomposition = _dec
sys.modules["tensorly"] = _tl
sys.modules["tensorly.decomposition"] = _dec

from cca_zoo.linear.gradient import CCA_EY, MCCA_EY, PLS_EY  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
sys.path.insert(0, os.path.dirname(OUT))
from conftest import save_npz_parts  # noqa: E402
os.makedirs(OUT, exist_ok=True)

MODELS = {"CCA_EY": CCA_EY, "PLS_EY": PLS_EY, "MCCA_EY": MCCA_EY}


def views(seed, n, dims, latent=2, noise=0.5, dtype=np.float64):
    """Views sharing a ``latent``-dimensional signal (+ offsets, so that centring matters)."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, latent))
    out = []
    for d in dims:
        A = rng.standard_normal((latent, d))
        x = z @ A + noise * rng.standard_normal((n, d)) + rng.uniform(-1, 1, d)
        out.append(x.astype(dtype))
    return out


def choice_branch(n, bs, seed=0):
    """Which branch NumPy's ``Generator.choice(n, bs, replace=False)`` takes, found by experiment: the tail shuffle of
    ``arange(n)`` fixes the LAST output first, so its last entry does not depend on ``bs``; Floyd's method ends
    with a shuffle of the whole sample, so it does."""
    a = np.random.default_rng(seed).choice(n, bs, replace=False)[-1]
    b = np.random.default_rng(seed).choice(n, bs + 1, replace=False)[-1]
    return "tail" if a == b else "floyd"


def confirm_choice_cutoff():
    """Generator.choice switches to the tail shuffle when n > 10000 and bs > n // 50 (numpy/random/_generator.pyx);
    check that on the installed NumPy before choosing the shapes of the two branch cases."""
    for n in (10000, 12000):
        cut = n // 50
        seen = {bs: {choice_branch(n, bs, s) for s in range(6)} for bs in (cut - 1, cut, cut + 1, cut + 2)}
        for bs, branches in seen.items():
            want = "tail" if (n > 10000 and bs > cut) else "floyd"
            # Floyd's final shuffle can leave the last entry unchanged by chance; a tail draw never moves it
            assert (branches == {"tail"}) == (want == "tail"), (n, bs, branches)
    return True


class _Rec:
    """Proxy of the fit's Generator that keeps every ``choice`` draw."""

    def __init__(self, g):
        self._g, self.draws = g, []

    def choice(self, *a, **k):
        r = self._g.choice(*a, **k)
        self.draws.append(np.asarray(r).copy())
        return r

    def __getattr__(self, name):
        return getattr(self._g, name)


CASES = [
    # name, model, params, dims, n, dtype, held-out n
    ("cca_c0", "CCA_EY", dict(latent_dimensions=2, c=0.0, batch_size=64, max_iter=200, tol=0.0, random_state=1),
     (12, 9), 500, np.float64),
    ("cca_c03", "CCA_EY", dict(latent_dimensions=3, c=0.3, batch_size=100, learning_rate=5e-3, max_iter=150,
                               random_state=2), (14, 10), 400, np.float64),
    # c = 0 with few rows per batch against the width: the reference runs to max_iter and returns NaN weights
    ("diverge_c0", "CCA_EY", dict(latent_dimensions=2, c=0.0, batch_size=12, learning_rate=0.05, max_iter=60,
                                  random_state=13), (14, 10), 200, np.float64),
    ("cca_c1_k1", "CCA_EY", dict(latent_dimensions=1, c=1.0, batch_size=40, max_iter=100, random_state=3), (8, 6), 300,
     np.float64),
    ("pls", "PLS_EY", dict(latent_dimensions=2, batch_size=50, max_iter=150, tol=0.0, random_state=4), (15, 10), 400,
     np.float64),
    ("mcca3", "MCCA_EY", dict(latent_dimensions=2, c=0.1, batch_size=60, max_iter=120, random_state=5), (10, 8, 6), 400,
     np.float64),
    ("mcca4", "MCCA_EY", dict(latent_dimensions=3, c=0.2, batch_size=80, max_iter=80, tol=0.0, random_state=6),
     (9, 7, 12, 5), 400, np.float64),
    ("nocenter", "CCA_EY", dict(latent_dimensions=2, c=0.2, center=False, batch_size=64, max_iter=100, tol=0.0,
                                random_state=7), (10, 8), 400, np.float64),
    ("fullbatch", "CCA_EY", dict(latent_dimensions=2, c=0.1, max_iter=300, random_state=8), (10, 7), 300, np.float64),
    ("fullbatch_pls", "PLS_EY", dict(latent_dimensions=2, max_iter=300, learning_rate=0.05, random_state=9), (6, 5), 200,
     np.float64),
    ("floyd_f32", "CCA_EY", dict(latent_dimensions=2, c=0.3, batch_size=200, max_iter=60, tol=0.0, random_state=10),
     (5, 4), 12000, np.float32),
    ("tail_f32", "CCA_EY", dict(latent_dimensions=2, c=0.3, batch_size=300, max_iter=60, tol=0.0, random_state=11),
     (5, 4), 12000, np.float32),
    ("f32_k3", "MCCA_EY", dict(latent_dimensions=3, c=0.5, batch_size=100, max_iter=100, random_state=12), (11, 9, 7),
     600, np.float32),
]


def run_case(name, model, params, dims, n, dtype):
    data = views(sum(name.encode()) + 17, n + 100, dims, dtype=dtype)
    train = [v[:n] for v in data]
    test = [v[n:] for v in data]
    est = MODELS[model](**params)
    objs = []
    orig = est._objective

    def rec(*a, **k):
        o = orig(*a, **k)
        objs.append(o)
        return o

    est._objective = rec
    real = np.random.default_rng
    box = {}

    def patched(seed=None):
        box["r"] = _Rec(real(seed))
        return box["r"]

    np.random.default_rng = patched
    try:
        est.fit(train)
    finally:
        np.random.default_rng = real
    del est._objective
    tol = float(est.tol)
    steps = len(objs)
    diffs = [abs(a - b) for a, b in zip([np.inf] + objs[:-1], objs)]
    last2 = np.array(diffs[-2:] if steps >= 2 else [np.inf] + diffs, dtype=np.float64)
    if tol > 0:
        for d in diffs:
            if np.isfinite(d) and abs(d - tol) < 0.01 * tol:
                raise SystemExit(f"{name}: a stop margin {d} is within 1% of tol {tol}")
    draws = box["r"].draws
    out = {f"X{i}": v for i, v in enumerate(train)}
    out.update({f"T{i}": v for i, v in enumerate(test)})
    out.update({f"W{i}": w for i, w in enumerate(est.weights_)})
    out.update({f"mean{i}": m for i, m in enumerate(est.means_)})
    if np.all([np.all(np.isfinite(w)) for w in est.weights_]):
        out.update({f"Z{i}": z for i, z in enumerate(est.transform(train))})
        out.update({f"Zt{i}": z for i, z in enumerate(est.transform(test))})
        out["score"] = np.asarray(est.score(train))
        out["score_test"] = np.asarray(est.score(test))
        out.update({f"L{i}": z for i, z in enumerate(est.get_factor_loadings(train))})
    out["n_iter"] = np.int64(steps)
    out["stop_margins"] = last2
    out["objectives"] = np.asarray(objs, dtype=np.float64)
    for t in range(min(3, len(draws))):
        out[f"draw{t}"] = draws[t].astype(np.int64)
    out["n_draws"] = np.int64(len(draws))
    out["model"] = np.array(model)
    out["params"] = np.array(repr(sorted(params.items())))
    out["n_views"] = np.int64(len(dims))
    save_npz_parts(os.path.join(OUT, f"ey_{name}.npz"), out)
    print(f"{name}: steps={steps} draws={len(draws)} last |dobj|={last2} "
          f"finite={all(np.all(np.isfinite(w)) for w in est.weights_)}")


def main():
    confirm_choice_cutoff()
    print("Generator.choice: Floyd's method below n > 10000 and bs > n // 50, tail shuffle above (confirmed)")
    assert choice_branch(12000, 200) == "floyd" and choice_branch(12000, 300) == "tail"
    for case in CASES:
        run_case(*case)


if __name__ == "__main__":
    main()
