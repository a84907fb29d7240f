#!/usr/bin/env python3
"""Golden vectors for the deep objectives on bfloat16 / float16 batches -> tests/golden/half_<type>_<case>.npz.

The REAL reference objectives (cca_zoo/deep/objectives.py: CCALoss, MCCALoss, GCCALoss, TCCALoss; the ``loss`` methods of
_dcca_ey.py, _barlowtwins.py, _vicreg.py, _dcca_sdl.py) run in float64 on the CPU at inputs that were ROUNDED TO THE HALF TYPE
first, so a golden says what the exact objective is at the very numbers a half batch holds.  Import shims as in
tools/gen_golden_ssl.py; the reference source never travels, only these data files are committed.

Stored per case: ``z<i>`` the inputs as uint16 bit patterns of the half type, ``loss`` (float64), the loss's terms by their
reference names (float64; moment-map losses only), ``g<i>`` the gradients (the float64 results stored as float32: 2^-24 against a
test bar of 2^-11 and wider), ``eps`` / ``params``, ``seed``.

Cases, each for both types:  cca 300 x (20, 12);  mcca 257 x (7, 5, 9);  gcca 257 x (6, 6, 6);  tcca 129 x (4, 3, 5);  ey, barlow,
vicreg, sdl at 301 x 2 x 16 on ONE shared draw;  and one offset case per family whose column means are about 20 sigma (cca, gcca,
tcca, ey), at smaller shapes.  A draw on which VICReg or SDL sits on a kink (as in tools/gen_golden_ssl.py) is dropped for the
next seed.

    python tools/gen_golden_half.py --reference /path/to/the/reference/checkout
"""
import argparse
import importlib.machinery
import importlib.metadata as md
import os
import sys
import types

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reference", required=True, help="checkout of the reference project (the directory that holds cca_zoo/)")
ARGS = ap.parse_args()
sys.dont_write_bytecode = True
if not os.path.isdir(os.path.join(ARGS.reference, "cca_zoo")):
    sys.exit("no cca_zoo/ under --reference; goldens can only be regenerated next to the reference")
sys.path.insert(0, ARGS.reference)
_orig_version = md.version
md.version = lambda name: "0.0.0+oracle" if name == "cca_zoo" else _orig_version(name)
_tl = types.ModuleType("tensorly")
_tl.set_backend = lambda *a, **k: None
_dec = types.ModuleType("tensorly.decomposition")
_dec.parafac = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("tensorly stub"))
_tl.decomposition = _dec
sys.modules["tensorly"] = _tl
sys.modules["tensorly.decomposition"] = _dec

import torch  # noqa: E402

if "lightning" not in sys.modules:      # shim: the model classes import the Lightning base class only to subclass it
    _l = types.ModuleType("lightning")
    _l.__spec__ = importlib.machinery.ModuleSpec("lightning", None)
    _lp = types.ModuleType("lightning.pytorch")
    _lp.__spec__ = importlib.machinery.ModuleSpec("lightning.pytorch", None)
    _lp.LightningModule = torch.nn.Module
    _l.pytorch = _lp
    sys.modules["lightning"] = _l
    sys.modules["lightning.pytorch"] = _lp

from cca_zoo.deep._barlowtwins import BarlowTwins  # noqa: E402
from cca_zoo.deep._dcca_ey import DCCA_EY  # noqa: E402
from cca_zoo.deep._dcca_sdl import DCCA_SDL  # noqa: E402
from cca_zoo.deep._vicreg import VICReg  # noqa: E402
from cca_zoo.deep.objectives import CCALoss, GCCALoss, MCCALoss, TCCALoss  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
TYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
VICREG_EPS = 1e-4

# (case, family, rows, widths, eps or params, offset in sigma)
CASES = (
    ("cca", "cca", 300, (20, 12), 1e-4, 0.0),
    ("mcca", "mcca", 257, (7, 5, 9), 1e-4, 0.0),
    ("gcca", "gcca", 257, (6, 6, 6), 1e-4, 0.0),
    ("tcca", "tcca", 129, (4, 3, 5), 1e-4, 0.0),
    ("ey", "ey", 301, (16, 16), (), 0.0),
    ("barlow", "barlow", 301, (16, 16), (5e-3,), 0.0),
    ("vicreg", "vicreg", 301, (16, 16), (25.0, 25.0, 1.0), 0.0),
    ("sdl", "sdl", 301, (16, 16), (0.5,), 0.0),
    ("cca_offset", "cca", 120, (8, 6), 1e-4, 20.0),
    ("gcca_offset", "gcca", 100, (4, 4, 4), 1e-4, 20.0),
    ("tcca_offset", "tcca", 65, (3, 2, 3), 1e-4, 20.0),
    ("ey_offset", "ey", 101, (8, 8), (), 20.0),
)
MOMENT = ("ey", "barlow", "vicreg", "sdl")


def draw(rng, n, dims, offset):
    """two shared latents + noise, every column scaled to sigma 0.7 or 1.5 (VICReg's hinge has both sides), then shifted"""
    lat = rng.standard_normal((n, 2))
    zs = []
    for i, d in enumerate(dims):
        z = lat @ rng.standard_normal((2, d)) + 0.6 * rng.standard_normal((n, d))
        z = (z - z.mean(axis=0)) / z.std(axis=0) * (0.7 + 0.8 * ((np.arange(d) + i) % 2))
        zs.append(z + offset * np.sign(rng.standard_normal(d)) * (0.7 + 0.8 * ((np.arange(d) + i) % 2)) if offset else z)
    return zs


def kinks_clear(family, zs):
    for z in zs:
        S = np.atleast_2d(np.cov(z.T))
        if family == "vicreg" and np.abs(np.sqrt(np.diag(S) + VICREG_EPS) - 1.0).min() < 0.05:
            return False
        if family == "sdl":
            off = np.abs(S[~np.eye(S.shape[0], dtype=bool)])
            if off.min() < 1e-3 * off.max():
                return False
    return True


def reference(family, par, views):
    ts = [torch.from_numpy(v.copy()).requires_grad_(True) for v in views]
    terms = {}
    if family == "cca":
        loss = CCALoss(eps=par)(ts)
    elif family == "mcca":
        loss = MCCALoss(eps=par)(ts)
    elif family == "gcca":
        loss = GCCALoss(eps=par)(ts)
    elif family == "tcca":
        loss = TCCALoss(eps=par)(ts)
    else:
        if family == "ey":
            out = DCCA_EY.loss(types.SimpleNamespace(), ts, None)
        elif family == "barlow":
            out = BarlowTwins.loss(types.SimpleNamespace(lam=par[0]), ts)
        elif family == "vicreg":
            out = VICReg.loss(types.SimpleNamespace(sim_coeff=par[0], std_coeff=par[1], cov_coeff=par[2]), ts)
        else:
            out = DCCA_SDL.loss(types.SimpleNamespace(lam=par[0]), ts)
        loss = out["objective"]
        terms = {k: np.float64(v.detach().numpy()) for k, v in out.items() if k != "objective"}
    loss.backward()
    assert loss.dtype == torch.float64
    return np.float64(loss.detach().numpy()), terms, [t.grad.numpy().copy() for t in ts]


total = 0
for tname, tdt in TYPES.items():
    shared = {}                                        # the moment-map losses share one draw per type
    for row, (case, family, n, dims, par, offset) in enumerate(CASES):
        key = (n, dims, offset) if family in MOMENT else None
        for attempt in range(1000):
            seed = 11000 + 100 * row + attempt if key not in shared else shared[key]
            rng = np.random.default_rng(seed)
            half = [torch.from_numpy(z).to(tdt) for z in draw(rng, n, dims, offset)]       # the rounding to the half type
            z64 = [h.to(torch.float64).numpy() for h in half]
            if all(kinks_clear(f, z64) for f in (MOMENT if family in MOMENT else (family,))):
                break
            assert key not in shared, (case, "the shared draw sits on a kink")
        else:
            sys.exit(f"{case}: no admissible draw")
        if key is not None:
            shared[key] = seed
        loss, terms, grads = reference(family, par, z64)
        store = {"loss": loss, "seed": np.int64(seed), "dtype": np.array(tname)}
        store["params" if family in MOMENT else "eps"] = np.asarray(par, dtype=np.float64)
        store.update(terms)
        for i, (h, g) in enumerate(zip(half, grads)):
            store[f"z{i}"] = h.view(torch.int16).numpy().view(np.uint16)
            store[f"g{i}"] = g.astype(np.float32)
        path = os.path.join(OUT, f"half_{tname}_{case}.npz")
        np.savez_compressed(path, **store)
        total += os.path.getsize(path)
        print(f"half_{tname}_{case}: seed {seed}  loss {float(loss):.6f}  max|g| {max(np.abs(g).max() for g in grads):.3e}  "
              f"{os.path.getsize(path)} bytes")
print("total", total, "bytes")
