#!/usr/bin/env python3
"""Golden vectors for ``EYLoss``, ``BarlowTwinsLoss``, ``VICRegLoss`` and ``SDLLoss`` (cca_zoo/deep/_dcca_ey.py:10-111,
_barlowtwins.py:83-112, _vicreg.py:12-67 and :142-169, _dcca_sdl.py:12-26 and :100-121), captured from the REAL reference in
the build container -> tests/golden/ssl_<tag>.npz.  Import shims as in tools/gen_golden.py, layout as in
tools/gen_golden_tcca.py.

The reference's ``loss`` methods are called unbound on a ``types.SimpleNamespace`` that carries the coefficients.  Every
case (tests/ssl_closed_form.py: CASES) draws its views once, rounds them to float32 and stores them as float32 (``z<i>``;
``zi<i>`` for EY's independent batch).  The reference then runs on the float64 cast (``loss64``, ``<term>64``, ``g64_<i>``,
``gi64_<i>``) and on the float32 arrays (``loss32``, ``<term>32``, ``g32_<i>``, ``gi32_<i>``); ``params`` and ``seed`` are stored
too.  Per case the script asserts that the NumPy closed form is within 1e-12 of the float64 run, and the conditions that keep
a kink of the loss from deciding a test:

* VICReg, d >= 4: both views have columns on both sides of sigma = 1;  every d: no column has |sigma - 1| < 0.05;
* SDL: no off-diagonal covariance is below 1e-3 of the largest of its view.

A draw that violates one is dropped for the next seed (seed = 9000 + 100 * row + attempt; the attempt is printed and stored).

    python tools/gen_golden_ssl.py
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ssl_closed_form import CASES, TERM_KEYS, VICREG_EPS, closed_form  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def reference(kind, params, views, independent):
    ts = [torch.from_numpy(v.copy()).requires_grad_(True) for v in views]
    ti = None if independent is None else [torch.from_numpy(v.copy()).requires_grad_(True) for v in independent]
    if kind == "ey":
        out = DCCA_EY.loss(types.SimpleNamespace(), ts, ti)
    elif kind == "barlow":
        out = BarlowTwins.loss(types.SimpleNamespace(lam=params[0]), ts)
    elif kind == "vicreg":
        out = VICReg.loss(types.SimpleNamespace(sim_coeff=params[0], std_coeff=params[1], cov_coeff=params[2]), ts)
    else:
        out = DCCA_SDL.loss(types.SimpleNamespace(lam=params[0]), ts)
    out["objective"].backward()
    terms = {k: v.detach().numpy().copy() for k, v in out.items()}
    return terms, [t.grad.numpy().copy() for t in ts], None if ti is None else [t.grad.numpy().copy() for t in ti]


def draw(rng, n, m, d, flavour):
    lat = rng.standard_normal((n, 2))
    zs = [lat @ rng.standard_normal((2, d)) + 0.6 * rng.standard_normal((n, d)) + 0.3 * i for i in range(m)]
    if flavour == "bn":
        zs = [(z - z.mean(axis=0)) / z.std(axis=0) for z in zs]
    elif flavour == "offset":
        zs = [z / z.std(axis=0) * (0.7 + 0.8 * ((np.arange(d) + i) % 2)) + rng.uniform(-1.5, 1.5, d) for i, z in enumerate(zs)]
    elif flavour == "scaled":
        zs = [z / z.std(axis=0) * (0.7 + 0.8 * ((np.arange(d) + i) % 2)) for i, z in enumerate(zs)]
    elif flavour == "cancel":
        base = zs[0] / zs[0].std(axis=0) * (0.7 + 0.8 * (np.arange(d) % 2))
        zs = [base, base + 1e-3 * rng.standard_normal((n, d))]
    return [z.astype(np.float32) for z in zs]


def conditions_hold(kind, z32):
    zs = [z.astype(np.float64) for z in z32]
    for z in zs:
        S = np.atleast_2d(np.cov(z.T))
        if kind == "vicreg":
            sig = np.sqrt(np.diag(S) + VICREG_EPS)
            if np.abs(sig - 1.0).min() < 0.05:
                return False
            if z.shape[1] >= 4 and not ((sig < 1.0).any() and (sig > 1.0).any()):
                return False
        if kind == "sdl":
            off = np.abs(S[~np.eye(S.shape[0], dtype=bool)])
            if off.min() < 1e-3 * off.max():
                return False
    return True


for row, (tag, case) in enumerate(CASES.items()):
    kind, n, m, d, params, flavour = case[:6]
    n_ind = case[6] if len(case) > 6 else 0
    for attempt in range(1000):
        seed = 9000 + 100 * row + attempt
        rng = np.random.default_rng(seed)
        z32 = draw(rng, n, m, d, flavour)
        if conditions_hold(kind, z32):
            break
    else:
        sys.exit(f"{tag}: no admissible draw")
    zi32 = draw(rng, n_ind, m, d, flavour) if n_ind else None
    up = lambda vs: None if vs is None else [v.astype(np.float64) for v in vs]   # noqa: E731
    t64, g64, gi64 = reference(kind, params, up(z32), up(zi32))
    t32, g32, gi32 = reference(kind, params, z32, zi32)
    assert t64["objective"].dtype == np.float64 and t32["objective"].dtype == np.float32
    t_cf, g_cf, gi_cf = closed_form(kind, z32, params, zi32)
    worst = max([abs(t_cf[k] - float(t64[k])) / max(abs(float(t64[k])), 1e-300) for k in t64]
                + [relmax(a, b) for a, b in zip(g_cf, g64)] + ([relmax(a, b) for a, b in zip(gi_cf, gi64)] if n_ind else []))
    assert worst < 1e-12, (tag, worst)
    gap = max([relmax(t32[k], t64[k]) for k in t64] + [relmax(a, b) for a, b in zip(g32, g64)])
    store = {"params": np.asarray(params, dtype=np.float64), "seed": np.int64(seed), "loss64": t64["objective"], "loss32": t32["objective"]}
    for k in TERM_KEYS[kind]:
        store[f"{k}64"], store[f"{k}32"] = t64[k], t32[k]
    for i, z in enumerate(z32):
        store[f"z{i}"], store[f"g64_{i}"], store[f"g32_{i}"] = z, g64[i], g32[i]
    if n_ind:
        for i, z in enumerate(zi32):
            store[f"zi{i}"], store[f"gi64_{i}"], store[f"gi32_{i}"] = z, gi64[i], gi32[i]
    path = os.path.join(OUT, f"ssl_{tag}.npz")
    np.savez_compressed(path, **store)
    print(f"ssl_{tag}: seed {seed} (attempt {attempt})  loss64 {float(t64['objective']):.6f}  closed form {worst:.1e}  f32 gap {gap:.1e}  "
          f"{os.path.getsize(path)} bytes")
