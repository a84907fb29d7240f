#!/usr/bin/env python3
"""Golden vectors for ``TCCALoss`` (cca_zoo/deep/objectives.py:256-289), captured from the REAL reference in the build
container -> tests/golden/tcca_<tag>.npz.  Same import shims as tools/gen_golden_deep_score.py.

Every case draws its views as ``latent @ W + 0.6 noise + 0.3 i`` with two shared latents, rounds them to float32 and stores
them once as float32 (``z<i>``).  The reference then runs on the float64 cast (``loss64``, ``g64_<i>``: float64) and on the
float32 arrays (``loss32``, ``g32_<i>``: float32); ``eps`` is stored too.  Per case the script asserts that the NumPy closed
form (tests/tcca_closed_form.py) is within 1e-10 of the float64 run and that the reference's float32-vs-float64 gradient gap
is below 1e-4 (the case is well conditioned).  No draw needed another seed: every case uses seed 7000 + its row number.

    python tools/gen_golden_tcca.py
"""
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
from cca_zoo.deep.objectives import TCCALoss  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tcca_closed_form import tcca_loss_closed_form  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CASES = (
    ("three", 96, (5, 4, 3), 1e-5),
    ("two", 64, (6, 4), 1e-4),
    ("four", 80, (3, 2, 4, 3), 1e-5),
    ("three17", 200, (17, 16, 9), 1e-5),
    ("odd", 70, (33, 2, 5), 1e-3),
    ("one_col", 33, (4, 1, 3), 1e-5),
    ("wide_last", 120, (2, 3, 40), 1e-4),
    ("tall", 4100, (3, 2, 2), 1e-5),
)


def relmax(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(np.asarray(b, np.float64)).max())


def reference(views, eps):
    ts = [torch.from_numpy(v.copy()).requires_grad_(True) for v in views]
    loss = TCCALoss(eps=eps)(ts)
    loss.backward()
    return loss.detach().numpy().copy(), [t.grad.numpy().copy() for t in ts]


for row, (tag, n, dims, eps) in enumerate(CASES):
    rng = np.random.default_rng(7000 + row)
    lat = rng.standard_normal((n, 2))
    z32 = [(lat @ rng.standard_normal((2, d)) + 0.6 * rng.standard_normal((n, d)) + 0.3 * i).astype(np.float32)
           for i, d in enumerate(dims)]
    loss64, g64 = reference([z.astype(np.float64) for z in z32], eps)
    loss32, g32 = reference(z32, eps)
    assert loss64.dtype == np.float64 and loss32.dtype == np.float32
    l_cf, g_cf = tcca_loss_closed_form(z32, eps)
    worst = max([abs(l_cf - float(loss64)) / abs(float(loss64))] + [relmax(a, b) for a, b in zip(g_cf, g64)])
    gap = max([abs(float(loss32) - float(loss64)) / abs(float(loss64))] + [relmax(a, b) for a, b in zip(g32, g64)])
    assert worst < 1e-10, (tag, worst)
    assert gap < 1e-4, (tag, gap)
    store = {"eps": np.float64(eps), "loss64": loss64, "loss32": loss32}
    for i, z in enumerate(z32):
        store[f"z{i}"], store[f"g64_{i}"], store[f"g32_{i}"] = z, g64[i], g32[i]
    path = os.path.join(OUT, f"tcca_{tag}.npz")
    np.savez_compressed(path, **store)
    print(f"tcca_{tag}: loss64 {float(loss64):.6f}  closed form {worst:.1e}  f32 gap {gap:.1e}  {os.path.getsize(path)} bytes")
