#!/usr/bin/env python3
"""Measure the ProbabilisticCCA leapfrog on one GPU and print one JSON object (``--out`` also writes it).

    python tools/pcca_probe.py [--out profiles/pcca_probe.json] [--only device|torch] [--shape wide|tall] [--k 1,8] [--steps 10]

device: leapfrog steps through the C ABI (``ccz_nuts_leapfrog``, the test seam: exactly what ``ccz_nuts_run`` takes per leaf,
        the record read included) on float32 views drawn on the device: ms per leapfrog, the achieved bytes per second
        against the model sum_i n p_i 4 bytes (ONE read of every view), also as a share of the 8.0 TB/s HBM peak.
        ``record_read_ms`` is the same record read on an idle stream (the copy through the pinned buffer and the host's
        wake-up, no kernel in front of it); ``host_wait_share`` is that over the leapfrog.  Beside it VariationalBayesCCA's
        step at the same shape, re-measured in the same run (``tools/vbcca_probe.py``'s routine).
        Shapes: wide, n = 4096, 2 x 262144, k in {1, 8}; tall, n = 1e6, 2 x 1024, k = 8.
torch:  the same potential and its gradient in stock torch autograd on the same GPU and the same views: float64 state, the
        float64 copies of the centred views made once, outside the timed window.
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vbcca_probe import HBM_PEAK, SHAPES, _svi, _views  # noqa: E402


def _nuts(h, varr, marr, n, p, k, steps):
    from cca_zoo_amd import _backend

    pd = C.POINTER(C.c_double)
    state = C.c_void_p()
    h.check(h.lib.ccz_nuts_create(h.raw, _backend.F32, 2, (C.c_int64 * 2)(p, p), n, k, 0, 1, 10, 0.8, 0, C.byref(state)))
    try:
        size = 2 * p * k + 2 * p + n * k
        q0 = np.random.default_rng(0).uniform(-1.0, 1.0, size=size)
        u0 = C.c_double(0.0)
        h.check(h.lib.ccz_nuts_set_init(h.raw, state, varr, marr, q0.ctypes.data_as(pd), C.byref(u0)))
        h.check(h.lib.ccz_nuts_set_adapt(h.raw, state, 1e-4, None))
        rec = np.zeros(27)

        def leaf(begin, i):
            h.check(h.lib.ccz_nuts_leapfrog(h.raw, state, varr, marr, 0, begin, 1, i, 10, rec.ctypes.data_as(pd)))

        leaf(1, 0)                       # untimed: the code-object loads and the momentum draw
        times = []
        for _ in range(2):
            t0 = time.perf_counter()
            for i in range(steps):
                leaf(0, 1 + i)
            times.append(time.perf_counter() - t0)
        ms = min(times) / steps * 1e3
        out26 = np.zeros(26)
        h.sync()
        reads = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(50):
                h.check(h.lib.ccz_nuts_peek(h.raw, state, 101, out26.ctypes.data_as(pd)))
            reads.append((time.perf_counter() - t0) / 50)
        read_ms = min(reads) * 1e3
        model = 2 * n * p * 4
        return {"ms_per_leapfrog": round(ms, 4), "tb_per_s": round(model / (ms * 1e-3) / 1e12, 3),
                "share_of_hbm_peak": round(model / (ms * 1e-3) / HBM_PEAK, 4), "timed_runs_ms": [round(t / steps * 1e3, 4) for t in times],
                "record_read_ms": round(read_ms, 4), "host_wait_share": round(read_ms / ms, 4), "model_bytes_per_leapfrog": model,
                "initial_potential": u0.value, "last_H_finite": bool(rec[25])}
    finally:
        h.check(h.lib.ccz_nuts_destroy(h.raw, state))


def _torch_potential(views, mus, n, p, k, steps):
    import torch

    xs = [(v - mu).double() for v, mu in zip(views, mus)]
    g = torch.Generator(device="cuda").manual_seed(0)
    shapes = [(p, k), (p,), (p, k), (p,), (n, k)]
    q = [(torch.rand(s, device="cuda", dtype=torch.float64, generator=g) * 2 - 1).requires_grad_(True) for s in shapes]
    l2pi = math.log(2 * math.pi)

    def grad():
        w0, s0, w1, s1, z = q
        u = 0.5 * sum((t * t).sum() for t in q) + 0.5 * l2pi * (sum(t.numel() for t in q) + 2 * n * p)
        for x, w, s in ((xs[0], w0, s0), (xs[1], w1, s1)):
            r = x - z @ w.T
            u = u + (n * s).sum() + 0.5 * (r * r * torch.exp(-2 * s)).sum()
        return torch.autograd.grad(u, q)

    grad()
    torch.cuda.synchronize()
    times = []
    for _ in range(2):
        t0 = time.perf_counter()
        for _ in range(steps):
            grad()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return {"ms_per_gradient": round(min(times) / steps * 1e3, 3), "timed_runs_ms": [round(t / steps * 1e3, 3) for t in times],
            "what": "the same potential through stock torch autograd, float64 state, float64 copies of the centred views made once"}


def device(out, shape, ks, steps, which):
    from cca_zoo_amd import _backend

    h = _backend.default_handle()
    n, p = SHAPES[shape]
    views, mus, varr, marr = _views(h, n, p)
    res = out.setdefault(f"device_{shape}", {"shape": {"n": n, "p": [p, p], "dtype": "float32", "steps": steps}})
    for k in ks:
        entry = res.setdefault(f"k{k}", {})
        if which in (None, "device"):
            entry.update(_nuts(h, varr, marr, n, p, k, steps))
            svi = _svi(h, varr, marr, n, p, k, steps)
            entry["vbcca_step_same_run"] = {"ms_per_step": svi["ms_per_step"], "timed_runs_ms": svi["timed_runs_ms"]}
            entry["leapfrog_over_vbcca_step"] = round(entry["ms_per_leapfrog"] / svi["ms_per_step"], 3)
        if which in (None, "torch"):
            entry["torch_autograd"] = _torch_potential(views, mus, n, p, k, max(2, steps // 3))
            if "ms_per_leapfrog" in entry:
                entry["torch_over_device"] = round(entry["torch_autograd"]["ms_per_gradient"] / entry["ms_per_leapfrog"], 2)
    del views, mus


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only", choices=["device", "torch"])
    ap.add_argument("--shape", choices=["wide", "tall"], help="this shape alone")
    ap.add_argument("--k", help="wide shape: comma-separated latent dimensions (default 1,8)")
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    out = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    for shape in ([a.shape] if a.shape else ["wide", "tall"]):
        ks = [int(x) for x in a.k.split(",")] if (a.k and shape == "wide") else ([1, 8] if shape == "wide" else [8])
        device(out, shape, ks, a.steps, a.only)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=2)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
