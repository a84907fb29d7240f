#!/usr/bin/env python3
"""Measure the VariationalBayesCCA step on one GPU and print one JSON object (``--out`` also writes it).

    python tools/vbcca_probe.py [--out profiles/vbcca_probe.json] [--only device|torch|cpu] [--shape wide|tall] [--k 1,8,32] [--steps 10]

device: whole SVI steps through the C ABI on float32 views drawn on the device (ccz_randn_fill): ms per step between two
        stream synchronisations (the first, untimed call holds the code-object loads), and the achieved bytes per second
        against the model sum_i n p_i 4 bytes per step (ONE read of every view), also as a share of the 8.0 TB/s HBM peak.
        Shapes: wide, n = 4096, 2 x 262144, k in {1, 8, 32}; tall, n = 1e6, 2 x 1024, k = 8.
torch:  the same step in stock torch autograd on the same GPU and the same views: float64 parameters, the reparameterised
        draw, the loss of include/ccz.h, ``backward`` and ``torch.optim.Adam``; the float64 copies of the views are made
        once, outside the timed window.
cpu:    the NumPy restatement (tests/vbcca_restatement.py) on the host threads the environment grants (OMP_NUM_THREADS) at
        n = 512, 2 x 32768, k = 8, scaled by 64 (the ratio of n p) to the wide shape and labelled as scaled.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"wide": (4096, 262144), "tall": (1000000, 1024)}
HBM_PEAK = 8.0e12


def _views(h, n, p):
    import torch

    from cca_zoo_amd import _backend

    views = []
    for i in range(2):
        x = torch.empty(n, p, device="cuda", dtype=torch.float32)
        h.check(h.lib.ccz_randn_fill(h.raw, _backend.F32, C.c_void_p(x.data_ptr()), n, p, p, 91 + i, 0, p, 1.0, 0))
        views.append(x)
    h.sync()
    mus = [v.mean(dim=0) for v in views]
    torch.cuda.synchronize()
    varr = (_backend.View * 2)()
    for i, v in enumerate(views):
        varr[i].data, varr[i].cols, varr[i].ld = v.data_ptr(), p, v.stride(0)
    return views, mus, varr, (C.c_void_p * 2)(*[mu.data_ptr() for mu in mus])


def _svi(h, varr, marr, n, p, k, steps):
    from cca_zoo_amd import _backend

    state = C.c_void_p()
    total = 3 * (steps + 1)
    h.check(h.lib.ccz_svi_create(h.raw, _backend.F32, 2, (C.c_int64 * 2)(p, p), n, k, total, 1e-2, 0, steps, C.byref(state)))
    try:
        size = k + 2 * p * k + 2 * p + n * k
        loc0 = np.random.default_rng(0).uniform(-2.0, 2.0, size=size)
        h.check(h.lib.ccz_svi_set_init(h.raw, state, loc0.ctypes.data_as(C.POINTER(C.c_double))))
        plan = np.empty(5)
        h.check(h.lib.ccz_svi_peek(h.raw, state, 10, plan.ctypes.data_as(C.POINTER(C.c_double))))
        times = []
        a, b = C.c_int64(0), C.c_int(0)
        for rep in range(3):
            h.check(h.lib.ccz_svi_steps(h.raw, state, varr, marr, 1, C.byref(a), C.byref(b)))
            h.sync()
            t0 = time.perf_counter()
            h.check(h.lib.ccz_svi_steps(h.raw, state, varr, marr, steps, C.byref(a), C.byref(b)))
            h.sync()
            if rep:
                times.append(time.perf_counter() - t0)
        done, stop, bad = C.c_int64(0), C.c_int(0), C.c_int64(0)
        h.check(h.lib.ccz_svi_status(h.raw, state, C.byref(done), C.byref(stop), C.byref(bad)))
        ms = min(times) / steps * 1e3
        model = 2 * n * p * 4
        nchunk, ns = int(plan[0]), int(plan[2])
        return {"ms_per_step": round(ms, 4), "tb_per_s": round(model / (ms * 1e-3) / 1e12, 3),
                "share_of_hbm_peak": round(model / (ms * 1e-3) / HBM_PEAK, 4), "timed_runs_ms": [round(t / steps * 1e3, 4) for t in times],
                "model_bytes_per_step": model, "steps_done": int(done.value), "bad_step": int(bad.value),
                "plan": {"row_chunks": nchunk, "rows_per_chunk": int(plan[1]), "strips": ns,
                         "partial_bytes": {"dW": nchunk * 2 * p * k * 8, "ds": nchunk * 2 * p * 8, "dZ": ns * n * k * 8}}}
    finally:
        h.check(h.lib.ccz_svi_destroy(h.raw, state))


def _torch_step(views, mus, n, p, k, steps):
    import torch

    a0 = b0 = 1e-3
    xs = [(v - mu).double() for v, mu in zip(views, mus)]
    g = torch.Generator(device="cuda").manual_seed(0)
    shapes = [(k,), (p, k), (p,), (p, k), (p,), (n, k)]
    loc = [(torch.rand(s, device="cuda", dtype=torch.float64, generator=g) * 4 - 2).requires_grad_(True) for s in shapes]
    rho = [torch.full(s, math.log(math.expm1(0.1)), device="cuda", dtype=torch.float64, requires_grad=True) for s in shapes]
    opt = torch.optim.Adam(loc + rho, lr=1e-2)
    l2pi = math.log(2 * math.pi)

    def step():
        opt.zero_grad(set_to_none=True)
        eps = [torch.randn(s, device="cuda", dtype=torch.float64, generator=g) for s in shapes]
        sc = [torch.nn.functional.softplus(r) for r in rho]
        a, w0, s0, w1, s1, z = [m + s * e for m, s, e in zip(loc, sc, eps)]
        alpha = torch.exp(a)
        lp = (k * (a0 * math.log(b0) - math.lgamma(a0)) + ((a0 - 1) * a - b0 * alpha).sum() + a.sum() + (-0.5 * l2pi - 0.5 * z * z).sum())
        for x, w, s in ((xs[0], w0, s0), (xs[1], w1, s1)):
            r = x - z @ w.T
            lp = lp + (-0.5 * l2pi - s - 0.5 * r * r * torch.exp(-2 * s)).sum() + (-0.5 * l2pi - 0.5 * s * s).sum()
            lp = lp + (-0.5 * l2pi + 0.5 * a - 0.5 * alpha * w * w).sum()
        lq = sum((-0.5 * l2pi - torch.log(s) - 0.5 * e * e).sum() for s, e in zip(sc, eps))
        loss = -(lp - lq)
        loss.backward()
        opt.step()
        return loss

    step()
    torch.cuda.synchronize()
    times = []
    for _ in range(2):
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return {"ms_per_step": round(min(times) / steps * 1e3, 3), "timed_runs_ms": [round(t / steps * 1e3, 3) for t in times],
            "what": "stock torch autograd + torch.optim.Adam, float64 parameters, float64 copies of the centred views made once"}


def device(out, shape, ks, steps, which):
    from cca_zoo_amd import _backend

    h = _backend.default_handle()
    n, p = SHAPES[shape]
    views, mus, varr, marr = _views(h, n, p)
    res = out.setdefault(f"device_{shape}", {"shape": {"n": n, "p": [p, p], "dtype": "float32", "steps": steps}})
    for k in ks:
        entry = res.setdefault(f"k{k}", {})
        if which in (None, "device"):
            entry.update(_svi(h, varr, marr, n, p, k, steps))
        if which in (None, "torch"):
            entry["torch_autograd"] = _torch_step(views, mus, n, p, k, max(2, steps // 3))
            if "ms_per_step" in entry:
                entry["torch_over_device"] = round(entry["torch_autograd"]["ms_per_step"] / entry["ms_per_step"], 2)
    del views, mus


def cpu(out, steps=2):
    import vbcca_restatement as R

    n, p, k = 512, 32768, 8
    rng = np.random.default_rng(0)
    xs = [rng.standard_normal((n, p)).astype(np.float32) for _ in range(2)]
    xc = R.centred(xs, [x.mean(axis=0) for x in xs])
    lay = R.Layout([p, p], n, k)
    st = R.new_state(R.init_loc(rng, lay))
    ts = []
    for t in range(steps + 1):
        t0 = time.perf_counter()
        R.step(lay, st, xc, 0, 1e-2, t)
        ts.append(time.perf_counter() - t0)
    per = float(min(ts[1:]))
    scale = (SHAPES["wide"][0] * SHAPES["wide"][1]) // (n * p)
    out["cpu_comparator"] = {
        "what": f"tests/vbcca_restatement.py step in NumPy float64, 2 x {n} x {p}, k = {k}, scaled x{scale} (the ratio of n p) to the wide shape",
        "threads": os.environ.get("OMP_NUM_THREADS", "unset"), "ms_per_step_measured": round(per * 1e3, 2),
        "ms_per_step_scaled_to_wide": round(per * scale * 1e3, 1), "scaled": True,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only", choices=["device", "torch", "cpu"])
    ap.add_argument("--shape", choices=["wide", "tall"], help="device part: this shape alone")
    ap.add_argument("--k", help="wide shape: comma-separated latent dimensions (default 1,8,32)")
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    out = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    if a.only in (None, "device", "torch"):
        for shape in ([a.shape] if a.shape else ["wide", "tall"]):
            ks = [int(x) for x in a.k.split(",")] if (a.k and shape == "wide") else ([1, 8, 32] if shape == "wide" else [8])
            device(out, shape, ks, a.steps, a.only)
    if a.only in (None, "cpu"):
        cpu(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=2)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
