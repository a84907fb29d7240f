#!/usr/bin/env python3
"""Measure ``EYLoss``, ``BarlowTwinsLoss``, ``VICRegLoss`` and ``SDLLoss`` forward + backward on one GPU and print one JSON object
(``--out`` also writes it).

    python tools/ssl_loss_probe.py [--out profiles/ssl_loss_probe.json] [--runs 7] [--iters 200]

Shape: 2 float32 views of 8192 rows x 512 columns (BASELINE configs[3], the DCCA batch).  Per loss: the median over ``--runs``
runs (after 2 untimed warm-up runs, which hold the code-object loads) of the ms per forward + backward call, each run ``--iters``
calls between two stream synchronisations, alternating with a stock-torch restatement of the reference's ``loss`` body
(cca_zoo/deep/_dcca_ey.py:10-111, _barlowtwins.py:83-112, _vicreg.py:12-67 and :142-169, _dcca_sdl.py:12-26 and :100-121) and
its autograd on the same device in the same process.  ``dispatches`` is the number of device kernels of ONE forward + backward
call, counted by torch's profiler in a separate, untimed call (null where the profiler is not available).  Nothing is gated on
these figures.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D = 8192, 512


def _views():
    import torch

    g = torch.Generator(device="cuda").manual_seed(4)
    base = torch.randn(N, D, device="cuda", generator=g)
    scale = 0.7 + 0.8 * (torch.arange(D, device="cuda") % 2)
    z1 = base * scale
    z2 = (0.8 * base + 0.6 * torch.randn(N, D, device="cuda", generator=g)) * scale.flip(0)
    return [z1.requires_grad_(True), z2.requires_grad_(True)]


def _cov(z):
    c = z - z.mean(dim=0)
    return c.T @ c / (z.shape[0] - 1)


def _torch_loss(kind, zs):
    """The reference's arithmetic restated in plain torch (same products, masks and reductions)."""
    import torch

    n, d = zs[0].shape
    if kind == "ey":
        zc = [z - z.mean(dim=0) for z in zs]
        v = sum(c.T @ c / (n - 1) for c in zc) / len(zs)
        c = sum(a.T @ b / (n - 1) for a in zc for b in zc) / len(zs)
        return -torch.trace(2.0 * c) + torch.trace(v @ v)
    mask = ~torch.eye(d, dtype=torch.bool, device=zs[0].device)
    if kind == "barlow":
        cc = zs[0].T @ zs[1] / n
        return torch.sum((1.0 - torch.diag(cc)) ** 2) + 5e-3 * torch.sum(cc[mask] ** 2)
    sq = torch.nn.functional.mse_loss(zs[0], zs[1])
    if kind == "vicreg":
        var = sum(torch.mean(torch.relu(1.0 - torch.sqrt(z.var(dim=0) + 1e-4))) for z in zs)
        cov = sum(_cov(z)[mask].pow(2).sum() / d for z in zs)
        return 25.0 * sq + 25.0 * var + 1.0 * cov
    return sq + 0.5 * sum(torch.cov(z.T)[mask].abs().mean() for z in zs)


def _run_ms(fn, iters):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def _dispatches(fn):
    import torch

    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception as e:       # the profiler is an aid here, not the measurement
        print(f"dispatch count not available: {e}", file=sys.stderr)
        return None


def probe(kind, runs, iters):
    import torch

    from cca_zoo_amd import deep

    mod = {"ey": deep.EYLoss, "barlow": deep.BarlowTwinsLoss, "vicreg": deep.VICRegLoss, "sdl": deep.SDLLoss}[kind]()
    zs = _views()

    def ours():
        for z in zs:
            z.grad = None
        mod(zs).backward()

    def stock():
        for z in zs:
            z.grad = None
        _torch_loss(kind, zs).backward()

    ours()
    g_ours = [z.grad.clone() for z in zs]
    stock()
    gap = max(float((a - z.grad).abs().max() / z.grad.abs().max()) for a, z in zip(g_ours, zs))
    a, b = [], []
    for r in range(runs + 2):            # alternating, the first two runs of each are warm-up
        ta, tb = _run_ms(ours, iters), _run_ms(stock, iters)
        if r >= 2:
            a.append(ta)
            b.append(tb)
    return {"loss": kind, "batch": N, "dims": [D, D], "dtype": "float32",
            "ms_per_forward_backward": round(statistics.median(a), 4), "ms_min_max": [round(min(a), 4), round(max(a), 4)],
            "torch_ms_per_forward_backward": round(statistics.median(b), 4), "torch_ms_min_max": [round(min(b), 4), round(max(b), 4)],
            "gradient_distance_to_torch_float32": gap, "dispatches": _dispatches(ours), "torch_dispatches": _dispatches(stock)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args(argv)
    if a.runs < 5:
        ap.error("--runs: at least 5 timed runs")
    res = {"losses": [probe(k, a.runs, a.iters) for k in ("ey", "barlow", "vicreg", "sdl")]}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
