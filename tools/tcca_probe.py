#!/usr/bin/env python3
"""Measure ``TCCALoss`` forward + backward on one GPU and print one JSON object (``--out`` also writes it).

    python tools/tcca_probe.py [--out profiles/tcca_probe.json] [--iters 20]

Batch 8192, three float32 views of width 32 and of width 64.  Per shape: ms per forward + backward call between two stream
synchronisations (after untimed warm-up calls, which hold the code-object loads), and -- timed separately on the same whitened
views -- ``ccz_kr_moment``, the three ``ccz_kr_apply`` calls and the three ``ccz_syevj`` calls, as shares of the call, with
the achieved fp64 flop rate of the two products against their model of ``2 n prod d`` flop each.  At 3 x 32 a plain torch
restatement of the reference's forward (whitening by ``eigh``, the ``n x d x d x d`` outer-product tensor -- 1 GB in float32
there --, its mean and norm) and its autograd run on the same GPU for comparison.  Nothing is gated on these times.
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 8192


def _views(d, dtype):
    import torch

    g = torch.Generator(device="cuda").manual_seed(d)
    lat = torch.randn(N, 2, device="cuda", generator=g)
    return [(lat @ torch.randn(2, d, device="cuda", generator=g) + 0.6 * torch.randn(N, d, device="cuda", generator=g) + 0.3 * i).to(dtype)
            for i in range(3)]


def _time(fn, iters, warmup=3):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def _torch_reference(zs, eps):
    """The reference's arithmetic (cca_zoo/deep/objectives.py:260-289) restated in plain torch."""
    import torch

    n = zs[0].shape[0]
    hs = []
    for z in zs:
        zc = z - z.mean(dim=0)
        cov = zc.T @ zc / (n - 1) + eps * torch.eye(z.shape[1], device=z.device, dtype=z.dtype)
        lam, vec = torch.linalg.eigh(cov)
        hs.append(zc @ (vec @ torch.diag(torch.clamp(lam, min=eps).rsqrt()) @ vec.T))
    m = hs[0]
    for hi in hs[1:]:
        m = m.unsqueeze(-1) * hi.reshape(n, *([1] * (m.dim() - 1)), hi.shape[1])
    return -torch.linalg.norm(m.mean(dim=0))


def probe_shape(d, iters):
    import torch

    from cca_zoo_amd import _backend
    from cca_zoo_amd.deep import TCCALoss
    from cca_zoo_amd.deep.objectives import _views_of

    zs = [z.requires_grad_(True) for z in _views(d, torch.float32)]
    loss_fn = TCCALoss(eps=1e-5)

    def step():
        for z in zs:
            z.grad = None
        loss_fn(zs).backward()

    total = _time(step, iters)
    h = _backend.handle_for(zs)
    hs = [torch.randn(N, d, device="cuda", dtype=torch.float64) / d ** 0.5 for _ in range(3)]
    views = _views_of(hs)
    M = torch.empty((d, d, d), dtype=torch.float64, device="cuda")
    out = torch.empty((N, d), dtype=torch.float64, device="cuda")
    cov = [(x.T @ x / N).contiguous() for x in hs]
    w = torch.empty(d, dtype=torch.float64, device="cuda")
    V = torch.empty((d, d), dtype=torch.float64, device="cuda")

    def moment():
        h.check(h.lib.ccz_kr_moment(h.raw, views, 3, N, 1.0 / N, C.c_void_p(M.data_ptr())))

    def applies():
        for mode in range(3):
            h.check(h.lib.ccz_kr_apply(h.raw, views, 3, N, C.c_void_p(M.data_ptr()), mode, 1.0 / N, C.c_void_p(out.data_ptr()), d))

    def evds():
        for c in cov:
            a = c.clone()
            h.check(h.lib.ccz_syevj(h.raw, C.c_void_p(a.data_ptr()), d, C.c_void_p(w.data_ptr()), C.c_void_p(V.data_ptr()), None))

    flop = 2.0 * N * d ** 3
    t_m, t_a, t_e = _time(moment, iters), _time(applies, iters), _time(evds, iters)
    return {
        "batch": N, "dims": [d, d, d], "dtype": "float32", "ms_per_forward_backward": round(total, 4),
        "ccz_kr_moment": {"ms": round(t_m, 4), "share": round(t_m / total, 3), "tflops_fp64": round(flop / t_m / 1e9, 2)},
        "ccz_kr_apply_x3": {"ms": round(t_a, 4), "share": round(t_a / total, 3), "tflops_fp64": round(3 * flop / t_a / 1e9, 2)},
        "ccz_syevj_x3": {"ms": round(t_e, 4), "share": round(t_e / total, 3)},
    }


def probe_torch(d, iters):
    import torch

    zs = [z.requires_grad_(True) for z in _views(d, torch.float32)]

    def step():
        for z in zs:
            z.grad = None
        _torch_reference(zs, 1e-5).backward()

    return {"what": "plain torch restatement of the reference's forward + autograd, same GPU", "batch": N, "dims": [d, d, d],
            "dtype": "float32", "outer_product_tensor_bytes": N * d ** 3 * 4, "ms_per_forward_backward": round(_time(step, iters, warmup=2), 4)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args(argv)
    res = {"shapes": [probe_shape(32, a.iters), probe_shape(64, a.iters)], "torch_reference_3x32": probe_torch(32, max(2, a.iters // 4))}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
