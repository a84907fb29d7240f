#!/usr/bin/env python3
"""Measure the device CP-ALS and ``TCCA.fit`` on one GPU and print one JSON object (``--out`` also writes it).

    python tools/tcca_fit_probe.py [--out profiles/tcca_fit_probe.json] [--iters 20] [--parts iterations,fit,torch,numpy]

- ``iterations``: ms per CP-ALS iteration through the C ABI (``tol = 0`` so that the fit never stops early; one chunk of
  ``iters`` iterations between two stream synchronisations, after an untimed warm-up chunk) for tensors of 3 x 256
  (2^24 entries) at k = 8 and 32 and of 3 x 64 at k = 8, with the achieved fp64 rate of the MTTKRPs against their model of
  ``2 k prod d`` flop per mode and the rate at which the unfoldings are read (``8 prod d`` bytes per mode).  The shares of
  the MTTKRP and of the small kernels come from a kernel trace of the same command taken in a run of its own
  (``rocprofv3 --kernel-trace --stats -- python tools/tcca_fit_probe.py --parts iterations``): the kernels are
  ``k_cp_mttkrp``, ``k_cp_fold`` and ``k_cp_update``.
- ``fit``: the whole ``TCCA(latent_dimensions=8).fit`` at n = 1e6, three float32 CUDA views of width 64.
- ``torch``: the same iteration at 3 x 64, k = 8 as a plain ``einsum`` restatement on the same GPU.
- ``numpy``: the NumPy restatement's iteration (tests/tcca_fit_restatement.py) on the host's cores at 3 x 64, k = 8.

Nothing is gated on these times."""

from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _tensor(d, k, device):
    """A planted rank-k tensor of three modes of width d plus noise, float64."""
    import torch

    g = torch.Generator(device=device).manual_seed(d + k)
    A = [torch.linalg.qr(torch.randn(d, k, device=device, dtype=torch.float64, generator=g))[0] for _ in range(3)]
    w = 1.1 ** -torch.arange(k, device=device, dtype=torch.float64)
    T = torch.einsum("r,ar,br,cr->abc", w, *A)
    return (T + 0.02 * T.norm() / d ** 1.5 * torch.randn(d, d, d, device=device, dtype=torch.float64, generator=g)).contiguous()


def probe_iterations(d, k, iters):
    import torch

    from cca_zoo_amd import _backend

    M = _tensor(d, k, "cuda")
    h = _backend.handle_for([M])
    state = C.c_void_p()
    dims = (C.c_int64 * 3)(d, d, d)
    total = 2 * iters
    h.check(h.lib.ccz_cp_create(h.raw, 3, dims, k, 0.0, total, iters, C.byref(state)))
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.check(h.lib.ccz_cp_setup(h.raw, state, C.c_void_p(M.data_ptr())))
        h.sync()
        setup_ms = (time.perf_counter() - t0) * 1e3
        a, b = C.c_int64(0), C.c_int(0)
        h.check(h.lib.ccz_cp_iterations(h.raw, state, iters, C.byref(a), C.byref(b)))     # warm-up chunk
        h.sync()
        t0 = time.perf_counter()
        h.check(h.lib.ccz_cp_iterations(h.raw, state, iters, C.byref(a), C.byref(b)))
        h.sync()
        ms = (time.perf_counter() - t0) * 1e3 / iters
        it, st = C.c_int64(0), C.c_int(0)
        h.check(h.lib.ccz_cp_status(h.raw, state, C.byref(it), C.byref(st), None, None, None))
        assert it.value == total, (it.value, total)
    finally:
        h.check(h.lib.ccz_cp_destroy(h.raw, state))
    flop, byts = 3 * 2.0 * k * d ** 3, 3 * 8.0 * d ** 3
    return {"dims": [d, d, d], "k": k, "setup_ms_first_call": round(setup_ms, 3), "ms_per_iteration": round(ms, 4),
            "mttkrp_model_tflops_fp64_over_whole_iteration": round(flop / ms / 1e9, 3),
            "unfoldings_read_tb_per_s_over_whole_iteration": round(byts / ms / 1e9, 3)}


def probe_fit(n, d, k):
    import torch

    from cca_zoo_amd.linear import TCCA

    g = torch.Generator(device="cuda").manual_seed(1)
    lat = torch.empty(n, k, device="cuda").exponential_(generator=g) - 1.0
    views = [(lat @ torch.randn(k, d, device="cuda", generator=g) + 0.6 * torch.randn(n, d, device="cuda", generator=g) + 0.3 * i)
             for i in range(3)]
    TCCA(latent_dimensions=k).fit([v[:4096] for v in views])        # code objects
    times = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model = TCCA(latent_dimensions=k).fit(views)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"what": "TCCA.fit, CUDA float32 views", "n": n, "dims": [d, d, d], "k": k, "fit_ms": [round(t, 2) for t in times],
            "n_iter": int(model.n_iter_)}


def probe_torch(d, k, iters):
    import torch

    M = _tensor(d, k, "cuda")
    A = [torch.linalg.svd(M.movedim(m, 0).reshape(d, -1), full_matrices=False)[0][:, :k].contiguous() for m in range(3)]
    subs = ("abc,br,cr->ar", "abc,ar,cr->br", "abc,ar,br->cr")

    def iteration():
        for m in range(3):
            o = [A[i] for i in range(3) if i != m]
            P = (o[0].T @ o[0]) * (o[1].T @ o[1])
            G = torch.einsum(subs[m], M, *o)
            A[m] = torch.linalg.solve(P.T, G.T).T

    for _ in range(3):
        iteration()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        iteration()
    torch.cuda.synchronize()
    return {"what": "torch einsum restatement of one iteration, same GPU", "dims": [d, d, d], "k": k,
            "ms_per_iteration": round((time.perf_counter() - t0) * 1e3 / iters, 4)}


def probe_numpy(d, k, iters):
    from tcca_fit_restatement import cp_als

    M = _tensor(d, k, "cpu").numpy()
    cp_als(M, k, n_iter_max=1)
    t0 = time.perf_counter()
    cp_als(M, k, n_iter_max=iters, tol=0.0)
    return {"what": "NumPy restatement (includes one SVD init), host cores", "dims": [d, d, d], "k": k, "cores": os.cpu_count(),
            "threads": os.environ.get("OMP_NUM_THREADS"), "ms_per_iteration": round((time.perf_counter() - t0) * 1e3 / iters, 3)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--parts", default="iterations,fit,torch,numpy")
    a = ap.parse_args(argv)
    parts = a.parts.split(",")
    res = {}
    if "iterations" in parts:
        res["iterations"] = [probe_iterations(256, 8, a.iters), probe_iterations(256, 32, a.iters), probe_iterations(64, 8, a.iters)]
    if "fit" in parts:
        res["fit"] = probe_fit(1_000_000, 64, 8)
    if "torch" in parts:
        res["torch_einsum_3x64_k8"] = probe_torch(64, 8, a.iters)
    if "numpy" in parts:
        res["numpy_3x64_k8"] = probe_numpy(64, 8, max(2, a.iters // 4))
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
