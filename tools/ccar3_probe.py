#!/usr/bin/env python3
"""Measure the device ADMM of CCAR3 (csrc/rrr.hip) on one GPU and print one JSON object (``--out`` also writes it).

    python tools/ccar3_probe.py [--out profiles/ccar3_probe.json] [--iters 50] [--parts iterations,setup,torch,numpy]

- ``iterations``: ms per ADMM iteration through the C ABI (``tol = 0`` so that the fit never stops early; one chunk of
  ``iters`` iterations between two stream synchronisations, after an untimed warm-up chunk) at (p, q) = (4096, 64),
  (16320, 64) -- the largest p that ``p + q <= 16384`` leaves at q = 64 -- and (512, 16).  Beside it the traffic model:
  one iteration reads ``M`` once, ``8 p^2`` bytes (HBM-bound once ``M`` outgrows the caches), and does ``2 p^2 q`` flop; at
  q = 64 that is 16 flop per byte, near the float64 MFMA ridge.  The share of ``k_rrr_step`` in the iteration comes from
  a kernel trace of the same command taken in a run of its own (``rocprofv3 --kernel-trace --stats -- python
  tools/ccar3_probe.py --parts iterations``): the kernels are ``k_rrr_step`` and ``k_rrr_finish``.
- ``setup``: at the same shapes, n = 4 p rows of float64 CUDA views: K1 over ``[X Y]``, then the shifted block, its
  Cholesky factor and triangular inverse (``ccz_cholinv``) and ``M = L^-T L^-1`` (``ccz_gemm_f64``).
- ``torch``: the same iteration with ``torch.cholesky_solve`` on the factor (what the reference does), same GPU.
- ``numpy``: the NumPy restatement's loop (tests/ccar3_restatement.py) on the host's threads, at (4096, 64) and (512, 16).

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

SHAPES = ((4096, 64), (16320, 64), (512, 16))
LAMBDA, RHO = 0.05, 1.0


def _problem(p, q, device):
    """(Sxx + rho I, P) of a random covariance with a few strong directions, float64."""
    import torch

    g = torch.Generator(device=device).manual_seed(p + q)
    n = 2 * p
    X = torch.randn(n, 4, device=device, dtype=torch.float64, generator=g) @ torch.randn(4, p, device=device, dtype=torch.float64, generator=g)
    X += torch.randn(n, p, device=device, dtype=torch.float64, generator=g)
    A = X.T @ X / n
    A.diagonal().add_(RHO)
    P = torch.randn(p, q, device=device, dtype=torch.float64, generator=g) / q ** 0.5
    return A, P.contiguous()


def probe_iterations(p, q, iters):
    import torch

    from cca_zoo_amd import _backend

    A, P = _problem(p, q, "cuda")
    h = _backend.handle_for([A])
    vp = C.c_void_p
    # M = A^-1 = L^-T L^-1 as the estimator forms it
    M, Xi = torch.empty_like(A), torch.zeros_like(A)
    torch.cuda.synchronize()
    h.check(h.lib.ccz_cholinv(h.raw, 1, (vp * 1)(A.data_ptr()), (C.c_int64 * 1)(p), (vp * 1)(M.data_ptr()), (vp * 1)(Xi.data_ptr())))
    h.gemm(True, False, p, p, p, 1.0, Xi.data_ptr(), p, Xi.data_ptr(), p, 0.0, M.data_ptr(), p)
    h.sync()
    del A, Xi
    state = C.c_void_p()
    h.check(h.lib.ccz_rrr_create(h.raw, p, q, LAMBDA, RHO, 0.0, 2 * iters, iters, C.byref(state)))
    try:
        torch.cuda.synchronize()
        h.check(h.lib.ccz_rrr_setup(h.raw, state, C.c_void_p(M.data_ptr()), C.c_void_p(P.data_ptr())))
        a, b = C.c_int64(0), C.c_int(0)
        h.check(h.lib.ccz_rrr_iterations(h.raw, state, iters, C.byref(a), C.byref(b)))     # warm-up chunk
        h.sync()
        t0 = time.perf_counter()
        h.check(h.lib.ccz_rrr_iterations(h.raw, state, iters, C.byref(a), C.byref(b)))
        h.sync()
        ms = (time.perf_counter() - t0) * 1e3 / iters
        it = C.c_int64(0)
        h.check(h.lib.ccz_rrr_status(h.raw, state, C.byref(it), None, None, None, None))
        assert it.value == 2 * iters, (it.value, iters)
    finally:
        h.check(h.lib.ccz_rrr_destroy(h.raw, state))
    return {"p": p, "q": q, "ms_per_iteration": round(ms, 4), "model_bytes_of_M": 8 * p * p, "model_flop": 2 * p * p * q,
            "M_read_tb_per_s_over_whole_iteration": round(8.0 * p * p / ms / 1e9, 3),
            "tflops_fp64_over_whole_iteration": round(2.0 * p * p * q / ms / 1e9, 3)}


def probe_setup(p, q):
    import torch

    from cca_zoo_amd import _backend

    n, D = 4 * p, p + q
    g = torch.Generator(device="cuda").manual_seed(7)
    X = torch.randn(n, p, device="cuda", dtype=torch.float64, generator=g)
    Y = torch.randn(n, q, device="cuda", dtype=torch.float64, generator=g)
    h = _backend.handle_for([X, Y])
    vp = C.c_void_p
    out = {"p": p, "q": q, "n": n}
    for rep in range(2):        # the first round loads the code objects
        torch.cuda.synchronize()
        mom, A, L, Xi = h.alloc((D * D + D) * 8), h.alloc(p * p * 8), h.alloc(p * p * 8), h.alloc(p * p * 8)
        t0 = time.perf_counter()
        h.moments([(X.data_ptr(), p, p), (Y.data_ptr(), q, q)], n, _backend.F64, True, mom.ptr, pilot=False, timed=False)
        h.sync()
        t1 = time.perf_counter()
        h.check(h.lib.ccz_moments_block(h.raw, vp(mom.ptr), D, n, 1, 0, p, 0, p, RHO, vp(A.ptr), p))
        h.memset0(Xi.ptr, p * p * 8)
        h.check(h.lib.ccz_cholinv(h.raw, 1, (vp * 1)(A.ptr), (C.c_int64 * 1)(p), (vp * 1)(L.ptr), (vp * 1)(Xi.ptr)))
        h.sync()
        t2 = time.perf_counter()
        h.gemm(True, False, p, p, p, 1.0, Xi.ptr, p, Xi.ptr, p, 0.0, L.ptr, p)
        h.sync()
        t3 = time.perf_counter()
        out.update(k1_ms=round((t1 - t0) * 1e3, 2), factor_and_triangular_inverse_ms=round((t2 - t1) * 1e3, 2),
                   inverse_product_ms=round((t3 - t2) * 1e3, 2))
        del mom, A, L, Xi
    return out


def probe_torch(p, q, iters):
    import torch

    A, P = _problem(p, q, "cuda")
    L = torch.linalg.cholesky(A)
    Z, U = torch.zeros_like(P), torch.zeros_like(P)
    thr = LAMBDA / RHO

    def iteration(Z, U):
        B = torch.cholesky_solve(P + RHO * (Z - U), L)
        T = B + U
        nr = T.norm(dim=1, keepdim=True)
        Zn = T * torch.where(nr > 0, (1.0 - thr / nr).clamp_min(0.0), torch.zeros_like(nr))
        return Zn, T - Zn, max((Zn - B).norm(), (Z - Zn).norm())       # the residuals stay on the device

    for _ in range(3):
        Z, U, _r = iteration(Z, U)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        Z, U, _r = iteration(Z, U)
    torch.cuda.synchronize()
    return {"what": "torch cholesky_solve iteration without the host's stop test, same GPU", "p": p, "q": q,
            "ms_per_iteration": round((time.perf_counter() - t0) * 1e3 / iters, 4)}


def probe_numpy(p, q, iters):
    from ccar3_restatement import admm_loop

    A, P = _problem(p, q, "cpu")
    M = np.linalg.inv(A.numpy())
    admm_loop(M, P.numpy(), LAMBDA, RHO, 0.0, 1)
    t0 = time.perf_counter()
    admm_loop(M, P.numpy(), LAMBDA, RHO, 0.0, iters)
    return {"what": "NumPy restatement's loop, host threads", "p": p, "q": q, "cores": os.cpu_count(),
            "threads": os.environ.get("OMP_NUM_THREADS"), "ms_per_iteration": round((time.perf_counter() - t0) * 1e3 / iters, 3)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--parts", default="iterations,setup,torch,numpy")
    a = ap.parse_args(argv)
    parts = a.parts.split(",")
    res = {}
    if "iterations" in parts:
        res["iterations"] = [probe_iterations(p, q, a.iters) for p, q in SHAPES]
    if "setup" in parts:
        res["setup"] = [probe_setup(p, q) for p, q in SHAPES]
    if "torch" in parts:
        res["torch_cholesky_solve"] = []
        for p, q in SHAPES:
            try:
                res["torch_cholesky_solve"].append(probe_torch(p, q, a.iters))
            except RuntimeError as e:        # a baseline that cannot run is reported as that, not measured around
                res["torch_cholesky_solve"].append({"p": p, "q": q, "not_measured": str(e).splitlines()[0][:200]})
    if "numpy" in parts:
        res["numpy"] = [probe_numpy(p, q, max(2, a.iters // 5)) for p, q in ((4096, 64), (512, 16))]
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
