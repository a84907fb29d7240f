#!/usr/bin/env python3
"""Measure the GFA iteration on one GPU and print one JSON object (``--out`` also writes it).

    python tools/gfa_probe.py [--out profiles/gfa_probe.json] [--only device|cpu] [--shape wide|tall] [--k 1,8,32] [--iters 10]

device: whole VB iterations through the C ABI on float32 views drawn on the device (ccz_randn_fill), tol = 0,
        drop_k off, a fixed number of iterations: ms per iteration between two stream synchronisations (the first,
        untimed call holds the code-object loads), and the achieved bytes per second against the model
        2 * sum_i n p_i 4 bytes per iteration.  Shapes: wide, n = 4096, 2 x 262144, k in {1, 8, 32}; tall, n = 1e6,
        2 x 1024, k = 8.  At the wide shape the PLS_ALS sweep (k = 1, the same bytes) is timed in the same run.  The
        per-kernel split comes from one ``rocprofv3 --kernel-trace --stats`` run of ``--only device --shape wide --k K``
        summarised by tools/rocpd_stats.py; ``--kernel-stats K=TABLE.md`` reads such a table back and adds the shares.
cpu:    the reference-structured float64 NumPy iteration (float64 copies of the views, X'z and Xw per view, the k x k
        algebra) on the host cores at n = 512 with the wide widths and k = 8, scaled by 8 to n = 4096 (labelled as scaled).
"""

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

SHAPES = {"wide": (4096, 262144), "tall": (1000000, 1024)}


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


def _gfa(h, varr, marr, n, p, k, iters):
    from cca_zoo_amd import _backend

    state = C.c_void_p()
    h.check(h.lib.ccz_gfa_create(h.raw, _backend.F32, 2, (C.c_int64 * 2)(p, p), n, k, 0.0, 10 ** 6, 0, iters, C.byref(state)))
    try:
        z0 = np.ascontiguousarray(np.random.default_rng(0).standard_normal((n, k)))
        times, setup = [], []
        a, b = C.c_int64(0), C.c_int(0)
        for rep in range(3):
            h.check(h.lib.ccz_gfa_set_init(h.raw, state, z0.ctypes.data_as(C.POINTER(C.c_double))))
            h.sync()
            t0 = time.perf_counter()
            h.check(h.lib.ccz_gfa_setup(h.raw, state, varr, marr))
            h.sync()
            setup.append(time.perf_counter() - t0)
            h.check(h.lib.ccz_gfa_iterations(h.raw, state, varr, marr, 1, C.byref(a), C.byref(b)))
            h.sync()
            t0 = time.perf_counter()
            h.check(h.lib.ccz_gfa_iterations(h.raw, state, varr, marr, iters, C.byref(a), C.byref(b)))
            h.sync()
            if rep:
                times.append(time.perf_counter() - t0)
        ms = min(times) / iters * 1e3
        model = 2 * 2 * n * p * 4
        return {"ms_per_iteration": round(ms, 4), "tb_per_s": round(model / (ms * 1e-3) / 1e12, 3),
                "timed_runs_ms": [round(t / iters * 1e3, 4) for t in times], "setup_ms": round(min(setup[1:]) * 1e3, 3),
                "model_bytes_per_iteration": model}
    finally:
        h.check(h.lib.ccz_gfa_destroy(h.raw, state))


def _pls(h, varr, marr, n, p, sweeps):
    from cca_zoo_amd import _backend
    from cca_zoo_amd.linear._iterative import RULE_NORMALISE, initial_vectors

    state = C.c_void_p()
    h.check(h.lib.ccz_als_create(h.raw, _backend.F32, 2, (C.c_int64 * 2)(p, p), n, 1, RULE_NORMALISE, (C.c_double * 2)(0.0, 0.0),
                                 0.0, 10 ** 6, sweeps, C.byref(state)))
    try:
        w0 = np.ascontiguousarray(initial_vectors(0, [p, p], 1))
        times = []
        a, b = C.c_int64(0), C.c_int(0)
        for rep in range(3):
            h.check(h.lib.ccz_als_set_init(h.raw, state, w0.ctypes.data_as(C.POINTER(C.c_double))))
            h.check(h.lib.ccz_als_sweeps(h.raw, state, varr, marr, 1, C.byref(a), C.byref(b)))
            h.sync()
            t0 = time.perf_counter()
            h.check(h.lib.ccz_als_sweeps(h.raw, state, varr, marr, sweeps, C.byref(a), C.byref(b)))
            h.sync()
            if rep:
                times.append(time.perf_counter() - t0)
        return {"ms_per_sweep": round(min(times) / sweeps * 1e3, 4)}
    finally:
        h.check(h.lib.ccz_als_destroy(h.raw, state))


def device(out, shape, ks, iters):
    from cca_zoo_amd import _backend

    h = _backend.default_handle()
    n, p = SHAPES[shape]
    views, mus, varr, marr = _views(h, n, p)
    res = {"shape": {"n": n, "p": [p, p], "dtype": "float32", "iterations": iters, "tol": 0.0, "drop_k": False}}
    for k in ks:
        res[f"k{k}"] = _gfa(h, varr, marr, n, p, k, iters)
    if shape == "wide":
        res["PLS_ALS_k1_same_run"] = _pls(h, varr, marr, n, p, iters)
        if "k1" in res:
            res["k1"]["ratio_to_pls_als_sweep"] = round(res["k1"]["ms_per_iteration"] / res["PLS_ALS_k1_same_run"]["ms_per_sweep"], 3)
    out[f"device_{shape}"] = res
    del views, mus


def cpu(out, iters=2):
    n, p, k = 512, SHAPES["wide"][1], 8
    rng = np.random.default_rng(0)
    xs = [rng.standard_normal((n, p)) for _ in range(2)]                # the reference's float64 copies
    z = rng.standard_normal((n, k))
    zz = z.T @ z + n * np.eye(k)
    alpha, tau = [np.ones(k), np.ones(k)], np.ones(2)
    y_const = [np.sum(x ** 2) for x in xs]                               # once per fit, as the reference
    ts = []
    for _ in range(iters + 1):
        t0 = time.perf_counter()
        w, ww = [], []
        for i in range(2):
            t = 1.0 / np.sqrt(alpha[i])
            c = np.linalg.cholesky(np.outer(t, t) * zz + np.eye(k) / tau[i])
            cov_w = (1.0 / tau[i]) * np.outer(t, t) * np.linalg.solve(c.T, np.linalg.solve(c, np.eye(k)))
            w.append(xs[i].T @ z @ cov_w * tau[i])
            ww.append(w[i].T @ w[i] + p * cov_w)
        c = np.linalg.cholesky(np.eye(k) + sum(tau[i] * ww[i] for i in range(2)))
        cov_z = np.linalg.solve(c.T, np.linalg.solve(c, np.eye(k)))
        xw = [xs[i] @ w[i] for i in range(2)]
        z = sum(xw[i] * tau[i] for i in range(2)) @ cov_z
        zz = z.T @ z + n * cov_z
        for i in range(2):
            alpha[i] = (p / 2.0) / (np.diag(ww[i]) / 2.0)
            tau[i] = (n * p / 2.0) / ((y_const[i] + np.sum(ww[i] * zz) - 2.0 * np.sum(z * xw[i])) / 2.0)
        ts.append(time.perf_counter() - t0)
    per = float(min(ts[1:]))
    out["cpu_comparator"] = {
        "what": "reference-structured float64 NumPy GFA iteration on host copies, 2 x 512 x 262144, k = 8, scaled x8 to n = 4096",
        "threads": os.environ.get("OMP_NUM_THREADS", "unset"), "measured_n": n, "ms_per_iteration_measured": round(per * 1e3, 2),
        "ms_per_iteration_scaled_to_n4096": round(per * 8 * 1e3, 1), "scaled": True,
    }


def kernel_split(out, spec):
    """``K=TABLE.md``: the share of the k_gfa_* kernel time of a profiled run (tools/rocpd_stats.py table) by kernel."""
    k, path = spec.split("=", 1)
    tot, calls = {}, {}
    with open(path) as f:
        for line in f:
            c = [x.strip() for x in line.split("|")]
            if len(c) == 9 and "k_gfa_" in c[1] and c[2].isdigit():
                name = c[1].strip("`").split("::")[-1].split("<")[0]
                tot[name] = tot.get(name, 0.0) + float(c[3])
                calls[name] = calls.get(name, 0) + int(c[2])
    all_ms, iters = sum(tot.values()), calls["k_gfa_finish"]
    out.setdefault("kernel_split", {})[f"k{k}"] = {
        "source": "rocprofv3 --kernel-trace --stats, k_gfa_* kernels only", "iterations_profiled": iters,
        "kernel_ms_per_iteration": round(all_ms / iters, 4),
        "share_by_kernel": {name: round(v / all_ms, 4) for name, v in sorted(tot.items(), key=lambda kv: -kv[1])},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only", choices=["device", "cpu", "none"])
    ap.add_argument("--shape", choices=["wide", "tall"], help="device part: this shape alone")
    ap.add_argument("--k", help="device part, wide shape: comma-separated latent dimensions (default 1,8,32)")
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="K=TABLE.md")
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    out = {}
    if a.only in (None, "device"):
        for shape in ([a.shape] if a.shape else ["wide", "tall"]):
            ks = [int(x) for x in a.k.split(",")] if (a.k and shape == "wide") else ([1, 8, 32] if shape == "wide" else [8])
            device(out, shape, ks, a.iters)
    if a.only in (None, "cpu"):
        cpu(out)
    for spec in a.kernel_stats:
        kernel_split(out, spec)
    if a.out:
        prev = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                prev = json.load(f)
        for key, val in out.items():
            if key == "kernel_split":
                prev.setdefault(key, {}).update(val)
            else:
                prev[key] = val
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(prev, f, indent=2)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
