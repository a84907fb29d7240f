#!/usr/bin/env python3
"""Measure the gradient (Eckart-Young) models on one GPU and print one JSON object (``--out`` also writes it).

    python tools/ey_probe.py [--out profiles/ey_probe.json] [--only wide|small|cpu]

wide:  CCA_EY on 2 x 32768 fp32 features, n = 65536 (drawn on the device with ccz_randn_fill), k = 16, bs = 4096,
       200 steps, tol = 0.  ms per step from the whole fit minus its setup (the same fit at 0 steps), bytes per step
       counted as two passes over the gathered rows (2 x bs x sum p x 4 B), 4 launches per step.
small: the reference docstring's example, 5000 x (200, 150) float64, k = 4, bs = 128, 1000 steps: fit time, the host
       time of the index draws alone, the one-off host QR of the initialisation.
cpu:   the float64 NumPy step of the reference (batch upcast, re-centred) on host rows of the wide batch shape, a few
       steps, extrapolated to 200 (labelled as such).
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


def wide(out, steps=200, reps=3):
    import torch

    from cca_zoo_amd import _backend
    from cca_zoo_amd.linear import CCA_EY

    n, p, k, bs = 65536, 32768, 16, 4096
    h = _backend.default_handle()
    views = []
    for i in range(2):
        x = torch.empty(n, p, device="cuda", dtype=torch.float32)
        h.check(h.lib.ccz_randn_fill(h.raw, _backend.F32, C.c_void_p(x.data_ptr()), n, p, p, 77 + i, 0, p, 1.0, 0))
        views.append(x)
    torch.cuda.synchronize()

    def fit(it):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = CCA_EY(latent_dimensions=k, c=0.5, batch_size=bs, learning_rate=1e-4, max_iter=it, tol=0.0,
                   random_state=0).fit(views)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, m

    fit(steps)                                     # warm-up (code objects, pool)
    t_setup = min(fit(0)[0] for _ in range(reps))
    runs = [fit(steps) for _ in range(reps)]
    t_fit = min(r[0] for r in runs)
    assert runs[0][1].n_iter_ == steps
    ms_step = (t_fit - t_setup) / steps * 1e3
    bytes_step = 2 * bs * 2 * p * 4
    out["wide"] = {
        "shape": {"n": n, "p": [p, p], "k": k, "batch_size": bs, "steps": steps, "dtype": "float32"},
        "fit_s": round(t_fit, 4), "setup_s": round(t_setup, 4), "ms_per_step": round(ms_step, 4),
        "bytes_per_step": bytes_step, "tb_per_s": round(bytes_step / (ms_step * 1e-3) / 1e12, 3),
        "launches_per_step": 4,
        "batch_bytes": bs * 2 * p * 4,
    }


def small(out):
    from cca_zoo_amd.linear import CCA_EY
    from cca_zoo_amd.linear.gradient._base import draw_batches

    rng = np.random.default_rng(0)
    X1 = rng.standard_normal((5000, 200))
    X2 = rng.standard_normal((5000, 150))
    CCA_EY(latent_dimensions=4, batch_size=128, random_state=0, max_iter=50).fit([X1, X2])
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        m = CCA_EY(latent_dimensions=4, batch_size=128, random_state=0).fit([X1, X2])
        ts.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    draw_batches(np.random.default_rng(0), 5000, 128, 1000)
    t_draw = time.perf_counter() - t0
    z = rng.standard_normal((128, 4))
    t0 = time.perf_counter()
    for _ in range(2):
        _, r = np.linalg.qr(z)
        np.linalg.solve(r, np.eye(4))
    t_qr = time.perf_counter() - t0
    out["small"] = {
        "shape": {"n": 5000, "p": [200, 150], "k": 4, "batch_size": 128, "steps": 1000, "dtype": "float64"},
        "fit_ms": round(min(ts) * 1e3, 2), "n_iter": m.n_iter_, "host_index_draw_ms": round(t_draw * 1e3, 2),
        "host_init_qr_ms": round(t_qr * 1e3, 3),
    }


def cpu(out, steps=3):
    n_threads = os.environ.get("OMP_NUM_THREADS", "unset")
    bs, p, k = 4096, 32768, 16
    rng = np.random.default_rng(0)
    xs = [rng.standard_normal((bs, p), dtype=np.float32) for _ in range(2)]
    W = [rng.standard_normal((p, k)) / np.sqrt(p) for _ in range(2)]
    c, m = 0.5, 2
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        Z = [x @ w for x, w in zip(xs, W)]
        Zc = [z - z.mean(axis=0) for z in Z]
        tot = sum(Zc)
        V = sum(z.T @ z for z in Zc) / ((bs - 1) * m)
        B = sum(w.T @ w for w in W) / m
        vb = (1 - c) * V + c * B
        for i in range(m):
            zt = 4.0 / (m * (bs - 1)) * (c * Zc[i] + (1 - c) * Zc[i] @ vb - tot)
            g = (xs[i] - xs[i].mean(axis=0)).T @ zt + (4 * c / m) * W[i] @ vb
            W[i] = W[i] - 1e-4 * g
        ts.append(time.perf_counter() - t0)
    per = float(np.median(ts))
    out["cpu_comparator"] = {
        "what": "float64 NumPy step of the reference on host rows of the wide batch shape (2 x 4096 x 32768)",
        "threads": n_threads, "measured_steps": steps, "s_per_step": round(per, 3),
        "extrapolated_200_steps_s": round(per * 200, 1), "extrapolated": True,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only", choices=["wide", "small", "cpu"])
    ap.add_argument("--steps", type=int, default=200, help="wide case: steps per fit (200 in the recorded numbers)")
    ap.add_argument("--reps", type=int, default=3, help="wide case: timed fits")
    a = ap.parse_args()
    out = {}
    if a.only in (None, "small"):
        small(out)
    if a.only in (None, "wide"):
        wide(out, a.steps, a.reps)
    if a.only in (None, "cpu"):
        cpu(out)
    if a.out:
        prev = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                prev = json.load(f)
        prev.update(out)
        with open(a.out, "w") as f:
            json.dump(prev, f, indent=2)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
