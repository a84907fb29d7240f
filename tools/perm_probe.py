#!/usr/bin/env python3
"""Measure ``permutation_test`` (csrc/perm.hip) on one GPU and print one JSON object (``--out`` also writes it).

    python tools/perm_probe.py [--out profiles/perm_probe.json] [--B 1000] [--parts device,draw,public,refit,numpy] [--shapes all]

Shapes: n = 16384 / 131072 / 1048576, (p1, p2) = (16, 16) and (64, 64), float32 host views (planted rank 2 plus noise).

- ``device``: the whitening (two K1 passes, two ``ccz_cholinv``, two float64 projections; host clock around a stream
  synchronise, second of two rounds) and the null through the C ABI: ``B`` permutations as calls of ``CHUNK`` permutations
  each (the public function's chunk length at that n) on indices that are ALREADY on the device (``CHUNK`` distinct
  permutations, reused), so the time is the two
  kernels' and not the host's drawing.  Beside it the traffic MODEL ``B n (p1 + p2) 8`` bytes -- an estimate: every row of
  both whitened views once per permutation, nothing for the indices, the partials or a cache -- and the rate it gives.
  The split between ``k_perm_cross`` and ``k_perm_fold_svd`` comes from a kernel trace of ``--parts device`` taken in a
  run of its own (``rocprofv3 --kernel-trace --stats``, summarised by tools/rocpd_stats.py into
  ``profiles/perm_kernel_stats.md``).  How much of ``Z_1`` is served from L2 is not measured here (it needs counters).
- ``draw``: ``ccz_draw_permutations`` (csrc/draw.hip) alone, through the C ABI: ``B`` permutations as calls of ``CHUNK`` each
  into one device buffer.  Beside it the traffic MODEL ``12 n`` bytes per permutation -- the rows written in bucket order, read
  back by the sort pass and written in their final order, 4 bytes each; nothing for the bucket cursors or the atomics -- and
  the rate it gives.  The share of each pass comes from a kernel trace of ``--parts draw`` taken in a run of its own
  (``profiles/draw_kernel_stats.md``).
- ``public``: ``permutation_test(rCCA(c=[0.1, 0.3]), views, n_permutations=B_public)`` end to end, once with ``draws="numpy"``
  (the host's ``rng.permutation`` draws and the index uploads) and once with ``draws="device"``, in the same run;
  ``B_public`` is ``B`` scaled down at the largest n (stated in the output).
- ``refit``: the loop a user writes today: ``rCCA.fit([X1, X2[pi]])`` on float32 CUDA views, the permuted view made by torch
  indexing on the device (``torch.randperm`` on the device); ``B'`` fits, stated.
- ``numpy``: the restatement's permutation step (tests/perm_restatement.py: gather, product, LAPACK SVD) on the host's threads,
  after one whitening; ``B'`` permutations, stated.

Nothing is gated on these times."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NS = (16384, 131072, 1048576)
WIDTHS = ((16, 16), (64, 64))
C_RIDGE = [0.1, 0.3]


def make_views(n, p1, p2):
    rng = np.random.default_rng(n + p1)
    z = rng.standard_normal((n, 2), dtype=np.float32)
    return [z @ rng.standard_normal((2, p), dtype=np.float32) + rng.standard_normal((n, p), dtype=np.float32) for p in (p1, p2)]


def probe_device(views, B):
    from cca_zoo_amd import _backend
    from cca_zoo_amd.model_selection import _permutation as pm

    n, (p1, p2) = views[0].shape[0], [v.shape[1] for v in views]
    r = min(p1, p2)
    h = _backend.default_handle()
    x64 = [h.to_device(np.ascontiguousarray(v, dtype=np.float64)) for v in views]
    for _ in range(2):                                   # the first round loads the code objects
        h.sync()
        t0 = time.perf_counter()
        Z = [pm._whiten(h, x64[i].ptr, n, (p1, p2)[i], C_RIDGE[i], True) for i in range(2)]
        h.sync()
        whiten_ms = (time.perf_counter() - t0) * 1e3
    rng = np.random.default_rng(0)
    CHUNK = pm.chunk_length(n)                           # the public function's rule: CHUNK_PERMS, fewer at large n
    idx = h.to_device(pm.draw_permutations(rng, n, CHUNK))
    sv = h.alloc(CHUNK * r * 8)
    calls = max(1, B // CHUNK)

    def run(k):
        for _ in range(k):
            pm.singular_values(h, n, p1, p2, Z[0][0].ptr, Z[1][0].ptr, idx.ptr, CHUNK, sv.ptr)
        h.sync()

    run(1)
    t0 = time.perf_counter()
    run(calls)
    null_ms = (time.perf_counter() - t0) * 1e3
    done = calls * CHUNK
    model = done * n * (p1 + p2) * 8
    return {"n": n, "p": [p1, p2], "whitening_ms": round(whiten_ms, 3), "permutations": done, "permutations_per_call": CHUNK,
            "null_ms": round(null_ms, 3), "us_per_permutation": round(null_ms * 1e3 / done, 3),
            "traffic_model_bytes": model, "traffic_model_tb_per_s": round(model / null_ms / 1e9, 3),
            "whitening_share_of_B_permutations": round(whiten_ms / (whiten_ms + null_ms), 4)}


def probe_draw(views, B):
    import ctypes as C

    from cca_zoo_amd import _backend
    from cca_zoo_amd.model_selection import _permutation as pm

    n = views[0].shape[0]
    h = _backend.default_handle()
    CHUNK = pm.chunk_length(n)
    out = h.alloc(CHUNK * n * 4)
    calls = max(1, B // CHUNK)

    def run(k):
        for i in range(k):
            h.check(h.lib.ccz_draw_permutations(h.raw, n, CHUNK, 12345, i * CHUNK, 0, C.c_void_p(out.ptr)))
        h.sync()

    run(1)
    t0 = time.perf_counter()
    run(calls)
    ms = (time.perf_counter() - t0) * 1e3
    done = calls * CHUNK
    model = done * n * 12
    return {"n": n, "permutations": done, "permutations_per_call": CHUNK, "draw_ms": round(ms, 3),
            "us_per_permutation": round(ms * 1e3 / done, 3), "traffic_model_bytes": model,
            "traffic_model_tb_per_s": round(model / ms / 1e9, 3)}


def probe_public(views, B):
    from cca_zoo_amd.linear import rCCA
    from cca_zoo_amd.model_selection import permutation_test

    n = views[0].shape[0]
    b = B if n < 1 << 20 else max(1, B // 10)
    permutation_test(rCCA(c=C_RIDGE), views, n_permutations=2, random_state=0)
    t0 = time.perf_counter()
    res = permutation_test(rCCA(c=C_RIDGE), views, n_permutations=b, random_state=0)
    ms = (time.perf_counter() - t0) * 1e3
    permutation_test(rCCA(c=C_RIDGE), views, n_permutations=2, random_state=0, draws="device")
    t0 = time.perf_counter()
    dev = permutation_test(rCCA(c=C_RIDGE), views, n_permutations=b, random_state=0, draws="device")
    dev_ms = (time.perf_counter() - t0) * 1e3
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    for _ in range(5):
        rng.permutation(n)
    draw_ms = (time.perf_counter() - t0) * 1e3 / 5
    return {"n": n, "p": [v.shape[1] for v in views], "B_public": b, "scaled_down_by": B // b, "total_ms": round(ms, 2),
            "ms_per_permutation": round(ms / b, 4), "host_rng_permutation_ms_each": round(draw_ms, 4), "pvalue_0": float(res.pvalues[0]),
            "device_draws_total_ms": round(dev_ms, 2), "device_draws_ms_per_permutation": round(dev_ms / b, 4),
            "device_draws_pvalue_0": float(dev.pvalues[0]), "numpy_over_device": round(ms / dev_ms, 2)}


def probe_refit(views, B):
    import torch

    from cca_zoo_amd.linear import rCCA

    n = views[0].shape[0]
    b = max(3, min(B, (20 << 20) // n))
    X1, X2 = (torch.tensor(v, device="cuda") for v in views)
    r = min(X1.shape[1], X2.shape[1])

    def loop(k):
        for _ in range(k):
            pi = torch.randperm(n, device="cuda")
            rCCA(latent_dimensions=r, c=C_RIDGE).fit([X1, X2[pi]]).singular_values_
        torch.cuda.synchronize()

    loop(2)
    t0 = time.perf_counter()
    loop(b)
    ms = (time.perf_counter() - t0) * 1e3
    return {"what": "rCCA.fit([X1, X2[pi]]) per permutation, float32 CUDA views, torch indexing, same GPU", "n": n,
            "p": [v.shape[1] for v in views], "B_prime": b, "scaled_down_by": round(B / b, 1), "ms_per_permutation": round(ms / b, 4)}


def probe_numpy(views, B):
    import perm_restatement as pr

    n = views[0].shape[0]
    b = max(3, min(B, (8 << 20) // n))
    t0 = time.perf_counter()
    Z1, Z2 = (pr.whiten(v, c, True) for v, c in zip(views, C_RIDGE))
    whiten_ms = (time.perf_counter() - t0) * 1e3
    rng = np.random.default_rng(0)
    pr.singular_values(Z1, Z2, rng.permutation(n))
    t0 = time.perf_counter()
    for _ in range(b):
        pr.singular_values(Z1, Z2, rng.permutation(n))
    ms = (time.perf_counter() - t0) * 1e3
    return {"what": "NumPy restatement: draw, gather, product, SVD per permutation, host threads", "n": n, "p": [v.shape[1] for v in views],
            "threads": os.environ.get("OMP_NUM_THREADS"), "B_prime": b, "scaled_down_by": round(B / b, 1), "whitening_ms": round(whiten_ms, 2),
            "ms_per_permutation": round(ms / b, 4)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--B", type=int, default=1000)
    ap.add_argument("--parts", default="device,draw,public,refit,numpy")
    ap.add_argument("--shapes", default="all", help="all, or n:p1:p2[,n:p1:p2...]")
    a = ap.parse_args(argv)
    parts = a.parts.split(",")
    shapes = [(n, p1, p2) for n in NS for p1, p2 in WIDTHS] if a.shapes == "all" else [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]
    fns = {"device": probe_device, "draw": probe_draw, "public": probe_public, "refit": probe_refit, "numpy": probe_numpy}
    res = {"B": a.B, **{k: [] for k in parts}}
    for n, p1, p2 in shapes:
        views = make_views(n, p1, p2)
        for k in parts:
            res[k].append(fns[k](views, a.B))
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
