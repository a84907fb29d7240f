#!/usr/bin/env python3
"""Measure ``bootstrap`` (csrc/boot.hip) on one GPU and print one JSON object (``--out`` also writes it).

    python tools/boot_probe.py [--out profiles/boot_probe.json] [--B 1000] [--parts device,draw,public,refit,numpy] [--shapes all]

Shapes: n = 16384 / 131072 / 1048576, (p1, p2) = (16, 16) and (64, 64), float32 host views (planted rank 2 plus noise), k = 2.

- ``device``: the shift (column means, ``ccz_transform`` with an identity; host clock around a stream synchronise, second of
  two rounds) and the resamples through the C ABI: ``B`` resamples as calls of ``CHUNK`` resamples each (the public function's
  chunk length at that n) on counts that are ALREADY on the device (``CHUNK`` distinct resamples, reused), so the time is the
  two kernels' and not the host's drawing.  Beside it the traffic MODEL ``B n (1 - 1/e) (p1 + p2) 8 * 3/2`` bytes -- an
  estimate: every drawn row of each view once per block that uses it (view 1 for 11 and 12, view 2 for 12 and 22; the second
  read of a row within one workgroup is taken to hit the cache), nothing for the counts, the partials or a cache across
  workgroups -- and the rate it gives.  The split between ``k_boot_moments`` and ``k_boot_solve`` comes from a kernel
  trace of ``--parts device`` taken in a run of its own (``rocprofv3 --kernel-trace --stats``, summarised by
  tools/rocpd_stats.py into ``profiles/boot_kernel_stats.md``).
- ``draw``: ``ccz_draw_counts`` (csrc/draw.hip) alone, through the C ABI: ``B`` resamples as calls of ``CHUNK`` each into one
  device buffer (the rows zeroed, then one integer atomic add per draw).  Beside it the traffic MODEL ``8 n`` bytes per
  resample -- 4 n zeroed, 4 n added -- and the rate it gives.
- ``public``: ``bootstrap(rCCA(latent_dimensions=2, c=[0.1, 0.3]), views, n_resamples=B_public)`` end to end, once with
  ``draws="numpy"`` (the host's ``rng.integers`` draws, ``np.bincount`` and the count uploads) and once with
  ``draws="device"``, in the same run; ``B_public`` is ``B`` scaled down at the largest n (stated in the output).  Beside it
  the host's draw + bincount alone, per resample.
- ``refit``: the loop a user writes without this function: ``rCCA.fit([X1[idx], X2[idx]])`` on float32 CUDA views, the
  resampled views made by torch indexing on the device (``torch.randint`` on the device); ``B'`` fits, stated.
- ``numpy``: the restatement's refit (tests/boot_restatement.py: gather, means, covariances, Cholesky, LAPACK SVD) on the
  host's threads; ``B'`` resamples, stated.

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
K = 2


def make_views(n, p1, p2):
    rng = np.random.default_rng(n + p1)
    z = rng.standard_normal((n, 2), dtype=np.float32)
    return [z @ rng.standard_normal((2, p), dtype=np.float32) + rng.standard_normal((n, p), dtype=np.float32) for p in (p1, p2)]


def probe_device(views, B):
    from cca_zoo_amd import _backend
    from cca_zoo_amd.model_selection import _bootstrap as bs

    n, (p1, p2) = views[0].shape[0], [v.shape[1] for v in views]
    r = min(p1, p2)
    h = _backend.default_handle()
    x64 = [h.to_device(np.ascontiguousarray(v, dtype=np.float64)) for v in views]
    for _ in range(2):                                   # the first round loads the code objects
        h.sync()
        t0 = time.perf_counter()
        Z = [bs._shifted(h, x64[i].ptr, n, (p1, p2)[i], True) for i in range(2)]
        h.sync()
        shift_ms = (time.perf_counter() - t0) * 1e3
    rng = np.random.default_rng(0)
    CHUNK = bs.chunk_length(n)                           # the public function's rule: CHUNK_RESAMPLES, fewer at large n
    counts = h.to_device(bs.draw_counts(rng, n, CHUNK))
    sv, W, info = h.alloc(CHUNK * r * 8), h.alloc(CHUNK * (p1 + p2) * K * 8), h.alloc(CHUNK * 4)
    calls = max(1, B // CHUNK)

    def run(k):
        for _ in range(k):
            bs.boot_rcca(h, n, p1, p2, Z[0].ptr, Z[1].ptr, counts.ptr, CHUNK, C_RIDGE[0], C_RIDGE[1], True, K, sv.ptr, W.ptr, info.ptr)
        h.sync()

    run(1)
    t0 = time.perf_counter()
    run(calls)
    ms = (time.perf_counter() - t0) * 1e3
    assert not h.to_host(info, (CHUNK,), dtype=np.int32).any()
    done = calls * CHUNK
    model = int(done * n * (1.0 - np.exp(-1.0)) * (p1 + p2) * 8 * 1.5)
    return {"n": n, "p": [p1, p2], "k": K, "shift_ms": round(shift_ms, 3), "resamples": done, "resamples_per_call": CHUNK,
            "resamples_ms": round(ms, 3), "us_per_resample": round(ms * 1e3 / done, 3),
            "traffic_model_bytes": model, "traffic_model_tb_per_s": round(model / ms / 1e9, 3),
            "shift_share_of_B_resamples": round(shift_ms / (shift_ms + ms), 4)}


def probe_draw(views, B):
    import ctypes as C

    from cca_zoo_amd import _backend
    from cca_zoo_amd.model_selection import _bootstrap as bs

    n = views[0].shape[0]
    h = _backend.default_handle()
    CHUNK = bs.chunk_length(n)
    out = h.alloc(CHUNK * n * 4)
    calls = max(1, B // CHUNK)

    def run(k):
        for i in range(k):
            h.check(h.lib.ccz_draw_counts(h.raw, n, CHUNK, 12345, i * CHUNK, C.c_void_p(out.ptr)))
        h.sync()

    run(1)
    t0 = time.perf_counter()
    run(calls)
    ms = (time.perf_counter() - t0) * 1e3
    assert int(h.to_host(out, (CHUNK, n), dtype=np.int32)[-1].sum()) == n
    done = calls * CHUNK
    model = done * n * 8
    return {"n": n, "resamples": done, "resamples_per_call": CHUNK, "draw_ms": round(ms, 3),
            "us_per_resample": round(ms * 1e3 / done, 3), "traffic_model_bytes": model,
            "traffic_model_tb_per_s": round(model / ms / 1e9, 3)}


def probe_public(views, B):
    from cca_zoo_amd.linear import rCCA
    from cca_zoo_amd.model_selection import bootstrap

    n = views[0].shape[0]
    b = B if n < 1 << 20 else max(2, B // 10)
    bootstrap(rCCA(latent_dimensions=K, c=C_RIDGE), views, n_resamples=2, random_state=0)
    t0 = time.perf_counter()
    res = bootstrap(rCCA(latent_dimensions=K, c=C_RIDGE), views, n_resamples=b, random_state=0)
    ms = (time.perf_counter() - t0) * 1e3
    bootstrap(rCCA(latent_dimensions=K, c=C_RIDGE), views, n_resamples=2, random_state=0, draws="device")
    t0 = time.perf_counter()
    dev = bootstrap(rCCA(latent_dimensions=K, c=C_RIDGE), views, n_resamples=b, random_state=0, draws="device")
    dev_ms = (time.perf_counter() - t0) * 1e3
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    for _ in range(5):
        np.bincount(rng.integers(0, n, size=n), minlength=n)
    draw_ms = (time.perf_counter() - t0) * 1e3 / 5
    return {"n": n, "p": [v.shape[1] for v in views], "B_public": b, "scaled_down_by": B // b, "total_ms": round(ms, 2),
            "ms_per_resample": round(ms / b, 4), "host_integers_plus_bincount_ms_each": round(draw_ms, 4),
            "sigma_1": float(res.singular_values[0]), "sigma_1_se": float(res.singular_values_se[0]),
            "device_draws_total_ms": round(dev_ms, 2), "device_draws_ms_per_resample": round(dev_ms / b, 4),
            "device_draws_sigma_1_se": float(dev.singular_values_se[0]), "numpy_over_device": round(ms / dev_ms, 2)}


def probe_refit(views, B):
    import torch

    from cca_zoo_amd.linear import rCCA

    n = views[0].shape[0]
    b = max(3, min(B, (20 << 20) // n))
    X1, X2 = (torch.tensor(v, device="cuda") for v in views)

    def loop(k):
        for _ in range(k):
            idx = torch.randint(0, n, (n,), device="cuda")
            fit = rCCA(latent_dimensions=K, c=C_RIDGE).fit([X1[idx], X2[idx]])
            fit.singular_values_, fit.weights_
        torch.cuda.synchronize()

    loop(2)
    t0 = time.perf_counter()
    loop(b)
    ms = (time.perf_counter() - t0) * 1e3
    return {"what": "rCCA.fit([X1[idx], X2[idx]]) per resample, float32 CUDA views, torch indexing, same GPU", "n": n,
            "p": [v.shape[1] for v in views], "B_prime": b, "scaled_down_by": round(B / b, 1), "ms_per_resample": round(ms / b, 4)}


def probe_numpy(views, B):
    import boot_restatement as br

    n = views[0].shape[0]
    b = max(3, min(B, (8 << 20) // n))
    X1, X2 = (np.asarray(v, dtype=np.float64) for v in views)
    rng = np.random.default_rng(0)
    idx = rng.integers(0, n, size=n)
    br.fit_rows(X1[idx], X2[idx], C_RIDGE, True, K)
    t0 = time.perf_counter()
    for _ in range(b):
        idx = rng.integers(0, n, size=n)
        br.fit_rows(X1[idx], X2[idx], C_RIDGE, True, K)
    ms = (time.perf_counter() - t0) * 1e3
    return {"what": "NumPy restatement: draw, gather, means, covariances, Cholesky, SVD per resample, host threads", "n": n,
            "p": [v.shape[1] for v in views], "threads": os.environ.get("OMP_NUM_THREADS"), "B_prime": b,
            "scaled_down_by": round(B / b, 1), "ms_per_resample": round(ms / b, 4)}


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
