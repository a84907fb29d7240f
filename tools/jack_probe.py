#!/usr/bin/env python3
"""Measure the jackknife (``ccz_jack_rcca``, csrc/boot.hip) on one GPU and print one JSON object (``--out`` also writes it).

    python tools/jack_probe.py [--out profiles/jack_probe.json] [--parts loo,groups,bca] [--shapes all]

float32 host views (planted rank 2 plus noise, tools/boot_probe.py's), ``rCCA(c=[0.1, 0.3])``, k = 2; no bootstrap resamples
except in ``bca``.

- ``loo``: leave-one-out through the C ABI on the shifted float64 views in HBM, n = 16384 and 131072, (16, 16) and (64, 64):
  one ``ccz_jack_rcca`` call for all n replicates (host clock around a stream synchronise, second of two calls), against the
  only route the C ABI had before it: ``ccz_boot_rcca`` on the 0/1 leave-one-out counts in chunks of 64 replicates.  The
  counts of the chunks that are timed are built on the host and uploaded first; their upload is timed on its own and their
  refits on their own.  Where all n / 64 chunks would take too long, ``COUNT_CHUNKS`` evenly spaced chunks are timed and both
  figures are multiplied up to n replicates: the result then says ``"scaled": true``.
- ``groups``: ``jackknife(estimator, views, n_groups=4096)`` at n = 1048576 end to end (the upload of the float32 views, the
  widening, the shift, the replicates, the read-back, the estimator's own fit), and the ``ccz_jack_rcca`` call alone.
- ``bca``: ``bootstrap(method="BCa", n_resamples=1000, draws="device")`` against ``method="percentile"`` at n = 16384, same run,
  alternating, second round.

The shares of ``k_jack_downdate``, ``k_boot_solve`` and ``k_boot_moments`` come from a kernel trace of ``--parts loo`` taken in a run
of its own (``rocprofv3 --kernel-trace --stats``, summarised by tools/rocpd_stats.py into ``profiles/jack_kernel_stats.md``).

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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from boot_probe import C_RIDGE, K, WIDTHS, make_views  # noqa: E402

LOO_NS = (16384, 131072)
GROUPS_N, GROUPS_J = 1048576, 4096
BCA_N, BCA_B = 16384, 1000
CHUNK = 64                                               # replicates per ccz_boot_rcca call on the counts route
COUNT_CHUNKS = 16                                        # chunks of the counts route that are timed when not all are


def estimator():
    from cca_zoo_amd.linear import rCCA

    return rCCA(latent_dimensions=K, c=C_RIDGE)


def shifted(h, views):
    from cca_zoo_amd.model_selection import _bootstrap as bs

    n = views[0].shape[0]
    x64 = [h.to_device(np.ascontiguousarray(v, dtype=np.float64)) for v in views]
    return [bs._shifted(h, x64[i].ptr, n, views[i].shape[1], True) for i in range(2)], x64


def probe_loo(views):
    from cca_zoo_amd import _backend
    from cca_zoo_amd.model_selection import _bootstrap as bs, _jackknife as jk

    n, (p1, p2) = views[0].shape[0], [v.shape[1] for v in views]
    r, pt = min(p1, p2), p1 + p2
    h = _backend.default_handle()
    Z, keep = shifted(h, views)
    sv, W, info = h.alloc(n * r * 8), h.alloc(n * pt * K * 8), h.alloc(n * 4)
    for _ in range(2):                                   # the first call loads the code objects
        h.sync()
        t0 = time.perf_counter()
        jk.jack_rcca(h, n, p1, p2, Z[0].ptr, Z[1].ptr, n, 0, n, C_RIDGE[0], C_RIDGE[1], True, K, sv.ptr, W.ptr, info.ptr)
        h.sync()
        jack_ms = (time.perf_counter() - t0) * 1e3
    assert not h.to_host(info, (n,), dtype=np.int32).any()
    sv_jack = h.to_host(sv, (n, r))

    total = n // CHUNK
    timed = total if n <= 16384 else COUNT_CHUNKS
    firsts = [CHUNK * int(c) for c in np.round(np.linspace(0, total - 1, timed)).astype(np.int64)]
    counts = np.ones((timed * CHUNK, n), dtype=np.int32)
    for i, g0 in enumerate(firsts):
        rows = np.arange(CHUNK)
        counts[i * CHUNK + rows, g0 + rows] = 0
    dev = h.alloc(counts.nbytes)
    h.sync()
    t0 = time.perf_counter()
    h.h2d(dev.ptr, counts)
    h.sync()
    upload_ms = (time.perf_counter() - t0) * 1e3
    sv_c, W_c, info_c = h.alloc(timed * CHUNK * r * 8), h.alloc(timed * CHUNK * pt * K * 8), h.alloc(timed * CHUNK * 4)

    def run():
        for i in range(timed):
            bs.boot_rcca(h, n, p1, p2, Z[0].ptr, Z[1].ptr, dev.ptr + i * CHUNK * n * 4, CHUNK, C_RIDGE[0], C_RIDGE[1], True, K,
                         sv_c.ptr + i * CHUNK * r * 8, W_c.ptr + i * CHUNK * pt * K * 8, info_c.ptr + i * CHUNK * 4)
        h.sync()

    run()
    t0 = time.perf_counter()
    run()
    counts_ms = (time.perf_counter() - t0) * 1e3
    assert not h.to_host(info_c, (timed * CHUNK,), dtype=np.int32).any()
    got = h.to_host(sv_c, (timed * CHUNK, r))
    want = np.concatenate([sv_jack[g0:g0 + CHUNK] for g0 in firsts])
    scale = total / timed
    del keep
    return {"n": n, "p": [p1, p2], "k": K, "replicates": n, "jack_ms": round(jack_ms, 3), "jack_us_per_replicate": round(jack_ms * 1e3 / n, 3),
            "counts_route_replicates_timed": timed * CHUNK, "scaled": timed != total, "scaled_by": round(scale, 2),
            "counts_route_refits_ms": round(counts_ms * scale, 3), "counts_route_upload_ms": round(upload_ms * scale, 3),
            "counts_route_bytes": int(n) * int(n) * 4, "counts_route_us_per_replicate": round(counts_ms * 1e3 / (timed * CHUNK), 3),
            "counts_route_over_jack": round((counts_ms + upload_ms) * scale / jack_ms, 2),
            "counts_route_refits_over_jack": round(counts_ms * scale / jack_ms, 2),
            "worst_sigma_difference_over_sigma_1": float(np.max(np.abs(got - want) / want[:, :1]))}


def probe_groups(views):
    from cca_zoo_amd import _backend
    from cca_zoo_amd.model_selection import _jackknife as jk, jackknife

    n, (p1, p2) = views[0].shape[0], [v.shape[1] for v in views]
    r, pt, J = min(p1, p2), p1 + p2, GROUPS_J
    jackknife(estimator(), [v[:4096] for v in views], n_groups=64)     # code objects
    t0 = time.perf_counter()
    res = jackknife(estimator(), views, n_groups=J)
    total_ms = (time.perf_counter() - t0) * 1e3
    h = _backend.default_handle()
    Z, keep = shifted(h, views)
    sv, W, info = h.alloc(J * r * 8), h.alloc(J * pt * K * 8), h.alloc(J * 4)
    for _ in range(2):
        h.sync()
        t0 = time.perf_counter()
        jk.jack_rcca(h, n, p1, p2, Z[0].ptr, Z[1].ptr, J, 0, J, C_RIDGE[0], C_RIDGE[1], True, K, sv.ptr, W.ptr, info.ptr)
        h.sync()
        call_ms = (time.perf_counter() - t0) * 1e3
    del keep
    return {"n": n, "p": [p1, p2], "n_groups": J, "rows_per_group": n // J, "jackknife_total_ms": round(total_ms, 2),
            "ccz_jack_rcca_ms": round(call_ms, 3), "sigma_1": float(res.singular_values[0]), "sigma_1_se": float(res.singular_values_se[0]),
            "sigma_1_bias": float(res.singular_values_bias[0])}


def probe_bca(views):
    from cca_zoo_amd.model_selection import bootstrap

    n = views[0].shape[0]
    ms = {}
    for _ in range(2):                                   # the second round counts
        for method in ("percentile", "BCa"):
            t0 = time.perf_counter()
            res = bootstrap(estimator(), views, n_resamples=BCA_B, random_state=0, draws="device", method=method)
            ms[method] = (time.perf_counter() - t0) * 1e3
    return {"n": n, "p": [v.shape[1] for v in views], "B": BCA_B, "n_groups": int(res.n_groups), "percentile_ms": round(ms["percentile"], 2),
            "bca_ms": round(ms["BCa"], 2), "bca_over_percentile": round(ms["BCa"] / ms["percentile"], 3),
            "sigma_1": float(res.singular_values[0]), "sigma_1_ci_bca": [float(x) for x in res.singular_values_ci[:, 0]],
            "sigma_1_ci_percentile": [float(x) for x in res.singular_values_ci_percentile[:, 0]],
            "sigma_1_z0": float(res.singular_values_z0[0]), "sigma_1_acceleration": float(res.singular_values_acceleration[0])}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--parts", default="loo,groups,bca")
    ap.add_argument("--shapes", default="all", help="all, or n:p1:p2[,n:p1:p2...] (for every part asked for)")
    a = ap.parse_args(argv)
    parts = a.parts.split(",")
    fns = {"loo": probe_loo, "groups": probe_groups, "bca": probe_bca}
    ns = {"loo": LOO_NS, "groups": (GROUPS_N,), "bca": (BCA_N,)}
    res = {k: [] for k in parts}
    for k in parts:
        shapes = [(n, p1, p2) for n in ns[k] for p1, p2 in WIDTHS] if a.shapes == "all" else [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]
        for n, p1, p2 in shapes:
            res[k].append(fns[k](make_views(n, p1, p2)))
            print(json.dumps(res[k][-1]), file=sys.stderr, flush=True)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
