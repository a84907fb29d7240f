#!/usr/bin/env python3
"""Measure the ALS sweep on sparse views against the dense sweep on ``toarray()`` of the same matrices, on one GPU, and
print one JSON object (``--out`` also writes it).

    python tools/sparse_als_probe.py [--out profiles/sparse_als_probe.json] [--density 0.01 0.1] [--sweeps 20]

Shape n = 4096, 2 x 262144 float32 values, k = 1, tol = 0, a fixed number of sweeps, PLS_ALS and SCCA_PMD through the C
ABI.  Per density: two random matrices (Bernoulli mask, values |N(0, 1)| + 0.25) in canonical CSR / CSC form
(ccz_als_set_sparse, float64 means from ccz_sparse_colmeans), and beside them the dense fit on the same numbers as float32
CUDA rows (scattered on the device, so no dense host copy is made), timed in the same run: ms per sweep between two stream
synchronisations, best of three after an untimed first call.  Effective bytes per second are against the traffic model of
DESIGN.md "Sparse views": per view 2 nnz (sizeof(V) + 4) bytes of values and indices, the int64 pointers of both forms, and
one pass over w (p doubles) and t~ (n doubles) for the gathers; the dense sweep reads 2 n p sizeof(V) per view.
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

N, P = 4096, 262144


def random_csr(seed, density):
    """A Bernoulli(density) mask over the n x p cells by geometric gaps between the stored cells (row-major), float32 values."""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    cells = N * P
    want = int(cells * density * 1.02) + 1024
    pos = np.cumsum(rng.geometric(density, size=want)) - 1
    pos = pos[pos < cells]
    val = (np.abs(rng.standard_normal(pos.size, dtype=np.float32)) + np.float32(0.25)).astype(np.float32)
    rows = pos // P
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=N), out=indptr[1:])
    return sp.csr_matrix((val, (pos % P).astype(np.int32), indptr), shape=(N, P)), pos


def timed_sweeps(h, state, varr, marr, w0, sweeps):
    times = []
    for rep in range(4):
        h.check(h.lib.ccz_als_set_init(h.raw, state, w0.ctypes.data_as(C.POINTER(C.c_double))))
        a, b = C.c_int64(0), C.c_int(0)
        h.check(h.lib.ccz_als_sweeps(h.raw, state, varr, marr, 1, C.byref(a), C.byref(b)))
        h.sync()
        t0 = time.perf_counter()
        h.check(h.lib.ccz_als_sweeps(h.raw, state, varr, marr, sweeps, C.byref(a), C.byref(b)))
        h.sync()
        if rep:
            times.append(time.perf_counter() - t0)
    return min(times) / sweeps * 1e3, [round(t / sweeps * 1e3, 4) for t in times]


def one_density(h, density, sweeps, seed):
    import torch

    from cca_zoo_amd import _backend
    from cca_zoo_amd._utils._resident import DeviceSparse, canonical_forms, sparse_group
    from cca_zoo_amd.linear._iterative import RULE_NORMALISE, RULE_SOFT_L1, initial_vectors

    t0 = time.perf_counter()
    mats = [random_csr(seed + i, density) for i in range(2)]
    forms = [canonical_forms(m, np.float32) for m, _ in mats]
    host_s = time.perf_counter() - t0
    nnz = [int(f[0].nnz) for f in forms]
    sparse = [DeviceSparse(h, *f) for f in forms]
    dense = []
    for (m, pos), (csr, _) in zip(mats, forms):                       # toarray() of the same numbers, formed on the device
        x = torch.zeros(N * P, device="cuda", dtype=torch.float32)
        x[torch.as_tensor(pos, device="cuda")] = torch.as_tensor(csr.data, device="cuda")
        dense.append(x.view(N, P))
    mats = forms = None
    mus32 = [x.mean(dim=0) for x in dense]
    torch.cuda.synchronize()
    mus64 = [h.alloc(P * 8) for _ in range(2)]
    for sv, mb in zip(sparse, mus64):
        h.check(h.lib.ccz_sparse_colmeans(h.raw, _backend.F32, C.byref(sv.view), C.c_void_p(mb.ptr)))
    varr_d, varr_s = (_backend.View * 2)(), (_backend.View * 2)()
    for i, x in enumerate(dense):
        varr_d[i].data, varr_d[i].cols, varr_d[i].ld = x.data_ptr(), P, x.stride(0)
        varr_s[i].data, varr_s[i].cols, varr_s[i].ld = None, P, P
    marr_d = (C.c_void_p * 2)(*[mu.data_ptr() for mu in mus32])
    marr_s = (C.c_void_p * 2)(*[mb.ptr for mb in mus64])
    w0 = np.ascontiguousarray(initial_vectors(0, [P, P], 1))
    bytes_sparse = sum(2 * z * (4 + 4) + 8 * (N + 1) + 8 * (P + 1) + 8 * P + 8 * N for z in nnz)
    bytes_dense = 2 * 2 * N * P * 4
    res = {"density": density, "nnz": nnz, "host_generation_and_canonical_forms_s": round(host_s, 1),
           "group_rows": [sparse_group(z, N) for z in nnz], "group_cols": [sparse_group(z, P) for z in nnz],
           "model_bytes_per_sweep_sparse": bytes_sparse, "model_bytes_per_sweep_dense": bytes_dense,
           "model_bytes_ratio": round(bytes_sparse / bytes_dense, 4)}
    for name, rule, par in (("PLS_ALS", RULE_NORMALISE, [0.0, 0.0]), ("SCCA_PMD", RULE_SOFT_L1, [0.02 * np.sqrt(P)] * 2)):
        out = {}
        for kind, varr, marr in (("sparse", varr_s, marr_s), ("dense", varr_d, marr_d)):
            state = C.c_void_p()
            h.check(h.lib.ccz_als_create(h.raw, _backend.F32, 2, (C.c_int64 * 2)(P, P), N, 1, rule, (C.c_double * 2)(*par), 0.0,
                                         10 ** 6, sweeps, C.byref(state)))
            try:
                if kind == "sparse":
                    for i, sv in enumerate(sparse):
                        h.check(h.lib.ccz_als_set_sparse(h.raw, state, i, C.byref(sv.view)))
                ms, runs = timed_sweeps(h, state, varr, marr, w0, sweeps)
                model = bytes_sparse if kind == "sparse" else bytes_dense
                out[kind] = {"ms_per_sweep": round(ms, 4), "timed_runs_ms": runs, "effective_gb_per_s": round(model / (ms * 1e-3) / 1e9, 1)}
            finally:
                h.check(h.lib.ccz_als_destroy(h.raw, state))
        out["dense_over_sparse"] = round(out["dense"]["ms_per_sweep"] / out["sparse"]["ms_per_sweep"], 2)
        res[name] = out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--density", type=float, nargs="+", default=[0.01, 0.1])
    ap.add_argument("--sweeps", type=int, default=20)
    a = ap.parse_args()
    from cca_zoo_amd import _backend

    h = _backend.default_handle()
    out = {"shape": {"n": N, "p": [P, P], "k": 1, "values": "float32", "sweeps": a.sweeps, "tol": 0.0},
           "device": h.device_info()["name"], "densities": [one_density(h, d, a.sweeps, 17 + 10 * i) for i, d in enumerate(a.density)]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=2)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
