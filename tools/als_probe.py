#!/usr/bin/env python3
"""Measure the ALS sweep on one GPU and print one JSON object (``--out`` also writes it).

    python tools/als_probe.py [--out profiles/als_probe.json] [--only device|cpu] [--model PLS_ALS|SCCA_PMD|SCCA_ADMM]
                              [--sweeps 20]

device: PLS_ALS, SCCA_PMD and SCCA_ADMM sweeps through the C ABI on n = 4096, 2 x 262144 float32 features drawn on the device
        (ccz_randn_fill), k = 1, tol = 0, a fixed number of sweeps: ms per sweep between two stream synchronisations
        (the first, untimed call holds the scores of the initial vectors and the code-object loads), achieved bytes per
        second against the model 2 * sum_i n p_i 4 bytes per sweep, and PMD's extra time per sweep over PLS_ALS (the
        price of its 12 extra passes over raw per view).  SCCA_ADMM (tau = 0.1 / sqrt(p), mu = 1) also reports its one-off
        setup, the two 4096 x 4096 float64 Grams of ccz_als_admm_setup, between two synchronisations (best of three), and
        the time of a dimension's first iteration (which adds the Frobenius norm of the Gram) over a later one.  The
        per-kernel split comes from one
        ``rocprofv3 --kernel-trace --stats`` run of ``--only device --model SCCA_PMD`` and one of ``--model PLS_ALS``,
        summarised by tools/rocpd_stats.py (profiles/als_kernel_stats.md); ``--kernel-stats MODEL=TABLE.md`` reads such a
        table back and adds the split of the sweep's kernel time (rule kernels, one-workgroup kernels) to the JSON.
cpu:    the reference-structured float64 NumPy sweep (float64 copies of the views, two matrix-vector products per
        view) on the host cores at n = 512 with the same widths, scaled by 8 to n = 4096 (labelled as scaled).
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


def device(out, sweeps, models=("PLS_ALS", "SCCA_PMD")):
    import torch

    from cca_zoo_amd import _backend
    from cca_zoo_amd.linear._iterative import RULE_ADMM, RULE_NORMALISE, RULE_SOFT_L1, initial_vectors

    h = _backend.default_handle()
    views = []
    for i in range(2):
        x = torch.empty(N, P, device="cuda", dtype=torch.float32)
        h.check(h.lib.ccz_randn_fill(h.raw, _backend.F32, C.c_void_p(x.data_ptr()), N, P, P, 91 + i, 0, P, 1.0, 0))
        views.append(x)
    x = None
    h.sync()
    mus = [v.mean(dim=0) for v in views]
    torch.cuda.synchronize()
    varr = (_backend.View * 2)()
    for i, v in enumerate(views):
        varr[i].data, varr[i].cols, varr[i].ld = v.data_ptr(), P, v.stride(0)
    marr = (C.c_void_p * 2)(*[mu.data_ptr() for mu in mus])
    w0 = np.ascontiguousarray(initial_vectors(0, [P, P], 1))
    model_bytes = 2 * 2 * N * P * 4
    res = {}
    for name, rule, par in (("PLS_ALS", RULE_NORMALISE, [0.0, 0.0]),
                            ("SCCA_PMD", RULE_SOFT_L1, [0.02 * np.sqrt(P)] * 2),
                            ("SCCA_ADMM", RULE_ADMM, [0.1 / np.sqrt(P)] * 2)):
        if name not in models:
            continue
        state = C.c_void_p()
        h.check(h.lib.ccz_als_create(h.raw, _backend.F32, 2, (C.c_int64 * 2)(P, P), N, 1, rule, (C.c_double * 2)(*par), 0.0,
                                     10 ** 6, sweeps, C.byref(state)))
        try:
            times, setup, first = [], [], []
            for rep in range(3 if rule == RULE_ADMM else 0):
                h.sync()
                t0 = time.perf_counter()
                h.check(h.lib.ccz_als_admm_setup(h.raw, state, varr, marr, 1.0))
                h.sync()
                setup.append(time.perf_counter() - t0)
            for rep in range(4):
                h.check(h.lib.ccz_als_set_init(h.raw, state, w0.ctypes.data_as(C.POINTER(C.c_double))))
                a, b = C.c_int64(0), C.c_int(0)
                h.sync()
                t0 = time.perf_counter()
                h.check(h.lib.ccz_als_sweeps(h.raw, state, varr, marr, 1, C.byref(a), C.byref(b)))
                h.sync()
                if rep:
                    first.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                h.check(h.lib.ccz_als_sweeps(h.raw, state, varr, marr, sweeps, C.byref(a), C.byref(b)))
                h.sync()
                if rep:
                    times.append(time.perf_counter() - t0)
            ms = min(times) / sweeps * 1e3
            wv = np.empty(P)
            h.check(h.lib.ccz_als_peek(h.raw, state, 0, 0, wv.ctypes.data_as(C.POINTER(C.c_double))))
            res[name] = {"ms_per_sweep": round(ms, 4), "tb_per_s": round(model_bytes / (ms * 1e-3) / 1e12, 3),
                         "timed_runs_ms": [round(t / sweeps * 1e3, 4) for t in times],
                         "support_view0": int(np.count_nonzero(wv))}
            if rule == RULE_ADMM:
                res[name]["setup_grams_ms"] = round(min(setup) * 1e3, 2)
                res[name]["setup_runs_ms"] = [round(t * 1e3, 2) for t in setup]
                res[name]["first_iteration_ms"] = round(min(first) * 1e3, 4)
        finally:
            h.check(h.lib.ccz_als_destroy(h.raw, state))
    out["device"] = {
        "shape": {"n": N, "p": [P, P], "k": 1, "dtype": "float32", "sweeps": sweeps, "tol": 0.0},
        "model_bytes_per_sweep": model_bytes, **res,
    }
    if "PLS_ALS" in res and "SCCA_PMD" in res:
        extra = res["SCCA_PMD"]["ms_per_sweep"] - res["PLS_ALS"]["ms_per_sweep"]
        out["device"]["pmd_extra_ms_per_sweep_over_pls"] = round(extra, 4)
        out["device"]["pmd_extra_fraction_of_sweep"] = round(extra / res["SCCA_PMD"]["ms_per_sweep"], 4)
    if "PLS_ALS" in res and "SCCA_ADMM" in res:
        out["device"]["admm_extra_ms_per_iteration_over_pls"] = round(res["SCCA_ADMM"]["ms_per_sweep"] - res["PLS_ALS"]["ms_per_sweep"], 4)


def cpu(out, sweeps=2):
    n = 512
    rng = np.random.default_rng(0)
    xs = [rng.standard_normal((n, P)) for _ in range(2)]                # the reference's float64 copies
    w = [rng.standard_normal(P) for _ in range(2)]
    w = [wi / np.linalg.norm(wi) for wi in w]
    ts = []
    for _ in range(sweeps + 1):
        t0 = time.perf_counter()
        for i in range(2):
            t = xs[1 - i] @ w[1 - i]
            t = t / np.linalg.norm(t)
            raw = xs[i].T @ t
            w[i] = raw / np.linalg.norm(raw)
        ts.append(time.perf_counter() - t0)
    per = float(min(ts[1:]))
    out["cpu_comparator"] = {
        "what": "reference-structured float64 NumPy PLS_ALS sweep on host copies, 2 x 512 x 262144, scaled x8 to n = 4096",
        "threads": os.environ.get("OMP_NUM_THREADS", "unset"), "measured_n": n, "ms_per_sweep_measured": round(per * 1e3, 2),
        "ms_per_sweep_scaled_to_n4096": round(per * 8 * 1e3, 1), "scaled": True,
    }


RULE_KERNELS = ("k_als_fold", "k_als_levels", "k_als_norm", "k_als_apply", "k_als_admm_fold", "k_als_admm_apply")
ONE_WORKGROUP_KERNELS = ("k_als_prologue", "k_als_admm_prologue", "k_als_finish", "k_als_advance", "k_als_admm_h",
                         "k_als_admm_lfinal")


def kernel_split(out, spec):
    """``MODEL=TABLE.md``: the share of the k_als_* kernel time of a profiled run (tools/rocpd_stats.py table) by kernel."""
    model, path = spec.split("=", 1)
    tot, calls = {}, {}
    with open(path) as f:
        for line in f:
            c = [x.strip() for x in line.split("|")]
            if len(c) == 9 and "k_als_" in c[1] and c[2].isdigit():     # the first table: kernel, calls, total ms, ...
                name = c[1].strip("`").split("::")[-1].split("<")[0]
                tot[name] = tot.get(name, 0.0) + float(c[3])
                calls[name] = calls.get(name, 0) + int(c[2])
    all_ms, sweeps = sum(tot.values()), calls["k_als_finish"]
    out.setdefault("kernel_split", {})[model] = {
        "source": "rocprofv3 --kernel-trace --stats, k_als_* kernels only", "sweeps_profiled": sweeps,
        "kernel_ms_per_sweep": round(all_ms / sweeps, 4),
        "ms_per_sweep_by_kernel": {k: round(v / sweeps, 4) for k, v in sorted(tot.items(), key=lambda kv: -kv[1])},
        "rule_kernels_fraction": round(sum(tot.get(k, 0.0) for k in RULE_KERNELS) / all_ms, 4),
        "one_workgroup_kernels_fraction": round(sum(tot.get(k, 0.0) for k in ONE_WORKGROUP_KERNELS) / all_ms, 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only", choices=["device", "cpu", "none"])
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="MODEL=TABLE.md")
    ap.add_argument("--model", choices=["PLS_ALS", "SCCA_PMD", "SCCA_ADMM"], help="device part: this model alone (for a profiler run)")
    ap.add_argument("--sweeps", type=int, default=20)
    a = ap.parse_args()
    out = {}
    if a.only in (None, "device"):
        device(out, a.sweeps, (a.model,) if a.model else ("PLS_ALS", "SCCA_PMD", "SCCA_ADMM"))
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
