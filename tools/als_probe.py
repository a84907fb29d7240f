#!/usr/bin/env python3
"""Measure the ALS sweep on one GPU and print one JSON object (``--out`` also writes it).

    python tools/als_probe.py [--out profiles/als_probe.json] [--only device|cpu] [--model PLS_ALS|SCCA_PMD|SCCA_ADMM]
                              [--sweeps 20]
    python tools/als_probe.py --model SCCA_IPLS|ElasticCCA [--out profiles/als_probe.json] [--only device|cpu]

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
enet:   ``--model SCCA_IPLS`` / ``ElasticCCA``: the estimator itself (k = 1, alpha = 0.05, l1_ratio = 0.5, tol = 1e-6, at most 20
        sweeps) on float32 CUDA tensors at a tall shape (n = 4096, p = 1024 + 768) and a wide one (n = 256, p = 4096 + 2048):
        ms per outer sweep (fit wall time over ``n_iter_``, warm), CD sweeps per solve, the one-off Gram time
        (ccz_als_enet_setup between two synchronisations, best of three), and PLS_ALS on the same tensors for the same
        number of sweeps -- the two streaming passes without a solve -- from which the share of the CD kernels is
        estimated.  Beside them the same fit by a scikit-learn-structured CPU restatement (float64 copies deflated
        explicitly, ``ElasticNet(selection="random", warm_start=True)`` per view) on the host cores.
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


ENET_SHAPES = {"tall": (4096, (1024, 768)), "wide": (256, (4096, 2048))}
ENET_PAR = dict(latent_dimensions=1, alpha=0.05, l1_ratio=0.5, tol=1e-6, max_iter=20, random_state=0)


def _enet_views(n, dims):
    rng = np.random.default_rng(n)
    z = rng.standard_normal((n, 2))
    return [(z @ rng.standard_normal((2, d)) + rng.standard_normal((n, d))).astype(np.float32) for d in dims]


def enet_device(out, model):
    import torch

    import cca_zoo_amd.linear as lin
    from cca_zoo_amd import _backend

    h = _backend.default_handle()
    res = {}
    for tag, (n, dims) in ENET_SHAPES.items():
        tens = [torch.as_tensor(v, device="cuda") for v in _enet_views(n, dims)]
        times = []
        for _ in range(3):                       # the first fit loads the code objects
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            est = getattr(lin, model)(**ENET_PAR).fit(tens)
            times.append(time.perf_counter() - t0)
        sweeps = est.n_iter_[0]
        pls = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lin.PLS_ALS(latent_dimensions=1, tol=0.0, max_iter=sweeps, random_state=0).fit(tens)
            pls.append(time.perf_counter() - t0)
        # the one-off Gram through the C ABI
        m = len(dims)
        varr = (_backend.View * m)()
        for i, v in enumerate(tens):
            varr[i].data, varr[i].cols, varr[i].ld = v.data_ptr(), dims[i], v.stride(0)
        mus = [v.mean(dim=0) for v in tens]
        marr = (C.c_void_p * m)(*[mu.data_ptr() for mu in mus])
        state = C.c_void_p()
        zeros = (C.c_double * m)(*([0.0] * m))
        h.check(h.lib.ccz_als_create(h.raw, _backend.F32, m, (C.c_int64 * m)(*dims), n, 1, 5, zeros, 1e-6, 20, 8, C.byref(state)))
        setup = []
        try:
            for _ in range(3):
                h.sync()
                t0 = time.perf_counter()
                h.check(h.lib.ccz_als_enet_setup(h.raw, state, varr, marr, zeros, zeros, (C.c_int * m)(*([0] * m)), 0, 0))
                h.sync()
                setup.append(time.perf_counter() - t0)
        finally:
            h.check(h.lib.ccz_als_destroy(h.raw, state))
        fit_ms, pls_ms = min(times[1:]) * 1e3, min(pls[1:]) * 1e3
        res[tag] = {"n": n, "p": list(dims), "sweeps": sweeps, "fit_ms": round(fit_ms, 2), "ms_per_sweep": round(fit_ms / sweeps, 3),
                    "cd_sweeps_per_solve": round(est.n_inner_iter_[0] / (sweeps * m), 2), "gram_setup_ms": round(min(setup) * 1e3, 3),
                    "pls_als_fit_ms_same_sweeps": round(pls_ms, 2),
                    "cd_share_estimate": round(max(0.0, 1.0 - pls_ms / fit_ms), 3),
                    "support": [int(np.count_nonzero(w)) for w in est.weights_]}
    out.setdefault("enet_device", {})[model] = {"params": ENET_PAR, "dtype": "float32", **res,
                                                "note": "fit wall time includes upload-free setup, the Gram and the read-back; "
                                                        "cd_share_estimate = 1 - PLS_ALS fit time / fit time"}


def enet_cpu(out, model):
    """The reference's structure with scikit-learn's own solver: float64 copies, explicit deflation, random selection."""
    from sklearn.linear_model import ElasticNet

    res = {}
    for tag, (n, dims) in ENET_SHAPES.items():
        X = [v.astype(np.float64) for v in _enet_views(n, dims)]
        X = [x - x.mean(axis=0) for x in X]
        m = len(X)
        rng = np.random.default_rng(0)
        w = [rng.standard_normal(d) for d in dims]
        w = [x / np.linalg.norm(x) for x in w]
        regs = [ElasticNet(alpha=ENET_PAR["alpha"], l1_ratio=ENET_PAR["l1_ratio"], fit_intercept=False, warm_start=True,
                           tol=ENET_PAR["tol"], random_state=0, selection="random") for _ in X]
        t0 = time.perf_counter()
        sweeps = 0
        for sweeps in range(1, ENET_PAR["max_iter"] + 1):
            prev = [x.copy() for x in w]
            for i in range(m):
                t = sum(X[j] @ w[j] for j in range(m) if model == "ElasticCCA" or j != i)
                nt = np.linalg.norm(t)
                t = t / nt if nt > 1e-12 else t
                c = regs[i].fit(X[i], t).coef_.copy()
                if model == "SCCA_IPLS":
                    sd = (X[i] @ c).std()
                    c = c / sd if sd > 1e-12 else c
                w[i] = c
            if max(np.linalg.norm(a - b) for a, b in zip(w, prev)) < ENET_PAR["tol"]:
                break
        dt = time.perf_counter() - t0
        res[tag] = {"n": n, "p": list(dims), "sweeps": sweeps, "fit_ms": round(dt * 1e3, 2), "ms_per_sweep": round(dt * 1e3 / sweeps, 3)}
    out.setdefault("enet_cpu_comparator", {})[model] = {
        "what": "scikit-learn-structured float64 fit on host copies (ElasticNet, selection=random, warm start)",
        "threads": os.environ.get("OMP_NUM_THREADS", "unset"), **res}


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
    ap.add_argument("--model", choices=["PLS_ALS", "SCCA_PMD", "SCCA_ADMM", "SCCA_IPLS", "ElasticCCA"],
                    help="device part: this model alone (for a profiler run); SCCA_IPLS / ElasticCCA: the elastic-net probe")
    ap.add_argument("--sweeps", type=int, default=20)
    a = ap.parse_args()
    out = {}
    if a.model in ("SCCA_IPLS", "ElasticCCA"):
        if a.only in (None, "device"):
            enet_device(out, a.model)
        if a.only in (None, "cpu"):
            enet_cpu(out, a.model)
    elif a.only in (None, "device"):
        device(out, a.sweeps, (a.model,) if a.model else ("PLS_ALS", "SCCA_PMD", "SCCA_ADMM"))
    if a.only in (None, "cpu") and a.model not in ("SCCA_IPLS", "ElasticCCA"):
        cpu(out)
    for spec in a.kernel_stats:
        kernel_split(out, spec)
    if a.out:
        prev = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                prev = json.load(f)
        for key, val in out.items():
            if key in ("kernel_split", "enet_device", "enet_cpu_comparator"):
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
