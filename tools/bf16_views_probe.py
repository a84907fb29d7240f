#!/usr/bin/env python3
"""Measure the closed-form path on bfloat16 against float32 device views on one GPU; print one JSON object (``--out`` also writes
it: profiles/bf16_views_probe.json).

``transform`` of one rows x width view at k = 16, 32, 64, four ways that alternate inside every round:

    bf16_kernel        ccz_transform_wide on the bf16 rows (csrc/project_bf16.hip)
    bf16_adapter       the same call with CCZ_PROJECT_BF16=0 (widened into float32 scratch, then the float32 projection)
    float_then_f32     what a caller had to do before: v.float() and ccz_transform(CCZ_F32), conversion included
    f32_alone          ccz_transform(CCZ_F32) on float32 rows that exist already

and ``CCA(64).fit`` on two views of the benchmark's latent-variable data (rounded to bfloat16; the float32 views hold the same
numbers), with the device memory in use right after each fit (views + the handle's pooled scratch, which keeps its high-water
mark; the pool is trimmed before each measurement).  Medians over the rounds, device events around the calls.

    python tools/bf16_views_probe.py --out profiles/bf16_views_probe.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fit-k", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from cca_zoo_amd import _backend
    from cca_zoo_amd.linear import CCA

    assert torch.cuda.is_available(), "bf16_views_probe needs a GPU"
    H = _backend.default_handle(0)
    n, d = a.rows, a.width
    torch.zeros(1, device="cuda")

    def used_gb():
        free, total = torch.cuda.mem_get_info()
        return (total - free) / 1e9

    def trim():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        H.pool_trim()

    def view(seed, dtype):
        g = torch.Generator(device="cuda").manual_seed(seed)
        out = torch.empty((n, d), dtype=dtype, device="cuda")
        step = max(1, (1 << 27) // d)
        lat_w = torch.randn(8, d, device="cuda", generator=g)
        for r0 in range(0, n, step):                       # in row blocks: no second full-size float32 temporary
            r1 = min(n, r0 + step)
            lat = torch.randn(r1 - r0, 8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1000 + r0))
            out[r0:r1] = (lat @ lat_w + torch.randn(r1 - r0, d, device="cuda", generator=g) + 0.3).to(dtype)
        return out

    def project(name, code, x, mean, W, out):
        sp = int(torch.cuda.current_stream().cuda_stream)
        H.acquire(sp)
        H.check(getattr(H.lib, name)(H.raw, code, C.c_void_p(x.data_ptr()), x.shape[0], x.shape[1], x.stride(0), C.c_void_p(mean.data_ptr()),
                                     C.c_void_p(W.data_ptr()), W.shape[1], C.c_void_p(out.data_ptr()), out.stride(0)))
        H.release(sp)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def route():
        r = C.c_int(0)
        H.check(H.lib.ccz_transform_last_route(H.raw, C.byref(r)))
        return r.value

    empty = used_gb()                                      # the context and the handle, before any view exists
    result = {"device": torch.cuda.get_device_name(0), "rows": n, "width": d, "rounds": a.rounds, "warmup": a.warmup, "transform": [],
              "model_ms_bf16_read": n * d * 2 / 5.5e9}

    # ---- transform -------------------------------------------------------------------------------------------------
    xb = view(1, torch.bfloat16)
    xf = xb.float()
    rng = np.random.default_rng(0)
    mean = torch.from_numpy(rng.standard_normal(d)).cuda()
    for k in (16, 32, 64):
        W = torch.from_numpy(rng.standard_normal((d, k)) / np.sqrt(d)).cuda()
        out = torch.empty((n, k), dtype=torch.float32, device="cuda")

        def bf16_kernel():
            os.environ.pop("CCZ_PROJECT_BF16", None)
            project("ccz_transform_wide", _backend.BF16, xb, mean, W, out)

        def bf16_adapter():
            os.environ["CCZ_PROJECT_BF16"] = "0"
            project("ccz_transform_wide", _backend.BF16, xb, mean, W, out)
            os.environ.pop("CCZ_PROJECT_BF16", None)

        def float_then_f32():
            project("ccz_transform", _backend.F32, xb.float(), mean, W, out)

        def f32_alone():
            project("ccz_transform", _backend.F32, xf, mean, W, out)

        ways = {"bf16_kernel": bf16_kernel, "bf16_adapter": bf16_adapter, "float_then_f32": float_then_f32, "f32_alone": f32_alone}
        times = {w: [] for w in ways}
        routes = {}
        for r in range(a.warmup + a.rounds):
            for w, fn in ways.items():
                t = timed(fn)
                if w.startswith("bf16"):
                    routes[w] = route()
                if r >= a.warmup:
                    times[w].append(t)
        row = {"k": k, "routes": routes}
        for w in ways:
            row[w] = {"ms_median": statistics.median(times[w]), "min": min(times[w]), "max": max(times[w])}
        row["bf16_kernel_over_float_then_f32"] = row["bf16_kernel"]["ms_median"] / row["float_then_f32"]["ms_median"]
        row["bf16_kernel_over_f32_alone"] = row["bf16_kernel"]["ms_median"] / row["f32_alone"]["ms_median"]
        row["bf16_kernel_read_TBps"] = n * d * 2 / row["bf16_kernel"]["ms_median"] / 1e9
        result["transform"].append(row)
        del out, W
    del xf
    trim()

    # ---- CCA(k).fit on two views --------------------------------------------------------------------------------------
    # the flagship workload's data (bench.py: JointData, k latent dimensions with scales 2 .. 0.5), rounded to bfloat16; the float32
    # views hold the same numbers
    from cca_zoo_amd.datasets import JointData

    del xb
    trim()
    fit = {"k": a.fit_k, "views": 2}
    jd = JointData(n_views=2, n_samples=n, latent_dimensions=a.fit_k, n_features=[d, d], signal_to_noise=1.0, random_state=0,
                   latent_scales=list(np.linspace(2.0, 0.5, a.fit_k)))
    drawn = jd.sample_device(device="cuda", dtype=torch.float32, n_samples=n, seed=1)
    sets = {"bfloat16": [v.to(torch.bfloat16) for v in drawn]}
    del drawn
    mem = {}
    trim()
    CCA(latent_dimensions=a.fit_k).fit(sets["bfloat16"])
    torch.cuda.synchronize()
    mem["bfloat16"] = used_gb() - empty
    trim()
    sets["float32"] = [v.float() for v in sets["bfloat16"]]
    CCA(latent_dimensions=a.fit_k).fit(sets["float32"])
    torch.cuda.synchronize()
    mem["float32"] = used_gb() - empty - sum(v.numel() * 2 for v in sets["bfloat16"]) / 1e9      # (the bf16 views are still resident)
    times = {s: [] for s in sets}
    detail = {}
    for r in range(a.warmup + a.rounds):
        for s, views in sets.items():
            holder = {}

            def run():
                holder["m"] = CCA(latent_dimensions=a.fit_k).fit(views)

            t = timed(run)
            detail[s] = {key: holder["m"].timings_[key] for key in ("moments_ms", "solve_ms", "k1_route")}
            if r >= a.warmup:
                times[s].append(t)
    for s in sets:
        fit[s] = {"fit_ms_median": statistics.median(times[s]), "min": min(times[s]), "max": max(times[s]), "last_fit": detail[s],
                  "views_gb": sum(v.numel() * v.element_size() for v in sets[s]) / 1e9, "in_use_after_fit_gb": mem[s]}
    fit["bfloat16_over_float32"] = fit["bfloat16"]["fit_ms_median"] / fit["float32"]["fit_ms_median"]
    result["fit"] = fit

    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
