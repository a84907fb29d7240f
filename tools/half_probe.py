#!/usr/bin/env python3
"""Measure ``CCALoss`` forward + backward on bfloat16 against float32 inputs on one GPU, and the split pass of K1 on bfloat16 against
float32 rows; print one JSON object (``--out`` also writes it: profiles/half_probe.json).

Two shapes: a DCCA batch (8192 x 2 x 512, default routes: the half batch is widened once and takes the float32 forward) and
262144 x 2 x 1024 with the split-bf16 route forced on the handle (the forward's K1 reads the half rows itself; the backward runs
through the row-chunk adapter).  The two dtypes alternate inside every round; the figures are medians over the rounds, device
events around forward + backward.  The split pass's own time comes from a timed ``ccz_moments`` (``ccz_moments_last_route``).

    python tools/half_probe.py --out profiles/half_probe.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from cca_zoo_amd import _backend
    from cca_zoo_amd.deep.objectives import CCALoss

    assert torch.cuda.is_available(), "half_probe needs a GPU"
    H = _backend.default_handle(0)
    loss_fn = CCALoss(eps=1e-4)

    def step_ms(z1, z2):
        z1.grad = z2.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss_fn([z1, z2]).backward()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def batch(n, d, dtype, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        lat = torch.randn(n, 16, device="cuda", generator=g)
        mk = lambda: (lat @ torch.randn(16, d, device="cuda", generator=g) + torch.randn(n, d, device="cuda", generator=g))   # noqa: E731
        return [mk().to(dtype).requires_grad_(True) for _ in range(2)]

    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup, "shapes": []}
    for n, d, route in ((8192, 512, "auto"), (262144, 1024, "bf16x2")):
        prev = H.k1_route(route)
        try:
            zs = {"float32": batch(n, d, torch.float32, 1), "bfloat16": batch(n, d, torch.bfloat16, 1)}
            times = {k: [] for k in zs}
            routes = {}
            for r in range(a.warmup + a.rounds):
                for k, (z1, z2) in zs.items():
                    t = step_ms(z1, z2)
                    if r >= a.warmup:
                        times[k].append(t)
                    routes[k] = H.loss_last_route()
            row = {"rows": n, "views": 2, "width": d, "k1_route": route}
            for k in zs:
                row[k] = {"fwd_bwd_ms_median": statistics.median(times[k]), "min": min(times[k]), "max": max(times[k]),
                          "loss_routes": routes[k]}
            row["bfloat16_over_float32"] = row["bfloat16"]["fwd_bwd_ms_median"] / row["float32"]["fwd_bwd_ms_median"]
            out["shapes"].append(row)
            del zs
        finally:
            H.k1_route(prev)
        torch.cuda.empty_cache()

    # the split pass alone: a timed ccz_moments on the forced route, float32 against bfloat16 rows of the same numbers
    n, d = 262144, 1024
    D = 2 * d
    mom = H.alloc((D * D + D) * 8)
    prev = H.k1_route("bf16x2")
    try:
        split = {}
        for name, dtype, code in (("float32", torch.float32, _backend.F32), ("bfloat16", torch.bfloat16, _backend.BF16)):
            z1, z2 = [z.detach() for z in batch(n, d, dtype, 1)]
            torch.cuda.synchronize()
            ms = []
            for r in range(a.warmup + a.rounds):
                H.moments([(z1.data_ptr(), d, d), (z2.data_ptr(), d, d)], n, code, True, mom.ptr)
                taken, split_ms, mfma_ms, reduce_ms = H.moments_last_route()
                assert taken == "bf16x2"
                if r >= a.warmup:
                    ms.append((split_ms, mfma_ms, reduce_ms))
            split[name] = {"split_ms_median": statistics.median(m[0] for m in ms), "mfma_ms_median": statistics.median(m[1] for m in ms),
                           "reduce_ms_median": statistics.median(m[2] for m in ms)}
            del z1, z2
            torch.cuda.empty_cache()
        split["rows"], split["views"], split["width"] = n, 2, d
        split["bytes_per_element"] = {"float32": 8, "bfloat16": 6}      # read + the two planes written
        out["split_pass"] = split
    finally:
        H.k1_route(prev)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
