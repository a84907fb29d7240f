#!/usr/bin/env python3
"""TreeCCA timing probe (not a test, not in bench.py): time per boosting round of ``TreeCCA.fit`` on CUDA-resident float32
views, by default n = 1e6, two views of p = 256, k = 4, depth 5, and the rate at which the histogram kernel's bin matrix is
read.

The time per round is the slope between a fit of ``--short`` and one of ``--long`` rounds (setup -- upload, cuts, bins, base
margin -- cancels).  A round reads ``views * depth * nsel * n`` bytes of the uint8 bin matrix in ``k_tree_hist`` (every
level reads the column of every candidate feature once); that figure over the WHOLE round time is a lower bound on the
histogram kernel's own rate, printed against the 6.29 TB/s a float4 copy reaches on the MI355X.  There is no reference
timing: xgboost is not installed here.

    python tools/treecca_probe.py [--n 1000000 --p 256 --k 4 --depth 5 --short 2 --long 6] [--json out.json]
"""
import argparse
import json
import time

import numpy as np
import torch

from cca_zoo_amd.tree import TreeCCA

HBM_COPY = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=256)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--short", type=int, default=2)
    ap.add_argument("--long", type=int, default=6)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    lat = torch.randn(a.n, 8, device="cuda", generator=gen)
    views = [lat @ torch.randn(8, a.p, device="cuda", generator=gen) + torch.randn(a.n, a.p, device="cuda", generator=gen) for _ in range(2)]
    torch.cuda.synchronize()
    times = {}
    for rounds in (a.short, a.short, a.long):          # the first fit also warms up
        t0 = time.perf_counter()
        model = TreeCCA(latent_dimensions=a.k, n_estimators=rounds, max_depth=a.depth).fit(views)
        torch.cuda.synchronize()
        times[rounds] = time.perf_counter() - t0
    per_round = (times[a.long] - times[a.short]) / (a.long - a.short)
    nsel = max(1, int(np.floor(0.8 * a.p)))
    hist_bytes = 2 * a.depth * nsel * a.n
    splits = int(sum((b.feature >= 0).sum() for bs in model.boosters_ for b in bs))
    out = {"n": a.n, "p": a.p, "k": a.k, "depth": a.depth, "fit_s": {str(r): t for r, t in times.items()}, "round_s": per_round,
           "setup_s": times[a.short] - a.short * per_round, "bin_bytes_per_round": hist_bytes,
           "bin_bytes_per_s_lower_bound": hist_bytes / per_round, "share_of_hbm_copy_rate": hist_bytes / per_round / HBM_COPY,
           "splits": splits}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
