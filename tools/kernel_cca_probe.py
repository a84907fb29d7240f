#!/usr/bin/env python3
"""Measure the nonparametric path on one GPU and print one JSON object (``--out`` also writes it).

    python tools/kernel_cca_probe.py [--out profiles/kernel_cca_probe.json] [--quick]
    python tools/kernel_cca_probe.py --reference /path/to/cca_zoo --merge profiles/kernel_cca_probe.json

The second form needs no GPU: it times the reference's own CPU ``KCCA.fit`` at n = 2000 (rbf, 2 views x 50 features,
latent_dimensions=1, the reference's defaults otherwise) and records it, with the host and its CPU count, in the
``reference_cpu_fit`` block of an existing result file.

Reports the kernel matrix at n = 16384, d = 1024 (rbf, symmetric: 2.7e11 flops counted as n^2 d), the fused projection at
n_train = 8192, n_test = 131072, d = 256, k = 16 (2 n_train n_test d + 2 n_train n_test k flops), and KCCA / KGCCA fits at
n = 4096 and 8192 (2 views, d = 256, rbf, k = 8) with the solve's phases (CCZ_TRACE_PHASES=1, synchronised boundaries).
"""

from __future__ import annotations

import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_F64_TFLOPS = 78.6


def timed(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return sorted(t)[len(t) // 2]


class StderrCapture:
    """Collect what the C library prints to fd 2 (the solve's phase lines)."""

    def __enter__(self):
        self.f = tempfile.TemporaryFile(mode="w+")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.f.fileno(), 2)
        return self

    def __exit__(self, *a):
        sys.stderr.flush()
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.f.seek(0)
        self.text = self.f.read()
        self.f.close()


def reference_cpu_fit(path, n=2000, d=50, reps=3):
    """Median wall time of the reference's ``KCCA(kernel="rbf").fit`` on this host (NumPy / SciPy on the CPU)."""
    import importlib.metadata as md
    import platform
    import types

    import numpy as np

    sys.path.insert(0, path)
    orig = md.version
    md.version = lambda name: "0.0.0+probe" if name == "cca_zoo" else orig(name)
    if "tensorly" not in sys.modules:      # KTCCA's import only; never called here
        tl = types.ModuleType("tensorly")
        tl.set_backend = lambda *a, **k: None
        dec = types.ModuleType("tensorly.decomposition")
        dec.parafac = None
        tl.decomposition = dec
        sys.modules["tensorly"], sys.modules["tensorly.decomposition"] = tl, dec
    from cca_zoo.nonparametric import KCCA

    rng = np.random.default_rng(0)
    views = [rng.standard_normal((n, d)) for _ in range(2)]
    KCCA(kernel="rbf").fit(views)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        KCCA(kernel="rbf").fit(views)
        t.append(time.perf_counter() - t0)
    return {"model": "KCCA", "n": n, "d": [d, d], "kernel": "rbf", "latent_dimensions": 1, "s": sorted(t)[len(t) // 2],
            "runs": reps, "host": platform.node(), "host_cpus": os.cpu_count(),
            "note": "the reference's CPU fit, timed by `kernel_cca_probe.py --reference` on the host named here "
                    "(not on the GPU run above)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="smaller sizes (a functional check of the probe itself)")
    ap.add_argument("--reference", help="path of a cca_zoo checkout: time its CPU KCCA.fit instead of the GPU probe")
    ap.add_argument("--merge", help="with --reference: result file whose reference_cpu_fit block is (re)written")
    a = ap.parse_args()
    if a.reference:
        block = reference_cpu_fit(a.reference)
        print(json.dumps(block, indent=1))
        if a.merge:
            with open(a.merge) as f:
                res = json.load(f)
            res["reference_cpu_fit"] = block
            with open(a.merge, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        return
    os.environ.setdefault("CCZ_TRACE_PHASES", "1")
    import torch

    from cca_zoo_amd import _backend
    from cca_zoo_amd.nonparametric import KCCA, KGCCA
    from cca_zoo_amd.nonparametric._kernel_base import _DevView, kernel_project, pairwise_kernel

    q = a.quick
    res = {"device": torch.cuda.get_device_name(0), "peak_f64_tflops": PEAK_F64_TFLOPS}
    g = torch.Generator(device="cuda").manual_seed(0)
    h = _backend.default_handle()

    n, d = (2048, 256) if q else (16384, 1024)
    X = torch.randn((n, d), device="cuda", dtype=torch.float64, generator=g)
    K = torch.empty((n, n), device="cuda", dtype=torch.float64)
    dv = _DevView(h, X)
    spec = (2, 1.0 / d, 1.0, 1.0)
    ms = timed(lambda: pairwise_kernel(h, dv, dv, spec, K.data_ptr(), n), 5)
    fl = float(n) * n * d
    res["kernel_matrix"] = {"n": n, "d": d, "kernel": "rbf", "ms": ms, "flops": fl, "tflops": fl / ms / 1e9,
                            "fraction_of_peak": fl / ms / 1e9 / PEAK_F64_TFLOPS}
    del K, X

    na, nb, d, k = (2048, 16384, 256, 16) if q else (8192, 131072, 256, 16)
    A = torch.randn((na, d), device="cuda", dtype=torch.float64, generator=g)
    B = torch.randn((nb, d), device="cuda", dtype=torch.float64, generator=g)
    W = torch.randn((na, k), device="cuda", dtype=torch.float64, generator=g)
    out = torch.empty((nb, k), device="cuda", dtype=torch.float64)
    da, db = _DevView(h, A), _DevView(h, B)
    ms = timed(lambda: kernel_project(h, da, db, spec, W.data_ptr(), k, out.data_ptr(), k), 5)
    fl = 2.0 * na * nb * d + 2.0 * na * nb * k
    res["kernel_project"] = {"n_train": na, "n_test": nb, "d": d, "k": k, "ms": ms, "flops": fl, "tflops": fl / ms / 1e9,
                             "fraction_of_peak": fl / ms / 1e9 / PEAK_F64_TFLOPS}
    del A, B, W, out

    fits = []
    for n in ((1024, 2048) if q else (4096, 8192)):
        z = torch.randn((n, 2), device="cuda", dtype=torch.float64, generator=g)
        views = [torch.tanh(z @ torch.randn((2, 256), device="cuda", dtype=torch.float64, generator=g))
                 + torch.randn((n, 256), device="cuda", dtype=torch.float64, generator=g) for _ in range(2)]
        for est in (KCCA, KGCCA):
            m = est(latent_dimensions=8, kernel="rbf")
            m.fit(views)                                   # warm-up (pool, code objects)
            torch.cuda.synchronize()
            with StderrCapture() as cap:
                t0 = time.perf_counter()
                m.fit(views)
                torch.cuda.synchronize()
                total = (time.perf_counter() - t0) * 1e3
            phases = {}
            for line in cap.text.splitlines():
                if "phases (ms):" in line:
                    for name, v in re.findall(r"(\w+) ([0-9.]+)", line.split("phases (ms):")[1]):
                        phases[name] = float(v)
            solve = sum(phases.values())
            fits.append({"model": est.__name__, "n": n, "d": 256, "k": 8, "fit_ms": total,
                         "phases_ms": {"kernel_and_rest": total - solve, **phases}})
    res["fits"] = fits
    res["note"] = ("the GPU numbers were measured on the run that wrote this file; phase boundaries are synchronised "
                   "(CCZ_TRACE_PHASES=1)")
    js = json.dumps(res, indent=1)
    print(js)
    if a.out:
        with open(a.out, "w") as f:
            f.write(js + "\n")


if __name__ == "__main__":
    main()
