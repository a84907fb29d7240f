"""The kernel paths behind libccz's runtime switches (cca_zoo_amd/csrc/env.h), each run once at a small shape that still
reaches it, against float64 NumPy (or the oracle's closed form where the existing test of the operation uses it), with the
bound the existing test of the same operation puts on the default path.

Rows marked ONCE, LOAD or HANDLE are read once per process: their paths run in a fresh child (tests/switch_paths_child.py,
one child at a time) that inherits the variables.  LIVE rows are set here, in process.  profiles/switch_paths_kernels.md
lists the kernels every child dispatched."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CHILD = os.path.join(ROOT, "tests", "switch_paths_child.py")

# One entry per child.  Switches share a child only where none of them decides whether another one's site is reached.
CASES = {
    # the two staged K1 kernels: launch_gram_f32 reads GRAM_IMPL only for fp32 views, launch_gram_f64 reads GRAM64_IMPL only for
    # fp64 views -- no launch reads both
    "k1_staged": {"CCZ_GRAM_IMPL": "0", "CCZ_GRAM64_IMPL": "0"},
    # GRAM_ROWS=256 is what makes a 16384-row launch a sliced grid (ntiles * ksplit >= 16 * ncu); GRAM_MAP picks the tile order
    # and the slicing of such a grid.  GRAM_ROWS alone is the next child.
    "k1_supertile": {"CCZ_GRAM_MAP": "0", "CCZ_GRAM_ROWS": "256"},
    "k1_rows": {"CCZ_GRAM_ROWS": "256"},
    # GRAM_FIFO_PILOT is read for pilot-shifted fp32 views on a sliced grid (GRAM_PILOT=1 and GRAM_ROWS=256 bring the probe
    # there; GRAM_IMPL stays 1, which would mask it).  GRAM_PARTIAL_MB is read on grids that are NOT sliced, GRAM64_IMPL for fp64
    # views: neither meets the first site.
    "k1_fifo_pilot": {"CCZ_GRAM_FIFO_PILOT": "0", "CCZ_GRAM_PILOT": "1", "CCZ_GRAM_ROWS": "256", "CCZ_GRAM_PARTIAL_MB": "0",
                      "CCZ_GRAM64_IMPL": "0"},
    # K1's pilot switches mask each other (GRAM_PILOT=0 ends automatic mode, where GRAM_PILOT_RATIO is read), so each shares a
    # child with fp64-GEMM switches instead: K1 never calls ccz_gemm_f64's dispatch.  BIG_MIN_TILES / BIG_MIN_K are the two
    # thresholds of one eligibility test.
    "pilot_never_gemm_big": {"CCZ_GRAM_PILOT": "0", "CCZ_GEMM_BIG_MIN_TILES": "1", "CCZ_GEMM_BIG_MIN_K": "16"},
    # GEMM_SKINNY_OFF is read first for every product, GEMM_HALF_TILE inside the big kernel's launch at the DEFAULT thresholds
    # (the probe adds a shape that takes it by default), GEMM_NN_IMPL by the fp32 product of ccz_transform
    "pilot_ratio_gemm_alt": {"CCZ_GRAM_PILOT_RATIO": "0.1", "CCZ_GEMM_HALF_TILE": "0", "CCZ_GEMM_SKINNY_OFF": "1",
                             "CCZ_GEMM_NN_IMPL": "0"},
    # super-blocked Cholesky (d > 1024): the look-ahead stream is on, so CHAIN_WGS_LA is read; CHAIN_SLEEP by every chain launch;
    # BACKPROJ_SPLIT by the batched back-projection of the rCCA solve.  The small-EVD generation and the block Jacobi's knobs
    # belong to other files and sizes (d <= 96 / d > 160) and none of them changes which factorization runs.
    "chol_eig_a": {"CCZ_POTRF_SB": "256", "CCZ_CHAIN_WGS_LA": "2", "CCZ_CHAIN_SLEEP": "8", "CCZ_BACKPROJ_SPLIT": "1",
                   "CCZ_SYEV_TWOSIDED": "1", "CCZ_EVD_REFRESH_MIN": "128", "CCZ_BJ_GROUP_MIN_TILES": "1", "CCZ_BJ_GRAM_SPLIT": "1",
                   "CCZ_RR1_TOL": "0"},
    # POTRF_LOOKAHEAD=0 masks CHAIN_WGS_LA (previous child); without the rider the first whitening solve is a launch sequence of
    # its own; CHEB_MAXDEG / CHEB_FIRSTCAP cap the same filter degree
    "chol_eig_b": {"CCZ_POTRF_SB": "1024", "CCZ_POTRF_LOOKAHEAD": "0", "CCZ_POTRF_RIDER": "0", "CCZ_BACKPROJ_SPLIT": "7",
                   "CCZ_SYEV_TWOSIDED": "0", "CCZ_BJ_GRAM_SPLIT": "3", "CCZ_CHEB_MAXDEG": "6", "CCZ_CHEB_FIRSTCAP": "2"},
    # SYEV_CHASE is read only by the default small-EVD generation (SYEV_TWOSIDED=2); CHEB_MARGIN by the filter design; K1_ROUTE
    # by ccz_moments, which no eigensolver calls
    "chase_margin_route": {"CCZ_SYEV_CHASE": "0", "CCZ_CHEB_MARGIN": "1", "CCZ_K1_ROUTE": "bf16x2"},
    # the loss's K1 (gram_partials_f32) and the host-view pipeline (moments_impl) are different entry points; H2D_CHUNK_MB (LIVE)
    # only cuts the 64 MiB input into chunks
    "loss_h2d": {"CCZ_LOSS_K1_FIFO": "0", "CCZ_H2D_PINNED_DIRECT": "0", "CCZ_H2D_CHUNK_MB": "16"},
    # GRAPHS=0: chains are issued directly; SPIN_WAIT_MS=0: host waits block.  Neither decides whether the other is consulted.
    "handle": {"CCZ_GRAPHS": "0", "CCZ_SPIN_WAIT_MS": "0"},
    # traces never change results
    "traces": {"CCZ_TRACE_PHASES": "1", "CCZ_TRACE_SOLVER": "1", "CCZ_TRACE_POOL": "1", "CCZ_TRACE_D2H": "1", "CCZ_CHAIN_DEBUG": "1",
               "CCZ_BJ_DEBUG": "1"},
}
assert len(CASES) <= 12


def run_child(case, timeout=120):
    e = dict(os.environ)
    for k in [k for k in e if k.startswith("CCZ_") and k not in ("CCZ_DEVICE",)]:
        del e[k]                                         # a child sees its case's switches and no others
    e.update(CASES[case])
    return subprocess.run([sys.executable, CHILD, case], env=e, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("case", [c for c in CASES if c != "traces"])
def test_switch_paths_in_a_child_process(case):
    r = run_child(case)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]


def test_trace_switches_change_no_result_and_write_to_stderr():
    r = run_child("traces")
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
    for mark in ("[ccz] topk", "[ccz] rayleigh_ritz", "[ccz] pool miss", "[ccz] d2h"):
        assert mark in r.stderr, (mark, r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------
# LIVE rows, in process
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def H():
    from cca_zoo_amd import _backend

    h = _backend.default_handle(0)
    yield h
    h.k1_route("auto")


def _split_plan(n, dims, split_rows, ncu, walk):
    """gram_split.hip split_row_plan for ONE launch of n rows, restated: (ksplit, sliced, chunk-per-XCD walk)."""
    ksteps, max_steps = -(-n // 16), max(1, split_rows // 16)
    npan = sum(-(-d // 256) for d in dims)
    ntiles = npan * (npan + 1) // 2
    kmin = max(1, -(-ksteps // max_steps))
    kmax = max(kmin, min(ksteps // 16, 8192))
    best, best_k = 1e300, 1
    for ks in range(kmin, kmax + 1):
        steps = -(-ksteps // ks)
        big = ntiles * ks >= 16 * ncu
        if big and ks % 8 == 0:
            rounds = -(-((ks // 8) * ntiles) // (ncu // 8))
        elif big:
            rounds = -(-(((ntiles + 7) // 8) * ks) // (ncu // 8))
        else:
            rounds = -(-(ntiles * ks) // ncu)
        cost = (1.03 if big and ks % 8 else 1.0) * rounds * (steps + 24)
        if cost < best:
            best, best_k = cost, ks
    steps = -(-ksteps // best_k)
    ksplit = -(-ksteps // steps)
    sliced = ntiles * ksplit >= 16 * ncu
    return ksplit, sliced, sliced and ksplit % 8 == 0 and not walk


@pytest.fixture(scope="module")
def split_inputs():
    """The rows of test_split_route_matches_float64 with their float64 moments: formed once, shared, left unchanged."""
    from test_gpu_k1_split import _latent, _ref

    out = {}
    for n, dims, shift in ((8192, [512, 512], 0.0), (5000, [300, 520], 0.0), (4099, [257, 63], 0.0), (20000, [256, 256], 10.0),
                           (33000, [128, 384, 200], 0.5), (40000, [1000], 0.0)):
        views = _latent(n, dims, seed=n + len(dims), shift=shift)
        out[n] = (dims, views, _ref(views))
    return out


def _split_check(H, views, ref):
    from test_gpu_k1_split import _moments, _rel

    G, s, taken, mom = _moments(H, views, "bf16x2")
    mom.free()
    assert taken == "bf16x2"
    assert _rel(G, ref[0]) < 2e-6                                        # tests/test_gpu_k1_split.py:90
    np.testing.assert_allclose(s, ref[1], rtol=1e-12, atol=1e-7)         # tests/test_gpu_k1_split.py:91


@pytest.mark.parametrize("n", [8192, 5000, 4099, 20000, 33000, 40000])
def test_split_pass_with_row_blocks_fastest(H, split_inputs, monkeypatch, n):
    """CCZ_SPLIT_ORDER=0: gram_split.hip launch_split_pass reads it in every split-route launch (grid (row blocks, panels) in
    place of (panels, row blocks)); no condition on the shape."""
    monkeypatch.setenv("CCZ_SPLIT_ORDER", "0")
    dims, views, ref = split_inputs[n]
    _split_check(H, views, ref)


@pytest.mark.parametrize("walk", [None, "1"])
@pytest.mark.parametrize("n,split_rows", [(8192, "16"), (33000, "48")])
def test_split_gram_on_a_sliced_grid_both_walks(H, split_inputs, monkeypatch, n, split_rows, walk):
    """CCZ_SPLIT_WALK=1: gram_split.hip split_row_plan reads it when the grid is sliced (ntiles * ksplit >= 16 * ncu) and
    ksplit % 8 == 0.  Of the six shapes only two can get there by shortening CCZ_SPLIT_ROWS: 8192 x [512, 512] (10 tiles, 512
    k-steps: one k-step per workgroup, ksplit 512) and 33000 x [128, 384, 200] (10 tiles, 2063 k-steps: three per workgroup,
    ksplit 688); the others have too few tiles or no chunk count that is a multiple of 8.  walk=None is the default
    chunk-per-XCD walk on the same grid, which no other test reaches either."""
    monkeypatch.setenv("CCZ_SPLIT_ROWS", split_rows)
    if walk:
        monkeypatch.setenv("CCZ_SPLIT_WALK", walk)
    dims, views, ref = split_inputs[n]
    ksplit, sliced, xchunks = _split_plan(n, dims, int(split_rows), H.device_info()["compute_units"], bool(walk))
    assert sliced and ksplit % 8 == 0 and xchunks == (walk is None), (ksplit, sliced, xchunks)
    _split_check(H, views, ref)


def test_projection_keeps_the_fp32_kernel_on_a_split_handle(H, monkeypatch):
    """CCZ_PROJECT_SPLIT=0 on a handle whose route is bf16x2: project_split.hip project_split_eligible holds otherwise at this
    shape (k <= 64, d % 16 == 0, n >= 32768, n d >= 2^26, aligned rows), so the switch decides.  ``transform_last_route()``
    records the routes of ccz_transform_wide only; what shows the fp32 kernel ran is that the output equals, bit for bit, the
    one an ``auto`` handle gives (same kernel, same operands, no atomics) and differs from the split arithmetic's.  Bound:
    tests/test_gpu_ops.py:251."""
    from cca_zoo_amd import _backend

    n, d, k = 32768 + 3, 2048, 24
    assert n * d >= 1 << 26
    rng = np.random.default_rng(n + d + k)
    X = ((rng.standard_normal((n, d)) * (1.0 + np.arange(d) / d)) + 0.3).astype(np.float32)
    mean, W = rng.standard_normal(d), rng.standard_normal((d, k))
    Xd, md, Wd = H.to_device(X), H.to_device(mean), H.to_device(W)
    ref = (X.astype(np.float64) - mean) @ W
    scale = np.abs(ref).max()

    def run(route):
        od = H.to_device(np.full((n, k), 7.0, dtype=np.float32))
        prev = H.k1_route(route)
        try:
            H.check(H.lib.ccz_transform(H.raw, _backend.F32, C.c_void_p(Xd.ptr), n, d, d, C.c_void_p(md.ptr), C.c_void_p(Wd.ptr), k,
                                        C.c_void_p(od.ptr), k))
        finally:
            H.k1_route(prev)
        out = H.to_host(od, (n, k), dtype=np.float32)
        od.free()
        return out

    auto, split = run("auto"), run("bf16x2")
    monkeypatch.setenv("CCZ_PROJECT_SPLIT", "0")
    kept = run("bf16x2")
    assert np.abs(kept - ref).max() < 2e-5 * scale * np.sqrt(d)
    assert np.array_equal(kept, auto)
    assert not np.array_equal(split, auto)                       # without the switch the split arithmetic runs at this shape


@pytest.mark.parametrize("trace", [False, True])
def test_small_read_backs_are_the_same_bytes_in_every_mode(H, monkeypatch, capfd, trace):
    """CCZ_D2H_MODE=1..4 (runtime.hip d2h: 16-byte lanes, hipMemcpyAsync + polled event, + hipStreamSynchronize, one blocking
    hipMemcpy) against mode 0, bit for bit; with CCZ_TRACE_D2H every read-back also reports to stderr.  1, 7, 513 and 4097
    doubles are odd byte counts for mode 1 (no multiple of 16: it falls back to 8-byte lanes), so 2 and 4098 doubles are read
    too, and 4098 once more from a source that is 8 but not 16 bytes aligned."""
    rng = np.random.default_rng(0)
    data = rng.standard_normal(4100)
    data[::7] = -0.0
    data[3] = np.nan
    buf = H.to_device(data)
    monkeypatch.delenv("CCZ_D2H_MODE", raising=False)
    reads = [(1, 0), (7, 0), (513, 0), (4097, 0), (2, 0), (4098, 0), (4098, 8)]
    base = [H.to_host(buf, (cnt,), offset_bytes=off).view(np.uint64) for cnt, off in reads]
    for (cnt, off), b in zip(reads, base):
        assert np.array_equal(b, data[off // 8: off // 8 + cnt].view(np.uint64))
    if trace:
        monkeypatch.setenv("CCZ_TRACE_D2H", "1")
    else:
        monkeypatch.delenv("CCZ_TRACE_D2H", raising=False)
    capfd.readouterr()
    for mode in ("1", "2", "3", "4"):
        monkeypatch.setenv("CCZ_D2H_MODE", mode)
        for (cnt, off), b in zip(reads, base):
            got = H.to_host(buf, (cnt,), offset_bytes=off).view(np.uint64)
            assert np.array_equal(got, b), (mode, cnt, off)
    err = capfd.readouterr().err
    if trace:
        for what in ("kernel", "sdma", "blocking"):
            assert "[ccz] d2h %s" % what in err, err[-1000:]
    else:
        assert "[ccz] d2h" not in err
