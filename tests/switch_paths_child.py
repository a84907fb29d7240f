"""Child program of tests/test_gpu_switch_paths.py (not collected by pytest): the kernel paths behind libccz's runtime
switches (cca_zoo_amd/csrc/env.h), each against float64 NumPy.

    python tests/switch_paths_child.py <case>

runs the probes of one case and prints ``child ok``.  The switches themselves come with the environment the parent starts
this process with (rows marked ONCE, LOAD or HANDLE in env.h are read once per process); a probe whose path depends on a
switch's value reads that value back from the environment and asserts the site's condition at its shape, so that a case
cannot fall off its path without notice.  Cases that do not need the deep objectives never import torch."""

import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

TORCH_CASES = ("loss_h2d", "handle")
if len(sys.argv) > 1 and sys.argv[1] not in TORCH_CASES:
    os.environ["CCZ_TORCHLESS"] = "1"              # ctypes only: libccz on the system's HIP runtime, a short start-up

from cca_zoo_amd import _backend  # noqa: E402
from test_gpu_cholinv import _spd_down  # noqa: E402  (the suite's structured generators, not copies of them)
from test_gpu_moments import _structured  # noqa: E402

_H = []


def handle():
    if not _H:
        _H.append(_backend.default_handle(0))
    return _H[0]


def ncu():
    n = handle().device_info()["compute_units"]
    assert n >= 8, n
    return n


def env_int(name, default):
    v = os.environ.get(name)
    return default if v is None else int(v)


def vp(buf):
    return C.c_void_p(buf.ptr)


def call(name, *args):
    H = handle()
    H.check(getattr(H.lib, name)(H.raw, *args))


# =============================================================================================
# K1
# =============================================================================================
K1_TOL = {np.float32: 2e-6, np.float64: 1e-13}          # tests/test_gpu_moments.py:68 (scaled by sqrt(G_ii G_jj))
K1_SUMS = dict(rtol=1e-12, atol=1e-9)                   # tests/test_gpu_moments.py:74
U32 = 2.0 ** -24                                        # unit roundoff of float32


def plan_rows(n, dims, dtype, lds=None):
    """gram.hip plan_rows + build_tile_table, restated: (rows per workgroup, ksplit, sliced, chunk-per-XCD order, fast,
    tiles) of a K1 launch over device views that start on 16-byte boundaries."""
    is32 = dtype == np.float32
    tile, es = (256, 4) if is32 else (128, 8)
    lds = list(lds or dims)
    fast = all(d % tile == 0 and (ld * es) % 16 == 0 for d, ld in zip(dims, lds))
    npan = sum((d + tile - 1) // tile for d in dims)
    ntiles = npan * (npan + 1) // 2
    cu, map_mode = ncu(), env_int("CCZ_GRAM_MAP", 1)
    rows_env = env_int("CCZ_GRAM_ROWS", 0)
    max_rows = rows_env if rows_env > 0 else 16384
    if fast:
        cap = min([max_rows] + [((1 << 31) - 1) // (ld * es) - 128 for ld in lds])
        if cap < 256:
            fast = False
        else:
            max_rows = cap
    gran = 32 if (is32 and fast) else 16
    kmin = max(1, -(-n // max_rows))
    kmax = max(kmin, min(n // 256, 8192))
    best, best_k = 1e300, kmin
    for ks in range(kmin, kmax + 1):
        rows = -(-(-(-n // ks)) // gran) * gran
        big = ntiles * ks >= 16 * cu
        penalty = 1.0
        if big and map_mode == 1 and ks % 8 == 0:
            rounds = -(-((ks // 8) * ntiles) // (cu // 8))
        elif big:
            rounds = -(-(((ntiles + 7) // 8) * ks) // (cu // 8))
            penalty = 1.03 if map_mode == 1 else 1.0
        else:
            rounds = -(-(ntiles * ks) // cu)
        cost = penalty * rounds * (rows + 320)
        if cost < best:
            best, best_k = cost, ks
    rows_per_wg = -(-(-(-n // best_k)) // gran) * gran
    ksplit = -(-n // rows_per_wg)
    sliced = ntiles * ksplit >= 16 * cu
    xchunks = sliced and map_mode == 1 and ksplit % 8 == 0
    return dict(rows=rows_per_wg, ksplit=ksplit, sliced=sliced, xchunks=xchunks, fast=fast, ntiles=ntiles)


def gram_ref(views):
    X = np.hstack([v.astype(np.float64) for v in views])
    return X.T @ X, X.sum(axis=0)


def k1(descr, n, dtype, D, pilot=None, mom=None, accumulate=False, on_device=True):
    """One ccz_moments call -> (symmetrised G, column sums, the moments buffer)."""
    H = handle()
    mom = mom if mom is not None else H.alloc((D * D + D) * 8)
    H.moments(descr, n, _backend.F32 if dtype == np.float32 else _backend.F64, on_device, mom.ptr, accumulate=accumulate, pilot=pilot)
    upper = H.to_host(mom, (D * D + D,))
    sym = H.to_device(upper)
    H.moments_symmetrize(sym.ptr, D)
    flat = H.to_host(sym, (D * D + D,))
    sym.free()
    return flat[: D * D].reshape(D, D), flat[D * D:], mom


def k1_check(G, s, Gr, sr, dtype, what):
    scale = np.sqrt(np.outer(np.diag(Gr), np.diag(Gr)))
    err = float(np.max(np.abs(G - Gr) / scale))
    print("k1 %s: scaled error %.3e" % (what, err), flush=True)
    assert err < K1_TOL[dtype], (what, err)
    np.testing.assert_allclose(s, sr, **K1_SUMS)
    assert np.array_equal(G, G.T), what


def on_device(views):
    bufs = [handle().to_device(v) for v in views]
    return bufs, [(b.ptr, v.shape[1], v.shape[1]) for b, v in zip(bufs, views)]


def k1_device_shapes():
    """The device shapes of test_moments_host_views in both dtypes: aligned + row tail inside a k-block, several tiles and
    row chunks, fewer rows than a k-block multiple with a ragged panel, three ragged views."""
    for dtype in (np.float32, np.float64):
        for n, dims in ((777, [256, 256]), (4100, [512, 256]), (33, [300, 7]), (1000, [40, 30, 20])):
            views = [_structured(n, d, dtype, 10 * i + d) for i, d in enumerate(dims)]
            bufs, descr = on_device(views)
            G, s, _ = k1(descr, n, dtype, sum(dims), pilot=False if dtype == np.float32 else None)
            assert handle().moments_last_route()[0] == ("fp32" if dtype == np.float32 else "fp64")
            k1_check(G, s, *gram_ref(views), dtype, "%s %d x %s" % (dtype.__name__, n, dims))


def shifted_views(n, dims, ratio, seed):
    """_structured rows moved so that every column's |mean| / std is `ratio` (signs alternate by column)."""
    out = []
    for i, d in enumerate(dims):
        v = _structured(n, d, np.float64, seed + i)
        sign = np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
        v = v - v.mean(axis=0) + ratio * v.std(axis=0) * sign
        out.append(v.astype(np.float32))
    return out


def unshifted_bound_holds(views, plan):
    """Why the bound of the UNSHIFTED fp32 kernel (2e-6 of sqrt(G_ii G_jj)) holds on shifted rows at this shape: a workgroup
    adds the products of `plan[rows]` rows in float32 and flushes in float64, so an entry's error is that of float32 sums of
    at most m = plan[rows] terms each, |error| <= sqrt(m) u sum |x_i x_j| (the probabilistic bound of a float32 sum of m terms,
    constant 1; the worst case has m in place of sqrt(m)), and sum |x_i x_j| <= sqrt(G_ii G_jj) by Cauchy-Schwarz -- whatever
    the shift.  Evaluated in float64 on the data: sqrt(m) u max_ij sum |x_i x_j| / sqrt(G_ii G_jj) must stay below 2e-6."""
    X = np.abs(np.hstack([v.astype(np.float64) for v in views]))
    A = X.T @ X
    d = np.sqrt(np.diag(A))
    worst = float(np.sqrt(plan["rows"]) * U32 * np.max(A / np.outer(d, d)))
    assert worst < K1_TOL[np.float32], (plan, worst)
    return worst


def k1_shifted(pilots=(True, False)):
    """mean / std = 5 in every column, 1000 x [256, 256] (3 tiles; 3 row chunks of 352 rows on 256 CUs): with the pilot
    the staged kernel with the subtraction at the load + k_pilot_fixup; without it the unshifted kernel on the raw rows."""
    H = handle()
    n, dims = 1000, [256, 256]
    views = shifted_views(n, dims, 5.0, 40)
    plan = plan_rows(n, dims, np.float32)
    unshifted_bound_holds(views, plan)
    Gr, sr = gram_ref(views)
    bufs, descr = on_device(views)
    for pilot in pilots:
        G, s, _ = k1(descr, n, np.float32, 512, pilot=pilot)
        assert H.moments_last_pilot() is pilot
        k1_check(G, s, Gr, sr, np.float32, "shifted rows, pilot=%s" % pilot)


def k1_accumulate():
    """Two row shards accumulated into moments that already hold the first (device views, both dtypes)."""
    for dtype in (np.float32, np.float64):
        v = [_structured(2000, 256, dtype, 3), _structured(2000, 256, dtype, 4)]
        a, b = [np.ascontiguousarray(x[:900]) for x in v], [np.ascontiguousarray(x[900:]) for x in v]
        ba, da = on_device(a)
        bb, db = on_device(b)
        pilot = False if dtype == np.float32 else None
        _, _, mom = k1(da, 900, dtype, 512, pilot=pilot)
        G, s, _ = k1(db, 1100, dtype, 512, pilot=pilot, mom=mom, accumulate=True)
        k1_check(G, s, *gram_ref(v), dtype, "%s accumulated shards" % dtype.__name__)


_SLICED = {}


def sliced_inputs(dtype):
    """The smallest chip-filling K1 grids under CCZ_GRAM_ROWS=256 (the rows with their float64 Gram, formed once per process):
    fp32 16384 (+ 37) x [1536, 1536] = 78 tiles x 64 (65) chunks, fp64 8192 (+ 37) x [1024, 1024] = 136 tiles x 32 (33)."""
    if dtype not in _SLICED:
        n, dims = (16384, [1536, 1536]) if dtype == np.float32 else (8192, [1024, 1024])
        views = [_structured(n + 37, d, dtype, 70 + i) for i, d in enumerate(dims)]
        X = np.hstack([v.astype(np.float64) for v in views])
        G0 = X[:n].T @ X[:n]
        G1 = G0 + X[n:].T @ X[n:]
        bufs, descr = on_device(views)
        _SLICED[dtype] = dict(n=n, dims=dims, descr=descr, bufs=bufs, ref={n: (G0, X[:n].sum(axis=0)), n + 37: (G1, X.sum(axis=0))})
    return _SLICED[dtype]


def k1_sliced(dtype, pilot=None, want_xchunks=None):
    """Both row counts of sliced_inputs: ksplit a multiple of 8 (the chunk-per-XCD order under CCZ_GRAM_MAP=1) and, with the 37
    extra rows, one more and SHORT last chunk (per-XCD slices of the tile list in either map mode)."""
    assert env_int("CCZ_GRAM_ROWS", 0) == 256
    w = sliced_inputs(dtype)
    for n in (w["n"], w["n"] + 37):
        plan = plan_rows(n, w["dims"], dtype)
        # gram.hip plan_rows: sliced = ntiles * ksplit >= 16 * ncu
        assert plan["fast"] and plan["sliced"] and plan["rows"] == 256 and plan["ksplit"] == -(-n // 256), plan
        assert plan["ntiles"] == (78 if dtype == np.float32 else 136)
        if want_xchunks is not None:
            assert plan["xchunks"] == (want_xchunks and n == w["n"]), plan      # the ragged count has ksplit % 8 == 1
        G, s, _ = k1(w["descr"], n, dtype, sum(w["dims"]), pilot=pilot)
        if dtype == np.float32 and pilot is not None:
            assert handle().moments_last_pilot() is bool(pilot)
        k1_check(G, s, *w["ref"][n], dtype, "%s sliced n=%d xchunks=%s" % (dtype.__name__, n, plan["xchunks"]))


def case_k1_staged():
    assert env_int("CCZ_GRAM_IMPL", 1) == 0 and env_int("CCZ_GRAM64_IMPL", 1) == 0
    # (4100, [512, 256]) fp32: 6 tiles, 15 row chunks, not sliced -> per-chunk partial tiles + k_gram_reduce; fp64: k_gram_f64
    p = plan_rows(4100, [512, 256], np.float32)
    assert p["fast"] and not p["sliced"] and p["ksplit"] >= 2, p
    k1_device_shapes()
    k1_shifted()
    k1_accumulate()


def case_k1_supertile():
    assert env_int("CCZ_GRAM_MAP", 1) == 0
    k1_sliced(np.float32, pilot=False, want_xchunks=False)
    k1_sliced(np.float64, want_xchunks=False)
    k1_device_shapes()                               # small grids read the same (re-dealt) tile list in the plain order


def case_k1_rows():
    assert env_int("CCZ_GRAM_MAP", 1) == 1
    k1_sliced(np.float32, pilot=False, want_xchunks=True)
    k1_sliced(np.float64, want_xchunks=True)
    k1_sliced(np.float32, pilot=True)                # the pilot-shifted FIFO kernel on whole ring periods + the staged rest


def case_k1_fifo_pilot():
    assert env_int("CCZ_GRAM_FIFO_PILOT", 1) == 0 and env_int("CCZ_GRAM_PILOT", -1) == 1 and env_int("CCZ_GRAM64_IMPL", 1) == 0
    assert env_int("CCZ_GRAM_PARTIAL_MB", 192) == 0
    H = handle()
    k1_sliced(np.float32)                            # sliced + pilot: k_gram_f32<true> with the pilot on a sliced grid
    assert H.moments_last_pilot() is True
    k1_sliced(np.float64)                            # k_gram_f64 on a sliced grid
    # small grids with several row chunks and a pilot: gram.hip launch_gram_f32 takes per-chunk partial tiles when
    # ksplit >= 2 && !sliced && bytes <= cap; the cap is 0 here -> the staged kernel's atomic flush
    for n, dims in ((1000, [256, 256]), (1000, [40, 30, 20])):
        plan = plan_rows(n, dims, np.float32)
        assert plan["ksplit"] >= 2 and not plan["sliced"], plan
        views = [_structured(n, d, np.float32, 10 * i + d) for i, d in enumerate(dims)]
        bufs, descr = on_device(views)
        G, s, _ = k1(descr, n, np.float32, sum(dims))
        assert H.moments_last_pilot() is True
        k1_check(G, s, *gram_ref(views), np.float32, "atomic flush %d x %s" % (n, dims))


def case_k1_pilot_never():
    """CCZ_GRAM_PILOT=0 overrides the caller's mode: rows at mean / std = 5 run unshifted even when the caller asks for the pilot."""
    assert env_int("CCZ_GRAM_PILOT", -1) == 0
    H = handle()
    n, dims = 1000, [256, 256]
    views = shifted_views(n, dims, 5.0, 40)
    unshifted_bound_holds(views, plan_rows(n, dims, np.float32))
    Gr, sr = gram_ref(views)
    bufs, descr = on_device(views)
    for pilot in (None, True):
        G, s, _ = k1(descr, n, np.float32, 512, pilot=pilot)
        assert H.moments_last_pilot() is False
        k1_check(G, s, Gr, sr, np.float32, "CCZ_GRAM_PILOT=0, caller's pilot=%s" % pilot)


def case_k1_pilot_ratio():
    """CCZ_GRAM_PILOT_RATIO=0.1: automatic mode shifts rows whose largest |mean| / std is 0.25 (the default threshold is 2)."""
    assert float(os.environ["CCZ_GRAM_PILOT_RATIO"]) == 0.1
    H = handle()
    n, dims = 4100, [512, 256]
    views = [_structured(n, d, np.float32, 10 * i + d) for i, d in enumerate(dims)]
    X = np.hstack(views).astype(np.float64)
    ratio = float(np.max(np.abs(X.mean(axis=0)) / X.std(axis=0)))
    assert 0.1 < ratio < 2.0, ratio
    bufs, descr = on_device(views)
    G, s, _ = k1(descr, n, np.float32, sum(dims))
    assert H.moments_last_pilot() is True
    k1_check(G, s, *gram_ref(views), np.float32, "automatic pilot at ratio %.2f" % ratio)
    centred = [(v - v.mean(axis=0, dtype=np.float64)).astype(np.float32) for v in views]
    bufs, descr = on_device(centred)
    G, s, _ = k1(descr, n, np.float32, sum(dims))
    assert H.moments_last_pilot() is False           # |mean| / std ~ 1e-8: still unshifted
    Gr, sr = gram_ref(centred)
    scale = np.sqrt(np.outer(np.diag(Gr), np.diag(Gr)))
    assert np.max(np.abs(G - Gr) / scale) < K1_TOL[np.float32]
    np.testing.assert_allclose(s, sr, rtol=1e-12, atol=1e-7)          # (sums of centred columns cancel to ~1e-4: an absolute bound)


# =============================================================================================
# fp64 GEMM (gemm64_big.hip, gemm64_skinny.hip) and the wide fp32 product (gemm_big.hip)
# =============================================================================================
def gemm_check(tA, tB, M, N, K, beta, seed):
    """tests/test_gpu_ops.py:37, :55, :71: rtol 1e-12, atol 1e-12 K."""
    H = handle()
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((K, M) if tA else (M, K)) * (1.0 + np.arange(M if tA else K) / 7.0 % 1.0)
    B = rng.standard_normal((N, K) if tB else (K, N)) + 0.25
    Cm = rng.standard_normal((M, N))
    ref = 0.7 * (A.T if tA else A) @ (B.T if tB else B) + beta * Cm
    Ad, Bd, Cd = H.to_device(A), H.to_device(B), H.to_device(Cm)
    call("ccz_gemm_f64", tA, tB, M, N, K, 0.7, vp(Ad), A.shape[1], vp(Bd), B.shape[1], beta, vp(Cd), N)
    np.testing.assert_allclose(H.to_host(Cd, (M, N)), ref, rtol=1e-12, atol=1e-12 * K)
    for b in (Ad, Bd, Cd):
        b.free()


def gemm_strided():
    """A, B and C inside wider matrices at (even) offsets, as in test_gemm_strided_views, at a size both fp64 kernels can take:
    what lies around C must stay untouched."""
    H = handle()
    rng = np.random.default_rng(0)
    M, N, K = 300, 140, 64
    bigA, bigB = rng.standard_normal((M + 5, K + 10)), rng.standard_normal((K + 3, N + 6)) + 0.5
    out0 = rng.standard_normal((M + 2, N + 8))
    A, B = bigA[2:2 + M, 4:4 + K], bigB[1:1 + K, 2:2 + N]
    Ad, Bd, Cd = H.to_device(bigA), H.to_device(bigB), H.to_device(out0)
    call("ccz_gemm_f64", 0, 0, M, N, K, 1.0, C.c_void_p(Ad.ptr + (2 * (K + 10) + 4) * 8), K + 10, C.c_void_p(Bd.ptr + ((N + 6) + 2) * 8),
         N + 6, 0.0, C.c_void_p(Cd.ptr + ((N + 8) + 4) * 8), N + 8)
    got = H.to_host(Cd, out0.shape)
    np.testing.assert_allclose(got[1:1 + M, 4:4 + N], A @ B, rtol=1e-12, atol=1e-12 * K)
    keep = np.ones(out0.shape, dtype=bool)
    keep[1:1 + M, 4:4 + N] = False
    assert np.array_equal(got[keep], out0[keep])


GEMM_SHAPES = ((257, 130, 304), (1111, 999, 48), (2048, 160, 2048), (1100, 78, 1024))


def gemm_all(extra=()):
    for M, N, K in GEMM_SHAPES + tuple(extra):
        for tA in (0, 1):
            for tB in (0, 1):
                for beta in (0.0, -1.3):
                    gemm_check(tA, tB, M, N, K, beta, M + 3 * N + 7 * K + 2 * tA + tB)
    gemm_strided()


def case_pilot_never_gemm_big():
    """CCZ_GRAM_PILOT=0 (K1) with CCZ_GEMM_BIG_MIN_TILES=1 and CCZ_GEMM_BIG_MIN_K=16 (fp64 GEMM)."""
    case_k1_pilot_never()
    assert env_int("CCZ_GEMM_BIG_MIN_TILES", 32) == 1 and env_int("CCZ_GEMM_BIG_MIN_K", 64) == 16
    # gemm64_big.hip gemm_f64_big_eligible: K % 16 == 0, K >= min_k, M >= 128, N >= 128, tiles >= min_tiles, EVEN leading
    # dimensions.  Of the four shapes (257, 130, 304) = 3 x 2 tiles qualifies here and not by default -- with A as stored only:
    # A' has the odd leading dimension 257 -- and (1111, 999, 48) never does (ldc = 999); both stay as what such shapes run.  Their
    # even neighbours are added: (258, 130, 304) = 6 tiles < 32 needs BIG_MIN_TILES, (1112, 1000, 48) = 72 tiles with
    # K = 48 < 64 needs BIG_MIN_K, (130, 4098, 16) is a single k-block.  All are grids smaller than the chip: half-height tiles.
    assert 9 * 8 < ncu()
    gemm_all(extra=((258, 130, 304), (1112, 1000, 48), (130, 4098, 16)))


def case_pilot_ratio_gemm_alt():
    """CCZ_GRAM_PILOT_RATIO=0.1 (K1) with CCZ_GEMM_HALF_TILE=0, CCZ_GEMM_SKINNY_OFF=1 (fp64 GEMM) and CCZ_GEMM_NN_IMPL=0 (fp32)."""
    case_k1_pilot_ratio()
    assert env_int("CCZ_GEMM_HALF_TILE", 1) == 0 and os.environ.get("CCZ_GEMM_SKINNY_OFF", "").startswith("1")
    # gemm64_big.hip gemm_f64_big: half-height tiles when tm * tn < ncu and M > 64 -- (1400, 1290, 144) is 11 x 11 = 121 tiles
    # (>= the default 32, K >= 64): full-height tiles on a grid smaller than the chip
    assert 32 <= 11 * 11 < ncu()
    # gemm64_skinny.hip gemm_f64_skinny_eligible (tB == 0, 48 < N <= 192 even, M, K >= 1024, K % 16 == 0) holds for
    # (2048, 160, 2048) and (1100, 78, 1024): the first then takes the big kernel (16 x 2 = 32 tiles), the second the 64 x 64 one
    gemm_all(extra=((1400, 1290, 144),))
    wide_fp32_product_staged()


def wide_fp32_product_staged():
    """The `impl == "0"` case of test_gpu_ops.py::test_transform_f32_wide_output_kernels (CCZ_GEMM_NN_IMPL is read once per
    process): (X - mean) W at 65536 x 256 x 256 = 256 output tiles on the register-staged 256 x 256 tile kernel."""
    assert env_int("CCZ_GEMM_NN_IMPL", 1) == 0
    H = handle()
    n, d, k = 65536, 256, 256
    rng = np.random.default_rng(n + d + k)
    Xp = (rng.standard_normal((n, d)) + 0.3).astype(np.float32)
    mean = rng.standard_normal(d)
    W = rng.standard_normal((d, k))
    Xd, md, Wd = H.to_device(Xp), H.to_device(mean), H.to_device(W)
    od = H.alloc(n * k * 4)
    call("ccz_transform", _backend.F32, vp(Xd), n, d, d, vp(md), vp(Wd), k, vp(od), k)
    got = H.to_host(od, (n, k), dtype=np.float32)
    rows = np.r_[0:300, n // 2:n // 2 + 300, n - 300:n]               # first / middle / last tile
    ref = (Xp[rows].astype(np.float64) - mean) @ W
    scale = np.abs(ref).max()
    assert np.abs(got[rows] - ref).max() < 2e-5 * scale * np.sqrt(d)   # tests/test_gpu_ops.py:302
    assert np.isfinite(got).all()


# =============================================================================================
# Cholesky, triangular solves, eigensolvers
# =============================================================================================
def potrf_trsm(d):
    """tests/test_gpu_ops.py:98, :106."""
    H = handle()
    rng = np.random.default_rng(d)
    S = _spd_down(rng, d, 1e3)                       # spectrum 1 .. 1e-3: the absolute bounds below are for ||S|| ~ 1
    Sd = H.to_device(S)
    call("ccz_potrf_lower", vp(Sd), d, d)
    L = np.tril(H.to_host(Sd, (d, d)))
    np.testing.assert_allclose(L @ L.T, S, rtol=1e-11, atol=1e-11)
    Lr = np.linalg.cholesky(S)
    R = rng.standard_normal((37, d)) + 0.5
    Ld = H.to_device(Lr)
    for trans in (1, 0):
        Rd = H.to_device(R)
        call("ccz_trsm_right_lower", trans, 37, d, vp(Ld), d, vp(Rd), d)
        got = H.to_host(Rd, (37, d))
        ref = np.linalg.solve(Lr, R.T).T if trans else np.linalg.solve(Lr.T, R.T).T
        np.testing.assert_allclose(got, ref, rtol=1e-8, atol=1e-9)


def cholinv_mixed():
    """tests/test_gpu_cholinv.py:69-70 on the mixed batch."""
    H = handle()
    rng = np.random.default_rng(7)
    mats = [_spd_down(rng, d, 1e4) for d in (512, 70, 1, 333, 64, 129)]
    bufs = [(H.to_device(A), H.to_device(np.full(A.shape, np.nan)), H.to_device(np.zeros(A.shape))) for A in mats]
    n = len(mats)
    arr = lambda i: (C.c_void_p * n)(*[b[i].ptr for b in bufs])          # noqa: E731
    call("ccz_cholinv", n, arr(0), (C.c_int64 * n)(*[A.shape[0] for A in mats]), arr(1), arr(2))
    for (a, l, x), A in zip(bufs, mats):
        Lr = np.linalg.cholesky(A)
        L, X = H.to_host(l, A.shape), H.to_host(x, A.shape)
        assert np.abs(np.tril(L) - Lr).max() < 1e-10 * np.abs(Lr).max()
        assert np.abs(np.tril(X) @ Lr - np.eye(A.shape[0])).max() < 1e-8


def rcca_from_moments():
    """rCCA from float64 moments with BOTH views wider than 1024 columns: potrf.hip potrf_dispatch factors them on
    super-blocks with kept inverses, so the first whitening solve rides along the factorization of view 2's factor
    (potrf_lower_batched_aux_rider; solve.cpp: rider.matrix = 1) and the back-projection of the k directions is the batched
    few-row solve (trsm_right_lower_aux_multi: every d > 1024, 1 <= r <= 256).  At (600, 520) neither site is reached.
    Reference: the oracle's float64 restatement on the same rows; bound: tests/test_gpu_handle_lifecycle.py:27."""
    from conftest import col_rel_err
    from oracle import reference_form as rf

    H = handle()
    n, dims, k = 6000, (1100, 1040), 8
    assert min(dims) > 1024
    rng = np.random.default_rng(11)
    zz = rng.standard_normal((n, k)) * np.linspace(12.0, 5.0, k)     # planted correlations 0.98 .. 0.92, above the noise's
    sv = [zz @ np.linalg.qr(rng.standard_normal((d, k)))[0].T + rng.standard_normal((n, d)) * (1.0 + np.arange(d) / d) + 0.25 for d in dims]
    G, s = gram_ref(sv)
    mom = H.to_device(np.concatenate([G.ravel(), s]))
    W, _, vals = H.rcca_solve(mom.ptr, n, list(dims), [0.1, 0.1], True, k)
    assert vals.shape == (k,)
    W_ref = rf.rcca_weights(sv, k, c=0.1)[0]
    for a, r in zip(W, W_ref):
        e = col_rel_err(a, r)
        print("rcca from moments: column error %.3e" % e, flush=True)
        assert e < 1e-8


def cholesky_probes():
    for d in (513, 1100, 1600):                      # step kernels; 1100, 1600 > 1024: super-blocks of CCZ_POTRF_SB columns
        potrf_trsm(d)
    cholinv_mixed()
    rcca_from_moments()


def syevj(d):
    """tests/test_gpu_ops.py:130-133."""
    H = handle()
    rng = np.random.default_rng(d)
    if d == 12:                                      # +/- eigenvalue pairs
        T = rng.standard_normal((7, 5))
        A = np.block([[np.zeros((7, 7)), T], [T.T, np.zeros((5, 5))]])
    else:
        A = rng.standard_normal((d, d)) * (1.0 + np.arange(d) / d)
        A = A + A.T
    Ad, wd, Vd = H.to_device(A), H.alloc(d * 8), H.alloc(d * d * 8)
    sw = C.c_int(0)
    call("ccz_syevj", vp(Ad), d, vp(wd), vp(Vd), C.byref(sw))
    w, V = H.to_host(wd, (d,)), H.to_host(Vd, (d, d))
    scale = max(1, np.abs(A).sum(1).max())
    np.testing.assert_allclose(w, np.linalg.eigvalsh(A)[::-1], atol=1e-11 * scale)
    np.testing.assert_allclose(V @ V.T, np.eye(d), atol=1e-12)
    np.testing.assert_allclose(V @ A @ V.T, np.diag(w), atol=1e-10 * scale)
    assert 1 <= sw.value <= 40


def gesvj(p, q):
    """tests/test_gpu_ops.py:145-146."""
    H = handle()
    rng = np.random.default_rng(p + q)
    A = rng.standard_normal((p, q)) * (1.0 + np.arange(q) / q)
    r = min(p, q)
    Ad, Ud, sd, Vd = H.to_device(A), H.alloc(p * r * 8), H.alloc(r * 8), H.alloc(r * q * 8)
    call("ccz_gesvj", vp(Ad), p, q, vp(Ud), vp(sd), vp(Vd), None)
    U, s, Vt = H.to_host(Ud, (p, r)), H.to_host(sd, (r,)), H.to_host(Vd, (r, q))
    np.testing.assert_allclose(s, np.linalg.svd(A, compute_uv=False), atol=1e-11)
    np.testing.assert_allclose(U * s @ Vt, A, atol=1e-11)


def gevp_topk(p, k):
    """tests/test_gpu_ops.py:161-172."""
    import scipy.linalg

    H = handle()
    rng = np.random.default_rng(2)
    lam = np.concatenate([np.linspace(5.0, 2.0, k), rng.uniform(-3.0, 1.0, p - k)])
    Qm, _ = np.linalg.qr(rng.standard_normal((p, p)))
    A = (Qm * lam) @ Qm.T
    A = 0.5 * (A + A.T)
    Ad, wd, Vd = H.to_device(A), H.alloc(k * 8), H.alloc(p * k * 8)
    call("ccz_gevp_topk", vp(Ad), None, p, k, vp(wd), vp(Vd))
    w, V = H.to_host(wd, (k,)), H.to_host(Vd, (p, k))
    np.testing.assert_allclose(w, np.sort(lam)[::-1][:k], atol=1e-9)
    assert np.linalg.norm(A @ V - V * w) < 1e-8 * np.linalg.norm(A)
    Bm = rng.standard_normal((p, p))
    Bm = Bm @ Bm.T / p + np.eye(p)
    wr, Vr = scipy.linalg.eigh(A, Bm, subset_by_index=[p - k, p - 1])
    Bd = H.to_device(Bm)
    call("ccz_gevp_topk", vp(Ad), vp(Bd), p, k, vp(wd), vp(Vd))
    w, V = H.to_host(wd, (k,)), H.to_host(Vd, (p, k))
    np.testing.assert_allclose(w, wr[::-1], atol=1e-9)
    np.testing.assert_allclose(np.diag(V.T @ Bm @ V), 1.0, atol=1e-9)
    S = np.sign(np.sum(V * Vr[:, ::-1], axis=0))
    assert np.linalg.norm(V * S - Vr[:, ::-1]) < 1e-6 * np.linalg.norm(Vr)


def svd_topk(p, q, k):
    """tests/test_gpu_ops.py:186-188."""
    H = handle()
    rng = np.random.default_rng(3)
    r = min(p, q)
    sv = np.concatenate([np.linspace(3.0, 1.5, k), rng.uniform(0.0, 1.0, r - k)])
    U0, _ = np.linalg.qr(rng.standard_normal((p, r)))
    V0, _ = np.linalg.qr(rng.standard_normal((q, r)))
    T = (U0 * sv) @ V0.T
    Td, Ud, sd, Vd = H.to_device(T), H.alloc(p * k * 8), H.alloc(k * 8), H.alloc(q * k * 8)
    call("ccz_svd_topk", vp(Td), p, q, k, vp(Ud), vp(sd), vp(Vd))
    U, s, V = H.to_host(Ud, (p, k)), H.to_host(sd, (k,)), H.to_host(Vd, (q, k))
    np.testing.assert_allclose(s, np.sort(sv)[::-1][:k], atol=1e-9)
    np.testing.assert_allclose(T @ V, U * s, atol=1e-8)
    np.testing.assert_allclose(U.T @ U, np.eye(k), atol=1e-9)


def eigen_probes():
    for d in (2, 3, 12, 65, 96, 97, 160, 161):       # syev_small.hip syev_small_max: 160 (mode 2), 96 (mode 1), 0 (else): the
        syevj(d)                                     # sizes either side of each; wider ones take evd_block.hip syev_block
    gevp_topk(60, 5)                                 # p <= 192: the direct route (one small / block EVD)
    for d in (200, 513):                             # evd_block.hip syev_block (two-sided), padded to 256 / 576
        syevj(d)
    gesvj(200, 513)                                  # syev_small.hip jacobi_rows: 200 x (513 + 200) doubles > 144 KiB -> jacobi_rows_block
    gevp_topk(300, 12)                               # solve.cpp topk_symmetric: p > 192, 3 k < p -> filter cycles + Rayleigh-Ritz
    svd_topk(250, 320, 10)


def case_chol_eig_a():
    assert env_int("CCZ_POTRF_SB", 512) == 256 and env_int("CCZ_SYEV_TWOSIDED", 2) == 1
    cholesky_probes()
    eigen_probes()


def case_chol_eig_b():
    assert env_int("CCZ_POTRF_SB", 512) == 1024 and env_int("CCZ_SYEV_TWOSIDED", 2) == 0
    cholesky_probes()
    eigen_probes()


def k1_env_route():
    """CCZ_K1_ROUTE=bf16x2 on a handle left at ``auto``: ccz_moments takes the split route far below the size from which auto
    mode would (gram_split.hip gram_split_worthwhile: 1e11 flop; here 4e9).  Bound: tests/test_gpu_k1_split.py:90-91."""
    assert os.environ.get("CCZ_K1_ROUTE") == "bf16x2"
    H = handle()
    assert H.k1_route(None) == "auto"
    n, dims = 8192, [512, 512]
    assert 2.0 * n * sum(dims) ** 2 < 1e11
    views = [_structured(n, d, np.float32, 90 + i) for i, d in enumerate(dims)]
    bufs, descr = on_device(views)
    mom = H.alloc((1024 * 1024 + 1024) * 8)
    H.moments(descr, n, _backend.F32, True, mom.ptr)
    assert H.moments_last_route()[0] == "bf16x2"
    flat = H.to_host(mom, (1024 * 1024 + 1024,))
    Gr, sr = gram_ref(views)
    iu = np.triu_indices(1024)
    scale = np.sqrt(np.outer(np.diag(Gr), np.diag(Gr)))
    assert float((np.abs(flat[: 1024 * 1024].reshape(1024, 1024) - Gr) / scale)[iu].max()) < 2e-6
    np.testing.assert_allclose(flat[1024 * 1024:], sr, rtol=1e-12, atol=1e-7)


def case_chase_margin_route():
    assert env_int("CCZ_SYEV_CHASE", 1) == 0
    eigen_probes()
    k1_env_route()


# =============================================================================================
# handle: graphs, host waits, traces; the loss's K1; pinned host views
# =============================================================================================
def estimators_small():
    """rCCA and MCCA on the separated two-view fixture against the oracle's weights, as
    tests/test_gpu_estimators.py:108-109 (bound :14), and a CCALoss forward / backward (loss_probe)."""
    from conftest import col_rel_err, load_golden
    from cca_zoo_amd.linear import MCCA, rCCA

    g = load_golden("separated_two_view_f64")
    train = [g["train0"], g["train1"]]
    for model, tag in ((rCCA(latent_dimensions=6, c=0.2), "rcca_k6_c0.2"), (MCCA(latent_dimensions=6, c=0.05), "mcca_k6_c0.05")):
        model.fit(train)
        for i, w in enumerate(model.weights_):
            assert col_rel_err(w, g["%s/w%d" % (tag, i)]) < 1e-5, (tag, i)
    loss_probe(((1504, 100, 37),))


def loss_probe(shapes):
    """tests/test_gpu_round5.py:53-62."""
    import torch

    from cca_zoo_amd.deep.objectives import CCALoss
    from oracle import losses as ol

    g = torch.Generator().manual_seed(11)
    for n_, d1, d2 in shapes:
        z1 = torch.randn(n_, d1, generator=g, dtype=torch.float64)
        z2 = 0.7 * z1 @ (torch.randn(d1, d2, generator=g, dtype=torch.float64) / d1 ** 0.5) + torch.randn(n_, d2, generator=g, dtype=torch.float64) + 0.5
        a = z1.float().cuda().requires_grad_(True)
        b = z2.float().cuda().requires_grad_(True)
        loss = CCALoss(eps=1e-5)([a, b])
        (2.5 * loss).backward()
        want, g1, g2 = ol.cca_loss_closed_form(a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy(), 1e-5)
        assert abs(loss.item() - want) <= 1e-3 * abs(want), (loss.item(), want)
        e1 = np.linalg.norm(a.grad.cpu().numpy() - 2.5 * g1) / np.linalg.norm(2.5 * g1)
        e2 = np.linalg.norm(b.grad.cpu().numpy() - 2.5 * g2) / np.linalg.norm(2.5 * g2)
        assert e1 < 1e-2 and e2 < 1e-2, (e1, e2)
        assert handle().loss_last_route()[0] == "fp32"


def pinned_host_views():
    """CCZ_H2D_PINNED_DIRECT=0: 64 MiB of PINNED float32 rows (one view inside a wider pinned matrix) in 16 MiB chunks, packed
    through the bounce buffers like pageable ones.  gram.hip moments_impl: piped needs n * row_bytes >= 64 MiB; 32779 rows of
    2048 bytes in chunks of 8192 rows (tapering) are five or more chunks.  Bound: tests/test_gpu_moments.py:100-101."""
    import torch

    assert env_int("CCZ_H2D_PINNED_DIRECT", 1) == 0 and env_int("CCZ_H2D_CHUNK_MB", 1024) == 16
    H = handle()
    n = 32768 + 11
    wide = torch.empty((n, 300), dtype=torch.float32).pin_memory()
    other = torch.empty((n, 256), dtype=torch.float32).pin_memory()
    wide.numpy()[:, 10:266] = _structured(n, 256, np.float32, 5)
    other.numpy()[:] = _structured(n, 256, np.float32, 6)
    a, b = wide.numpy()[:, 10:266], other.numpy()
    assert wide.is_pinned() and other.is_pinned() and n * 2048 >= 64 << 20
    mom = H.alloc((512 * 512 + 512) * 8)
    H.moments([(a, 256, 300), (b, 256, 256)], n, _backend.F32, False, mom.ptr)
    H.moments_symmetrize(mom.ptr, 512)
    flat = H.to_host(mom, (512 * 512 + 512,))
    Gr, sr = gram_ref([a, b])
    scale = np.sqrt(np.outer(np.diag(Gr), np.diag(Gr)))
    assert np.max(np.abs(flat[: 512 * 512].reshape(512, 512) - Gr) / scale) < 2e-6
    np.testing.assert_allclose(flat[512 * 512:], sr, rtol=1e-12, atol=1e-8)


def case_loss_h2d():
    assert env_int("CCZ_LOSS_K1_FIFO", 1) == 0
    # gram.hip gram_partials_f32: the FIFO form needs fast views, n % 32 == 0 and <= 64 tiles -- 4096 x (512, 512) has all three
    # (10 tiles), so the switch decides there; 1504 x (100, 37) has ragged widths and takes k_gram_f32<false> either way
    loss_probe(((4096, 512, 512), (1504, 100, 37)))
    pinned_host_views()


def case_handle():
    assert env_int("CCZ_GRAPHS", 1) == 0 and float(os.environ["CCZ_SPIN_WAIT_MS"]) == 0.0
    estimators_small()
    eigen_probes()                                   # the block Jacobi's sweeps are the graphs that are now issued directly


def case_traces():
    """Every trace switch at once: the same probes, the same bounds (a trace never changes results); the parent checks stderr."""
    for name in ("CCZ_TRACE_PHASES", "CCZ_TRACE_SOLVER", "CCZ_TRACE_POOL", "CCZ_TRACE_D2H", "CCZ_CHAIN_DEBUG", "CCZ_BJ_DEBUG"):
        assert os.environ.get(name), name
    cholesky_probes()
    eigen_probes()


CASES = {
    "k1_staged": case_k1_staged,
    "k1_supertile": case_k1_supertile,
    "k1_rows": case_k1_rows,
    "k1_fifo_pilot": case_k1_fifo_pilot,
    "pilot_never_gemm_big": case_pilot_never_gemm_big,
    "pilot_ratio_gemm_alt": case_pilot_ratio_gemm_alt,
    "chol_eig_a": case_chol_eig_a,
    "chol_eig_b": case_chol_eig_b,
    "chase_margin_route": case_chase_margin_route,
    "loss_h2d": case_loss_h2d,
    "handle": case_handle,
    "traces": case_traces,
}


if __name__ == "__main__":
    CASES[sys.argv[1]]()
    handle().sync()
    print("child ok", flush=True)
