"""csrc/half_cvt.h on the host: the bfloat16 / float16 conversions of the deep objectives' 2-byte formats, compiled by g++ and
compared BIT FOR BIT with torch's CPU conversions -- widening over all 65536 bit patterns of each type, narrowing over every
half value, its float32 neighbours, every tie between adjacent half values, the overflow threshold, fp16's subnormal range and
the special values."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = {"bf16": (0, torch.bfloat16), "f16": (1, torch.float16)}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("half_cvt") / "libhalf_cvt_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(HERE, "half_cvt_host.cpp")])
    lib = ctypes.CDLL(so)
    lib.half_widen.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.half_narrow.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.half_widen.restype = lib.half_narrow.restype = None
    return lib


def _all_halves(dtype):
    """every bit pattern of the type as a torch tensor, and the patterns"""
    bits = np.arange(65536, dtype=np.uint16)
    return torch.from_numpy(bits.view(np.int16).copy()).view(dtype), bits


def _widen(lib, kind, bits16):
    bits16 = np.ascontiguousarray(bits16, dtype=np.uint16)
    out = np.empty(bits16.size, dtype=np.uint32)
    lib.half_widen(kind, bits16.ctypes.data, bits16.size, out.ctypes.data)
    return out


def _narrow(lib, kind, bits32):
    bits32 = np.ascontiguousarray(bits32, dtype=np.uint32)
    out = np.empty(bits32.size, dtype=np.uint16)
    lib.half_narrow(kind, bits32.ctypes.data, bits32.size, out.ctypes.data)
    return out


def _torch_narrow(bits32, dtype):
    f = torch.from_numpy(np.ascontiguousarray(bits32, dtype=np.uint32).view(np.int32).copy()).view(torch.float32)
    return f.to(dtype).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("name", sorted(KINDS))
def test_widening_is_exact_for_every_bit_pattern(lib, name):
    kind, dtype = KINDS[name]
    t, bits = _all_halves(dtype)
    want = t.to(torch.float32).view(torch.int32).numpy().view(np.uint32)
    got = _widen(lib, kind, bits)
    nan = np.isnan(want.view(np.float32))
    assert np.array_equal(np.isnan(got.view(np.float32)), nan)               # NaN stays NaN (the payload is not compared)
    assert np.array_equal(got[~nan], want[~nan])


@pytest.mark.parametrize("name", sorted(KINDS))
def test_narrowing_rounds_like_torch(lib, name):
    kind, dtype = KINDS[name]
    t, bits = _all_halves(dtype)
    wide = t.to(torch.float32).view(torch.int32).numpy().view(np.uint32)
    finite = np.isfinite(wide.view(np.float32))
    w = wide[finite]
    cases = [w, w + 1, w - 1]                                                # every half value and its float32 neighbours (+-0 wrap into NaNs: below)
    # the ties: the midpoint of every pair of adjacent half values of one sign, exact in float64 and in float32 (one more bit)
    mag = np.sort(np.unique(np.abs(w.view(np.float32)).astype(np.float64)))
    mid = (0.5 * (mag[:-1] + mag[1:])).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), 0.5 * (mag[:-1] + mag[1:]))
    mid_bits = mid.view(np.uint32)
    cases += [mid_bits, mid_bits | 0x80000000, mid_bits + 1, mid_bits - 1]
    # the overflow threshold (largest finite + half a step) and its neighbours, both signs
    big = mag[-1] + 0.5 * (mag[-1] - mag[-2])
    thr = np.array([big], dtype=np.float32).view(np.uint32)[0]
    around = np.arange(int(thr) - 4, int(thr) + 5, dtype=np.int64).astype(np.uint32)
    cases += [around, around | 0x80000000]
    if name == "f16":
        # the subnormal range and below it: every float32 exponent from 2^-27 to 2^-13 on a fine grid of significands
        grid = (np.arange(0, 1 << 23, 4093, dtype=np.uint32))[None, :] | (np.arange(100, 115, dtype=np.uint32) << 23)[:, None]
        cases += [grid.ravel(), grid.ravel() | 0x80000000, np.array([0x33000000, 0x33000001, 0x32ffffff, 0x33800000], dtype=np.uint32)]
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e38, -1e38, 3.4028235e38, 1e-45, -1e-45], dtype=np.float32).view(np.uint32)
    cases.append(special)
    x = np.concatenate([np.asarray(c, dtype=np.uint32).ravel() for c in cases])
    got, want = _narrow(lib, kind, x), _torch_narrow(x, dtype)
    xf = x.view(np.float32)
    nan = np.isnan(xf)
    t_got = torch.from_numpy(got.view(np.int16).copy()).view(dtype)
    assert bool(torch.isnan(t_got[torch.from_numpy(nan)]).all())              # NaN stays NaN, whatever its payload
    bad = np.flatnonzero(~nan & (got != want))
    assert bad.size == 0, [(hex(x[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]
    # (a NaN's bits are not compared: torch's own differ between its scalar and its vectorised bfloat16 path, 0x7fc0 and 0xffff)
    assert bool(torch.isnan(torch.from_numpy(want.view(np.int16).copy()).view(dtype)[torch.from_numpy(nan)]).all())


def test_the_header_needs_no_hip_header():
    with open(os.path.join(os.path.dirname(HERE), "cca_zoo_amd", "csrc", "half_cvt.h"), encoding="utf-8") as f:
        text = f.read()
    assert "#include <hip" not in text and "hip_runtime" not in text
