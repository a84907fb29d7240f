"""The arithmetic of the bfloat16 projection kernel (cca_zoo_amd/csrc/project_bf16.hip), restated in NumPy (CPU only).

A bf16 value is the top 16 bits of a float32; rounding is to nearest even on the bit pattern, as v_cvt_pk_bf16_f32 does.  The
kernel multiplies bf16 rows x with three bf16 planes of W, ``hi + mid + lo``, and adds the products in float32:

  * the three planes reproduce fl32(w) exactly (so nothing of W is lost beyond its float32 rounding),
  * every product of two bf16 values has at most 16 significant bits: it is exact in float32,
  * what is left is float32 accumulation, which has to hold the float32 projection's own bar against float64.
"""

import numpy as np


def bf16_round(x):
    """float32 -> the nearest bfloat16 (ties to even), returned as float32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def planes(w):
    """k_project_prep's split of fl32(w): hi = bf16(w), mid = bf16(w - hi), lo = bf16(w - hi - mid), each difference in float32."""
    w = np.asarray(w, dtype=np.float32)
    hi = bf16_round(w)
    r = (w - hi).astype(np.float32)
    mid = bf16_round(r)
    lo = bf16_round((r - mid).astype(np.float32))
    return hi, mid, lo


def test_rounding_is_to_nearest_even():
    one = np.float32(1.0)
    ulp = np.float32(2.0 ** -7)                            # spacing of bf16 in [1, 2)
    assert bf16_round(one + ulp / 2) == one                # tie: 1.0 has the even mantissa
    assert bf16_round(one + ulp + ulp / 2) == one + 2 * ulp
    assert bf16_round(one + ulp * np.float32(0.75)) == one + ulp
    assert bf16_round(np.float32(-3.0)) == np.float32(-3.0)


def test_three_planes_reproduce_float32_exactly():
    rng = np.random.default_rng(0)
    mant = rng.uniform(1.0, 2.0, 100_000)
    expo = rng.integers(-20, 20, 100_000)                  # 40 binades, every plane stays a normal number
    w = (np.where(rng.random(100_000) < 0.5, -1.0, 1.0) * mant * 2.0 ** expo).astype(np.float32)
    w = np.concatenate([w, np.array([0.0, -0.0], dtype=np.float32)])
    hi, mid, lo = planes(w)
    back = hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64)
    assert np.array_equal(back, w.astype(np.float64))
    # and in float32, in the order the accumulator sees them scaled by an x of one
    assert np.array_equal(((hi + mid).astype(np.float32) + lo).astype(np.float32), w)
    for p in (hi, mid, lo):                                # each plane IS a bf16: the low 16 bits are clear
        assert not np.any(p.view(np.uint32) & 0xFFFF)


def test_products_of_bf16_values_are_exact_in_float32():
    rng = np.random.default_rng(1)
    x = bf16_round((rng.standard_normal(100_000) + 0.3).astype(np.float32))
    w = (rng.standard_normal(100_000) * 2.0 ** rng.integers(-10, 10, 100_000)).astype(np.float32)
    for p in planes(w):
        exact = x.astype(np.float64) * p.astype(np.float64)
        assert np.array_equal((x * p).astype(np.float32).astype(np.float64), exact)


def emulate(x, mean, W):
    """The kernel's sums: per k-step of 16 columns and per output, acc += Wh x; acc += Wm x; acc += Wl x in float32 (a k-step's
    16 exact products added in float32 here, which is no better than the matrix pipe's own sum), bias = mean' W in float64,
    out = fl32(acc - bias)."""
    n, d = x.shape
    hi, mid, lo = planes(W)
    acc = np.zeros((n, W.shape[1]), dtype=np.float32)
    for s in range(0, d, 16):
        for p in (hi, mid, lo):
            part = np.zeros_like(acc)
            for c in range(s, min(s + 16, d)):
                part = (part + x[:, c:c + 1] * p[c:c + 1, :]).astype(np.float32)
            acc = (acc + part).astype(np.float32)
    bias = mean @ W if mean is not None else 0.0
    return (acc.astype(np.float64) - bias).astype(np.float32)


def test_emulated_projection_holds_the_float32_bar():
    rng = np.random.default_rng(300 + 1040 + 5)
    n, d, k = 300, 1040, 5
    x = bf16_round((rng.standard_normal((n, d)) + 0.3).astype(np.float32))
    mean, W = rng.standard_normal(d), rng.standard_normal((d, k))
    for m in (mean, None):
        ref = (x.astype(np.float64) - (m if m is not None else 0.0)) @ W
        got = emulate(x, m, W)
        scale = np.abs(ref).max()
        err = np.abs(got - ref).max()
        print(f"emulated 300 x 1040 x 5, mean={'yes' if m is not None else 'no'}: err {err:.3e}, bar {2e-5 * scale * np.sqrt(d):.3e}")
        assert err < 2e-5 * scale * np.sqrt(d)             # the bar of tests/test_gpu_ops.py for the float32 projection
