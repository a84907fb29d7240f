"""The split-bf16 K1 route (cca_zoo_amd/csrc/gram_split.hip, the split branch of gram.hip::launch_moments) restated in NumPy, the
slow literal way (imported by tests/test_k1_split_emulation_host.py and tests/test_gpu_k1_split_structured.py).

For float32 views x (n rows, stacked width D) and a float32 pilot p the route computes

    d = fl32(x - p),   hi = bf16(d),   mid = bf16(d - hi)                    (round to nearest even; d - hi is exact in float32)
    G = H'H + H'M + M'H,   G_ii += sum_k mid_ki^2                            (the diagonal of G only: k_split_reduce)
    X'X = G + p s' + s p' - n p p'                                           (s: exact float64 column sums; k_pilot_fixup)

with float32 accumulation inside a row chunk of a workgroup and float64 across chunks.  ``moments`` is that arithmetic with float64
accumulation throughout -- the error of the DESIGN, nothing of float32 summation in it; ``moments_f32_chunks`` puts float32 sums
inside row chunks back to size what accumulation may add; ``exact_int`` is the same in integers for inputs on a grid.

The pilot is the one launch_moments forms for float32 views (k_sample_grid, k_pilot_coarse): from rows ``i * (n // nsamp)``,
``i < nsamp = min(n, 2048)``, with float64 sums and sums of squares,

    mean = s / nsamp,   sd = sqrt(max(0, sq / nsamp - mean^2)),   u = 2^(ilogb(sd) - 3),   p = fl32(rint(mean / u) * u)

for every column that lies ON A GRID -- each sampled value a multiple of u / 8, or of at most 8 significant bits (up-cast from
bfloat16) -- and ``p = fl32(s * (1 / nsamp))``, the sample mean the route always used, for every other column, and where sd == 0 or
anything is not finite.  |p - mean| <= sd / 8, so the coarse pilot centres as well as the mean does, and it has the fewest
significant bits of the candidates that near: grid-valued columns (0/1, one-hot, pixels, counts, integers) keep their grid under
``x - p``, hi then holds them exactly and mid = 0.  Why not the coarse pilot for every column: it gains nothing on generic
float32 values (Gaussian columns: 1.4e-7 against 1.3e-7), but it is another rounding of every product -- the moments of inputs
the route served well, and every weight computed from them, would stop being the bits they were.  So ReLU outputs keep the mean
pilot and their design error (2e-6, pinned in the GPU tests).  ``rule="mean"`` is the plain sample mean for every column, what
the route did before; ``rule="coarse_all"`` the coarse pilot for every column; both stay here so that the host tests keep showing
why the rule is what it is.
"""

import numpy as np

K_STEP = 16            # rows per k-step of the Gram kernel (SP_K)
PILOT_SAMPLE = 2048    # rows of the pilot sample at most


def bf16_round(x):
    """float32 -> the nearest bfloat16 (ties to even), as float32: on the bit pattern, what ``sp_pack2`` does (finite inputs)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32)
    r = (b + (np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)       # (no carry out of 32 bits: finite)
    return r.view(np.float32).reshape(x.shape)


def stack(views):
    X = np.ascontiguousarray(np.hstack([np.asarray(v) for v in views]))
    assert X.dtype == np.float32
    return X


def pilot_sample(views):
    """The rows the pilot is formed from, float64: (nsamp, D)."""
    X = stack(views)
    n = X.shape[0]
    nsamp = min(n, PILOT_SAMPLE)
    stride = n // nsamp
    return X[: nsamp * stride : stride].astype(np.float64)


def sample_grid(S32):
    """Per column of the float32 sample: the exponent of the lowest set bit over its nonzero values (10**6: none seen) and
    the most significant bits any value has -- k_sample_grid."""
    b = np.ascontiguousarray(S32, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    e = (b >> np.uint32(23)).astype(np.int64)
    m = (b & np.uint32(0x7FFFFF)).astype(np.int64)
    m = np.where(e > 0, m | 0x800000, m)
    e = np.where(e > 0, e, 1)
    low = m & -m
    tz = np.frexp(np.where(low > 0, low, 1).astype(np.float64))[1] - 1
    width = np.frexp(np.where(m > 0, m, 1).astype(np.float64))[1] - tz
    nz = b != 0
    assert np.all(e[nz] < 255), "non-finite sample"
    return np.where(nz, e - 150 + tz, 10 ** 6).min(axis=0), np.where(nz, width, 0).max(axis=0)


def pilot_stats(views, rule="coarse"):
    """mean, sd and the unit u of every column of the sample (u = 0 where the rule takes the mean)."""
    X = stack(views)
    n = X.shape[0]
    nsamp = min(n, PILOT_SAMPLE)
    S32 = X[: nsamp * (n // nsamp) : n // nsamp]
    S = S32.astype(np.float64)
    with np.errstate(all="ignore"):
        mean = S.sum(axis=0) / float(nsamp)
        var = (S * S).sum(axis=0) / float(nsamp) - mean * mean
        ok = np.isfinite(mean) & np.isfinite(var) & (var > 0.0)
        sd = np.sqrt(np.where(ok, var, 0.0))
        eu = np.frexp(np.where(ok, sd, 1.0))[1] - 1 - 3            # ilogb(sd) - 3
        if rule == "coarse" and np.all(np.isfinite(S32)):
            gexp, bits = sample_grid(S32)
            ok &= (gexp < 10 ** 6) & ((gexp >= eu - 3) | (bits <= 8))
        elif rule == "coarse":
            ok &= False                                            # (per column on the device; the tests have no use for it)
        u = np.where(ok, np.ldexp(1.0, eu), 0.0)
    return mean, sd, u


def pilot(views, rule="coarse"):
    assert rule in ("coarse", "coarse_all", "mean")
    S = pilot_sample(views)
    with np.errstate(all="ignore"):
        plain = S.sum(axis=0) * (1.0 / float(S.shape[0]))
        if rule == "mean":
            return plain.astype(np.float32)
        mean, _, u = pilot_stats(views, rule)
        r = np.rint(mean / np.where(u > 0.0, u, 1.0)) * u
    return np.where((u > 0.0) & np.isfinite(r), r, plain).astype(np.float32)


def planes(views, p):
    """d = fl32(x - p) as the two bf16 planes (float32 arrays): hi, mid."""
    X = stack(views)
    d = X - np.asarray(p, dtype=np.float32)[None, :]               # float32 - float32: one rounding
    hi = bf16_round(d)
    mid = bf16_round(d - hi)
    return hi, mid


def fixup(G, views, p):
    """G + p s' + s p' - n p p' in float64 with the exact float64 column sums; returns (moments, s)."""
    X = stack(views)
    s = X.astype(np.float64).sum(axis=0)
    p64 = np.asarray(p, dtype=np.float32).astype(np.float64)
    return G + np.outer(p64, s) + np.outer(s, p64) - float(X.shape[0]) * np.outer(p64, p64), s


def moments(views, p):
    """The designed arithmetic, float64 accumulation: (D x D moments, column sums)."""
    hi, mid = planes(views, p)
    H, M = hi.astype(np.float64), mid.astype(np.float64)
    HM = H.T @ M
    G = H.T @ H + HM + HM.T
    G[np.diag_indices_from(G)] += (M * M).sum(axis=0)
    return fixup(G, views, p)


def moments_f32_chunks(views, p, rows):
    """The same planes with float32 accumulation inside chunks of ``rows`` rows -- one float32 matmul of the stacked operands
    (H, H, M)' (H, M, H) per chunk -- and float64 across chunks: the host model of "fp32 inside a row chunk, fp64 across"."""
    hi, mid = planes(views, p)
    D = hi.shape[1]
    G = np.zeros((D, D))
    for r0 in range(0, hi.shape[0], rows):
        h, m = hi[r0:r0 + rows], mid[r0:r0 + rows]
        G += (np.vstack([h, h, m]).T @ np.vstack([h, m, h])).astype(np.float64)
    M = mid.astype(np.float64)
    G[np.diag_indices_from(G)] += (M * M).sum(axis=0)
    return fixup(G, views, p)


def grid_unit(d):
    """Per column the largest power of two that divides every entry of the float32 array d (1 for a column of zeros)."""
    m, e = np.frexp(d)                                             # float32 in, m in [0.5, 1) exactly
    k = np.ldexp(m, 24).astype(np.int32)                           # the 24-bit integer mantissa
    low = (k & -k).astype(np.float32)                              # its lowest set bit, a power of two
    ex = np.where(k != 0, e - 25 + np.frexp(low)[1], np.int32(1 << 20))
    emin = ex.min(axis=0)
    return np.ldexp(1.0, np.where(emin == (1 << 20), 0, emin))


def _int_product(A, B):
    """A'B of integer-valued float64 arrays as int64.  The sums are carried by the float64 BLAS product, which is integer
    arithmetic as long as no partial sum reaches 2^53 -- asserted on sqrt(max_i sum A_i^2  max_j sum B_j^2), which bounds every
    entry of |A|'|B| and with it every partial sum."""
    assert np.sqrt((A * A).sum(axis=0).max(initial=0.0) * (B * B).sum(axis=0).max(initial=0.0)) < 2.0 ** 52
    if not A.any() or not B.any():
        return np.zeros((A.shape[1], B.shape[1]), dtype=np.int64)
    return np.rint(A.T @ B).astype(np.int64)


def exact_int(views, p, window_steps=16):
    """For inputs whose d / u are integers (u: ``grid_unit`` of d, per column): the three plane products and the diagonal term in
    integers, scaled back by u_i u_j and fixed up like ``moments`` -- (moments, column sums, units u, window maximum).  The window
    maximum is max over (i, j) and over every window of ``window_steps`` consecutive k-steps (256 rows; windows start at every
    k-step, i.e. every multiple of 16 rows) of  sum |terms| / (u_i u_j):  below 2^24 every float32 partial sum a workgroup can form
    over such a window is an integer multiple of u_i u_j that float32 holds exactly, whatever the order of the additions."""
    hi, mid = planes(views, p)
    d = hi + mid
    X = stack(views)
    assert np.array_equal(d, X - np.asarray(p, dtype=np.float32)[None, :]), "d does not fit two bf16 planes"
    u = grid_unit(d)
    H, M = (hi / u.astype(np.float32)).astype(np.float64), (mid / u.astype(np.float32)).astype(np.float64)      # exact: powers of two
    HH = _int_product(H, H)
    HM = _int_product(H, M)
    K = HH + HM + HM.T
    K[np.diag_indices_from(K)] += np.rint((M * M).sum(axis=0)).astype(np.int64)
    assert np.abs(K).max(initial=0) < 2 ** 52
    G = K.astype(np.float64) * np.outer(u, u)                      # exact: powers of two
    # sum |terms| over a window is W = A'A - B'B of its rows, A = |H| + |M|, B = |M|.  W_ij <= sqrt(sum A_i^2 sum A_j^2) <= the largest
    # column sum of A^2 over the window, which costs O(n D) for all windows: the windows are visited from the largest such bound
    # down and the search stops where the bound no longer exceeds the maximum found -- the exact maximum, a few products.
    n, D = H.shape
    steps = (n + K_STEP - 1) // K_STEP
    B = np.abs(M)
    A = np.abs(H) + B
    sq = np.add.reduceat(A * A, np.arange(0, n, K_STEP), axis=0)   # per k-step
    cum = np.vstack([np.zeros((1, D)), np.cumsum(sq, axis=0)])
    starts = np.arange(max(1, steps - window_steps + 1))           # (later starts are sub-windows of these)
    bound = (cum[np.minimum(starts + window_steps, steps)] - cum[starts]).max(axis=1)
    worst = 0.0
    for w in np.argsort(-bound):
        if bound[w] <= worst:
            break
        r0, r1 = starts[w] * K_STEP, (starts[w] + window_steps) * K_STEP
        worst = max(worst, float((A[r0:r1].T @ A[r0:r1] - B[r0:r1].T @ B[r0:r1]).max()))
    out, s = fixup(G, views, p)
    return out, s, u, worst


def rel(G, Gr):
    """The measure of tests/test_gpu_k1_split.py::_rel: max over the upper triangle of |G - Gr| / sqrt(Gr_ii Gr_jj)."""
    iu = np.triu_indices(G.shape[0])
    scale = np.sqrt(np.outer(np.diag(Gr), np.diag(Gr)))
    return float((np.abs(G - Gr) / scale)[iu].max())


def centred(G, s, n):
    return G - np.outer(s, s) / float(n)


def float64_moments(views):
    X = stack(views).astype(np.float64)
    return X.T @ X, X.sum(axis=0)


def pilot_fragile_columns(views, tol=1e-6):
    """Columns whose coarse pilot could depend on the order of the sample's float64 sums: mean / u within ``tol`` of a half-integer,
    or the sample's sd within ``tol`` (relative) of a power of two."""
    mean, sd, u = pilot_stats(views)
    live = u > 0.0
    q = mean / np.where(live, u, 1.0)
    m = np.frexp(np.where(live, sd, 0.75))[0]                      # in [0.5, 1): a power of two sits at 0.5 (and at 1)
    return live & ((np.abs(q - np.floor(q) - 0.5) <= tol) | (m - 0.5 <= tol) | (1.0 - m <= tol))


def pilot_is_order_robust(views, tol=1e-6):
    return not bool(np.any(pilot_fragile_columns(views, tol)))


def settle_pilot(views, lo, hi, onehot=False):
    """Grid-valued columns sit ON such a boundary with a probability of about 2^-7 each (0/1 features: mean / u = ones / 128), so
    among hundreds of columns one always does.  This moves one entry of a SAMPLED row of every fragile column by one grid step
    (inside [lo, hi]; one-hot blocks: the row's label moves to the neighbouring class) and repeats until no column is left.  In
    place; the views stay on their grid and in their range."""
    n = views[0].shape[0]
    nsamp = min(n, PILOT_SAMPLE)
    stride = n // nsamp
    where = [(v, j) for v in views for j in range(v.shape[1])]
    for it in range(200):
        bad = np.flatnonzero(pilot_fragile_columns(views))
        if bad.size == 0:
            return views
        for g in bad:
            v, j = where[g]
            if onehot:
                j2 = j + 1 if (j % 8 != 7 and j + 1 < v.shape[1]) else j - 1
                rows = np.flatnonzero(v[: nsamp * stride : stride, j] == 1.0)
                r = rows[it % rows.size] * stride
                v[r, j], v[r, j2] = 0.0, 1.0
            else:
                r = ((7 * it + 13 * int(g)) % nsamp) * stride
                v[r, j] = v[r, j] + 1.0 if v[r, j] + 1.0 <= hi else v[r, j] - 1.0
                assert lo <= v[r, j] <= hi
    raise AssertionError("the pilot of some column stays on a rounding boundary")


# ---------------------------------------------------------------------------------------------------------------------------
# inputs: the structured float32 views the tests run (fixed seeds; every generator returns a list of float32 views)
# ---------------------------------------------------------------------------------------------------------------------------
def _base(rng, n, dims, k=4):
    z = rng.standard_normal((n, k))
    return [z @ rng.standard_normal((k, d)) + rng.standard_normal((n, d)) for d in dims]


def _f32(vs):
    return [np.ascontiguousarray(v, dtype=np.float32) for v in vs]


SETTLE = {"binary": (0.0, 1.0), "onehot": (0.0, 1.0), "pixels8": (0.0, 255.0), "pixels7": (0.0, 127.0), "counts": (0.0, 2.0 ** 20),
          "int300": (297.0, 303.0)}


def make_views(kind, n, dims, seed, settle=False):
    """``settle``: grid-valued kinds are passed through ``settle_pilot`` (the other kinds are returned as drawn)."""
    views = _draw(kind, n, dims, seed)
    if settle and kind in SETTLE:
        settle_pilot(views, *SETTLE[kind], onehot=kind == "onehot")
    return views


def _draw(kind, n, dims, seed):
    rng = np.random.default_rng(seed)
    if kind == "gaussian":
        return _f32(_base(rng, n, dims))
    if kind == "binary":                                           # 0/1 features, correlated through the latent
        return _f32([b > 0.3 for b in _base(rng, n, dims)])
    if kind == "onehot":                                           # blocks of 8 classes (the last block of a view may be cut)
        out = []
        for d in dims:
            nb = (d + 7) // 8
            lab = rng.integers(0, 8, size=(n, nb))
            out.append((lab[:, :, None] == np.arange(8)[None, None, :]).reshape(n, nb * 8)[:, :d])
        return _f32(out)
    if kind == "pixels8":                                          # 8-bit pixel values
        return _f32([np.clip(np.rint(b * 30.0 + 127.0), 0, 255) for b in _base(rng, n, dims)])
    if kind == "pixels7":                                          # 7-bit pixel values
        return _f32([np.clip(np.rint(b * 15.0 + 63.0), 0, 127) for b in _base(rng, n, dims)])
    if kind == "counts":
        return _f32([rng.poisson(3.0, (n, d)) for d in dims])
    if kind == "int300":                                           # integer-valued measurements, 300 +- 3
        return _f32([300.0 + rng.integers(-3, 4, size=(n, d)) for d in dims])
    if kind == "sparse_int":
        # signed integers of 9 and 10 bits (mid != 0), zero elsewhere, an independent pattern per column.  One entry of magnitude v
        # alone puts v^2 into a window's sum |terms| on the diagonal, so a window bound of 2^22 admits no value from 2^11 on and
        # about four of 2^10: hence magnitudes in [256, 1023] on 1/512 of the entries.
        out = []
        for d in dims:
            mag = rng.integers(256, 1024, size=(n, d)) * rng.choice([-1, 1], size=(n, d))
            out.append(np.where(rng.random((n, d)) < 1.0 / 512.0, mag, 0))
        return _f32(out)
    if kind == "relu":
        return _f32([np.maximum(b, 0.0) for b in _base(rng, n, dims)])
    if kind == "from_bf16":                                        # float32 values up-cast from bfloat16
        return [bf16_round((b + 1.5).astype(np.float32)) for b in _base(rng, n, dims)]
    if kind == "mean1000":                                         # every column mean 1000 sigma away from zero
        return _f32([b / b.std(axis=0) + 1000.0 for b in _base(rng, n, dims)])
    if kind == "duplicate":                                        # the later views repeat columns of the first
        vs = _f32(_base(rng, n, dims))
        for v in vs[1:]:
            w = min(v.shape[1], vs[0].shape[1]) // 2 if len(dims) > 2 else min(v.shape[1], vs[0].shape[1])
            v[:, :w] = vs[0][:, :w]
        return vs
    if kind == "outlier_row":                                      # one row at 1e4 sigma
        vs = _f32(_base(rng, n, dims))
        for v in vs:
            v[n // 3] += np.float32(1e4)
        return vs
    if kind == "student_t":
        return _f32([rng.standard_t(2.5, (n, d)) for d in dims])
    if kind == "period16":                                         # phase 0 of a period of 16 rows shifted by 20 sigma
        return _f32([b + (np.arange(n)[:, None] % 16 == 0) * 20.0 for b in _base(rng, n, dims)])
    raise ValueError(kind)
