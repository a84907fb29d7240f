"""bfloat16 / float16 batches in the deep objectives (include/ccz.h: CCZ_BF16, CCZ_F16; csrc/half_cvt.h, half_io.hip, the half
instantiation of gram_split.hip's split pass).  Half precision is a FORMAT: an element is widened exactly on load, the float32
routes compute, every gradient is rounded once.  So K1 is held to the bars of tests/test_gpu_k1_split.py against float64
moments of the exactly widened views, and the objectives to the project's float32 bar (1e-3) plus one rounding of the type
against goldens that the reference computed in float64 at the rounded inputs (tools/gen_golden_half.py)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}                     # unit roundoff of one rounding to the type
TINY = {"bf16": 0.0, "f16": 2.0 ** -25}                       # half the spacing of fp16's subnormals
CASES = ("cca", "mcca", "gcca", "tcca", "ey", "barlow", "vicreg", "sdl", "cca_offset", "gcca_offset", "tcca_offset", "ey_offset")


def _tdt(name):
    import torch

    return {"bf16": torch.bfloat16, "f16": torch.float16}[name]


def _code(name):
    from cca_zoo_amd import _backend

    return {"bf16": _backend.BF16, "f16": _backend.F16}[name]


@pytest.fixture(scope="module")
def H():
    from cca_zoo_amd import _backend

    h = _backend.default_handle(0)
    yield h
    h.k1_route("auto")


# ---------------------------------------------------------------------------------------------------------------------
# K1 through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _half_views(name, n, dims, lds, shift=0.0, elem_offset=0):
    """Half views on the device, view v = columns [0, dims[v]) of an (n, lds[v]) buffer that starts `elem_offset` elements into
    its allocation; and their exact float64 images.  The draw is that of tests/test_gpu_k1_split.py (_latent, six shared latents,
    seed = rows + views as in its parametrised cases), rounded to the half type: the bars below were set on such rows."""
    import torch

    rng = np.random.default_rng(n + len(dims))
    lat = rng.standard_normal((n, 6))
    views, wide = [], []
    for d, ld in zip(dims, lds):
        x = torch.from_numpy(lat @ rng.standard_normal((6, d)) + rng.standard_normal((n, d)) + shift).to(_tdt(name))
        flat = torch.zeros(n * ld + 8, dtype=_tdt(name), device="cuda")
        v = flat[elem_offset:elem_offset + n * ld].view(n, ld)[:, :d]
        v.copy_(x)
        views.append(v)
        wide.append(x.to(torch.float64).numpy())
    return views, wide


def _k1(H, name, views, route, mom=None):
    import torch

    n = views[0].shape[0]
    D = sum(v.shape[1] for v in views)
    accumulate = mom is not None
    mom = mom if accumulate else H.alloc((D * D + D) * 8)
    torch.cuda.synchronize()
    prev = H.k1_route(route)
    try:
        H.moments([(v.data_ptr(), v.shape[1], v.stride(0)) for v in views], n, _code(name), True, mom.ptr, accumulate=accumulate)
        taken = H.moments_last_route()[0]
    finally:
        H.k1_route(prev)
    flat = H.to_host(mom, (D * D + D,))
    return flat[: D * D].reshape(D, D), flat[D * D:], taken, mom


def _ref(wide):
    X = np.hstack(wide)
    return X.T @ X, X.sum(axis=0)


def _rel(G, Gr):                                               # the measure of tests/test_gpu_k1_split.py
    iu = np.triu_indices(G.shape[0])
    scale = np.sqrt(np.outer(np.diag(Gr), np.diag(Gr)))
    return float((np.abs(G - Gr) / scale)[iu].max())


def _bar(n):
    """tests/test_gpu_k1_split.py on float32 views: 2e-6, and 1.2e-5 below 4096 rows (test_split_route_random_shapes: with a few
    dozen rows the dropped 2^-16 terms do not average out yet)."""
    return 1.2e-5 if n < 4096 else 2e-6


def _check_k1(H, name, views, wide, route, what):
    Gr, sr = _ref(wide)
    G, s, taken, _ = _k1(H, name, views, route)
    print(f"{what} {name} {route}: K1 error {_rel(G, Gr):.2e} (bar {_bar(views[0].shape[0]):.1e})")
    assert taken == route
    assert _rel(G, Gr) < _bar(views[0].shape[0])
    np.testing.assert_allclose(s, sr, rtol=1e-12, atol=1e-7)


@pytest.mark.parametrize("route", ["fp32", "bf16x2"])
@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_k1_ragged_panel_odd_rows_odd_ld(H, name, route):
    views, wide = _half_views(name, 47, (5, 259), (7, 261))
    _check_k1(H, name, views, wide, route, "47 x (5, 259)")


@pytest.mark.parametrize("route", ["fp32", "bf16x2"])
@pytest.mark.parametrize("name", ["bf16", "f16"])
@pytest.mark.parametrize("elem_offset", [0, 1])
def test_k1_aligned_rows_and_a_base_pointer_one_element_off(H, name, route, elem_offset):
    """4100 x (256, 256), ld 264: the 8-byte loads of the split pass / the 16-byte lanes of the widening kernel; the same views
    from a base pointer that is only 2-byte aligned take the element-wise paths.

    bfloat16 rows are the hard case of the split route: on an 8-bit grid an arbitrary float32 pilot makes the residual plane nearly
    the same number for every row of a binade, and the dropped mid_i mid_j products then add up over the rows (2.37e-6 here, above
    the bar, measured with the sample-mean pilot); K1 snaps the pilot of half rows to their grid instead (gram.hip:
    k_pilot_on_grid)."""
    views, wide = _half_views(name, 4100, (256, 256), (264, 264), elem_offset=elem_offset)
    assert views[0].data_ptr() % 16 == 2 * elem_offset
    _check_k1(H, name, views, wide, route, f"4100 x (256, 256), offset {elem_offset}")


@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_k1_split_route_super_chunks_and_accumulate(H, name, monkeypatch):
    """Several row super-chunks of 256-row workgroup chunks on inputs shifted by 2, then a second, accumulating call."""
    monkeypatch.setenv("CCZ_SPLIT_SCRATCH_GB", "0.008")
    monkeypatch.setenv("CCZ_SPLIT_ROWS", "256")
    a, wa = _half_views(name, 6000, (300, 200), (300, 200), shift=2.0)
    b, wb = _half_views(name, 2500, (300, 200), (300, 200), shift=2.0)
    (Ga, sa), (Gb, sb) = _ref(wa), _ref(wb)
    G, s, taken, mom = _k1(H, name, a, "bf16x2")
    assert taken == "bf16x2" and _rel(G, Ga) < 2e-6, _rel(G, Ga)
    G, s, taken, _ = _k1(H, name, b, "bf16x2", mom=mom)
    assert taken == "bf16x2" and _rel(G, Ga + Gb) < 2e-6, _rel(G, Ga + Gb)
    np.testing.assert_allclose(s, sa + sb, rtol=1e-12, atol=1e-7)


@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_k1_fp32_route_adapter_chunks_with_a_one_row_tail(H, name, monkeypatch):
    """CCZ_HALF_SCRATCH_MB=1 with 300 + 224 float32 scratch columns: 2096 bytes per row, 500 rows per chunk (half_io.hip:
    half_chunk_rows), so 6001 rows are twelve chunks and a 1-row tail that is folded into the twelfth."""
    monkeypatch.setenv("CCZ_HALF_SCRATCH_MB", "1")
    chunk = (1 << 20) // (4 * (300 + 224))
    n = 12 * chunk + 1
    assert (chunk, n) == (500, 6001)
    views, wide = _half_views(name, n, (300, 224), (300, 224), shift=0.5)
    _check_k1(H, name, views, wide, "fp32", "6001 x (300, 224) in chunks")


@pytest.mark.parametrize("route", ["fp32", "bf16x2"])
@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_k1_inf_reaches_its_column_sum(H, name, route):
    views, wide = _half_views(name, 300, (40, 24), (40, 24))
    views[0][17, 5] = float("inf")
    G, s, taken, _ = _k1(H, name, views, route)
    assert taken == route and not np.isfinite(s[5]) and np.isfinite(s[6])


@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_k1_host_half_views_are_refused(H, name):
    x = np.zeros((64, 8), dtype=np.uint16)
    mom = H.alloc((64 + 8) * 8)
    with pytest.raises(ValueError, match="moments.*on the device"):             # CCZ_EUNSUP
        H.moments([(x, 8, 8)], 64, _code(name), False, mom.ptr)


def test_another_familys_entry_still_refuses_bf16(H):
    from cca_zoo_amd import _backend

    buf = H.alloc(64 * 8 * 8)
    rc = H.lib.ccz_randn_fill(H.raw, _backend.BF16, C.c_void_p(buf.ptr), 64, 8, 8, 1, 0, 8, 1.0, 0)
    assert rc == -6                                                             # CCZ_EUNSUP
    with pytest.raises(ValueError):
        H.check(rc)


# ---------------------------------------------------------------------------------------------------------------------
# the objectives against the goldens
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def goldens():
    out = {}
    for name in ("bf16", "f16"):
        for case in CASES:
            with np.load(os.path.join(GOLDEN, f"half_{name}_{case}.npz")) as f:
                out[name, case] = {k: f[k] for k in f.files}
    return out


def _module(case, g):
    from cca_zoo_amd.deep import objectives as ob
    from cca_zoo_amd.deep import _ssl

    family = case.split("_")[0]
    if family in ("cca", "mcca", "gcca", "tcca"):
        cls = {"cca": ob.CCALoss, "mcca": ob.MCCALoss, "gcca": ob.GCCALoss, "tcca": ob.TCCALoss}[family]
        return cls(eps=float(g["eps"]))
    cls = {"ey": _ssl.EYLoss, "barlow": _ssl.BarlowTwinsLoss, "vicreg": _ssl.VICRegLoss, "sdl": _ssl.SDLLoss}[family]
    return cls(*[float(p) for p in g["params"]])


def _inputs(name, g, requires_grad=True):
    import torch

    zs, i = [], 0
    while f"z{i}" in g:
        z = torch.from_numpy(g[f"z{i}"].view(np.int16).copy()).view(_tdt(name)).cuda()
        zs.append(z.requires_grad_(requires_grad))
        i += 1
    return zs


def _check_grad(name, got, ref, what, factor=1.0):
    """every element: |g - ref| <= u |ref| + 1e-3 max|ref| (+ 2^-25 for fp16): one rounding of the type plus the float32 bar"""
    ref = factor * ref.astype(np.float64)
    got = got.detach().to("cpu").double().numpy()
    bound = U[name] * np.abs(ref) + 1e-3 * np.abs(ref).max() + TINY[name]
    worst = float((np.abs(got - ref) / bound).max())
    print(f"{what}: worst |g - ref| / bound {worst:.3f}")
    assert worst <= 1.0, (what, worst)


def _check_case(name, case, g, zs=None, wanted=None, factor=1.0, module=None):
    import torch

    zs = _inputs(name, g) if zs is None else zs
    mod = module or _module(case, g)
    loss = mod(zs)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    (loss * factor).backward()
    torch.cuda.synchronize()
    ref = float(g["loss"])
    print(f"{name} {case}: loss {float(loss.detach()):.6f} reference {ref:.6f}")
    assert abs(float(loss.detach()) - ref) <= 1e-3 * abs(ref)
    for i, z in enumerate(zs):
        if wanted is not None and not wanted[i]:
            assert z.grad is None
            continue
        assert z.grad.dtype == z.dtype and z.grad.shape == z.shape
        _check_grad(name, z.grad, g[f"g{i}"], f"{name} {case} view {i}", factor)
    return mod, zs


@pytest.mark.parametrize("scratch_mb", [None, "0.01"])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_objective_matches_the_float64_reference(goldens, name, case, scratch_mb, monkeypatch):
    """Loss, terms and gradients; again with a scratch budget of 10 KiB -- a few dozen rows per chunk, forward (K1 through the adapter or
    the split pass) and backward."""
    import torch

    if scratch_mb:
        monkeypatch.setenv("CCZ_HALF_SCRATCH_MB", scratch_mb)
    g = goldens[name, case]
    mod, zs = _check_case(name, case, g)
    if hasattr(mod, "terms"):
        terms = mod.terms([z.detach() for z in zs])
        assert terms["objective"].dtype == torch.float32
        assert abs(float(terms["objective"]) - float(g["loss"])) <= 1e-3 * abs(float(g["loss"]))
        for k, v in terms.items():
            if k != "objective":
                assert v.dtype == torch.float32
                assert abs(float(v) - float(g[k])) <= 1e-3 * abs(float(g[k])), (k, float(v), float(g[k]))


@pytest.mark.parametrize("scratch_mb", [None, "0.01"])
@pytest.mark.parametrize("case", ["cca", "mcca", "gcca", "vicreg"])
@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_a_loss_scalers_factor_is_applied_before_the_rounding(goldens, name, case, scratch_mb, monkeypatch):
    if scratch_mb:
        monkeypatch.setenv("CCZ_HALF_SCRATCH_MB", scratch_mb)
    _check_case(name, case, goldens[name, case], factor=1024.0)


@pytest.mark.parametrize("scratch_mb", [None, "0.01"])
@pytest.mark.parametrize("case", ["cca", "mcca", "sdl"])
@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_detached_strided_and_mixed_inputs(goldens, name, case, scratch_mb, monkeypatch):
    import torch

    if scratch_mb:
        monkeypatch.setenv("CCZ_HALF_SCRATCH_MB", scratch_mb)
    g = goldens[name, case]
    # a detached second view
    zs = _inputs(name, g)
    zs[1] = zs[1].detach()
    _check_case(name, case, g, zs=zs, wanted=[i != 1 for i in range(len(zs))])
    # a strided first view: columns of a wider buffer with an odd leading dimension
    zs = _inputs(name, g)
    n, d = zs[0].shape
    wide = torch.zeros(n, d + 3, dtype=zs[0].dtype, device="cuda")
    wide[:, :d] = zs[0].detach()
    leaf = wide.requires_grad_(True)
    mod = _module(case, g)
    loss = mod([leaf[:, :d]] + zs[1:])
    loss.backward()
    assert leaf.grad.dtype == leaf.dtype
    _check_grad(name, leaf.grad[:, :d], g["g0"], f"{name} {case} strided view 0")
    assert float(leaf.grad[:, d:].abs().max()) == 0.0
    _check_grad(name, zs[1].grad, g["g1"], f"{name} {case} view 1 next to a strided view")
    # mixed dtypes follow the first view: a half first view, the second as its exact float32 image
    zs = _inputs(name, g)
    zs[1] = zs[1].detach().float().requires_grad_(True)
    loss = _module(case, g)(zs)
    loss.backward()
    assert loss.dtype == torch.float32 and zs[0].grad.dtype == zs[0].dtype and zs[1].grad.dtype == torch.float32
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-3 * abs(float(g["loss"]))
    for i in (0, 1):
        _check_grad(name, zs[i].grad, g[f"g{i}"], f"{name} {case} mixed view {i}")


@pytest.mark.parametrize("scratch_mb", [None, "0.01"])
@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_row_sharded_forms_at_world_size_one(goldens, name, scratch_mb, monkeypatch):
    import torch.distributed as dist

    from cca_zoo_amd import row_sharded

    if scratch_mb:
        monkeypatch.setenv("CCZ_HALF_SCRATCH_MB", scratch_mb)
    started = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29683", rank=0, world_size=1)
        started = True
    try:
        for case in ("cca", "mcca", "gcca"):
            with row_sharded():
                _check_case(name, case, goldens[name, case])
                _check_case(name, case, goldens[name, case], factor=1024.0)
    finally:
        if started:
            dist.destroy_process_group()


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_forced_split_forward_and_backward(H, name, fused, monkeypatch):
    """32768 x 2 x 256 with both split-bf16 products forced (as test_offset_inputs_on_the_split_backward forces them), against the float64
    closed form at the exactly widened batch.  fused: a scratch budget below the batch, so the forward's K1 is the split pass reading
    the half rows itself; else the batch is widened once and the float32 forward takes its own split-route fast path."""
    import torch

    from cca_zoo_amd.deep.objectives import CCALoss
    from oracle import losses as ol

    monkeypatch.setenv("CCZ_LOSS_BWD_SPLIT", "2")
    monkeypatch.setenv("CCZ_SPLIT_MIN_FLOP", "1e9")
    if fused:
        monkeypatch.setenv("CCZ_HALF_SCRATCH_MB", "16")
    torch.manual_seed(3)
    n, d = 32768, 256
    lat = torch.randn(n, 8)
    z1 = (lat @ torch.randn(8, d) + torch.randn(n, d) + 0.5).to(_tdt(name)).cuda().requires_grad_(True)
    z2 = (lat @ torch.randn(8, d) + torch.randn(n, d) - 0.25).to(_tdt(name)).cuda().requires_grad_(True)
    loss = CCALoss(eps=1e-4)([z1, z2])
    loss.backward()
    torch.cuda.synchronize()
    assert H.loss_last_route() == ("bf16x2", "bf16x2")
    l_ref, g1, g2 = ol.cca_loss_closed_form(z1.detach().double().cpu().numpy(), z2.detach().double().cpu().numpy(), 1e-4)
    print(f"{name} split forward + backward (fused {fused}): loss {float(loss.detach()):.6f} reference {l_ref:.6f}")
    assert loss.dtype == torch.float32 and abs(float(loss.detach()) - l_ref) <= 1e-3 * abs(l_ref)
    _check_grad(name, z1.grad, g1, f"{name} split view 0")
    _check_grad(name, z2.grad, g2, f"{name} split view 1")


def test_training_under_autocast():
    """Thirty Adam steps of a two-encoder model under torch.autocast(bfloat16): the encoders' outputs are bfloat16, the loss float32,
    and it falls as in tests/test_gpu_loss.py::test_loss_drives_training_step."""
    import torch

    from cca_zoo_amd.deep.objectives import CCALoss

    torch.manual_seed(0)
    n = 1024
    zlat = torch.randn(n, 4)
    x1 = (zlat @ torch.randn(4, 20) + 0.5 * torch.randn(n, 20)).cuda()
    x2 = (zlat @ torch.randn(4, 16) + 0.5 * torch.randn(n, 16)).cuda()
    e1, e2 = torch.nn.Linear(20, 4).cuda(), torch.nn.Linear(16, 4).cuda()
    opt = torch.optim.Adam(list(e1.parameters()) + list(e2.parameters()), lr=1e-2)
    obj = CCALoss(eps=1e-4)
    first = None
    for _ in range(30):
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            a, b = e1(x1), e2(x2)
            assert a.dtype == torch.bfloat16
            loss = obj([a, b])
        assert loss.dtype == torch.float32
        loss.backward()
        opt.step()
        first = loss.item() if first is None else first
    assert loss.item() < first - 0.1


def test_batch_whiten_keeps_bfloat16():
    """A bfloat16 batch comes back as bfloat16, within one rounding (u = 2^-8, relative) of the float32 module on the exactly widened
    batch; 1e-5 of the largest entry covers the two float32 evaluations (the project's float32 bar is 1e-3)."""
    import torch

    from cca_zoo_amd.deep._dcca_noi import _BatchWhiten

    torch.manual_seed(1)
    x = (torch.randn(300, 12) @ torch.randn(12, 12) + 0.3).to(torch.bfloat16).cuda()
    half, full = _BatchWhiten(12).cuda().train(), _BatchWhiten(12).cuda().train()
    y, y32 = half(x), full(x.float())
    assert y.dtype == torch.bfloat16 and y32.dtype == torch.float32
    ref = y32.double()
    bound = U["bf16"] * ref.abs() + 1e-5 * ref.abs().max()
    assert bool(((y.double() - ref).abs() <= bound).all())
    assert torch.allclose(half.running_covar, full.running_covar, rtol=1e-5, atol=1e-6)


def test_other_dtypes_are_still_a_type_error():
    import torch

    from cca_zoo_amd.deep.objectives import CCALoss

    z = torch.zeros(8, 2, dtype=torch.int32, device="cuda")
    with pytest.raises(TypeError, match="float32, float64, bfloat16 or float16"):
        CCALoss()([z, z])
