"""GPU parity of EYLoss, BarlowTwinsLoss, VICRegLoss and SDLLoss against goldens captured from the reference
(tools/gen_golden_ssl.py): the objective, every term and every gradient against the reference's float64 run, with the measure of
test_gpu_tcca_loss.py and the project's own bars (test_gpu_loss.py): 1e-6 for float64 inputs, 1e-3 for float32 inputs.

Measured on an MI355X (worst distance over all cases of a loss; float64 inputs / float32 inputs): see DESIGN.md 4j."""

import numpy as np
import pytest
import torch

from conftest import load_golden
from ssl_closed_form import CASES, TERM_KEYS

pytestmark = pytest.mark.gpu

TOL = {torch.float64: 1e-6, torch.float32: 1e-3}


def _rel(a, b):
    """The measure of test_gpu_tcca_loss.py; the plain difference where the reference is exactly zero (VICReg's cov_loss with one
    column per view)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() or 1.0))


def _module(kind, params):
    from cca_zoo_amd import deep

    if kind == "ey":
        return deep.EYLoss()
    if kind == "barlow":
        return deep.BarlowTwinsLoss(lam=params[0])
    if kind == "vicreg":
        return deep.VICRegLoss(*params)
    return deep.SDLLoss(lam=params[0])


_GOLDEN = {}


def _load(tag):
    """(golden, module, float32 views, float32 independent views or None); read once, never written to."""
    if tag not in _GOLDEN:
        kind, _, m, _, params = CASES[tag][:5]
        g = load_golden(f"ssl_{tag}")
        zi = [g[f"zi{i}"] for i in range(m)] if "zi0" in g else None
        _GOLDEN[tag] = (g, kind, params, [g[f"z{i}"] for i in range(m)], zi)
    g, kind, params, zs, zi = _GOLDEN[tag]
    return g, kind, _module(kind, params), zs, zi


def _leaves(arrays, dtype, detach=()):
    return [torch.tensor(z, dtype=dtype, device="cuda", requires_grad=i not in detach) for i, z in enumerate(arrays)]


def _run(tag, dtype, upstream=1.0, detach=(), detach_ind=()):
    g, kind, mod, zs32, zi32 = _load(tag)
    zs = _leaves(zs32, dtype, detach)
    zi = _leaves(zi32, dtype, detach_ind) if zi32 is not None else None
    loss = mod(zs, zi) if zi is not None else mod(zs)
    (upstream * loss).backward()
    return loss, zs, zi


@pytest.mark.parametrize("tag", CASES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_matches_reference(tag, dtype):
    g, kind, mod, _, _ = _load(tag)
    loss, zs, zi = _run(tag, dtype)
    assert loss.dim() == 0 and loss.dtype == dtype and loss.device == zs[0].device
    terms = mod.terms([z.detach() for z in zs], [z.detach() for z in zi]) if zi is not None else mod.terms([z.detach() for z in zs])
    assert tuple(terms) == ("objective",) + TERM_KEYS[kind]
    for v in terms.values():
        assert v.dim() == 0 and v.dtype == dtype and not v.requires_grad and v.device == zs[0].device
    # (a second device pass: K1 sums its row chunks in arrival order, so the two objectives may differ in the last bits)
    errs = {"objective": _rel(loss.detach().cpu().numpy(), g["loss64"]), "terms.objective": _rel(terms["objective"].cpu().numpy(), g["loss64"])}
    for k in TERM_KEYS[kind]:
        errs[k] = _rel(terms[k].cpu().numpy(), g[f"{k}64"])
    for i, z in enumerate(zs):
        assert z.grad.dtype == dtype and z.grad.shape == z.shape
        errs[f"g{i}"] = _rel(z.grad.cpu().numpy(), g[f"g64_{i}"])
    for i, z in enumerate(zi or []):
        assert z.grad.dtype == dtype and z.grad.shape == z.shape
        errs[f"gi{i}"] = _rel(z.grad.cpu().numpy(), g[f"gi64_{i}"])
    worst = max(errs, key=errs.get)
    print(f"ssl_{tag} [{kind}] {dtype}: worst relative distance to the float64 reference {errs[worst]:.2e} ({worst})")
    assert errs[worst] <= TOL[dtype], errs


@pytest.mark.parametrize("tag,key", [("vic_cancel", "sim_loss"), ("sdl_cancel", "l2")])
def test_cancellation_value_in_float32(tag, key):
    """z_2 = z_1 + 1e-3 noise: the value of mean((z_1 - z_2)^2) in float32 stays within 4x the reference's own float32-to-float64
    gap (the factor: the orders of summation differ) -- it is summed from the differences, not from the Gram."""
    g, _, mod, zs32, _ = _load(tag)
    terms = mod.terms(_leaves(zs32, torch.float32))
    ours = _rel(terms[key].cpu().numpy(), g[f"{key}64"])
    gap = _rel(g[f"{key}32"], g[f"{key}64"])
    print(f"ssl_{tag} float32 {key}: distance to the float64 reference {ours:.2e}, the reference's own float32-to-float64 gap {gap:.2e}")
    assert ours <= 4.0 * gap, (ours, gap)


@pytest.mark.parametrize("tag", ["ey_three", "bt_offset", "vic_offset", "sdl_three"])
def test_upstream_factor_no_grad_and_detached_view(tag):
    g, _, mod, zs32, _ = _load(tag)
    _, base, _ = _run(tag, torch.float64)
    _, tripled, _ = _run(tag, torch.float64, upstream=3.0)
    for a, b in zip(base, tripled):
        # the factor is applied to Gamma on the device (one rounding of 3 Gamma per entry), not to the finished gradient
        assert float((b.grad - 3.0 * a.grad).abs().max()) <= 1e-14 * 3.0 * float(a.grad.abs().max())
    with torch.no_grad():
        val = mod([z.detach() for z in base])
    assert not val.requires_grad
    assert float(val) == pytest.approx(float(g["loss64"]), rel=TOL[torch.float64])
    _, part, _ = _run(tag, torch.float64, detach=(1,))
    assert part[1].grad is None
    for i in range(len(base)):
        if i != 1:
            assert torch.equal(part[i].grad, base[i].grad)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_strided_input_is_accepted(dtype):
    """A view cut out of a wider tensor: odd leading dimension, rows that are not 16-byte aligned (the scalar form of the
    squared-difference kernel)."""
    g, _, mod, zs32, _ = _load("vic_small")
    d = zs32[1].shape[1]
    wide = torch.zeros((zs32[1].shape[0], d + 5), dtype=dtype, device="cuda")
    wide[:, 2:2 + d] = torch.tensor(zs32[1], dtype=dtype)
    wide.requires_grad_(True)
    zs = _leaves(zs32, dtype)
    zs[1] = wide[:, 2:2 + d]
    assert not zs[1].is_contiguous()
    loss = mod(zs)
    loss.backward()
    assert _rel(loss.detach().cpu().numpy(), g["loss64"]) <= TOL[dtype]
    got = wide.grad.cpu().numpy()
    assert _rel(got[:, 2:2 + d], g["g64_1"]) <= TOL[dtype]
    assert not got[:, :2].any() and not got[:, 2 + d:].any()
    assert _rel(zs[0].grad.cpu().numpy(), g["g64_0"]) <= TOL[dtype]
    sim = mod.terms([z.detach() for z in zs])["sim_loss"]
    assert _rel(sim.cpu().numpy(), g["sim_loss64"]) <= TOL[dtype]


def test_ey_independent_batch_gradients_flow_into_either_list():
    g, _, mod, _, _ = _load("ey_ind")
    _, zs, zi = _run("ey_ind", torch.float64)
    _, zs_a, zi_a = _run("ey_ind", torch.float64, detach_ind=(0, 1))           # only the batch wants gradients
    assert all(z.grad is None for z in zi_a)
    assert all(torch.equal(a.grad, b.grad) for a, b in zip(zs_a, zs))
    _, zs_b, zi_b = _run("ey_ind", torch.float64, detach=(0, 1))               # only the independent batch does
    assert all(z.grad is None for z in zs_b)
    assert all(torch.equal(a.grad, b.grad) for a, b in zip(zi_b, zi))
    for i, z in enumerate(zi):
        assert _rel(z.grad.cpu().numpy(), g[f"gi64_{i}"]) <= TOL[torch.float64]


def test_mixed_dtypes_follow_the_first_view():
    g, _, mod, zs32, _ = _load("bt_small")
    zs = [torch.tensor(zs32[0], dtype=torch.float64, device="cuda", requires_grad=True),
          torch.tensor(zs32[1], dtype=torch.float32, device="cuda", requires_grad=True)]
    loss = mod(zs)
    loss.backward()
    assert loss.dtype == torch.float64 and zs[0].grad.dtype == torch.float64 and zs[1].grad.dtype == torch.float32
    assert _rel(loss.detach().cpu().numpy(), g["loss64"]) <= TOL[torch.float64]
    assert _rel(zs[1].grad.cpu().numpy(), g["g64_1"]) <= TOL[torch.float32]


def test_successive_calls_with_different_shapes_on_one_handle():
    """Pooled scratch and the handle's K1 plans are reused across shapes: a shape met again gives the reference's values again."""
    for tag in ("ey_four17", "bt_small", "vic_tall", "ey_four17", "sdl_three", "vic_tall", "bt_small"):
        g = _load(tag)[0]
        loss, zs, _ = _run(tag, torch.float32)
        errs = [_rel(loss.detach().cpu().numpy(), g["loss64"])] + [_rel(z.grad.cpu().numpy(), g[f"g64_{i}"]) for i, z in enumerate(zs)]
        assert max(errs) <= TOL[torch.float32], (tag, errs)


# ---- shapes without a golden: a float64 restatement of the four losses in torch, differentiated by autograd on the device ----
def _cov(z):
    c = z - z.mean(dim=0)
    return c.T @ c / (z.shape[0] - 1)


def _restated(kind, params, zs):
    n, d = zs[0].shape
    off = ~torch.eye(d, dtype=torch.bool, device=zs[0].device)
    if kind == "ey":
        V = sum(_cov(z) for z in zs) / len(zs)
        total = sum(z - z.mean(dim=0) for z in zs)
        return -2.0 * (total * total).sum() / (len(zs) * (n - 1)) + (V * V).sum()
    if kind == "barlow":
        C = zs[0].T @ zs[1] / n
        return ((1.0 - torch.diagonal(C)) ** 2).sum() + params[0] * (C[off] ** 2).sum()
    sq = ((zs[0] - zs[1]) ** 2).mean()
    if kind == "vicreg":
        var = sum(torch.relu(1.0 - torch.sqrt(torch.diagonal(_cov(z)) + 1e-4)).mean() for z in zs)
        cov = sum((_cov(z)[off] ** 2).sum() / d for z in zs)
        return params[0] * sq + params[1] * var + params[2] * cov
    return sq + params[0] * sum(_cov(z)[off].abs().mean() for z in zs)


def _wide_pair(n, d, seed):
    """Two correlated float32 views with column spreads on both sides of 1 and column offsets of order 1 (Gamma_r and the centring
    row both matter)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    base = torch.randn(n, d, generator=gen)
    scale = 0.7 + 0.8 * (torch.arange(d) % 2)
    z1 = base * scale + torch.rand(d, generator=gen) * 3.0 - 1.5
    z2 = (0.8 * base + 0.6 * torch.randn(n, d, generator=gen)) * scale.flip(0) + torch.rand(d, generator=gen) * 3.0 - 1.5
    return z1.float().cuda(), z2.float().cuda()


def _check_against_restatement(kind, params, z1, z2):
    mod = _module(kind, params)
    zs = [z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)]
    loss = mod(zs)
    loss.backward()
    ref_in = [z.detach().double().requires_grad_(True) for z in zs]
    ref = _restated(kind, params, ref_in)
    ref.backward()
    errs = [_rel(loss.detach().cpu().numpy(), ref.detach().cpu().numpy())]
    errs += [_rel(z.grad.cpu().numpy(), r.grad.cpu().numpy()) for z, r in zip(zs, ref_in)]
    return errs


@pytest.mark.parametrize("kind,params", [("ey", ()), ("barlow", (5e-3,)), ("vicreg", (25.0, 25.0, 1.0)), ("sdl", (0.5,))])
def test_large_shape_float32(kind, params):
    """2 views of 1024 x 256 in float32 with offset columns: 8 x 8 tiles of Gamma, the vector form of the squared-difference kernel
    and the two-view fp32 product of the backward that reads the views where they lie."""
    errs = _check_against_restatement(kind, params, *_wide_pair(1024, 256, 11))
    print(f"{kind} 2 x (1024 x 256) float32: worst relative distance to the float64 restatement {max(errs):.2e}")
    assert max(errs) <= TOL[torch.float32], errs


@pytest.mark.parametrize("kind,params", [("barlow", (5e-3,)), ("vicreg", (25.0, 25.0, 1.0))])
def test_offset_inputs_on_the_split_backward(kind, params, monkeypatch):
    """The split-bf16 backward shifts the rows by fl32(mean) and subtracts the state's fourth row: with Gamma_r != 0 and
    mean != 0 that row has to reproduce the centring row mean' Gamma_c exactly (csrc/ssl_loss.hip)."""
    from cca_zoo_amd import _backend

    monkeypatch.setenv("CCZ_LOSS_BWD_SPLIT", "2")
    monkeypatch.setenv("CCZ_SPLIT_MIN_FLOP", "1e9")
    z1, z2 = _wide_pair(4096, 256, 12)
    errs = _check_against_restatement(kind, params, z1, z2)
    torch.cuda.synchronize()
    assert _backend.handle_for([z1]).loss_last_route()[1] == "bf16x2"
    print(f"{kind} 2 x (4096 x 256) float32, split backward: worst relative distance to the float64 restatement {max(errs):.2e}")
    assert max(errs) <= TOL[torch.float32], errs
