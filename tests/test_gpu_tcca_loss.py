"""GPU parity of TCCALoss against goldens captured from the reference (tools/gen_golden_tcca.py): loss and gradients within
1e-6 of the reference's float64 run for float64 AND float32 inputs (the device computes in float64 on the stored float32
values), and for float32 inputs no further from the reference's own float32 run than twice its float32-to-float64 gap."""

import numpy as np
import pytest
import torch

from conftest import load_golden
from tcca_closed_form import CASES

pytestmark = pytest.mark.gpu

TOL = 1e-6


def _load(tag):
    g = load_golden(f"tcca_{tag}")
    nv = sum(k.startswith("z") for k in g)
    return g, [g[f"z{i}"] for i in range(nv)]


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _run(zs32, eps, dtype, upstream=1.0, detach=()):
    from cca_zoo_amd.deep import TCCALoss

    zs = [torch.tensor(z, dtype=dtype, device="cuda", requires_grad=i not in detach) for i, z in enumerate(zs32)]
    loss = TCCALoss(eps=eps)(zs)
    (upstream * loss).backward()
    return loss, zs


@pytest.mark.parametrize("tag", CASES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_tcca_loss_matches_reference(tag, dtype):
    g, zs32 = _load(tag)
    loss, zs = _run(zs32, float(g["eps"]), dtype)
    assert loss.dim() == 0 and loss.dtype == dtype and loss.device == zs[0].device
    # float32 outputs are the float64 results rounded once: half an ulp (6e-8) inside the 1e-6
    errs = [_rel(loss.detach().cpu().numpy(), g["loss64"])]
    for i, z in enumerate(zs):
        assert z.grad.dtype == dtype and z.grad.shape == z.shape
        errs.append(_rel(z.grad.cpu().numpy(), g[f"g64_{i}"]))
    print(f"tcca_{tag} {dtype}: worst relative distance to the float64 reference {max(errs):.2e}")
    assert max(errs) <= TOL, errs
    if dtype == torch.float32:
        # one figure per golden on either side: the worst relative distance over the loss and all gradients
        gap = max([_rel(g["loss32"], g["loss64"])] + [_rel(g[f"g32_{i}"], g[f"g64_{i}"]) for i in range(len(zs))])
        ours = max([_rel(loss.detach().cpu().numpy(), g["loss32"])] + [_rel(z.grad.cpu().numpy(), g[f"g32_{i}"]) for i, z in enumerate(zs)])
        print(f"tcca_{tag} float32: distance to the float32 reference {ours:.2e}, its own float32-to-float64 gap {gap:.2e}")
        assert ours <= 2.0 * gap, (ours, gap)


def test_upstream_factor_no_grad_and_detached_view():
    from cca_zoo_amd.deep import TCCALoss

    g, zs32 = _load("three")
    eps = float(g["eps"])
    _, base = _run(zs32, eps, torch.float64)
    _, tripled = _run(zs32, eps, torch.float64, upstream=3.0)
    for a, b in zip(base, tripled):
        np.testing.assert_allclose(b.grad.cpu().numpy(), 3.0 * a.grad.cpu().numpy(), rtol=1e-14, atol=0)
    with torch.no_grad():
        val = TCCALoss(eps=eps)([z.detach() for z in base])
    assert not val.requires_grad
    assert float(val) == pytest.approx(float(g["loss64"]), rel=TOL)
    loss, part = _run(zs32, eps, torch.float64, detach=(1,))
    assert part[1].grad is None
    assert torch.equal(part[0].grad, base[0].grad) and torch.equal(part[2].grad, base[2].grad)


def test_strided_input_is_accepted():
    from cca_zoo_amd.deep import TCCALoss

    g, zs32 = _load("four")
    wide = torch.zeros((zs32[1].shape[0], 7), dtype=torch.float64, device="cuda")
    wide[:, 2:2 + zs32[1].shape[1]] = torch.tensor(zs32[1], dtype=torch.float64)
    wide.requires_grad_(True)
    zs = [torch.tensor(z, dtype=torch.float64, device="cuda", requires_grad=True) for z in zs32]
    zs[1] = wide[:, 2:2 + zs32[1].shape[1]]
    assert not zs[1].is_contiguous()
    loss = TCCALoss(eps=float(g["eps"]))(zs)
    loss.backward()
    assert _rel(loss.detach().cpu().numpy(), g["loss64"]) <= TOL
    got = wide.grad.cpu().numpy()
    assert _rel(got[:, 2:2 + zs32[1].shape[1]], g["g64_1"]) <= TOL
    assert not got[:, :2].any() and not got[:, 2 + zs32[1].shape[1]:].any()
    assert _rel(zs[0].grad.cpu().numpy(), g["g64_0"]) <= TOL


def test_tall_twice_gives_the_same_bits():
    g, zs32 = _load("tall")
    la, za = _run(zs32, float(g["eps"]), torch.float32)
    lb, zb = _run(zs32, float(g["eps"]), torch.float32)
    assert torch.equal(la, lb)
    for a, b in zip(za, zb):
        assert torch.equal(a.grad, b.grad)


def test_zero_moment_tensor_gives_zero_gradients():
    from cca_zoo_amd.deep import TCCALoss

    # a constant view (mean exactly 1, so Z_c = H = 0 exactly) makes M exactly zero: torch's subgradient of the norm there is 0
    torch.manual_seed(0)
    zs = [torch.randn(32, 3, dtype=torch.float64), torch.ones(32, 2, dtype=torch.float64), torch.randn(32, 2, dtype=torch.float64)]
    zs = [z.cuda().requires_grad_(True) for z in zs]
    loss = TCCALoss()(zs)
    loss.backward()
    assert float(loss.detach()) == 0.0
    for z in zs:
        assert torch.isfinite(z.grad).all() and not z.grad.any()
