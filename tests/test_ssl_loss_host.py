"""CPU tests of the moment-map losses (EYLoss, BarlowTwinsLoss, VICRegLoss, SDLLoss): exports, constructor defaults,
statelessness, the validation order (everything that needs no device is checked before the device is touched), the NumPy closed
forms of tests/ssl_closed_form.py against the reference's float64 run in every ``ssl_*`` golden, and the ctypes table."""

import numpy as np
import pytest
import torch

from conftest import load_golden
from ssl_closed_form import CASES, TERM_KEYS, closed_form

NAMES = ("EYLoss", "BarlowTwinsLoss", "VICRegLoss", "SDLLoss")


def _rel(a, b):
    """Largest difference over the largest reference entry; the plain difference where the reference is exactly zero."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() or 1.0))


def test_exports():
    import cca_zoo_amd.deep as deep

    for name in NAMES:
        assert name in deep.__all__ and isinstance(getattr(deep, name), type)
        assert issubclass(getattr(deep, name), torch.nn.Module)


def test_constructor_defaults_and_statelessness():
    from cca_zoo_amd.deep import BarlowTwinsLoss, EYLoss, SDLLoss, VICRegLoss

    assert BarlowTwinsLoss().lam == 5e-3 and BarlowTwinsLoss(lam=0.1).lam == 0.1
    v = VICRegLoss()
    assert (v.sim_coeff, v.std_coeff, v.cov_coeff) == (25.0, 25.0, 1.0)
    v = VICRegLoss(1.0, 2.0, 3.0)
    assert (v.sim_coeff, v.std_coeff, v.cov_coeff) == (1.0, 2.0, 3.0)
    assert SDLLoss().lam == 0.5 and SDLLoss(lam=0.2).lam == 0.2
    for mod in (EYLoss(), BarlowTwinsLoss(), VICRegLoss(), SDLLoss()):
        assert list(mod.parameters()) == [] and list(mod.buffers()) == [] and len(mod.state_dict()) == 0
        assert callable(mod.terms)


def _views(k, n=8, d=3):
    return [torch.randn(n, d) for _ in range(k)]


@pytest.mark.parametrize("name", ["BarlowTwinsLoss", "VICRegLoss"])
@pytest.mark.parametrize("k", [1, 3])
def test_two_view_losses_want_exactly_two(name, k):
    import cca_zoo_amd.deep as deep

    mod = getattr(deep, name)()
    bad = _views(k)
    bad[0] = torch.randn(8)                         # the count is checked before the shapes
    with pytest.raises(ValueError, match=f"{name} expects exactly 2 representations, got {k}"):
        mod(bad)
    with pytest.raises(ValueError, match="exactly 2"):
        mod.terms(_views(k))


@pytest.mark.parametrize("name", ["EYLoss", "SDLLoss"])
@pytest.mark.parametrize("k", [1, 9])
def test_multi_view_losses_want_two_to_eight(name, k):
    import cca_zoo_amd.deep as deep

    with pytest.raises(ValueError, match=f"{name} expects 2 to 8 representations, got {k}"):
        getattr(deep, name)()(_views(k))


@pytest.mark.parametrize("name", NAMES)
def test_validation_order_and_messages(name):
    import cca_zoo_amd.deep as deep

    mod = getattr(deep, name)()
    # 2. every input is a (batch, d_i) tensor -- before the batch sizes are compared
    with pytest.raises(ValueError, match=rf"{name} expects \(batch, d_i\) tensors$"):
        mod([torch.randn(8, 3), torch.randn(7)])
    with pytest.raises(ValueError, match=rf"{name} expects \(batch, d_i\) tensors$"):
        mod([torch.randn(8, 3), np.zeros((8, 3))])
    # 3. equal batch size -- before the widths
    with pytest.raises(ValueError, match="equal batch size"):
        mod([torch.randn(8, 3), torch.randn(7, 4)])
    # 4. equal widths, named
    with pytest.raises(ValueError, match=r"same width, got widths \[3, 4\]"):
        mod([torch.randn(8, 3), torch.randn(8, 4)])
    # 6. the device and dtype checks come last
    with pytest.raises(RuntimeError, match="no CPU fallback$"):
        mod([torch.randn(8, 3), torch.randn(8, 3)])
    with pytest.raises(RuntimeError, match="no CPU fallback$"):
        mod.terms([torch.randn(8, 3), torch.randn(8, 3)])


def test_sdl_needs_two_columns_before_the_device_check():
    from cca_zoo_amd.deep import SDLLoss

    with pytest.raises(ValueError, match="SDLLoss needs at least 2 columns per view, got 1"):
        SDLLoss()([torch.randn(8, 1), torch.randn(8, 1)])
    with pytest.raises(ValueError, match="same width"):                      # the widths are compared first
        SDLLoss()([torch.randn(8, 1), torch.randn(8, 2)])


def test_ey_independent_batch_is_validated_like_the_batch():
    from cca_zoo_amd.deep import EYLoss

    zs = _views(2)
    with pytest.raises(ValueError, match="as many independent representations as representations"):
        EYLoss()(zs, _views(3, n=6))
    with pytest.raises(ValueError, match="equal batch size"):
        EYLoss()(zs, [torch.randn(6, 3), torch.randn(5, 3)])
    with pytest.raises(ValueError, match="same width"):
        EYLoss()(zs, _views(2, n=6, d=4))
    with pytest.raises(RuntimeError, match="no CPU fallback$"):
        EYLoss()(zs, _views(2, n=6))


@pytest.mark.parametrize("tag", CASES)
def test_closed_form_matches_the_reference(tag):
    kind, n, m, d, params = CASES[tag][:5]
    g = load_golden(f"ssl_{tag}")
    zs = [g[f"z{i}"] for i in range(m)]
    assert all(z.shape == (n, d) and z.dtype == np.float32 for z in zs)
    assert tuple(np.atleast_1d(g["params"])) == tuple(params)
    zi = [g[f"zi{i}"] for i in range(m)] if "zi0" in g else None
    assert (zi is not None) == (len(CASES[tag]) > 6)
    terms, grads, gi = closed_form(kind, zs, params, zi)
    errs = [_rel(terms["objective"], g["loss64"])]
    errs += [_rel(terms[k], g[f"{k}64"]) for k in TERM_KEYS[kind]]      # (one column per view: VICReg's cov_loss is exactly 0)
    errs += [_rel(grads[i], g[f"g64_{i}"]) for i in range(m)]
    if zi is not None:
        errs += [_rel(gi[i], g[f"gi64_{i}"]) for i in range(m)]
    assert max(errs) <= 1e-12, errs


def test_backend_declares_the_entry_points():
    from cca_zoo_amd import _backend

    assert {"ccz_moment_loss_state_bytes", "ccz_moment_loss_forward"} <= set(_backend.SIGNATURES)
    res, args = _backend.SIGNATURES["ccz_moment_loss_forward"]
    assert len(args) == 13
