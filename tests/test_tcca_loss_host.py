"""CPU tests of TCCALoss: exports, constructor, validation before the device is touched, and the NumPy closed form
(tests/tcca_closed_form.py -- the specification of the device node) against the reference's float64 autograd in every
``tcca_*`` golden."""

import numpy as np
import pytest
import torch

from conftest import load_golden
from tcca_closed_form import CASES, tcca_loss_closed_form


def test_tcca_loss_is_exported():
    import cca_zoo_amd.deep as deep
    from cca_zoo_amd.deep import TCCALoss
    from cca_zoo_amd.deep.objectives import TCCALoss as T2

    assert TCCALoss is T2
    assert "TCCALoss" in deep.__all__


def test_constructor_and_eps_round_trip():
    from cca_zoo_amd.deep import TCCALoss

    assert TCCALoss().eps == 1e-5
    assert TCCALoss(eps=1e-3).eps == 1e-3
    assert isinstance(TCCALoss(), torch.nn.Module)
    assert list(TCCALoss().parameters()) == [] and list(TCCALoss().buffers()) == []      # stateless


def test_validation_fires_before_the_device_is_touched():
    from cca_zoo_amd.deep import TCCALoss

    loss = TCCALoss()
    with pytest.raises(ValueError, match="2 to 8"):
        loss([torch.randn(8, 2)])
    with pytest.raises(ValueError, match="2 to 8"):
        loss([])
    with pytest.raises(ValueError, match="2 to 8"):
        loss([torch.randn(8, 2) for _ in range(9)])
    with pytest.raises(ValueError, match=r"\(batch, d_i\)"):
        loss([torch.randn(8, 2), torch.randn(8)])
    with pytest.raises(ValueError, match=r"\(batch, d_i\)"):
        loss([torch.randn(8, 2, 2), torch.randn(8, 2)])
    with pytest.raises(ValueError, match="equal batch size"):
        loss([torch.randn(8, 2), torch.randn(7, 2)])
    with pytest.raises(ValueError, match="2\\^24"):
        loss([torch.randn(4, 4096), torch.randn(4, 4096), torch.randn(4, 2)])       # 2^25 entries
    loss_ok = [torch.randn(4, 4096), torch.randn(4, 4096)]                         # exactly 2^24: passes validation
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss(loss_ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss([torch.randn(8, 2), torch.randn(8, 3), torch.randn(8, 2)])


@pytest.mark.parametrize("tag", CASES)
def test_closed_form_matches_the_reference_float64(tag):
    g = load_golden(f"tcca_{tag}")
    zs = [g[f"z{i}"] for i in range(sum(k.startswith("z") for k in g))]
    assert all(z.dtype == np.float32 for z in zs)
    loss, grads = tcca_loss_closed_form(zs, float(g["eps"]))
    assert abs(loss - float(g["loss64"])) <= 1e-10 * abs(float(g["loss64"]))
    for i, gr in enumerate(grads):
        ref = g[f"g64_{i}"]
        assert ref.dtype == np.float64 and g[f"g32_{i}"].dtype == np.float32
        assert np.abs(gr - ref).max() <= 1e-10 * np.abs(ref).max()
