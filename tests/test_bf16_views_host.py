"""Which estimators let bfloat16 device views through validation (CPU only).

``validate_views`` looks at a device tensor's ``is_cuda`` / ``dim`` / ``dtype`` / ``element_size`` alone, so a host tensor that says
it is on the device stands in for one: everything checked here happens before the device is touched.
"""

import pytest


def _device_like(n, d, dtype):
    import torch

    class OnDevice(torch.Tensor):
        @property
        def is_cuda(self):
            return True

    OnDevice.__module__ = "torch._stand_in"
    return torch.zeros((n, d), dtype=dtype).as_subclass(OnDevice)


def test_validate_views_flag():
    import torch

    from cca_zoo_amd._utils._validation import is_bf16_tensor, validate_views

    b, h, f = (_device_like(10, 3, t) for t in (torch.bfloat16, torch.float16, torch.float32))
    assert is_bf16_tensor(b) and not is_bf16_tensor(h) and not is_bf16_tensor(f)
    assert not is_bf16_tensor(torch.zeros((2, 2), dtype=torch.bfloat16))           # a host tensor
    out = validate_views([b, f], check_finite=False, allow_bf16=True)
    assert out[0] is b and out[1] is f
    with pytest.raises(ValueError, match="float32 or float64"):
        validate_views([b, b], check_finite=False)
    for flag in (False, True):
        with pytest.raises(ValueError, match="float32 or float64"):
            validate_views([h, h], check_finite=False, allow_bf16=flag)
    with pytest.raises(ValueError, match="Expected 2D"):
        validate_views([b[0], b[0]], allow_bf16=True)
    with pytest.raises(ValueError, match="same number of samples"):
        validate_views([b, _device_like(9, 3, torch.bfloat16)], allow_bf16=True)


def test_only_the_closed_form_family_sets_the_flag():
    from cca_zoo_amd import linear, nonparametric, probabilistic, tree

    yes = {"rCCA", "CCA", "PLS", "MCCA", "GCCA", "PartialCCA", "GRCCA"}
    seen = set()
    for mod in (linear, nonparametric, probabilistic, tree):
        for name in mod.__all__:
            cls = getattr(mod, name)
            if hasattr(cls, "_bf16_views"):
                assert cls._bf16_views == (name in yes), name
                seen.add(name)
    assert yes <= seen and len(seen) > len(yes)


def test_other_families_refuse_before_the_device_is_touched():
    import torch

    from cca_zoo_amd.linear import CCA_EY, CCAR3, PLS_ALS, SCCA_IPLS, TCCA
    from cca_zoo_amd.nonparametric import KCCA
    from cca_zoo_amd.probabilistic import GFA, ProbabilisticCCA, VariationalBayesCCA
    from cca_zoo_amd.tree import TreeCCA

    views = [_device_like(50, 6, torch.bfloat16), _device_like(50, 4, torch.bfloat16)]
    for est in (CCA_EY(), PLS_ALS(), SCCA_IPLS(), GFA(), VariationalBayesCCA(), ProbabilisticCCA(), KCCA(), TCCA(), CCAR3(), TreeCCA()):
        with pytest.raises(ValueError, match="float32 or float64"):
            est.fit(views)
