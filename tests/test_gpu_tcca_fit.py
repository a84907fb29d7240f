"""GPU tests of the estimators ``TCCA`` / ``KTCCA``: every ``tccafit_*`` golden (tools/gen_golden_tcca_fit.py: the
reference's whitening, tensor and weight mapping around the written-out CP-ALS) with host arrays and with CUDA tensors.

Bars.  Float64 views: 1e-8 per column of ``weights_`` after sign alignment, the project's standing device bar; the
goldens' admission checks bound the growth of an init error to a factor of 100, which leaves the device's init and tensor
(1e-12) four orders of room.  Float32 views: ``n_iter_`` equals the float64 run's and every column is within twice the
case's stored ``gap32``, the reference's own float32-to-float64 gap.  The product over the views of the alignment signs is
+1 for every column: the rank-one terms agree, not only the columns.  KTCCA's ``transform`` of held-out rows is held to
what those bars imply for the product ``K' w`` (see the comment there)."""

import numpy as np
import pytest

from conftest import load_golden
from tcca_fit_restatement import align_signs, pairwise_kernel
from test_tcca_fit_host import CASES, F32, KCASES, golden_case

pytestmark = pytest.mark.gpu

BAR = 1e-8


def _fit(tag, device):
    from cca_zoo_amd.linear import TCCA
    from cca_zoo_amd.nonparametric import KTCCA

    g = load_golden(f"tccafit_{tag}")
    m = sum(k.startswith("x") for k in g)
    views = [g[f"x{i}"] for i in range(m)]
    held = [g[f"t{i}"] for i in range(m)] if tag in KCASES else None
    if device:
        import torch

        views = [torch.as_tensor(v, device="cuda") for v in views]
        held = [torch.as_tensor(v, device="cuda") for v in held] if held else None
    model = (KTCCA(latent_dimensions=int(g["k"]), **KCASES[tag]) if tag in KCASES else TCCA(latent_dimensions=int(g["k"]), **CASES[tag]))
    return g, m, views, held, model.fit(views)


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


@pytest.mark.parametrize("device", [False, True], ids=["ndarray", "cuda"])
@pytest.mark.parametrize("tag", list(CASES) + list(KCASES))
def test_golden(tag, device):
    g, m, views, held, model = _fit(tag, device)
    k = int(g["k"])
    bars = 2.0 * g["gap32"] if tag in F32 else np.full((m, k), BAR)
    signs, errs = [], []
    for i in range(m):
        w, ref = model.weights_[i], g[f"w{i}"]
        assert w.shape == ref.shape and w.dtype == np.float64
        s = align_signs(w, ref)
        signs.append(s)
        errs.append(np.linalg.norm(w * s - ref, axis=0) / np.linalg.norm(ref, axis=0))
    errs = np.stack(errs)
    print(tag, "cuda" if device else "ndarray", "n_iter", model.n_iter_, int(g["n_iter"]), "worst", errs.max(), "worst / bar", (errs / bars).max())
    assert model.n_iter_ == int(g["n_iter"])
    assert np.all(errs <= bars), (errs, bars)
    assert np.all(np.prod(np.stack(signs), axis=0) == 1.0)
    assert model.rec_error_.shape == (model.n_iter_,)
    if tag not in F32:
        assert np.abs(model.rec_error_ - g["trace"]).max() <= BAR
    if held is not None:
        # z = K(train, held)' w: a weight error of bar * |w_c| moves column c by at most bar * |K|_2 * |w_c|, and the kernel
        # matrix's own rounding (a d-term distance or product, the kernel function, an n-term sum: 64 ulp allowed) adds
        # 64 eps * |K|_2 * |w_c|.  Relative to |z_c| itself this can be large: the leading rbf column of a held-out
        # projection nearly cancels (|z_c| = 3e-9 against |K|_2 |w_c| = 3 in k_rbf), in the golden as on the device.
        fit = golden_case(tag)[2]
        zs = model.transform(held)
        for i, z in enumerate(zs):
            z, ref, w = _host(z), g[f"z{i}"], g[f"w{i}"]
            assert z.shape == ref.shape
            K = pairwise_kernel(fit["train"][i], g[f"t{i}"].astype(np.float64), *fit["kernel_args"][i])
            scale = np.linalg.norm(K, 2) * np.linalg.norm(w, axis=0)
            ez = np.linalg.norm(z * signs[i] - ref, axis=0) / scale
            print(tag, "transform view", i, "error / (|K| |w_c|)", ez, "bar", bars[i] + 64 * np.finfo(float).eps)
            assert np.all(ez <= bars[i] + 64 * np.finfo(float).eps), (ez, bars[i])
    score = _host(model.score(views))
    assert score.shape == (k,) and np.all(np.isfinite(score))
    zs = model.transform(views)
    assert len(zs) == m and all(tuple(z.shape) == (views[0].shape[0], k) for z in zs)


def test_tcca_means_dtypes_and_extras():
    from cca_zoo_amd.linear import TCCA

    g = load_golden("tccafit_f32_three")
    views = [g[f"x{i}"] for i in range(3)]
    model = TCCA(latent_dimensions=2).fit(views)
    assert all(mu.dtype == np.float32 for mu in model.means_) and all(w.dtype == np.float64 for w in model.weights_)
    for mu, v in zip(model.means_, views):
        assert np.abs(mu - v.mean(axis=0)).max() <= 1e-6
    assert model.n_views_ == 3 and model.n_features_in_ == [6, 5, 4] and model.n_samples_ == 500
    nc = TCCA(latent_dimensions=2, center=False).fit([v.astype(np.float64) for v in views])
    assert all(np.all(mu == 0) for mu in nc.means_)


def test_random_state_is_unused_and_two_fits_agree():
    """The decomposition has no random step.  Two fits still differ in the last bits: K1 adds its row-split partial Grams
    with atomics, so the covariances do (a few ulp; the CP-ALS behind them is bit-reproducible, tests/test_gpu_cp_als.py).
    The admission checks bound the growth of such a difference to a factor of 100: 1e-10 per column is six orders above it."""
    from cca_zoo_amd.linear import TCCA

    g = load_golden("tccafit_three17")
    views = [g[f"x{i}"] for i in range(3)]
    a = TCCA(latent_dimensions=4, c=[0.0, 0.2, 0.05]).fit(views)
    b = TCCA(latent_dimensions=4, c=[0.0, 0.2, 0.05], random_state=7).fit(views)
    assert a.n_iter_ == b.n_iter_
    for x, y in zip(a.weights_, b.weights_):
        assert (np.linalg.norm(x - y, axis=0) / np.linalg.norm(y, axis=0)).max() <= 1e-10


def test_mixed_host_and_device_views_are_refused():
    import torch

    from cca_zoo_amd.linear import TCCA

    g = load_golden("tccafit_three")
    views = [g["x0"], torch.as_tensor(g["x1"], device="cuda"), g["x2"]]
    with pytest.raises(ValueError):
        TCCA(latent_dimensions=2).fit(views)
