"""The latent residual summary without a device: the numpy model of tests/latent_model.py against scipy, what the statistics
say about calibrated and miscalibrated latents, the argument checks of the two new ABI entry points, and the fitter's signatures."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch
from scipy import stats

import latent_model as LM
from cases import make_case


@pytest.mark.parametrize("D", range(1, 17))
def test_model_chi2_cdf_matches_scipy(D):
    r2 = np.concatenate([[0.0, 1e-6, 1e-3, 200.0], np.random.default_rng(100 + D).chisquare(D, size=2000)])
    err = np.abs(LM.chi2_cdf(r2, D) - stats.chi2.cdf(r2, D)).max()
    assert err < 1e-13, (D, err)
    assert np.all(LM.chi2_cdf(np.array([1e5, 1e30, 6e77]), D) == 1.0)   # past the guard: exactly 1, nothing overflows


def test_model_normal_cdf_matches_scipy():
    z = np.concatenate([np.linspace(-12, 12, 4801), np.random.default_rng(3).standard_normal(4000)])
    ref = stats.norm.cdf(z)
    assert np.abs(LM.norm_cdf(z) - ref).max() < 1e-15
    lower = z < 0                                                       # the lower tail keeps its relative accuracy
    assert np.abs(LM.norm_cdf(z[lower]) / ref[lower] - 1).max() < 1e-12
    assert LM.norm_cdf(12.0) == 1.0 and LM.bins_of(LM.norm_cdf(12.0), 100) == 99 and LM.bins_of(0.0, 100) == 0


@pytest.mark.parametrize("D", [1, 5, 16])
def test_model_separates_calibrated_from_miscalibrated_latents(D):
    z = np.random.default_rng(7).standard_normal((4096, D)).astype(np.float32)
    good = LM.latent_summary(z, 100)
    print(D, "calibrated", good["radial_ks"], good["ks"].max(), "halved", LM.latent_summary(z * np.float32(0.5), 100)["radial_ks"],
          "x1.2", LM.latent_summary(z * np.float32(1.2), 100)["radial_ks"])
    assert good["n"] == 4096 and good["n_bad"] == 0
    assert good["radial_ks"] < 0.03 and good["ks"].max() < 0.03
    assert LM.latent_summary(z * np.float32(0.5), 100)["radial_ks"] > 0.3
    assert LM.latent_summary(z * np.float32(1.2), 100)["radial_ks"] > 0.08
    assert np.abs(good["mean"]).max() < 0.08 and np.abs(good["cov"] - np.eye(D)).max() < 0.1
    assert good["pit_counts"].sum(1).tolist() == [4096] * D and good["radial_counts"].sum() == 4096
    assert good["ecp"][0] == 0.0 and good["ecp"][-1] == 1.0 and len(good["alpha"]) == 101


def test_model_skips_rows_that_are_not_finite():
    z = np.random.default_rng(1).standard_normal((50, 3)).astype(np.float32)
    z[4, 1] = np.nan
    z[9, 0] = np.inf
    z[10] = 0.0
    r = LM.raw_sums(z, 7)
    assert (r["n"], r["n_bad"]) == (48, 2) and r["radial_counts"].sum() == 48 and r["radial_counts"][0] >= 1
    keep = np.delete(z, [4, 9], 0).astype(np.float64)
    assert np.allclose(r["psum"][1], (keep ** 2).sum(0), rtol=1e-14) and np.allclose(r["cross"], keep.T @ keep, rtol=1e-13)


def test_abi_refuses_bad_arguments(lib):
    d = C.c_void_p(4096)                                               # never dereferenced: the checks come first
    for D, nb, N in ((0, 10, 8), (17, 10, 8), (4, 0, 8), (4, 1025, 8), (4, 10, -1)):
        assert lib.sf_latent_summary(d, N, D, nb, d, d, d, d, d, None) == -1, (D, nb, N)      # SF_ERR_INVALID
        assert lib.sf_last_error().startswith(b"sf_latent_summary:"), lib.sf_last_error()
    assert lib.sf_latent_summary(None, 8, 4, 10, d, d, d, d, d, None) == -1
    assert lib.sf_last_error().startswith(b"sf_latent_summary:")
    assert lib.sf_flow_to_noise(None, d, d, 8, d, d, None) == -1
    assert lib.sf_last_error().startswith(b"sf_flow_to_noise:")


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_new_entry_points_fail_loudly_without_a_gpu(lib):
    from synference_amd.engine import HipFlow
    d = C.c_void_p(4096)
    assert lib.sf_latent_summary(d, 8, 4, 10, d, d, d, d, d, None) == -3                       # SF_ERR_NO_DEVICE
    assert lib.sf_last_error().startswith(b"sf_latent_summary: no usable device: "), lib.sf_last_error()
    ospec, spec, flat, theta, x = make_case("maf_small", B=4)
    f = HipFlow(spec)
    assert lib.sf_flow_to_noise(f.handle, d, d, 4, d, d, None) == -3
    assert b"no CPU fallback" in lib.sf_last_error()
    with pytest.raises(RuntimeError, match="no GPU|fallback"):
        f.to_noise(theta, x)


def test_signatures():
    from synference_amd.engine import HipFlow
    from synference_amd.estimator import FlowEstimator
    from synference_amd.features import latent_summary
    from synference_amd.fitter import SBI_Fitter
    from synference_amd.posterior import EnsemblePosterior, FlowPosterior
    sig = inspect.signature(SBI_Fitter.calculate_latent_residuals)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [
        ("X", None), ("y", None), ("posteriors", None), ("num_bins", 100), ("return_latents", False)]
    ev = inspect.signature(SBI_Fitter.evaluate_model).parameters
    assert ev["latent"].default is False and list(ev).index("latent") == list(ev).index("tarp") + 1
    assert list(inspect.signature(latent_summary).parameters.items())[1][1].default == 100
    for cls, name in ((HipFlow, "to_noise"), (FlowEstimator, "transform_to_noise"), (FlowPosterior, "to_noise_catalogue"),
                      (EnsemblePosterior, "to_noise_catalogue")):
        assert callable(getattr(cls, name))
    assert "no latent space of its own" in " ".join(EnsemblePosterior.to_noise_catalogue.__doc__.split())
    with pytest.raises(RuntimeError, match="runs on the GPU"):
        latent_summary(torch.zeros(8, 2))
