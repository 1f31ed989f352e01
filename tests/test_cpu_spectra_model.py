"""tests/spectra_model.py against answers that do not come from it, the condition on the shared cases, the tolerance of the
device comparison, and the host half of the spectra path (argument checks, coefficient tables) -- no device needed."""
from pathlib import Path

import numpy as np
import pytest
from scipy.ndimage import gaussian_filter1d

import spectra_cases as SC
import spectra_model as SM


# ---- convolution -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.5, 1.5, 2.0, 3.25])
def test_convolution_equals_scipy_for_a_constant_sigma(sigma):
    f = np.random.default_rng(1).uniform(1.0, 5.0, 97)
    assert int(np.ceil(4.0 * sigma)) == int(4.0 * sigma + 0.5)      # scipy's radius: the same taps
    got = SM.convolve(f, np.full(97, sigma))
    ref = gaussian_filter1d(f, sigma, mode="nearest", truncate=4.0)
    assert np.abs(got - ref).max() < 1e-12


def test_convolution_keeps_a_constant_and_copies_below_the_threshold():
    sg = np.random.default_rng(2).uniform(0.02, 6.0, 50)
    assert np.abs(SM.convolve(np.full(50, 3.5), sg) - 3.5).max() < 1e-14
    f = np.random.default_rng(3).normal(size=50)
    assert np.array_equal(SM.convolve(f, np.full(50, 0.005)), f)
    assert np.array_equal(SM.convolve(f, np.full(50, 0.01)), f)     # sigma <= 0.01 is copied


# ---- rebinning -------------------------------------------------------------------------------------------------------
def test_rebin_identity_merge_constant_and_fill():
    w = np.geomspace(1.0, 2.0, 31)
    f = np.random.default_rng(4).uniform(1.0, 2.0, 31)
    assert np.abs(SM.rebin(w, w, f) - f).max() < 1e-14
    # a uniform grid merged three by three: new centres at the middle one of each triple have the triples' edges
    wu = 1.0 + 0.01 * np.arange(30)
    fu = np.random.default_rng(5).uniform(1.0, 2.0, 30)
    got = SM.rebin(wu[1::3], wu, fu)
    assert np.abs(got - fu.reshape(10, 3).mean(axis=1)).max() < 1e-12
    # unequal widths: the width-weighted mean, by hand for one new bin over old bins 2..4 of a geometric grid
    e = SM.bin_edges(w)
    centre, half = (e[2] + e[5]) / 2, (e[5] - e[2]) / 2
    new = np.array([centre - 2 * half, centre, centre + 2 * half])
    hand = np.sum(np.diff(e)[2:5] * f[2:5]) / (e[5] - e[2])
    assert abs(SM.rebin(new, w, f)[1] - hand) < 1e-12
    assert np.abs(SM.rebin(np.linspace(1.1, 1.9, 7), w, np.full(31, 2.5)) - 2.5).max() < 1e-14
    out = SM.rebin(np.linspace(0.5, 2.5, 21), w, f)
    ne = SM.bin_edges(np.linspace(0.5, 2.5, 21))
    beyond = (ne[:-1] < e[0]) | (ne[1:] > e[-1])
    assert beyond.sum() >= 8 and (out[beyond] == 0.0).all() and (out[~beyond] > 0).all()


def test_one_pixel_has_no_bin_edges():
    with pytest.raises(ValueError, match="at least 2 pixels"):
        SM.rebin(np.array([1.0]), np.array([0.9, 1.0, 1.1]), np.ones(3))


# ---- normalisation ---------------------------------------------------------------------------------------------------
def test_norm_factors_by_hand_and_the_device_coefficients():
    from synference_amd.spectra import norm_coefficients
    w = np.array([1.0, 2.0, 3.0, 5.0, 6.0])
    f = np.array([2.0, 4.0, 8.0, 1.0, 3.0])
    top = dict(center=3.0, width=2.0)                               # pixels at 2 and 3 (both bounds included)
    assert SM.norm_factor(w, f, "tophat", top) == 6.0
    assert SM.norm_factor(w, f, "tophat", dict(center=4.0, width=0.5)) == 0.0
    filt = (np.array([1.5, 3.0, 5.5]), np.array([0.0, 1.0, 0.0]))    # T on the grid: 0, 1/3, 1, 0.2, 0
    t = np.array([0.0, 1.0 / 3.0, 1.0, 0.2, 0.0])
    num = (0 + 4 / 3) / 2 + (4 / 3 + 8) / 2 + (8 + 0.2) / 2 * 2 + (0.2 + 0) / 2
    den = (0 + 1 / 3) / 2 + (1 / 3 + 1) / 2 + (1 + 0.2) / 2 * 2 + 0.2 / 2
    assert abs(SM.norm_factor(w, f, "bandpass", dict(filter=filt)) - num / den) < 1e-14
    assert SM.norm_factor(w, f, "bandpass", dict(filter=(np.array([7.0, 8.0]), np.array([1.0, 1.0])))) == 0.0
    assert np.array_equal(SM.normalise(w, f, "tophat", dict(center=4.0, width=0.5)), np.zeros(5))

    class Filt:
        lam, transmission = filt
    # the host's coefficient tables give the same factors as one dot product
    for method, pars in (("tophat", top), ("bandpass", dict(filter=filt)), ("bandpass", dict(filter=Filt())),
                         ("tophat", dict(center=4.0, width=0.5))):
        assert abs(np.dot(norm_coefficients(w, method, pars), f) - SM.norm_factor(w, f, method, pars)) < 1e-14
    assert np.allclose(t, np.interp(w, *filt, left=0, right=0))      # the hand values used the right transmission


# ---- the shared cases ------------------------------------------------------------------------------------------------
def test_cases_keep_clear_of_ties():
    closest = np.inf
    for name, c in SC.cases().items():
        sg = SC.sigmas(c)
        assert np.isfinite(sg).all(), name
        conv = sg > 0.01
        four = 4.0 * sg[conv]
        if four.size:
            closest = min(closest, np.abs(four - np.round(four)).min())
        closest = min(closest, np.abs(sg - 0.01).min())
    assert closest >= SC.TIE_MARGIN, closest


def test_cases_cover_what_they_are_meant_to():
    c = SC.cases()
    main = SC.model("main_rinf")
    assert (main[0] == 0).sum() >= 20 and (main[-1] == 0).sum() <= 3           # low z: most bins beyond the spectrum
    passthrough = (SC.sigmas(c["main_r100"]) <= 0.01).sum(axis=1)
    assert (passthrough > 20).sum() >= 4 and passthrough.max() >= 150 and (SC.sigmas(c["main_rinf"]) > 0.01).all()
    sg = SC.sigmas(c["fine"])
    L = sg.shape[1]
    h = np.ceil(4 * sg)
    assert sg.max() > 8 and h[:, 0].min() > 0 and (h[:, -1] > 0).all() and (h.max(axis=1) > 30).all()
    oe, ne = SM.bin_edges(c["fine"]["wave"] * 4.7), SM.bin_edges(c["fine"]["observed"])     # z = 3.7
    per_new = np.searchsorted(oe, ne[1:]) - np.searchsorted(oe, ne[:-1])
    assert (per_new == 0).any() and per_new.max() >= 24 and L == 1000
    assert (SC.model("outside") == 0).all()
    assert SC.model("l2").shape == (2, 5) and (SC.model("l2") != 0).any()


def test_float32_model_against_float64_model_sets_the_device_tolerance():
    worst = 0.0
    for name in SC.cases():
        r64, r32 = SC.model(name), SC.model(name, np.float32)
        assert ((r64 == 0) == (r32 == 0)).all()
        scale = np.abs(r64).max(axis=1, keepdims=True)
        scale[scale == 0] = 1.0
        worst = max(worst, float((np.abs(r32.astype(np.float64) - r64) / scale).max()))
        c64, c32 = SC.model_convolved(name), SC.model_convolved(name, np.float32)
        worst = max(worst, float((np.abs(c32.astype(np.float64) - c64) / np.abs(c64).max(axis=1, keepdims=True)).max()))
    print(f"float32 model - float64 model, worst over the cases: {worst:.3e} of the row maximum")
    assert SC.TOL_MEASURED / 1.5 <= worst <= SC.TOL_MEASURED, worst   # the stored figure is the measured one, rounded up


# ---- host logic of the fitter ----------------------------------------------------------------------------------------
def _fitter(observation_type="spectra", with_redshift=True, grid=True):
    from synference_amd.fitter import SBI_Fitter
    g, wave, pars = SC.fitter_library(n=12, L=20)
    names = ["redshift", "mass", "slope"] if with_redshift else ["zed", "mass", "slope"]
    return SBI_Fitter(name="spec", parameter_names=names, raw_observation_names=[f"{w:.8f}" for w in wave],
                      raw_observation_grid=g if grid else None, parameter_array=pars, raw_observation_units="nJy",
                      observation_type=observation_type)


def test_fitter_argument_checks_need_no_device():
    obs = np.linspace(1.0, 4.0, 8)
    curve = dict(inst_resolution_wavelengths=np.array([0.5, 5.0]), inst_resolution_r=np.array([50.0, 100.0]))
    with pytest.raises(ValueError, match="only for spectra"):
        _fitter("photometry").create_feature_array_from_raw_spectra(resample_wavelengths=obs, **curve)
    with pytest.raises(ValueError, match="library is not set"):
        _fitter(grid=False).create_feature_array_from_raw_spectra(resample_wavelengths=obs, **curve)
    with pytest.raises(ValueError, match="Feature metallicity not found"):
        _fitter().create_feature_array_from_raw_spectra(extra_features=["metallicity"], resample_wavelengths=obs, **curve)
    with pytest.raises(AssertionError, match="resample_wavelengths must be provided"):
        _fitter().create_feature_array_from_raw_spectra(**curve)
    with pytest.raises(AssertionError, match="inst_resolution_wavelengths must be provided"):
        _fitter().create_feature_array_from_raw_spectra(resample_wavelengths=obs, inst_resolution_r=curve["inst_resolution_r"])
    with pytest.raises(AssertionError, match="inst_resolution_r must be provided"):
        _fitter().create_feature_array_from_raw_spectra(resample_wavelengths=obs,
                                                        inst_resolution_wavelengths=curve["inst_resolution_wavelengths"])
    with pytest.raises(ValueError, match='"tophat" or "bandpass"'):
        _fitter().create_feature_array_from_raw_spectra(flux_norm_method=lambda w, f: 1.0, resample_wavelengths=obs, **curve)
    with pytest.raises(ValueError, match="requires 'center' and 'width'"):
        _fitter().create_feature_array_from_raw_spectra(flux_norm_method="tophat", resample_wavelengths=obs, **curve)
    with pytest.raises(ValueError, match="not supported"):
        _fitter().create_feature_array_from_raw_spectra(normed_flux_units="erg", resample_wavelengths=obs, **curve)
    with pytest.raises(ValueError, match="Feature redshift not found"):        # the default extra feature
        _fitter(with_redshift=False).create_feature_array_from_raw_spectra()
    # create_feature_array reaches the spectra path (and its checks) instead of refusing spectra
    with pytest.raises(AssertionError, match="resample_wavelengths must be provided"):
        _fitter().create_feature_array(flux_units="nJy")


def test_unit_codes_and_entry_point_rejections(lib):
    import ctypes as C
    from synference_amd import _lib, spectra as SP
    assert SP.unit_conversion("nJy", "AB") == (SP.UNIT_AB, 1e-9)
    assert SP.unit_conversion("nJy", "log10 uJy") == (SP.UNIT_LOG10, 1e-3)
    assert SP.unit_conversion("uJy", "nJy") == (SP.UNIT_LINEAR, 1e3)
    hdr = (Path(__file__).resolve().parents[1] / "include" / "synference_hip.h").read_text()
    for name in ("MAX_L", "MAX_CURVE", "MAX_HALF_WIDTH"):
        assert f"#define SF_SPECTRA_{name} {getattr(SP, name)}\n" in hdr
    d = _lib.sf_spectra_desc()
    d.mode, d.N, d.L, d.M, d.ld_flux, d.ld_out, d.h_limit, d.trunc, d.n_curve = SP.MODE_TRANSFORM, 4, SP.MAX_L + 1, 8, 1 << 20, 8, 8, 4.0, 2
    assert lib.sf_spectra_transform(C.byref(d), None) == -1 and b"exceeds the cap of 16384" in lib.sf_last_error()
    d.L, d.n_curve = 64, SP.MAX_CURVE + 1
    assert lib.sf_spectra_transform(C.byref(d), None) == -1 and b"does not fit the table of 256" in lib.sf_last_error()
    d.n_curve, d.M = 2, 1
    assert lib.sf_spectra_transform(C.byref(d), None) == -1 and b"at least 2 pixels" in lib.sf_last_error()
    d.M, d.N = 8, 0                                                  # nothing to do: no pointer is looked at
    d.wave = d.z = d.observed_wave = d.curve_wave = d.curve_r = 4096
    assert lib.sf_spectra_transform(C.byref(d), None) == 0
