"""sf_spectra_transform on the device against the float64 model of tests/spectra_model.py on the shared cases of
tests/spectra_cases.py (bound: 4 x the float32-model discrepancy measured by tests/test_cpu_spectra_model.py, in units of
the row's maximum), its launch-shape invariance, units / clip / normalisation / crop, the rejections, and the fitter end to
end: create_feature_array_from_raw_spectra -> FCN embedding + MAF -> sample -> save / reload."""
import numpy as np
import pytest
import torch

import spectra_cases as SC
import spectra_model as SM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32_EPS = float(np.finfo(np.float32).eps)


def _run(c, rows=slice(None)):
    from synference_amd.spectra import transform_spectrum
    flux = torch.as_tensor(c["flux"][rows]).to(DEV)
    ow, out = transform_spectrum(c["wave"], flux, c["z"][rows], c["observed"], c["curve_wave"], c["curve_r"], c["theory_r"])
    assert ow is c["observed"] and out.dtype == torch.float32 and out.is_contiguous()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", list(SC.cases()))
def test_transform_spectrum_against_the_float64_model(name):
    c = SC.cases()[name]
    ref = SC.model(name)
    got = _run(c)
    assert got.shape == ref.shape
    assert np.array_equal(got == 0, ref == 0) and (got[ref == 0] == 0).all()         # filled bins are exactly 0
    scale = np.abs(ref).max(axis=1, keepdims=True)
    scale[scale == 0] = 1.0
    err = float((np.abs(got.astype(np.float64) - ref) / scale).max())
    print(f"{name}: device - float64 model = {err:.3e} of the row maximum (bound {SC.TOL_BOUND:.3e})")
    assert err <= SC.TOL_BOUND


@pytest.mark.parametrize("name", ["main_r100", "fine", "theory_r_array"])
def test_convolve_variable_width_gaussian_against_the_float64_model(name):
    from synference_amd.spectra import convolve_variable_width_gaussian
    c = SC.cases()[name]
    sg = SC.sigmas(c)
    ref = SC.model_convolved(name)
    flux = torch.as_tensor(c["flux"]).to(DEV)
    got = convolve_variable_width_gaussian(flux, sg).cpu().numpy()
    err = float((np.abs(got.astype(np.float64) - ref) / np.abs(ref).max(axis=1, keepdims=True)).max())
    print(f"{name}: convolution, device - float64 model = {err:.3e} of the row maximum (bound {SC.TOL_BOUND:.3e})")
    assert err <= SC.TOL_BOUND
    copied = sg <= 0.01
    assert np.array_equal(got[copied], c["flux"][copied])                            # pass-through pixels are copies
    # one sigma row for every spectrum, and a single spectrum
    one = convolve_variable_width_gaussian(flux, sg[0]).cpu().numpy()
    assert np.array_equal(one[0], got[0])
    assert np.array_equal(convolve_variable_width_gaussian(flux[0], sg[0]).cpu().numpy(), got[0])


def test_result_does_not_depend_on_the_launch_shape():
    from synference_amd.spectra import transform_spectrum
    c = SC.cases()["main_r100"]
    full = _run(c)
    assert np.array_equal(_run(c), full)                                              # a repeated call
    assert np.array_equal(_run(c, slice(0, 2)), full[:2])                             # the first k rows alone
    # more rows than workgroups launched at once share workgroups: the same bits per row
    reps = 4000
    flux = torch.as_tensor(np.tile(c["flux"], (reps, 1))).to(DEV)
    _, big = transform_spectrum(c["wave"], flux, np.tile(c["z"], reps), c["observed"], c["curve_wave"], c["curve_r"], c["theory_r"])
    big = big.cpu().numpy().reshape(reps, *full.shape)
    assert np.array_equal(big, np.broadcast_to(full, big.shape))
    # a single spectrum with a scalar redshift, and one spectrum at several redshifts
    _, single = transform_spectrum(c["wave"], torch.as_tensor(c["flux"][2]).to(DEV), float(c["z"][2]), c["observed"],
                                   c["curve_wave"], c["curve_r"], c["theory_r"])
    assert single.shape == (len(c["observed"]),) and np.array_equal(single.cpu().numpy(), full[2])
    _, fan = transform_spectrum(c["wave"], torch.as_tensor(c["flux"][2]).to(DEV), c["z"], c["observed"], c["curve_wave"],
                                c["curve_r"], c["theory_r"])
    assert fan.shape == full.shape and np.array_equal(fan[2].cpu().numpy(), full[2])


def test_empty_batch_and_largest_spectrum():
    from synference_amd.spectra import MAX_L, transform_spectrum
    c = SC.cases()["main_rinf"]
    _, out = transform_spectrum(c["wave"], torch.empty((0, 301), device=DEV), np.empty(0), c["observed"], c["curve_wave"],
                                c["curve_r"])
    assert out.shape == (0, 37)
    # L at the cap (128 KiB of LDS per workgroup): a constant spectrum stays constant wherever the bins are covered
    wave = np.geomspace(0.1, 2.0, MAX_L)
    flux = torch.full((3, MAX_L), 7.5, device=DEV)
    _, out = transform_spectrum(wave, flux, np.array([0.5, 2.0, 3.7]), c["observed"], np.array([0.1, 20.0]),
                                np.array([2000.0, 4000.0]))
    out = out.cpu().numpy()
    ref = np.stack([SM.rebin(c["observed"], wave * (1 + z), np.full(MAX_L, 7.5)) for z in (0.5, 2.0, 3.7)])
    assert np.array_equal(out == 0, ref == 0) and np.abs(out - ref).max() <= 7.5 * SC.TOL_BOUND


def _features(c, **kw):
    from synference_amd import spectra as SP
    flux = torch.as_tensor(c["flux"]).to(DEV)
    return SP.spectra_features(flux, c["wave"], z=c["z"], observed_wave=c["observed"], resolution_curve_wave=c["curve_wave"],
                               resolution_curve_r=c["curve_r"], theory_r=c["theory_r"], **kw).cpu().numpy()


def test_units_and_clip():
    """Each unit against the float64 model's conversion of the float64 model's bins.  Bound: the bins' own bound, carried
    through the conversion (d log10 f = df / (f ln 10)), plus float32 roundings of the result and of the logarithm's
    argument (4 eps of the value, 4 eps / ln 10 absolute)."""
    from synference_amd import spectra as SP
    c = SC.cases()["main_rinf"]
    ref = SC.model("main_rinf")
    rowmax = np.abs(ref).max(axis=1, keepdims=True)
    live = ref > 0
    dlog = SC.TOL_BOUND * rowmax / np.where(live, ref, 1.0) / np.log(10) + 4 * F32_EPS / np.log(10)
    for units in ("AB", "log10 nJy", "uJy", "log10 mJy"):
        code, scale = SP.unit_conversion("nJy", units)
        got = _features(c, unit_code=code, unit_scale=scale).astype(np.float64)
        want = SM.to_units(ref, "nJy", units)
        if units == "AB":
            assert np.isposinf(got[~live]).all() and np.isposinf(want[~live]).all()      # zero flux: +inf, as numpy gives
            bound = 2.5 * dlog + 4 * F32_EPS * np.abs(want)
        elif units.startswith("log10"):
            assert np.isneginf(got[~live]).all()
            bound = dlog + 4 * F32_EPS * np.abs(want)
        else:
            assert (got[~live] == 0).all()
            bound = (SC.TOL_BOUND * rowmax + 4 * F32_EPS * np.abs(ref)) * scale
        assert (np.abs(got[live] - want[live]) <= np.broadcast_to(bound, want.shape)[live]).all(), units
    # clip: [lo, hi] in the output unit; +inf comes down to the maximum
    code, scale = SP.unit_conversion("nJy", "AB")
    got = _features(c, unit_code=code, unit_scale=scale, clip=(24.0, 30.0))
    want = np.clip(SM.to_units(ref, "nJy", "AB"), 24.0, 30.0)
    assert (got[~live] == 30.0).all() and got.min() >= 24.0 and (want == 24.0).any() and np.abs(got - want).max() < 1e-4
    # negative flux: NaN in AB, and the clip keeps it
    neg = dict(c, flux=-c["flux"])
    got = _features(neg, unit_code=code, unit_scale=scale, clip=(24.0, 30.0))
    assert np.isnan(got[live]).all() and (got[~live] == 30.0).all()


@pytest.mark.parametrize("method", ["tophat", "bandpass"])
@pytest.mark.parametrize("rest", [True, False])
def test_normalisation(method, rest):
    from synference_amd import spectra as SP
    c = SC.cases()["main_rinf"]
    ref = SC.model("main_rinf")
    grid = c["wave"] if rest else c["observed"]
    pars = dict(center=1.0, width=0.5) if rest else dict(center=4.0, width=1.0)
    if method == "bandpass":
        lam = np.linspace(pars["center"] - pars["width"], pars["center"] + pars["width"], 9)
        pars = dict(filter=(lam, np.exp(-0.5 * ((lam - pars["center"]) / (0.4 * pars["width"])) ** 2) - np.exp(-3.125)))
    table = SP.norm_coefficients(grid, method, pars)
    got = _features(c, norm_frame=SP.NORM_REST if rest else SP.NORM_OBSERVED, norm_table=table).astype(np.float64)
    # the factor is one scalar per spectrum and the transform is linear: the model's bins over the model's factor
    source = c["flux"].astype(np.float64) if rest else ref
    fac = np.array([SM.norm_factor(grid, source[i], method, pars) for i in range(len(ref))])
    want = np.where(fac[:, None] != 0, ref / np.where(fac != 0, fac, 1.0)[:, None], 0.0)
    if not rest:
        assert (fac[:2] == 0).all() and (fac[2:] != 0).all()          # z = 0, 0.5: the band lies beyond the spectrum
        assert (got[:2] == 0).all()                                    # a factor of 0: the whole row is 0
    else:
        assert (fac != 0).all()
    # bound, with t the bins' bound and m = max|want| of the row = row maximum / factor: the bins carry t m; the rest-frame
    # factor is a float64 sum of float32 inputs, exact here, while the observed-frame factor is a mean of device bins, off
    # by up to t m relative, which moves want by |want| t m; then the float32 division
    m = np.abs(want).max(axis=1, keepdims=True)
    bound = SC.TOL_BOUND * m * (1.0 if rest else 1.0 + np.abs(want)) + 4 * F32_EPS * np.abs(want)
    assert (np.abs(got - want) <= bound).all()


def test_zero_factor_row_in_the_rest_frame_and_no_redshift_crop():
    from synference_amd import spectra as SP
    c = SC.cases()["main_rinf"]
    flux = c["flux"].copy()
    flux[1] = 0.0                                                      # a spectrum with no flux in the band: factor 0
    table = SP.norm_coefficients(c["wave"], "tophat", dict(center=1.0, width=0.5))
    got = _features(dict(c, flux=flux), norm_frame=SP.NORM_REST, norm_table=table)
    assert (got[1] == 0).all() and (got[0] != 0).any()
    # no redshift: columns 40 .. 239 of the theory grid, normalised on the WHOLE theory grid, log10 uJy, clipped
    code, scale = SP.unit_conversion("nJy", "log10 uJy")
    out = SP.spectra_features(torch.as_tensor(flux).to(DEV), c["wave"], norm_frame=SP.NORM_REST, norm_table=table, unit_code=code,
                              unit_scale=scale, clip=(-4.0, -3.0), columns=(40, 200)).cpu().numpy()
    assert out.shape == (5, 200)
    fac = np.array([SM.norm_factor(c["wave"], flux[i], "tophat", dict(center=1.0, width=0.5)) for i in range(5)])
    want = np.clip(SM.to_units(np.where(fac[:, None] != 0, flux / np.where(fac != 0, fac, 1.0)[:, None], 0.0), "nJy", "log10 uJy"),
                   -4.0, -3.0)[:, 40:240]
    assert (out[1] == -4.0).all() and (want == -3.0).any() and (want < -3.0).any()
    # the factor is a float64 sum of float32 inputs: what is left are the float32 roundings of the quotient and of the scaled
    # argument (eps / ln 10 in the logarithm) and the float32 logarithm itself, a few ulp of a value of at most 4
    assert np.abs(out - want).max() <= 2 * F32_EPS / np.log(10) + 4 * F32_EPS * 4.0


def test_rejections():
    from synference_amd.spectra import MAX_L, convolve_variable_width_gaussian, transform_spectrum
    c = SC.cases()["main_rinf"]
    flux = torch.as_tensor(c["flux"]).to(DEV)
    args = (c["observed"], c["curve_wave"], c["curve_r"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transform_spectrum(c["wave"], torch.as_tensor(c["flux"]), c["z"], *args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        convolve_variable_width_gaussian(c["flux"], np.ones(301))
    big = torch.zeros((2, MAX_L + 1), device=DEV)
    with pytest.raises(RuntimeError, match="exceeds the cap of 16384"):
        transform_spectrum(np.geomspace(0.1, 2.0, MAX_L + 1), big, np.zeros(2), *args)
    with pytest.raises(RuntimeError, match="does not fit the table of 256"):
        transform_spectrum(c["wave"], flux, c["z"], c["observed"], np.linspace(0.5, 5, 300), np.full(300, 100.0))
    with pytest.raises(ValueError, match="pixels but the spectra have"):
        transform_spectrum(c["wave"][:-1], flux, c["z"], *args)
    with pytest.raises(ValueError, match="redshifts for"):
        transform_spectrum(c["wave"], flux, c["z"][:3], *args)
    with pytest.raises(ValueError, match="same length"):
        transform_spectrum(c["wave"], flux, c["z"], c["observed"], c["curve_wave"], c["curve_r"][:-1])
    with pytest.raises(ValueError, match="theory_r must be"):
        transform_spectrum(c["wave"], flux, c["z"], *args, theory_r=np.ones(7))
    with pytest.raises(ValueError, match="at least 2 pixels"):        # M = 1: one pixel has no bin edges (as in the model)
        transform_spectrum(c["wave"], flux, c["z"], c["observed"][:1], c["curve_wave"], c["curve_r"])
    with pytest.raises(ValueError, match="strictly ascending"):
        transform_spectrum(c["wave"][::-1], flux, c["z"], *args)
    with pytest.raises(ValueError, match="sigma_pixels must be"):
        convolve_variable_width_gaussian(flux, np.ones(300))
    with pytest.raises(ValueError, match="more than the 65536"):
        transform_spectrum(c["wave"], flux, c["z"], c["observed"], c["curve_wave"], c["curve_r"] * 1e-5)


# ---- the fitter, end to end ------------------------------------------------------------------------------------------
RESAMPLE = np.linspace(0.8, 4.6, 48)
CURVE = dict(inst_resolution_wavelengths=np.array([0.5, 1.5, 3.0, 5.5]), inst_resolution_r=np.array([30.0, 60.0, 150.0, 300.0]))
FEATURE_KW = dict(normed_flux_units="log10 nJy", min_flux_value=-2.0, flux_norm_method="tophat",
                  flux_norm_parameters=dict(center=0.5, width=0.3, rest_frame=True), resample_wavelengths=RESAMPLE, theory_r=200.0)


@pytest.fixture(scope="module")
def spectra_fitter():
    from synference_amd import SBI_Fitter
    grid, wave, pars = SC.fitter_library()
    f = SBI_Fitter(name="spec", parameter_names=["redshift", "mass", "slope"], raw_observation_names=[repr(float(w)) for w in wave],
                   raw_observation_grid=grid, parameter_array=pars, raw_observation_units="nJy", observation_type="spectra",
                   device=DEV)
    f.create_feature_array_from_raw_spectra(**FEATURE_KW, **CURVE)
    return f, grid, wave, pars


def test_fitter_feature_array_equals_the_model_row_for_row(spectra_fitter):
    from synference_amd import SBI_Fitter
    f, grid, wave, pars = spectra_fitter
    want, wavs = SM.feature_array(grid, wave, pars, ["redshift", "mass", "slope"], **FEATURE_KW, **CURVE)
    got = f.feature_array
    assert got.shape == (600, 49) and got.dtype == np.float32 and got.flags.c_contiguous
    assert f.feature_names == ["spectra", "redshift"] and f.feature_units == ["log10 nJy"] and f.has_features
    assert np.array_equal(f.feature_wavelengths, RESAMPLE) and np.array_equal(wavs, RESAMPLE)
    assert set(f.feature_array_flags) == {"extra_features", "crop_wavelength_range", "normed_flux_units", "flux_norm_method",
                                          "flux_norm_parameters", "parameters_to_remove", "parameters_to_add",
                                          "parameter_transformations", "resample_wavelengths"}
    assert np.array_equal(got[:, 48], pars[:, 0].astype(np.float32))
    assert f.fitted_parameter_array.shape == (600, 3)
    clipped = want[:, :48] == -2.0
    assert np.array_equal(got[:, :48] == -2.0, clipped) and clipped.any() and not clipped.all()
    # log10 of normalised bins: the bins' bound (of the row maximum) through d log10 f = df / (f ln 10) -- the rest-frame
    # factor is a float64 sum of float32 inputs --, plus the float32 roundings of the argument and the float32 logarithm
    lin = 10.0 ** want[:, :48]
    bound = SC.TOL_BOUND * lin.max(axis=1, keepdims=True) / lin / np.log(10) + 8 * F32_EPS * (1 + np.abs(want[:, :48]))
    assert (np.abs(got[:, :48] - want[:, :48])[~clipped] <= bound[~clipped]).all()
    # create_feature_array reaches the same code, cropped in the observed frame
    g = SBI_Fitter(name="spec2", parameter_names=["redshift", "mass", "slope"], raw_observation_names=list(f.raw_observation_names),
                   raw_observation_grid=grid, parameter_array=pars, raw_observation_units="nJy", observation_type="spectra", device=DEV)
    kw = {k: v for k, v in FEATURE_KW.items() if k != "normed_flux_units"}
    g.create_feature_array(flux_units="log10 nJy", extra_features=[], crop_wavelength_range=(1.0, 3.0), **kw, **CURVE)
    keep = (RESAMPLE >= 1.0) & (RESAMPLE <= 3.0)
    assert g.feature_array.shape == (600, int(keep.sum())) and np.array_equal(g.feature_wavelengths, RESAMPLE[keep])
    want_c, _ = SM.feature_array(grid, wave, pars, ["redshift", "mass", "slope"], extra_features=(), crop_wavelength_range=(1.0, 3.0),
                                 **FEATURE_KW, **CURVE)
    ok = want_c != -2.0
    lin = 10.0 ** want_c
    bound = SC.TOL_BOUND * lin.max(axis=1, keepdims=True) / lin / np.log(10) + 8 * F32_EPS * (1 + np.abs(want_c))
    assert (np.abs(g.feature_array - want_c)[ok] <= bound[ok]).all()


def test_fitter_trains_samples_saves_and_reloads(spectra_fitter, tmp_path):
    from synference_amd import FCN, SBI_Fitter
    f = spectra_fitter[0]
    post, stats = f.run_single_sbi(model_type="maf", hidden_features=32, num_transforms=3, training_batch_size=128,
                                   learning_rate=2e-3, stop_after_epochs=3, max_num_epochs=6, random_seed=2, save_model=True,
                                   out_dir=str(tmp_path), name_append="t", verbose=False, plot=False, evaluate_model=False,
                                   embedding_net=FCN([64, 16]))
    est = post.posteriors[0].posterior_estimator
    assert est.has_embedding and est.spec.C == 16
    loss = stats[0]["training_loss"]
    assert np.isfinite(loss).all() and loss[-1] < loss[0]
    X = f._X_test[:5]
    s = f.sample_posterior(X, num_samples=50, seed=3)
    assert s.shape == (5, 50, 3) and np.isfinite(s).all()
    g = SBI_Fitter("spec", ["redshift", "mass", "slope"], observation_type="spectra", device=DEV)
    g.load_model_from_pkl(str(tmp_path / "spec"))       # (out_dir gets the fitter's name appended)
    assert np.array_equal(g.feature_wavelengths, RESAMPLE) and g.feature_names == ["spectra", "redshift"]
    assert g.feature_array_flags["normed_flux_units"] == "log10 nJy" and g.feature_array_flags["flux_norm_method"] == "tophat"
    assert np.array_equal(g.feature_array_flags["resample_wavelengths"], RESAMPLE)
    assert np.array_equal(g.feature_array, f.feature_array)
    assert np.array_equal(g.sample_posterior(X, num_samples=50, seed=3), s)
