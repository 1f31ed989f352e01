"""Empirical noise models, host side: known answers, the sampled distributions of the numpy model (tests/noise_model.py)
against scipy's truncated normal, the host fit against scipy.stats.binned_statistic, serialisation, the packed struct against
the header, the refusals of the fitter, and the tolerance of the device comparison (tests/test_gpu_noise.py) -- the float32
evaluation of the model against its float64 one on the very inputs of that test."""
import ctypes as C
import pickle
import re
from pathlib import Path

import numpy as np
import pytest

import noise_cases as NC
import noise_model as NM
from synference_amd import _lib
from synference_amd.noise_models import (AsinhEmpiricalUncertaintyModel, GeneralEmpiricalUncertaintyModel,
                                         UncertaintyModel, band_fields, pack_models)

ROOT = Path(__file__).resolve().parents[1]


def _run(model, flux, in_unit, out_unit, seed=0, dtype=np.float64):
    bands, table = pack_models([model], in_unit, out_unit)
    flux = np.asarray(flux, np.float32)
    return NM.scatter_band(band_fields(bands)[0], table, flux, NM.uniforms(seed, np.arange(len(flux)), 0), dtype)


def _ab_model(**kw):
    f, e = NC.mock_catalogue()
    m, me = NC.ab_of(f, e)
    return GeneralEmpiricalUncertaintyModel(m, me, flux_unit="AB", return_noise=True, **kw)


# ---- known answers ----------------------------------------------------------------------------------------------------
def test_static_unit_conversions():
    assert UncertaintyModel.ab_to_jy(8.9) == pytest.approx(1.0)
    assert UncertaintyModel.jy_to_ab(1e-6) == pytest.approx(23.9)
    fj = UncertaintyModel.ab_to_jy(25.0)
    ej = UncertaintyModel.ab_err_to_jy(0.1, fj)
    assert UncertaintyModel.jy_err_to_ab(ej, fj) == pytest.approx(0.1)


def test_units_are_plain_strings_and_anything_else_is_refused():
    f, e = NC.mock_catalogue()
    with pytest.raises(ValueError, match="unit"):
        GeneralEmpiricalUncertaintyModel(f, e, flux_unit="erg/s")
    with pytest.raises(ValueError, match="unit"):
        AsinhEmpiricalUncertaintyModel(f, e, interpolation_flux_unit="AB")
    m = GeneralEmpiricalUncertaintyModel(f * 1e6, e * 1e6, flux_unit="uJy")
    with pytest.raises(ValueError, match="unit"):
        pack_models([m], "parsec", "uJy")
    with pytest.raises(ValueError, match="asinh"):
        pack_models([m], "uJy", "asinh")                     # the reference silently returns AB magnitudes (982-987)
    a = AsinhEmpiricalUncertaintyModel(f, e)
    with pytest.raises(ValueError, match="asinh"):
        pack_models([a], "nJy", "AB")                        # the reference silently returns asinh magnitudes (560)
    with pytest.raises(ValueError, match="mixed"):
        pack_models([m, a], "nJy", "asinh")


def test_every_source_below_the_snr_cut_lands_on_the_limit():
    m = _ab_model(upper_limits=True, treat_as_upper_limits_below=1e6, upper_limit_flux_behaviour="upper_limit")
    assert m.upper_limit_value is not None
    r = _run(m, np.linspace(22.0, 27.0, 500), "AB", "AB")
    assert np.all(r["y"] == np.float32(m.upper_limit_value))


@pytest.mark.parametrize("behaviour", ["flux", "upper_limit", "max", "sig_3"])
def test_each_error_behaviour_gives_its_value(behaviour):
    m = _ab_model(upper_limits=True, treat_as_upper_limits_below=1e6, upper_limit_flux_err_behaviour=behaviour,
                  max_flux_error=0.75)
    want = {"flux": float(m._mu_sigma_interpolator(m.upper_limit_value)), "upper_limit": m.upper_limit_value, "max": 0.75,
            "sig_3": 2.5 / (3 * np.log(10))}[behaviour]
    fields = band_fields(pack_models([m], "AB", "AB")[0])[0]
    assert fields["replace_err"] == 1 and fields["err_value"] == pytest.approx(want, rel=1e-6)
    r = _run(m, np.full(200, 25.0), "AB", "AB")
    assert np.allclose(r["s"], min(want, 0.75), rtol=1e-6)   # the clip to max_flux_error comes last
    m.upper_limit_flux_err_behaviour = "something_else"      # not a recognised rule: the errors stay (the reference's fall-through)
    assert band_fields(pack_models([m], "AB", "AB")[0])[0]["replace_err"] == 0


def test_noise_at_constant_flux_has_the_interpolated_median_as_its_width():
    m = _ab_model()
    f0 = 24.0
    r = _run(m, np.full(20000, f0), "AB", "AB", seed=5)
    noise = r["y"] - f0
    want = float(m._mu_sigma_interpolator(f0))
    print(f"mean {noise.mean():.5f} std {noise.std():.5f} interpolated median {want:.5f}")
    assert abs(noise.mean()) < 0.1 * want and noise.std() == pytest.approx(want, rel=0.1)


# ---- distributions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(NC.REGIME_SEEDS))
def test_sampled_sigma_and_truncated_noise_follow_scipys_truncnorm(name):
    model, f0, mu, ss = NC.regimes()[name]
    r = _run(model, np.full(NC.KS_ROWS, f0), "uJy", "uJy", seed=NC.REGIME_SEEDS[name])
    assert np.allclose(r["parts1"]["mu"], mu) and np.allclose(r["parts1"]["ss"], ss)
    p_sigma, p_noise = NC.ks_pvalues(model, f0, mu, ss, r["y"], r["s"])
    print(f"{name}: p(sigma) {p_sigma:.3g} p(noise) {p_noise:.3g}")
    assert p_sigma > 1e-2 and p_noise > 1e-2                 # the seed was chosen for this; the device test asks for 1e-3
    assert (r["s"] >= 0).all() and np.abs((r["y"] - f0) / r["s"]).max() <= 3.0 + 1e-9


def test_upper_tail_of_the_sigma_quantile_survives_float32():
    """q = Q(a) (1 - u) keeps the upper tail that P(a) + u (1 - P(a)) rounds away in float32."""
    b = NM.Band(dict(n_bins=0, table_offset=0), np.zeros(0, np.float32), np.float32)
    u = np.float32(1) - np.float32(2.0 ** -24) * np.arange(1, 200, dtype=np.float32)
    for a in (-8.0, 0.5, 6.0, 12.0):
        t32 = NM.lower_trunc_quantile(b, np.full(u.shape, a, np.float32), u)
        b64 = NM.Band(dict(n_bins=0, table_offset=0), np.zeros(0, np.float32), np.float64)
        t64 = NM.lower_trunc_quantile(b64, np.full(u.shape, a), u.astype(np.float64))
        assert np.isfinite(t32).all() and np.allclose(t32, t64, rtol=2e-5, atol=2e-5), a
        assert (t32 >= np.float32(a) - 1e-4).all()


# ---- the host fit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_bins", [True, False], ids=["log", "linear"])
def test_fit_equals_scipys_binned_statistic(log_bins):
    stats = pytest.importorskip("scipy.stats")
    f, e = NC.mock_catalogue(3000)
    fu, eu = f * 1e6, e * 1e6
    m = GeneralEmpiricalUncertaintyModel(fu, eu, flux_unit="uJy", log_bins=log_bins, num_bins=20)
    ok = np.isfinite(fu) & np.isfinite(eu) & (eu > 0)
    x, v = fu[ok], eu[ok]
    edges = (np.logspace(np.log10(x[x > 0].min()), np.log10(x.max()), 21) if log_bins else np.linspace(x.min(), x.max(), 21))
    med = stats.binned_statistic(x, v, "median", bins=edges)[0]
    std = stats.binned_statistic(x, v, np.std, bins=edges)[0]
    cnt = stats.binned_statistic(x, x, "count", bins=edges)[0]
    keep = cnt >= 10
    assert 2 <= keep.sum()
    assert np.allclose(m.bin_centers, ((edges[:-1] + edges[1:]) / 2)[keep])
    assert np.allclose(m.median_error_in_bin, med[keep]) and np.allclose(m.std_error_in_bin, std[keep])


def test_a_thin_bin_is_dropped_and_too_few_bins_raise():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(0, 1, 50), rng.uniform(1, 2, 4), rng.uniform(2, 3, 50), [3.0]])
    v = rng.uniform(0.1, 0.2, x.size)
    m = GeneralEmpiricalUncertaintyModel(x, v, flux_unit="uJy", flux_bins=np.array([0.0, 1.0, 2.0, 3.0]))
    assert np.allclose(m.bin_centers, [0.5, 2.5])
    assert m.median_error_in_bin[1] == pytest.approx(np.median(v[x >= 2.0]))     # the last bin is closed on the right
    with pytest.raises(ValueError, match="enough valid bins"):
        GeneralEmpiricalUncertaintyModel(x, v, flux_unit="uJy", flux_bins=np.array([0.0, 1.0, 2.0, 3.0]), min_samples_per_bin=51)


def test_upper_limit_value_is_the_log_log_interpolation():
    f, e = NC.mock_catalogue(3000)
    fu, eu = f * 1e6, e * 1e6
    m = GeneralEmpiricalUncertaintyModel(fu, eu, flux_unit="uJy", upper_limits=True, treat_as_upper_limits_below=3.0)
    ok = np.isfinite(fu) & (eu > 0)
    snr = fu[ok] / eu[ok]
    good = (snr > 0) & (fu[ok] > 0)
    order = np.argsort(snr[good])
    lx, ly = np.log10(snr[good][order]), np.log10(fu[ok][good][order] * 1e-6)
    want = 10 ** np.interp(np.log10(3.0), lx, ly) * 1e6
    assert lx[0] < np.log10(3.0) < lx[-1] and m.upper_limit_value == pytest.approx(want, rel=1e-12)
    # fewer than 2 valid points: the early return leaves no limit
    m2 = GeneralEmpiricalUncertaintyModel(-np.abs(fu), eu, flux_unit="uJy", log_bins=False, upper_limits=True,
                                          treat_as_upper_limits_below=3.0)
    assert m2.upper_limit_value is None


def test_already_binned_path():
    m1 = _ab_model()
    m2 = GeneralEmpiricalUncertaintyModel(m1.bin_centers[::-1], None, flux_unit="AB", already_binned=True,
                                          bin_median_errors=m1.median_error_in_bin[::-1],
                                          bin_std_errors=m1.std_error_in_bin[::-1])
    x = np.linspace(20.0, 30.0, 64)
    assert np.allclose(m1._mu_sigma_interpolator(x), m2._mu_sigma_interpolator(x))
    assert np.array_equal(pack_models([m1], "AB", "AB")[1], pack_models([m2], "AB", "AB")[1])   # packed ascending
    assert m2.upper_limit_value is None


def test_asinh_softening_and_binning_space():
    f, e = NC.mock_catalogue()
    a = AsinhEmpiricalUncertaintyModel(f, e, asinh_b_factor=5.0)
    assert a.b == pytest.approx(5.0 * np.median(e)) and a.interpolation_flux_unit == "asinh"
    assert 15 < a.bin_centers.mean() < 30                           # asinh magnitudes
    p = AsinhEmpiricalUncertaintyModel(f, e, interpolation_flux_unit="uJy")
    assert 0 < p.bin_centers.min() < p.bin_centers.max() < 400      # uJy
    fa, fp = (band_fields(pack_models([m], "nJy", "asinh")[0])[0] for m in (a, p))
    assert (fa["resample"], fp["resample"]) == (0, 1)               # "empirical": first draw in asinh space, second in flux space
    assert fp["unit_per_jy"] == pytest.approx(1e6) and fa["b_jy"] == pytest.approx(a.b)


# ---- serialisation, ABI, public surface ---------------------------------------------------------------------------------
def test_pickle_round_trip():
    for m in NC.five_models():
        m2 = pickle.loads(pickle.dumps(m))
        assert type(m2) is type(m)
        for k in ("bin_centers", "median_error_in_bin", "std_error_in_bin"):
            assert np.array_equal(getattr(m, k), getattr(m2, k))
        unit = "asinh" if isinstance(m, AsinhEmpiricalUncertaintyModel) else "AB"
        b1, t1 = pack_models([m], "nJy", unit)
        b2, t2 = pack_models([m2], "nJy", unit)
        assert band_fields(b1) == band_fields(b2) and np.array_equal(t1, t2)


def test_noise_band_struct_matches_header_field_order():
    hdr = (ROOT / "include" / "synference_hip.h").read_text()
    body = hdr[hdr.index("typedef struct sf_noise_band {"):hdr.index("} sf_noise_band;")]
    fields = re.findall(r"\b(int32_t|float)\s+([a-zA-Z_][a-zA-Z_0-9]*)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [n for _, n in fields] == [f[0] for f in _lib.sf_noise_band._fields_]
    assert [C.c_int32 if t == "int32_t" else C.c_float for t, _ in fields] == [f[1] for f in _lib.sf_noise_band._fields_]
    assert C.sizeof(_lib.sf_noise_band) == 4 * len(fields)


def test_packed_bins_of_the_comparison_bands():
    _, bands, table, flux = NC.five_bands()
    assert tuple(b["n_bins"] for b in band_fields(bands)) == NC.BINS
    assert flux.shape == (NC.N_ROWS, 5) and flux[11, 0] == 0.0 and flux[12, 0] < 0.0 and table.dtype == np.float32


def test_abi_refuses_bad_models_before_any_device(lib):
    _, bands, table, _ = NC.five_bands()
    p = C.cast((C.c_float * 64)(), C.c_void_p)               # never dereferenced: the argument checks come first
    tp = table.ctypes.data_as(_lib.c_f32p)

    def sc(N=4, Cb=5, b=bands, t=tp, nt=table.size, ns=2):
        return lib.sf_scatter_empirical(p, N, Cb, b, t, nt, ns, 1, p, p, None)
    assert sc(N=0) == 0                                      # nothing to do is not an error
    for kw in (dict(Cb=0), dict(N=-1), dict(ns=0), dict(b=None), dict(t=None), dict(nt=table.size - 1)):
        assert sc(**kw) == -1, kw
        assert b"sf_scatter_empirical" in lib.sf_last_error()
    big = (_lib.sf_noise_band * 1)()
    C.memmove(big, bands, C.sizeof(_lib.sf_noise_band))
    big[0].n_bins, big[0].table_offset = 257, 0
    t_big = np.arange(3 * 257, dtype=np.float32)
    assert lib.sf_scatter_empirical(p, 4, 1, big, t_big.ctypes.data_as(_lib.c_f32p), t_big.size, 1, 1, p, p, None) == -1
    assert b"256 bins" in lib.sf_last_error()
    t_huge = np.zeros(16385 + 6, np.float32)                 # above 64 KiB
    big[0].n_bins = 2
    assert lib.sf_apply_scalings(p, p, 4, 1, big, t_huge.ctypes.data_as(_lib.c_f32p), t_huge.size, p, p, None) == -1
    assert b"64 KiB" in lib.sf_last_error() and b"sf_apply_scalings" in lib.sf_last_error()
    assert lib.sf_apply_scalings(p, p, 0, 1, big, tp, table.size, p, p, None) == 0


def test_entry_points_fail_loudly_without_a_gpu():
    import torch
    from synference_amd.features import apply_scalings, scatter_empirical
    m = NC.five_models()[0]
    with pytest.raises(RuntimeError, match="GPU"):
        scatter_empirical(torch.zeros(3, 1), [m], "nJy", "AB")
    with pytest.raises(RuntimeError, match="GPU"):
        apply_scalings(torch.zeros(3, 1), torch.ones(3, 1), [m], "AB", "AB")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            m.apply_noise(np.ones(3), true_flux_units="nJy", out_units="AB")
        with pytest.raises(RuntimeError, match="GPU"):
            m.apply_scalings(np.ones(3), np.ones(3), true_flux_units="AB", out_units="AB")
    with pytest.raises(ValueError, match="disagree"):
        m.apply_scalings(np.ones(3), np.ones(3), flux_units="AB", true_flux_units="uJy", out_units="AB")


def _fitter(C_=3, N=16):
    from synference_amd import SBI_Fitter
    rng = np.random.default_rng(0)
    names = [f"F{i}" for i in range(C_)]
    return SBI_Fitter("noise", ["p0", "p1"], raw_observation_names=names, raw_observation_units="nJy",
                      raw_observation_grid=10 ** rng.uniform(2, 4, size=(C_, N)), parameter_array=rng.normal(size=(N, 2))), names


def test_fitter_refusals(monkeypatch):
    """Every ValueError of the wiring comes before the device is touched (``torch.cuda.is_available`` is patched to True so
    that the checks behind the GPU gate are reached; nothing here launches)."""
    import torch
    from synference_amd import features
    f, names = _fitter()
    models = NC.five_models()
    general = {n: models[0] for n in names}
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)

    def no_launch(*a, **k):
        from synference_amd.noise_models import pack_models as pm
        pm(a[1], a[2], a[3])
        raise AssertionError("reached the device")
    monkeypatch.setattr(features, "scatter_empirical", no_launch)
    with pytest.raises(ValueError, match="must be a dictionary"):
        f.create_feature_array_from_raw_photometry(scatter_fluxes=2, empirical_noise_models=[models[0]] * 3)
    with pytest.raises(ValueError, match="No empirical noise model found for filter F2"):
        f.create_feature_array_from_raw_photometry(scatter_fluxes=2, empirical_noise_models={"F0": models[0], "F1": models[0]})
    with pytest.raises(ValueError, match="Filter F9 in empirical_noise_models is not in phot_names"):
        f.create_feature_array_from_raw_photometry(scatter_fluxes=2, empirical_noise_models=dict(general, F9=models[0]))
    with pytest.raises(ValueError, match="asinh"):           # General models cannot return asinh magnitudes
        f.create_feature_array_from_raw_photometry(scatter_fluxes=2, empirical_noise_models=general, normed_flux_units="asinh",
                                                   asinh_softening_parameters=[5.0] * 3)
    with pytest.raises(ValueError, match="asinh"):           # Asinh models cannot return AB
        f.create_feature_array_from_raw_photometry(scatter_fluxes=2, empirical_noise_models={n: models[3] for n in names})
    with pytest.raises(ValueError, match="mixed"):
        f.create_feature_array_from_raw_photometry(scatter_fluxes=2, normed_flux_units="asinh",
                                                   empirical_noise_models={"F0": models[3], "F1": models[3], "F2": models[0]},
                                                   asinh_softening_parameters=[5.0] * 3)
    with pytest.raises(AssertionError, match="reached the device"):      # all-Asinh: no softening parameters needed
        f.create_feature_array_from_raw_photometry(scatter_fluxes=2, normed_flux_units="asinh",
                                                   empirical_noise_models={n: models[3] for n in names})
    with pytest.raises(AssertionError, match="asinh_softening_parameters must be provided"):
        f.create_feature_array_from_raw_photometry(scatter_fluxes=2, normed_flux_units="asinh",
                                                   empirical_noise_models={"F0": models[3], "F1": models[3], "F2": models[0]})


def test_missing_data_mcmc_still_refuses_model_built_arrays():
    from synference_amd.missing import MissingPhotometryHandler
    f, names = _fitter()
    f.feature_array, f.feature_names = np.zeros((8, 3), np.float32), list(names)
    f.feature_array_flags = dict(scatter_fluxes=2, empirical_noise_models={n: NC.five_models()[0] for n in names},
                                 raw_observation_names=names)
    with pytest.raises(ValueError, match="Mode 2"):
        MissingPhotometryHandler.init_from_synference(f)


# ---- the tolerance of the device comparison -----------------------------------------------------------------------------
def test_float32_model_stays_within_the_recorded_tolerance():
    """The figures behind tests/test_gpu_noise.py: on its inputs, the float32 evaluation of the model against the float64
    one, in units of each element's own scale; and the elements within 1e-5 of an SNR threshold stay within the cap."""
    _, bands, table, flux = NC.five_bands()
    bf = band_fields(bands)
    r64 = NM.scatter(bf, table, flux, NC.N_SCATTERS, NC.SEED, np.float64)
    r32 = NM.scatter(bf, table, flux, NC.N_SCATTERS, NC.SEED, np.float32)
    worst_f = worst_e = 0.0
    for c in range(5):
        ff, fe, left_out = NC.compare(r32[c]["y"], r32[c]["s"], r64[c], f"band {c}")
        print(f"band {c}: flux {ff:.3e} sigma, error {fe:.3e} ss, left out {left_out}")
        worst_f, worst_e = max(worst_f, ff), max(worst_e, fe)
    assert worst_f <= NC.TOL_FLUX_MEASURED and worst_e <= NC.TOL_ERR_MEASURED
    assert worst_f > 0.5 * NC.TOL_FLUX_MEASURED and worst_e > 0.5 * NC.TOL_ERR_MEASURED     # the record is the measurement
    lim = r64[2]["s"] == np.float32(bf[2]["err_value"])
    assert 20 < lim.sum() < 700                              # band 2 has limited and unlimited elements
    assert np.isinf(r64[0]["y"][11 * 3:12 * 3]).all() and np.isnan(r64[0]["y"][12 * 3:13 * 3]).all()
