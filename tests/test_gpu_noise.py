"""Empirical noise models on the device (csrc/sf_noise.hip) against the float64 numpy model (tests/noise_model.py): draw for
draw on one band of each kind, reproducibility, the sampled distributions, the deterministic twin, the fitter end to end, and
the rejections.  Tolerance: tests/noise_cases.py (measured on the CPU by tests/test_cpu_noise_model.py, float32 model against
float64 model on these inputs: 2.6e-2 sigma for fluxes, 3.3e-5 ss for errors; the bounds here are 4x those)."""
import numpy as np
import pytest
import torch

import noise_cases as NC
import noise_model as NM
from synference_amd import _lib
from synference_amd.features import apply_scalings, scatter_empirical
from synference_amd.noise_models import (AsinhEmpiricalUncertaintyModel, GeneralEmpiricalUncertaintyModel, band_fields,
                                         pack_models)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def five():
    """The five bands, the device output of the full call and the float64 model of it -- computed once."""
    models, bands, table, flux = NC.five_bands()
    y, s = scatter_empirical(torch.as_tensor(flux).cuda(), (bands, table), n_scatters=NC.N_SCATTERS, seed=NC.SEED)
    ref = NM.scatter(band_fields(bands), table, flux, NC.N_SCATTERS, NC.SEED)
    return dict(models=models, bands=bands, table=table, flux=flux, y=y.cpu().numpy(), s=s.cpu().numpy(), ref=ref)


def _check(y, s, ref, label):
    ff, fe, left_out = NC.compare(y, s, ref, label)
    print(f"{label}: flux {ff:.3e} sigma (bound {NC.TOL_FLUX_BOUND:.3e}), error {fe:.3e} ss (bound {NC.TOL_ERR_BOUND:.3e}), "
          f"left out {left_out}")
    assert ff <= NC.TOL_FLUX_BOUND and fe <= NC.TOL_ERR_BOUND, (label, ff, fe)


def test_draw_for_draw_on_one_band_of_each_kind(five):
    """N = 257, C = 5 (no multiple of 4: the guarded tail group), n_scatters = 3, bins 2 / 7 / 20 / 33 / 20."""
    assert five["y"].shape == five["s"].shape == (NC.N_ROWS * NC.N_SCATTERS, 5)
    for c in range(5):
        _check(five["y"][:, c], five["s"][:, c], five["ref"][c], f"band {c}")
    assert np.isinf(five["y"][33:36, 0]).all() and np.isnan(five["y"][36:39, 0]).all()     # the zero and the negative flux


@pytest.mark.parametrize("case", ["C1", "N0", "one_scatter", "C4_float4"])
def test_small_shapes(five, case):
    bf, table, flux = band_fields(five["bands"]), five["table"], five["flux"]
    sub = lambda cols: ((_lib.sf_noise_band * len(cols))(*[five["bands"][c] for c in cols]), table)      # noqa: E731
    if case == "C1":
        y, s = scatter_empirical(torch.as_tensor(flux[:, 2:3].copy()).cuda(), sub([2]), n_scatters=2, seed=9)
        ref = NM.scatter([bf[2]], table, flux[:, 2:3], 2, 9)
        _check(y.cpu().numpy()[:, 0], s.cpu().numpy()[:, 0], ref[0], "C=1")
    elif case == "N0":
        y, s = scatter_empirical(torch.zeros((0, 5), device="cuda"), (five["bands"], table), n_scatters=3, seed=1)
        assert y.shape == s.shape == (0, 5)
    elif case == "one_scatter":
        y, s = scatter_empirical(torch.as_tensor(flux).cuda(), (five["bands"], table), n_scatters=1, seed=NC.SEED)
        ref = NM.scatter(bf, table, flux, 1, NC.SEED)
        for c in range(5):
            _check(y.cpu().numpy()[:, c], s.cpu().numpy()[:, c], ref[c], f"n_scatters=1 band {c}")
    else:                                                    # C % 4 == 0: the float4 stores
        cols = [1, 2, 3, 4]
        y, s = scatter_empirical(torch.as_tensor(flux[:, cols].copy()).cuda(), sub(cols), n_scatters=3, seed=4)
        ref = NM.scatter([bf[c] for c in cols], table, flux[:, cols], 3, 4)
        for j in range(4):
            _check(y.cpu().numpy()[:, j], s.cpu().numpy()[:, j], ref[j], f"C=4 column {j}")


def test_reproducible_and_independent_of_the_launch_shape(five):
    again = scatter_empirical(torch.as_tensor(five["flux"]).cuda(), (five["bands"], five["table"]), n_scatters=NC.N_SCATTERS,
                              seed=NC.SEED)
    head = scatter_empirical(torch.as_tensor(five["flux"][:100].copy()).cuda(), (five["bands"], five["table"]),
                             n_scatters=NC.N_SCATTERS, seed=NC.SEED)
    for k, (a, h) in zip(("y", "s"), zip(again, head)):
        assert np.array_equal(a.cpu().numpy(), five[k], equal_nan=True)
        assert np.array_equal(h.cpu().numpy(), five[k][:300], equal_nan=True)


@pytest.mark.parametrize("name", list(NC.REGIME_SEEDS))
def test_distributions_on_the_device(name):
    model, f0, mu, ss = NC.regimes()[name]
    y, s = scatter_empirical(torch.full((NC.KS_ROWS, 1), f0, device="cuda"), [model], "uJy", "uJy", n_scatters=1,
                             seed=NC.REGIME_SEEDS[name])
    p_sigma, p_noise = NC.ks_pvalues(model, f0, mu, ss, y.cpu().numpy()[:, 0], s.cpu().numpy()[:, 0])
    print(f"{name}: p(sigma) {p_sigma:.3g} p(noise) {p_noise:.3g}")
    assert p_sigma > 1e-3 and p_noise > 1e-3


def test_apply_scalings_matches_the_model(five):
    """N = 300 with rows below the SNR cut and NaN rows, through one band of each kind and both unit directions."""
    rng = np.random.default_rng(3)
    models = five["models"]
    flux = (10 ** rng.uniform(1.3, 5.3, size=(300, 5))).astype(np.float32)
    err = (100.0 * np.exp(0.2 * rng.normal(size=(300, 5)))).astype(np.float32)        # SNR 0.2 .. 2000 against a cut at 3
    flux[5], err[6] = np.nan, np.nan
    flux[7, 2], flux[8, 2] = 0.0, -25.0
    bands, table = pack_models(models, [u[0] for u in NC.FIVE_UNITS], [u[1] for u in NC.FIVE_UNITS])
    y, s = apply_scalings(torch.as_tensor(flux).cuda(), torch.as_tensor(err).cuda(), (bands, table))
    y, s = y.cpu().numpy(), s.cpu().numpy()
    bf = band_fields(bands)
    for c in range(5):
        ref = NM.scalings_band(bf[c], table, flux[:, c], err[:, c])
        near = ref["margin"] < NC.SNR_MARGIN
        assert near.sum() <= NC.SNR_MAX_EXCLUDED
        for is_err, got, want in ((False, y[:, c], ref["y"]), (True, s[:, c], ref["s"])):
            got, want = got[~near].astype(np.float64), want[~near]
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[np.isinf(want)], want[np.isinf(want)])
            ok = np.isfinite(want)
            # deterministic: an error's own scale is its value, a flux's its error (its own size where the error is NaN)
            es = np.abs(ref["s"][~near][ok])
            scale = np.maximum(np.abs(want[ok]) if is_err else np.where(np.isfinite(es), es, np.abs(want[ok])), 1e-30)
            fig = float(np.max(np.abs(got[ok] - want[ok]) / scale)) if ok.any() else 0.0
            print(f"scalings band {c}: {fig:.3e}")
            assert fig <= (NC.TOL_ERR_BOUND if is_err else NC.TOL_FLUX_BOUND)
    lim = y[:, 2] == np.float32(bf[2]["limit_value"])
    assert 10 < lim.sum() < 290 and np.all(s[lim, 2] == np.float32(bf[2]["err_value"]))
    # the model's own method, true_flux_units as the alias of flux_units
    m = models[2]
    y1, s1 = m.apply_scalings(flux[:, 2], err[:, 2], true_flux_units="nJy", out_units="AB")
    assert np.array_equal(y1, y[:, 2], equal_nan=True) and np.array_equal(s1, s[:, 2], equal_nan=True)


def test_rejections_launch_nothing():
    lib = _lib.load()
    out = torch.full((8, 1), -7.0, device="cuda")
    err = torch.full((8, 1), -7.0, device="cuda")
    flux = torch.ones((8, 1), device="cuda")
    m = NC.five_models()[1]
    bands, _ = pack_models([m], "nJy", "uJy")
    stream = _lib.stream_ptr(flux.device)
    bands[0].n_bins, bands[0].table_offset = 257, 0
    t = np.linspace(1.0, 2.0, 3 * 257).astype(np.float32)
    rc = lib.sf_scatter_empirical(_lib.ptr(flux), 8, 1, bands, t.ctypes.data_as(_lib.c_f32p), t.size, 1, 1, _lib.ptr(out),
                                  _lib.ptr(err), stream)
    assert rc == -1 and b"256 bins" in lib.sf_last_error()
    bands[0].n_bins = 2
    t = np.linspace(1.0, 2.0, 16390).astype(np.float32)
    rc = lib.sf_scatter_empirical(_lib.ptr(flux), 8, 1, bands, t.ctypes.data_as(_lib.c_f32p), t.size, 1, 1, _lib.ptr(out),
                                  _lib.ptr(err), stream)
    assert rc == -1 and b"64 KiB" in lib.sf_last_error()
    rc = lib.sf_apply_scalings(_lib.ptr(flux), _lib.ptr(flux), 8, 1, bands, t.ctypes.data_as(_lib.c_f32p), t.size, _lib.ptr(out),
                               _lib.ptr(err), stream)
    assert rc == -1 and b"64 KiB" in lib.sf_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((err == -7.0).all())
    with pytest.raises(RuntimeError, match="256 bins"):
        big = GeneralEmpiricalUncertaintyModel(np.linspace(1, 2, 300), None, flux_unit="uJy", already_binned=True,
                                               bin_median_errors=np.full(300, 0.1), bin_std_errors=np.full(300, 0.01))
        scatter_empirical(flux, [big], "nJy", "uJy")


# ---- the fitter, end to end -----------------------------------------------------------------------------------------------
def _library(C_=6, N=64, seed=5):
    from synference_amd import SBI_Fitter
    rng = np.random.default_rng(seed)
    grid = (10 ** rng.uniform(2.0, 5.0, size=(C_, N))).astype(np.float64)           # nJy
    grid[2, 4] = 0.0                                        # F2 has no upper-limit rule: magnitude inf -> norm_mag_limit
    names = [f"F{i}" for i in range(C_)]
    params = rng.normal(size=(N, 3))
    f = SBI_Fitter("noise_e2e", ["p0", "p1", "p2"], raw_observation_names=names, raw_observation_grid=grid,
                   parameter_array=params, raw_observation_units="nJy")
    return f, grid, names, params


def _models(names, asinh):
    f, e = NC.mock_catalogue(4000, seed=3)
    m, me = NC.ab_of(f, e)
    out = {}
    for i, n in enumerate(names):
        if asinh:
            out[n] = AsinhEmpiricalUncertaintyModel(f, e * (1 + 0.1 * i), num_bins=12, return_noise=True)
        else:
            out[n] = GeneralEmpiricalUncertaintyModel(m, me * (1 + 0.1 * i), flux_unit="AB", num_bins=10 + i, return_noise=True,
                                                      upper_limits=bool(i % 2), treat_as_upper_limits_below=2.0,
                                                      upper_limit_flux_behaviour="upper_limit",
                                                      upper_limit_flux_err_behaviour="sig_2")
    return out


def _bounds(feat, ref):
    err = np.abs((feat - ref) / np.maximum(1.0, np.abs(ref)))
    print(f"feature array: 99.9 % quantile {np.quantile(err, 0.999):.3e}, max {err.max():.3e}")
    assert np.quantile(err, 0.999) < 2e-5 and err.max() < 2e-3, (np.quantile(err, 0.999), err.max())


def test_feature_array_with_general_models_end_to_end(tmp_path):
    f, grid, names, params = _library()
    models = _models(names, asinh=False)
    feat, fnames = f.create_feature_array_from_raw_photometry(scatter_fluxes=3, empirical_noise_models=models, seed=21,
                                                             include_errors_in_feature_array=True, normalize_method="F0",
                                                             verbose=False)
    bands, table = pack_models([models[n] for n in names], "nJy", "AB")
    ref = NM.scatter(band_fields(bands), table, grid.T.astype(np.float32), 3, 21)
    mag = np.stack([r["y"] for r in ref], axis=1)
    mag = np.where(np.isfinite(mag), mag, 50.0)
    sig = np.stack([r["s"] for r in ref], axis=1)
    norm = -2.5 * np.log10(np.repeat(grid[0], 3) * 1e-3) + 23.9
    want = np.column_stack([np.minimum(mag[:, 1:] - mag[:, :1], 50.0), sig[:, 1:], norm])
    keep = np.isfinite(want).all(axis=1)
    assert keep.sum() >= 180 and fnames == names[1:] + [f"unc_{n}" for n in names[1:]] + ["norm_F0_AB"]
    assert feat.shape == (keep.sum(), 11)
    _bounds(feat, want[keep])
    assert np.any(feat[:, 1] > 20.0)                                           # the zero flux of F2: limit minus F0
    assert np.allclose(f.fitted_parameter_array, np.repeat(params, 3, axis=0)[keep])
    flags = f.feature_array_flags
    assert flags["empirical_noise_models"] is models and f.empirical_noise_models is models
    # save_state / load_model_from_pkl bring the models back
    import pickle
    f.save_state(str(tmp_path), "t")
    with open(tmp_path / "noise_e2e_t_posterior.pkl", "wb") as fh:             # (no flow is trained here)
        pickle.dump(None, fh)
    from synference_amd import SBI_Fitter
    g = SBI_Fitter("noise_e2e", ["p0", "p1", "p2"])
    g.load_model_from_pkl(str(tmp_path), set_self=True)
    back = g.feature_array_flags["empirical_noise_models"]
    assert sorted(back) == sorted(models)
    for n in names:
        assert np.array_equal(back[n].bin_centers, models[n].bin_centers) and back[n].upper_limits == models[n].upper_limits
    # create_features_from_observations: a catalogue in the raw flux unit goes through the models' apply_scalings
    import pandas as pd
    rng = np.random.default_rng(8)
    cat_f = (10 ** rng.uniform(1.5, 4.5, size=(40, 6))).astype(np.float32)
    cat_e = (60.0 * np.exp(0.2 * rng.normal(size=(40, 6)))).astype(np.float32)
    df = pd.DataFrame({**{n: cat_f[:, i] for i, n in enumerate(names[1:], start=1)},
                       **{f"unc_{n}": cat_e[:, i] for i, n in enumerate(names[1:], start=1)},
                       "norm_F0_AB": np.full(40, 24.0, np.float32)})
    obs, removed = f.create_features_from_observations(df, flux_units="nJy")
    assert not removed.any() and obs.shape == (40, 11)
    bf = band_fields(bands)
    nf = 10 ** ((23.9 - 24.0) / 2.5)
    for i, n in enumerate(names[1:], start=1):
        r = NM.scalings_band(bf[i], table, cat_f[:, i], cat_e[:, i])
        assert (r["margin"] > NC.SNR_MARGIN).all()
        assert np.allclose(obs[:, i - 1], np.minimum(r["y"] - nf, 50.0), rtol=0, atol=2e-5 * 30)
        assert np.allclose(obs[:, 5 + i - 1], r["s"], rtol=2e-5, atol=1e-7)
    with pytest.raises(AssertionError, match="do not match"):                  # without models the units must already agree
        f.create_features_from_observations(df, flux_units="nJy", override_transformations={"empirical_noise_models": None})
    with pytest.raises(ValueError, match="Mode 2"):
        f.fit_catalogue(df, flux_units="nJy", missing_data_mcmc=True)


def test_feature_array_with_asinh_models_needs_no_softening_parameters():
    f, grid, names, params = _library()
    models = _models(names, asinh=True)
    feat, fnames = f.create_feature_array_from_raw_photometry(scatter_fluxes=3, empirical_noise_models=models, seed=22,
                                                             include_errors_in_feature_array=True, normed_flux_units="asinh",
                                                             verbose=False)
    bands, table = pack_models([models[n] for n in names], "nJy", "asinh")
    ref = NM.scatter(band_fields(bands), table, grid.T.astype(np.float32), 3, 22)
    want = np.column_stack([np.stack([r["y"] for r in ref], axis=1), np.stack([r["s"] for r in ref], axis=1)])
    assert feat.shape == want.shape == (192, 12) and fnames == names + [f"unc_{n}" for n in names]
    _bounds(feat, want)
    assert f.fitted_parameter_array.shape == (192, 3) and np.allclose(f.fitted_parameter_array, np.repeat(params, 3, axis=0))
    assert f.feature_array_flags["empirical_noise_models"] is models and f.feature_units == ["asinh"] * 12
