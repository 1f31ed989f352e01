"""Numpy model of csrc/sf_spectra.hip and of ``SBI_Fitter.create_feature_array_from_raw_spectra`` (TEST INFRASTRUCTURE):
library spectra -> observed-frame spectral features, restated step by step and evaluated in float64 (the yardstick) or,
``dtype=np.float32``, with the flux, the Gaussian weights and the sums of the convolution and of the rebinning in float32 as
the kernel keeps them (wavelengths, bin edges, overlap fractions, sigma and the half-width stay float64 in both).

What it restates of the reference (src/synference): utils.py:185-254 ``transform_spectrum`` (212-213 the redshifted grid,
217-238 the kernel width in pixels, 241-243 the convolution, 246-252 the rebinning), utils.py:129-182
``convolve_variable_width_gaussian``, sbi_runner.py:1096-1178 ``_apply_flux_normalization`` and 1180-1427
``create_feature_array_from_raw_spectra``.  The rebinning is SpectRes with ``fill=0.0`` restated from its paper (Carnall
2017, arXiv:1705.05165, section 2): bin edges from the bin centres, a new bin takes the width-weighted mean of the old bins it
overlaps, the first and the last of them weighted by the overlapping part of their width.
"""
import numpy as np

FWHM_PER_SIGMA = 2 * np.sqrt(2 * np.log(2))
UNITS_PER_JY = {"Jy": 1.0, "mJy": 1.0e3, "uJy": 1.0e6, "nJy": 1.0e9}
_trapz = getattr(np, "trapezoid", None) or np.trapz


def sigma_pixels(theory_wave, z, resolution_curve_wave, resolution_curve_r, theory_r=np.inf):
    """ref: utils.py:212-238 -- the float64 Gaussian sigma of every theory pixel, in pixels of the redshifted grid."""
    w = np.asarray(theory_wave, np.float64)
    wz = w * (1 + z)                                                                           # 212
    r_inst = np.interp(wz, np.asarray(resolution_curve_wave, np.float64), np.asarray(resolution_curve_r, np.float64))  # 217
    s_inst = wz / r_inst / FWHM_PER_SIGMA                                                      # 218-219
    tr = np.asarray(theory_r, np.float64)
    r_th = np.full_like(wz, float(tr)) if tr.ndim == 0 else tr                                 # 222-225 (interp onto itself)
    with np.errstate(divide="ignore"):
        s_th = wz / r_th / FWHM_PER_SIGMA                                                      # 226-227
    sq = s_inst ** 2 - s_th ** 2                                                               # 230
    sq[sq < 0] = 0                                                                             # 231
    scale = np.median(np.diff(wz))                                                             # 234
    return np.sqrt(sq) / scale if scale != 0 else np.zeros_like(wz)                            # 232, 236-238


def convolve(flux, sigma, trunc=4.0, dtype=np.float64):
    """ref: utils.py:129-182 -- ``sigma`` float64 [L]; the weights and the sum in ``dtype``.  The taps are summed in the
    kernel's order: the centre, then the pairs at distance 1, 2, ... (w(x) = w(-x))."""
    dt = dtype
    f = np.asarray(flux, dt)
    L = len(f)
    out = np.zeros(L, dt)
    for i in range(L):
        s = float(sigma[i])
        if s <= 0.01:                                                                          # 151-153
            out[i] = f[i]
            continue
        h = int(np.ceil(s * trunc))                                                            # 156
        x = np.arange(1, h + 1)
        wt = np.exp(dt(-0.5 / (s * s)) * (x.astype(dt) * x.astype(dt)))                        # 160-161, one side
        lo, hi = np.maximum(i - x, 0), np.minimum(i + x, L - 1)                                # 172-176 'nearest' padding
        if dt == np.float64:
            acc, wsum = f[i] + np.sum(wt * (f[lo] + f[hi])), 1.0 + 2.0 * np.sum(wt)
        else:
            acc, wsum = f[i], dt(1)
            for k in range(h):
                acc = dt(acc + wt[k] * dt(f[lo[k]] + f[hi[k]]))
                wsum = dt(wsum + dt(2) * wt[k])
        out[i] = acc / wsum                                                                    # 162, 178
    return out


def bin_edges(wave):
    """SpectRes section 2: interior edges at the midpoints, the outer two half a neighbouring spacing beyond the ends."""
    w = np.asarray(wave, np.float64)
    if len(w) < 2:
        raise ValueError("a wavelength grid needs at least 2 pixels: one pixel has no bin width")
    e = np.empty(len(w) + 1)
    e[0] = w[0] - (w[1] - w[0]) / 2
    e[-1] = w[-1] + (w[-1] - w[-2]) / 2
    e[1:-1] = (w[1:] + w[:-1]) / 2
    return e


def rebin(new_wave, old_wave, flux, fill=0.0, dtype=np.float64):
    """SpectRes: ``flux`` on ``old_wave`` -> the mean flux in the bins of ``new_wave``; edges and overlaps float64."""
    dt = dtype
    oe, ne = bin_edges(old_wave), bin_edges(new_wave)
    ow = np.diff(oe)
    f = np.asarray(flux, dt)
    L = len(f)
    out = np.zeros(len(ne) - 1, dt)
    for j in range(len(out)):
        nl, nr = ne[j], ne[j + 1]
        if nl < oe[0] or nr > oe[-1]:
            out[j] = fill
            continue
        start = min(int(np.searchsorted(oe, nl, side="right")) - 1, L - 1)    # the last old bin with oe[start] <= nl
        stop = start
        while stop < L - 1 and oe[stop + 1] < nr:                             # the first old bin with oe[stop + 1] >= nr
            stop += 1
        if start == stop:
            out[j] = f[start]
            continue
        wd = ow[start:stop + 1].copy()
        wd[0] = (oe[start + 1] - nl) / (oe[start + 1] - oe[start]) * wd[0]
        wd[-1] = (nr - oe[stop]) / (oe[stop + 1] - oe[stop]) * wd[-1]
        if dt == np.float64:
            out[j] = np.sum(wd * f[start:stop + 1]) / np.sum(wd)
        else:
            num = dt(0)
            for k in range(len(wd)):
                num = dt(num + dt(wd[k]) * f[start + k])
            out[j] = num / dt(np.sum(wd))
    return out


def transform_spectrum(theory_wave, theory_flux, z, observed_wave, resolution_curve_wave, resolution_curve_r,
                       theory_r=np.inf, trunc_constant=4.0, dtype=np.float64):
    """ref: utils.py:185-254, one spectrum."""
    w = np.asarray(theory_wave, np.float64)
    sg = sigma_pixels(w, z, resolution_curve_wave, resolution_curve_r, theory_r)
    conv = convolve(theory_flux, sg, trunc_constant, dtype)                                    # 241-243 (flux not / (1 + z))
    return np.asarray(observed_wave, np.float64), rebin(observed_wave, w * (1 + z), conv, 0.0, dtype)   # 246-252


def filter_arrays(filt):
    """A bandpass filter -> (wavelength in um, transmission): an object with ``.lam`` and ``.transmission`` or a pair."""
    if hasattr(filt, "lam") and hasattr(filt, "transmission"):
        lam = filt.lam
        lam = lam.to_value("um") if hasattr(lam, "to_value") else lam
        return np.asarray(lam, np.float64), np.asarray(filt.transmission, np.float64)
    lam, tr = filt
    return np.asarray(lam, np.float64), np.asarray(tr, np.float64)


def norm_factor(wave, flux, method, parameters):
    """ref: sbi_runner.py:1119-1163 -- the scalar a spectrum is divided by."""
    wave, flux = np.asarray(wave, np.float64), np.asarray(flux, np.float64)
    if method == "tophat":
        c, wd = parameters["center"], parameters["width"]
        m = (wave >= c - wd / 2.0) & (wave <= c + wd / 2.0)                                     # 1127-1128
        return float(np.mean(flux[m])) if m.sum() > 0 else 0.0                                 # 1129-1132
    if method == "bandpass":
        lam, tr = filter_arrays(parameters["filter"])
        t = np.interp(wave, lam, tr, left=0.0, right=0.0)                                      # 1154-1156
        den = _trapz(t, x=wave)                                                              # 1161
        return float(_trapz(flux * t, x=wave) / den) if den > 0 else 0.0                     # 1160, 1163
    raise ValueError(f"Unknown flux_norm_method: {method}")


def normalise(wave, flux, method, parameters):
    """ref: sbi_runner.py:1168-1176."""
    fac = norm_factor(wave, flux, method, parameters)
    return np.asarray(flux, np.float64) / fac if fac != 0 else np.zeros(len(flux))


def to_units(flux, grid_unit, normed_flux_units):
    """ref: sbi_runner.py:1361-1367 with the unit strings of ``noise_models.PHYSICAL_UNITS`` in place of unyt."""
    f = np.asarray(flux, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if normed_flux_units.startswith("log10 "):
            return np.log10(f * (UNITS_PER_JY[normed_flux_units[6:]] / UNITS_PER_JY[grid_unit]))
        if normed_flux_units == "AB":
            return -2.5 * np.log10(f * (1.0 / UNITS_PER_JY[grid_unit])) + 8.90
        return f * (UNITS_PER_JY[normed_flux_units] / UNITS_PER_JY[grid_unit])


def feature_array(grid, wave, parameter_array, parameter_names, grid_unit="nJy", extra_features=("redshift",),
                  crop_wavelength_range=None, normed_flux_units="AB", flux_norm_method=None, flux_norm_parameters=None,
                  resample_wavelengths=None, inst_resolution_wavelengths=None, inst_resolution_r=None, theory_r=np.inf,
                  min_flux_value=-np.inf, max_flux_value=np.inf, dtype=np.float64):
    """ref: sbi_runner.py:1276-1396 -- ``grid`` (L, N) as the library holds it -> (features (N, M + extras) float64, the M
    wavelengths)."""
    grid = np.asarray(grid, np.float64)
    wave = np.asarray(wave, np.float64)
    pars = flux_norm_parameters or {}
    names = list(parameter_names)
    rest = pars.get("rest_frame", False)                                                       # 1282
    N = grid.shape[1]
    if flux_norm_method is not None and rest:                                                  # 1284-1291
        grid = np.stack([normalise(wave, grid[:, i], flux_norm_method, pars) for i in range(N)], axis=1)
    if "redshift" in names:                                                                    # 1293-1338
        ow = np.asarray(resample_wavelengths, np.float64)
        if crop_wavelength_range is not None:
            ow = ow[(ow >= crop_wavelength_range[0]) & (ow <= crop_wavelength_range[1])]        # 1312-1315
        zs = np.asarray(parameter_array)[:, names.index("redshift")]
        grid = np.stack([transform_spectrum(wave, grid[:, i], zs[i], ow, inst_resolution_wavelengths, inst_resolution_r,
                                            theory_r, dtype=dtype)[1].astype(np.float64) for i in range(N)], axis=1)
        wavs, mask = ow, np.ones(len(ow), bool)
    elif crop_wavelength_range is not None:                                                    # 1339-1340
        wavs, mask = wave, (wave >= crop_wavelength_range[0]) & (wave <= crop_wavelength_range[1])
    else:
        wavs, mask = wave, np.ones(len(wave), bool)
    if flux_norm_method is not None and not rest:                                              # 1344-1351 (before the crop)
        grid = np.stack([normalise(wavs, grid[:, i], flux_norm_method, pars) for i in range(N)], axis=1)
    feat = to_units(grid, grid_unit, normed_flux_units)[mask, :]                               # 1361-1369
    with np.errstate(invalid="ignore"):
        feat = np.clip(feat, min_flux_value, max_flux_value)                                   # 1376-1381
    extras = [np.asarray(parameter_array, np.float64)[:, names.index(e)] for e in extra_features]   # 1388-1394
    return np.concatenate([feat.T] + [e.reshape(-1, 1) for e in extras], axis=1), wavs[mask]
