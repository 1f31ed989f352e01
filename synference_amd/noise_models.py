"""Empirical photometric noise models: p(sigma | flux) per filter, learned from an observed catalogue.

Host side (numpy only): the fit -- binned median / standard deviation of the catalogue's errors against its fluxes
(ref: src/synference/noise_models.py:285-320 ``_compute_bins_from_data``, with ``scipy.stats.binned_statistic``'s edge rule
restated), the flux at which a source reaches the upper-limit SNR (782-816 ``_setup_upper_limit_interpolator``), the asinh
model's softening (483-505) -- and the packing of a list of models into ``sf_noise_band`` structs plus one float table
(include/synference_hip.h).  Applying a model -- ``apply_noise`` (507-560, 818-880) and ``apply_scalings`` (562-592,
1074-1099) -- runs on the device (csrc/sf_noise.hip through ``synference_amd.features``): GPU only, like every other
catalogue tool of this package.

Units are plain strings: "AB", "asinh", "Jy", "mJy", "uJy", "nJy"; anything else is a ``ValueError``.  The models pickle
through ``__getstate__`` / ``__setstate__`` as in the reference (392-404) and so travel inside ``feature_array_flags``; the
reference's side HDF5 file is out of scope.  Deviations from the reference: DESIGN.md section 13.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Sequence

import numpy as np

from ._lib import sf_noise_band

PHYSICAL_UNITS = {"Jy": 1.0, "mJy": 1.0e3, "uJy": 1.0e6, "nJy": 1.0e9}      # units per Jy
KIND_GENERAL, KIND_ASINH = 0, 1
SPACE_PHYSICAL, SPACE_AB, SPACE_ASINH = 0, 1, 2
FLUX_SCATTER, FLUX_LIMIT, FLUX_NUMBER = 0, 1, 2


def unit_per_jy(unit) -> float:
    """How many of ``unit`` make one Jy."""
    if not isinstance(unit, str) or unit not in PHYSICAL_UNITS:
        raise ValueError(f"unit {unit!r} is not a physical flux unit: one of {sorted(PHYSICAL_UNITS)}")
    return PHYSICAL_UNITS[unit]


def check_unit(unit, allowed=("AB", "asinh") + tuple(PHYSICAL_UNITS)) -> str:
    if not isinstance(unit, str) or unit not in allowed:
        raise ValueError(f"unit {unit!r} is not supported here: one of {list(allowed)}")
    return unit


def ab_zero_point(unit: str) -> float:
    """zp of a physical unit: m_AB = zp - 2.5 log10(f_unit) (8.9 for Jy, 23.9 for uJy)."""
    return 8.90 + 2.5 * np.log10(unit_per_jy(unit))


def binned_statistics(x: np.ndarray, values: np.ndarray, edges: np.ndarray):
    """Median, standard deviation (ddof 0) and count of ``values`` per bin of ``x``, with the edge rule of
    ``scipy.stats.binned_statistic``: bin i is [edges[i], edges[i+1]), the last bin is closed on the right -- a value that
    equals the last edge when both are rounded to int(-log10(smallest bin width)) + 6 decimals moves one bin down --
    and values outside all edges are ignored.  Empty bins: NaN, count 0."""
    x, values, edges = np.asarray(x, np.float64), np.asarray(values, np.float64), np.asarray(edges, np.float64)
    nb = len(edges) - 1
    idx = np.digitize(x, edges)
    decimal = int(-np.log10(np.diff(edges).min())) + 6
    idx[np.around(x, decimal) == np.around(edges[-1], decimal)] -= 1
    med, std, cnt = np.full(nb, np.nan), np.full(nb, np.nan), np.zeros(nb)
    order = np.argsort(idx, kind="stable")
    bounds = np.searchsorted(idx[order], np.arange(1, nb + 2))
    for i in range(nb):
        v = values[order[bounds[i]:bounds[i + 1]]]
        cnt[i] = len(v)
        if len(v):
            med[i], std[i] = np.median(v), np.std(v)
    return med, std, cnt


def interp_table(x, centers, values, extrapolate: bool):
    """Linear interpolation over ascending ``centers``: outside them the end values, or the end segments continued."""
    x = np.asarray(x, np.float64)
    c, v = np.asarray(centers, np.float64), np.asarray(values, np.float64)
    if not extrapolate:
        return np.interp(x, c, v)
    lo = np.clip(np.searchsorted(c, x, side="right") - 1, 0, len(c) - 2)
    return v[lo] + (x - c[lo]) * (v[lo + 1] - v[lo]) / (c[lo + 1] - c[lo])


class UncertaintyModel:
    """Base: the static unit conversions (ref: noise_models.py:55-73) on plain numbers in Jy."""

    def __init__(self, return_noise: bool = False, **kwargs: Any) -> None:
        self.return_noise = return_noise

    @staticmethod
    def ab_to_jy(magnitude):
        return 10 ** (-0.4 * (np.asarray(magnitude, np.float64) - 8.90))

    @staticmethod
    def jy_to_ab(flux_jy):
        return -2.5 * np.log10(np.asarray(flux_jy, np.float64)) + 8.90

    @staticmethod
    def ab_err_to_jy(magnitude_err, flux_jy):
        return (np.asarray(flux_jy, np.float64) * np.asarray(magnitude_err, np.float64) * np.log(10)) / 2.5

    @staticmethod
    def jy_err_to_ab(flux_err_jy, flux_jy):
        return np.abs((2.5 / np.log(10)) * (np.asarray(flux_err_jy, np.float64) / np.asarray(flux_jy, np.float64)))


def f_jy_to_asinh(f_jy, f_b):
    """ref: utils.py:672."""
    f_jy = np.asarray(f_jy, np.float64)
    return -2.5 * np.log10(np.e) * (np.arcsinh(f_jy / (2 * f_b)) + np.log(f_b / 3631.0))


def f_jy_err_to_asinh(f_jy, f_jy_err, f_b):
    """ref: utils.py:704."""
    f_jy = np.asarray(f_jy, np.float64)
    return 2.5 * np.log10(np.e) * np.asarray(f_jy_err, np.float64) / np.sqrt(f_jy ** 2 + (2 * f_b) ** 2)


class EmpiricalUncertaintyModel(UncertaintyModel):
    """Binned p(sigma | flux): ``bin_centers``, ``median_error_in_bin``, ``std_error_in_bin`` (ref: 262-404)."""

    def __init__(self, extrapolate: bool = False, min_samples_per_bin: int = 10, num_bins: int = 20, log_bins: bool = True,
                 **kwargs: Any):
        super().__init__(**kwargs)
        self.extrapolate = extrapolate
        self._min_samples_per_bin = min_samples_per_bin
        self._num_bins = num_bins
        self._log_bins = log_bins
        self.bin_centers = None
        self.median_error_in_bin = None
        self.std_error_in_bin = None

    def _compute_bins_from_data(self, fluxes, errors, precomputed_bins=None):
        fluxes, errors = np.asarray(fluxes, np.float64), np.asarray(errors, np.float64)
        if precomputed_bins is not None:
            bins = np.asarray(precomputed_bins, np.float64)
        else:
            valid = np.isfinite(fluxes)
            if not np.any(valid):
                raise ValueError("No valid finite data to build bins.")
            f = fluxes[valid]
            if self._log_bins:
                if not np.any(f > 0):
                    raise ValueError("Log-binning requires positive flux values.")
                bins = np.logspace(np.log10(np.min(f[f > 0])), np.log10(np.max(f)), self._num_bins + 1)
            else:
                bins = np.linspace(np.min(f), np.max(f), self._num_bins + 1)
        med, std, cnt = binned_statistics(fluxes, errors, bins)
        centers = (bins[:-1] + bins[1:]) / 2.0
        ok = cnt >= self._min_samples_per_bin
        if np.sum(ok) < 2:
            raise ValueError("Could not create enough valid bins for interpolation.")
        self.bin_centers, self.median_error_in_bin, self.std_error_in_bin = centers[ok], med[ok], std[ok]

    def _tables(self):
        """The three tables, ascending in the centres, float64."""
        if self.bin_centers is None or len(self.bin_centers) < 2:
            raise AttributeError("Binned data not found. Cannot create interpolators.")
        c = np.asarray(self.bin_centers, np.float64)
        order = np.argsort(c, kind="stable")
        c = c[order]
        if not (np.all(np.isfinite(c)) and np.all(np.diff(c) > 0)):
            raise ValueError("bin_centers must be finite and distinct")
        return c, np.asarray(self.median_error_in_bin, np.float64)[order], np.asarray(self.std_error_in_bin, np.float64)[order]

    def _mu_sigma_interpolator(self, x):
        c, m, _ = self._tables()
        return interp_table(x, c, m, bool(getattr(self, "extrapolate", False)))

    def _sigma_sigma_interpolator(self, x):
        c, _, s = self._tables()
        return np.maximum(0, interp_table(x, c, s, bool(getattr(self, "extrapolate", False))))

    def __getstate__(self) -> Dict[str, Any]:
        return self.__dict__.copy()

    def __setstate__(self, state: Dict[str, Any]) -> None:
        self.__dict__.update(state)

    # ---- the device calls ---------------------------------------------------------------------------------------------
    def _band(self, in_unit: Optional[str], out_unit: Optional[str]) -> dict:
        raise NotImplementedError

    def apply_noise(self, flux, true_flux_units: Optional[str] = None, out_units: Optional[str] = None, seed: int = 0):
        """Scatter ``flux`` (1-D, in ``true_flux_units``) through the model on the device: the noisy flux in ``out_units``,
        and its error too with ``return_noise``.  Randomness: Philox stream 6 under ``seed`` (element i is output row i)."""
        from .features import scatter_empirical
        f = _device_column(flux, "apply_noise")
        y, s = scatter_empirical(f, [self], true_flux_units, out_units, n_scatters=1, seed=seed)
        y, s = y.reshape(-1).cpu().numpy(), s.reshape(-1).cpu().numpy()
        return (y, s) if self.return_noise else y

    def apply_scalings(self, flux, error, flux_units: Optional[str] = None, out_units: Optional[str] = None,
                       true_flux_units: Optional[str] = None):
        """The deterministic transformations of an observed (flux, error) pair: units, SNR cut, error rule, clip.
        ``true_flux_units`` is an alias of ``flux_units``."""
        from .features import apply_scalings
        if flux_units is None:
            flux_units = true_flux_units
        elif true_flux_units is not None and true_flux_units != flux_units:
            raise ValueError("flux_units and its alias true_flux_units disagree")
        f, e = _device_column(flux, "apply_scalings"), _device_column(error, "apply_scalings")
        y, s = apply_scalings(f, e, [self], flux_units, out_units)
        return y.reshape(-1).cpu().numpy(), s.reshape(-1).cpu().numpy()


def _device_column(a, who):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(f"{who} runs on the GPU (no CPU fallback)")
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float32))
    return t.to("cuda", torch.float32).reshape(-1, 1)


class GeneralEmpiricalUncertaintyModel(EmpiricalUncertaintyModel):
    """ref: noise_models.py:638-1099 -- tables over AB magnitudes or a physical unit, optional upper-limit rules."""

    def __init__(self, observed_fluxes, observed_errors, flux_unit: str = "AB", interpolation_flux_unit: Optional[str] = None,
                 already_binned: bool = False, bin_median_errors=None, bin_std_errors=None, flux_bins=None,
                 min_flux_for_binning: Optional[float] = None, sigma_clip: Optional[float] = None,
                 min_flux_error: float = 0.0, max_flux_error: float = np.inf, error_type: str = "empirical",
                 upper_limits: bool = False, treat_as_upper_limits_below: Optional[float] = None,
                 upper_limit_flux_behaviour="scatter_limit", upper_limit_flux_err_behaviour: str = "flux", **kwargs: Any):
        super().__init__(**kwargs)
        self.flux_unit = check_unit(flux_unit, ("AB",) + tuple(PHYSICAL_UNITS))
        self.interpolation_flux_unit = check_unit(interpolation_flux_unit if interpolation_flux_unit else flux_unit,
                                                  ("AB",) + tuple(PHYSICAL_UNITS))
        self.sigma_clip = sigma_clip
        self.min_flux_error = 0.0 if min_flux_error is None else min_flux_error
        self.max_flux_error = np.inf if max_flux_error is None else max_flux_error
        self.error_type = error_type
        self.upper_limits = upper_limits
        self.treat_as_upper_limits_below = treat_as_upper_limits_below
        self.upper_limit_flux_behaviour = upper_limit_flux_behaviour
        self.upper_limit_flux_err_behaviour = upper_limit_flux_err_behaviour
        self.upper_limit_value = None
        self._snr_x_data = self._snr_y_data = None
        if already_binned:
            self.bin_centers = np.asarray(observed_fluxes, np.float64)
            self.median_error_in_bin = np.asarray(bin_median_errors, np.float64)
            self.std_error_in_bin = np.asarray(bin_std_errors, np.float64)
            self._tables()
            return
        f, e = self._convert_units(np.asarray(observed_fluxes, np.float64), np.asarray(observed_errors, np.float64))
        valid = np.isfinite(f) & np.isfinite(e) & (e > 0)
        if min_flux_for_binning is not None:
            valid &= f > min_flux_for_binning
        self._compute_bins_from_data(f[valid], e[valid], precomputed_bins=flux_bins)
        if self.upper_limits:
            self._setup_upper_limit_interpolator(f[valid], e[valid])

    def _convert_units(self, fluxes, errors, fluxes_unit=None):
        """(flux, error) from ``fluxes_unit`` (default: the model's ``flux_unit``) to the interpolation unit (ref: 747-780)."""
        src = check_unit(self.flux_unit if fluxes_unit is None else fluxes_unit, ("AB",) + tuple(PHYSICAL_UNITS))
        dst = self.interpolation_flux_unit
        with np.errstate(divide="ignore", invalid="ignore"):
            if src == dst:
                return fluxes, errors
            if src == "AB":
                fj = self.ab_to_jy(fluxes)
                return fj * unit_per_jy(dst), self.ab_err_to_jy(errors, fj) * unit_per_jy(dst)
            if dst == "AB":
                return self.jy_to_ab(fluxes / unit_per_jy(src)), self.jy_err_to_ab(errors, fluxes)
            k = unit_per_jy(dst) / unit_per_jy(src)
            return fluxes * k, errors * k

    def _setup_upper_limit_interpolator(self, fluxes, errors):
        """ref: 782-816 -- log10(flux in Jy) against log10(SNR), linear with linear extrapolation, read at the threshold."""
        if self.interpolation_flux_unit == "AB":
            fj = self.ab_to_jy(fluxes)
            ej = self.ab_err_to_jy(errors, fj)
        else:
            fj, ej = fluxes / unit_per_jy(self.interpolation_flux_unit), errors / unit_per_jy(self.interpolation_flux_unit)
        with np.errstate(divide="ignore", invalid="ignore"):
            snr = fj / ej
        valid = np.isfinite(snr) & (snr > 0) & np.isfinite(fj) & (fj > 0)
        if np.sum(valid) < 2:
            return
        order = np.argsort(snr[valid])
        self._snr_x_data = np.log10(snr[valid][order])
        self._snr_y_data = np.log10(fj[valid][order])
        ul_jy = 10 ** self.log_snr_interpolator(np.log10(self.treat_as_upper_limits_below))
        self.upper_limit_value = float(self.jy_to_ab(ul_jy) if self.interpolation_flux_unit == "AB"
                                       else ul_jy * unit_per_jy(self.interpolation_flux_unit))

    def log_snr_interpolator(self, log_snr):
        if self._snr_x_data is None:
            raise ValueError("SNR interpolator is not available for 'sig_X' error behaviour in flux space.")
        return interp_table(log_snr, self._snr_x_data, self._snr_y_data, True)

    def _replacement_error(self):
        """The one number that ``_apply_error_behaviour`` (ref: 925-957) writes into limited elements, or None when the
        behaviour is not a recognised one (the reference then leaves the errors as they are)."""
        beh = self.upper_limit_flux_err_behaviour
        if beh == "flux":
            return float(self._mu_sigma_interpolator(self.upper_limit_value))
        if beh == "upper_limit":
            return float(self.upper_limit_value)
        if beh == "max":
            return float(self.max_flux_error)
        if isinstance(beh, str) and beh.startswith("sig_"):
            sig = float(beh.split("_")[1])
            if self.interpolation_flux_unit == "AB":
                return float((2.5 / np.log(10)) / sig)
            f_int = 10 ** self.log_snr_interpolator(np.log10(sig)) * unit_per_jy(self.interpolation_flux_unit)
            return float(self._mu_sigma_interpolator(f_int))
        return None

    def _band(self, in_unit, out_unit):
        in_unit = check_unit(self.flux_unit if in_unit is None else in_unit)
        out_unit = check_unit(self.flux_unit if out_unit is None else out_unit)
        if "asinh" in (in_unit, out_unit):
            raise ValueError("a GeneralEmpiricalUncertaintyModel neither reads nor returns asinh magnitudes: use an "
                             "AsinhEmpiricalUncertaintyModel for normed_flux_units='asinh'")
        u = self.interpolation_flux_unit
        phys = lambda x: x != "AB"   # noqa: E731
        c, med, std = self._tables()
        d = dict(kind=KIND_GENERAL, interp_space=SPACE_AB if u == "AB" else SPACE_PHYSICAL,
                 in_space=SPACE_AB if in_unit == "AB" else SPACE_PHYSICAL,
                 out_space=SPACE_AB if out_unit == "AB" else SPACE_PHYSICAL, extrapolate=int(bool(self.extrapolate)),
                 resample=int(self.error_type == "observed"), upper_limits=int(bool(self.upper_limits)),
                 sigma_clip=-1.0 if self.sigma_clip is None else float(self.sigma_clip),
                 in_to_unit=unit_per_jy(u) / unit_per_jy(in_unit) if phys(u) and phys(in_unit) else 1.0,
                 unit_to_out=unit_per_jy(out_unit) / unit_per_jy(u) if phys(u) and phys(out_unit) else 1.0,
                 zp_in=ab_zero_point(in_unit) if phys(in_unit) else 8.9, zp_unit=ab_zero_point(u) if phys(u) else 8.9,
                 zp_out=ab_zero_point(out_unit) if phys(out_unit) else 8.9, in_to_jy=1.0 / unit_per_jy(in_unit) if phys(in_unit) else 1.0,
                 unit_per_jy=unit_per_jy(u) if phys(u) else 1.0, jy_per_unit=1.0 / unit_per_jy(u) if phys(u) else 1.0,
                 min_err=float(self.min_flux_error), max_err=float(self.max_flux_error))
        if self.upper_limits:
            if self.treat_as_upper_limits_below is None:
                raise ValueError("upper_limits=True needs treat_as_upper_limits_below")
            d["snr_threshold"] = float(self.treat_as_upper_limits_below)
            if self.upper_limit_value is not None:
                d["has_limit"], d["limit_value"] = 1, float(self.upper_limit_value)
                beh = self.upper_limit_flux_behaviour
                if beh == "scatter_limit":
                    d["flux_rule"] = FLUX_SCATTER
                elif beh == "upper_limit":
                    d["flux_rule"] = FLUX_LIMIT
                else:
                    d["flux_rule"], d["flux_number"] = FLUX_NUMBER, float(beh)
                d["std_at_limit"] = float(self._sigma_sigma_interpolator(self.upper_limit_value))
                err = self._replacement_error()
                if err is not None:
                    d["replace_err"], d["err_value"] = 1, err
        d["tables"] = (c, med, std)
        return d


class AsinhEmpiricalUncertaintyModel(EmpiricalUncertaintyModel):
    """ref: noise_models.py:443-635 -- asinh magnitudes out; tables over asinh magnitudes or a physical unit;
    ``b = asinh_b_factor * median(error_jy)`` in Jy."""

    def __init__(self, observed_phot_jy=None, observed_phot_errors_jy=None, asinh_b_factor: float = 5.0,
                 error_type: str = "empirical", min_flux_error: Optional[float] = None, max_flux_error: Optional[float] = None,
                 interpolation_flux_unit: str = "asinh", **kwargs: Any):
        super().__init__(**kwargs)
        self.error_type = error_type
        self.min_flux_error = min_flux_error if min_flux_error is not None else 0.0
        self.max_flux_error = max_flux_error if max_flux_error is not None else np.inf
        self.interpolation_flux_unit = check_unit(interpolation_flux_unit, ("asinh",) + tuple(PHYSICAL_UNITS))
        self.b = None
        if observed_phot_jy is not None and observed_phot_errors_jy is not None:
            f, e = np.asarray(observed_phot_jy, np.float64), np.asarray(observed_phot_errors_jy, np.float64)
            valid = np.isfinite(f) & np.isfinite(e)
            f, e = f[valid], e[valid]
            self.b = float(asinh_b_factor * np.median(e))
            if self.interpolation_flux_unit == "asinh":
                self._compute_bins_from_data(f_jy_to_asinh(f, self.b), f_jy_err_to_asinh(f, e, self.b))
            else:
                k = unit_per_jy(self.interpolation_flux_unit)
                self._compute_bins_from_data(f * k, e * k)

    def _band(self, in_unit, out_unit):
        in_unit = check_unit("Jy" if in_unit is None else in_unit, ("AB",) + tuple(PHYSICAL_UNITS))
        if out_unit is not None and out_unit != "asinh":
            raise ValueError(f"an AsinhEmpiricalUncertaintyModel returns asinh magnitudes, not {out_unit!r}: use "
                             "normed_flux_units='asinh'")
        if self.b is None or not self.b > 0:
            raise ValueError("the asinh model has no softening b: it was built without data")
        u = self.interpolation_flux_unit
        in_space = self.interpolation_flux_unit == "asinh"
        d = dict(kind=KIND_ASINH, interp_space=SPACE_ASINH if in_space else SPACE_PHYSICAL,
                 in_space=SPACE_AB if in_unit == "AB" else SPACE_PHYSICAL, out_space=SPACE_ASINH,
                 extrapolate=int(bool(self.extrapolate)),
                 resample=int(self.error_type != "empirical") if in_space else int(self.error_type == "empirical"),
                 in_to_jy=1.0 / unit_per_jy(in_unit) if in_unit != "AB" else 1.0,
                 unit_per_jy=1.0 if in_space else unit_per_jy(u), jy_per_unit=1.0 if in_space else 1.0 / unit_per_jy(u),
                 b_jy=float(self.b), sigma_clip=-1.0, min_err=float(self.min_flux_error), max_err=float(self.max_flux_error),
                 zp_in=8.9, zp_unit=8.9, zp_out=8.9, in_to_unit=1.0, unit_to_out=1.0)
        d["tables"] = self._tables()
        return d


def pack_models(models: Sequence[EmpiricalUncertaintyModel], in_unit: Optional[str], out_unit: Optional[str]):
    """One ``sf_noise_band`` per model (= per photometry column) and the float32 table that holds, band after band,
    ``centers[n]``, ``median[n]``, ``std[n]``.  ``in_unit`` / ``out_unit``: one unit for all, or one per model; None: each
    model's own default."""
    models = list(models)
    for m in models:
        if not isinstance(m, EmpiricalUncertaintyModel):
            raise TypeError(f"Invalid empirical noise model type: {type(m)}.")
    one_out_unit = out_unit is None or isinstance(out_unit, str)
    if one_out_unit and len({isinstance(m, AsinhEmpiricalUncertaintyModel) for m in models}) > 1:
        raise ValueError("General and Asinh noise models cannot be mixed in one call: their outputs are in different units")
    in_unit, out_unit = ([u] * len(models) if u is None or isinstance(u, str) else list(u) for u in (in_unit, out_unit))
    if len(in_unit) != len(models) or len(out_unit) != len(models):
        raise ValueError("one unit per model")
    if not models:
        raise ValueError("no noise models")
    bands = (sf_noise_band * len(models))()
    parts, offset = [], 0
    for i, m in enumerate(models):
        d = m._band(in_unit[i], out_unit[i])
        c, med, std = d.pop("tables")
        for k, v in d.items():
            setattr(bands[i], k, v)
        bands[i].n_bins, bands[i].table_offset = len(c), offset
        parts += [c, med, std]
        offset += 3 * len(c)
    table = np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)
    return bands, table


def band_fields(bands) -> list:
    """The packed structs as dicts (for tests and for reading a model's packed form)."""
    return [{name: getattr(b, name) for name, _ in sf_noise_band._fields_} for b in bands]
