"""``SBI_Fitter`` surface of the reference for the amortised-posterior flow path, HIP backend.

Same method names, argument meaning and error behaviour as ref: src/synference/sbi_runner.py for
  run_single_sbi (4392-4435), create_priors (3442-3450), split_dataset (3407-3440),
  sample_posterior (6350-6474), log_prob (7162-7198), fit_catalogue sampling + quantile section
  (2948-2989, 3230-3282), evaluate_model's flow-derived metrics (6484-6735), calculate_MAP (7204-7207: a stub there;
  here [UPSTREAM] sbi ``posterior.map`` per catalogue row, synference_amd/map.py).
What is NOT here (out of scope): library generation, feature engineering from
raw fluxes, noise models, Optuna search, MDN / likelihood / ratio engines, MCMC / VI samplers,
plotting.  Asking for them raises ``ValueError`` rather than falling through to another backend.

The per-galaxy Python loops of the reference (6438-6442, 7193-7196) collapse into one catalogue
call on the GPU; return types and shapes are the reference's ((N,S,D) float64 ndarray; (N,) float64).
"""
from __future__ import annotations

import logging
import os
import time
import warnings
from typing import Callable, List, Optional, Union

import numpy as np
import torch

from .estimator import SUPPORTED_MODELS, load_nde_hip
from .priors import CustomIndependentUniform, prior_from_parameters
from .runner import HIPRunner, NumpyLoader

logger = logging.getLogger("synference_amd")

# the reference's default model directory is f"{code_path}/models/" with code_path = the directory above the package
# (sbi_runner.py:87-89, 4413)
DEFAULT_MODEL_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "models") + "/"


def _warn_unknown(fn: str, unknown: dict) -> None:
    """Keywords outside the mirrored signature are named in a warning instead of vanishing."""
    if unknown:
        warnings.warn(f"{fn}: unknown keyword argument(s) {sorted(unknown)} ignored", stacklevel=3)


class StandardScaler:
    """The two-method subset of sklearn.preprocessing.StandardScaler that ``prior_method="manual"`` uses (``feature_scalar`` /
    ``target_scalar`` defaults of run_single_sbi, sbi_runner.py:4416-4417, 4664-4671), with sklearn's attribute names
    (``mean_``, ``scale_``: population std, zeros replaced by 1) so that the product does not import scikit-learn; any class with
    fit / transform / inverse_transform can be passed instead."""

    def fit(self, X, y=None):
        X = np.asarray(X, dtype=np.float64)
        self.mean_ = X.mean(axis=0)
        self.scale_ = X.std(axis=0)
        self.scale_[self.scale_ == 0.0] = 1.0
        return self

    def transform(self, X):
        return (np.asarray(X, dtype=np.float64) - self.mean_) / self.scale_

    def fit_transform(self, X, y=None):
        return self.fit(X).transform(X)

    def inverse_transform(self, X):
        return np.asarray(X, dtype=np.float64) * self.scale_ + self.mean_


class SBI_Fitter:
    device = "cuda"

    @property
    def _timestamp(self):
        """Current date and time as a string (ref: sbi_runner.py:7640-7643)."""
        return time.strftime("%Y%m%d_%H%M%S")

    def __init__(self, name: str, parameter_names: list, raw_observation_names: list = None,
                 raw_observation_grid: np.ndarray = None, parameter_array: np.ndarray = None,
                 parameter_units: list = None, raw_observation_units: list = None, simulator: callable = None,
                 feature_array: np.ndarray = None, feature_names: list = None, feature_units: list = None,
                 library_path: str = None, supplementary_parameters: np.ndarray = None,
                 supplementary_parameter_names: list = None, supplementary_parameter_units: list = None,
                 device: str = "cuda", observation_type: str = "photometry") -> None:
        if simulator is not None:
            raise ValueError("online simulators are outside the accelerated path: the HIP backend trains on a library "
                             "(init_from_hdf5) or on a feature array + parameter array")
        self.library_path = library_path
        self.raw_observation_grid = None if raw_observation_grid is None else np.asarray(raw_observation_grid)
        self.raw_observation_units = raw_observation_units
        self.supplementary_parameters = supplementary_parameters
        self.supplementary_parameter_names = supplementary_parameter_names
        self.supplementary_parameter_units = supplementary_parameter_units
        self.name = name
        self.parameter_names = list(parameter_names)
        self.fitted_parameter_names = list(parameter_names)
        self.simple_fitted_parameter_names = [str(p).split("/")[-1] for p in parameter_names]
        self.fitted_parameter_units = parameter_units
        self.raw_observation_names = raw_observation_names
        self.feature_names = feature_names if feature_names is not None else raw_observation_names
        self.feature_units = feature_units
        self.device = device
        self.observation_type = observation_type
        self.feature_array = None
        self.fitted_parameter_array = None
        self.has_features = False
        if feature_array is not None:
            # reference: feature_array.astype(np.float32), (N, C) (sbi_runner.py:2150)
            self.feature_array = np.ascontiguousarray(np.asarray(feature_array).astype(np.float32))
            self.has_features = True
        self.parameter_array = None
        self.parameter_units = parameter_units
        if parameter_array is not None:
            self.parameter_array = np.asarray(parameter_array)
            self.fitted_parameter_array = np.asarray(parameter_array)
            if self.fitted_parameter_array.shape[1] != len(self.parameter_names):
                raise ValueError("parameter_array must be (N, len(parameter_names))")
        self.has_simulator = False
        self._feature_scalar = None      # prior_method="manual" (sbi_runner.py:287-288)
        self._target_scalar = None
        self.posteriors = None
        self.last_lc2st = None
        self.last_misspecification = None
        self.marginal_trainer = self.marginal_trainer_est = None
        self.stats = None
        self._prior = None
        self._train_indices = self._test_indices = None
        self._X_train = self._y_train = self._X_test = self._y_test = None
        self.fitted_model_name = None

    # ---------------------------------------------------------------------------------------
    @classmethod
    def init_from_hdf5(cls, model_name: str, hdf5_path: str, return_output: bool = False, **kwargs):
        """ref: sbi_runner.py:309-405 -- a fitter on top of a library file (``Grid/Photometry`` (C,N) in nJy,
        ``Grid/Parameters`` (D,N), root attributes ``FilterCodes`` / ``ParameterNames`` / units), read by
        ``synference_amd.library.load_library_from_hdf5`` (no h5py needed)."""
        from .library import load_library_from_hdf5
        output = load_library_from_hdf5(hdf5_path)
        if return_output:
            return output
        if "photometry" in output:
            grid, otype = output["photometry"], "photometry"
        elif "spectra" in output:
            grid, otype = output["spectra"], "spectra"
        else:
            raise ValueError("HDF5 file must contain 'photometry' or 'spectra' data.")
        return cls(name=model_name, raw_observation_grid=grid, raw_observation_names=list(output["filter_codes"]),
                   parameter_array=output["parameters"].T, parameter_names=list(output["parameter_names"]),
                   parameter_units=None if output["parameter_units"] is None else list(output["parameter_units"]),
                   raw_observation_units=output["photometry_units"], library_path=hdf5_path,
                   supplementary_parameters=output.get("supplementary_parameters"),
                   supplementary_parameter_names=list(output.get("supplementary_parameter_names", [])),
                   supplementary_parameter_units=list(output.get("supplementary_parameter_units", [])),
                   observation_type=otype, **kwargs)

    def create_feature_array(self, flux_units: str = "AB", extra_features: list = None, **kwargs):
        """ref: sbi_runner.py:1065-1094 -- the simple wrapper: no noise, every filter of the library."""
        if self.observation_type == "photometry":
            return self.create_feature_array_from_raw_photometry(normed_flux_units=flux_units, extra_features=extra_features,
                                                                 **kwargs)
        if self.observation_type == "spectra":
            return self.create_feature_array_from_raw_spectra(normed_flux_units=flux_units, extra_features=extra_features,
                                                              **kwargs)
        raise ValueError(f"Observation type {self.observation_type} not supported. Please use 'photometry' or 'spectra'.")

    def create_feature_array_from_raw_spectra(self, extra_features=["redshift"], crop_wavelength_range: Union[tuple, list] = None,
                                              normed_flux_units: str = "AB", flux_norm_method: Optional[str] = None,
                                              flux_norm_parameters: dict = None, parameters_to_remove: list = None,
                                              parameters_to_add: list = None, parameter_transformations: dict = None,
                                              resample_wavelengths=None, inst_resolution_wavelengths=None,
                                              inst_resolution_r=None, theory_r: float = np.inf,
                                              min_flux_value: float = -np.inf, max_flux_value: float = np.inf):
        """ref: sbi_runner.py:1180-1427 -- the library's (L, N) spectra (wavelengths in um as ``raw_observation_names``) become
        the (N, M + extras) float32 feature array, with the per-spectrum work on the device (``sf_spectra_transform``).

        The reference's argument names, order and defaults.  With ``redshift`` among the parameters every spectrum is
        redshifted, convolved with the instrument's line-spread function (``inst_resolution_wavelengths`` in um,
        ``inst_resolution_r``, less the model's own ``theory_r``) and rebinned onto ``resample_wavelengths`` (um;
        ``crop_wavelength_range`` then crops those, in the observed frame); without it ``crop_wavelength_range`` crops the
        theory grid and nothing is convolved or rebinned.  ``flux_norm_method`` "tophat" (``center``, ``width`` in um) or
        "bandpass" (``filter``: an object with ``.lam`` and ``.transmission``, or a ``(wavelength_um, transmission)`` pair)
        divides every spectrum by its mean flux there, on the theory grid with ``flux_norm_parameters["rest_frame"]``, else
        on the final grid; then ``normed_flux_units`` ("AB", "log10 <unit>" or a unit of ``noise_models.PHYSICAL_UNITS``),
        the clip to [``min_flux_value``, ``max_flux_value``] and the ``extra_features`` columns from the parameter array.
        Wavelengths are plain arrays in um (anything with ``to_value("um")`` is converted).  ``self.feature_wavelengths``
        holds the M output wavelengths.  Deviations from the reference: DESIGN.md, "Spectra features"."""
        from . import spectra as SP
        if self.observation_type != "spectra":
            raise ValueError("This method is only for spectra models.")
        if self.raw_observation_grid is None:
            raise ValueError("Raw observation library is not set. Please provide a valid library.")
        extra_features = [] if extra_features is None else extra_features
        if not isinstance(extra_features, list):
            raise ValueError("extra_features must be a list of feature names.")
        parameters_to_remove = [] if parameters_to_remove is None else parameters_to_remove
        parameters_to_add = [] if parameters_to_add is None else parameters_to_add
        norm_pars = {} if flux_norm_parameters is None else flux_norm_parameters
        if flux_norm_method is not None and (callable(flux_norm_method) or flux_norm_method not in ("tophat", "bandpass")):
            raise ValueError(f'flux_norm_method {flux_norm_method!r} is outside the HIP path: use "tophat" or "bandpass"')
        if getattr(self, "parameter_array", None) is None:
            raise ValueError("no parameter array: build the fitter from a library or pass parameter_array")
        pnames = [str(p) for p in self.parameter_names]
        extra_cols = []
        for feature in extra_features:
            if feature not in [str(p) for p in self.fitted_parameter_names] or feature not in pnames:
                raise ValueError(f"Feature {feature} not found in parameter names.")
            extra_cols.append(pnames.index(feature))
        wavs = SP._grid(np.array(self.raw_observation_names, dtype=float), "the library's wavelength grid")
        grid = self.raw_observation_grid
        if grid.ndim != 2 or grid.shape[0] != len(wavs) or grid.shape[1] != self.parameter_array.shape[0]:
            raise ValueError("the spectra grid must be (len(raw_observation_names), number of parameter rows)")
        unit_code, unit_scale = SP.unit_conversion(self._grid_flux_unit(), normed_flux_units)
        has_redshift = "redshift" in pnames
        is_rest_norm = bool(norm_pars.get("rest_frame", False))
        kw = dict(unit_code=unit_code, unit_scale=unit_scale, clip=(min_flux_value, max_flux_value))
        if has_redshift:
            # (the reference asserts: the same exception type and messages)
            if resample_wavelengths is None:
                raise AssertionError("resample_wavelengths must be provided when transforming to observed frame.")
            if inst_resolution_wavelengths is None:
                raise AssertionError("inst_resolution_wavelengths must be provided for convolution.")
            if inst_resolution_r is None:
                raise AssertionError("inst_resolution_r must be provided for convolution.")
            out_wavs = SP._grid(resample_wavelengths, "resample_wavelengths")
            if crop_wavelength_range is not None:
                logger.warning('Assuming crop_wavelength_range is in observed frame when "redshift" is a feature.')
                out_wavs = out_wavs[(out_wavs >= crop_wavelength_range[0]) & (out_wavs <= crop_wavelength_range[1])]
            resample_wavelengths = out_wavs
            kw.update(observed_wave=out_wavs, resolution_curve_wave=inst_resolution_wavelengths,
                      resolution_curve_r=inst_resolution_r, theory_r=theory_r)
            zcol = np.asarray(self.parameter_array[:, pnames.index("redshift")], np.float64)
        else:
            mask = np.ones(len(wavs), bool) if crop_wavelength_range is None else \
                (wavs >= crop_wavelength_range[0]) & (wavs <= crop_wavelength_range[1])
            first = int(np.argmax(mask)) if mask.any() else 0
            kw.update(columns=(first, int(mask.sum())))
            out_wavs = wavs[mask]
        if flux_norm_method is not None:
            on_theory = is_rest_norm or not has_redshift      # without a redshift both frames are the uncropped theory grid
            kw.update(norm_frame=SP.NORM_REST if on_theory else SP.NORM_OBSERVED,
                      norm_table=SP.norm_coefficients(wavs if on_theory else out_wavs, flux_norm_method, norm_pars))
        N, L, M = grid.shape[1], len(wavs), len(out_wavs)
        feat = torch.empty((N, M + len(extra_cols)), dtype=torch.float32, device=self.device)
        rows = max(1, (1 << 30) // (4 * L))                   # the (L, N) grid transposed in row chunks of about 1 GiB
        for a in range(0, N, rows):
            b = min(N, a + rows)
            chunk = torch.from_numpy(np.ascontiguousarray(grid[:, a:b].T, dtype=np.float32)).to(self.device)
            SP.spectra_features(chunk, wavs, z=zcol[a:b] if has_redshift else None, out=feat[a:b], **kw)
        for i, c in enumerate(extra_cols):
            feat[:, M + i] = torch.from_numpy(np.asarray(self.parameter_array[:, c], np.float32)).to(self.device)
        self.feature_array = np.ascontiguousarray(feat.cpu().numpy())
        self.feature_wavelengths = np.array(out_wavs, dtype=np.float64)
        self.feature_names = ["spectra"] + extra_features
        self.feature_units = [normed_flux_units]
        self.has_features = True
        self.feature_array_flags = {"extra_features": extra_features, "crop_wavelength_range": crop_wavelength_range,
                                    "normed_flux_units": normed_flux_units, "flux_norm_method": flux_norm_method,
                                    "flux_norm_parameters": flux_norm_parameters,
                                    "parameters_to_remove": parameters_to_remove, "parameters_to_add": parameters_to_add,
                                    "parameter_transformations": parameter_transformations,
                                    "resample_wavelengths": resample_wavelengths}
        self.update_parameter_array(parameters_to_remove=parameters_to_remove, parameters_to_add=parameters_to_add,
                                    parameter_transformations=parameter_transformations)
        logger.info(f"Spectra feature array created with shape {self.feature_array.shape}.")
        return self.feature_array, self.feature_names

    def create_feature_array_from_raw_photometry(self, normalize_method: Optional[str] = None, extra_features: list = None,
                                                 normed_flux_units: str = "AB", normalization_unit: str = "AB",
                                                 verbose: bool = True, scatter_fluxes: Union[int, bool] = False,
                                                 empirical_noise_models=None, depths=None,
                                                 include_errors_in_feature_array: bool = False,
                                                 min_flux_pc_error: float = 0.0, simulate_missing_fluxes: bool = False,
                                                 norm_mag_limit: float = 50.0, remove_nan_inf: bool = True,
                                                 parameters_to_remove: Optional[list] = None,
                                                 photometry_to_remove: Optional[list] = None,
                                                 parameters_to_add: Optional[list] = None, drop_dropouts: bool = False,
                                                 drop_dropout_fraction: float = 1.0, max_rows: int = -1,
                                                 parameter_transformations: Optional[dict] = None,
                                                 asinh_softening_parameters=None, seed: int = 0, **unknown):
        """The AB-magnitude branch of the reference's feature engineering (ref: sbi_runner.py:1429-2222) with the
        arithmetic on the device: the library's (C, N) fluxes in nJy become the (N', F) float32 feature array.

        Same argument names and meaning as the reference for what is supported:
          * ``photometry_to_remove`` (1566-1589), ``scatter_fluxes`` + ``depths`` (array, or dict by filter name; same
            unit as the grid) + ``min_flux_pc_error`` (1629-1655, ``_apply_depths`` 580-691; ``sf_scatter_depths``),
            ``include_errors_in_feature_array`` (magnitude errors 2.5 e / (ln 10 f), 1698-1702, columns ``unc_<filter>``);
          * nJy -> AB with negative fluxes and anything fainter set to ``norm_mag_limit`` (1704-1716, 1927-1932;
            ``sf_flux_to_abmag``);
          * ``normalize_method`` = a filter name (1783-1834): that band is removed, the others become colours relative
            to it, and the band itself -- the UNSCATTERED library flux, as ``normalization_unit`` "AB" or "log10 nJy"
            -- is the last column ``norm_<filter>_<unit>`` (2002-2027);
          * ``remove_nan_inf``, ``drop_dropouts`` / ``drop_dropout_fraction``, ``max_rows`` (2084-2140), and the
            parameter bookkeeping of ``update_parameter_array`` (476-578: ``parameters_to_remove``,
            ``parameters_to_add`` from the supplementary parameters, repetition per scatter copy, deleted rows,
            ``parameter_transformations``).
          * ``normed_flux_units="asinh"`` (1591-1627, 1718-1732; utils.py:647-704; ``sf_flux_to_asinh``): softening
            ``asinh_softening_parameters`` per filter in the grid's unit -- an array, a dict by filter name, or
            ``"SNR_<k>"`` = k x depth / 5 when scattering with depths; no magnitude-limit clip there, as in the reference.
          * ``scatter_fluxes`` + ``empirical_noise_models`` = {filter: model of ``synference_amd.noise_models``}
            (1679-1693, ``_apply_empirical_noise_models`` 813-903; ``sf_scatter_empirical``): every filter is scattered through
            its own model from the grid's unit straight to ``normed_flux_units``, errors included; for AB, NaN and inf become
            ``norm_mag_limit`` (1707-1714); all-Asinh models make ``asinh_softening_parameters`` optional (1592-1600).  Depths
            win when both are given and ``min_flux_pc_error`` is ignored on this path, as in the reference.  General models with
            ``normed_flux_units="asinh"``, Asinh models with "AB" and mixed dicts are a ``ValueError``.
        Outside the accelerated path (``ValueError``): other flux units, extra feature expressions, simulated missing
        fluxes, normalisation by a supplementary parameter or of asinh magnitudes.  ``seed`` replaces numpy's global
        generator for the scatter noise and the ``max_rows`` draw."""
        _warn_unknown("create_feature_array_from_raw_photometry", unknown)
        if self.raw_observation_grid is None:
            raise ValueError("no raw observation grid: build the fitter with init_from_hdf5 or pass feature_array")
        if extra_features or normed_flux_units not in ("AB", "asinh") or simulate_missing_fluxes:
            raise ValueError("only normed_flux_units='AB' / 'asinh' without extra features or simulated missing fluxes is on "
                             "the HIP path")
        asinh = normed_flux_units == "asinh"
        if asinh and normalize_method is not None:
            raise ValueError("normalisation of asinh magnitudes is outside the HIP path")
        # the models scatter only when there are no depths: depths win when both are given (ref: 1636 / 1679)
        use_models = bool(scatter_fluxes) and depths is None and empirical_noise_models is not None
        if use_models and not isinstance(empirical_noise_models, dict):
            raise ValueError("empirical_noise_models must be a dictionary")
        if asinh:
            from .noise_models import AsinhEmpiricalUncertaintyModel
            err_is_asinh = isinstance(empirical_noise_models, dict) and all(
                isinstance(m, AsinhEmpiricalUncertaintyModel) for m in empirical_noise_models.values())   # ref: 1592-1600
            assert asinh_softening_parameters is not None or (err_is_asinh and use_models), \
                "asinh_softening_parameters must be provided for asinh normalization."
        if not torch.cuda.is_available():
            raise RuntimeError("create_feature_array_from_raw_photometry runs on the GPU (no CPU fallback)")
        from .features import flux_to_abmag, flux_to_asinh, scatter_depths
        names = [str(n_) for n_ in self.raw_observation_names]
        grid = np.asarray(self.raw_observation_grid)                                    # (C, N)
        photometry_to_remove = list(photometry_to_remove or [])
        if photometry_to_remove:
            rm = [i for i, n_ in enumerate(names) if n_ in photometry_to_remove]
            if not rm:
                raise ValueError(f"No matching photometry filters found in the raw photometry names: {photometry_to_remove}")
            grid = np.delete(grid, rm, axis=0)
            names = [n_ for i, n_ in enumerate(names) if i not in rm]
            if not names:
                raise ValueError("No photometry filters left after removing the specified ones.")
        n_sc = int(scatter_fluxes) if scatter_fluxes else 0
        flux = torch.as_tensor(np.ascontiguousarray(grid.T), dtype=torch.float32).cuda()  # (N, C) on the device
        err = None
        converted = False
        if n_sc and use_models:
            flux, err = self._apply_empirical_noise_models(flux, names, empirical_noise_models, n_sc, normed_flux_units, seed)
            self.empirical_noise_models = empirical_noise_models
            converted = True                                  # magnitudes and their errors already (ref: 1693-1715)
        elif n_sc:
            if depths is None:
                raise ValueError("If scattering fluxes, depths or empirical noise models must be provided.")
            if isinstance(depths, dict):
                depths = np.asarray([depths[n_] for n_ in names], dtype=np.float32)
            self.phot_depths, self.min_flux_pc_error = depths, min_flux_pc_error
            flux, err = scatter_depths(flux, depths, n_sc, 5.0, min_flux_pc_error, seed=seed, return_errors=True)
        if converted:
            mag, mag_err = flux, err
            if not asinh:                                      # NaN and inf (zero and negative fluxes) to the limit (1707-1714)
                mag = torch.where(torch.isfinite(mag), mag, torch.full_like(mag, norm_mag_limit))
        elif asinh:
            if isinstance(asinh_softening_parameters, str):
                assert asinh_softening_parameters.startswith("SNR_"), "If a string, asinh_softening_parameters must start with 'SNR_'."
                assert n_sc and depths is not None, ("If setting asinh_softening_parameters from noise models, "
                                                     "depths or empirical_noise_models must be provided.")
                fb = float(asinh_softening_parameters.split("_")[-1]) * np.asarray(depths, dtype=np.float64).reshape(-1) / 5.0
            elif isinstance(asinh_softening_parameters, dict):
                fb = np.asarray([asinh_softening_parameters[n_] for n_ in names], dtype=np.float64)
            else:
                fb = np.asarray(asinh_softening_parameters, dtype=np.float64).reshape(-1)
            if fb.size not in (1, len(names)):
                raise AssertionError("asinh_softening_parameter must be a list of the same length as the number of photometry filters.")
            fb = np.broadcast_to(fb, (len(names),)).astype(np.float32)
            mag, mag_err = flux_to_asinh(flux, fb, err) if err is not None else (flux_to_asinh(flux, fb, None), None)
        else:
            mag, mag_err = flux_to_abmag(flux, err, norm_mag_limit) if err is not None else (flux_to_abmag(flux, None, norm_mag_limit), None)
        norm_col, norm_name = None, None
        if normalize_method is not None:
            if normalize_method not in names:
                raise NotImplementedError("Normalization method not implemented.\n                    Please use a filter name for normalization.")
            j = names.index(normalize_method)
            keep = [i for i in range(len(names)) if i != j]
            ref = mag[:, j:j + 1]
            orig = torch.as_tensor(np.ascontiguousarray(grid[j]), dtype=torch.float64).cuda()   # unscattered library flux (nJy)
            if n_sc:
                orig = orig.repeat_interleave(n_sc)
            mag = mag[:, keep] - ref                                                   # colours (norm_func = np.subtract)
            if mag_err is not None:
                mag_err = mag_err[:, keep]
            if normalization_unit == "AB":
                norm_col = -2.5 * torch.log10(orig * 1e-3) + 23.9
            elif normalization_unit.startswith("log10 "):
                if normalization_unit.split(" ")[1] != "nJy":
                    raise ValueError("normalization_unit: 'AB' or 'log10 nJy' on the HIP path")
                norm_col = torch.log10(orig)
                norm_col[torch.isinf(norm_col)] = 0.0
            else:
                raise ValueError("normalization_unit: 'AB' or 'log10 nJy' on the HIP path")
            zero_norm = (ref.reshape(-1) == 0)
            names = [names[i] for i in keep]
            norm_name = f"norm_{normalize_method}_{normalization_unit}"
        if not asinh:
            mag = torch.where(mag > norm_mag_limit, torch.full_like(mag, norm_mag_limit), mag)   # 1927-1932 (AB only)
        cols, feature_names, units = [mag], list(names), [normed_flux_units] * len(names)
        error_names = [f"unc_{n_}" for n_ in names] if mag_err is not None else []
        if mag_err is not None and include_errors_in_feature_array:
            cols.append(mag_err)
            feature_names += error_names
            units += [normed_flux_units] * len(error_names)
        if norm_col is not None:
            cols.append(norm_col.float().reshape(-1, 1))
            feature_names.append(norm_name)
            units.append(normalization_unit)
        feat = torch.cat(cols, dim=1)
        delete = torch.zeros(feat.shape[0], dtype=torch.bool, device=feat.device)
        if norm_col is not None:
            delete |= zero_norm                                                        # 1917-1925
        if remove_nan_inf:
            bad = ~torch.isfinite(feat).all(dim=1)
            if verbose and int(bad.sum()):
                logger.warning(f"Warning: Deleting {int(bad.sum())} rows with NaN or Inf\n                    values in the feature array.")
            delete |= bad
        if drop_dropouts:
            nb = len(names)
            drop = (feat[:, :nb].abs() >= norm_mag_limit).sum(dim=1) >= nb * drop_dropout_fraction
            if verbose and int(drop.sum()):
                logger.warning(f"Warning: Dropping {int(drop.sum())} dropouts where more than\n                    "
                               f"{drop_dropout_fraction * 100}% of bands are at the norm_mag_limit.")
            delete |= drop
        delete_rows = torch.nonzero(delete).reshape(-1).cpu().numpy()
        if max_rows > 0 and feat.shape[0] - len(delete_rows) > max_rows:
            options = np.setdiff1d(np.arange(feat.shape[0]), delete_rows)
            chosen = np.random.default_rng(seed).choice(options, size=max_rows, replace=False)
            delete_rows = np.concatenate([delete_rows, np.setdiff1d(options, chosen)])
        keep_rows = np.setdiff1d(np.arange(feat.shape[0]), delete_rows)
        if keep_rows.size == 0:
            raise ValueError("All rows in the feature array were deleted. Please check the input parameters.")
        feat = feat[torch.as_tensor(keep_rows, device=feat.device)]
        self.feature_array = np.ascontiguousarray(feat.cpu().numpy().astype(np.float32))
        self.feature_names, self.feature_units, self.has_features = feature_names, units, True
        self.feature_array_flags = dict(normalize_method=normalize_method, extra_features=extra_features,
                                        normed_flux_units=normed_flux_units, normalization_unit=normalization_unit,
                                        scatter_fluxes=scatter_fluxes, depths=depths,
                                        include_errors_in_feature_array=include_errors_in_feature_array,
                                        min_flux_pc_error=min_flux_pc_error, norm_mag_limit=norm_mag_limit,
                                        remove_nan_inf=remove_nan_inf, parameters_to_remove=parameters_to_remove,
                                        photometry_to_remove=photometry_to_remove, parameters_to_add=parameters_to_add,
                                        drop_dropouts=drop_dropouts, drop_dropout_fraction=drop_dropout_fraction,
                                        raw_observation_names=names, error_names=error_names, norm_name=norm_name,
                                        empirical_noise_models=empirical_noise_models if converted else None)
        self.update_parameter_array(parameters_to_remove=list(parameters_to_remove or []), delete_rows=np.sort(delete_rows),
                                    n_scatters=max(n_sc, 1), parameters_to_add=list(parameters_to_add or []),
                                    parameter_transformations=parameter_transformations)
        return self.feature_array, self.feature_names

    def _grid_flux_unit(self) -> str:
        """The unit of the raw observation grid as one of the noise models' unit strings (the library convention is nJy)."""
        from .noise_models import PHYSICAL_UNITS
        u = self.raw_observation_units
        u = u if isinstance(u, str) or u is None else (str(u[0]) if len(u) else None)
        return u if u in PHYSICAL_UNITS or u == "AB" else "nJy"

    def _apply_empirical_noise_models(self, flux, phot_names, empirical_noise_models, n_scatters, normed_flux_units, seed):
        """ref: sbi_runner.py:813-903 -- every filter scattered ``n_scatters`` times through its own model on the device
        (``sf_scatter_empirical``): (N, C) grid fluxes -> (N * n_scatters, C) values and errors in ``normed_flux_units``."""
        from .features import scatter_empirical
        if not isinstance(empirical_noise_models, dict):
            raise ValueError("empirical_noise_models must be a dictionary")
        for name in phot_names:
            if name not in empirical_noise_models:
                raise ValueError(f"""No empirical noise model found for filter {name}.
                    Please provide a valid model.""")
        for name in empirical_noise_models.keys():
            if name not in phot_names:
                raise ValueError(f"Filter {name} in empirical_noise_models is not in phot_names:\
                    {phot_names}. Please provide a valid filter name.")
        return scatter_empirical(flux, [empirical_noise_models[n_] for n_ in phot_names], self._grid_flux_unit(),
                                 normed_flux_units, n_scatters=n_scatters, seed=seed)

    def update_parameter_array(self, parameters_to_remove: list = [], delete_rows=[], n_scatters: int = 1,
                               parameters_to_add: list = [], parameter_transformations: dict = None) -> None:
        """ref: sbi_runner.py:476-578 -- the fitted parameter array that goes with the feature array: columns removed /
        added (from the supplementary parameters), rows repeated per scatter copy, deleted rows dropped, optional
        per-parameter transformations (the column is renamed ``<fn>_<name>``)."""
        if getattr(self, "parameter_array", None) is None:
            raise ValueError("no parameter array: build the fitter from a library or pass parameter_array")
        arr = np.array(self.parameter_array, copy=True)
        pnames = [str(n_) for n_ in self.parameter_names]
        punits = None if self.parameter_units is None else list(self.parameter_units)
        for prm in np.unique(list(parameters_to_remove)):
            if prm in pnames:
                i = pnames.index(prm)
                arr = np.delete(arr, i, axis=1)
                pnames.pop(i)
                if punits is not None:
                    punits.pop(i)
        for prm in parameters_to_add:
            sn = [str(n_) for n_ in (self.supplementary_parameter_names or [])]
            if prm not in sn:
                raise ValueError(f"Can't add {prm} to parameter array - not found in supplementary parameters. "
                                 f"Available parameters: {self.supplementary_parameter_names}")
            i = sn.index(prm)
            arr = np.column_stack((arr, np.asarray(self.supplementary_parameters)[i]))
            pnames.append(prm)
            if punits is not None and self.supplementary_parameter_units is not None:
                punits.append(self.supplementary_parameter_units[i])
        if n_scatters > 1:
            arr = np.repeat(arr, n_scatters, axis=0)
        if len(delete_rows) > 0:
            arr = np.delete(arr, np.asarray(delete_rows, dtype=np.int64), axis=0)
        if parameter_transformations is not None:
            for prm, fn in parameter_transformations.items():
                if prm not in pnames:
                    raise ValueError(f"Parameter {prm} not found in fitted parameter names for transformation.")
                i = pnames.index(prm)
                arr[:, i] = fn(arr[:, i])
                pnames[i] = f"{fn.__name__}_{prm}"
                if punits is not None and punits[i] is not None and str(punits[i]) != "dimensionless":
                    punits[i] = f"{fn.__name__}({punits[i]})"
        self.fitted_parameter_array = arr
        self.fitted_parameter_names = pnames
        self.simple_fitted_parameter_names = [n_.split("/")[-1] for n_ in pnames]
        self.fitted_parameter_units = punits

    def split_dataset(self, train_fraction: float = 0.8, random_seed: int = None, verbose: bool = True) -> tuple:
        if random_seed is not None:
            np.random.seed(random_seed)
        if not self.has_features:
            raise ValueError("Feature array not created. Please create the feature array first.")
        n = self.feature_array.shape[0]
        idx = np.arange(n)
        np.random.shuffle(idx)
        k = int(n * train_fraction)
        return idx[:k], idx[k:]

    def create_priors(self, override_prior_ranges: dict = {}, prior=CustomIndependentUniform, verbose: bool = True,
                      debug_sample_acceptance: bool = False, extend_prior_range_pc: float = 0.0,
                      set_self: bool = False):
        if not self.has_features:
            raise ValueError("Feature array not created and no simulator.\n"
                             "                Please create the feature array first.")
        if self.fitted_parameter_array is None:
            raise ValueError("Parameter grid not created. Please create the parameter grid first.")
        p = prior_from_parameters(self.fitted_parameter_array, self.fitted_parameter_names,
                                  override_prior_ranges, extend_prior_range_pc, device="cpu")
        if verbose:
            logger.info("Prior ranges:")
            for n_, lo, hi in zip(self.fitted_parameter_names, p.low.tolist(), p.high.tolist()):
                logger.info(f"{n_}: {lo:.2f} - {hi:.2f}")
        if set_self:
            self._prior = p
        return p

    # ---------------------------------------------------------------------------------------
    def run_single_sbi(self, train_test_fraction: float = 0.8, random_seed: Optional[int] = None,
                       backend: str = "sbi", engine: Union[str, List[str]] = "NPE",
                       train_indices: Optional[np.ndarray] = None, test_indices: Optional[np.ndarray] = None,
                       n_nets: int = 1, model_type: Union[str, List[str]] = "mdn",
                       hidden_features: Union[int, List[int]] = 50, num_components: Union[int, List[int]] = 4,
                       num_transforms: Union[int, List[int]] = 4, training_batch_size: int = 64,
                       learning_rate: float = 1e-4, validation_fraction: float = 0.2, stop_after_epochs: int = 15,
                       clip_max_norm: float = 5.0, additional_model_args: dict = {}, save_model: bool = True,
                       verbose: bool = True, prior_method: str = "ili", out_dir: str = DEFAULT_MODEL_DIR, plot: bool = True,
                       name_append: str = "timestamp", feature_scalar: Callable = StandardScaler,
                       target_scalar: Callable = StandardScaler, set_self: bool = True, learning_type: str = "offline",
                       simulator: Optional[Callable] = None, num_simulations: int = 1000, num_online_rounds: int = 5,
                       initial_training_from_library: bool = False, override_prior_ranges: dict = {},
                       online_training_xobs: Optional[np.ndarray] = None, load_existing_model: bool = True,
                       use_existing_indices: bool = True, evaluate_model: bool = True, save_method: str = "joblib",
                       num_posterior_draws_per_sample: int = 1000, embedding_net: Optional[torch.nn.Module] = None,
                       custom_config_yaml: Optional[str] = None, sql_db_path: Optional[str] = None, *,
                       max_num_epochs: Optional[int] = None, optimizer_choice: str = "Adam", **unknown) -> tuple:
        """Train an ensemble of n_nets flows; returns (posteriors, stats) like the reference.

        ``custom_config_yaml`` (ref: sbi_runner.py:4570-4597, custom_runner.py:226-244, 298-365): a YAML file whose
        ``train_args`` has ``skip_optimization: True`` and ``fixed_params`` (``model_choice``, ``optimizer_choice``,
        ``learning_rate``, ``training_batch_size``, ``stop_after_epochs``, ``clip_max_norm`` and the model's own
        ``<model>_hidden_features`` / ``<model>_num_transforms`` / ``<model>_num_bins`` ...) trains ONE model with those
        values, ``validation_fraction`` from ``train_args`` (default 0.1); the Optuna search branch is out of scope.

        Positional order, names and defaults are the reference's (sbi_runner.py:4392-4435); ``max_num_epochs`` and
        ``optimizer_choice`` are keyword-only additions.  What the defaults mean here: ``backend="sbi"`` (alias ``"hip"``) = the
        nflows-style MAF / NSF that ili's sbi backend builds, on the HIP engine; ``"lampe"`` = its zuko-style NSF;
        ``model_type="mdn"`` -- the reference's default -- is NOT on the HIP path and raises, so a caller names "maf" or "nsf";
        ``plot=True`` is accepted and skipped with one log line (plotting is out of scope); ``evaluate_model=True`` runs
        ``evaluate_model`` on the test split.  ``out_dir`` gets the fitter's name appended (4541), an existing
        ``{out_dir}/{name}_{name_append}_params.pkl`` is loaded instead of training when ``load_existing_model`` (4546-4563:
        returns None when it is False), ``use_existing_indices`` re-uses a stored split that covers the feature array
        (4617-4636).  ``prior_method="manual"`` (4664-4690): ``feature_scalar()`` / ``target_scalar()`` are fit on the training
        rows, the flow is trained on the SCALED arrays and the box prior is min / max -+ 3 sigma of the scaled parameters --
        like the reference, nothing un-scales the draws afterwards: ``self._feature_scalar`` / ``self._target_scalar`` are the
        caller's tools for that.  Online learning (``simulator`` ...), ``sql_db_path`` and unknown keywords are refused or
        warned about, never silently dropped."""
        _warn_unknown("run_single_sbi", unknown)
        if simulator is not None or learning_type == "online" or initial_training_from_library or online_training_xobs is not None:
            raise ValueError("only learning_type='offline' (amortised NPE on a fixed library) is on the HIP path; simulator / "
                             "online rounds are not built")
        if sql_db_path is not None:
            raise ValueError("sql_db_path (the Optuna study database) belongs to the hyper-parameter search, which is outside the HIP path")
        if plot:
            logger.info("run_single_sbi(plot=True): plotting is outside the HIP path and is skipped")
        if custom_config_yaml is not None:
            import yaml
            with open(custom_config_yaml) as fh:
                ta = yaml.safe_load(fh)["train_args"]
            if not ta.get("skip_optimization", False):
                raise ValueError("custom_config_yaml without skip_optimization asks for the Optuna hyper-parameter search, "
                                 "which is outside the HIP path: set train_args.skip_optimization and fixed_params")
            fp = ta.get("fixed_params")
            if not fp or "model_choice" not in fp:  # custom_runner.py:229-233
                raise ValueError("`skip_optimization` is True, but `fixed_params` (including 'model_choice') "
                                 "are not defined in `train_args`.")
            model_type = fp["model_choice"]
            n_nets = 1
            margs = {k.split("_", 1)[1]: v for k, v in fp.items() if k.startswith(model_type + "_")}
            hidden_features = int(margs.pop("hidden_features", hidden_features))
            num_transforms = int(margs.pop("num_transforms", num_transforms))
            additional_model_args = {**additional_model_args, **margs}
            optimizer_choice = fp.get("optimizer_choice", "Adam")
            learning_rate = fp["learning_rate"]
            training_batch_size = fp.get("training_batch_size", 32)
            stop_after_epochs = fp.get("stop_after_epochs", 20)
            clip_max_norm = fp.get("clip_max_norm", 5.0)
            validation_fraction = ta.get("validation_fraction", 0.1)
        if backend == "lampe":   # the reference's second backend name (sbi_runner.py:5123-5125): its NSF, on the HIP engine
            additional_model_args = dict(additional_model_args or {}, backend="lampe")
            backend = "hip"
        if backend == "sbi":     # ili's sbi backend = nflows-style flows: what the HIP engine implements
            backend = "hip"
        if backend != "hip":
            raise ValueError(f"backend '{backend}' is not available in synference_amd: use backend='sbi' (alias 'hip': nflows-style "
                             "MAF / NSF) or 'lampe' (the zuko-style autoregressive NSF of the reference's lampe backend)")
        if learning_type != "offline":
            raise ValueError("only learning_type='offline' (amortised NPE) is on the HIP path")
        if prior_method not in ("ili", "manual"):
            raise ValueError("Invalid prior method. Use 'manual' or 'ili'.")   # sbi_runner.py:4700-4701
        if not self.has_features:
            raise ValueError("Feature array not created. Please create the feature array first.")
        if self.fitted_parameter_array is None:
            raise ValueError("Parameter grid not created. Please create the parameter grid first.")
        run_out_dir = None
        if out_dir is not None:
            run_out_dir = os.path.join(os.path.abspath(out_dir), self.name)      # sbi_runner.py:4541
        stamp = self._timestamp if name_append == "timestamp" else str(name_append)
        if run_out_dir is not None and save_model and os.path.exists(f"{run_out_dir}/{self.name}_{stamp}_params.pkl"):
            if load_existing_model:   # sbi_runner.py:4546-4557
                logger.info(f"Loading existing model from {run_out_dir}/{self.name}_{stamp}_params.pkl")
                posteriors, stats, _params = self.load_model_from_pkl(f"{run_out_dir}/{self.name}_{stamp}_posterior.pkl", set_self=set_self)
                return posteriors, stats
            logger.info("Model with same name already exists. Please change the name of this model or delete the existing one.")
            return None
        engines = [engine] * n_nets if isinstance(engine, str) else list(engine)
        models = [model_type] * n_nets if isinstance(model_type, str) else list(model_type)
        hf = [hidden_features] * n_nets if isinstance(hidden_features, int) else list(hidden_features)
        nt = [num_transforms] * n_nets if isinstance(num_transforms, int) else list(num_transforms)
        for m in models:
            if m not in SUPPORTED_MODELS:
                raise ValueError(f"model_type '{m}' is not on the HIP path; supported: {SUPPORTED_MODELS}")
        if train_indices is None:   # sbi_runner.py:4617-4636
            have = getattr(self, "_train_indices", None) is not None and getattr(self, "_test_indices", None) is not None
            if (not have or not use_existing_indices or
                    len(self._train_indices) + len(self._test_indices) != self.feature_array.shape[0]):
                train_indices, test_indices = self.split_dataset(train_test_fraction, random_seed, verbose)
            else:
                logger.info("Using existing train and test indices.")
                train_indices, test_indices = self._train_indices, self._test_indices
        X_train = self.feature_array[train_indices]
        y_train = self.fitted_parameter_array[train_indices]
        X_test = self.feature_array[test_indices] if test_indices is not None else None
        y_test = self.fitted_parameter_array[test_indices] if test_indices is not None else None
        if prior_method == "manual":   # sbi_runner.py:4664-4690
            self._feature_scalar, self._target_scalar = feature_scalar(), target_scalar()
            X_train = np.asarray(self._feature_scalar.fit(X_train).transform(X_train), dtype=np.float32)
            y_train = np.asarray(self._target_scalar.fit(y_train).transform(y_train))
            if X_test is not None:
                X_test = np.asarray(self._feature_scalar.transform(X_test), dtype=np.float32)
                y_test = np.asarray(self._target_scalar.transform(y_test))
            y_std, y_min, y_max = np.std(y_train, axis=0), np.min(y_train, axis=0), np.max(y_train, axis=0)
            from .priors import CustomIndependentUniform
            prior = CustomIndependentUniform(low=torch.tensor(y_min - 3 * y_std, dtype=torch.float32),
                                             high=torch.tensor(y_max + 3 * y_std, dtype=torch.float32),
                                             name_list=self.fitted_parameter_names, device="cpu")
        else:
            # the prior box spans the WHOLE parameter array (train + test rows), as in the reference's create_priors
            # (sbi_runner.py:3519-3520)
            prior = self.create_priors(override_prior_ranges, verbose=verbose)
        nets = []
        for i in range(n_nets):
            args = dict(hidden_features=hf[i], num_transforms=nt[i])
            args.update(additional_model_args)
            nets.append(load_nde_hip(engines[i], model=models[i], embedding_net=embedding_net, **args))
        train_args = dict(training_batch_size=training_batch_size, learning_rate=learning_rate,
                          validation_fraction=validation_fraction, stop_after_epochs=stop_after_epochs,
                          clip_max_norm=clip_max_norm, log_every=1 if verbose else 0,
                          optimizer_choice=optimizer_choice)
        if max_num_epochs is not None:
            train_args["max_num_epochs"] = max_num_epochs
        run_name = f"{self.name}_{stamp}_"
        trainer = HIPRunner.load(backend="hip", engine=engines[0], prior=prior, nets=nets, train_args=train_args,
                                 out_dir=(run_out_dir if save_model else None), device=self.device, name=run_name)
        t0 = time.time()
        try:
            posteriors, stats = trainer(NumpyLoader(X_train, y_train), seed=random_seed)
        except Exception as e:  # sbi_runner.py:4940-4941
            raise RuntimeError(f"Error during SBI training: {e}") from e
        self.training_time = time.time() - t0
        if set_self:
            self.posteriors, self.stats, self._prior = posteriors, stats, prior
            self._train_indices, self._test_indices = train_indices, test_indices
            self._X_train, self._y_train, self._X_test, self._y_test = X_train, y_train, X_test, y_test
            self.fitted_model_name = run_name
        if save_model and run_out_dir is not None:  # sbi_runner.py:4973-5014: the fitter's state next to the posterior pickle
            prior_was = self._prior
            self._prior = prior
            try:
                self.save_state(out_dir=run_out_dir, name_append=stamp, save_method=save_method, has_grid=True, engine=engine, learning_type=learning_type,
                                ensemble_model_types=list(models), ensemble_model_args=[dict(hidden_features=hf[i],
                                num_transforms=nt[i], **additional_model_args) for i in range(n_nets)], n_nets=n_nets,
                                train_args=train_args, stats=stats, training_time=self.training_time,
                                train_fraction=train_test_fraction, test_indices=test_indices, train_indices=train_indices)
            finally:
                self._prior = prior_was if not set_self else prior
        if evaluate_model and X_test is not None:
            self.evaluate_model(posteriors=posteriors, X_test=X_test, y_test=y_test,
                                num_samples=num_posterior_draws_per_sample)
        return posteriors, stats

    # ---------------------------------------------------------------------------------------
    def sample_posterior(self, X_test: np.ndarray = None, sample_method: str = "direct", sample_kwargs: dict = {},
                         posteriors: object = None, num_samples: int = 1000, timeout_seconds_per_test=30,
                         log_times=False, seed: Optional[int] = None, **kwargs) -> np.ndarray:
        """(num_objects, num_samples, num_parameters) float64; NaN rows where sampling failed
        (ref: sbi_runner.py:6436, 6458-6460); a single observation returns (num_samples, num_parameters)."""
        if posteriors is None:
            posteriors = self.posteriors
        if X_test is None:
            if getattr(self, "_X_test", None) is not None:
                X_test = self._X_test
            else:
                raise ValueError("X_test must be provided or set in the object.")
        if sample_method != "direct":
            raise ValueError("Invalid sample method for the HIP backend. Use 'direct'.")
        X = np.asarray(X_test, dtype=np.float32)
        single = X.ndim == 1 or (X.ndim == 2 and X.shape[0] == 1)
        if X.ndim == 1:
            X = X[None, :]
        # Under an initialised process group (one process per GPU) the catalogue is sharded: rank r samples rows
        # [r N / W, (r+1) N / W) -- rows are independent (ref: sbi_runner.py:6438-6442), weights are replicated, there is no
        # data-path collective -- and the blocks are gathered afterwards.  ``gather`` (keyword): "rank0" (default) -- rank 0
        # returns the whole (N, S, D) array, every other rank its own block (rows ``self.last_shard_rows``): ONE copy of the
        # array exists (configs[4]: 3.2 GB; all ranks holding it would move 8 x that over xGMI); "all" -- every rank returns
        # the whole array; "none" -- every rank keeps its block.  The random streams are keyed by the row's position in the
        # catalogue: the gathered result is the single-process one, bit for bit.
        from .hostio import to_host_f64
        from .posterior import all_gather_rows, broadcast_seed, dist_world, gather_rows, shard_bounds
        rank, world = dist_world()
        # ``row_offset`` (keyword): X holds rows [row_offset, ...) of a larger catalogue -- same seed, same draws as there
        off = int(kwargs.get("row_offset", 0))
        if world > 1 and len(X) >= world and kwargs.get("shard", True):
            if seed is None:
                seed = posteriors._next_seed(None)
            seed = broadcast_seed(seed)
            b = shard_bounds(len(X), world)
            tmo = float(timeout_seconds_per_test) * (b[rank + 1] - b[rank]) if timeout_seconds_per_test else None
            t0 = time.time()
            local = posteriors.sample_catalogue(torch.as_tensor(X[b[rank]:b[rank + 1]]), num_samples, seed,
                                                timeout_seconds=tmo, row_offset=off + b[rank])
            if log_times:
                per = (time.time() - t0) / max(1, b[rank + 1] - b[rank])
                self.last_times_per_object = np.full(b[rank + 1] - b[rank], per)
                self.last_time_per_object = float(per)
            self.last_shard_rows = (int(b[rank]), int(b[rank + 1]))
            how = kwargs.get("gather", "rank0")
            if how not in ("rank0", "all", "none"):
                raise ValueError("gather must be 'rank0', 'all' or 'none'")
            full = all_gather_rows(local, b) if how == "all" else (gather_rows(local, b, dst=0) if how == "rank0" else None)
            return to_host_f64(full if full is not None else local)
        # log_times: the reference times every object (sbi_runner.py:6438-6469: median and 16th-84th percentile of the
        # per-object wall time); the catalogue call is timed in chunks instead and each chunk's time is shared equally
        # by its objects, so the three statistics keep their meaning without a per-galaxy host loop
        # without log_times ONE catalogue call, then the native hand-over.  (Measured: cutting the catalogue in 2 .. 6 chunks so
        # that chunk k crosses the bus while chunk k + 1 is drawn costs more than it hides -- every chunk pays the sampler's
        # tail: 3.6 / 3.9 / 4.3 / 4.8 ms for 1 / 2 / 3 / 4 chunks of the cfg2 catalogue.)
        n_chunks = min(len(X), 16) if log_times else 1
        if seed is None and n_chunks > 1:
            seed = posteriors._next_seed(None)
        bounds = np.linspace(0, len(X), n_chunks + 1).astype(int)
        # (uninitialised: every chunk either fills its rows or, on failure, sets them to NaN below)
        from .hostio import pinned_result, result_array
        # ONE catalogue call on a one-member flow posterior: the sampler writes the float64 host container itself (pinned memory
        # mapped into the device's address space; sf_flow_set_sample_output_f64) -- the draws cross PCIe while the kernel runs
        # instead of in a copy + widening pass afterwards (cfg2 catalogue: 2.9 ms against 2.6 + 1.0)
        direct = None
        if n_chunks == 1 and not log_times and os.environ.get("SF_API_DIRECT", "1") != "0":
            members = getattr(posteriors, "posteriors", [posteriors])
            try:
                if len(members) == 1 and members[0].posterior_estimator.flow.supports_f64_out():
                    direct = pinned_result((len(X), num_samples, len(self.fitted_parameter_names)))
            except AttributeError:
                direct = None
        if direct is not None:
            pin_t, samples = direct
        else:
            samples = result_array((len(X), num_samples, len(self.fitted_parameter_names)))
        times = []
        pending = []
        for ci in range(n_chunks):
            a, b = int(bounds[ci]), int(bounds[ci + 1])
            if b <= a:
                continue
            t0 = time.time()
            try:
                # the reference's per-object timeout (sbi_runner.py:6358) becomes the wall-clock ceiling of the chunk
                tmo = float(timeout_seconds_per_test) * (b - a) if timeout_seconds_per_test else None
                # (same seed, rows keyed by their position: the draws do not depend on the chunking)
                if direct is not None:
                    posteriors.sample_catalogue(torch.as_tensor(X[a:b]), num_samples, seed, timeout_seconds=tmo,
                                                row_offset=off + a, out=pin_t[a:b])
                    torch.cuda.synchronize()     # the host array is complete when the stream is
                    times.extend([(time.time() - t0) / (b - a)] * (b - a))
                    continue
                s = posteriors.sample_catalogue(torch.as_tensor(X[a:b]), num_samples, seed, timeout_seconds=tmo,
                                                row_offset=off + a)
                # D2H in float32 (half the PCIe bytes of a device-side .double()) through a ring of pinned staging buffers
                # on a copy stream, widened into the reference's float64 container by a thread pool while the next piece
                # is on the bus (hostio.py); with log_times the chunk's time includes its hand-over
                # (one chunk, or timed chunks: the call itself; several untimed chunks: a helper thread, so that the next
                #  chunk's kernels are launched meanwhile)
                if log_times or n_chunks == 1:
                    to_host_f64(s, out=samples[a:b])
                else:
                    pending.append((a, b, to_host_f64(s, out=samples[a:b], wait=False)))
            except Exception as e:  # sbi_runner.py:6458-6460: failed objects are NaN rows
                logger.error(f"Error occurred while sampling objects {a}..{b}: {e}")
                samples[a:b] = np.nan
            times.extend([(time.time() - t0) / (b - a)] * (b - a))
        for a, b, p in pending:
            try:
                p.result()
            except Exception as e:
                logger.error(f"Error occurred while copying objects {a}..{b} to the host: {e}")
                samples[a:b] = np.nan
        if log_times and times:
            self.last_times_per_object = np.asarray(times)
            self.last_time_per_object = float(np.median(times))
            logger.info(f"Median time per sample: {np.median(times):.5f} seconds."
                        f"16th-84th: {np.percentile(times, 16):.5f}-{np.percentile(times, 84):.5f}s.")
        return np.squeeze(samples, 0) if single else samples

    def log_prob(self, X: np.ndarray, y: np.ndarray, posteriors: object = None, verbose=True,
                 norm_posterior: bool = True, num_rejection_samples: int = 10000) -> np.ndarray:
        """(N,) float64 posterior log-density of y[i] given X[i]  (ref: sbi_runner.py:7188-7198; upstream
        DirectPosterior default norm_posterior=True -> leakage-corrected)."""
        if posteriors is None:
            posteriors = self.posteriors
        Xt = torch.as_tensor(np.asarray(X, dtype=np.float32))
        yt = torch.as_tensor(np.asarray(y, dtype=np.float32))
        from .posterior import all_gather_rows, broadcast_seed, dist_world, shard_bounds
        rank, world = dist_world()
        if world > 1 and Xt.dim() == 2 and yt.dim() == 2 and len(Xt) == len(yt) and len(Xt) >= world:
            # rank-sharded (rows independent, ref: sbi_runner.py:7193-7196): every rank evaluates its row block; the
            # DISTINCT contexts behind the leakage correction are split over the ranks too and their acceptance rates
            # gathered, with streams keyed by the position in the sorted list of distinct rows -- same result as one process
            b = shard_bounds(len(Xt), world)
            members = getattr(posteriors, "posteriors", [posteriors])
            acc = None
            if norm_posterior and posteriors.prior is not None:
                dev = members[0].device
                acc = []
                for mem in members:
                    E = mem._embed(Xt)
                    ux, inv = torch.unique(E, dim=0, return_inverse=True)
                    ub = shard_bounds(ux.shape[0], world)
                    seed = broadcast_seed(mem._next_seed(None))
                    part = mem.acceptance_rows(ux[ub[rank]:ub[rank + 1]], num_rejection_samples, seed, row_offset=ub[rank])
                    acc_all = all_gather_rows(part, ub) if ux.shape[0] >= world else mem.acceptance_rows(ux, num_rejection_samples, seed)
                    acc.append(acc_all.to(dev)[inv][b[rank]:b[rank + 1]])
            sl = slice(b[rank], b[rank + 1])
            if hasattr(posteriors, "posteriors"):
                lp = posteriors.log_prob_catalogue(yt[sl], Xt[sl], norm_posterior, num_rejection_samples, acc=acc)
            else:
                lp = posteriors.log_prob_catalogue(yt[sl], Xt[sl], norm_posterior, num_rejection_samples,
                                                   **({} if acc is None else {"acc_rows": acc[0]}))
            return all_gather_rows(lp.contiguous(), b).double().cpu().numpy()
        lp = posteriors.log_prob_catalogue(yt, Xt, norm_posterior, num_rejection_samples)
        return lp.double().cpu().numpy()

    def _map_rows(self, X, posteriors, row_offset: int = 0, **map_kwargs):
        """(theta_map (N, D), log_prob_map (N,)) float64 of the rows of X; under a process group rank r works rows
        [r N / W, (r+1) N / W) and the blocks are gathered on every rank (streams keyed by the row's position)."""
        from .map import check_map_args
        from .posterior import all_gather_rows, broadcast_seed, dist_world, shard_bounds
        kw = dict(num_iter=1000, num_to_optimize=100, learning_rate=0.01, init_method="posterior", num_init_samples=1000,
                  save_best_every=10, seed=None)
        unknown = {k: v for k, v in map_kwargs.items() if k not in kw and k not in ("show_progress_bars", "force_update")}
        if unknown:
            raise TypeError(f"calculate_MAP: unknown keyword(s) {sorted(unknown)}")
        kw.update({k: v for k, v in map_kwargs.items() if k in kw})
        check_map_args(kw["num_iter"], kw["num_to_optimize"], kw["learning_rate"], kw["init_method"], kw["num_init_samples"],
                       kw["save_best_every"])
        Xt = torch.as_tensor(np.asarray(X, dtype=np.float32))
        rank, world = dist_world()
        if world > 1 and len(Xt) >= world:
            if kw["seed"] is None:
                kw["seed"] = posteriors._next_seed(None)
            kw["seed"] = broadcast_seed(kw["seed"])
            b = shard_bounds(len(Xt), world)
            sl = slice(b[rank], b[rank + 1])
            if torch.is_tensor(kw["init_method"]):
                kw["init_method"] = kw["init_method"][sl]
            th, lp = posteriors.map_catalogue(Xt[sl], row_offset=int(row_offset) + b[rank], **kw)
            th, lp = all_gather_rows(th.contiguous(), b), all_gather_rows(lp.contiguous(), b)
        else:
            th, lp = posteriors.map_catalogue(Xt, row_offset=int(row_offset), **kw)
        return th.double().cpu().numpy(), lp.double().cpu().numpy()

    def calculate_MAP(self, X: np.ndarray = None, posteriors: object = None, **map_kwargs) -> np.ndarray:
        """(N, D) float64 posterior mode of every row of X (default: the test split).  The reference names the method and
        leaves it empty (sbi_runner.py:7204-7207); this is [UPSTREAM] sbi ``posterior.map`` per row, with its keywords
        (``num_iter``, ``num_to_optimize``, ``learning_rate``, ``init_method``, ``num_init_samples``, ``save_best_every``)
        plus ``seed``.  The log-density at the modes is kept in ``self.last_map_log_prob``.  Like ``sample_posterior``
        the result is in the units the posterior was trained in (``prior_method="manual"``: nothing un-scales, as there);
        under a process group the rows are sharded like ``sample_posterior``'s and every rank returns the whole array."""
        if posteriors is None:
            posteriors = self.posteriors
        if X is None:
            if getattr(self, "_X_test", None) is not None:
                X = self._X_test
            else:
                raise ValueError("X must be provided or set in the object.")
        X = np.asarray(X, dtype=np.float32)
        if X.ndim == 1:
            X = X[None, :]
        th, lp = self._map_rows(X, posteriors, **map_kwargs)
        self.last_map_log_prob = lp
        return th

    def save_state(self, out_dir, name_append: str = "", save_method: str = "joblib", has_grid: bool = True, **extras):
        """ref: sbi_runner.py:693-830 -- what a later session needs next to ``{name}_{append}_posterior.pkl``: feature /
        parameter names and units, the prior, the feature-array flags and (``has_grid``) the feature and parameter
        arrays, plus ``extras`` (train arguments, split indices, stats ...), as ``{name}{_append}_params.pkl``
        (``save_method`` 'joblib' -- the reference's default --, 'pickle' or 'torch'); ``stats`` also go to
        ``{name}{_append}_summary.json`` with the scalar entries of the dictionary appended."""
        import json
        import pickle
        os.makedirs(out_dir, exist_ok=True)
        param_dict = {"feature_names": self.feature_names, "feature_units": self.feature_units,
                      "fitted_parameter_units": self.fitted_parameter_units,
                      "fitted_parameter_names": self.fitted_parameter_names,
                      "timestamp": time.strftime("%Y%m%d_%H%M%S"), "prior": self._prior,
                      "library_path": self.library_path, "name": self.name, "has_simulator": self.has_simulator}
        if len(name_append) > 0 and name_append[0] != "_":
            name_append = f"_{name_append}"
        save_path = f"{out_dir}/{self.name}{name_append}_params.pkl"
        param_dict.update(extras)
        if has_grid:
            param_dict["feature_array_flags"] = getattr(self, "feature_array_flags", {})
            if getattr(self, "feature_wavelengths", None) is not None:      # spectra features: the M output wavelengths in um
                param_dict["feature_wavelengths"] = self.feature_wavelengths
            param_dict["feature_array"] = self.feature_array
            param_dict["parameter_array"] = self.fitted_parameter_array
        if "stats" in param_dict:
            summary = list(param_dict["stats"]) + [{k: v for k, v in param_dict.items()
                                                    if isinstance(v, (list, str, float, int, bool)) and k != "stats"}]
            try:
                with open(f"{out_dir}/{self.name}{name_append}_summary.json", "w") as fh:
                    json.dump(summary, fh, indent=4, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o))
            except Exception as e:  # (the reference logs and goes on)
                logger.error(f"Error saving stats: {e}")
        if save_method == "joblib":
            from joblib import dump
            dump(param_dict, save_path, compress=3)
        elif save_method == "pickle":
            with open(save_path, "wb") as fh:
                pickle.dump(param_dict, fh, protocol=pickle.HIGHEST_PROTOCOL)
        elif save_method == "torch":
            torch.save(param_dict, save_path)
        else:
            raise ValueError("save_method: 'joblib', 'pickle' or 'torch' on the HIP path")
        return save_path

    def load_model_from_pkl(self, model_file: str, set_self: bool = True, load_arrays: bool = True):
        """ref: sbi_runner.py:7401-7633 -- (posteriors, stats, params) of a model trained by THIS backend: ``model_file`` is
        the ``*_posterior.pkl`` or the directory that holds exactly one; ``*_summary.json`` and ``*_params.pkl`` next to
        it are read when present and, with ``set_self``, put back on the fitter (names, units, flags, prior, arrays,
        the train / test split).  sbi's own pickles need sbi and stay outside the build (see ``importer.py`` for their
        weights)."""
        import glob
        import json
        import pickle
        if not os.path.exists(model_file):
            raise ValueError(f"Model file {model_file} does not exist.")
        if os.path.isdir(model_file):
            files = glob.glob(os.path.join(model_file, "*_posterior.pkl"))
            if len(files) == 0:
                raise ValueError(f"No parameter files found in {model_file}.")
            if len(files) > 1:
                raise ValueError(f"Multiple parameter files found in {model_file}.\n                    Please specify a single file.")
            model_file = files[0]
        with open(model_file, "rb") as fh:
            posteriors = pickle.load(fh)
        stats = None
        sfile = model_file.replace("posterior.pkl", "summary.json")
        if os.path.exists(sfile):
            with open(sfile, "r", encoding="utf-8") as fh:
                stats = json.load(fh)
            if set_self:
                self.stats = stats
        else:
            logger.info(f"Warning: No summary file found for {model_file}.")
        if hasattr(posteriors, "to"):
            posteriors = posteriors.to(self.device) or posteriors
        if set_self:
            self.posteriors = posteriors
        pfile = model_file.replace("posterior.pkl", "params.pkl")
        params = None
        if os.path.exists(pfile):
            try:
                from joblib import load as jl_load
                params = jl_load(pfile)
            except Exception:
                try:
                    with open(pfile, "rb") as fh:
                        params = pickle.load(fh)
                except Exception:
                    params = torch.load(pfile, map_location="cpu", weights_only=False)
            if set_self:
                self.fitted_parameter_names = list(params["fitted_parameter_names"])
                self.simple_fitted_parameter_names = [str(i).split("/")[-1] for i in self.fitted_parameter_names]
                self.fitted_parameter_units = params.get("fitted_parameter_units", self.parameter_units)
                self.feature_names = params["feature_names"]
                self.feature_units = params.get("feature_units", None)
                if "feature_array_flags" in params:
                    self.feature_array_flags = params["feature_array_flags"]
                    self.has_features = True
                if "feature_wavelengths" in params:
                    self.feature_wavelengths = params["feature_wavelengths"]
                if load_arrays and params.get("feature_array") is not None:
                    self.fitted_parameter_array = params["parameter_array"]
                    self.feature_array = params["feature_array"]
                    self.has_features = True
                    self._train_indices = params.get("train_indices")
                    self._test_indices = params.get("test_indices")
                    self._train_fraction = params.get("train_fraction")
                    if self._train_indices is not None and self._test_indices is not None:
                        self._X_test = self.feature_array[self._test_indices]
                        self._y_test = self.fitted_parameter_array[self._test_indices]
                        self._X_train = self.feature_array[self._train_indices]
                        self._y_train = self.fitted_parameter_array[self._train_indices]
                self._train_args = params.get("train_args")
                self._prior = params.get("prior")
                self._ensemble_model_types = params.get("ensemble_model_types")
                self._ensemble_model_args = params.get("ensemble_model_args")
        else:
            logger.warning(f"No parameter file found for {model_file}.")
        return posteriors, stats, params

    def create_features_from_observations(self, observations, columns_to_feature_names: dict = None, flux_units=None,
                                          missing_data_flag=-99, override_transformations: dict = {},
                                          ignore_missing: bool = False):
        """ref: sbi_runner.py:2473-2937 -- the observed catalogue as the (N', F) float32 feature array the model was
        trained on, plus the mask of removed rows, from the transformations recorded by
        ``create_feature_array_from_raw_photometry`` (``self.feature_array_flags``).

        When the flags hold empirical noise models and the error columns are features, each band's flux and error columns
        first go through its model's ``apply_scalings`` from ``flux_units`` to the training unit (2767-2843, on the device).
        Otherwise, as in the reference, the photometry columns must ALREADY be in the training units (``flux_units`` has to equal
        ``normed_flux_units``, an assertion there too); what happens then is column mapping and validation (every
        filter, every ``unc_`` column when errors were features, the ``norm_<filter>_<unit>`` column), the error-NaN
        check, the normalisation step exactly as the reference writes it (2844-2865), removal of rows that carry the
        missing-data flag, the ``norm_mag_limit`` clip and inf -> NaN.  Flags and simulated missing fluxes are outside the
        HIP path."""
        import pandas as pd
        flags = dict(getattr(self, "feature_array_flags", None) or {})
        if len(flags) == 0:
            raise ValueError("No feature array flags found. Please create the feature array first.")
        flags.update(override_transformations)
        if not isinstance(observations, pd.DataFrame):
            raise TypeError("Observations must be a pandas DataFrame or an astropy Table.")
        if columns_to_feature_names is None:
            columns_to_feature_names = {col: col for col in observations.columns}
        feature_names_to_columns = {v: k for k, v in columns_to_feature_names.items()}
        for name in flags["raw_observation_names"]:
            if name not in feature_names_to_columns:
                raise ValueError(f"Column '{name}' not found in observations. Please provide a mapping for all photometry filters.")
        if flags.get("include_errors_in_feature_array"):
            for name in flags["error_names"]:
                if name not in feature_names_to_columns:
                    raise ValueError(f"Column '{name}' not found in observations. Please provide a mapping for all errors.")
        if flags.get("norm_name") is not None and flags["norm_name"] not in feature_names_to_columns:
            raise ValueError(f"Column '{flags['norm_name']}' not found in\n                observations. "
                             "Please provide a mapping for the normalization factor.")
        training_flux_units = flags["normed_flux_units"]
        fnames = list(self.feature_names)
        nrows, ncols = observations.shape[0], np.shape(self.feature_array)[1]
        fa = np.zeros((ncols, nrows), dtype=np.float32)
        photometry_columns = [feature_names_to_columns[name] for name in flags["raw_observation_names"]]
        for col in photometry_columns:
            if col not in observations.columns:
                raise ValueError(f"Column '{col}' not found in observations.\n                    "
                                 "Please provide a mapping for all photometry filters.")
            fa[fnames.index(columns_to_feature_names[col]), :] = observations[col].values
        err_names = flags["error_names"] if flags.get("include_errors_in_feature_array") else []
        for col in err_names:
            ocol = feature_names_to_columns[col]
            if ocol not in observations.columns:
                raise ValueError(f"Column '{ocol}' not found in observations.\n                    "
                                 "Please provide a mapping for all errors.")
            fa[fnames.index(col), :] = observations[ocol].values
        for col in err_names:
            ev, fv = fa[fnames.index(col), :], fa[fnames.index(col.replace("unc_", "")), :]
            bad = np.isnan(ev) & ~np.isnan(fv)
            if np.sum(bad) > 0:
                raise ValueError(f"Error column '{col}' contains NaN values where the\n                    corresponding flux "
                                 f"column '{col.replace('unc_', '')}' does not.{np.sum(bad)} NaN values found.")
        if flags.get("empirical_noise_models") is not None and err_names:
            flux_units = self._apply_model_scalings(fa, fnames, flags, columns_to_feature_names, feature_names_to_columns,
                                                    flux_units, missing_data_flag)
        assert flux_units == training_flux_units, (f"Flux units '{flux_units}' do not match\n                    "
                                                   f"training data units '{training_flux_units}'.")
        if flags.get("norm_name") is not None:
            ncol = feature_names_to_columns[flags["norm_name"]]
            if ncol not in observations.columns:
                raise ValueError(f"Column '{flags['norm_name']}'\n                    not found in observations.\n"
                                 "                    Please provide a mapping for the normalization factor.")
            fa[fnames.index(flags["norm_name"]), :] = observations[ncol].values
        if flags.get("normalize_method") is not None:
            nf = fa[fnames.index(flags["norm_name"]), :]
            # exactly as the reference writes it (2847-2849): the AB column goes back to a uJy flux and is SUBTRACTED
            nf = 10 ** ((23.9 - nf) / 2.5)
            for col in photometry_columns:
                i = fnames.index(columns_to_feature_names[col])
                fa[i, :] = np.subtract(fa[i, :], nf)
        removed = np.zeros(nrows, dtype=bool)
        missing = np.isnan(fa) if (isinstance(missing_data_flag, float) and np.isnan(missing_data_flag)) else (fa == missing_data_flag)
        if not ignore_missing:
            if missing.sum() > 0:
                logger.info(f"Removing {int(missing.sum())} observations with missing data.")
            removed[missing.any(axis=0)] = True
        fa, missing = fa[:, ~removed], missing[:, ~removed]
        clip = (fa > flags["norm_mag_limit"]) & ~missing
        fa[clip] = flags["norm_mag_limit"]
        fa[~np.isfinite(fa)] = np.nan
        return fa.T, removed

    def _apply_model_scalings(self, fa, fnames, flags, columns_to_feature_names, feature_names_to_columns, flux_units,
                              missing_data_flag):
        """ref: sbi_runner.py:2767-2843 -- each band's flux and error rows of ``fa`` through its noise model's
        ``apply_scalings`` (``sf_apply_scalings``), from ``flux_units`` to the training unit; a band without a matching
        ``unc_`` column is skipped with a warning.  Entries that carry the missing-data flag keep it.  Returns the unit the
        photometry is in afterwards."""
        from .features import apply_scalings
        from .noise_models import UncertaintyModel
        if not torch.cuda.is_available():
            raise RuntimeError("create_features_from_observations with empirical noise models runs on the GPU (no CPU fallback)")
        rows, models = [], []
        for model_name, model in flags["empirical_noise_models"].items():
            if not isinstance(model, UncertaintyModel):
                raise TypeError(f"Invalid empirical noise model type: {type(model)}. Expected an EmpiricalUncertaintyModel instance.")
            if model_name in columns_to_feature_names:
                model_name = columns_to_feature_names[model_name]
            if model_name not in feature_names_to_columns or model_name not in fnames:
                logger.warning(f"Empirical noise model '{model_name}' not found in feature names.")
                continue
            eindex, tail = None, model_name.split(".")[-1]
            for ecol in flags["error_names"]:
                if ecol == f"unc_{model_name}" or (ecol.startswith("unc_") and ecol.endswith(tail)):
                    eindex = fnames.index(ecol)
                    break
            if eindex is None:
                logger.warning(f"No matching error column for '{model_name}'. Skipping empirical scaling.")
                continue
            rows.append((fnames.index(model_name), eindex))
            models.append(model)
        if models:
            fi, ei = [r[0] for r in rows], [r[1] for r in rows]
            f_in, e_in = fa[fi, :].T, fa[ei, :].T
            new_f, new_e = apply_scalings(torch.as_tensor(np.ascontiguousarray(f_in)).cuda(),
                                          torch.as_tensor(np.ascontiguousarray(e_in)).cuda(), models, flux_units,
                                          flags["normed_flux_units"])
            new_f, new_e = new_f.cpu().numpy(), new_e.cpu().numpy()
            if not (isinstance(missing_data_flag, float) and np.isnan(missing_data_flag)):
                new_f = np.where(f_in == missing_data_flag, f_in, new_f)
                new_e = np.where(e_in == missing_data_flag, e_in, new_e)
            fa[fi, :], fa[ei, :] = new_f.T, new_e.T
        return flags["normed_flux_units"]

    def fit_catalogue(self, observations, columns_to_feature_names: dict = None, num_samples: int = 1000,
                      quantiles=(0.16, 0.5, 0.84), sample_method: str = "direct", append_to_input: bool = True,
                      return_samples: bool = False, log_times: bool = False, seed: Optional[int] = None,
                      device_quantiles: bool = True, flux_units=None, missing_data_flag=-99,
                      override_transformations: dict = {}, timeout_seconds_per_row: float = 5,
                      return_feature_array: bool = False, return_full_samples: bool = False,
                      missing_data_mcmc: bool = False, missing_data_mcmc_params: Optional[dict] = None,
                      missing_data_sigma=None, check_out_of_distribution: bool = False, outlier_methods=None,
                      map_estimate: bool = False, map_kwargs: Optional[dict] = None,
                      fixed_parameters: Optional[dict] = None, conditional_kwargs: Optional[dict] = None, **unknown):
        """Sampling + quantile section of the reference's fit_catalogue (sbi_runner.py:3230-3282).

        ``fixed_parameters`` (an addition; default None: the call is what it was): a dict from parameter name to a scalar,
        an (N,) array or the name of a column of ``observations`` -- the rows where it holds a finite value are fitted with
        that parameter held at it (``sample_conditional_posterior``; ``conditional_kwargs``: its keywords).  Their quantile
        columns come from the conditional draws, so a fixed parameter's quantiles equal its value, and the table gains
        ``conditional_acceptance`` (NaN where nothing was fixed).  Rows whose fixed entries are all NaN are sampled as
        without the keyword, bit for bit; masked, out-of-distribution and missing-band rows stay NaN; the ``map_estimate``
        columns stay those of the unconditional posterior.  Not combined with ``missing_data_mcmc``.  Under a process group
        every rank runs the whole conditional call.

        ``map_estimate=True`` (an addition; default False: the call is what it was): the table gains ``{param}_map`` per
        parameter and ``map_log_prob`` -- the posterior mode of every row by ``calculate_MAP`` (``map_kwargs``: its
        keywords) -- NaN for masked rows, out-of-distribution rows and rows with missing bands.  The quantile columns are
        those of the same call without the switch: the MAP inits are drawn on a seed stream of their own.

        ``observations`` is a pandas DataFrame / dict of columns / (N, C) array.  With ``flux_units`` given and a feature
        array that was built by ``create_feature_array_from_raw_photometry`` the table goes through
        ``create_features_from_observations`` first (3061-3068: column mapping, normalisation, missing-data rows);
        otherwise its columns are taken as the model's feature columns.  Masked rows get NaN quantiles.
        ``timeout_seconds_per_row`` (reference default 5 s) x rows is the wall-clock ceiling of the catalogue call
        (sbi_runner.py:3246-3253); ``return_feature_array`` returns (feature_array, mask) like line 3092-3094;
        ``return_full_samples`` is the reference's name for ``return_samples``.

        ``missing_data_mcmc=True`` (sbi_runner.py:3102-3219, 3284-3317): rows whose only defect is the missing-data flag are
        not dropped but marginalised over their missing bands by ``MissingPhotometryHandler`` (synference_amd/missing.py:
        ``nmc`` imputations x ``nposterior`` draws, pooled; ``missing_data_mcmc_params`` are its ``run_params`` and ARE applied,
        unlike in the reference).  Complete rows are sampled exactly as without the switch.  The table gains
        ``has_missing_data`` and, per band that was imputed somewhere, ``predicted_<band>``; a row the handler fails on
        keeps NaN quantiles; with ``return_samples`` the flagged rows are NaN in the (N, num_samples, D) array (their pooled
        draws have another length: ``self.missing_handler.last_posterior_samples``).  The chi2 uncertainty is the row's error
        feature columns when errors are features, else ``missing_data_sigma`` (scalar, [B] or (N, B)) -- an addition.

        ``check_out_of_distribution=True`` (sbi_runner.py:3078-3092, 3299-3305; the reference's default is True, here it is
        False: DESIGN.md section 0): every complete row is tested against ``self.feature_array`` by
        ``test_in_distribution_pyod(methods=outlier_methods, contamination=0.01)`` -- ``outlier_methods=None`` means
        ("knn", "lof", "kde"), majority rule -- on the device (synference_amd/ood.py).  Flagged rows join the row mask: they
        are not sampled, their quantiles are NaN and ``is_outlier`` is the final row mask.  The other rows keep the draws
        they would have had (the random streams are keyed by the row's position).  Rows with missing bands
        (``missing_data_mcmc``) are not checked.  Under a process group every rank runs the whole check."""
        import pandas as pd
        _warn_unknown("fit_catalogue", unknown)
        return_samples = return_samples or return_full_samples
        if fixed_parameters is not None and not return_feature_array:
            if missing_data_mcmc:
                raise ValueError("fit_catalogue: fixed_parameters cannot be combined with missing_data_mcmc=True (the pooled draws "
                                 "of an imputed row are unconditional)")
            return self._fit_catalogue_conditional(
                observations, fixed_parameters, conditional_kwargs,
                dict(columns_to_feature_names=columns_to_feature_names, num_samples=num_samples, quantiles=quantiles,
                     sample_method=sample_method, append_to_input=append_to_input, return_samples=return_samples,
                     log_times=log_times, seed=seed, device_quantiles=device_quantiles, flux_units=flux_units,
                     missing_data_flag=missing_data_flag, override_transformations=override_transformations,
                     timeout_seconds_per_row=timeout_seconds_per_row, check_out_of_distribution=check_out_of_distribution,
                     outlier_methods=outlier_methods, map_estimate=map_estimate, map_kwargs=map_kwargs))
        ood_kw = dict(check_out_of_distribution=check_out_of_distribution, outlier_methods=outlier_methods)
        ood_kw.update(map_estimate=map_estimate, map_kwargs=map_kwargs)   # (both travel with the check to the inner call)
        if missing_data_mcmc and not return_feature_array:
            return self._fit_catalogue_missing(observations, columns_to_feature_names, missing_data_flag, flux_units,
                                               override_transformations, missing_data_mcmc_params, missing_data_sigma, quantiles,
                                               append_to_input, return_samples, seed,
                                               dict(num_samples=num_samples, quantiles=quantiles, sample_method=sample_method,
                                                    log_times=log_times, seed=seed, device_quantiles=device_quantiles,
                                                    timeout_seconds_per_row=timeout_seconds_per_row, **ood_kw))
        if flux_units is not None and getattr(self, "feature_array_flags", None):
            df0 = pd.DataFrame(observations) if isinstance(observations, dict) else observations
            feats_ok, removed = self.create_features_from_observations(df0, columns_to_feature_names, flux_units,
                                                                       missing_data_flag, override_transformations)
            if return_feature_array:
                if check_out_of_distribution and len(feats_ok):
                    removed = removed.copy()
                    removed[~removed] |= self._catalogue_outliers(feats_ok, outlier_methods)
                return feats_ok, removed
            full = np.full((len(df0), feats_ok.shape[1]), np.nan, dtype=np.float32)
            full[~removed] = feats_ok
            out = self.fit_catalogue(full, columns_to_feature_names=None, num_samples=num_samples, quantiles=quantiles,
                                     sample_method=sample_method, append_to_input=False, return_samples=return_samples,
                                     log_times=log_times, seed=seed, device_quantiles=device_quantiles,
                                     timeout_seconds_per_row=timeout_seconds_per_row, **ood_kw)
            qt = out[0] if return_samples else out
            table = df0.copy() if append_to_input else pd.DataFrame({"ID": np.arange(len(df0)) + 1})
            for c in qt.columns:
                if c != "ID":
                    table[c] = qt[c].to_numpy()
            return (table, out[1]) if return_samples else table
        if isinstance(observations, np.ndarray):
            df = pd.DataFrame(observations, columns=list(self.feature_names)[: observations.shape[1]])
        elif isinstance(observations, dict):
            df = pd.DataFrame(observations)
        else:
            df = observations.copy()
        cols = list(self.feature_names)
        if columns_to_feature_names:
            df = df.rename(columns=columns_to_feature_names)
        missing = [c for c in cols if c not in df.columns]
        if missing:
            raise ValueError(f"observations lack the feature columns {missing}")
        feats = df[cols].to_numpy(dtype=np.float32)
        finite = np.isfinite(feats).all(1)
        obs_mask = ~finite
        good = feats[finite]                      # the rows' positions here key their random streams, flagged or not
        keep = np.ones(len(good), bool)
        if check_out_of_distribution and len(good):
            keep = ~self._catalogue_outliers(good, outlier_methods)
            obs_mask = obs_mask.copy()
            obs_mask[~obs_mask] = ~keep
        if return_feature_array:
            return good, obs_mask                    # sbi_runner.py:3093-3095: the features as built, the mask with the outliers
        edges = np.flatnonzero(np.diff(np.concatenate([[False], keep, [False]]).astype(np.int8)))
        runs = list(zip(edges[0::2].tolist(), edges[1::2].tolist()))   # [a, b) blocks of rows to sample
        kept_runs, seed_given = list(runs), seed     # (for the MAP columns: the runs and the seed as the caller gave them)
        if seed is None and len(runs) > 1:
            seed = self.posteriors._next_seed(None)
        tmo = float(timeout_seconds_per_row) * max(1, int((~obs_mask).sum())) if timeout_seconds_per_row else None
        if device_quantiles and not return_samples and num_samples <= 8192:
            # f3: quantiles reduced on the GPU; only (N, D, Q) floats cross PCIe
            from .posterior import device_quantiles as _dq
            table = df.copy() if append_to_input else pd.DataFrame({"ID": np.arange(len(df)) + 1})
            qarr = np.full((len(df), len(self.fitted_parameter_names), len(quantiles)), np.nan)
            if (~obs_mask).any():
                if sample_method != "direct":
                    raise ValueError("Invalid sample method for the HIP backend. Use 'direct'.")
                from .posterior import all_gather_rows, broadcast_seed, dist_world, shard_bounds
                rank, world = dist_world()
                def block(lo, hi):
                    """quantiles of rows [lo, hi) of `good`, NaN for flagged rows: one sampler call per run of kept rows"""
                    if runs == [(lo, hi)]:
                        s_dev = self.posteriors.sample_catalogue(torch.as_tensor(good[lo:hi]), num_samples, seed,
                                                                 timeout_seconds=tmo, row_offset=lo)
                        return _dq(s_dev, quantiles)
                    q = None
                    for a, b in runs:
                        a, b = max(a, lo), min(b, hi)
                        if b <= a:
                            continue
                        s_dev = self.posteriors.sample_catalogue(torch.as_tensor(good[a:b]), num_samples, seed,
                                                                 timeout_seconds=tmo, row_offset=a)
                        qr = _dq(s_dev, quantiles)
                        if q is None:
                            q = torch.full((hi - lo,) + tuple(qr.shape[1:]), float("nan"), dtype=qr.dtype, device=qr.device)
                        q[a - lo:b - lo] = qr
                    if q is None:
                        q = torch.full((hi - lo, len(self.fitted_parameter_names), len(quantiles)), float("nan"),
                                       dtype=torch.float32, device=self.posteriors.device)
                    return q
                if world > 1 and len(good) >= world:   # rank r: its row block; only the (n, D, Q) quantiles are gathered
                    if seed is None:
                        seed = self.posteriors._next_seed(None)
                    seed = broadcast_seed(seed)
                    b = shard_bounds(len(good), world)
                    if runs == [(0, len(good))]:
                        runs = [(int(b[rank]), int(b[rank + 1]))]
                    qarr[finite] = all_gather_rows(block(int(b[rank]), int(b[rank + 1])).contiguous(), b).double().cpu().numpy()
                else:
                    qarr[finite] = block(0, len(good)).double().cpu().numpy()
            for i, param in enumerate(self.simple_fitted_parameter_names):
                for j, qv in enumerate(quantiles):
                    table[f"{param}_{int(qv * 100)}"] = qarr[:, i, j]
            if check_out_of_distribution:
                table["is_outlier"] = obs_mask
            if map_estimate:
                self._add_map_columns(table, good, np.flatnonzero(finite), kept_runs, seed_given, map_kwargs)
            return table
        samples = np.full((len(df), num_samples, len(self.fitted_parameter_names)), np.nan)
        pos = np.flatnonzero(finite)
        for a, b in runs:
            samples[pos[a:b]] = self.sample_posterior(good[a:b], sample_method=sample_method,
                                                      num_samples=num_samples, log_times=log_times, seed=seed,
                                                      timeout_seconds_per_test=timeout_seconds_per_row,
                                                      gather="all", row_offset=a)   # every rank fills the whole table
        samples_quant = samples.transpose(2, 0, 1)
        table = df.copy() if append_to_input else pd.DataFrame({"ID": np.arange(len(df)) + 1})
        for i, param in enumerate(self.simple_fitted_parameter_names):
            with np.errstate(invalid="ignore"):
                q = np.nanquantile(samples_quant[i], quantiles, axis=1) if (~obs_mask).any() else \
                    np.full((len(quantiles), len(df)), np.nan)
            for j, quant in enumerate(q):
                col = np.asarray(quant, dtype=np.float64)
                col[obs_mask] = np.nan
                table[f"{param}_{int(quantiles[j] * 100)}"] = col
        if check_out_of_distribution:
            table["is_outlier"] = obs_mask
        if map_estimate:
            self._add_map_columns(table, good, pos, kept_runs, seed_given, map_kwargs)
        return (table, samples) if return_samples else table

    def _add_map_columns(self, table, good, pos, runs, seed, map_kwargs):
        """fit_catalogue(map_estimate=True): ``{param}_map`` and ``map_log_prob`` from the rows the quantile path sampled --
        ``good`` (table rows ``pos``), its ``runs`` [a, b) of kept rows -- NaN elsewhere.  One ``_map_rows`` call per run,
        streams keyed by the row's position in ``good``; an (N, R0, D) ``init_method`` tensor is indexed by table row."""
        th = np.full((len(table), len(self.fitted_parameter_names)), np.nan)
        lp = np.full(len(table), np.nan)
        mk = dict(map_kwargs or {})
        if "seed" not in mk:   # a stream of its own: the quantile draws of this call do not move
            mk["seed"] = None if seed is None else (int(seed) + 0xD1B54A32D192ED03) & (2 ** 63 - 1)
        if mk["seed"] is None and len(runs) > 1:
            mk["seed"] = self.posteriors._next_seed(None)
        inits = mk.get("init_method")
        if torch.is_tensor(inits) and (inits.dim() != 3 or inits.shape[0] != len(table)):
            raise ValueError(f"map_kwargs['init_method']: an (N = {len(table)}, R0, D) tensor, one block of inits per table row, "
                             f"not {tuple(inits.shape)}")
        for a, b in runs:
            if torch.is_tensor(inits):
                mk["init_method"] = inits[torch.as_tensor(pos[a:b])]
            th[pos[a:b]], lp[pos[a:b]] = self._map_rows(good[a:b], self.posteriors, row_offset=a, **mk)
        for i, param in enumerate(self.simple_fitted_parameter_names):
            table[f"{param}_map"] = th[:, i]
        table["map_log_prob"] = lp

    # ---- conditional posteriors (synference_amd/conditional.py) ---------------------------------------------------------------
    def _fixed_condition(self, fixed_parameters: dict, N: int, table=None) -> np.ndarray:
        """``fixed_parameters`` -> the (N, D) float32 condition of ``sample_conditional_catalogue`` (NaN = free): a value is a
        scalar, an (N,) array or -- with ``table`` -- the name of one of its columns.  No GPU needed."""
        names = list(self.fitted_parameter_names)
        simple = list(getattr(self, "simple_fitted_parameter_names", None) or names)
        if not isinstance(fixed_parameters, dict):
            raise TypeError("fixed_parameters must be a dict from parameter name to a scalar, an (N,) array or a column name")
        cond = np.full((N, len(names)), np.nan, dtype=np.float32)
        for key, val in fixed_parameters.items():
            if key in names:
                d = names.index(key)
            elif key in simple:
                d = simple.index(key)
            else:
                raise ValueError(f"fixed_parameters: unknown parameter '{key}'; the fitted parameters are {names}")
            if isinstance(val, str):
                if table is None or val not in table:
                    raise ValueError(f"fixed_parameters['{key}']: '{val}' is not a column of the observations")
                val = np.asarray(table[val], dtype=np.float64)
            val = np.asarray(val, dtype=np.float64)
            if val.ndim > 1 or (val.ndim == 1 and len(val) != N):
                raise ValueError(f"fixed_parameters['{key}']: a scalar or an (N = {N},) array, not {val.shape}")
            cond[:, d] = val
        return cond

    def sample_conditional_posterior(self, X_test: np.ndarray = None, fixed_parameters: dict = None, num_samples: int = 1000,
                                     posteriors: object = None, seed: Optional[int] = None, row_offset: int = 0,
                                     **conditional_kwargs) -> np.ndarray:
        """(num_objects, num_samples, num_parameters) float64 draws with the parameters of ``fixed_parameters`` -- a dict
        from parameter name to a scalar or an (N,) array, NaN = free in that row -- held at the given values: the first
        follow-up of an SED fit ("this galaxy has a spectroscopic redshift").  [UPSTREAM] reaches it through
        ``sbi.analysis.conditional_potential`` behind an MCMC posterior, one Python chain per object; here every row runs
        an ensemble sampler on the device (``sample_conditional_catalogue``; ``conditional_kwargs``: ``num_walkers``,
        ``burn_in``, ``thin``, ``num_init_samples``).  The accepted fraction per row -- the diagnostic to quote -- is kept in
        ``self.last_conditional_acceptance``; NaN rows as there.  Under a process group every rank runs the whole call."""
        from .conditional import check_conditional_args
        if posteriors is None:
            posteriors = self.posteriors
        if X_test is None:
            if getattr(self, "_X_test", None) is not None:
                X_test = self._X_test
            else:
                raise ValueError("X_test must be provided or set in the object.")
        if fixed_parameters is None:
            raise ValueError("sample_conditional_posterior needs fixed_parameters")
        X = np.asarray(X_test, dtype=np.float32)
        if X.ndim == 1:
            X = X[None, :]
        kw = dict(num_walkers=64, burn_in=200, thin=5, num_init_samples=1000, dims_to_sample=None)
        unknown = {k: v for k, v in conditional_kwargs.items() if k not in kw}
        if unknown:
            raise TypeError(f"sample_conditional_posterior: unknown keyword(s) {sorted(unknown)}")
        kw.update(conditional_kwargs)
        cond = self._fixed_condition(fixed_parameters, len(X))
        check_conditional_args(num_samples, kw["num_walkers"], kw["burn_in"], kw["thin"], kw["num_init_samples"])
        from .hostio import to_host_f64
        s, acc = posteriors.sample_conditional_catalogue(torch.as_tensor(X), cond, num_samples=num_samples, seed=seed,
                                                         row_offset=int(row_offset), **kw)
        self.last_conditional_acceptance = acc.double().cpu().numpy()
        return to_host_f64(s)

    def _fit_catalogue_conditional(self, observations, fixed_parameters, conditional_kwargs, kw):
        """fit_catalogue(fixed_parameters=...): the ordinary call first, then the rows with something fixed are drawn again
        from their conditional posterior and their quantile columns replaced.  The streams are keyed by the row's position
        among the complete rows, like the ordinary call's."""
        import pandas as pd
        from .posterior import device_quantiles as _dq, device_quantiles_large as _dql
        table_in = pd.DataFrame(observations) if isinstance(observations, dict) else observations
        named = table_in if hasattr(table_in, "columns") else None
        cond = self._fixed_condition(fixed_parameters, len(table_in), named)
        ckw = dict(conditional_kwargs or {})
        out = self.fit_catalogue(observations, **kw)
        table = out[0] if kw["return_samples"] else out
        # the complete rows as the ordinary call saw them (their positions key the streams), then the rows it sampled
        fa_kw = {k: kw[k] for k in ("columns_to_feature_names", "flux_units", "missing_data_flag", "override_transformations")}
        good, base_mask = self.fit_catalogue(observations, return_feature_array=True, **fa_kw)
        pos = np.flatnonzero(~np.asarray(base_mask))
        final_mask = table["is_outlier"].to_numpy(bool) if kw["check_out_of_distribution"] else np.asarray(base_mask)
        want = (~final_mask[pos]) & np.isfinite(cond[pos]).any(1)
        acc = np.full(len(table), np.nan)
        seed, S, quantiles = kw["seed"], int(kw["num_samples"]), kw["quantiles"]
        edges = np.flatnonzero(np.diff(np.concatenate([[False], want, [False]]).astype(np.int8)))
        runs = list(zip(edges[0::2].tolist(), edges[1::2].tolist()))
        if seed is None and len(runs) > 1:
            seed = self.posteriors._next_seed(None)
        for a, b in runs:
            s_dev, a_dev = self.posteriors.sample_conditional_catalogue(torch.as_tensor(good[a:b]), cond[pos[a:b]], num_samples=S,
                                                                        seed=seed, row_offset=a, **ckw)
            q = (_dq if S <= 8192 else _dql)(s_dev, quantiles).double().cpu().numpy()
            for i, param in enumerate(self.simple_fitted_parameter_names):
                for j, qv in enumerate(quantiles):
                    table.iloc[pos[a:b], table.columns.get_loc(f"{param}_{int(qv * 100)}")] = q[:, i, j]
            acc[pos[a:b]] = a_dev.double().cpu().numpy()
            if kw["return_samples"]:
                out[1][pos[a:b]] = s_dev.double().cpu().numpy()
        table["conditional_acceptance"] = acc
        return (table, out[1]) if kw["return_samples"] else table

    # ---- out-of-distribution check (synference_amd/ood.py) ------------------------------------------------------------------
    def _ood_base(self):
        """The fitted base side of the detectors for ``self.feature_array``: kept until the array is replaced."""
        from .ood import FittedBase
        cache = getattr(self, "_ood_cache", None)
        if cache is None or cache[0] is not self.feature_array:
            cache = (self.feature_array, FittedBase(self.feature_array, self.device))
            self._ood_cache = cache
        return cache[1]

    def _catalogue_outliers(self, rows, outlier_methods=None) -> np.ndarray:
        methods = ("knn", "lof", "kde") if outlier_methods is None else outlier_methods
        outliers = np.asarray(self.test_in_distribution_pyod(np.asarray(rows), direction="in", methods=methods,
                                                             contamination=0.01), bool)
        if outliers.any():
            logger.warning(f"{int(outliers.sum())} outlier(s) detected in the observational data.")
        return outliers

    def _ood_sides(self, X_test, direction):
        assert self.has_features, "Feature array not created. Please create the feature array first."
        if not isinstance(X_test, np.ndarray):
            raise TypeError("X_test must be a numpy array.")
        assert direction in ["in", "out"], "Direction must be either 'in' or 'out'."
        if X_test.ndim != 2 or X_test.shape[1] != self.feature_array.shape[1]:
            raise ValueError("Base distribution and observations must have same number of features")
        return (self._ood_base, X_test) if direction == "in" else (lambda: X_test, self.feature_array)

    def test_in_distribution_pyod(self, X_test: np.ndarray, methods=("knn", "lof", "kde"), contamination=0.01, direction="in",
                                  combination_method="majority"):
        """ref sbi_runner.py:3777-3831: is ``X_test`` inside the distribution of ``self.feature_array`` (``direction="in"``) or
        the feature array inside that of ``X_test`` ("out")?  pyod's knn / lof / kde restated on the device
        (``ood.detect_outliers_pyod``); the reference's default methods ("lof", "isolation_forest") include one that is not
        built, so the default here is the three that are.  Returns the combined boolean mask."""
        from .ood import _validate_pyod, detect_outliers_pyod
        _validate_pyod(methods, combination_method)
        base, obs = self._ood_sides(X_test, direction)
        return detect_outliers_pyod(base(), obs, methods=methods, contamination=contamination, combination=combination_method,
                                    return_scores=False, device=self.device)

    def test_in_distribution(self, X_test: np.ndarray, method="mahalanobis", direction="in", contamination=0.1, n_neighbors=20,
                             threshold=None, confidence=0.95, n_components=None, plot=True, feature_breakdown=False, **kwargs):
        """ref sbi_runner.py:3833-3945, a wrapper of ``ood.detect_outliers``: ``outlier_mask``, ``scores``, ``threshold_used``,
        ``method_info``.  The reference's default method, robust_mahalanobis, is not built (``ValueError`` when asked for), so
        the default here is mahalanobis; ``feature_breakdown`` is presentation and raises ``ValueError``."""
        from .ood import _validate, detect_outliers
        if feature_breakdown:
            raise ValueError("feature_breakdown is outside the accelerated path (presentation; DESIGN.md section 7)")
        _validate(method, 1, 1)
        base, obs = self._ood_sides(X_test, direction)
        return detect_outliers(base(), obs, method=method, contamination=contamination, n_neighbors=n_neighbors,
                               threshold=threshold, confidence=confidence, n_components=n_components, plot=plot,
                               device=self.device, **kwargs)

    def _fit_catalogue_missing(self, observations, columns_to_feature_names, missing_data_flag, flux_units,
                               override_transformations, params, sigma_spec, quantiles, append_to_input, return_samples, seed,
                               inner_kw):
        """fit_catalogue(missing_data_mcmc=True): the complete rows through the ordinary call (same seed, same positions
        among the complete rows: the same table entries), the flagged rows through the handler."""
        import pandas as pd
        from .missing import MissingPhotometryHandler
        from .posterior import broadcast_seed
        flags = dict(getattr(self, "feature_array_flags", None) or {})
        if flags.get("scatter_fluxes") and flags.get("empirical_noise_models"):
            raise ValueError("missing_data_mcmc on a feature array built with empirical noise models and scatter_fluxes needs "
                             "the reference's 'Mode 2' imputation, which is not built on the HIP path (DESIGN.md section 7)")
        names = list(self.feature_names)
        if flux_units is not None and flags:
            df0 = pd.DataFrame(observations) if isinstance(observations, dict) else observations
            feats, _ = self.create_features_from_observations(df0, columns_to_feature_names, flux_units, missing_data_flag,
                                                              override_transformations, ignore_missing=True)
            bands = list(flags["raw_observation_names"])
            bcols = [names.index(n) for n in bands]
            ecols = None
            if flags.get("include_errors_in_feature_array"):
                ecols = [names.index(f"unc_{b}") if f"unc_{b}" in names else names.index(flags["error_names"][i])
                         for i, b in enumerate(bands)]
        else:
            if isinstance(observations, np.ndarray):
                df0 = pd.DataFrame(observations, columns=names[: observations.shape[1]])
            elif isinstance(observations, dict):
                df0 = pd.DataFrame(observations)
            else:
                df0 = observations
            if columns_to_feature_names:
                df0 = df0.rename(columns=columns_to_feature_names)
            lacking = [c for c in names if c not in df0.columns]
            if lacking:
                raise ValueError(f"observations lack the feature columns {lacking}")
            feats = df0[names].to_numpy(dtype=np.float32)
            bands, bcols, ecols = names, list(range(len(names))), None      # every feature column is a band
        flag_nan = isinstance(missing_data_flag, float) and np.isnan(missing_data_flag)
        flagged = np.isnan(feats) if flag_nan else (feats == np.float32(missing_data_flag))
        N, B = len(feats), len(bcols)
        miss = flagged[:, bcols]
        if ecols is not None:
            miss = miss | flagged[:, ecols]                                     # value or error flagged: the band is missing
        has_missing = flagged.any(1)
        full = feats.copy()
        full[flagged] = np.nan
        complete = np.where(has_missing[:, None], np.nan, full).astype(np.float32)
        out = self.fit_catalogue(complete, columns_to_feature_names=None, append_to_input=False,
                                 return_samples=return_samples, **inner_kw)
        qt = out[0] if return_samples else out
        table = df0.copy() if append_to_input else pd.DataFrame({"ID": np.arange(N) + 1})
        for c in qt.columns:
            if c != "ID" and c not in names:
                table[c] = qt[c].to_numpy()
        if "is_outlier" in table.columns:       # rows with missing bands are not checked: NaN rows in the inner call
            table["is_outlier"] = table["is_outlier"].to_numpy(dtype=bool) & ~has_missing
        self.missing_handler = None
        if has_missing.any():
            logger.info(f"{int(has_missing.sum())} rows with missing data found. Marginalizing over missing data.")
            rows = np.where(has_missing)[0]
            if ecols is not None:
                sigma = full[np.ix_(rows, ecols)]
            elif sigma_spec is not None:
                sg = np.asarray(sigma_spec, dtype=np.float32)
                sigma = sg[rows] if sg.ndim == 2 else np.broadcast_to(sg, (len(rows), B))
            else:
                raise ValueError("missing_data_mcmc needs an uncertainty for the neighbour search: the model has no error "
                                 "features (include_errors_in_feature_array), so give missing_data_sigma (scalar, [B] or (N, B))")
            handler = MissingPhotometryHandler.init_from_synference(self, run_params=params)
            self.missing_handler = handler
            seed_h = None if seed is None else (int(seed) + 0x9E3779B97F4A7C15) & (2 ** 63 - 1)
            if seed_h is None:
                seed_h = self.posteriors._next_seed(None)
            seed_h = broadcast_seed(seed_h)                                       # every rank processes all flagged rows
            res = handler.process_catalogue(full[rows], sigma, miss[rows], seed=seed_h, quantiles=quantiles,
                                            return_draws=return_samples)
            # a flag outside the bands (an extra feature, the normalisation column) cannot be imputed: the row fails
            other = np.ones(feats.shape[1], bool)
            other[bcols] = False
            if ecols is not None:
                other[ecols] = False
            ok = res["success"] & ~flagged[rows][:, other].any(1)
            q = np.where(ok[:, None, None], res["quantiles"], np.nan)
            for i, param in enumerate(self.simple_fitted_parameter_names):
                for j, qv in enumerate(quantiles):
                    col = table[f"{param}_{int(qv * 100)}"].to_numpy(dtype=np.float64).copy()
                    col[rows] = q[:, i, j]
                    table[f"{param}_{int(qv * 100)}"] = col
            table["has_missing_data"] = has_missing
            recon = np.full((N, B), np.nan)
            recon[rows] = np.where(ok[:, None] & miss[rows], res["reconstructed_photometry"], np.nan)
            for b, name in enumerate(bands):
                if not np.all(np.isnan(recon[:, b])):
                    table[f"predicted_{name}"] = recon[:, b]
            self.last_missing_result = res
        return (table, out[1]) if return_samples else table

    def evaluate_model(self, posteriors=None, X_test=None, y_test=None, num_samples: int = 1000,
                       independent_metrics: bool = True, seed: Optional[int] = None, samples=None,
                       verbose: bool = False, tarp: bool = False, latent: bool = False, **unknown) -> dict:
        """The reference's evaluate_model for flow posteriors (sbi_runner.py:6484-6735), same keys and arithmetic:
        ``MSE``, ``RMSE``, ``mean_ae``, ``median_ae``, ``R_squared`` (total sum of squares about the GLOBAL mean of
        y_test, as there), ``RMSE_norm`` / ``mean_ae_norm`` (divided by the global std), ``log_dpit_max``
        (-0.5 log max |PIT - uniform|, 6613-6616) and ``mean_log_prob``; per parameter with ``independent_metrics``, else
        pooled.  ``tarp=True`` adds the reference's ``tarp`` key (6618-6637), a one-element list holding ``calculate_TARP``
        of the same draws (the reference computes it on every call through the third-party ``tarp`` package; here it is
        opt-in and runs on the device, ``sf_tarp_coverage``).  ``latent=True`` adds ``latent_radial_ks`` and ``latent_ks_max``
        from ``calculate_latent_residuals`` of the test pairs: the members' ``radial_ks`` averaged with the ensemble weights,
        and the largest per-dimension ``ks`` of any member (both 0 for a calibrated posterior; they draw nothing, so the
        other keys do not move).  The draws stay on the device: means, medians, PIT ranks and the TARP counts are reduced
        there and only (N, D) summaries cross PCIe."""
        _warn_unknown("evaluate_model", unknown)
        posteriors = posteriors if posteriors is not None else self.posteriors
        X_test = self._X_test if X_test is None else X_test
        y_test = self._y_test if y_test is None else y_test
        if isinstance(samples, str):
            samples = np.load(samples)
        if samples is not None:
            if samples.shape[1] != num_samples:
                raise ValueError(f"Samples must have {num_samples} samples per test sample, but got {samples.shape[1]}.")
            sd = torch.as_tensor(np.asarray(samples, dtype=np.float32)).to(self.device)
        else:
            sd = posteriors.sample_catalogue(torch.as_tensor(np.asarray(X_test, dtype=np.float32)), num_samples, seed)
        mean_pred = torch.nanmean(sd, dim=1).double().cpu().numpy()
        from .posterior import device_quantiles as _dq
        median_pred = _dq(sd, (0.5,)).double().cpu().numpy()[:, :, 0]       # numpy's rule (sf_quantiles), NaN-aware
        y = np.asarray(y_test, dtype=np.float64)
        axis = 0 if independent_metrics else None
        ss_res = np.sum((y - mean_pred) ** 2, axis=axis)
        ss_tot = np.sum((y - np.mean(y)) ** 2, axis=axis)
        pit = self.calculate_PIT(X_test, y, samples=sd, posteriors=posteriors)
        dpit_max = np.max(np.abs(pit - np.linspace(0, 1, len(pit))))
        metrics = {"MSE": np.mean((y - mean_pred) ** 2, axis=axis),
                   "RMSE": np.sqrt(np.mean((y - mean_pred) ** 2, axis=axis)),
                   "mean_ae": np.mean(np.abs(y - mean_pred), axis=axis),
                   "median_ae": np.median(np.abs(y - median_pred), axis=axis),
                   "R_squared": 1 - (ss_res / ss_tot),
                   "RMSE_norm": np.sqrt(np.mean((y - mean_pred) ** 2, axis=axis)) / np.std(y),
                   "mean_ae_norm": np.mean(np.abs(y - mean_pred), axis=axis) / np.std(y),
                   "log_dpit_max": float(-0.5 * np.log(dpit_max))}
        if tarp:
            metrics["tarp"] = np.array([self._tarp_value(sd, y, posteriors=posteriors, seed=seed)])
        try:
            metrics["mean_log_prob"] = float(np.mean(self.log_prob(X_test, y_test, posteriors=posteriors)))
        except Exception:
            pass
        if latent:
            res = self.calculate_latent_residuals(X_test, y_test, posteriors=posteriors)
            metrics["latent_radial_ks"] = float(np.dot(res["weights"], [m["radial_ks"] for m in res["members"]]))
            metrics["latent_ks_max"] = float(max(np.max(m["ks"]) for m in res["members"]))
        metrics = {k: (v.tolist() if isinstance(v, np.ndarray) else float(v)) for k, v in metrics.items()}
        if verbose:
            for k, v in metrics.items():
                logger.info(f"{k}: {v}")
        self.last_metrics = metrics
        return metrics

    def _tarp_value(self, sd: torch.Tensor, y, posteriors=None, num_bootstrap: int = 200, seed: Optional[int] = None,
                    norm_axis: int = 0) -> float:
        """| mean over the bootstrap passes of ecp[:, (n + 1) // 2] - 0.5 | of (N,S,D) device draws."""
        from .features import tarp_coverage
        if seed is None and hasattr(posteriors, "_next_seed"):
            seed = posteriors._next_seed(None)
        y2 = np.asarray(y, dtype=np.float32).reshape(sd.shape[0], -1)
        ecp, _ = tarp_coverage(sd, y2, norm=True, bootstrap=True, num_bootstrap=num_bootstrap, seed=seed,
                               norm_axis=norm_axis)
        return float(abs(np.mean(ecp[:, ecp.shape[1] // 2]) - 0.5))

    def calculate_TARP(self, X: np.ndarray, y: np.ndarray, num_samples: int = 1000, posteriors=None,
                       num_bootstrap: int = 200, samples=None, seed: Optional[int] = None,
                       norm_axis: int = 0) -> torch.Tensor:
        """Tests of Accuracy with Random Points (ref: sbi_runner.py:7090-7126): ``|mean_b ecp[b, mid] - 0.5|`` of
        ``get_tarp_coverage(samples, y, norm=True, bootstrap=True, num_bootstrap=num_bootstrap)``, as a 0-dim float64
        tensor on ``self.device``; 0 for a calibrated posterior.  The coverage test is a restatement of the published
        algorithm that runs on the device (``features.tarp_coverage``), not the ``tarp`` package.  ``samples``, when given,
        is in the reference's (S, N, D) order.  When it is not, the draws come from ``posteriors.sample_catalogue`` and
        stay on the device in (N, S, D) order; the reference passes ``sample_posterior``'s (N, S, D) array on that
        branch without the transpose the package needs (6618-6620 do it for evaluate_model only), so its value there is
        computed over the wrong axes -- here both branches test the same thing.  ``seed`` (row resampling and reference
        points; None: the posterior's next seed, as ``sample_catalogue`` takes it) and ``norm_axis`` (see
        ``features.tarp_coverage``) are additions."""
        posteriors = posteriors if posteriors is not None else self.posteriors
        if isinstance(samples, str):
            samples = np.load(samples)
        if samples is None:
            sd = posteriors.sample_catalogue(torch.as_tensor(np.asarray(X, dtype=np.float32)), num_samples, None)
        elif isinstance(samples, torch.Tensor):
            sd = samples.to(self.device).float().permute(1, 0, 2).contiguous()
        else:
            sd = torch.as_tensor(np.ascontiguousarray(np.asarray(samples, dtype=np.float32).transpose(1, 0, 2))).to(self.device)
        val = self._tarp_value(sd, y, posteriors=posteriors, num_bootstrap=num_bootstrap, seed=seed, norm_axis=norm_axis)
        return torch.tensor(val, dtype=torch.float64, device=self.device)

    def calculate_latent_residuals(self, X=None, y=None, posteriors=None, num_bins: int = 100, return_latents: bool = False):
        """Calibration read in the base space of the flows (the numbers behind the reference's empty ``plot_latent_residual``,
        sbi_runner.py:7200): every ensemble member maps the test pairs to its latents ``z_i = T(y_i; X_i)``, which are
        N(0, I) for a calibrated posterior, and ``features.latent_summary`` reduces them on the device -- moments, the
        per-dimension PIT histograms of Phi(z_d) and the histogram of F_chi2_D(|z_i|^2), whose cumulative curve is the expected
        coverage of the joint posterior.  One density-direction pass per pair and member: no draws, where ``calculate_TARP``
        and ``calculate_PIT`` need ``num_samples`` of them per pair.  ``X`` / ``y`` default to the stored test split.  Returns
        ``{"members": [summary, ...], "weights": [...]}`` (a mixture has no latent space of its own: one summary per member);
        with ``return_latents`` also the list of the members' float64 (N, D) host arrays.  Under a process group every rank
        computes the whole thing.  The test is on the flow's own density q: where the prior box truncates q (leakage) the
        posterior is q renormalised inside the box and the latents of in-box truths are not exactly N(0, I) -- quote
        ``acceptance_rows`` next to the result."""
        from .features import latent_summary
        posteriors = posteriors if posteriors is not None else self.posteriors
        X = self._X_test if X is None else X
        y = self._y_test if y is None else y
        Xt = torch.as_tensor(np.asarray(X, dtype=np.float32))
        yt = torch.as_tensor(np.asarray(y, dtype=np.float32))
        if Xt.dim() == 2:
            yt = yt.reshape(len(Xt), -1)
        if hasattr(posteriors, "posteriors"):
            pairs = posteriors.to_noise_catalogue(yt, Xt)
            weights = [float(w) for w in posteriors.weights]
        else:
            pairs = [posteriors.to_noise_catalogue(yt, Xt)]
            weights = [1.0]
        out = {"members": [latent_summary(z, num_bins) for z, _ in pairs], "weights": weights}
        if return_latents:
            from .hostio import to_host_f64
            return out, [to_host_f64(z) for z, _ in pairs]
        return out

    def calculate_PIT(self, X: np.ndarray, y: np.ndarray, num_samples: int = 1000, posteriors=None,
                      samples=None, seed: Optional[int] = None) -> np.ndarray:
        """Sorted, max-normalised probability integral transform values, one per row
        (ref: sbi_runner.py:7128-7160: ``mean(samples[i] < y[i])`` over draws and parameters).  The draws are
        ranked on the device (``sf_pit_ranks``)."""
        from .features import pit_ranks
        posteriors = posteriors if posteriors is not None else self.posteriors
        if samples is None:
            sd = posteriors.sample_catalogue(torch.as_tensor(np.asarray(X, dtype=np.float32)), num_samples, seed)
        elif isinstance(samples, torch.Tensor):
            sd = samples.to(self.device).float()
        else:
            sd = torch.as_tensor(np.asarray(samples, dtype=np.float32)).to(self.device)
        y2 = np.asarray(y, dtype=np.float32).reshape(sd.shape[0], -1)
        n_valid = torch.isfinite(sd).sum(1).double().cpu().numpy()
        ranks = pit_ranks(sd, torch.as_tensor(y2)).double().cpu().numpy()
        # reference semantics: NaN draws compare False but stay in the denominator
        pit = np.nan_to_num(ranks * n_valid, nan=0.0).sum(1) / (sd.shape[1] * sd.shape[2])
        pit = np.sort(pit)
        return pit / pit[-1]

    def lc2st(self, x_obs, posterior=None, X_test=None, y_test=None, *, num_posterior_samples: int = 10000,
              num_trials_null: int = 100, alpha: float = 0.05, seed: Optional[int] = None, **lc2st_kwargs) -> dict:
        """The L-C2ST local calibration test at ``x_obs`` (ref: sbi_runner.py:986-1063; Linhart et al. 2023): is the posterior
        calibrated at THIS observation?  ``X_test`` / ``y_test`` are the calibration pairs (default: the training split, as in
        the reference).  One posterior draw per calibration row comes from ``posterior.sample_catalogue(X, 1)``, the
        ``num_posterior_samples`` draws at ``x_obs`` stay on the device, and 1 + ``num_trials_null`` classifiers train in one
        launch sequence (``lc2st.LC2ST``).  The reference plots and returns nothing; this returns, and
        keeps as ``self.last_lc2st``, ``p_value``, ``reject`` (p_value < alpha), ``statistic``, ``null_statistics`` (T,),
        ``probs_data`` (S,), ``probs_null`` (T, S) and ``n_iter`` (T + 1,).  ``x_obs`` may be (C,), (1, C) or (M, C); with M
        rows every entry gains a leading M axis.  ``seed`` (None: the posterior's next seed) keys the draws and the
        classifiers; under a process group every rank runs the whole test on rank 0's seed.  ``lc2st_kwargs`` go to
        ``LC2ST`` (``hidden_width``, ``max_iter``, ``n_iter_no_change``, ``timeout_seconds``, ...)."""
        from .lc2st import LC2ST
        from .posterior import broadcast_seed
        if X_test is None:
            if self._X_train is None:
                raise ValueError("No training data found. Please set the training data first.")
            X_test = self._X_train
        if y_test is None:
            if self._y_train is None:
                raise ValueError("No training labels found. Please set the training labels first.")
            y_test = self._y_train
        if posterior is None:
            if self.posteriors is None:
                raise ValueError("No posterior found. Please set the posterior first.")
            posterior = self.posteriors
        if seed is None:
            seed = posterior._next_seed(None)
        seed = int(broadcast_seed(seed))
        X = torch.as_tensor(np.asarray(X_test, dtype=np.float32))
        y = torch.as_tensor(np.asarray(y_test, dtype=np.float32)).reshape(X.shape[0], -1)
        cal = posterior.sample_catalogue(X, 1, seed)[:, 0, :]                   # (N, D) on the device, no per-row loop
        ok = torch.isfinite(cal).all(1)
        if not bool(ok.all()):
            logger.warning("lc2st: %d calibration rows without a posterior draw are left out", int((~ok).sum()))
            keep = ok.cpu()
            X, y, cal = X[keep], y[keep], cal[ok]
        test = LC2ST(y, X, cal, seed=seed, num_trials_null=num_trials_null, device=cal.device, **lc2st_kwargs)
        test.train_all()
        xo = torch.as_tensor(np.asarray(x_obs, dtype=np.float32))
        xo = xo[None, :] if xo.dim() == 1 else xo
        n_iter = test.training_state()["n_iter"]
        rows = []
        for m in range(xo.shape[0]):
            draws = posterior.sample_catalogue(xo[m:m + 1], int(num_posterior_samples), (seed + 1) & (2 ** 63 - 1))[0]
            draws = draws[torch.isfinite(draws).all(1)]
            probs_data, stat = test.get_scores(draws, xo[m], return_probs=True, trained_clfs=test.trained_clfs)
            probs_null, null = test.get_statistics_under_null_hypothesis(draws, xo[m], return_probs=True)
            p = float((stat.mean() < null).mean())
            rows.append({"p_value": p, "reject": bool(p < alpha), "statistic": float(stat.mean()), "null_statistics": null,
                         "probs_data": probs_data[0], "probs_null": probs_null, "n_iter": n_iter})
        out = rows[0] if len(rows) == 1 else {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}
        self.last_lc2st = out
        return out

    def detect_misspecification(self, x_obs, X_train=None, retrain=False, *, method: str = "logprob", alpha: float = 0.05,
                                seed: Optional[int] = None, plot: bool = False, **kwargs) -> dict:
        """Is the library misspecified for the observations (ref: sbi_runner.py:905-984; Schmitt et al. 2023)?
        ``method="logprob"`` is the reference's path: an unconditional flow of the training features
        (``misspecification.MarginalTrainer``, kept as ``self.marginal_trainer`` / ``self.marginal_trainer_est``) and where
        ``log p(x_obs)`` falls among ``log p(X_train)``; ``retrain=False`` reuses a kept flow (the reference tests a misspelt
        attribute and so always retrains), ``kwargs`` go to ``MarginalTrainer.train``.  ``method="mmd"`` is the catalogue-level
        permutation test of ``misspecification.calc_misspecification_mmd``: ``mode=``, ``n_shuffle=`` and its other keywords
        come from ``kwargs``, ``self.posteriors`` serves ``mode="embedding"``.  ``X_train`` defaults to the training split.
        The reference plots and returns nothing; this returns, and keeps as ``self.last_misspecification``,
        ``{"method", "p_value", "reject", "log_prob_obs", "log_prob_train"}`` or ``{"method", "p_value", "reject", "mmd",
        "mmds_baseline", "mmd2", "null_mmd2", "scale"}``.  ``seed`` None: the posterior's next seed (0 without one); under a
        process group every rank runs the whole test on rank 0's seed."""
        from . import misspecification as MS
        from .posterior import broadcast_seed
        if method not in MS.METHODS:
            raise ValueError(f"Unknown method: {method}; available: {list(MS.METHODS)}")
        if X_train is None:
            if self._X_train is None:
                raise ValueError("No training data found. Please set the training data first.")
            X_train = self._X_train
        if plot:
            logger.info("detect_misspecification: plot=True is skipped on the HIP path (plotting is out of scope)")
        post = getattr(self, "posteriors", None)
        if seed is None:
            seed = post._next_seed(None) if post is not None and hasattr(post, "_next_seed") else 0
        seed = int(broadcast_seed(int(seed)))
        if method == "mmd":
            kw = dict(kwargs)
            mode, n_shuffle = kw.pop("mode", "x_space"), kw.pop("n_shuffle", 1000)
            out = MS.calc_misspecification_mmd(post, x_obs, X_train, mode, n_shuffle, seed=seed, alpha=alpha, return_details=True,
                                               **kw)
            out = {"method": "mmd", **out}
        else:
            X = np.asarray(X_train, dtype=np.float32)
            MS._check_features(X.shape[1] if X.ndim == 2 else 0)
            if retrain or getattr(self, "marginal_trainer_est", None) is None:
                self.marginal_trainer = MS.MarginalTrainer(density_estimator="NSF")
                self.marginal_trainer.append_samples(X)
                self.marginal_trainer_est = self.marginal_trainer.train(seed=seed, **kwargs)
            est = self.marginal_trainer_est
            p_value, reject = MS.calc_misspecification_logprob(X, x_obs, est, alpha=alpha)
            xo = np.asarray(x_obs, dtype=np.float32)
            lp_o = est.log_prob(xo).double().cpu().numpy()
            out = {"method": "logprob", "p_value": p_value, "reject": reject,
                   "log_prob_obs": float(lp_o[0]) if xo.ndim == 1 else lp_o, "log_prob_train": est.log_prob(X).double().cpu().numpy()}
        self.last_misspecification = out
        return out
