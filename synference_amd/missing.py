"""SBI++ marginalisation over missing bands on the device (ref: sbi_runner.py:7676-8004, ``MissingPhotometryHandler``).

For an observed row with missing bands: the training rows nearest in the observed bands, one weighted Gaussian KDE per
missing band, ``nmc`` completed photometry vectors drawn from them (``sf_impute_missing``, csrc/sf_impute.hip), ``nposterior``
posterior draws for each (the batched sampler), the ``nmc * nposterior`` draws pooled and reduced to quantiles on the device
(``sf_quantiles_large``).  ``process_catalogue`` does this for a whole list of rows; the reference's per-object methods are
built on it.

Deviations from the reference, all deliberate:

* the caller's ``run_params`` are honoured (the reference's ``init_from_synference(self, run_params=...)`` swallows them in
  ``**run_params``), and ``ini_chi`` -- the key ``fit_catalogue``'s default dictionary spells -- is an alias of ``ini_chi2``;
* random streams: Philox stream 5 keyed by (seed, the row's position in the catalogue, imputation, band) plus the
  sampler's own streams, not numpy's global generator: a catalogue is reproducible and independent of the chunking;
* the error feature of an imputed band is the drawn neighbour's own error value (the reference leaves it NaN without
  empirical noise models, which would condition the flow on NaN);
* ``sigma`` may come from ``missing_data_sigma`` when errors are not features (the reference has no value there);
* ``tmax_all`` (minutes) is a wall-clock ceiling over the whole stage, checked between object chunks; objects not reached are
  failures with ``timeout=True``;
* draws are float32;
* Mode 2 (empirical noise models re-applied to the imputed flux) is not built: it raises.

Kept as written: nansum / dof, the threshold ladder with its quirk (an empty set falls back to the 100 nearest rows, a set of
1-29 rows fails), independent KDEs per band, the reconstructed photometry as the mean of the imputations.
"""
from __future__ import annotations

import ctypes as C
import logging
import time
from typing import Any, Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _ptr

logger = logging.getLogger("synference_amd")

_DEFAULTS = {"ini_chi2": 5.0, "max_chi2": 50.0, "nmc": 100, "nposterior": 1000, "tmax_all": 10, "verbose": False}
# (not in the reference's dictionary, where they are literals: sbi_runner.py:7753-7760, 7778)
_EXTRA = {"chi2_step": 5.0, "min_neighbours": 30, "fallback_k": 100, "bw": 0.2}


class MissingPhotometryHandler:
    def __init__(self, training_photometry, posterior_estimator=None, run_params: Optional[Dict[str, Any]] = None,
                 photometry_units: Optional[str] = "AB", uncertainty_models=None, band_names=None, feature_names=None,
                 device: str = "cuda", band_columns=None, error_columns=None, default_sigma=None,
                 draw_budget_bytes: int = 1 << 30):
        """``training_photometry``: (NT, B) complete photometry, every column a band (the reference's argument) -- or, with
        ``band_columns`` (and optionally ``error_columns``, one per band), the whole (NT, F) training feature array, of which
        those columns are the bands.  ``posterior_estimator``: a posterior with ``sample_catalogue`` (FlowPosterior /
        EnsemblePosterior) or a fitter that holds one in ``.posteriors``.  ``default_sigma``: the uncertainty used in chi2
        when an observation brings none (scalar or [B]).  ``draw_budget_bytes``: ceiling of the pooled draw buffer of one
        chunk of objects (nmc * nposterior * D floats each: 2 MB at the defaults and D = 5)."""
        if uncertainty_models:
            raise ValueError("empirical noise models on imputed bands (the reference's 'Mode 2') are not built on the HIP path")
        self.y_train = np.ascontiguousarray(np.asarray(training_photometry, dtype=np.float32))
        if self.y_train.ndim != 2:
            raise ValueError("training_photometry must be (NT, F)")
        F = self.y_train.shape[1]
        self.band_columns = np.arange(F, dtype=np.int32) if band_columns is None else np.asarray(band_columns, dtype=np.int32)
        self.error_columns = None if error_columns is None else np.asarray(error_columns, dtype=np.int32)
        if self.error_columns is not None and len(self.error_columns) != len(self.band_columns):
            raise ValueError("error_columns must hold one column per band")
        self.posterior_estimator = posterior_estimator
        self.device = device
        self.uncertainty_models = None
        self.band_names = list(band_names) if band_names is not None else None
        self.photometry_units = photometry_units
        self.feature_names = list(feature_names) if feature_names is not None else None
        self.default_sigma = default_sigma
        self.draw_budget_bytes = int(draw_budget_bytes)
        self.run_params: Dict[str, Any] = dict(_DEFAULTS)
        self.run_params.update(_EXTRA)
        rp = dict(run_params or {})
        if "ini_chi" in rp:                     # fit_catalogue's default dictionary in the reference spells it so
            rp.setdefault("ini_chi2", rp.pop("ini_chi"))
            rp.pop("ini_chi", None)
        unknown = set(rp) - set(self.run_params)
        if unknown:
            raise ValueError(f"unknown run_params {sorted(unknown)}; known: {sorted(self.run_params)}")
        self.run_params.update(rp)
        self._train_dev = None
        self.last_posterior_samples, self.last_imputed, self.last_chunk_rows = None, None, None

    @classmethod
    def init_from_synference(cls, synference, run_params: Optional[Dict[str, Any]] = None, **kwargs):
        """From a fitter that holds its training feature array (ref: sbi_runner.py:7963-8004).  With ``feature_array_flags`` the
        bands are ``raw_observation_names`` and, when errors are features, their ``unc_`` columns; without, every feature
        column is a band."""
        flags = getattr(synference, "feature_array_flags", None) or {}
        if flags.get("scatter_fluxes") and flags.get("empirical_noise_models"):
            raise ValueError("a feature array built with empirical noise models and scatter_fluxes needs the reference's "
                             "'Mode 2' imputation, which is not built on the HIP path (DESIGN.md section 7)")
        fa = getattr(synference, "feature_array", None)
        if fa is None:
            raise ValueError("the fitter holds no training feature array to search for neighbours")
        names = list(synference.feature_names)
        if flags.get("raw_observation_names"):
            bands = list(flags["raw_observation_names"])
            bcols = [names.index(n) for n in bands]
            ecols = None
            if flags.get("include_errors_in_feature_array"):
                enames = list(flags["error_names"])
                ecols = [names.index(f"unc_{b}") if f"unc_{b}" in names else names.index(enames[i]) for i, b in enumerate(bands)]
        else:
            bands, bcols, ecols = names, list(range(len(names))), None
        return cls(np.asarray(fa, dtype=np.float32), synference, run_params=run_params,
                   photometry_units=flags.get("normed_flux_units", "AB"), band_names=bands, feature_names=names,
                   device=str(getattr(synference, "device", "cuda")), band_columns=bcols, error_columns=ecols, **kwargs)

    # ---- plumbing -----------------------------------------------------------------------------------------------------------
    def _posterior(self):
        p = self.posterior_estimator
        if p is not None and not hasattr(p, "sample_catalogue") and hasattr(p, "posteriors"):
            p = p.posteriors
        if p is None or not hasattr(p, "sample_catalogue"):
            raise ValueError("the handler needs a posterior with sample_catalogue (or a fitter that holds one)")
        return p

    def _dev(self):
        if not torch.cuda.is_available():
            raise RuntimeError("missing-band imputation runs on the GPU (sf_impute_missing); there is no CPU fallback")
        dev = torch.device(self.device if str(self.device).startswith("cuda") else "cuda")
        if self._train_dev is None or self._train_dev.device != dev:
            self._train_dev = torch.as_tensor(self.y_train, device=dev).contiguous()
        return dev

    def impute(self, feature_rows, sigma, missing_mask, seed: int, row_offset: int = 0, diagnostics: bool = False):
        """The imputation stage alone: (M, F) rows, (M, B) sigma, (M, B) mask -> dict of device tensors ``imputed``
        (M, nmc, F), ``recon`` (M, B), ``n_used`` (M,) (negative: failure) and, with ``diagnostics``, ``thr``, ``kde_var``,
        ``draw_idx``."""
        dev = self._dev()
        rp = self.run_params
        B, F, nmc = len(self.band_columns), self.y_train.shape[1], int(rp["nmc"])
        rows = torch.as_tensor(feature_rows, dtype=torch.float32, device=dev).contiguous()
        sig = torch.as_tensor(sigma, dtype=torch.float32, device=dev).contiguous()
        miss = torch.as_tensor(np.asarray(missing_mask, dtype=np.uint8) if not torch.is_tensor(missing_mask) else missing_mask,
                               device=dev).to(torch.uint8).contiguous()
        M = rows.shape[0]
        if rows.shape != (M, F) or sig.shape != (M, B) or miss.shape != (M, B):
            raise ValueError(f"need feature rows (M, {F}), sigma (M, {B}) and a mask (M, {B})")
        out = {"imputed": torch.empty((M, nmc, F), dtype=torch.float32, device=dev),
               "recon": torch.empty((M, B), dtype=torch.float32, device=dev),
               "n_used": torch.empty((M,), dtype=torch.int32, device=dev)}
        if diagnostics:
            out["thr"] = torch.empty((M,), dtype=torch.float32, device=dev)
            out["kde_var"] = torch.empty((M, B), dtype=torch.float64, device=dev)
            out["draw_idx"] = torch.empty((M, nmc, B), dtype=torch.int32, device=dev)
        bc = (C.c_int32 * B)(*[int(c) for c in self.band_columns])
        ec = None if self.error_columns is None else (C.c_int32 * B)(*[int(c) for c in self.error_columns])
        st = _lib.stream_ptr(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().sf_impute_missing(
                _ptr(self._train_dev), self.y_train.shape[0], F, bc, ec, B, _ptr(rows), _ptr(sig), _ptr(miss), M, int(row_offset),
                float(rp["ini_chi2"]), float(rp["chi2_step"]), float(rp["max_chi2"]), int(rp["min_neighbours"]),
                int(rp["fallback_k"]), float(rp["bw"]), nmc, C.c_uint64(int(seed) & (2 ** 64 - 1)), _ptr(out["imputed"]),
                _ptr(out["recon"]), _ptr(out["n_used"]), _ptr(out.get("thr")), _ptr(out.get("kde_var")), None, 0,
                _ptr(out.get("draw_idx")), st))
        return out

    # ---- the batched call ---------------------------------------------------------------------------------------------------
    def process_catalogue(self, feature_rows, sigma, missing_mask, seed: Optional[int] = None, quantiles=(0.16, 0.5, 0.84),
                          row_offset: int = 0, return_draws: bool = False) -> Dict[str, Any]:
        """Every row of ``feature_rows`` (M, F) with the bands of ``missing_mask`` (M, B) imputed ``nmc`` times and
        ``nposterior`` posterior draws for each.  Returns ``quantiles`` (M, D, Q), ``reconstructed_photometry`` (M, B; NaN
        for observed bands), ``success``, ``timeout`` (M,) bool, ``count`` (imputations made) and ``n_neighbours`` (M,) --
        numpy -- and with ``return_draws`` ``posterior_samples``: the pooled (m, nmc * nposterior, D) DEVICE draws of the
        last chunk of objects (rows ``last_chunk_rows``).  ``row_offset``: the rows are [row_offset, ...) of a larger list;
        with the same seed they draw what a single call over the whole list would."""
        from .posterior import device_quantiles_large
        post = self._posterior()
        dev = self._dev()
        rp = self.run_params
        nmc, S = int(rp["nmc"]), int(rp["nposterior"])
        rows = torch.as_tensor(feature_rows, dtype=torch.float32, device=dev)
        rows = rows[None, :] if rows.dim() == 1 else rows
        M, F = rows.shape
        B = len(self.band_columns)
        sig = torch.as_tensor(sigma, dtype=torch.float32, device=dev).reshape(M, B)
        miss = torch.as_tensor(np.asarray(missing_mask).astype(np.uint8), device=dev).reshape(M, B)
        if seed is None:
            seed = post._next_seed(None)
        seed = int(seed)
        D = getattr(post, "posteriors", [post])[0].spec.D
        q = np.full((M, D, len(quantiles)), np.nan)
        recon = np.full((M, B), np.nan, dtype=np.float32)
        success, timeout = np.zeros(M, bool), np.zeros(M, bool)
        count, n_nb = np.zeros(M, np.int64), np.zeros(M, np.int64)
        t0 = time.monotonic()
        limit = None if not rp.get("tmax_all") else 60.0 * float(rp["tmax_all"])
        per_obj = 4 * nmc * (S * D + F)         # the pooled draws and the imputed contexts of one object
        a = 0
        self.last_posterior_samples, self.last_imputed, self.last_chunk_rows = None, None, None
        while a < M:
            if limit is not None and time.monotonic() - t0 > limit:
                timeout[a:] = True
                logger.warning(f"missing-band marginalisation stopped after tmax_all = {rp['tmax_all']} min: "
                               f"{M - a} object(s) not reached")
                break
            b = min(M, a + max(1, self.draw_budget_bytes // per_obj))
            imp = self.impute(rows[a:b], sig[a:b], miss[a:b], seed, row_offset + a)
            ok = imp["n_used"] > 0
            ctx = imp["imputed"]
            # a failed object still occupies its nmc sampler rows (the streams are keyed by position): it is given a
            # training row as context and its draws are discarded
            ctx = torch.where(ok[:, None, None], ctx, self._train_dev[0][None, None, :].expand_as(ctx))
            left = None if limit is None else max(1.0, limit - (time.monotonic() - t0))
            draws = post.sample_catalogue(ctx.reshape((b - a) * nmc, F), S, seed, timeout_seconds=left,
                                          row_offset=(row_offset + a) * nmc)
            draws = draws.reshape(b - a, nmc * S, D)
            draws[~ok] = float("nan")
            q[a:b] = device_quantiles_large(draws, quantiles).double().cpu().numpy()
            okh = ok.cpu().numpy()
            recon[a:b] = imp["recon"].cpu().numpy()
            n_nb[a:b] = imp["n_used"].cpu().numpy()
            success[a:b] = okh
            count[a:b] = np.where(okh, nmc, 0)
            if return_draws:
                self.last_posterior_samples, self.last_imputed, self.last_chunk_rows = draws, imp["imputed"], (a, b)
            a = b
        if rp.get("verbose"):
            logger.info(f"missing bands: {int(success.sum())} of {M} objects imputed ({nmc} x {S} draws each) in "
                        f"{time.monotonic() - t0:.2f} s")
        out = {"quantiles": q, "reconstructed_photometry": recon, "success": success, "timeout": timeout, "count": count,
               "n_neighbours": n_nb}
        if return_draws:
            out["posterior_samples"] = self.last_posterior_samples
        return out

    # ---- the reference's per-object surface -----------------------------------------------------------------------------------
    def _row_of(self, obs: Dict[str, Any]):
        B, F = len(self.band_columns), self.y_train.shape[1]
        mags = np.asarray(obs["mags_sbi"], dtype=np.float32)
        miss = np.asarray(obs["missing_mask"], dtype=bool)
        unc = obs.get("mags_unc_sbi")
        row = np.full(F, np.nan, dtype=np.float32)
        row[self.band_columns] = mags
        if unc is not None and self.error_columns is not None:
            row[self.error_columns] = np.asarray(unc, dtype=np.float32)
        for name, value in (obs.get("extra") or {}).items():
            row[self.feature_names.index(name)] = value
        if unc is None:
            if self.default_sigma is None:
                raise ValueError("the observation brings no uncertainties ('mags_unc_sbi') and the handler has no default_sigma")
            unc = np.broadcast_to(np.asarray(self.default_sigma, dtype=np.float32), (B,))
        return row, np.asarray(unc, dtype=np.float32), miss

    def generate_imputations(self, obs: Dict[str, Any], true_flux_units=None, out_units=None, seed: Optional[int] = None):
        """(nmc, F) completed feature vectors of one observation and {'success', 'timeout', 'count'} (ref: 7796-7868)."""
        row, unc, miss = self._row_of(obs)
        seed = self._posterior()._next_seed(None) if seed is None else int(seed)
        imp = self.impute(row[None], unc[None], miss[None], seed)
        if int(imp["n_used"][0]) <= 0:
            return np.nan, {"success": False, "timeout": False, "count": 0}
        return imp["imputed"][0].cpu().numpy(), {"success": True, "timeout": False, "count": int(self.run_params["nmc"])}

    def sample_posterior(self, observation_vectors, seed: Optional[int] = None) -> np.ndarray:
        """(n_vectors * nposterior, D) draws for one or more complete vectors (ref: 7873-7894)."""
        x = torch.as_tensor(np.asarray(observation_vectors, dtype=np.float32))
        x = x[None, :] if x.dim() == 1 else x
        s = self._posterior().sample_catalogue(x, int(self.run_params["nposterior"]), seed)
        return s.reshape(-1, s.shape[-1]).cpu().numpy()

    def process_observation(self, obs: Dict[str, Any], true_flux_units=None, out_units=None, seed: Optional[int] = None):
        """One observation end to end (ref: 7899-7961): 'posterior_samples' (nmc * nposterior, D), 'reconstructed_photometry'
        (B; the mean of the imputations at the missing bands, the observed values elsewhere), 'imputed_vectors', 'success',
        'timeout', 'count'."""
        row, unc, miss = self._row_of(obs)
        if not miss.any():
            return {"posterior_samples": self.sample_posterior(row, seed), "success": True}
        res = self.process_catalogue(row[None], unc[None], miss[None], seed=seed, return_draws=True)
        ok = bool(res["success"][0])
        phot = np.asarray(obs["mags_sbi"], dtype=np.float32).copy()
        phot[miss] = res["reconstructed_photometry"][0][miss]
        return {"posterior_samples": res["posterior_samples"][0].cpu().numpy() if ok else np.array([]),
                "reconstructed_photometry": phot if ok else np.full_like(phot, np.nan),
                "imputed_vectors": self.last_imputed[0].cpu().numpy() if ok else np.nan, "success": ok, "timeout": bool(res["timeout"][0]), "count": int(res["count"][0])}
