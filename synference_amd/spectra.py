"""Observed-frame spectra features on the device (``sf_spectra_transform``, csrc/sf_spectra.hip).

``transform_spectrum`` and ``convolve_variable_width_gaussian`` carry the reference's names and argument order
(ref: src/synference/utils.py:185-254 and 129-182) and are batched: one workgroup per spectrum redshifts it, convolves it with
the instrument's wavelength-dependent Gaussian line-spread function and rebins it (SpectRes, fill 0) onto the observed pixels.
``spectra_features`` is the whole per-row pipeline behind ``SBI_Fitter.create_feature_array_from_raw_spectra``
(ref: sbi_runner.py:1096-1178, 1180-1427): transform, normalisation, units, clip.  Plain arrays in microns stand where the
reference takes unyt arrays.  The flux is a float32 tensor on the GPU; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import stream_ptr as _stream
from .noise_models import PHYSICAL_UNITS

MODE_UNITS, MODE_TRANSFORM, MODE_CONVOLVE = 0, 1, 2
NORM_NONE, NORM_REST, NORM_OBSERVED = 0, 1, 2
UNIT_LINEAR, UNIT_LOG10, UNIT_AB = 0, 1, 2
MAX_L, MAX_CURVE, MAX_HALF_WIDTH = 16384, 256, 65536
FWHM_PER_SIGMA = 2.0 * np.sqrt(2.0 * np.log(2.0))


def _grid(a, name, min_len=1):
    """A 1-D strictly ascending float64 wavelength grid in um (anything with ``to_value('um')`` is converted)."""
    a = a.to_value("um") if hasattr(a, "to_value") else a
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    if len(a) < min_len:
        raise ValueError(f"{name} needs at least {min_len} pixels" + (": one pixel has no bin width" if min_len == 2 else ""))
    if len(a) > 1 and not (np.diff(a) > 0).all():
        raise ValueError(f"{name} must be strictly ascending")
    return a


def _dev(a, device):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def _ptr(t):
    return None if t is None else t.data_ptr()


def unit_conversion(grid_unit: str, normed_flux_units: str):
    """(unit code, scale) of ref: sbi_runner.py:1361-1367 for a grid in ``grid_unit``: 'AB', 'log10 <unit>' or a plain unit,
    units being the strings of ``noise_models.PHYSICAL_UNITS``."""
    if grid_unit not in PHYSICAL_UNITS:
        raise ValueError(f"the spectra grid's unit {grid_unit!r} is not a physical flux unit: one of {sorted(PHYSICAL_UNITS)}")
    if not isinstance(normed_flux_units, str):
        raise ValueError("normed_flux_units must be a string")
    if normed_flux_units == "AB":
        return UNIT_AB, 1.0 / PHYSICAL_UNITS[grid_unit]
    code, unit = (UNIT_LOG10, normed_flux_units[6:]) if normed_flux_units.startswith("log10 ") else (UNIT_LINEAR, normed_flux_units)
    if unit not in PHYSICAL_UNITS:
        raise ValueError(f"normed_flux_units {normed_flux_units!r} is not supported: 'AB', or one of {sorted(PHYSICAL_UNITS)}, "
                         "plain or after 'log10 '")
    return code, PHYSICAL_UNITS[unit] / PHYSICAL_UNITS[grid_unit]


def filter_arrays(filt):
    """A bandpass filter -> (wavelength in um, transmission): an object with ``.lam`` (um, or something with
    ``to_value('um')``) and ``.transmission``, or a ``(wavelength_um, transmission)`` pair."""
    if hasattr(filt, "lam") and hasattr(filt, "transmission"):
        lam, tr = filt.lam, filt.transmission
    else:
        try:
            lam, tr = filt
        except (TypeError, ValueError):
            raise ValueError("Filter object must have 'lam' (um) and 'transmission' attributes, or be a "
                             "(wavelength_um, transmission) pair") from None
    lam = lam.to_value("um") if hasattr(lam, "to_value") else lam
    lam, tr = np.asarray(lam, np.float64).reshape(-1), np.asarray(tr, np.float64).reshape(-1)
    if len(lam) != len(tr) or len(lam) == 0:
        raise ValueError("the filter's wavelengths and transmission must have the same, non-zero length")
    return lam, tr


def norm_coefficients(wave_um, method, parameters) -> np.ndarray:
    """The normalisation factor of ref: sbi_runner.py:1119-1163 as coefficients a[.] on the grid ``wave_um``: factor =
    sum(flux * a).  'tophat': 1 / n on the n pixels inside [center - width / 2, center + width / 2]; 'bandpass':
    T dx / trapz(T) with T the transmission interpolated onto the grid (0 outside the filter) and dx the trapezoid weights.
    No overlap, or a denominator that is not positive: all zero -- the factor is 0 and the row becomes 0."""
    w = np.asarray(wave_um, np.float64)
    parameters = parameters or {}
    if callable(method):
        raise ValueError('a callable flux_norm_method is outside the HIP path: use "tophat" or "bandpass"')
    if method == "tophat":
        center, width = parameters.get("center"), parameters.get("width")
        if center is None or width is None:
            raise ValueError("'tophat' norm requires 'center' and 'width' in flux_norm_parameters")
        m = (w >= center - width / 2.0) & (w <= center + width / 2.0)
        return m / m.sum() if m.sum() > 0 else np.zeros(len(w))
    if method == "bandpass":
        if parameters.get("filter") is None:
            raise ValueError("'bandpass' norm requires a 'filter' object in flux_norm_parameters")
        lam, tr = filter_arrays(parameters["filter"])
        t = np.interp(w, lam, tr, left=0.0, right=0.0)
        dx = np.zeros(len(w))
        if len(w) > 1:
            d = np.diff(w)
            dx[:-1] += d / 2.0
            dx[1:] += d / 2.0
        den = float(np.sum(t * dx))
        return t * dx / den if den > 0 else np.zeros(len(w))
    raise ValueError(f'Unknown flux_norm_method: {method} (use "tophat" or "bandpass")')


def _half_width_limit(wave, curve_r, trunc):
    """An upper bound of ceil(trunc sigma) over every pixel and redshift: sigma in pixels is at most
    wave / (R 2 sqrt(2 ln 2) median(diff(wave))) -- the factor 1 + z cancels -- whatever the model's own resolution."""
    r_min = float(np.min(curve_r))
    if not (np.isfinite(curve_r).all() and r_min > 0):
        raise ValueError("the resolution curve must be finite and positive")
    med = float(np.median(np.diff(wave)))
    h = np.ceil(trunc * wave[-1] / (r_min * FWHM_PER_SIGMA * med)) + 1
    if not h <= MAX_HALF_WIDTH:
        raise ValueError(f"a resolving power of {r_min:g} on this grid asks for a kernel of +-{h:.0f} pixels, more than the "
                         f"{MAX_HALF_WIDTH} the kernel is bounded to: rebin the library or check the curve's units")
    return int(h)


def _check_flux(flux, who):
    if not isinstance(flux, torch.Tensor) or flux.device.type != "cuda":
        raise RuntimeError(f"{who} runs on the GPU (no CPU fallback)")


def _rows(flux):
    """(N, L) float32 with contiguous rows (the row stride may exceed L: a column block of a wider tensor is used in place)."""
    f = flux if flux.dtype == torch.float32 else flux.float()
    return f if f.stride(1) == 1 and f.stride(0) >= f.shape[1] else f.contiguous()


def spectra_features(flux: torch.Tensor, wave_um, z=None, observed_wave=None, resolution_curve_wave=None,
                     resolution_curve_r=None, theory_r=np.inf, trunc: float = 4.0, norm_frame: int = NORM_NONE,
                     norm_table: Optional[np.ndarray] = None, unit_code: int = UNIT_LINEAR, unit_scale: float = 1.0,
                     clip=(-np.inf, np.inf), columns: Optional[tuple] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One call of ``sf_spectra_transform`` over the (N, L) float32 device rows ``flux`` on the grid ``wave_um``.

    With ``z`` ((N,) redshifts): every row is redshifted, convolved and rebinned onto ``observed_wave`` (M pixels), then
    normalised (``norm_frame`` NORM_REST: ``norm_table`` [L] against the raw row; NORM_OBSERVED: [M] against the bins),
    converted (``unit_code``, ``unit_scale``: see ``unit_conversion``) and clipped.  Without ``z`` nothing is convolved or
    rebinned: the columns ``columns = (first, count)`` (default all) go through normalisation (``norm_table`` [L], the whole
    row), units and clip.  ``out``: a float32 device tensor (N, >= M) whose first M columns are written -- extra feature
    columns can sit behind them; default a new (N, M) tensor."""
    _check_flux(flux, "spectra_features")
    if flux.dim() != 2:
        raise ValueError("flux must be (N, L)")
    f = _rows(flux)
    N, L = f.shape
    dev = f.device
    wave = _grid(wave_um, "the theory wavelength grid", 2 if z is not None else 1)
    if len(wave) != L:
        raise ValueError(f"the wavelength grid has {len(wave)} pixels but the spectra have {L}")
    d = _lib.sf_spectra_desc()
    keep = [f]
    if z is not None:
        ow = _grid(observed_wave, "observed_wave", 2)
        cw, cr = _grid(resolution_curve_wave, "resolution_curve_wave"), np.asarray(resolution_curve_r, np.float64).reshape(-1)
        if len(cw) != len(cr):
            raise ValueError("resolution_curve_wave and resolution_curve_r must have the same length")
        zz = np.asarray(z, np.float64).reshape(-1)
        if len(zz) != N:
            raise ValueError(f"{len(zz)} redshifts for {N} spectra")
        tr = np.asarray(theory_r.detach().cpu().numpy() if isinstance(theory_r, torch.Tensor) else theory_r, np.float64)
        if tr.ndim > 0 and tr.size != 1 and tr.shape != (L,):
            raise ValueError(f"theory_r must be a scalar or have the {L} pixels of the theory grid")
        order = np.argsort(np.diff(wave), kind="stable")
        M = len(ow)
        d.mode, d.M, d.n_curve = MODE_TRANSFORM, M, len(cw)
        d.med_lo, d.med_hi = int(order[(L - 2) // 2]), int(order[(L - 1) // 2])
        d.h_limit, d.trunc = _half_width_limit(wave, cr, float(trunc)), float(trunc)
        tz, tw, tcw, tcr = _dev(zz, dev), _dev(ow, dev), _dev(cw, dev), _dev(cr, dev)
        keep += [tz, tw, tcw, tcr]
        d.z, d.observed_wave, d.curve_wave, d.curve_r = _ptr(tz), _ptr(tw), _ptr(tcw), _ptr(tcr)
        if tr.size == 1:
            d.theory_r = float(tr.reshape(-1)[0])
        else:
            ttr = _dev(tr, dev)
            keep.append(ttr)
            d.theory_r_arr, d.theory_r = _ptr(ttr), float("inf")
    else:
        col0, M = (0, L) if columns is None else (int(columns[0]), int(columns[1]))
        if col0 < 0 or M < 0 or col0 + M > L:
            raise ValueError("columns reach past the row")
        d.mode, d.M, d.col0, d.trunc, d.h_limit = MODE_UNITS, M, col0, 4.0, 1
    if norm_frame != NORM_NONE:
        nt = np.asarray(norm_table, np.float64).reshape(-1)
        need = M if (norm_frame == NORM_OBSERVED and z is not None) else L
        if len(nt) != need:
            raise ValueError(f"the normalisation table has {len(nt)} coefficients, not {need}")
        tn = _dev(nt, dev)
        keep.append(tn)
        d.norm_table = _ptr(tn)
    tw0 = _dev(wave, dev)
    keep.append(tw0)
    if out is None:
        out = torch.empty((N, M), dtype=torch.float32, device=dev)
    if (out.dtype != torch.float32 or out.device != dev or out.dim() != 2 or out.shape[0] != N or out.shape[1] < M
            or (N > 1 and out.stride(0) < out.shape[1]) or (out.shape[1] > 1 and out.stride(1) != 1)):
        raise ValueError("out must be a float32 tensor (N, >= M) on the flux's device with contiguous rows")
    d.flux, d.wave, d.out = _ptr(f), _ptr(tw0), _ptr(out)
    d.N, d.L, d.ld_flux, d.ld_out = N, L, (f.stride(0) if N > 1 else L), (out.stride(0) if N > 1 else max(out.shape[1], 1))
    d.norm_frame, d.unit_code, d.unit_scale = int(norm_frame), int(unit_code), float(unit_scale)
    d.clip_lo, d.clip_hi = float(clip[0]), float(clip[1])
    # (`keep` holds the small tables until the launch is queued; torch's allocator hands their memory out again in stream order)
    _lib.check(_lib.load().sf_spectra_transform(C.byref(d), _stream(dev)))
    del keep
    return out


def transform_spectrum(theory_wave, theory_flux, z, observed_wave, resolution_curve_wave, resolution_curve_r,
                       theory_r=np.inf, trunc_constant: float = 4.0):
    """ref: utils.py:185-254, batched -- ``theory_flux`` a float32 device tensor (L,) or (N, L) on ``theory_wave`` (um), ``z`` a
    scalar or (N,): redshift (the flux is not divided by 1 + z), convolution to the resolution curve (less the model's own
    ``theory_r``, scalar or (L,)), SpectRes rebinning with fill 0.  Returns ``(observed_wave, flux)`` with flux (M,) or (N, M)."""
    _check_flux(theory_flux, "transform_spectrum")
    zz = np.asarray(z.detach().cpu().numpy() if isinstance(z, torch.Tensor) else z, np.float64)
    single = theory_flux.dim() == 1 and zz.ndim == 0
    f = theory_flux.reshape(1, -1) if theory_flux.dim() == 1 else theory_flux
    if f.dim() != 2:
        raise ValueError("theory_flux must be (L,) or (N, L)")
    zz = zz.reshape(-1)
    if f.shape[0] == 1 and len(zz) > 1:
        f = f.expand(len(zz), -1).contiguous()
    if len(zz) == 1 and f.shape[0] != 1:
        zz = np.repeat(zz, f.shape[0])
    out = spectra_features(f, theory_wave, z=zz, observed_wave=observed_wave, resolution_curve_wave=resolution_curve_wave,
                           resolution_curve_r=resolution_curve_r, theory_r=theory_r, trunc=trunc_constant)
    return observed_wave, (out[0] if single else out)


def convolve_variable_width_gaussian(flux, sigma_pixels, trunc: float = 4.0):
    """ref: utils.py:129-182, batched -- ``flux`` a float32 device tensor (L,) or (N, L), ``sigma_pixels`` (L,) for every row
    or (N, L): the Gaussian sigma in pixels at each position (kept in float64).  Pixels with sigma <= 0.01 are copied."""
    _check_flux(flux, "convolve_variable_width_gaussian")
    single = flux.dim() == 1
    f = flux.reshape(1, -1) if single else flux
    if f.dim() != 2:
        raise ValueError("flux must be (L,) or (N, L)")
    f = _rows(f)
    N, L = f.shape
    sg = sigma_pixels.detach().cpu().numpy() if isinstance(sigma_pixels, torch.Tensor) else sigma_pixels
    sg = np.ascontiguousarray(np.asarray(sg, np.float64))
    if sg.shape not in ((L,), (N, L)):
        raise ValueError(f"sigma_pixels must be ({L},) or ({N}, {L}), not {sg.shape}")
    if not float(trunc) > 0:
        raise ValueError("trunc must be positive")
    h = np.ceil(float(trunc) * float(np.nanmax(sg))) + 1 if sg.size and np.isfinite(np.nanmax(sg)) else np.inf
    if not h <= MAX_HALF_WIDTH:
        raise ValueError(f"sigma_pixels asks for a kernel of +-{h:.0f} pixels, more than the {MAX_HALF_WIDTH} the kernel is bounded to")
    ts = _dev(sg, f.device)
    out = torch.empty((N, L), dtype=torch.float32, device=f.device)
    d = _lib.sf_spectra_desc()
    d.mode, d.N, d.L, d.M = MODE_CONVOLVE, N, L, 0
    d.flux, d.sigma_pixels, d.out = _ptr(f), _ptr(ts), _ptr(out)
    d.ld_flux, d.ld_out, d.sigma_stride = (f.stride(0) if N > 1 else L), L, (L if sg.ndim == 2 else 0)
    d.trunc, d.h_limit = float(trunc), int(max(h, 1))
    d.unit_code, d.unit_scale, d.clip_lo, d.clip_hi = UNIT_LINEAR, 1.0, float("-inf"), float("inf")
    _lib.check(_lib.load().sf_spectra_transform(C.byref(d), _stream(f.device)))
    return out[0] if single else out
