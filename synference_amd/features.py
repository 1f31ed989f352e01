"""Feature transform on the device.

``flux_to_abmag`` is the AB branch of the reference's feature engineering
(ref: src/synference/sbi_runner.py:1698-1716: ``-2.5 log10(f_uJy) + 23.9``, negative fluxes set to
``norm_mag_limit``; 1927-1932: magnitudes fainter than the limit clipped to it; 1699-1702: errors
``2.5 sigma / (ln 10 f)``).  ``flux_to_asinh`` is the asinh-magnitude branch (ref: src/synference/utils.py:647-704,
used at sbi_runner.py:1718-1731) and ``scatter_depths`` the depth-noise augmentation of the library
(ref: sbi_runner.py:580-691, 0-D / 1-D depths).  ``scatter_empirical`` / ``apply_scalings`` apply the empirical noise models of
``synference_amd.noise_models`` (ref: noise_models.py:507-592, 818-1099).  ``pit_ranks`` (ref: sbi_runner.py:7153-7158) and ``tarp_coverage`` (the
coverage test behind ``calculate_TARP``, ref: sbi_runner.py:7090-7126) live here too.
Normalisation to a reference band, extra feature columns and unit parsing stay host-side and out of scope.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _p, stream_ptr as _stream


def flux_to_abmag(flux_njy: torch.Tensor, err_njy: Optional[torch.Tensor] = None, norm_mag_limit: float = 50.0):
    """(N,C) fluxes in nJy on the GPU -> AB magnitudes (and magnitude errors when ``err_njy`` is given)."""
    if flux_njy.device.type != "cuda":
        raise RuntimeError("flux_to_abmag runs on the GPU (no CPU fallback)")
    def _aligned(t):  # the kernel moves float4: a contiguous view that starts off a 16-byte boundary is copied
        t = t.contiguous().float()
        return t if t.data_ptr() % 16 == 0 else t.clone()
    f = _aligned(flux_njy)
    e = None if err_njy is None else _aligned(err_njy)
    mag = torch.empty_like(f)
    mag_err = None if e is None else torch.empty_like(f)
    _lib.check(_lib.load().sf_flux_to_abmag(_p(f), _p(e), f.numel(), C.c_float(norm_mag_limit), _p(mag), _p(mag_err),
                                            _stream(f.device)))
    return mag if e is None else (mag, mag_err)


def flux_to_asinh(flux_njy: torch.Tensor, f_b_njy, err_njy: Optional[torch.Tensor] = None):
    """(N,C) fluxes in nJy on the GPU -> asinh magnitudes with softening ``f_b_njy`` (scalar or per band [C])."""
    if flux_njy.device.type != "cuda":
        raise RuntimeError("flux_to_asinh runs on the GPU (no CPU fallback)")
    f = flux_njy.contiguous().float()
    N, Cb = f.shape
    fb = torch.as_tensor(f_b_njy, dtype=torch.float32, device=f.device).reshape(-1)
    if fb.numel() == 1:
        fb = fb.expand(Cb)
    if fb.numel() != Cb:
        raise ValueError("Flux softening must match the number of filters.")
    fb = fb.contiguous()
    e = None if err_njy is None else err_njy.contiguous().float()
    mag = torch.empty_like(f)
    mag_err = None if e is None else torch.empty_like(f)
    _lib.check(_lib.load().sf_flux_to_asinh(_p(f), _p(e), N, Cb, _p(fb), _p(mag), _p(mag_err), _stream(f.device)))
    return mag if e is None else (mag, mag_err)


def scatter_depths(flux: torch.Tensor, depths, n_scatters: int = 5, depth_sigma: float = 5.0,
                   min_flux_pc_error: float = 0.0, seed: int = 0, return_errors: bool = False):
    """(N,C) library photometry -> (N*n_scatters, C) noisy copies, sigma = depths / depth_sigma per band
    (``depths`` scalar, [C], or [k, C] = k depth sets: as in the reference, one set is then drawn per band and
    scatter copy, from a generator seeded with ``seed``); row i*n_scatters + s is scatter s of row i."""
    if flux.device.type != "cuda":
        raise RuntimeError("scatter_depths runs on the GPU (no CPU fallback)")
    f = flux.contiguous().float()
    N, Cb = f.shape
    dep = torch.as_tensor(depths, dtype=torch.float32, device=f.device)
    # a device divisor: torch divides by a Python scalar as a product with its rounded reciprocal, up to 1.5 ulp off depth / depth_sigma
    ds = torch.tensor(float(depth_sigma), dtype=torch.float32, device=f.device)
    if dep.dim() == 2:  # (k, C) depth sets: depths[idx[c, s], c] per band and scatter (sbi_runner.py:636-649)
        if dep.shape[1] != Cb:
            raise ValueError(f"Mismatch in dimensions: photometry has {Cb} bands but depths has {dep.shape[1]} columns")
        g = torch.Generator().manual_seed(int(seed) & 0x7FFFFFFF)
        idx = torch.randint(0, dep.shape[0], (n_scatters, Cb), generator=g).to(f.device)
        sg = dep.gather(0, idx) / ds                                       # [n_scatters, C]
    else:
        sg = dep.reshape(-1) / ds
        if sg.numel() == 1:
            sg = sg.expand(Cb)
        if sg.numel() != Cb:
            raise ValueError(f"Mismatch in dimensions: photometry has {Cb} bands but depths has {sg.numel()} elements")
        sg = sg.reshape(1, Cb)
    sg = sg.contiguous()
    out = torch.empty((N * n_scatters, Cb), dtype=torch.float32, device=f.device)
    err = torch.empty_like(out) if return_errors else None
    _lib.check(_lib.load().sf_scatter_depths(_p(f), N, Cb, _p(sg), sg.shape[0], n_scatters, C.c_float(min_flux_pc_error),
                                             C.c_uint64(seed & (2 ** 64 - 1)), _p(out), _p(err), _stream(f.device)))
    return (out, err) if return_errors else out


def _pack_noise(models, in_units, out_units, n_cols):
    """``models``: one model per photometry column, or an already packed ``(bands, table)`` pair."""
    from .noise_models import pack_models
    if isinstance(models, tuple) and len(models) == 2 and isinstance(models[1], np.ndarray):
        bands, table = models
    else:
        bands, table = pack_models(models, in_units, out_units)
    if len(bands) != n_cols:
        raise ValueError(f"Mismatch in dimensions: photometry has {n_cols} bands but there are {len(bands)} noise models")
    return bands, np.ascontiguousarray(table, dtype=np.float32)


def scatter_empirical(flux: torch.Tensor, models, true_flux_units: Optional[str] = None, out_units: Optional[str] = None,
                      n_scatters: int = 5, seed: int = 0):
    """(N,C) library photometry in ``true_flux_units`` -> (N*n_scatters, C) noisy copies and their errors in ``out_units``,
    column c through ``models[c]`` (``sf_scatter_empirical``); row i*n_scatters + s is scatter s of row i.  Noise: Philox
    stream 6 under ``seed``, one call per output element."""
    if not isinstance(flux, torch.Tensor) or flux.device.type != "cuda":
        raise RuntimeError("scatter_empirical runs on the GPU (no CPU fallback)")
    f = flux.contiguous().float()
    N, Cb = f.shape
    bands, table = _pack_noise(models, true_flux_units, out_units, Cb)
    out = torch.empty((N * int(n_scatters), Cb), dtype=torch.float32, device=f.device)
    err = torch.empty_like(out)
    _lib.check(_lib.load().sf_scatter_empirical(_p(f), N, Cb, bands, table.ctypes.data_as(_lib.c_f32p), table.size,
                                                int(n_scatters), C.c_uint64(int(seed) & (2 ** 64 - 1)), _p(out), _p(err),
                                                _stream(f.device)))
    return out, err


def apply_scalings(flux: torch.Tensor, error: torch.Tensor, models, flux_units: Optional[str] = None,
                   out_units: Optional[str] = None):
    """(N,C) observed fluxes and errors in ``flux_units`` -> the same in ``out_units`` after each column's model has applied
    its deterministic rules: SNR cut, upper-limit flux and error, error clip (``sf_apply_scalings``)."""
    if not isinstance(flux, torch.Tensor) or flux.device.type != "cuda":
        raise RuntimeError("apply_scalings runs on the GPU (no CPU fallback)")
    f = flux.contiguous().float()
    e = error.to(f.device).contiguous().float()
    if e.shape != f.shape:
        raise ValueError("flux and error must have the same shape")
    N, Cb = f.shape
    bands, table = _pack_noise(models, flux_units, out_units, Cb)
    out, err = torch.empty_like(f), torch.empty_like(f)
    _lib.check(_lib.load().sf_apply_scalings(_p(f), _p(e), N, Cb, bands, table.ctypes.data_as(_lib.c_f32p), table.size,
                                             _p(out), _p(err), _stream(f.device)))
    return out, err


def pit_ranks(samples: torch.Tensor, truth: torch.Tensor) -> torch.Tensor:
    """(N,S,D) draws and (N,D) truths on the GPU -> (N,D) #{draws < truth} / #{non-NaN draws}: NaN draws are ignored (none left ->
    NaN), +-inf draws are ordered values and count in numerator and denominator, a NaN truth gives 0."""
    if samples.device.type != "cuda":
        raise RuntimeError("pit_ranks runs on the GPU (no CPU fallback)")
    s = samples.contiguous().float()
    N, S, D = s.shape
    t = truth.to(s.device).contiguous().float().reshape(N, D)
    out = torch.empty((N, D), dtype=torch.float32, device=s.device)
    _lib.check(_lib.load().sf_pit_ranks(_p(s), _p(t), N, S, D, _p(out), _stream(s.device)))
    return out


def tarp_coverage(samples: torch.Tensor, theta, references="random", metric: str = "euclidean", norm: bool = False,
                  bootstrap: bool = False, num_alpha_bins: Optional[int] = None, num_bootstrap: int = 100,
                  seed: Optional[int] = None, norm_axis: int = 0, return_counts: bool = False):
    """TARP expected coverage (Lemos et al. 2023) of (N,S,D) device draws against (N,D) truths: names and defaults of the
    ``tarp`` package's ``get_tarp_coverage`` (which the reference calls at sbi_runner.py:7116-7122 with ``norm=True,
    bootstrap=True``), restated from the paper and run on the device (``sf_tarp_coverage``; the draws are in THIS project's
    (N,S,D) order, not the package's (S,N,D)).  Returns numpy float64 ``(ecp, alpha)``: ``ecp`` (num_bootstrap, n+1) with
    ``bootstrap``, else (n+1,); ``alpha`` the n+1 credibility levels (of the last pass), n = ``num_alpha_bins`` or N // 10.
    ``references``: "random" (uniform in the unit cube, Philox stream 4 of ``seed``) or an (N,D) array used in every pass.
    ``norm_axis``: which axis ``norm`` takes the min / max of the truths over -- 0 per parameter (the paper's scaling, the
    default), 1 per row; the package's choice is version-dependent and not pinned here.
    ``seed=None`` draws one from numpy's global generator, as the package draws from it.  ``return_counts``: also the
    int32 (B,N) counts #{draws closer to the reference point than the truth} and the int32 (B,N) resampled rows."""
    if not isinstance(samples, torch.Tensor) or samples.device.type != "cuda":
        raise RuntimeError("tarp_coverage runs on the GPU (no CPU fallback)")
    if samples.dim() != 3:
        raise ValueError("samples must be (N, S, D)")
    if metric not in ("euclidean", "manhattan"):
        raise ValueError(f"metric must be 'euclidean' or 'manhattan', not {metric!r}")
    if norm_axis not in (0, 1):
        raise ValueError("norm_axis must be 0 (per parameter) or 1 (per row)")
    s = samples.contiguous().float()
    N, S, D = s.shape
    t = torch.as_tensor(np.array(theta, dtype=np.float32) if not isinstance(theta, torch.Tensor) else theta)
    t = t.to(s.device).float().reshape(N, D).contiguous()
    if isinstance(references, str):
        if references != "random":
            raise ValueError("references must be 'random' or an (N, D) array")
        refs = None
    else:
        refs = torch.as_tensor(np.array(references, dtype=np.float32) if not isinstance(references, torch.Tensor)
                               else references).to(s.device).float().reshape(N, D).contiguous()
    if num_alpha_bins is None:
        if N < 10:
            raise ValueError("num_alpha_bins=None takes N // 10 bins: it needs at least 10 rows")
        num_alpha_bins = N // 10
    n = int(num_alpha_bins)
    B = int(num_bootstrap) if bootstrap else 0
    if bootstrap and B < 1:
        raise ValueError("num_bootstrap must be at least 1")
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 31 - 1))
    rows = max(B, 1)
    ecp = torch.empty((rows, n + 1), dtype=torch.float64, device=s.device)
    alpha = torch.empty((n + 1,), dtype=torch.float64, device=s.device)
    counts = torch.empty((rows, N), dtype=torch.int32, device=s.device) if return_counts else None
    bidx = torch.empty((B, N), dtype=torch.int32, device=s.device) if return_counts and B else None
    _lib.check(_lib.load().sf_tarp_coverage(_p(s), _p(t), N, S, D, _p(refs), 0 if metric == "euclidean" else 1,
                                            int(norm_axis) if norm else -1, B, n, C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                            _p(ecp), _p(alpha), _p(counts), _p(bidx), _stream(s.device)))
    e = ecp.cpu().numpy()
    e = e if bootstrap else e[0]
    if not return_counts:
        return e, alpha.cpu().numpy()
    if bidx is None:
        bidx = torch.arange(N, dtype=torch.int32).reshape(1, N)
    return e, alpha.cpu().numpy(), counts.cpu().numpy(), bidx.cpu().numpy()


def latent_summary(z: torch.Tensor, num_bins: int = 100) -> dict:
    """Residual statistics of (N, D) device latents ``z`` (``FlowPosterior.to_noise_catalogue``), which are N(0, I) for a calibrated
    posterior.  One pass on the device (``sf_latent_summary``: fp64 sums, integer histograms, the same bits on every call) over
    the rows whose D values are all finite; the rest is derived here in float64.  Keys: ``n``, ``n_bad`` (rows with a NaN or
    an infinity, skipped); ``mean`` [D], ``cov`` [D, D] (population, about the mean), ``skew`` [D], ``excess_kurtosis`` [D];
    ``pit_counts`` [D, num_bins], the histogram of u = Phi(z_d), and ``radial_counts`` [num_bins], that of
    u_r = F_chi2_D(|z|^2) -- the expected coverage of the joint posterior read in the base space; ``ks`` [D] and
    ``radial_ks`` = max_k |cum_k / n - k / num_bins|, the distance of each histogram from uniform; ``alpha`` = k / num_bins and
    ``ecp`` = cum_k / n of the radial histogram, k = 0 .. num_bins, a curve to read like ``calculate_TARP``'s.  With no
    finite row the derived values are NaN.  The statistics are those of the flow's own density: see the leakage caveat of
    ``FlowPosterior.to_noise_catalogue``."""
    if not isinstance(z, torch.Tensor) or z.device.type != "cuda":
        raise RuntimeError("latent_summary runs on the GPU (no CPU fallback)")
    if z.dim() != 2:
        raise ValueError("z must be (N, D)")
    zz = z.contiguous().float()
    N, D = zz.shape
    nb = int(num_bins)
    dev = zz.device
    n2 = torch.empty(2, dtype=torch.int64, device=dev)
    psum = torch.empty((4, D), dtype=torch.float64, device=dev)
    cross = torch.empty((D, D), dtype=torch.float64, device=dev)
    pit = torch.empty((D, nb), dtype=torch.int64, device=dev)
    rad = torch.empty((nb,), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().sf_latent_summary(_p(zz), N, D, nb, _p(n2), _p(psum), _p(cross), _p(pit), _p(rad), _stream(dev)))
    n, n_bad = (int(v) for v in n2.cpu().numpy())
    s = psum.cpu().numpy()
    cr = cross.cpu().numpy()
    pit_c, rad_c = pit.cpu().numpy(), rad.cpu().numpy()
    alpha = np.arange(nb + 1, dtype=np.float64) / nb
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.float64(1.0) / np.float64(n) if n else np.float64("nan")
        m1, r2, r3, r4 = (s[k] * inv for k in range(4))                       # raw moments
        cov = cr * inv - np.outer(m1, m1)
        c2 = r2 - m1 ** 2                                                       # central moments
        c3 = r3 - 3.0 * m1 * r2 + 2.0 * m1 ** 3
        c4 = r4 - 4.0 * m1 * r3 + 6.0 * m1 ** 2 * r2 - 3.0 * m1 ** 4
        skew = c3 / c2 ** 1.5
        kurt = c4 / c2 ** 2 - 3.0
        cum = np.concatenate([np.zeros((D, 1)), np.cumsum(pit_c, axis=1, dtype=np.float64)], 1) * inv
        ecp = np.concatenate([[0.0], np.cumsum(rad_c, dtype=np.float64)]) * inv
        ks = np.abs(cum - alpha[None, :]).max(1)
        radial_ks = float(np.abs(ecp - alpha).max())
    return {"n": n, "n_bad": n_bad, "mean": m1, "cov": cov, "skew": skew, "excess_kurtosis": kurt, "pit_counts": pit_c,
            "radial_counts": rad_c, "ks": ks, "radial_ks": radial_ks, "alpha": alpha, "ecp": ecp}
