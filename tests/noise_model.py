"""Numpy model of csrc/sf_noise.hip (TEST INFRASTRUCTURE): the two entry points restated on the PACKED model -- the
``sf_noise_band`` fields and the float32 table that the host hands to the device -- with explicit uniforms, evaluated in
float64 (the yardstick) or, ``dtype=np.float32``, with every intermediate rounded as the kernel rounds it.

What it restates of the reference (src/synference/noise_models.py): 383-390 ``sample_uncertainty`` (a normal truncated to
sigma >= 0, here by its quantile function instead of ``scipy.stats.truncnorm.rvs``), 818-880 the General ``apply_noise``,
882-894 the SNR mask, 896-957 the flux and error rules (as the one number per band that the host packs), 959-987 the units
out, 507-560 the Asinh ``apply_noise`` in the reference's own order, 1074-1099 and 562-592 ``apply_scalings``; magnitudes:
utils.py:672 and 704.  The uniforms are the kernel's: one Philox4x32-10 call per output element, key (seed, stream 6),
counter (out_row lo, out_row hi, 0, band), u = ((r >> 9) + 0.5) 2^-23 (oracle/philox.py).
"""
import numpy as np
from scipy import special

from oracle import philox

STREAM = 6
GENERAL, ASINH = 0, 1
PHYSICAL, AB, ASINH_SPACE = 0, 1, 2
SCATTER, LIMIT, NUMBER = 0, 1, 2


def uniforms(seed: int, out_rows, band: int):
    """u0..u3 [4, n] float32 of the output rows ``out_rows`` of column ``band``."""
    rows = np.asarray(out_rows, dtype=np.uint64)
    k0, k1 = seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ STREAM
    r = philox.philox4x32_10((rows & philox.MASK).astype(np.uint32), (rows >> np.uint64(32)).astype(np.uint32),
                             np.zeros(rows.shape, np.uint32), np.full(rows.shape, band, np.uint32), k0, k1)
    return np.stack([philox._u01(x) for x in r])


class Band:
    """One packed band: the struct's fields as attributes (floats in ``dt``) and its three tables."""

    def __init__(self, fields: dict, table: np.ndarray, dt):
        self.dt = dt
        for k, v in fields.items():
            setattr(self, k, dt(v) if isinstance(v, float) else v)
        n, o = self.n_bins, self.table_offset
        self.c, self.med, self.std = (table[o + i * n:o + (i + 1) * n].astype(dt) for i in range(3))


def _k(b, v):
    return b.dt(v)


def interp(b: Band, x):
    """mu, ss = the median table and max(0, std table) at x; NaN in, NaN out."""
    n = b.n_bins
    lo = np.clip(np.searchsorted(b.c, x, side="right") - 1, 0, n - 2)
    with np.errstate(invalid="ignore"):
        xc = x if b.extrapolate else np.minimum(np.maximum(x, b.c[0]), b.c[n - 1])
        t = (xc - b.c[lo]) / (b.c[lo + 1] - b.c[lo])
        mu = b.med[lo] + t * (b.med[lo + 1] - b.med[lo])
        sv = b.std[lo] + t * (b.std[lo + 1] - b.std[lo])
        ss = np.where(np.isnan(sv), sv, np.maximum(_k(b, 0), sv))
    nan = np.isnan(x)
    return np.where(nan, _k(b, np.nan), mu).astype(b.dt), np.where(nan, _k(b, np.nan), ss).astype(b.dt)


def lower_trunc_quantile(b, a, u):
    """Quantile u of N(0,1) truncated to [a, inf), from the tail mass Q(a) (1 - u)."""
    dt = b.dt
    with np.errstate(invalid="ignore", under="ignore"):
        Qa = dt(0.5) * special.erfc(a * dt(0.70710678118654752))
        q = np.maximum(Qa * (dt(1) - u), dt(1.17549435e-38))
        Pa = dt(0.5) * special.erfc(-a * dt(0.70710678118654752))
        low = -special.ndtri(np.minimum(q, dt(0.5)))
        high = special.ndtri(np.minimum(Pa + u * Qa, dt(1)))
        return np.where(np.isnan(q), q, np.where(q <= dt(0.5), low, high)).astype(dt)


def clip_quantile(b, c, u):
    """Quantile u of N(0,1) truncated to [-c, c], evaluated in the lower half and mirrored."""
    dt = b.dt
    Pl = dt(0.5) * special.erfc(dt(c) * dt(0.70710678118654752))
    up = u > dt(0.5)
    v = np.where(up, dt(1) - u, u).astype(dt)
    z = special.ndtri(Pl + v * (dt(1) - dt(2) * Pl)).astype(dt)
    return np.where(up, -z, z).astype(dt)


def sample_sigma(b, x, u, parts=None):
    mu, ss = interp(b, x)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.minimum(-mu / np.where(ss > _k(b, 1e-9), ss, _k(b, 1)), _k(b, 12))
        a = np.where(np.isnan(mu), mu, a).astype(b.dt)
        t = lower_trunc_quantile(b, a, u.astype(b.dt))
        if parts is not None:
            parts.update(mu=mu, ss=ss, a=a, t=t)
        return (mu + ss * t).astype(b.dt)


K25 = 1.0857362047581294      # 2.5 / ln 10
L25 = 0.92103403719761836     # ln 10 / 2.5


def snr(b, x, e):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        if b.interp_space == AB:
            fj = np.power(_k(b, 10), _k(b, -0.4) * (x - _k(b, 8.9)))
            return ((fj / fj) * (_k(b, K25) / e)).astype(b.dt)
        return (x / e).astype(b.dt)


def snr_below(b, x, e):
    s = snr(b, x, e)
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(s) | (s < b.snr_threshold)


def clip_err(b, s):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(s), s, np.minimum(np.maximum(s, b.min_err), b.max_err)).astype(b.dt)


def asinh_mag(b, fj):
    return (-_k(b, K25) * (np.arcsinh(fj / (_k(b, 2) * b.b_jy)) + np.log(b.b_jy * (_k(b, 1) / _k(b, 3631))))).astype(b.dt)


def exp10(b, x):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.power(_k(b, 10), x).astype(b.dt)


def input_jy(b, f):
    return exp10(b, _k(b, -0.4) * (f - _k(b, 8.9))) if b.in_space == AB else (f * b.in_to_jy).astype(b.dt)


def general_out(b, y, s, clip=True):
    """(y, s) from the interpolation space to the output space; the error is linear in s (used for the scales, clip=False)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        if b.interp_space == AB:
            if b.out_space != AB:
                fo = exp10(b, _k(b, -0.4) * (y - b.zp_out))
                y, s = fo, fo * s * _k(b, L25)
        elif b.out_space == AB:
            y, s = b.zp_unit - _k(b, 2.5) * np.log10(y), np.abs(_k(b, K25) * (s / y))
        else:
            y, s = y * b.unit_to_out, s * b.unit_to_out
    return y.astype(b.dt), (clip_err(b, s) if clip else s.astype(b.dt))


def general_in(b, f):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        if b.interp_space == AB:
            return (f if b.in_space == AB else b.zp_in - _k(b, 2.5) * np.log10(f)).astype(b.dt)
        return (exp10(b, _k(b, -0.4) * (f - b.zp_unit)) if b.in_space == AB else f * b.in_to_unit).astype(b.dt)


def scatter_band(fields, table, flux, u, dtype=np.float64):
    """One column: flux [n] (already repeated per scatter copy) and u [4, n] -> dict(y, s, flux_scale, err_scale, margin):
    the scales are the scatter sigma and the std of the sigma distribution carried to the output space (each element's
    own yardstick), margin the smallest relative distance of an SNR that was tested to the threshold (inf: not tested)."""
    b = Band(fields, table, dtype)
    f, u = np.asarray(flux, np.float32).astype(dtype), np.asarray(u, np.float32).astype(dtype)
    p1, p2 = {}, {}
    margin = np.full(f.shape, np.inf)

    def test_snr(x, e):
        nonlocal margin
        with np.errstate(invalid="ignore", divide="ignore"):
            s_ = snr(b, x, e).astype(np.float64)
            m = np.abs(s_ - float(b.snr_threshold)) / abs(float(b.snr_threshold))
        margin = np.minimum(margin, np.where(np.isfinite(s_), m, np.inf))
        return snr_below(b, x, e)

    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        if b.kind == GENERAL:
            x = general_in(b, f)
            s1 = sample_sigma(b, x, u[0], p1)
            lim0 = test_snr(x, s1) if b.upper_limits else np.zeros(f.shape, bool)
            z = clip_quantile(b, b.sigma_clip, u[1]) if b.sigma_clip >= 0 else special.ndtri(u[1]).astype(dtype)
            y = np.where(lim0, x, x + s1 * z).astype(dtype)
            s = sample_sigma(b, y, u[2], p2) if b.resample else s1
            ss_last = p2["ss"] if b.resample else p1["ss"]
            if b.upper_limits and b.has_limit:
                lim = lim0 | test_snr(y, s)
                if b.flux_rule == SCATTER:
                    yl = b.limit_value + b.std_at_limit * clip_quantile(b, 3.0, u[3])
                else:
                    yl = np.full(f.shape, b.limit_value if b.flux_rule == LIMIT else b.flux_number, dtype)
                y = np.where(lim, yl, y).astype(dtype)
                if b.replace_err:
                    s = np.where(lim, b.err_value, s).astype(dtype)
            oy, os_ = general_out(b, y, s)
            _, fs = general_out(b, y, s1, clip=False)
            _, es = general_out(b, y, ss_last, clip=False)
        else:
            fj = input_jy(b, f)
            z = special.ndtri(u[1]).astype(dtype)
            if b.interp_space == ASINH_SPACE:
                m = asinh_mag(b, fj)
                s1 = sample_sigma(b, m, u[0], p1)
                oy = (m + s1 * z).astype(dtype)
                s = sample_sigma(b, oy, u[2], p2) if b.resample else s1
                fs, es = s1, (p2["ss"] if b.resample else p1["ss"])
            else:
                s1 = sample_sigma(b, (fj * b.unit_per_jy).astype(dtype), u[0], p1)
                yj = (fj + (s1 * b.jy_per_unit) * z).astype(dtype)
                oy = asinh_mag(b, yj)
                e = sample_sigma(b, (yj * b.unit_per_jy).astype(dtype), u[2], p2) if b.resample else s1
                g = _k(b, K25) * b.jy_per_unit / np.sqrt(yj * yj + _k(b, 4) * b.b_jy * b.b_jy)
                s = (_k(b, K25) * (e * b.jy_per_unit) / np.sqrt(yj * yj + _k(b, 4) * b.b_jy * b.b_jy)).astype(dtype)
                fs, es = s1 * g, (p2["ss"] if b.resample else p1["ss"]) * g
            os_ = clip_err(b, s)
    return dict(y=oy, s=os_, flux_scale=np.abs(np.asarray(fs, np.float64)), err_scale=np.abs(np.asarray(es, np.float64)),
                margin=margin, sigma1=s1, parts1=p1)


def scalings_band(fields, table, flux, err, dtype=np.float64):
    """The deterministic twin on one column: dict(y, s, margin)."""
    b = Band(fields, table, dtype)
    f, e = np.asarray(flux, np.float32).astype(dtype), np.asarray(err, np.float32).astype(dtype)
    margin = np.full(f.shape, np.inf)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        if b.kind == ASINH:
            fj = input_jy(b, f)
            ej = fj * e * _k(b, L25) if b.in_space == AB else e * b.in_to_jy
            s = _k(b, K25) * ej / np.sqrt(fj * fj + _k(b, 4) * b.b_jy * b.b_jy)
            return dict(y=asinh_mag(b, fj), s=clip_err(b, s.astype(dtype)), margin=margin)
        if b.interp_space == AB:
            x, s = (f, e) if b.in_space == AB else (b.zp_in - _k(b, 2.5) * np.log10(f), np.abs(_k(b, K25) * (e / f)))
        elif b.in_space == AB:
            x = exp10(b, _k(b, -0.4) * (f - b.zp_unit))
            s = x * e * _k(b, L25)
        else:
            x, s = f * b.in_to_unit, e * b.in_to_unit
        x, s = x.astype(dtype), s.astype(dtype)
        if b.upper_limits and b.has_limit:
            sn = snr(b, x, s).astype(np.float64)
            margin = np.where(np.isfinite(sn), np.abs(sn - float(b.snr_threshold)) / abs(float(b.snr_threshold)), np.inf)
            lim = snr_below(b, x, s)
            x = np.where(lim, b.flux_number if b.flux_rule == NUMBER else b.limit_value, x).astype(dtype)
            if b.replace_err:
                s = np.where(lim, b.err_value, s).astype(dtype)
        oy, os_ = general_out(b, x, s)
    return dict(y=oy, s=os_, margin=margin)


def scatter(bands_fields, table, flux, n_scatters, seed, dtype=np.float64, row_offset=0):
    """The whole call: flux [N, C] -> per column results of ``scatter_band`` for the N * n_scatters output rows."""
    flux = np.asarray(flux, np.float32)
    rows = np.arange(flux.shape[0] * n_scatters, dtype=np.uint64) + np.uint64(row_offset)
    rep = np.repeat(flux, n_scatters, axis=0)
    return [scatter_band(fb, table, rep[:, c], uniforms(seed, rows, c), dtype) for c, fb in enumerate(bands_fields)]
