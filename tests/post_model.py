"""Plain numpy fp64 reference of the six entry points of csrc/sf_post.hip (quantiles by sort and by radix select, PIT ranks, AB
and asinh magnitudes, depth scatter).  Helper module, no tests in it, no device.

The two rules every kernel, wrapper, header and document states:

  quantile   per (row, dim): drop NaN; n = the non-NaN draws, +-inf included as ordered values; n == 0 -> NaN;
             pos = (n - 1) * float64(float32(q))  (the ABI carries q as float32: the reference uses THAT value, widened);
             lo = clamp(floor(pos), 0, n - 1), hi = min(lo + 1, n - 1), f = pos - lo;
             v[lo] where f == 0, else v[lo] + f (v[hi] - v[lo]) in the extended reals (NaN only where that is inf - inf).
  PIT        #{s < t} / #{non-NaN s}; NaN when there is no non-NaN draw; +-inf draws are ordered values and count on both sides;
             a NaN truth is above nothing and gives 0.

``quantiles`` and ``pit_ranks`` take switches that plant the defects the device code once had (tests/test_cpu_post_cases.py
shows that the comparison functions below reject each of them); the default of every switch is the rule.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from oracle import features as OF
from sharp_cases import check_bar  # noqa: F401  (the one bar rule: imported, not copied; re-exported for the tests)

QDetail = namedtuple("QDetail", "value vlo vhi f n")   # [N, D, Q] float64 each (n: [N, D] int)


# ---------------------------------------------------------------------------------------------------------------------------
# quantiles
# ---------------------------------------------------------------------------------------------------------------------------
def quantiles_detail(x, q, position_dtype=np.float64, drop_pos_inf: bool = False, guard: bool = True) -> QDetail:
    """The rule above on x [N, S, D]; every output [N, D, Q] float64.  ``vlo`` / ``vhi``: the two order statistics the result lies
    between (the knots the bar is taken at), ``f`` the fraction.
    Planted defects: ``position_dtype=np.float32`` forms pos and f in fp32 (and interpolates with the fp32 f), ``drop_pos_inf``
    leaves +inf draws out of n, ``guard=False`` evaluates v[lo] + f (v[hi] - v[lo]) at f == 0 as well."""
    x = np.asarray(x)
    N, S, D = x.shape
    q32 = np.asarray(q, dtype=np.float32).reshape(-1)
    pd = np.dtype(position_dtype).type
    qq = q32.astype(position_dtype)
    out = {k: np.full((N, D, len(q32)), np.nan) for k in ("value", "vlo", "vhi", "f")}
    cnt = np.zeros((N, D), np.int64)
    for g in range(N):
        for d in range(D):
            col = x[g, :, d].astype(np.float64)
            v = np.sort(col[~np.isnan(col)])                     # (+-0 compare equal: either order is a sorted row)
            n = len(v) - (int(np.sum(v == np.inf)) if drop_pos_inf else 0)
            cnt[g, d] = n
            if n == 0:
                continue
            pos = pd(n - 1) * qq
            lo = np.clip(np.floor(pos).astype(np.int64), 0, n - 1)
            hi = np.minimum(lo + 1, n - 1)
            f = (pos - lo.astype(position_dtype)).astype(np.float64)
            with np.errstate(invalid="ignore"):
                lin = v[lo] + f * (v[hi] - v[lo])
            out["value"][g, d] = np.where(f == 0, v[lo], lin) if guard else lin
            out["vlo"][g, d], out["vhi"][g, d], out["f"][g, d] = v[lo], v[hi], f
    return QDetail(out["value"], out["vlo"], out["vhi"], out["f"], cnt)


def quantiles(x, q, position_dtype=np.float64, **defects):
    return quantiles_detail(x, q, position_dtype, **defects).value


def ulp32(a):
    """One fp32 ulp at |a| (float64 array); the smallest subnormal at 0, inf at inf."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    with np.errstate(over="ignore", invalid="ignore"):
        a32 = a.astype(np.float32)
        return np.where(np.isfinite(a32), np.spacing(np.where(np.isfinite(a32), a32, np.float32(0))).astype(np.float64), np.inf)


def check_quantiles(label: str, got, det: QDetail):
    """The comparison of tests/test_gpu_post.py: NaN exactly where the model has NaN; an infinite model value exactly; where
    f == 0 the order statistic itself, with no tolerance; elsewhere |got - model| <= 1 fp32 ulp of max(|v[lo]|, |v[hi]|): the device
    interpolates in fp64 and rounds once, half an ulp of the result, and the result's magnitude never exceeds the larger knot's.
    The bar sits at the knots so that a result near zero between two modes is not given a vanishing one.
    Returns the worst |difference| / bar."""
    got = np.asarray(got, dtype=np.float64)
    want = det.value
    assert got.shape == want.shape, (label, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (label, "NaN pattern", np.argwhere(np.isnan(got) != nan)[:5].tolist())
    exact = ~nan & ((det.f == 0) | np.isinf(want))
    bad = exact & (got != want)
    assert not bad.any(), (label, "order statistic / infinite value not exact", np.argwhere(bad)[:5].tolist(),
                           got[bad][:5].tolist(), want[bad][:5].tolist())
    rest = ~nan & ~exact
    worst = 0.0
    if rest.any():
        bar = ulp32(np.maximum(np.abs(det.vlo[rest]), np.abs(det.vhi[rest])))
        err = np.abs(got[rest] - want[rest])
        worst = float((err / bar).max())
        assert np.isfinite(got[rest]).all() and (err <= bar).all(), (label, "worst |difference| / (ulp at the knots)", worst)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# PIT
# ---------------------------------------------------------------------------------------------------------------------------
def pit_ranks(s, t, strict: bool = True, finite_denominator: bool = False):
    """The rule above on s [N, S, D], t [N, D] -> [N, D] float64.  Planted defects: ``strict=False`` counts s <= t,
    ``finite_denominator`` divides by the finite draws."""
    s = np.asarray(s, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)[:, None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        below = ((s < t) if strict else (s <= t)).sum(1)
        valid = (np.isfinite(s) if finite_denominator else ~np.isnan(s)).sum(1)
        return np.where(valid > 0, below / np.maximum(valid, 1), np.nan)


def check_pit(label: str, got, want):
    """NaN exactly where the model has NaN; elsewhere 1 fp32 ulp of the fp64 ratio: both counts are exact integers below 2^24 and
    the division is the only rounding (half an ulp).  Returns the worst |difference| / bar."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (label, "NaN pattern", np.argwhere(np.isnan(got) != nan)[:5].tolist())
    ok = ~nan
    if not ok.any():
        return 0.0
    bar = ulp32(want[ok])
    err = np.abs(got[ok] - want[ok])
    worst = float((err / bar).max())
    assert (err <= bar).all(), (label, "worst |difference| / ulp", worst, np.argwhere(ok)[np.argmax(err / bar)].tolist())
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# magnitudes: the formulas of oracle/features.py, evaluated in ``dtype`` (float64: the reference; float32: its own fp32 error)
# ---------------------------------------------------------------------------------------------------------------------------
def abmag(f, e=None, lim: float = 50.0, dtype=np.float64):
    """mag = -2.5 log10(f / 1000) + 23.9; f < 0 -> lim; mag > lim (f == +-0 gives +inf) -> lim; a NaN flux stays NaN; +inf flux
    -> -inf.  With ``e``: (mag, 2.5 e / (ln 10 f)), not special-cased (inf at f == 0, negative at f < 0)."""
    T = np.dtype(dtype).type
    f = np.asarray(f).astype(dtype)
    with np.errstate(all="ignore"):
        mag = T(-2.5) * np.log10(f / T(1000.0)) + T(23.9)
        mag = np.where(f < 0, T(lim), mag)
        mag = np.where(mag > T(lim), T(lim), mag).astype(dtype)
        if e is None:
            return mag
        return mag, (T(2.5) * np.asarray(e).astype(dtype) / (T(np.log(10.0)) * f)).astype(dtype)


def asinh_mag(f, fb, e=None, dtype=np.float64):
    """oracle.features.flux_to_asinh in ``dtype``: -K (asinh(f / 2 f_b) + ln(f_b 1e-9 / 3631)); with ``e`` also
    K e / sqrt(f^2 + (2 f_b)^2)."""
    T = np.dtype(dtype).type
    f = np.asarray(f).astype(dtype)
    fb = np.broadcast_to(np.asarray(fb).astype(dtype), f.shape[-1:])
    K = T(OF.K)
    with np.errstate(all="ignore"):
        mag = (-K * (np.arcsinh(f / (T(2) * fb)) + np.log(fb * T(1e-9) / T(3631.0)))).astype(dtype)
        if e is None:
            return mag
        return mag, (K * np.asarray(e).astype(dtype) / np.sqrt(f * f + (T(2) * fb) ** 2)).astype(dtype)


def check_ulps(label: str, got, want, ulps: float):
    """Per element: non-finite reference values (as fp32) exactly, the others to ``ulps`` fp32 ulp of |want|."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(over="ignore"):
        w32 = want.astype(np.float32).astype(np.float64)
    special = ~np.isfinite(w32)
    assert np.array_equal(np.isnan(got), np.isnan(w32)), (label, "NaN pattern")
    inf = special & ~np.isnan(w32)
    assert np.array_equal(got[inf], w32[inf]), (label, "infinite values")
    ok = ~special
    err = np.abs(got[ok] - want[ok]) / ulp32(want[ok])
    worst = float(err.max()) if err.size else 0.0
    assert np.isfinite(got[ok]).all() and worst <= ulps, (label, "worst |difference| / ulp", worst)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# depth scatter
# ---------------------------------------------------------------------------------------------------------------------------
def scatter_depths(flux, sigma, n_scatters, min_flux_pc_error, seed, rows=None):
    """oracle.features.scatter_depths on sigma rows given as the ABI takes them ([1, C] or [n_scatters, C], = depth / depth_sigma
    already), for the output rows ``rows`` only (all when None): the Philox counter is the output row, so a 2-million-row
    case is checked on a few hundred rows without generating the rest.  Returns (out, sigma) [len(rows), C] float64."""
    sigma = np.atleast_2d(np.asarray(sigma, dtype=np.float64))
    return OF.scatter_depths(flux, sigma if sigma.shape[0] > 1 else sigma[0], n_scatters, 1.0, min_flux_pc_error, seed, rows=rows)


def draw_bar(out_ref, sigma_ref):
    """The existing 2e-4 of test_scatter_depths_matches_oracle_draw_for_draw, scaled: that bar was set with sigma <= 6 and
    |out| <= ~200; the fp32 Box-Muller error (|dz| ~ 1e-6 .. 1e-5) scales with sigma and the final rounding with |out|."""
    return 2e-4 * np.maximum(1.0, np.maximum(np.asarray(sigma_ref) / 6.0, np.abs(out_ref) / 200.0))
