"""Model of the conditional-posterior sampler (synference_amd/conditional.py, csrc/sf_stretch.hip): float64 numpy on the
Philox stream of ``oracle/philox.py``.  The density is a callable ``potential(theta [B, D], x [B, C]) -> lp [B]``.

The algorithm is the affine-invariant stretch move of Goodman & Weare (2010), emcee's default move, with a = 2, run for
every catalogue row on the slice ``theta_fixed = value`` of the joint density:

Per row i (position p = row_offset + i): a mask over the D parameters and the fixed values, n = D - popcount(mask) >= 1
free coordinates, W walkers (even, 4 <= W <= 64, W >= 2 n + 2) with their raw log-densities.

Start: ``R0`` accepted unconditional draws of the row, fixed coordinates overwritten with the fixed values, the density
evaluated on all of them, the W highest kept (lower index first on ties, non-finite last).  The row is dead (NaN, with
acceptance NaN) with fewer than W finite starts, or a fixed value that is non-finite or outside the prior box.

Step t = 0, 1, ..., half h in {0, 1}: the active walkers are w % 2 == h; for each,
  r       = philox4x32_10((p_lo, p_hi, 2 t + h, w), (seed_lo, seed_hi ^ STREAM_STRETCH))
  partner   j = 2 * (((r0 >> 9) * (W / 2)) >> 23) + (1 - h)                      (integers only: the other half)
  stretch   z = ((a - 1) u01(r1) + 1)^2 / a
  proposal  y_d = theta_j,d + z (theta_w,d - theta_j,d) on the free coordinates; fixed coordinates are copied
  accept    iff y lies inside the box, lp_y is finite and log(u01(r2)) < (n - 1) log z + lp_y - lp_w
The second half reads the walkers the first half has just moved.

Output: after ``burn_in`` steps every ``thin``-th step writes the W walkers and their lp to slots c W + w of the row's S
slots (collecting point c = 0, 1, ...; n_keep = ceil(S / W) of them; slots >= S dropped), so the chain runs
``burn_in + n_keep * thin`` steps; the acceptance is the accepted fraction of all W proposals of all steps.
"""
from __future__ import annotations

import numpy as np

from oracle import philox

STREAM_STRETCH = 0x53545200
A = 2.0


# ---- the random words -------------------------------------------------------------------------------------------------
def words(seed: int, pos, half_step: int, W: int):
    """(r0, r1, r2, r3) uint32 [N, W] for the rows at catalogue positions ``pos`` [N] and walkers 0 .. W - 1."""
    pos = np.asarray(pos, dtype=np.uint64)[:, None]
    w = np.arange(W, dtype=np.uint32)[None, :]
    c0 = np.broadcast_to((pos & philox.MASK).astype(np.uint32), (pos.shape[0], W))
    c1 = np.broadcast_to((pos >> np.uint64(32)).astype(np.uint32), (pos.shape[0], W))
    seed = int(seed) & (2 ** 64 - 1)
    k0 = seed & 0xFFFFFFFF
    k1 = ((seed >> 32) & 0xFFFFFFFF) ^ STREAM_STRETCH
    return philox.philox4x32_10(c0, c1, np.full(c0.shape, half_step, dtype=np.uint32), np.broadcast_to(w, c0.shape), k0, k1)


def u01(r):
    """The stream's uniform ((r >> 9) + 0.5) 2^-23, exact in fp32, as float64."""
    return ((np.asarray(r, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def partner(r0, W: int, h: int):
    """Partner index in the complementary half, integers only."""
    return (2 * (((np.asarray(r0, dtype=np.uint32) >> np.uint32(9)).astype(np.uint64) * np.uint64(W // 2)) >> np.uint64(23))
            + np.uint64(1 - h)).astype(np.int64)


def stretch_z(r1):
    return ((A - 1.0) * u01(r1) + 1.0) ** 2 / A


# ---- row state --------------------------------------------------------------------------------------------------------
def row_plan(condition, lo=None, hi=None):
    """condition [N, D] (NaN = free) -> (mask bool [N, D], n_free [N], dead bool [N]): +-inf where a value is given, or a
    value outside [lo, hi], makes the row dead."""
    c = np.asarray(condition, dtype=np.float64)
    mask = ~np.isnan(c)
    dead = (mask & ~np.isfinite(c)).any(1)
    if lo is not None:
        with np.errstate(invalid="ignore"):
            dead |= (mask & ((c < np.asarray(lo)) | (c > np.asarray(hi)))).any(1)
    return mask, c.shape[1] - mask.sum(1), dead


def select_starts(potential, x, draws, mask, values, W):
    """draws [N, R0, D] -> (theta [N, W, D], lp [N, W], enough bool [N]): the W most probable of the draws with their fixed
    coordinates overwritten; ``enough``: the row has W finite starts."""
    draws = np.array(draws, dtype=np.float64)
    N, R0, D = draws.shape
    draws = np.where(mask[:, None, :], np.asarray(values, np.float64)[:, None, :], draws)
    p0 = np.asarray(potential(draws.reshape(N * R0, D), np.repeat(np.asarray(x), R0, axis=0)), np.float64).reshape(N, R0)
    key = np.where(np.isfinite(p0), p0, -np.inf)
    idx = np.argsort(-key, axis=1, kind="stable")[:, :W]
    theta = np.take_along_axis(draws, idx[:, :, None], axis=1)
    lp = np.take_along_axis(key, idx, axis=1)
    return theta, lp, np.isfinite(lp).all(1)


# ---- one half-step ----------------------------------------------------------------------------------------------------
def propose(theta, mask, seed, pos, half_step):
    """theta [N, W, D] -> (y [N, W/2, D], j [N, W/2], z [N, W/2]) of the active walkers w = 2 q + h, in q order."""
    N, W, D = theta.shape
    h = half_step & 1
    r = words(seed, pos, half_step, W)
    act = np.arange(h, W, 2)
    j = partner(r[0][:, act], W, h)
    z = stretch_z(r[1][:, act])
    tw = theta[:, act, :]
    tj = np.take_along_axis(theta, j[:, :, None], axis=1)
    y = np.where(mask[:, None, :], tw, tj + z[:, :, None] * (tw - tj))
    return y, j, z


def accept_margin(lp_w, lp_y, z, n_free, seed, pos, half_step, W):
    """margin [N, W/2] = (n - 1) log z + lp_y - lp_w - log u01(r2): accepted iff > 0 (and inside the box, lp_y finite)."""
    h = half_step & 1
    r = words(seed, pos, half_step, W)
    logu = np.log(u01(r[2][:, h::2]))
    with np.errstate(invalid="ignore"):
        return (np.asarray(n_free)[:, None] - 1.0) * np.log(z) + lp_y - lp_w - logu


def inside_box(y, lo, hi):
    if lo is None:
        return np.ones(y.shape[:-1], bool)
    return ((y >= np.asarray(lo)) & (y <= np.asarray(hi))).all(-1)


def n_steps(S, W, burn_in, thin):
    return int(burn_in) + (-(-int(S) // int(W))) * int(thin)


# ---- the chain --------------------------------------------------------------------------------------------------------
def run(potential, x, theta0, lp0, mask, alive, lo=None, hi=None, num_samples=1000, burn_in=200, thin=5, seed=0,
        row_offset=0, trace=None):
    """x [N, C], theta0 [N, W, D], lp0 [N, W], mask bool [N, D], alive bool [N] -> (samples [N, S, D], lp [N, S],
    acceptance [N]); dead rows are NaN.  ``trace``: a list that receives one dict per half-step."""
    theta = np.array(theta0, dtype=np.float64)
    lp = np.array(lp0, dtype=np.float64)
    N, W, D = theta.shape
    S = int(num_samples)
    pos = int(row_offset) + np.arange(N)
    n_free = D - mask.sum(1)
    xr = np.repeat(np.asarray(x), W // 2, axis=0)
    out = np.full((N, S, D), np.nan)
    out_lp = np.full((N, S), np.nan)
    acc = np.zeros(N)
    T = n_steps(S, W, burn_in, thin)
    for t in range(T):
        for h in (0, 1):
            hs = 2 * t + h
            y, j, z = propose(theta, mask, seed, pos, hs)
            lpy = np.asarray(potential(y.reshape(N * (W // 2), D), xr), np.float64).reshape(N, W // 2)
            m = accept_margin(lp[:, h::2], lpy, z, n_free, seed, pos, hs, W)
            ok = inside_box(y, lo, hi) & np.isfinite(lpy) & (m > 0)
            if trace is not None:
                trace.append(dict(half_step=hs, prop=y, partner=j, z=z, lp_prop=lpy, margin=m, accept=ok))
            theta[:, h::2] = np.where(ok[:, :, None], y, theta[:, h::2])
            lp[:, h::2] = np.where(ok, lpy, lp[:, h::2])
            acc += ok.sum(1)
        done = t + 1
        if done > burn_in and (done - burn_in) % thin == 0:
            c = (done - burn_in) // thin - 1
            n = min(W, S - c * W)
            out[:, c * W:c * W + n] = theta[:, :n]
            out_lp[:, c * W:c * W + n] = lp[:, :n]
    dead = ~np.asarray(alive, bool)
    out[dead], out_lp[dead] = np.nan, np.nan
    return out, out_lp, np.where(dead, np.nan, acc / (T * W))


# ---- comparison with a tabulated distribution ----------------------------------------------------------------------
def ks_distance(draws, grid, cdf):
    """sup |ECDF - F| of a sample against a CDF tabulated on ``grid`` (linear interpolation)."""
    s = np.sort(np.asarray(draws, np.float64))
    F = np.interp(s, grid, cdf)
    n = len(s)
    return float(max(np.abs(F - np.arange(n) / n).max(), np.abs(F - np.arange(1, n + 1) / n).max()))


# ---- analytic target --------------------------------------------------------------------------------------------------
def gaussian_potential(mean, cov):
    mean, P = np.asarray(mean, np.float64), np.linalg.inv(np.asarray(cov, np.float64))
    _, logdet = np.linalg.slogdet(np.asarray(cov, np.float64))

    def fn(theta, x):
        d = np.asarray(theta, np.float64) - mean
        return -0.5 * np.einsum("bi,ij,bj->b", d, P, d) - 0.5 * logdet - 0.5 * len(mean) * np.log(2 * np.pi)
    return fn


def gaussian_conditional(mean, cov, fixed_idx, values):
    """Mean and covariance of the free coordinates of N(mean, cov) given theta[fixed_idx] = values."""
    mean, cov = np.asarray(mean, np.float64), np.asarray(cov, np.float64)
    f = np.asarray(fixed_idx)
    u = np.array([d for d in range(len(mean)) if d not in set(f.tolist())])
    K = cov[np.ix_(u, f)] @ np.linalg.inv(cov[np.ix_(f, f)])
    return u, mean[u] + K @ (np.asarray(values, np.float64) - mean[f]), cov[np.ix_(u, u)] - K @ cov[np.ix_(f, u)]
