"""TARP expected coverage in numpy -- the model that sf_tarp_coverage (synference_amd/csrc/sf_tarp.hip) is tested against.

TEST INFRASTRUCTURE ONLY.  "Tests of Accuracy with Random Points" (Lemos et al. 2023, "Sampling-Based Accuracy Testing of
Posterior Estimators"), restated from the paper; the reference reaches it through the third-party ``tarp`` package
(ref: src/synference/sbi_runner.py:7090-7126, ``get_tarp_coverage(samples, y, norm=True, bootstrap=True, ...)``).

Inputs: draws x[i, s, :] (N rows, S draws, D parameters, float32) and truths theta[i, :] (float32).  Everything below is
computed in float64 ON those float32 values.  One pass over a row list idx[0..N) and reference points r[j, :], i = idx[j]:

1. normalisation (``norm_axis`` 0 or 1; -1 / None: none): low, high = min / max of the RESAMPLED truths theta[idx] over
   the positions (axis 0, shape [D]) or over the parameters (axis 1, shape [N]); v = (v - low) / (high - low + 1e-10) for
   draws and truths alike
2. distance: euclidean sqrt(sum_d (r - v)^2) or manhattan sum_d |r - v|
3. k_j = #{s : dist(r_j, x[i, s]) < dist(r_j, theta_i)} (a NaN draw compares False and stays in the denominator),
   f_j = k_j / S
4. curve: h, alpha = np.histogram(f, density=True, bins=n); ecp = [0, cumsum(h) * (alpha[1] - alpha[0])]
   -- ``curve_histogram`` -- or, in exact terms -- ``curve_counts`` -- ecp[e] = #{j : f_j < edges[e]} / N for 0 < e < n,
   ecp[0] = 0, ecp[n] = 1 on the same edges
5. bootstrap: B passes, each with its own idx (N positions drawn with replacement) and its own r; explicit references are
   used by position j in every pass.  Without bootstrap: one pass, idx = arange(N), b = 0.

Random streams (oracle/philox.py, csrc/sf_rng.h; streams 0-2 are the sampler's and the depth scatter's):
  row resample      key (seed, stream 3), counter (j_lo, j_hi, b, 0):      idx[b, j] = (uint64(r0) * N) >> 32
  reference points  key (seed, stream 4), counter (j_lo, j_hi, b, d // 4): r[b, j, d] = u01(r[d % 4])
"""
from __future__ import annotations

import numpy as np

from oracle.philox import MASK, _u01, philox4x32_10


def _key(seed: int, stream: int):
    return seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ stream


def _jb(N: int, B: int):
    j = np.broadcast_to(np.arange(N, dtype=np.uint64)[None, :], (B, N))
    b = np.broadcast_to(np.arange(B, dtype=np.uint32)[:, None], (B, N))
    return (j & MASK).astype(np.uint32), (j >> np.uint64(32)).astype(np.uint32), b


def boot_indices(seed: int, N: int, B: int) -> np.ndarray:
    """[B, N] int64 rows drawn with replacement (stream 3)."""
    jl, jh, b = _jb(N, B)
    k0, k1 = _key(seed, 3)
    r0 = philox4x32_10(jl, jh, b, np.zeros((B, N), np.uint32), k0, k1)[0]
    return ((r0.astype(np.uint64) * np.uint64(N)) >> np.uint64(32)).astype(np.int64)


def reference_points(seed: int, N: int, D: int, B: int) -> np.ndarray:
    """[B, N, D] float32 uniforms in [0, 1) (stream 4)."""
    jl, jh, b = _jb(N, B)
    k0, k1 = _key(seed, 4)
    out = np.empty((B, N, D), np.float32)
    for blk in range((D + 3) // 4):
        r = philox4x32_10(jl, jh, b, np.full((B, N), blk, np.uint32), k0, k1)
        for t in range(4):
            if 4 * blk + t < D:
                out[:, :, 4 * blk + t] = _u01(r[t])
    return out


def _normalise(xs, th, norm_axis):
    """xs [N,S,D], th [N,D] (already resampled, float64) -> normalised copies."""
    if norm_axis is None or norm_axis < 0:
        return xs, th
    if norm_axis == 0:
        low, high = th.min(axis=0), th.max(axis=0)                    # [D]
        return (xs - low) / (high - low + 1e-10), (th - low) / (high - low + 1e-10)
    low, high = th.min(axis=1, keepdims=True), th.max(axis=1, keepdims=True)   # [N,1]
    return (xs - low[:, None, :]) / (high - low + 1e-10)[:, None, :], (th - low) / (high - low + 1e-10)


def _dist(a, metric):
    if metric == "euclidean":
        return np.sqrt(np.sum(a * a, axis=-1))
    if metric == "manhattan":
        return np.sum(np.abs(a), axis=-1)
    raise ValueError(f"metric must be 'euclidean' or 'manhattan', not {metric!r}")


# The band.  The device evaluates the same expressions in float32.  With normalised coordinates of order one, a
# coordinate (v - low) * inv carries 2-3 roundings (subtraction, reciprocal, product), r - t one more, and the D <= 16
# squares and their sum about 2 D more: some 40-50 roundings of 2^-24 = 6e-8 on each side of the comparison, about a
# hundred in all, i.e. an absolute distance error below 100 * 6e-8 * (1 + dist) ~ 6e-6 (1 + dist).  tau = 2e-5 (1 + dist)
# leaves a factor three on top, and is still so narrow that only a handful of draws per thousand cells fall inside it.
TAU = 2e-5


def pass_counts(x, theta, idx, r, metric="euclidean", norm_axis=0, band=False):
    """Counts k[j] of one pass (int64 [N]); with ``band`` also (k_lo, k_hi) for dist_theta -/+ tau."""
    xs = np.asarray(x)[idx].astype(np.float64)
    th = np.asarray(theta)[idx].astype(np.float64)
    xs, th = _normalise(xs, th, norm_axis)
    r = np.asarray(r, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d_s = _dist(r[:, None, :] - xs, metric)                        # [N,S]
        d_t = _dist(r - th, metric)                                    # [N]
        k = np.sum(d_s < d_t[:, None], axis=1).astype(np.int64)
        if not band:
            return k
        tau = TAU * (1.0 + d_t)
        k_lo = np.sum(d_s < (d_t - tau)[:, None], axis=1).astype(np.int64)
        k_hi = np.sum(d_s < (d_t + tau)[:, None], axis=1).astype(np.int64)
    return k, k_lo, k_hi


def curve_histogram(k, S: int, n: int):
    """(ecp [n+1], alpha [n+1]) the way the package forms them."""
    f = np.asarray(k, dtype=np.int64) / int(S)
    h, alpha = np.histogram(f, density=True, bins=n)
    dx = alpha[1] - alpha[0]
    return np.concatenate([[0.0], np.cumsum(h) * dx]), alpha


def curve_counts(k, S: int, n: int):
    """The same curve in exact terms: integer counts below the float64 edges of np.histogram / np.linspace."""
    k = np.asarray(k, dtype=np.int64)
    N = len(k)
    f = k / int(S)
    first, last = f.min(), f.max()
    if first == last:
        first, last = first - 0.5, last + 0.5
    step = (last - first) / n
    edges = np.arange(n + 1, dtype=np.float64) * step + first         # a multiply, then an add
    edges[n] = last
    ecp = np.empty(n + 1)
    ecp[0], ecp[n] = 0.0, 1.0
    for e in range(1, n):
        ecp[e] = np.count_nonzero(f < edges[e]) / N
    return ecp, edges


def tarp_coverage(x, theta, references="random", metric="euclidean", norm=False, bootstrap=False, num_alpha_bins=None,
                  num_bootstrap=100, seed=0, norm_axis=0, curve=curve_counts, band=False):
    """The whole call.  Returns a dict: ecp [B, n+1] ([n+1] without bootstrap), alpha (last pass), counts [B, N],
    idx [B, N], and with ``band`` k_lo / k_hi [B, N]."""
    x, theta = np.asarray(x, np.float32), np.asarray(theta, np.float32)
    N, S, D = x.shape
    n = num_alpha_bins if num_alpha_bins is not None else N // 10
    if n < 1:
        raise ValueError("num_alpha_bins=None needs at least 10 rows")
    B = int(num_bootstrap) if bootstrap else 1
    idx = boot_indices(seed, N, B) if bootstrap else np.arange(N, dtype=np.int64)[None, :]
    if isinstance(references, str):
        if references != "random":
            raise ValueError("references must be 'random' or an (N, D) array")
        refs = reference_points(seed, N, D, B)
    else:
        refs = np.broadcast_to(np.asarray(references, np.float32).reshape(1, N, D), (B, N, D))
    ax = norm_axis if norm else -1
    out = {"counts": np.empty((B, N), np.int64), "idx": idx, "ecp": np.empty((B, n + 1)), "alpha": None}
    if band:
        out["k_lo"], out["k_hi"] = np.empty((B, N), np.int64), np.empty((B, N), np.int64)
    for b in range(B):
        res = pass_counts(x, theta, idx[b], refs[b], metric, ax, band)
        if band:
            out["counts"][b], out["k_lo"][b], out["k_hi"][b] = res
        else:
            out["counts"][b] = res
        out["ecp"][b], out["alpha"] = curve(out["counts"][b], S, n)
    if not bootstrap:
        out["ecp"] = out["ecp"][0]
    return out


def tarp_value(ecp) -> float:
    """| mean_b ecp[b, (n + 1) // 2] - 0.5 |: the reference's ``ecp[:, ecp.shape[1] // 2]`` (sbi_runner.py:7124-7126)."""
    ecp = np.atleast_2d(ecp)
    return float(abs(ecp[:, ecp.shape[1] // 2].mean() - 0.5))


def gaussian_case(N: int, S: int, D: int, seed: int, shift: float = 0.0):
    """The unit normal-normal model: truths theta ~ N(0, 1), observation x = theta + N(0, 1); the exact conjugate
    posterior is N(x / 2, 1 / 2).  ``shift`` moves its mean by that many posterior sigmas in every parameter
    (miscalibrated).  Returns draws (N, S, D) and truths (N, D), float32."""
    rng = np.random.default_rng(seed)
    theta = rng.normal(size=(N, D))
    obs = theta + rng.normal(size=(N, D))
    ps = np.sqrt(0.5)
    mu = obs / 2 + shift * ps
    draws = mu[:, None, :] + ps * rng.normal(size=(N, S, D))
    return draws.astype(np.float32), theta.astype(np.float32)
