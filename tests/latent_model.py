"""numpy float64 model of the latent residual summary (csrc/sf_latent.hip, features.latent_summary), written from the
definitions: helper module, no tests in it, no device.

A row of z (N, D) counts if all its D values are finite.  Per dimension u = Phi(z_d) = 0.5 erfc(-z_d / sqrt 2); per row
u_r = F_chi2_D(sum_d z_d^2), the closed forms with y = r^2 / 2
    D = 2m     : 1 - e^-y sum_{k<m} y^k / k!
    D = 2m + 1 : erf(sqrt y) - e^-y sum_{k<m} y^(k+1/2) / Gamma(k + 3/2)
clipped to [0, 1] (1 past y = 700, where the subtracted term is below the smallest double); a value u falls in bin
min(floor(u nb), nb - 1)."""
import math

import numpy as np
from scipy import special


def norm_cdf(z):
    return 0.5 * special.erfc(-np.asarray(z, dtype=np.float64) / np.sqrt(2.0))


def chi2_cdf(r2, D):
    y = np.asarray(r2, dtype=np.float64) / 2.0
    m = D // 2
    big = y > 700.0
    ys = np.where(big, 0.0, y)
    if D % 2 == 0:
        tail = sum(ys ** k / math.factorial(k) for k in range(m))
        u = 1.0 - np.exp(-ys) * tail
    else:
        tail = sum(ys ** (k + 0.5) / math.gamma(k + 1.5) for k in range(m)) if m else 0.0
        u = special.erf(np.sqrt(ys)) - np.exp(-ys) * tail
    return np.where(big, 1.0, np.clip(u, 0.0, 1.0))


def bins_of(u, nb):
    return np.minimum(np.floor(np.asarray(u) * nb), nb - 1).astype(np.int64)


def near_edge(u, nb, tol=1e-9):
    """u * nb within tol of an integer: the bin of such a value may legitimately differ by a rounding.  Not u = 0, 0.5 and 1
    themselves: they come out exactly (z = 0: erfc(0) = 1 and an empty radius; saturation: erfc -> 2, e^-y -> 0) in any
    IEEE arithmetic, so their bins are certain."""
    u = np.asarray(u)
    v = u * nb
    return (np.abs(v - np.rint(v)) <= tol) & (u != 0.0) & (u != 0.5) & (u != 1.0)


def raw_sums(z, num_bins):
    """What the device returns: n, n_bad, psum [4, D], cross [D, D], pit_counts [D, nb], radial_counts [nb]; plus the sums of
    the absolute terms (the scale of the fp64 accumulation error) and the number of rows a bin edge could move."""
    z = np.asarray(z)
    N, D = z.shape
    ok = np.isfinite(z).all(1)
    v = z[ok].astype(np.float64)
    n = int(ok.sum())
    psum = np.stack([(v ** p).sum(0) for p in (1, 2, 3, 4)]) if n else np.zeros((4, D))
    psum_abs = np.stack([(np.abs(v) ** p).sum(0) for p in (1, 2, 3, 4)]) if n else np.zeros((4, D))
    cross = v.T @ v
    cross_abs = np.abs(v).T @ np.abs(v)
    u = norm_cdf(v)
    ur = chi2_cdf((v * v).sum(1), D)
    pit = np.zeros((D, num_bins), np.int64)
    for d in range(D):
        pit[d] = np.bincount(bins_of(u[:, d], num_bins), minlength=num_bins)
    rad = np.bincount(bins_of(ur, num_bins), minlength=num_bins).astype(np.int64)
    edge_rows = int((near_edge(u, num_bins).any(1) | near_edge(ur, num_bins)).sum()) if n else 0
    return {"n": n, "n_bad": int(N - n), "psum": psum, "cross": cross, "pit_counts": pit, "radial_counts": rad,
            "psum_abs": psum_abs, "cross_abs": cross_abs, "edge_rows": edge_rows}


def latent_summary(z, num_bins=100):
    """The dict of features.latent_summary, every statistic straight from the finite rows."""
    z = np.asarray(z)
    D = z.shape[1]
    r = raw_sums(z, num_bins)
    v = z[np.isfinite(z).all(1)].astype(np.float64)
    n = r["n"]
    alpha = np.arange(num_bins + 1) / num_bins
    if n == 0:
        nan = np.full(D, np.nan)
        return {"n": 0, "n_bad": r["n_bad"], "mean": nan, "cov": np.full((D, D), np.nan), "skew": nan, "excess_kurtosis": nan,
                "pit_counts": r["pit_counts"], "radial_counts": r["radial_counts"], "ks": nan, "radial_ks": float("nan"),
                "alpha": alpha, "ecp": np.full(num_bins + 1, np.nan)}
    mean = v.mean(0)
    c = v - mean
    var = (c ** 2).mean(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        skew = (c ** 3).mean(0) / var ** 1.5
        kurt = (c ** 4).mean(0) / var ** 2 - 3.0
    cum = np.concatenate([np.zeros((D, 1)), np.cumsum(r["pit_counts"], 1)], 1) / n
    ecp = np.concatenate([[0.0], np.cumsum(r["radial_counts"])]) / n
    return {"n": n, "n_bad": r["n_bad"], "mean": mean, "cov": c.T @ c / n, "skew": skew, "excess_kurtosis": kurt,
            "pit_counts": r["pit_counts"], "radial_counts": r["radial_counts"], "ks": np.abs(cum - alpha).max(1),
            "radial_ks": float(np.abs(ecp - alpha).max()), "alpha": alpha, "ecp": ecp}
