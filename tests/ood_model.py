"""The out-of-distribution check in numpy -- the model that sf_knn / sf_kde_logsumexp (synference_amd/csrc/sf_ood.hip) and
synference_amd/ood.py are tested against.

TEST INFRASTRUCTURE ONLY.  A fresh statement of what sklearn's LocalOutlierFactor / NearestNeighbors, scipy's gaussian_kde
and pyod's KNN / LOF / KDE compute (the detectors behind ref: src/synference/utils.py:991-1340), written from their
published formulas.

a. ``d2_f32``: the device's squared distance, acc = 0; for c ascending: t = q[c] - b[c]; acc = acc + t * t, every operation
   rounded to float32 on its own (numpy float32 arithmetic does exactly that); a NaN result counts as +inf
b. ``knn_f32``: the k smallest (d2 bits, row) keys per query, ascending; ``exclude_self``: base row self_offset + m is not a
   neighbour of query m
c. everything else in float64 on the same float32 inputs: ``knn_f64`` (distances, neighbours, and the relative gap between the
   k-th and the (k+1)-th squared distance), ``lof_fit`` / ``lof_score`` (sklearn's formulas), ``kde_whiten`` /
   ``kde_logsumexp`` (scipy's Scott factor and kernel covariance; pyod's fixed bandwidth), mahalanobis / hotelling / pca
d. ``detect_outliers`` / ``detect_outliers_pyod``: the reference's thresholds, masks and scores on top of c.

The device selects neighbours on float32 distances.  A row whose float64 gap between the k-th and (k+1)-th squared distance is
below GAP (relative), or one of whose neighbours has such a gap on the base side, could get another neighbour set; a row whose
score lies within the comparison's bound of its threshold could fall on either side.  ``undecidable_*`` list them; the
fixtures are REQUIRED to have at most 5 % of them (tests/test_cpu_ood.py).
"""
from __future__ import annotations

import math

import numpy as np

GAP = 1e-5
RTOL = 1e-5          # scores, device against model
KDE_ATOL = 2e-5      # log-density on the same whitened float32 inputs: v_exp_f32 ((|a| + 2) 2^-23 per term) + ordered fp64 sums
CASES = {"main": (2500, 7, 70, 20), "small": (300, 3, 33, 5)}   # N, C, M, k


def make_case(N, C, M, seed=0):
    """Correlated Gaussian features around magnitude 25; every third query is inflated 3x about the centre."""
    rng = np.random.default_rng(seed)
    A = np.eye(C) + 0.3 * rng.normal(size=(C, C))
    base = 25.0 + 0.5 * rng.normal(size=(N, C)) @ A.T
    infl = np.where(np.arange(M) % 3 == 0, 3.0, 1.0)[:, None]
    query = 25.0 + 0.5 * infl * (rng.normal(size=(M, C)) @ A.T)
    return base.astype(np.float32), query.astype(np.float32)


# ---- a / b: what the kernels compute -------------------------------------------------------------------------------------
def d2_f32(query, base):
    q, b = np.asarray(query, np.float32), np.asarray(base, np.float32)
    acc = np.zeros((len(q), len(b)), np.float32)
    with np.errstate(all="ignore"):
        for c in range(q.shape[1]):
            t = q[:, c, None] - b[None, :, c]
            acc = acc + t * t
    acc[np.isnan(acc)] = np.inf
    return acc


def knn_f32(base, query, k, exclude_self=0, self_offset=0):
    d2 = d2_f32(query, base)
    keys = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(base), dtype=np.uint64)[None, :]
    if exclude_self:
        keys[np.arange(len(query)), self_offset + np.arange(len(query))] = np.uint64(2 ** 64 - 1)
    keys = np.sort(keys, axis=1)[:, :k]
    return (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), (keys & np.uint64(0xFFFFFFFF)).astype(np.int32)


# ---- c: float64 ----------------------------------------------------------------------------------------------------------
def d2_f64(query, base):
    q, b = np.asarray(query, np.float64), np.asarray(base, np.float64)
    return ((q[:, None, :] - b[None, :, :]) ** 2).sum(-1)


def knn_f64(base, query, k, exclude_self=False):
    """-> distances [M,k], rows [M,k], relative gap [M] between the k-th and the (k+1)-th squared distance."""
    d2 = d2_f64(query, base)
    if exclude_self:
        d2[np.arange(len(query)), np.arange(len(query))] = np.inf
    order = np.argsort(d2, axis=1, kind="stable")
    s = np.take_along_axis(d2, order, 1)
    nxt = s[:, k] if s.shape[1] > k else np.full(len(s), np.inf)
    with np.errstate(all="ignore"):
        gap = np.where(np.isfinite(nxt), (nxt - s[:, k - 1]) / np.maximum(nxt, 1e-300), np.inf)
    return np.sqrt(s[:, :k]), order[:, :k], gap


def lof_fit(base, k):
    d, nbr, gap = knn_f64(base, base, k, exclude_self=True)
    k_dist = d[:, -1]
    lrd = 1.0 / (np.maximum(d, k_dist[nbr]).mean(1) + 1e-10)
    nof = -(lrd[nbr] / lrd[:, None]).mean(1)
    return dict(base=np.asarray(base), k=k, k_dist=k_dist, lrd=lrd, nof=nof, gap=gap, nbr=nbr)


def lof_score(fit, query):
    """-> sklearn's score_samples (minus the local outlier factor), and the rows whose neighbour set is fragile."""
    d, nbr, gap = knn_f64(fit["base"], query, fit["k"])
    lrd = 1.0 / (np.maximum(d, fit["k_dist"][nbr]).mean(1) + 1e-10)
    fragile = (gap < GAP) | (fit["gap"][nbr] < GAP).any(1)
    return -(fit["lrd"][nbr] / lrd[:, None]).mean(1), fragile


def kde_whiten(base, query, bandwidth=None, dtype=np.float32):
    """Whitened float32 rows about the base mean and the log of the normalisation: log density = logsumexp - lognorm
    (dtype=np.float64: unrounded, what scipy itself evaluates).
    bandwidth None: scipy.stats.gaussian_kde (Scott factor N^(-1/(C+4)), kernel covariance factor^2 cov); a number: an
    isotropic Gaussian of that width (sklearn KernelDensity, pyod KDE)."""
    b, q = np.asarray(base, np.float64), np.asarray(query, np.float64)
    N, C = b.shape
    mu = b.mean(0)
    if bandwidth is None:
        factor = N ** (-1.0 / (C + 4))
        L = np.linalg.cholesky(np.atleast_2d(np.cov(b.T)) * factor ** 2)
        Li = np.linalg.inv(L)
        lognorm = math.log(N) + np.log(np.diag(L)).sum() + 0.5 * C * math.log(2 * math.pi)
        info = factor
    else:
        Li = np.eye(C) / bandwidth
        lognorm = math.log(N) + C * math.log(bandwidth) + 0.5 * C * math.log(2 * math.pi)
        info = bandwidth
    return ((b - mu) @ Li.T).astype(dtype), ((q - mu) @ Li.T).astype(dtype), lognorm, info


def kde_logsumexp(query_w, base_w):
    a = -0.5 * d2_f64(query_w, base_w)
    mx = a.max(1)
    return mx + np.log(np.exp(a - mx[:, None]).sum(1))


def kde_input_term(query_w, base_w):
    """Bound on what rounding the whitened coordinates to float32 can move a log-density: 4 2^-24 w_max sqrt(C e_min), e_min
    the row's smallest whitened squared distance (the terms that carry the sum lie near it)."""
    C = base_w.shape[1]
    w_max = max(np.abs(base_w).max(), np.abs(query_w).max())
    e_min = d2_f64(query_w, base_w).min(1)
    return 4 * 2.0 ** -24 * w_max * np.sqrt(C * e_min)


def _chi2_ppf(p, df):
    """Quantile of chi-square by bisection on the regularised lower incomplete gamma (series / continued fraction)."""
    def cdf(x):
        a, x = df / 2.0, x / 2.0
        if x <= 0:
            return 0.0
        if x < a + 1:
            term = s = 1.0 / a
            n = a
            for _ in range(10000):
                n += 1
                term *= x / n
                s += term
                if abs(term) < abs(s) * 1e-16:
                    break
            return s * math.exp(-x + a * math.log(x) - math.lgamma(a))
        b = x + 1 - a
        c = 1e300
        d = 1 / b
        h = d
        for i in range(1, 10000):
            an = -i * (i - a)
            b += 2
            d = an * d + b
            d = 1e-300 if abs(d) < 1e-300 else d
            c = b + an / c
            c = 1e-300 if abs(c) < 1e-300 else c
            d = 1 / d
            h *= d * c
            if abs(d * c - 1) < 1e-16:
                break
        return 1 - math.exp(-x + a * math.log(x) - math.lgamma(a)) * h
    lo, hi = 0.0, max(10.0 * df, 100.0)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if cdf(mid) < p else (lo, mid)
    return 0.5 * (lo + hi)


# ---- d: the reference's functions -----------------------------------------------------------------------------------------
def detect_outliers(base, obs, method="mahalanobis", contamination=0.1, n_neighbors=20, threshold=None, confidence=0.95,
                    n_components=None):
    b, o = np.asarray(base, np.float64), np.asarray(obs, np.float64)
    N, C = b.shape
    res = dict(method_info={})
    if method in ("mahalanobis", "hotelling_t2"):
        mean, cov = b.mean(0), np.atleast_2d(np.cov(b.T))
        diff = o - mean
        m2 = np.sum(diff @ np.linalg.inv(cov) * diff, axis=1)
        if method == "mahalanobis":
            thr = math.sqrt(_chi2_ppf(confidence, C)) if threshold is None else threshold
            sc = np.sqrt(m2)
        else:
            sc = m2 * N * (N - C) / ((N - 1) * C)
            thr = threshold          # the F quantile needs scipy: tests/test_cpu_ood.py passes it in
        res.update(scores=sc, outlier_mask=sc > thr, threshold_used=thr)
    elif method == "pca":
        nc = min(C, N - 1) if n_components is None else n_components
        mean = b.mean(0)
        _, _, Vt = np.linalg.svd(b - mean, full_matrices=False)
        V = Vt[:nc].T

        def err(x):
            r = (x - mean) - (x - mean) @ V @ V.T
            return (r ** 2).sum(1)
        thr = np.percentile(err(b), confidence * 100) if threshold is None else threshold
        res.update(scores=err(o), outlier_mask=err(o) > thr, threshold_used=thr)
    elif method == "kde":
        bw, qw, lognorm, factor = kde_whiten(base, obs)
        dens = np.exp(kde_logsumexp(qw, bw) - lognorm)
        thr = np.percentile(np.exp(kde_logsumexp(bw, bw) - lognorm), (1 - confidence) * 100) if threshold is None else threshold
        res.update(scores=-np.log(dens + 1e-10), outlier_mask=dens < thr, threshold_used=thr,
                   method_info={"kde_bandwidth": factor}, density=dens)
    elif method == "lof":
        fit = lof_fit(base, n_neighbors)
        offset = np.percentile(fit["nof"], 100.0 * contamination)
        ss, fragile = lof_score(fit, obs)
        dec = ss - offset
        res.update(scores=-dec, outlier_mask=dec < 0, threshold_used=0, fragile=fragile, offset=offset, decision=dec)
    else:
        raise ValueError(method)
    return res


def pyod_scores(base, obs, method, contamination=0.1, n_neighbors=None, bandwidth=1.0):
    """-> (scores of obs, threshold_, fragile rows)"""
    if method == "knn":
        k = 5 if n_neighbors is None else n_neighbors
        dtr, _, gtr = knn_f64(base, base, k, exclude_self=True)
        d, _, _ = knn_f64(base, obs, k)
        train, sc, fragile = dtr[:, -1], d[:, -1], np.zeros(len(obs), bool)   # the k-th distance itself is not fragile
    elif method == "lof":
        k = 20 if n_neighbors is None else n_neighbors
        fit = lof_fit(base, k)
        ss, fragile = lof_score(fit, obs)
        train, sc = -fit["nof"], -ss
    elif method == "kde":
        bw, qw, lognorm, _ = kde_whiten(base, obs, bandwidth)
        train, sc = lognorm - kde_logsumexp(bw, bw), lognorm - kde_logsumexp(qw, bw)
        fragile = np.zeros(len(obs), bool)
    else:
        raise ValueError(method)
    return sc, np.percentile(train, 100.0 * (1.0 - contamination)), fragile


def combine(masks, combination):
    masks = np.asarray(masks, bool)
    if combination == "majority":
        return masks.sum(1) >= masks.shape[1] / 2
    if combination == "any":
        return masks.any(1)
    if combination == "all":
        return masks.all(1)
    if combination == "none":
        return masks
    raise ValueError(combination)


def undecidable(scores, threshold, fragile, bound):
    """Rows the device may legitimately decide the other way: a fragile neighbour set, or a score within `bound` (absolute)
    of the threshold."""
    return np.asarray(fragile, bool) | (np.abs(np.asarray(scores) - threshold) <= bound)


def fixture_undecidable(base, query, method, k, contamination=0.1, confidence=0.95, pyod=False, n_components=None, threshold=None):
    """Rows of a fixture whose mask the device may decide the other way (module docstring): bool [M]."""
    if pyod:
        sc, thr, fragile = pyod_scores(base, query, method, contamination, n_neighbors=k)
        if method == "kde":
            bw, qw, _, _ = kde_whiten(base, query, 1.0)
            return undecidable(sc, thr, fragile, 2 * KDE_ATOL + kde_input_term(qw, bw))
        return undecidable(sc, thr, fragile, RTOL * (np.abs(sc) + abs(thr)))
    r = detect_outliers(base, query, method, contamination=contamination, n_neighbors=k, confidence=confidence,
                        n_components=n_components, threshold=threshold)
    if method == "lof":
        return undecidable(r["decision"], 0.0, r["fragile"], RTOL * (np.abs(r["decision"] + r["offset"]) + abs(r["offset"])))
    if method == "kde":
        bw, qw, _, _ = kde_whiten(base, query)
        return undecidable(np.log(r["density"]), math.log(r["threshold_used"]), False, 2 * KDE_ATOL + kde_input_term(qw, bw))
    return undecidable(r["scores"], r["threshold_used"], False, RTOL * (np.abs(r["scores"]) + abs(r["threshold_used"])))
