"""Out-of-distribution check on the device: is a set of observed rows inside the distribution of a base (training) set?

``detect_outliers`` and ``detect_outliers_pyod`` carry the names, defaults, return values and combination rules of the
reference (ref: src/synference/utils.py:991-1340); ``SBI_Fitter.test_in_distribution`` / ``test_in_distribution_pyod`` and
``fit_catalogue(check_out_of_distribution=True)`` sit on them.  The all-pairs work -- every observation against every base
row, and the base against itself -- is two HIP kernels (csrc/sf_ood.hip): ``sf_knn`` (exact brute-force neighbours, ordered by
(distance bits, row)) and ``sf_kde_logsumexp`` (log of a Gaussian kernel sum over whitened rows).  Everything around them is
small: mean, covariance, Cholesky, eigen-decomposition, percentiles and gathers over [N, k] arrays, torch on the device in
float64.  The detectors are restated from their published formulas:

* ``lof``: sklearn.neighbors.LocalOutlierFactor(novelty=True); ``kde``: scipy.stats.gaussian_kde (Scott factor);
  ``mahalanobis``, ``hotelling_t2``, ``pca`` as the reference writes them;
* pyod's ``knn`` (distance to the 5th neighbour), ``lof`` (n_neighbors=20) and ``kde`` (bandwidth 1.0), each with
  ``threshold_ = percentile(training scores, 100 (1 - contamination))``.  [UPSTREAM], unpinned: pyod cannot be run beside this.

Other method names raise ``ValueError`` that lists what exists.  There is no CPU path: the kernels are the product.

``FittedBase`` keeps the base side -- the device copy, its own neighbours, k-distances, reachability densities, thresholds and
whitening matrices -- so that a second catalogue against the same library pays only M x N.
"""
from __future__ import annotations

import logging
import math
from typing import Any, Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _ptr

logger = logging.getLogger("synference_amd")

METHODS = ("mahalanobis", "hotelling_t2", "pca", "kde", "lof")
NOT_BUILT = ("robust_mahalanobis", "isolation_forest", "one_class_svm")
PYOD_METHODS = ("knn", "lof", "kde")
COMBINATIONS = ("majority", "any", "all", "none")
KMAX, CMAX = 64, 64


# ---- the two kernels ------------------------------------------------------------------------------------------------------
def knn(base: torch.Tensor, query: torch.Tensor, k: int, exclude_self: bool = False, self_offset: int = 0):
    """The k nearest rows of ``base`` [N, C] for every row of ``query`` [M, C] (float32 device tensors): squared distances
    [M, k] float32 ascending and rows [M, k] int32; ties go to the lowest row."""
    if not (base.is_cuda and query.is_cuda):
        raise RuntimeError("the neighbour search runs on the GPU (sf_knn); there is no CPU fallback")
    base, query = base.contiguous(), query.contiguous()
    M = query.shape[0]
    d2 = torch.empty((M, k), dtype=torch.float32, device=base.device)
    idx = torch.empty((M, k), dtype=torch.int32, device=base.device)
    with torch.cuda.device(base.device):
        st = _lib.stream_ptr(base.device)
        _lib.check(_lib.load().sf_knn(_ptr(base), base.shape[0], base.shape[1], _ptr(query), M, int(k), int(bool(exclude_self)),
                                      int(self_offset), _ptr(d2), _ptr(idx), st))
    return d2, idx


def kde_logsumexp(base_w: torch.Tensor, query_w: torch.Tensor) -> torch.Tensor:
    """log sum_i exp(-|query_w[m] - base_w[i]|^2 / 2), float64 [M], over whitened float32 device rows."""
    if not (base_w.is_cuda and query_w.is_cuda):
        raise RuntimeError("the kernel sum runs on the GPU (sf_kde_logsumexp); there is no CPU fallback")
    base_w, query_w = base_w.contiguous(), query_w.contiguous()
    out = torch.empty((query_w.shape[0],), dtype=torch.float64, device=base_w.device)
    with torch.cuda.device(base_w.device):
        st = _lib.stream_ptr(base_w.device)
        _lib.check(_lib.load().sf_kde_logsumexp(_ptr(base_w), base_w.shape[0], base_w.shape[1], _ptr(query_w),
                                                query_w.shape[0], _ptr(out), st))
    return out


# ---- quantiles of chi-square and F (the thresholds of mahalanobis / hotelling_t2) ----------------------------------------
def _betacf(a, b, x):
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    d = 1e-300 if abs(d) < 1e-300 else d
    d = 1.0 / d
    h = d
    for m in range(1, 1000):
        m2 = 2 * m
        for aa in (m * (b - m) * x / ((qam + m2) * (a + m2)), -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))):
            d = 1.0 + aa * d
            d = 1e-300 if abs(d) < 1e-300 else d
            c = 1.0 + aa / c
            c = 1e-300 if abs(c) < 1e-300 else c
            d = 1.0 / d
            h *= d * c
        if abs(d * c - 1.0) < 1e-16:
            break
    return h


def _betainc(a, b, x):
    if x <= 0.0 or x >= 1.0:
        return 0.0 if x <= 0.0 else 1.0
    bt = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x))
    return bt * _betacf(a, b, x) / a if x < (a + 1.0) / (a + b + 2.0) else 1.0 - bt * _betacf(b, a, 1.0 - x) / b


def _bisect(cdf, p, hi):
    lo = 0.0
    while cdf(hi) < p:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if cdf(mid) < p else (lo, mid)
    return 0.5 * (lo + hi)


def chi2_ppf(p: float, df: float) -> float:
    a = torch.tensor(df / 2.0, dtype=torch.float64)
    return _bisect(lambda x: float(torch.special.gammainc(a, torch.tensor(x / 2.0, dtype=torch.float64))), p, max(4.0 * df, 16.0))


def f_ppf(p: float, d1: float, d2: float) -> float:
    return _bisect(lambda x: _betainc(d1 / 2.0, d2 / 2.0, d1 * x / (d1 * x + d2)), p, 16.0)


# ---- the base side ----------------------------------------------------------------------------------------------------------
def _device(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("the out-of-distribution check runs on the GPU (sf_knn, sf_kde_logsumexp); there is no CPU fallback")
    return torch.device(device if device is not None and str(device).startswith("cuda") else "cuda")


def _rows(x, dev) -> torch.Tensor:
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    if t.dim() != 2:
        raise ValueError("need a two-dimensional array (rows, features)")
    return t.to(device=dev, dtype=torch.float32).contiguous()


def _percentile(x: torch.Tensor, q: float) -> float:
    """np.percentile(x, q) (linear interpolation) on the device in float64."""
    s = torch.sort(x.double().reshape(-1)).values
    pos = (s.numel() - 1) * (q / 100.0)
    lo = int(math.floor(pos))
    hi = min(lo + 1, s.numel() - 1)
    a, b = float(s[lo]), float(s[hi])
    return a + (b - a) * (pos - lo)


class FittedBase:
    """The base side of the detectors, computed on first use and kept."""

    def __init__(self, base_distribution, device=None):
        self.x = _rows(base_distribution, _device(device))
        self.N, self.C = self.x.shape
        if self.C > CMAX:
            raise ValueError(f"the device kernels take at most {CMAX} features")
        self._cache: Dict[Any, Any] = {}

    def _get(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def moments(self):
        def make():
            x = self.x.double()
            mean = x.mean(0)
            cov = torch.atleast_2d(torch.cov(x.T))
            try:
                inv = torch.linalg.inv(cov)
            except RuntimeError:
                inv = torch.linalg.pinv(cov)
            return mean, cov, inv
        return self._get("moments", make)

    def _check_k(self, k, exclude_self):
        if not 1 <= k <= KMAX:
            raise ValueError(f"n_neighbors must lie in [1, {KMAX}] on the device path")
        if k > self.N - int(exclude_self):
            raise ValueError(f"n_neighbors = {k} needs more than {k - 1 + int(exclude_self)} base rows")

    def self_knn(self, k):
        """Distances [N, k] float64 and rows [N, k] int64 of every base row's neighbours among the others."""
        def make():
            self._check_k(k, True)
            d2, idx = knn(self.x, self.x, k, exclude_self=True)
            return d2.double().sqrt(), idx.long()
        return self._get(("knn", k), make)

    def query_knn(self, obs, k):
        self._check_k(k, False)
        d2, idx = knn(self.x, obs, k)
        return d2.double().sqrt(), idx.long()

    def lof(self, k):
        def make():
            d, nbr = self.self_knn(k)
            k_dist = d[:, -1].contiguous()
            lrd = 1.0 / (torch.maximum(d, k_dist[nbr]).mean(1) + 1e-10)
            nof = -(lrd[nbr] / lrd[:, None]).mean(1)
            return dict(k_dist=k_dist, lrd=lrd, nof=nof)
        return self._get(("lof", k), make)

    def lof_score(self, obs, k):
        """sklearn's score_samples: minus the local outlier factor of every observation."""
        f = self.lof(k)
        d, nbr = self.query_knn(obs, k)
        lrd = 1.0 / (torch.maximum(d, f["k_dist"][nbr]).mean(1) + 1e-10)
        return -(f["lrd"][nbr] / lrd[:, None]).mean(1)

    def kde(self, bandwidth=None):
        """Whitening about the base mean (float64), the whitened base (float32), the log normalisation and the base's own
        log-densities.  bandwidth None: gaussian_kde's Scott factor and kernel covariance; a number: isotropic."""
        def make():
            mean, cov, _ = self.moments()
            N, Cn = self.N, self.C
            if bandwidth is None:
                factor = N ** (-1.0 / (Cn + 4))
                L = torch.linalg.cholesky(cov * factor ** 2)
                Li = torch.linalg.inv(L)
                lognorm = math.log(N) + float(torch.log(torch.diagonal(L)).sum()) + 0.5 * Cn * math.log(2 * math.pi)
                info = factor
            else:
                if not bandwidth > 0:
                    raise ValueError("bandwidth must be positive")
                Li = torch.eye(Cn, dtype=torch.float64, device=self.x.device) / float(bandwidth)
                lognorm = math.log(N) + Cn * math.log(bandwidth) + 0.5 * Cn * math.log(2 * math.pi)
                info = float(bandwidth)
            bw = ((self.x.double() - mean) @ Li.T).float().contiguous()
            return dict(mean=mean, Li=Li, base_w=bw, lognorm=lognorm, info=info, train_logdens=kde_logsumexp(bw, bw) - lognorm)
        return self._get(("kde", bandwidth), make)

    def kde_logdens(self, obs, bandwidth=None):
        f = self.kde(bandwidth)
        qw = ((obs.double() - f["mean"]) @ f["Li"].T).float().contiguous()
        return kde_logsumexp(f["base_w"], qw) - f["lognorm"]

    def pca(self, n_components):
        def make():
            mean = self.moments()[0]
            _, S, Vt = torch.linalg.svd(self.x.double() - mean, full_matrices=False)
            var = S ** 2 / (self.N - 1)
            return mean, Vt[:n_components].T.contiguous(), (var / var.sum())[:n_components]
        return self._get(("pca", n_components), make)


def _as_base(base_distribution, device=None) -> FittedBase:
    return base_distribution if isinstance(base_distribution, FittedBase) else FittedBase(base_distribution, device)


# ---- the reference's two functions -----------------------------------------------------------------------------------------
def _validate(method, n_features_base, n_features_obs):
    if method in NOT_BUILT:
        raise ValueError(f"method '{method}' is not built on the HIP path (DESIGN.md section 7); available: {list(METHODS)}")
    if method not in METHODS:
        raise ValueError(f"Unknown method: {method}; available: {list(METHODS)}")
    if n_features_base != n_features_obs:
        raise ValueError("Base distribution and observations must have same number of features")


def _shape(x):
    s = tuple(x.x.shape) if isinstance(x, FittedBase) else tuple(x.shape) if hasattr(x, "shape") else np.asarray(x).shape
    if len(s) != 2:
        raise ValueError("need a two-dimensional array (rows, features)")
    return s


def detect_outliers(base_distribution, observations, method="mahalanobis", contamination=0.1, n_neighbors=20, threshold=None,
                    confidence=0.95, n_components=None, plot=True, **kwargs) -> Dict[str, Any]:
    """ref utils.py:1085-1340.  ``base_distribution``: an array, a device tensor or a ``FittedBase``; ``device=`` picks the
    GPU.  Returns ``outlier_mask``, ``scores`` (numpy), ``threshold_used`` and ``method_info``."""
    _validate(method, _shape(base_distribution)[1], _shape(observations)[1])
    if plot:
        logger.info("detect_outliers: plot=True is skipped on the HIP path (plotting is out of scope)")
    fb = _as_base(base_distribution, kwargs.get("device"))
    obs = _rows(observations, fb.x.device)
    N, Cn = fb.N, fb.C
    info: Dict[str, Any] = {}
    if method in ("mahalanobis", "hotelling_t2"):
        mean, cov, inv = fb.moments()
        diff = obs.double() - mean
        m2 = (diff @ inv * diff).sum(1)
        if method == "mahalanobis":
            scores = m2.sqrt()
            if threshold is None:
                threshold = math.sqrt(chi2_ppf(confidence, Cn))
            info = {"mean": mean.cpu().numpy(), "covariance": cov.cpu().numpy()}
        else:
            scores = m2 * N * (N - Cn) / ((N - 1) * Cn)
            if threshold is None:
                threshold = f_ppf(confidence, Cn, N - Cn)
            info = {"n_base_samples": N, "degrees_of_freedom": (Cn, N - Cn)}
        mask = scores > threshold
    elif method == "pca":
        if n_components is None:
            n_components = min(Cn, N - 1)
        mean, V, evr = fb.pca(n_components)

        def err(x):
            c = x.double() - mean
            return ((c - c @ V @ V.T) ** 2).sum(1)
        scores = err(obs)
        if threshold is None:
            threshold = fb._get(("pca_thr", n_components, confidence), lambda: _percentile(err(fb.x), confidence * 100))
        mask = scores > threshold
        info = {"n_components": n_components, "explained_variance_ratio": evr.cpu().numpy()}
    elif method == "kde":
        f = fb.kde(None)
        dens = torch.exp(fb.kde_logdens(obs, None))
        if threshold is None:
            threshold = fb._get(("kde_thr", confidence),
                                lambda: _percentile(torch.exp(f["train_logdens"]), (1 - confidence) * 100))
        scores = -torch.log(dens + 1e-10)
        mask = dens < threshold
        info = {"kde_bandwidth": f["info"]}
    else:   # lof
        offset = fb._get(("lof_off", n_neighbors, contamination),
                         lambda: _percentile(fb.lof(n_neighbors)["nof"], 100.0 * contamination))
        dec = fb.lof_score(obs, n_neighbors) - offset
        scores, mask, threshold = -dec, dec < 0, 0
        info = {"n_neighbors": n_neighbors}
    return {"outlier_mask": mask.cpu().numpy(), "scores": scores.cpu().numpy(), "threshold_used": threshold, "method_info": info}


def _validate_pyod(methods, combination):
    if isinstance(methods, str):
        methods = [methods]
    methods = list(methods)
    for m in methods:
        if str(m).lower() not in PYOD_METHODS:
            raise ValueError(f"Method {m} is not recognized on the HIP path; available pyod methods: {list(PYOD_METHODS)}")
    if combination not in COMBINATIONS:
        raise ValueError("Combination method must be 'majority', 'any', 'all' or 'none'.")
    return [str(m).lower() for m in methods]


def detect_outliers_pyod(base_distribution, observations, methods=("knn", "lof", "kde"), combination="majority",
                         return_scores=False, **kwargs):
    """ref utils.py:991-1082 for pyod's KNN, LOF and KDE (``methods`` defaults to the three that exist here; the reference's
    default, ecod, does not).  ``contamination`` [0.1], ``n_neighbors`` and ``bandwidth`` reach the methods that take them."""
    methods = _validate_pyod(methods, combination)
    if _shape(base_distribution)[1] != _shape(observations)[1]:
        raise ValueError("Base distribution and observations must have same number of features")
    kwargs = dict(kwargs)
    device = kwargs.pop("device", None)
    contamination = float(kwargs.pop("contamination", 0.1))
    n_neighbors = kwargs.pop("n_neighbors", None)
    bandwidth = float(kwargs.pop("bandwidth", 1.0))
    if kwargs:
        raise ValueError(f"unknown keyword argument(s) {sorted(kwargs)} for the pyod methods {list(PYOD_METHODS)}")
    if not 0.0 < contamination <= 0.5:
        raise ValueError("contamination must be in (0, 0.5]")
    fb = _as_base(base_distribution, device)
    obs = _rows(observations, fb.x.device)
    masks, scores = [], []
    for m in methods:
        if m == "knn":
            k = 5 if n_neighbors is None else int(n_neighbors)
            train = lambda: fb.self_knn(k)[0][:, -1]
            sc = fb.query_knn(obs, k)[0][:, -1]
        elif m == "lof":
            k = 20 if n_neighbors is None else int(n_neighbors)
            train = lambda: -fb.lof(k)["nof"]
            sc = -fb.lof_score(obs, k)
        else:
            k = bandwidth
            train = lambda: -fb.kde(bandwidth)["train_logdens"]
            sc = -fb.kde_logdens(obs, bandwidth)
        thr = fb._get(("pyod_thr", m, k, contamination), lambda: _percentile(train(), 100.0 * (1.0 - contamination)))
        masks.append((sc > thr).cpu().numpy())
        scores.append(sc.cpu().numpy())
    outlier_mask = np.stack(masks, 1)
    if combination == "majority":
        final = outlier_mask.sum(1) >= len(methods) / 2
    elif combination == "any":
        final = outlier_mask.any(1)
    elif combination == "all":
        final = outlier_mask.all(1)
    else:
        final = outlier_mask
    if return_scores:
        return {"outlier_mask": final, "scores": np.stack(scores, 1)}
    return final
