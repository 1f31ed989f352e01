"""Model misspecification tests on the device (Schmitt et al. 2023): is the observed catalogue AS A WHOLE a plausible draw from
the simulator?  Two tests carry the names, argument order and return values of ``sbi.diagnostics.misspecification``
([UPSTREAM], restated from its published source, unpinned: sbi cannot be run beside this):

* ``calc_misspecification_mmd``: a permutation test on the unbiased MMD^2 (Gaussian kernel) between the observed rows and the
  training rows, in z-scored feature space or in the summary space of a posterior's embedding net;
* ``calc_misspecification_logprob``: where does ``log p(x_o)`` fall among ``log p(x_train)`` under an unconditional flow of
  the training features (``MarginalTrainer`` -> ``MarginalEstimator``: the existing flow engine, the features as "theta" and one
  constant zero context column).

The all-pairs work of the MMD test is two HIP kernels (csrc/sf_mmd.hip).  With ``k(a, b) = exp2(d2(a, b) c2)``,
``r_i = sum_{j != i} k(z_i, z_j)`` over the N training rows and ``R = sum_i r_i``, shuffle ``s`` -- a keyed subset ``S_s`` of M
training rows against its complement -- needs only the M x M block:

    A_s = sum_{a != b in S_s} k,   Cx_s = sum_{i in S_s} r_i - A_s,   B_s = R - A_s - 2 Cx_s
    mmd2 = A / (m (m - 1)) + B / (n (n - 1)) - 2 Cx / (m n)

so the whole null costs one N x N pass (``sf_rbf_rowsum``) and ``n_shuffle`` M x M passes (``sf_rbf_subset_sums``), where the
upstream loop evaluates all N x N pairs again for every shuffle.  ``p_value = mean(null_mmd2 > mmd2)`` on the UNCLAMPED squares
(about half of the null's unbiased squares are negative); the values handed back under sbi's names are ``sqrt(max(0, .))``.
Where ``mmd2 > 0`` the two conventions agree.  The bandwidth is computed once (upstream: per call).  There is no CPU path.

Subsets: ``mmd_subsets`` -- the first ``m`` positions of a keyed bijection of [0, N), the Feistel network of
``lc2st.keyed_order`` with round keys ``philox4x32_10((s, 0, 0, 0), (seed_lo, seed_hi ^ STREAM_MMD))``.  Set ``2^31 - 1`` orders
the rows the bandwidth looks at, set ``2^31 - 2`` the ``max_train`` subsample.
"""
from __future__ import annotations

import ctypes as C
import logging
import math
from typing import Any, Dict, Optional

import numpy as np

from .lc2st import _mix, _philox

logger = logging.getLogger("synference_amd")

STREAM_MMD = 0x4D4D4400
SET_SCALE, SET_TRAIN = 2 ** 31 - 1, 2 ** 31 - 2
CMAX, SCALE_ROWS = 64, 2048
MAX_F = 16                       # the flow engine's D <= 16
INDEX_BYTES = 64 << 20           # index chunk handed to one sf_rbf_subset_sums call
MODES, METHODS = ("x_space", "embedding"), ("logprob", "mmd")
LOG2E = 1.4426950408889634


# ---- keyed subsets ----------------------------------------------------------------------------------------------------------
def _half_bits(N: int) -> int:
    hb = 1
    while (1 << (2 * hb)) < N:
        hb += 1
    return hb


def _set_keys(seed: int, sets) -> np.ndarray:
    """uint32 [4, n]: the Feistel round keys of the sets numbered ``sets``."""
    sets = np.asarray(sets, dtype=np.uint32).reshape(-1)
    return np.stack(_philox(sets, 0, 0, 0, int(seed) & (2 ** 64 - 1), STREAM_MMD))


def mmd_subsets(seed: int, n_shuffle: int, N: int, m: int, first: int = 0) -> np.ndarray:
    """int32 [n_shuffle, m]: row ``s`` is the subset of shuffle ``first + s`` -- the images of positions 0 .. m - 1 under that
    shuffle's keyed bijection of [0, N): four Feistel rounds on 2 hb bits (4^hb >= N), values outside [0, N) walked through the
    bijection again.  Only these m positions are computed.  This function is the definition."""
    if not 1 <= m <= N or N >= 2 ** 31:
        raise ValueError("need 1 <= m <= N < 2^31")
    key = _set_keys(seed, first + np.arange(n_shuffle, dtype=np.int64))[:, :, None]       # [4, n, 1]
    hb = _half_bits(N)
    mask, hbu = np.uint32((1 << hb) - 1), np.uint32(hb)
    x = np.broadcast_to(np.arange(m, dtype=np.uint32), (n_shuffle, m)).copy()
    todo = np.ones(x.shape, dtype=bool)
    with np.errstate(over="ignore"):
        while todo.any():
            L, R = x >> hbu, x & mask
            for r in range(4):
                L, R = R, L ^ (_mix(R ^ key[r]) & mask)
            x = np.where(todo, (L << hbu) | R, x)
            todo = x >= N
    return x.astype(np.int32)


def _subsets_device(seed: int, first: int, n_sets: int, N: int, m: int, device):
    """``mmd_subsets`` in torch integer arithmetic on ``device`` (int64 words masked to 32 bits): int32 [n_sets, m]."""
    import torch
    key = torch.as_tensor(_set_keys(seed, first + np.arange(n_sets, dtype=np.int64)).astype(np.int64)).to(device)[:, :, None]
    hb = _half_bits(N)
    mask, M32 = (1 << hb) - 1, 0xFFFFFFFF

    def mix(u):
        u = u ^ (u >> 16)
        u = (u * 0x7FEB352D) & M32
        u = u ^ (u >> 15)
        u = (u * 0x846CA68B) & M32        # (a product past 2^63 wraps: its low 32 bits are still the product's)
        return u ^ (u >> 16)

    x = torch.arange(m, dtype=torch.int64, device=device).expand(n_sets, m).clone()
    todo = torch.ones_like(x, dtype=torch.bool)
    while bool(todo.any()):
        L, R = x >> hb, x & mask
        for r in range(4):
            L, R = R, L ^ (mix(R ^ key[r]) & mask)
        x = torch.where(todo, (L << hb) | R, x)
        todo = x >= N
    return x.to(torch.int32).contiguous()


# ---- the two kernels --------------------------------------------------------------------------------------------------------
def _need_gpu(what: str):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(f"{what} runs on the GPU (sf_rbf_rowsum, sf_rbf_subset_sums, the flow engine); there is no CPU fallback")
    return torch


def c2_of(scale: float) -> float:
    """The exponent factor of the kernels, k = exp2(d2 c2): -0.5 / scale^2 log2(e), computed in double and rounded once."""
    if not (scale > 0 and math.isfinite(scale)):
        raise ValueError("scale must be positive and finite")
    return float(np.float32(-0.5 / (float(scale) * float(scale)) * LOG2E))


def rbf_rowsum(base, query, c2: float, exclude_self: bool = False, self_offset: int = 0):
    """float64 [M]: sum_i exp2(d2(query[q], base[i]) c2) over float32 device rows; ``exclude_self``: base row self_offset + q is
    skipped (by position)."""
    if not (getattr(base, "is_cuda", False) and getattr(query, "is_cuda", False)):
        raise RuntimeError("the kernel row sums run on the GPU (sf_rbf_rowsum); there is no CPU fallback")
    import torch
    from . import _lib
    if base.dtype != torch.float32 or query.dtype != torch.float32 or base.dim() != 2 or query.dim() != 2 or \
            base.shape[1] != query.shape[1]:
        raise ValueError("base and query must be float32 tensors (rows, features) with the same number of features")
    base, query = base.contiguous(), query.contiguous()
    out = torch.empty((query.shape[0],), dtype=torch.float64, device=base.device)
    with torch.cuda.device(base.device):
        _lib.check(_lib.load().sf_rbf_rowsum(_lib.ptr(base), base.shape[0], base.shape[1], _lib.ptr(query), query.shape[0],
                                             C.c_float(c2), int(bool(exclude_self)), int(self_offset), _lib.ptr(out),
                                             _lib.stream_ptr(base.device)))
    return out


def rbf_subset_sums(rows, idx, c2: float, rowsum=None, check: bool = True):
    """``pair_sum`` float64 [n_sets] = sum over positions a != b of k(rows[idx[s, a]], rows[idx[s, b]]) and, with ``rowsum``
    (float64 [N]), ``picked_rowsum`` [n_sets] = sum_a rowsum[idx[s, a]]; ``idx`` int32 [n_sets, m] on the device, entries inside
    [0, N) (``check``) and distinct within a set (the caller's contract)."""
    if not (getattr(rows, "is_cuda", False) and getattr(idx, "is_cuda", False)):
        raise RuntimeError("the subset kernel sums run on the GPU (sf_rbf_subset_sums); there is no CPU fallback")
    import torch
    from . import _lib
    if idx.dim() != 2 or idx.dtype != torch.int32:
        raise ValueError("idx must be an int32 tensor of shape (n_sets, m)")
    if rows.dim() != 2 or rows.dtype != torch.float32:
        raise ValueError("rows must be a float32 tensor (rows, features)")
    rows, idx = rows.contiguous(), idx.contiguous()
    n_sets, m = idx.shape
    if check and idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= rows.shape[0]):
        raise ValueError(f"idx holds entries outside [0, {rows.shape[0]})")
    pair = torch.empty((n_sets,), dtype=torch.float64, device=rows.device)
    picked = torch.empty((n_sets,), dtype=torch.float64, device=rows.device) if rowsum is not None else None
    if rowsum is not None:
        rowsum = rowsum.to(device=rows.device, dtype=torch.float64).contiguous()
        if rowsum.shape != (rows.shape[0],):
            raise ValueError("rowsum must have one entry per row")
    with torch.cuda.device(rows.device):
        _lib.check(_lib.load().sf_rbf_subset_sums(_lib.ptr(rows), rows.shape[0], rows.shape[1], _lib.ptr(idx), n_sets, m,
                                                  C.c_float(c2), _lib.ptr(rowsum), _lib.ptr(pair), _lib.ptr(picked),
                                                  _lib.stream_ptr(rows.device)))
    return (pair, picked) if rowsum is not None else pair


# ---- the statistic ----------------------------------------------------------------------------------------------------------
def _as_rows(a, name: str) -> np.ndarray:
    import torch
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if a.ndim != 2:
        raise ValueError(f"{name} must be two-dimensional (rows, features), got shape {tuple(a.shape)}")
    a = np.ascontiguousarray(a, dtype=np.float32)
    if not np.isfinite(a).all():
        raise ValueError(f"{name} holds non-finite values: the misspecification tests take finite rows")
    return a


def rbf_scale(z, seed: int = 0) -> float:
    """The median heuristic: ``numpy.median`` of the Euclidean distances (float64) over all pairs i < j of the first
    min(N, 2048) rows of the keyed order (set 2^31 - 1) of ``z``.  Array or tensor; computed where ``z`` lives."""
    import torch
    t = z if torch.is_tensor(z) else torch.tensor(np.asarray(z))
    if t.dim() != 2 or t.shape[0] < 2:
        raise ValueError("need at least two rows (rows, features)")
    N = t.shape[0]
    n = min(N, SCALE_ROWS)
    pick = torch.as_tensor(mmd_subsets(seed, 1, N, n, first=SET_SCALE)[0].astype(np.int64)).to(t.device)
    a = t[pick].double()
    d = torch.cdist(a, a, compute_mode="donot_use_mm_for_euclid_dist")
    iu = torch.triu_indices(n, n, offset=1, device=t.device)
    v = torch.sort(d[iu[0], iu[1]]).values
    k = v.numel()
    return float(v[k // 2]) if k % 2 else 0.5 * (float(v[k // 2 - 1]) + float(v[k // 2]))


def mmd2_unbiased(x, y, scale: float) -> float:
    """The unbiased MMD^2 (Gaussian kernel of width ``scale``) of two sets of float32 device rows."""
    if not (getattr(x, "is_cuda", False) and getattr(y, "is_cuda", False)):
        raise RuntimeError("the MMD runs on the GPU (sf_rbf_rowsum); there is no CPU fallback")
    m, n = x.shape[0], y.shape[0]
    if m < 2 or n < 2 or x.shape[1] != y.shape[1] or x.shape[1] > CMAX:
        raise ValueError(f"need two sets of at least 2 rows with the same number (<= {CMAX}) of features")
    c2 = c2_of(scale)
    A = float(rbf_rowsum(x, x, c2, exclude_self=True).sum())
    B = float(rbf_rowsum(y, y, c2, exclude_self=True).sum())
    Cx = float(rbf_rowsum(y, x, c2).sum())
    return A / (m * (m - 1)) + B / (n * (n - 1)) - 2.0 * Cx / (m * n)


def null_mmd2(A, picked, R: float, N: int, M: int):
    """The null's MMD^2 from the subset sums (module docstring); arrays or tensors, float64."""
    n = N - M
    Cx = picked - A
    B = R - A - 2.0 * Cx
    return A / (M * (M - 1)) + B / (n * (n - 1)) - 2.0 * Cx / (M * n)


def _estimator_of(inference):
    """The ``FlowEstimator`` behind a posterior, an ensemble (member 0) or an estimator itself."""
    obj = inference
    if hasattr(obj, "posteriors") and not hasattr(obj, "posterior_estimator"):
        obj = obj.posteriors[0]
    obj = getattr(obj, "posterior_estimator", obj)
    if not hasattr(obj, "embed"):
        raise ValueError("mode='embedding' needs a posterior or a FlowEstimator (something with .embed) as `inference`")
    return obj


def calc_misspecification_mmd(inference, x_obs, x, mode: str = "x_space", n_shuffle: int = 1000, *,
                              scale: Optional[float] = None, z_score: bool = True, max_train: Optional[int] = None,
                              seed: int = 0, alpha: float = 0.05, return_details: bool = False, device=None):
    """sbi's ``calc_misspecification_mmd``: ``(p_value, (mmds_baseline, mmd))`` of the observed rows ``x_obs`` (M, C) against the
    training rows ``x`` (N, C); M >= 2, N >= M + 2, at most 64 columns after the embedding.  ``mode="x_space"``: both z-scored
    with the training rows' mean and unbiased std (clamped at 1e-7; ``z_score=False`` skips it); ``mode="embedding"``: both
    through ``FlowEstimator.embed`` of ``inference`` (a posterior, an ensemble -- member 0 -- or an estimator).  ``scale`` None:
    ``rbf_scale`` of the transformed training rows, once.  ``max_train`` keeps a keyed subsample of the training rows.
    ``return_details``: a dict that adds ``mmd2``, ``null_mmd2``, ``scale`` and ``reject`` (p_value < alpha)."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {list(MODES)}, got {mode!r}")
    est = None
    if mode == "embedding":
        if inference is None:
            raise ValueError("mode='embedding' needs a posterior or a FlowEstimator as `inference`")
        est = _estimator_of(inference)
    xo, xt = _as_rows(x_obs, "x_obs"), _as_rows(x, "x")
    if xo.shape[1] != xt.shape[1]:
        raise ValueError(f"x_obs has {xo.shape[1]} features and x has {xt.shape[1]}: they must agree")
    if n_shuffle < 1:
        raise ValueError("n_shuffle must be at least 1")
    seed = int(seed) & (2 ** 64 - 1)
    if max_train is not None and int(max_train) < xt.shape[0]:
        if int(max_train) < 1:
            raise ValueError("max_train must be positive")
        xt = xt[mmd_subsets(seed, 1, xt.shape[0], int(max_train), first=SET_TRAIN)[0]]
    M, N = xo.shape[0], xt.shape[0]
    if M < 2 or N < M + 2:
        raise ValueError(f"need M >= 2 observed rows and N >= M + 2 training rows, got M = {M}, N = {N}")
    if mode == "x_space" and xt.shape[1] > CMAX:
        raise ValueError(f"{xt.shape[1]} features: the device kernels take at most {CMAX}")
    torch = _need_gpu("the MMD misspecification test")
    if est is not None:
        dev = est.flat.device
        if dev.type != "cuda":
            raise RuntimeError("the embedding of the MMD misspecification test runs on the GPU; there is no CPU fallback")
        with torch.no_grad():
            z = est.embed(torch.tensor(xt)).float().contiguous()
            zo = est.embed(torch.tensor(xo)).float().contiguous()
        if z.dim() != 2 or z.shape[1] > CMAX:
            raise ValueError(f"the embedding has shape {tuple(z.shape)}: the device kernels take (rows, at most {CMAX} columns)")
        if not (bool(torch.isfinite(z).all()) and bool(torch.isfinite(zo).all())):
            raise ValueError("the embedding holds non-finite values")
    else:
        dev = torch.device(device if device is not None and str(device).startswith("cuda") else "cuda")
        z, zo = torch.tensor(xt).to(dev), torch.tensor(xo).to(dev)
        if z_score:
            mean, std = z.mean(0), z.std(0, unbiased=True).clamp_min(1e-7)
            z, zo = ((z - mean) / std).contiguous(), ((zo - mean) / std).contiguous()
    scale = rbf_scale(z, seed) if scale is None else float(scale)
    c2 = c2_of(scale)
    r = rbf_rowsum(z, z, c2, exclude_self=True)
    R = float(r.sum())
    A_o = float(rbf_rowsum(zo, zo, c2, exclude_self=True).sum())
    Cx_o = float(rbf_rowsum(z, zo, c2).sum())
    mmd2 = A_o / (M * (M - 1)) + R / (N * (N - 1)) - 2.0 * Cx_o / (M * N)
    per = max(1, min(int(n_shuffle), INDEX_BYTES // (4 * M)))
    null = []
    for s0 in range(0, int(n_shuffle), per):
        idx = _subsets_device(seed, s0, min(per, int(n_shuffle) - s0), N, M, dev)
        A_s, picked = rbf_subset_sums(z, idx, c2, r, check=False)
        null.append(null_mmd2(A_s, picked, R, N, M))
    null = torch.cat(null).cpu().numpy()
    p_value = float(np.mean(null > mmd2))
    mmds_baseline, mmd = np.sqrt(np.maximum(null, 0.0)), math.sqrt(max(mmd2, 0.0))
    if return_details:
        return {"p_value": p_value, "reject": bool(p_value < alpha), "mmd": mmd, "mmds_baseline": mmds_baseline, "mmd2": mmd2,
                "null_mmd2": null, "scale": scale}
    return p_value, (mmds_baseline, mmd)


# ---- the marginal flow ------------------------------------------------------------------------------------------------------
def _check_features(F: int):
    if F > MAX_F:
        raise ValueError(f"{F} features: the flow engine takes D <= {MAX_F}, so the marginal flow (method='logprob') stops there; "
                         "method='mmd' has no such limit")


class MarginalEstimator:
    """An unconditional density of the training features: a ``FlowEstimator`` whose context is one constant zero column."""

    def __init__(self, estimator, summary: Dict[str, Any]):
        self.estimator, self.summary = estimator, summary
        self.n_features = int(estimator.spec.D)

    def _rows(self, x):
        import torch
        t = torch.as_tensor(np.asarray(x, dtype=np.float32) if not torch.is_tensor(x) else x)
        t = t.to(device=self.estimator.flat.device, dtype=torch.float32)
        t = t[None, :] if t.dim() == 1 else t
        if t.dim() != 2 or t.shape[1] != self.n_features:
            raise ValueError(f"x must be ({self.n_features},) or (rows, {self.n_features}), got {tuple(t.shape)}")
        return t.contiguous()

    def log_prob(self, x):
        """float32 device tensor [rows]: ``estimator.log_prob(x, zeros)``."""
        torch = _need_gpu("the marginal flow")
        t = self._rows(x)
        with torch.no_grad():
            return self.estimator.log_prob(t, torch.zeros((t.shape[0], 1), dtype=torch.float32, device=t.device))

    def sample(self, sample_shape=(1,), seed: int = 0):
        """Draws (n, F) of the density, a float32 device tensor."""
        torch = _need_gpu("the marginal flow")
        n = int(np.prod(tuple(sample_shape))) if not isinstance(sample_shape, int) else int(sample_shape)
        ctx = torch.zeros((1, 1), dtype=torch.float32, device=self.estimator.flat.device)
        return self.estimator.sample(n, ctx, seed=int(seed))[0]


class MarginalTrainer:
    """sbi's ``MarginalTrainer`` on the flow engine.  ``density_estimator``: "NSF" (default) or "MAF"; with the default
    ``backend="lampe"`` these are the zuko-style autoregressive kinds (5 transforms, 50 hidden units), ``backend="sbi"`` selects
    the nflows-style kinds.  Other ``build_kwargs`` go to ``estimator.build_flow``."""

    def __init__(self, density_estimator: str = "NSF", **build_kwargs):
        model = str(density_estimator).lower()
        if model not in ("nsf", "maf"):
            raise ValueError(f"density_estimator={density_estimator!r} is not built: 'NSF' or 'MAF'")
        self.model = model
        kw = dict(backend="lampe", num_transforms=5, hidden_features=50)
        kw.update(build_kwargs)
        self.build_kwargs = kw
        self._x: Optional[np.ndarray] = None
        self.estimator: Optional[MarginalEstimator] = None

    def append_samples(self, x):
        a = _as_rows(x, "x")
        _check_features(a.shape[1])
        if self._x is not None and self._x.shape[1] != a.shape[1]:
            raise ValueError(f"appended rows have {a.shape[1]} features, the stored ones {self._x.shape[1]}")
        self._x = a if self._x is None else np.concatenate([self._x, a], 0)
        return self

    def train(self, training_batch_size: int = 200, learning_rate: float = 5e-4, validation_fraction: float = 0.1,
              stop_after_epochs: int = 20, max_num_epochs: int = 2 ** 31 - 1, clip_max_norm: Optional[float] = 5.0,
              seed: Optional[int] = None, device=None) -> MarginalEstimator:
        if self._x is None:
            raise ValueError("no samples: call append_samples(x) first")
        torch = _need_gpu("the marginal flow")
        from .estimator import build_flow
        from .runner import train_flow
        dev = torch.device(device if device is not None and str(device).startswith("cuda") else "cuda")
        dev = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        theta = torch.tensor(self._x).to(dev).contiguous()
        ctx = torch.zeros((theta.shape[0], 1), dtype=torch.float32, device=dev)   # its std is clamped: it standardises to 0
        gen = torch.Generator().manual_seed(0 if seed is None else int(seed) & (2 ** 63 - 1))
        est = build_flow(self.model, theta, ctx, device=dev, generator=gen, **self.build_kwargs).to(dev)
        with torch.no_grad():
            initial = float(-est.log_prob(theta, ctx).double().mean())
        with torch.cuda.device(dev):
            summary = train_flow(est, theta, ctx, batch_size=int(training_batch_size), learning_rate=float(learning_rate),
                                 validation_fraction=float(validation_fraction), stop_after_epochs=int(stop_after_epochs),
                                 max_num_epochs=int(max_num_epochs), clip_max_norm=clip_max_norm, seed=seed, log_every=0)
        summary["initial_loss"] = initial
        self.estimator = MarginalEstimator(est, summary)
        return self.estimator


def calc_misspecification_logprob(x_train, x_o, estimator, alpha: float = 0.05):
    """sbi's ``calc_misspecification_logprob``: ``p_value = mean(log_prob(x_train) < log_prob(x_o))`` and
    ``reject_H0 = p_value < alpha``.  ``x_o`` of shape (F,) gives scalars, (M, F) gives arrays of M."""
    import torch
    xo = x_o.detach().cpu().numpy() if torch.is_tensor(x_o) else np.asarray(x_o)
    single = xo.ndim == 1
    xo = _as_rows(xo[None, :] if single else xo, "x_o")
    xt = _as_rows(x_train, "x_train")
    if xo.shape[1] != xt.shape[1]:
        raise ValueError(f"x_o has {xo.shape[1]} features and x_train has {xt.shape[1]}: they must agree")
    _need_gpu("the log-prob misspecification test")
    lp_t = np.asarray(estimator.log_prob(xt).detach().cpu().numpy(), dtype=np.float64).reshape(-1)
    lp_o = np.asarray(estimator.log_prob(xo).detach().cpu().numpy(), dtype=np.float64).reshape(-1)
    p = (lp_t[None, :] < lp_o[:, None]).mean(1)
    reject = p < alpha
    return (float(p[0]), bool(reject[0])) if single else (p, reject)
