"""L-C2ST, the local classifier two-sample test (Linhart et al. 2023), on the device: is the posterior calibrated AT ONE
observation?  ``LC2ST`` carries the constructor arguments and method names of ``sbi.diagnostics.lc2st.LC2ST`` as the reference
calls it (ref: src/synference/sbi_runner.py:986-1063: ``classifier="mlp"``, ``num_ensemble=1``, ``num_folds=1``,
``z_score=True``, ``num_trials_null=100``, ``permutation=True``).  The algorithm is restated from sbi's published source
([UPSTREAM], the orchestration is unpinned: sbi cannot be run beside this); the classifier is sklearn's ``MLPClassifier`` with
sbi's settings, and ITS arithmetic is pinned (tests/test_cpu_lc2st.py holds the restatement to sklearn at 1e-12).

One classifier separates class 0 rows ``[z(posterior_samples_n), z(x_n)]`` from class 1 rows ``[z(theta_n), z(x_n)]``;
``num_trials_null`` more see the same 2N rows with a random half labelled 0 (sbi's permutation null).  All of them train in one
launch sequence of ``sf_c2st_train`` (csrc/sf_lc2st.hip: one workgroup per classifier); ``sf_c2st_scores`` evaluates
``p = predict_proba(.)[:, 0]`` and ``mean((p - 0.5)^2)`` at ``(theta_o, x_o)``.  There is no CPU path.

Streams (Philox4x32-10, key ``(seed_lo, seed_hi ^ stream)``, counter ``(index, 0, classifier, 0)``, first output word ``u``):

* ``STREAM_LABELS``: null classifier t >= 1 orders the rows by ``(u(row), row)``; the first N get label 0, the rest label 1.
  Classifier 0 has the true labels (rows 0 .. N-1 class 0, rows N .. 2N-1 class 1).
* ``STREAM_SPLIT``: per classifier and per label value, its rows are ordered by ``(u(row), row)`` and the first
  ``(n_class + 5) // 10`` are the validation rows (sklearn: a stratified 10 % split).
* ``STREAM_INIT``: element e of the dense parameter vector (W1, b1, W2, b2, w3, b3; row major) is
  ``(2 U - 1) sqrt(6 / (fan_in + fan_out))`` with ``U = ((u(e) >> 9) + 0.5) 2^-23``, in float64, rounded to float32.
* ``STREAM_ORDER``: ``keyed_order`` -- the row order of one epoch, computed per index inside the kernel.
"""
from __future__ import annotations

import ctypes as C
import logging
import time
from typing import Optional, Sequence

import numpy as np

logger = logging.getLogger("synference_amd")

STREAM_ORDER, STREAM_LABELS, STREAM_SPLIT, STREAM_INIT = 0x4C433200, 0x4C433201, 0x4C433202, 0x4C433203
MAX_IN, MAX_W, MAX_D = 80, 128, 16
BATCH = 200
# Epochs per kernel launch.  A launch must stay far below a second on a shared device, and a host round trip (launch, copy of
# the state words, synchronise) costs some tens of microseconds, so anything from a few epochs up amortises it.  At the
# reference's size (18 000 training rows: 90 minibatches per epoch) an epoch was measured at 11 ms, a launch of eight at 90 ms.
EPOCHS_PER_LAUNCH = 8

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def _philox(c0, c1, c2, c3, seed: int, stream: int):
    """philox4x32_10(counter, (seed_lo, seed_hi ^ stream)): four uint32 arrays (csrc/sf_rng.h)."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(a, dtype=np.uint32) for a in (c0, c1, c2, c3)))
    k0, k1 = seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ stream
    for _ in range(10):
        p0, p1 = _M0 * c0.astype(np.uint64), _M1 * c2.astype(np.uint64)
        hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & _MASK).astype(np.uint32)
        hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & _MASK).astype(np.uint32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint32(k0), lo1, hi0 ^ c3 ^ np.uint32(k1), lo0
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _mix(u):
    u = u ^ (u >> np.uint32(16)); u = u * np.uint32(0x7FEB352D)
    u = u ^ (u >> np.uint32(15)); u = u * np.uint32(0x846CA68B)
    return u ^ (u >> np.uint32(16))


def keyed_order(seed: int, clf: int, epoch: int, n: int) -> np.ndarray:
    """The row order of epoch ``epoch`` (0-based) of classifier ``clf``: position j visits training row number ``out[j]``.
    A bijection of [0, n): four Feistel rounds on 2 hb bits (hb the smallest with 4^hb >= n, at least 1), round function
    ``mix(R ^ key_r) & (2^hb - 1)`` with ``mix`` the lowbias32 finaliser and the four keys one Philox block; values outside
    [0, n) are walked through the bijection again until they fall inside."""
    key = [np.uint32(int(k)) for k in _philox(clf, epoch, 0, 0, seed, STREAM_ORDER)]
    hb = 1
    while (1 << (2 * hb)) < n:
        hb += 1
    mask, hbu = np.uint32((1 << hb) - 1), np.uint32(hb)
    x = np.arange(n, dtype=np.uint32)
    todo = np.ones(n, dtype=bool)
    with np.errstate(over="ignore"):
        while todo.any():
            v = x[todo]
            L, R = v >> hbu, v & mask
            for r in range(4):
                L, R = R, L ^ (_mix(R ^ key[r]) & mask)
            x[todo] = (L << hbu) | R
            todo = x >= n
    return x.astype(np.int64)


def _ranked(u, rows):
    return rows[np.lexsort((rows, u))]


def make_labels(seed: int, n_cls: int, N: int) -> np.ndarray:
    """uint8 [n_cls, 2N]: classifier 0 the true classes, classifier t >= 1 a keyed random half (exactly N zeros)."""
    R = 2 * N
    lab = np.ones((n_cls, R), dtype=np.uint8)
    lab[0, :N] = 0
    rows = np.arange(R)
    for t in range(1, n_cls):
        u = _philox(rows, 0, t, 0, seed, STREAM_LABELS)[0]
        lab[t, _ranked(u, rows)[:N]] = 0
    return lab


def make_validation_mask(seed: int, labels: np.ndarray) -> np.ndarray:
    """uint8 [n_cls, R]: 1 for the validation rows, (n_class + 5) // 10 of each label value."""
    n_cls, R = labels.shape
    vm = np.zeros((n_cls, R), dtype=np.uint8)
    rows = np.arange(R)
    for t in range(n_cls):
        u = _philox(rows, 0, t, 0, seed, STREAM_SPLIT)[0]
        for k in (0, 1):
            rk = rows[labels[t] == k]
            vm[t, _ranked(u[rk], rk)[:(len(rk) + 5) // 10]] = 1
    return vm


def num_params(n_in: int, W: int) -> int:
    return n_in * W + W + W * W + W + W + 1


def make_init(seed: int, n_cls: int, n_in: int, W: int) -> np.ndarray:
    """float32 [n_cls, num_params]: Glorot-uniform weights AND biases, as sklearn's ``_init_coef`` bounds them."""
    NP = num_params(n_in, W)
    bound = np.empty(NP, dtype=np.float64)
    o1, o2 = n_in * W + W, n_in * W + W + W * W + W
    bound[:o1] = np.sqrt(6.0 / (n_in + W))
    bound[o1:o2] = np.sqrt(6.0 / (W + W))
    bound[o2:] = np.sqrt(6.0 / (W + 1))
    e = np.arange(NP)
    out = np.empty((n_cls, NP), dtype=np.float32)
    for t in range(n_cls):
        u = _philox(e, 0, t, 0, seed, STREAM_INIT)[0]
        U = ((u >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
        out[t] = ((2.0 * U - 1.0) * bound).astype(np.float32)
    return out


def _as_2d(a, name):
    shape = tuple(a.shape)
    if len(shape) != 2:
        raise ValueError(f"{name} must be two-dimensional (rows, columns), got shape {shape}")
    return shape


class LC2ST:
    """``sbi.diagnostics.lc2st.LC2ST`` on the device.  ``thetas`` (N, D) and ``xs`` (N, C) are calibration pairs from the
    joint, ``posterior_samples`` (N, D) one draw of q(theta | x_n) per row; arrays or tensors, on any device.

    Only what the reference uses exists: ``classifier="mlp"``, ``num_ensemble=1``, ``num_folds=1``, ``permutation=True``;
    anything else raises ``ValueError``.  Limits: D <= 16, D + C <= 80, hidden width <= 128 (sbi's 10 D is capped there).
    Random numbers are the seed-keyed streams of the module docstring, not numpy / torch global state.

    Keyword-only additions: ``hidden_width`` (default min(10 D, 128)), ``max_iter`` (1000), ``n_iter_no_change`` (50; None
    turns early stopping off: every classifier runs ``max_iter`` epochs and keeps its last weights), ``timeout_seconds``
    (checked between launches; classifiers still running then end where they stand), ``epochs_per_launch``.

    Classifier 0 is the observed one and 1 .. num_trials_null the null ones; ``trained_clfs`` arguments are sequences of
    these indices.  ``train_all()`` trains both kinds in one launch sequence."""

    def __init__(self, thetas, xs, posterior_samples, seed: int = 1, num_folds: int = 1, num_ensemble: int = 1,
                 classifier="mlp", z_score: bool = True, num_trials_null: int = 100, permutation: bool = True, *,
                 hidden_width: Optional[int] = None, max_iter: int = 1000, n_iter_no_change: Optional[int] = 50,
                 timeout_seconds: Optional[float] = None, epochs_per_launch: int = EPOCHS_PER_LAUNCH, device=None):
        if classifier != "mlp":
            raise ValueError(f"classifier={classifier!r} is not built: only 'mlp' (sklearn's MLPClassifier) exists")
        if num_ensemble != 1:
            raise ValueError(f"num_ensemble={num_ensemble} is not built: only num_ensemble=1 exists")
        if num_folds != 1:
            raise ValueError(f"num_folds={num_folds} is not built: only num_folds=1 exists")
        if not permutation:
            raise ValueError("permutation=False is not built: only the permutation null (permutation=True) exists")
        (N, D), (Nx, Cx), (Np, Dp) = _as_2d(thetas, "thetas"), _as_2d(xs, "xs"), _as_2d(posterior_samples, "posterior_samples")
        if not (N == Nx == Np) or D != Dp:
            raise ValueError(f"thetas {N, D}, xs {Nx, Cx} and posterior_samples {Np, Dp} do not agree")
        if D > MAX_D:
            raise ValueError(f"D = {D} parameters: the device classifiers take D <= {MAX_D}")
        if D + Cx > MAX_IN:
            raise ValueError(f"D + C = {D + Cx} classifier inputs: the device classifiers take n_in <= {MAX_IN}")
        if hidden_width is not None and not 1 <= int(hidden_width) <= MAX_W:
            raise ValueError(f"hidden_width = {hidden_width}: the device classifiers take 1 <= W <= {MAX_W}")
        if N < 5:
            raise ValueError("need at least 5 calibration rows (a stratified 10 % validation split of each class)")
        if num_trials_null < 0 or max_iter < 1 or epochs_per_launch < 1 or (n_iter_no_change is not None and n_iter_no_change < 0):
            raise ValueError("num_trials_null >= 0, max_iter >= 1, epochs_per_launch >= 1 and n_iter_no_change >= 0 are needed")
        self.N, self.D, self.C, self.n_in = N, D, Cx, D + Cx
        self.W = int(hidden_width) if hidden_width is not None else min(10 * D, MAX_W)
        self.seed, self.z_score, self.num_trials_null = int(seed) & (2 ** 64 - 1), bool(z_score), int(num_trials_null)
        self.max_iter, self.n_iter_no_change = int(max_iter), n_iter_no_change
        self.timeout_seconds, self.epochs_per_launch = timeout_seconds, int(epochs_per_launch)
        self.num_folds, self.num_ensemble, self.permutation, self.classifier = 1, 1, True, "mlp"
        self._inputs, self._device_arg = (thetas, xs, posterior_samples), device
        self.n_cls, self.num_params = 1 + self.num_trials_null, num_params(self.n_in, self.W)
        self._h = None
        self.trained_clfs: Optional[list] = None
        self.trained_clfs_null: Optional[list] = None
        self.timed_out = False

    # ---- device side --------------------------------------------------------------------------------------------------
    def _device(self):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("L-C2ST runs on the GPU (sf_c2st_train, sf_c2st_scores); there is no CPU fallback")
        d = self._device_arg
        return torch.device(d if d is not None and str(d).startswith("cuda") else "cuda")

    def _ensure(self):
        if self._h is not None:
            return
        import torch
        from . import _lib
        dev = self._device()
        th, xs, ps = (torch.as_tensor(np.ascontiguousarray(a) if not torch.is_tensor(a) else a).to(device=dev, dtype=torch.float64)
                      for a in self._inputs)
        if self.z_score:
            self.theta_mean, self.theta_std = ps.mean(0), ps.std(0, unbiased=True).clamp_min(1e-14)
            self.x_mean, self.x_std = xs.mean(0), xs.std(0, unbiased=True).clamp_min(1e-14)
        else:
            self.theta_mean, self.theta_std = torch.zeros(self.D, dtype=torch.float64, device=dev), torch.ones(self.D, dtype=torch.float64, device=dev)
            self.x_mean, self.x_std = torch.zeros(self.C, dtype=torch.float64, device=dev), torch.ones(self.C, dtype=torch.float64, device=dev)
        zx = (xs - self.x_mean) / self.x_std
        rows = torch.cat([torch.cat([(ps - self.theta_mean) / self.theta_std, zx], 1),
                          torch.cat([(th - self.theta_mean) / self.theta_std, zx], 1)], 0)
        self.rows = rows.to(torch.float32).contiguous()                       # [2N, n_in]
        labels = make_labels(self.seed, self.n_cls, self.N)
        vmask = make_validation_mask(self.seed, labels)
        init = make_init(self.seed, self.n_cls, self.n_in, self.W)
        self.labels = torch.as_tensor(labels).to(dev)
        self.vmask = torch.as_tensor(vmask).to(dev)
        init_d = torch.as_tensor(init).to(dev)
        desc = _lib.sf_c2st_desc(
            n_in=self.n_in, width=self.W, n_cls=self.n_cls, max_iter=self.max_iter,
            n_iter_no_change=0 if self.n_iter_no_change is None else int(self.n_iter_no_change),
            early_stopping=0 if self.n_iter_no_change is None else 1, batch=BATCH, R=2 * self.N, seed=self.seed,
            lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, alpha=1e-4, tol=1e-4,
            rows=self.rows.data_ptr(), labels=self.labels.data_ptr(), vmask=self.vmask.data_ptr(), init_weights=init_d.data_ptr())
        h = C.c_void_p()
        with torch.cuda.device(dev):
            _lib.check(_lib.load().sf_c2st_create(C.byref(desc), C.byref(h), _lib.stream_ptr(dev)))
        self._h, self._dev = h, dev

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            try:
                from . import _lib
                _lib.load().sf_c2st_destroy(h)
            except Exception:   # interpreter shutdown
                pass

    def _train(self, first: int, count: int) -> None:
        import torch
        from . import _lib
        self._ensure()
        lib, t0 = _lib.load(), time.monotonic()
        n_active = C.c_int32(0)
        with torch.cuda.device(self._dev):
            st = _lib.stream_ptr(self._dev)
            while True:
                _lib.check(lib.sf_c2st_train(self._h, first, count, self.epochs_per_launch, 0, C.byref(n_active), st))
                if n_active.value == 0:
                    break
                if self.timeout_seconds is not None and time.monotonic() - t0 > self.timeout_seconds:
                    logger.warning("LC2ST: timeout_seconds=%s reached with %d classifiers still training; they end where they "
                                   "stand", self.timeout_seconds, n_active.value)
                    _lib.check(lib.sf_c2st_train(self._h, first, count, 0, 1, C.byref(n_active), st))
                    self.timed_out = True
                    break

    def train_on_observed_data(self, seed: Optional[int] = None, verbosity: int = 0):
        self._train(0, 1)
        self.trained_clfs = [0]
        return self.trained_clfs

    def train_under_null_hypothesis(self, verbosity: int = 0):
        if self.num_trials_null > 0:
            self._train(1, self.num_trials_null)
        self.trained_clfs_null = list(range(1, self.n_cls))
        return self.trained_clfs_null

    def train_all(self):
        """Observed and null classifiers in one launch sequence."""
        self._train(0, self.n_cls)
        self.trained_clfs, self.trained_clfs_null = [0], list(range(1, self.n_cls))

    def training_state(self):
        """``weights`` float32 [n_cls, num_params] (W1, b1, W2, b2, w3, b3), ``validation_scores`` float64 [n_cls, max_iter]
        (NaN: epoch not run), ``n_iter``, ``best_iter``, ``done``, ``n_train``, ``n_val`` per classifier."""
        import torch
        from . import _lib
        self._ensure()
        w = np.empty((self.n_cls, self.num_params), dtype=np.float32)
        sl = np.empty((self.n_cls, self.max_iter), dtype=np.int32)
        stt = np.empty((self.n_cls, 8), dtype=np.int32)
        with torch.cuda.device(self._dev):
            _lib.check(_lib.load().sf_c2st_get(self._h, w.ctypes.data, sl.ctypes.data, stt.ctypes.data, _lib.stream_ptr(self._dev)))
        n_val = stt[:, 6].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            scores = np.where(sl >= 0, sl / n_val[:, None], np.nan)
        return {"weights": w, "validation_scores": scores, "validation_counts": sl, "n_iter": stt[:, 0].copy(),
                "best_iter": stt[:, 3].copy(), "done": stt[:, 4].astype(bool), "n_train": stt[:, 5].copy(), "n_val": stt[:, 6].copy()}

    # ---- scores ---------------------------------------------------------------------------------------------------------
    def _rows_o(self, theta_o, x_row):
        import torch
        th = torch.as_tensor(np.ascontiguousarray(theta_o) if not torch.is_tensor(theta_o) else theta_o).to(device=self._dev, dtype=torch.float64)
        if th.dim() != 2 or th.shape[1] != self.D:
            raise ValueError(f"theta_o must be (S, {self.D}), got {tuple(th.shape)}")
        zx = ((x_row - self.x_mean) / self.x_std).expand(th.shape[0], self.C)
        return torch.cat([(th - self.theta_mean) / self.theta_std, zx], 1).to(torch.float32).contiguous()

    def _x_rows(self, x_o):
        import torch
        x = torch.as_tensor(np.ascontiguousarray(x_o) if not torch.is_tensor(x_o) else x_o).to(device=self._dev, dtype=torch.float64)
        x = x[None, :] if x.dim() == 1 else x
        if x.dim() != 2 or x.shape[1] != self.C or x.shape[0] < 1:
            raise ValueError(f"x_o must be ({self.C},), (1, {self.C}) or (M, {self.C}), got {tuple(x.shape)}")
        return x, x.shape[0] == 1

    def _score_range(self, rows_o, clfs: Sequence[int], want_probs: bool):
        import torch
        from . import _lib
        S = rows_o.shape[0]
        stats = torch.empty(len(clfs), dtype=torch.float64, device=self._dev)
        probs = torch.empty((len(clfs), S), dtype=torch.float32, device=self._dev) if want_probs else None
        lib, i = _lib.load(), 0
        with torch.cuda.device(self._dev):
            st = _lib.stream_ptr(self._dev)
            while i < len(clfs):                      # one launch per run of consecutive indices
                j = i + 1
                while j < len(clfs) and clfs[j] == clfs[j - 1] + 1:
                    j += 1
                _lib.check(lib.sf_c2st_scores(self._h, int(clfs[i]), j - i, _lib.ptr(rows_o), S, C.c_void_p(stats[i:].data_ptr()),
                                              None if probs is None else C.c_void_p(probs[i:].data_ptr()), st))
                i = j
        return stats.cpu().numpy(), None if probs is None else probs.cpu().numpy()

    def get_scores(self, theta_o, x_o, return_probs: bool = False, trained_clfs: Optional[Sequence[int]] = None):
        """``scores`` float64 [n] = mean_s (p - 0.5)^2 per classifier of ``trained_clfs`` (default: the observed one), and with
        ``return_probs`` first ``probs`` float32 [n, S]: sbi's ``(probs, scores)`` order.  An (M, C) ``x_o`` adds a leading
        M axis to both (``theta_o`` is then (M, S, D))."""
        clfs = list(self.trained_clfs if trained_clfs is None else trained_clfs) if (trained_clfs is not None or self.trained_clfs) else None
        if clfs is None:
            raise ValueError("no trained classifiers: call train_on_observed_data() / train_under_null_hypothesis() first")
        if any(not 0 <= int(c) < self.n_cls for c in clfs):
            raise ValueError(f"trained_clfs holds classifier indices 0 .. {self.n_cls - 1}")
        self._ensure()
        x, single = self._x_rows(x_o)
        if single:
            s, p = self._score_range(self._rows_o(theta_o, x[0]), clfs, return_probs)
        else:
            if len(theta_o) != x.shape[0]:
                raise ValueError("an (M, C) x_o needs theta_o of shape (M, S, D)")
            res = [self._score_range(self._rows_o(theta_o[m], x[m]), clfs, return_probs) for m in range(x.shape[0])]
            s = np.stack([r[0] for r in res])
            p = np.stack([r[1] for r in res]) if return_probs else None
        return (p, s) if return_probs else s

    def get_statistic_on_observed_data(self, theta_o, x_o):
        if not self.trained_clfs:
            raise ValueError("the observed classifier is not trained: call train_on_observed_data() first")
        return self.get_scores(theta_o, x_o, trained_clfs=self.trained_clfs).mean(-1)

    def get_statistics_under_null_hypothesis(self, theta_o, x_o, return_probs: bool = False, verbosity: int = 0):
        if self.trained_clfs_null is None:
            raise ValueError("the null classifiers are not trained: call train_under_null_hypothesis() first")
        return self.get_scores(theta_o, x_o, return_probs=return_probs, trained_clfs=self.trained_clfs_null)

    def p_value(self, theta_o, x_o):
        stat = self.get_statistic_on_observed_data(theta_o, x_o)
        null = self.get_statistics_under_null_hypothesis(theta_o, x_o)
        return (np.asarray(stat)[..., None] < null).mean(-1)

    def reject_test(self, theta_o, x_o, alpha: float = 0.05):
        return self.p_value(theta_o, x_o) < alpha
