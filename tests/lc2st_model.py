"""The numpy model of the L-C2ST classifiers: an independent restatement of what
synference_amd/lc2st.py and csrc/sf_lc2st.hip compute -- z-score, labels, stratified split and Glorot init from the documented
streams (Philox from ``oracle.philox``), the keyed per-epoch order, sklearn's MLPClassifier training loop and stopping rule,
scores and p-value.  ``dtype`` selects the arithmetic: float64 is the reference, float32 gives the rounding-error scale that
the device tolerances are built from.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

from oracle.philox import philox4x32_10

STREAM_ORDER, STREAM_LABELS, STREAM_SPLIT, STREAM_INIT = 0x4C433200, 0x4C433201, 0x4C433202, 0x4C433203
LR, B1, B2, EPS, ALPHA, TOL, BATCH = 1e-3, 0.9, 0.999, 1e-8, 1e-4, 1e-4, 200


def _u(index, clf, seed, stream):
    n = len(index)
    z = np.zeros(n, dtype=np.uint32)
    return philox4x32_10(np.asarray(index, dtype=np.uint32), z, np.full(n, clf, dtype=np.uint32), z,
                         seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ stream)[0]


def zscore(thetas, xs, posterior_samples):
    """class 0 rows [z(posterior_samples), z(xs)], then class 1 rows [z(thetas), z(xs)]; float64."""
    th, xs, ps = (np.asarray(a, dtype=np.float64) for a in (thetas, xs, posterior_samples))
    tm, ts, xm, xsd = ps.mean(0), ps.std(0, ddof=1), xs.mean(0), xs.std(0, ddof=1)
    zx = (xs - xm) / xsd
    rows = np.concatenate([np.concatenate([(ps - tm) / ts, zx], 1), np.concatenate([(th - tm) / ts, zx], 1)], 0)
    return rows, (tm, ts, xm, xsd)


def rows_at(theta_o, x_o, stats):
    tm, ts, xm, xsd = stats
    theta_o = np.asarray(theta_o, dtype=np.float64)
    zx = np.broadcast_to((np.asarray(x_o, dtype=np.float64).reshape(-1) - xm) / xsd, (len(theta_o), len(xm)))
    return np.concatenate([(theta_o - tm) / ts, zx], 1)


def labels_for(seed, clf, N):
    lab = np.ones(2 * N, dtype=np.uint8)
    if clf == 0:
        lab[:N] = 0
        return lab
    u = _u(np.arange(2 * N), clf, seed, STREAM_LABELS)
    order = sorted(range(2 * N), key=lambda r: (int(u[r]), r))
    lab[order[:N]] = 0
    return lab


def validation_mask(seed, clf, lab):
    vm = np.zeros(len(lab), dtype=np.uint8)
    u = _u(np.arange(len(lab)), clf, seed, STREAM_SPLIT)
    for k in (0, 1):
        rk = [r for r in range(len(lab)) if lab[r] == k]
        rk.sort(key=lambda r: (int(u[r]), r))
        vm[rk[:(len(rk) + 5) // 10]] = 1
    return vm


def offsets(n_in, W):
    o_b1 = n_in * W
    o_w2 = o_b1 + W
    o_b2 = o_w2 + W * W
    o_w3 = o_b2 + W
    o_b3 = o_w3 + W
    return o_b1, o_w2, o_b2, o_w3, o_b3, o_b3 + 1


def glorot_init(seed, clf, n_in, W):
    o_b1, o_w2, o_b2, o_w3, o_b3, NP = offsets(n_in, W)
    u = _u(np.arange(NP), clf, seed, STREAM_INIT)
    U = ((u >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    bound = np.concatenate([np.full(o_w2, np.sqrt(6.0 / (n_in + W))), np.full(o_w3 - o_w2, np.sqrt(6.0 / (2 * W))),
                            np.full(NP - o_w3, np.sqrt(6.0 / (W + 1)))])
    return ((2.0 * U - 1.0) * bound).astype(np.float32)


def _mix(u):
    u = u ^ (u >> np.uint32(16)); u = u * np.uint32(0x7FEB352D)
    u = u ^ (u >> np.uint32(15)); u = u * np.uint32(0x846CA68B)
    return u ^ (u >> np.uint32(16))


def keyed_order(seed, clf, epoch, n):
    one = np.zeros(1, dtype=np.uint32)
    key = [np.uint32(int(k[0])) for k in philox4x32_10(one + np.uint32(clf), one + np.uint32(epoch), one, one, seed & 0xFFFFFFFF,
                                                       ((seed >> 32) & 0xFFFFFFFF) ^ STREAM_ORDER)]
    hb = 1
    while 4 ** hb < n:
        hb += 1
    mask = np.uint32((1 << hb) - 1)
    out = np.empty(n, dtype=np.int64)
    with np.errstate(over="ignore"):
        for j in range(n):
            x = np.uint32(j)
            while True:
                L, R = x >> np.uint32(hb), x & mask
                for r in range(4):
                    L, R = R, L ^ (_mix(R ^ key[r]) & mask)
                x = (L << np.uint32(hb)) | R
                if x < n:
                    break
            out[j] = int(x)
    return out


def unpack(w, n_in, W):
    o_b1, o_w2, o_b2, o_w3, o_b3, NP = offsets(n_in, W)
    return [w[:o_b1].reshape(n_in, W), w[o_w2:o_b2].reshape(W, W), w[o_w3:o_b3].reshape(W, 1)], [w[o_b1:o_w2], w[o_b2:o_w3], w[o_b3:NP]]


def pack(coefs, intercepts):
    return np.concatenate([coefs[0].ravel(), intercepts[0], coefs[1].ravel(), intercepts[1], coefs[2].ravel(), intercepts[2]])


def logits(w, X, n_in, W):
    (W1, W2, W3), (b1, b2, b3) = unpack(w, n_in, W)
    h1 = np.maximum(X @ W1 + b1, 0)
    h2 = np.maximum(h1 @ W2 + b2, 0)
    return (h2 @ W3 + b3)[:, 0], h1, h2


def sigmoid(z):
    return 1 / (1 + np.exp(-z))


def gradient(w, X, y, n_in, W, alpha=ALPHA):
    """sklearn's _backprop: mean BCE gradient, plus alpha W / n on the weights (not on the intercepts)."""
    dt = w.dtype
    (W1, W2, W3), _ = unpack(w, n_in, W)
    z, h1, h2 = logits(w, X, n_in, W)
    n = dt.type(len(X))
    d3 = (sigmoid(z) - y.astype(dt))[:, None]
    d2 = (d3 @ W3.T) * (h2 > 0)
    d1 = (d2 @ W2.T) * (h1 > 0)
    a = dt.type(alpha)
    return pack([(X.T @ d1 + a * W1) / n, (h1.T @ d2 + a * W2) / n, (h2.T @ d3 + a * W3) / n],
                [d1.sum(0) / n, d2.sum(0) / n, d3.sum(0) / n])


class Adam:
    """sklearn's AdamOptimizer: the step size carries both bias corrections (float64, then the working dtype)."""

    def __init__(self, n, dtype):
        self.m, self.v, self.t, self.dt = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype), 0, np.dtype(dtype)

    def step(self, w, g):
        dt = self.dt.type
        self.t += 1
        self.m = dt(B1) * self.m + (dt(1) - dt(B1)) * g
        self.v = dt(B2) * self.v + (dt(1) - dt(B2)) * g * g
        lr_t = dt(LR * np.sqrt(1.0 - B2 ** self.t) / (1.0 - B1 ** self.t))
        return w + (-lr_t * self.m / (np.sqrt(self.v) + dt(EPS)))


class StoppingRule:
    """sklearn's _update_no_improvement_count (early_stopping=True) and the test that follows it in _fit_stochastic."""

    def __init__(self, n_iter_no_change, tol=TOL):
        self.best, self.count, self.best_iter, self.n, self.limit, self.tol = -np.inf, 0, 0, 0, n_iter_no_change, tol

    def update(self, score):
        """-> (new best?, stop?)"""
        self.n += 1
        self.count = self.count + 1 if score < self.best + self.tol else 0
        better = score > self.best
        if better:
            self.best, self.best_iter = score, self.n
        return better, self.count > self.limit


def apply_rule(scores, n_iter_no_change, max_iter, tol=TOL):
    """(n_iter, best_iter, best_score) of a score sequence that is at least as long as the run."""
    rule = StoppingRule(n_iter_no_change, tol)
    for s in scores[:max_iter]:
        _, stop = rule.update(s)
        if stop:
            break
    return rule.n, rule.best_iter, rule.best


def train(rows, lab, vmask, w0, seed, clf, *, max_iter, n_iter_no_change=None, dtype=np.float64, batch=BATCH, shuffle=True):
    """One classifier.  ``n_iter_no_change=None``: early stopping off (max_iter epochs, the last weights).  Returns weights,
    validation counts and scores per epoch, n_iter, best_iter and the smallest |logit| met on a validation row."""
    dt = np.dtype(dtype)
    X, n_in = np.asarray(rows, dtype=dt), rows.shape[1]
    W = int(round((-(n_in + 3) + np.sqrt((n_in + 3) ** 2 - 4 * (1 - len(w0)))) / 2))
    assert offsets(n_in, W)[5] == len(w0)
    tr, va = np.flatnonzero(vmask == 0), np.flatnonzero(vmask == 1)
    w, opt = np.asarray(w0, dtype=dt).copy(), Adam(len(w0), dt)
    rule = StoppingRule(n_iter_no_change) if n_iter_no_change is not None else None
    best_w, counts, min_abs = w.copy(), [], np.inf
    for epoch in range(max_iter):
        order = keyed_order(seed, clf, epoch, len(tr)) if shuffle else np.arange(len(tr))
        for mb in range(0, len(tr), batch):
            r = tr[order[mb:mb + batch]]
            w = opt.step(w, gradient(w, X[r], lab[r], n_in, W))
        if len(va):
            z = logits(w, X[va], n_in, W)[0]
            min_abs = min(min_abs, float(np.abs(z).min()))
            counts.append(int(((z > 0).astype(np.uint8) == lab[va]).sum()))
        else:
            counts.append(0)
        if rule is not None and len(va):
            better, stop = rule.update(counts[-1] / len(va))
            if better:
                best_w = w.copy()
            if stop:
                break
    n_iter = len(counts)
    final = best_w if rule is not None and len(va) else w
    return {"weights": final, "counts": np.asarray(counts), "scores": np.asarray(counts) / max(len(va), 1), "n_iter": n_iter,
            "best_iter": rule.best_iter if rule is not None and len(va) else n_iter, "min_abs_val_logit": min_abs, "n_val": len(va)}


def scores(w, rows_o, n_in, W, dtype=np.float64):
    """p = 1 - sigmoid(logit) per row and mean((p - 0.5)^2), every step in ``dtype``."""
    dt = np.dtype(dtype)
    z = logits(np.asarray(w, dtype=dt), np.asarray(rows_o, dtype=dt), n_in, W)[0]
    p = dt.type(1) - sigmoid(z)
    return p, float(np.mean((p - dt.type(0.5)) ** 2, dtype=dt))


def p_value(stat_data, stats_null):
    return float(np.mean(stat_data < np.asarray(stats_null)))
