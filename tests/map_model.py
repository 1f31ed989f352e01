"""Model of the posterior-mode search (synference_amd/map.py, csrc/sf_gradtheta.hip): numpy plus the torch oracle.

Restates [UPSTREAM] sbi ``gradient_ascent`` (sbi 0.22 - 0.25, behind ``DirectPosterior.map`` / ``EnsemblePosterior.map``);
the constants are its named defaults.

1. Inits: ``R0`` points per row (accepted posterior draws, or a given tensor); the potential -- the raw estimator
   density, no leakage term: it is constant in theta -- is evaluated on all of them and the ``R = min(num_to_optimize,
   R0)`` highest are kept, lower index first on ties, non-finite values last.  A row without a finite init is NaN.
2. Unconstrained coordinates: ``phi_0 = logit(clamp((theta - lo) / (hi - lo), 1e-6, 1 - 1e-6))``; without a prior box
   the transform is the identity.  The potential excludes the transform's Jacobian: the mode is that of theta space.
3. Ascent, k = 0 .. num_iter - 1: evaluate (p_k, g_k) at theta_k = theta(phi_k); if ``k % save_best_every == 0`` and
   p_k > best (strictly), the candidate's best becomes (theta_k, p_k); then one ``torch.optim.Adam`` step on -sum p
   (betas 0.9 / 0.999, eps 1e-8, no weight decay, bias correction): elementwise, so the candidates are independent.
   A candidate whose value or gradient is not finite is frozen: it keeps its point, its moments and its best.
4. Result: p at phi_num_iter updates the best once more; the row's result is its best candidate, lowest index on ties;
   ``log_prob_map`` is that potential value.

Deviation from upstream: upstream scores phi_{k+1} after the step with a second evaluation of the potential; here the
value computed for the step is the one that is scored, plus one evaluation after the last step.  The scored iterates
are therefore {0, s, 2s, ..., num_iter} (s = save_best_every) instead of {s, 2s, ...}.  A candidate's best starts at
its init (when the init lies inside the box; the clamp of 2. can move the first iterate by 1e-6 of the box), so the
result is never below the best init.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import flows as OF

U_EPS = 1e-6
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8


# ---- potentials -------------------------------------------------------------------------------------------------------
def flow_potential(ospec, flat, dtype=torch.float64):
    """potential(theta [B, D], x [B, C]) -> (p [B], g [B, D]) by autograd through the oracle."""
    fl = torch.as_tensor(np.asarray(flat)).to(dtype)

    def fn(theta, x):
        th = torch.as_tensor(np.asarray(theta)).to(dtype).requires_grad_(True)
        lp = OF.log_prob(ospec, fl, th, torch.as_tensor(np.asarray(x)).to(dtype))
        (g,) = torch.autograd.grad(lp.sum(), th)
        return lp.detach().double().numpy(), g.double().numpy()
    return fn


def ensemble_potential(ospecs, flats, weights, dtype=torch.float64):
    """The mixture potential logsumexp_e(log w_e + lp_e) (oracle.posterior.ensemble_log_prob's formula, no box) and its
    autograd gradient."""
    w = np.asarray(weights, dtype=np.float64)
    logw = torch.as_tensor(np.log(w / w.sum())).to(dtype)
    fls = [torch.as_tensor(np.asarray(f)).to(dtype) for f in flats]

    def fn(theta, x):
        th = torch.as_tensor(np.asarray(theta)).to(dtype).requires_grad_(True)
        xt = torch.as_tensor(np.asarray(x)).to(dtype)
        lps = torch.stack([OF.log_prob(sp, fl, th, xt) for sp, fl in zip(ospecs, fls)], 0)
        lp = torch.logsumexp(lps + logw[:, None], dim=0)
        (g,) = torch.autograd.grad(lp.sum(), th)
        return lp.detach().double().numpy(), g.double().numpy()
    return fn


# ---- pieces -----------------------------------------------------------------------------------------------------------
def select_inits(p0, R):
    """[N, R0] potentials -> [N, R] indices of the R highest: lower index first on ties, non-finite last."""
    key = np.where(np.isfinite(p0), p0, -np.inf)
    return np.argsort(-key, axis=1, kind="stable")[:, :R]


def to_phi(theta, lo, hi):
    if lo is None:
        return np.array(theta, copy=True)
    u = np.clip((theta - lo) / (hi - lo), U_EPS, 1.0 - U_EPS)
    return np.log(u) - np.log1p(-u)


def sigmoid(phi):
    return 1.0 / (1.0 + np.exp(-phi))


def to_theta(phi, lo, hi):
    return np.array(phi, copy=True) if lo is None else lo + (hi - lo) * sigmoid(phi)


def gradient_ascent(potential, x, inits, lo=None, hi=None, num_iter=1000, num_to_optimize=100, learning_rate=0.01,
                    save_best_every=10, dtype=np.float64):
    """x [N, C], inits [N, R0, D] -> dict(theta_map [N, D], log_prob_map [N], theta_last [N, R, D], best_lp [N, R],
    init_idx [N, R], init_lp [N, R0]).  ``potential(theta [B, D], x [B, C]) -> (p, g)``; the state (phi, the moments)
    is kept in ``dtype``."""
    x = np.asarray(x)
    inits = np.asarray(inits, dtype=dtype)
    N, R0, D = inits.shape
    R = min(int(num_to_optimize), R0)
    if lo is not None:
        lo, hi = np.asarray(lo, dtype=dtype), np.asarray(hi, dtype=dtype)
    xr0 = np.repeat(x, R0, axis=0)
    p0, _ = potential(inits.reshape(N * R0, D), xr0)
    p0 = np.asarray(p0, dtype=np.float64).reshape(N, R0)
    idx = select_inits(p0, R)
    th0 = np.take_along_axis(inits, idx[:, :, None], axis=1).reshape(N * R, D)
    p_init = np.take_along_axis(np.where(np.isfinite(p0), p0, -np.inf), idx, axis=1).reshape(N * R)
    xr = np.repeat(x, R, axis=0)
    phi = to_phi(th0, lo, hi).astype(dtype)
    inside = np.ones(N * R, bool) if lo is None else ((th0 >= lo) & (th0 <= hi)).all(-1)
    keep = inside & np.isfinite(p_init)
    best_lp = np.where(keep, p_init, -np.inf)
    best_th = np.where(keep[:, None], th0, np.nan)
    theta = to_theta(phi, lo, hi).astype(dtype)
    theta[~np.isfinite(p_init)] = np.nan
    m, v = np.zeros_like(phi), np.zeros_like(phi)
    one = dtype(1.0)

    def score(p, ok):
        up = ok & (p > best_lp)
        best_lp[up] = p[up]
        best_th[up] = theta[up]

    for k in range(int(num_iter)):
        p, g = potential(theta, xr)
        p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=dtype)
        ok = np.isfinite(p) & np.isfinite(g).all(-1)
        if k % int(save_best_every) == 0:
            score(p, ok)
        gphi = g
        if lo is not None:
            s = sigmoid(phi)
            gphi = g * (hi - lo) * s * (one - s)
        gi = -gphi
        t = k + 1
        m_new = dtype(BETA1) * m + dtype(1 - BETA1) * gi
        v_new = dtype(BETA2) * v + dtype(1 - BETA2) * gi * gi
        step_size = dtype(learning_rate / (1.0 - BETA1 ** t))
        denom = np.sqrt(v_new) / dtype(np.sqrt(1.0 - BETA2 ** t)) + dtype(ADAM_EPS)
        phi_new = phi - step_size * (m_new / denom)
        okc = ok[:, None]
        m, v, phi = np.where(okc, m_new, m), np.where(okc, v_new, v), np.where(okc, phi_new, phi)
        theta = np.where(okc, to_theta(phi, lo, hi).astype(dtype), theta)
    p, _ = potential(theta, xr)
    p = np.asarray(p, dtype=np.float64)
    score(p, np.isfinite(p))
    bl = best_lp.reshape(N, R)
    j = np.argsort(-bl, axis=1, kind="stable")[:, 0]
    lp_map = bl[np.arange(N), j]
    th_map = best_th.reshape(N, R, D)[np.arange(N), j]
    found = np.isfinite(lp_map)
    return dict(theta_map=np.where(found[:, None], th_map, np.nan), log_prob_map=np.where(found, lp_map, np.nan),
                theta_last=theta.reshape(N, R, D), best_lp=bl, init_idx=idx, init_lp=p0)


# ---- known answer -----------------------------------------------------------------------------------------------------
def zero_maf_sigma(ospec):
    """A MAF with all-zero parameters is N(theta_mean, c theta_std): every transform multiplies u by the constant scale of
    a zero pre-activation, so c = scale ** -T."""
    a = torch.zeros(1, dtype=torch.float64)
    s = float(OF._scale_from_unconstrained(ospec, a))
    return np.asarray(ospec.theta_std, dtype=np.float64) * s ** (-ospec.T)


def gaussian_potential(mean, sigma):
    mean, sigma = np.asarray(mean, np.float64), np.asarray(sigma, np.float64)

    def fn(theta, x):
        z = (np.asarray(theta, np.float64) - mean) / sigma
        return -0.5 * (z * z).sum(-1) - np.log(sigma).sum() - 0.5 * len(mean) * np.log(2 * np.pi), -z / sigma
    return fn
