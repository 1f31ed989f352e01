"""Conditional posteriors on the device: draws from ``q(theta_free | theta_fixed, x)`` for whole catalogues.

[UPSTREAM] sbi reaches this through ``sbi.analysis.conditional_potential(..., condition, dims_to_sample)`` behind an MCMC
posterior -- one Python chain per object.  Here every catalogue row runs an ensemble of ``W`` walkers with the
affine-invariant stretch move (Goodman & Weare 2010, emcee's default move) on the slice of the joint density: one
``sf_stretch_step`` launch per half-step over all rows x walkers, and between two launches one density evaluation of the
``W / 2`` proposals of every row (the proposals of a row share its context row: ``rows_per_x``, where the kind has the
forward half of ``sf_flow_log_prob_grad``; ``sf_flow_log_prob`` on repeated context rows otherwise).  The algorithm is
pinned by ``tests/stretch_model.py`` and written down in DESIGN.md section 19.

Row blocks: a block holds at most ``BLOCK_DRAWS`` init draws; rows are independent and every random stream is keyed by
the row's position in the whole catalogue, so the result does not depend on the blocking.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .map import _stable_top

BLOCK_DRAWS = 1 << 22
STREAM_STRETCH = 0x53545200          # csrc/sf_stretch.hip: key = (seed_lo, seed_hi ^ STREAM_STRETCH)
INIT_SEED_OFFSET = 0xA0761D6478BD642F    # the starting draws use a seed stream of their own
MAX_WALKERS, MIN_WALKERS, DMAX = 64, 4, 16


def check_conditional_args(num_samples, num_walkers, burn_in, thin, num_init_samples):
    """Argument validation shared by the whole surface (no GPU needed)."""
    W = int(num_walkers)
    if int(num_samples) < 1:
        raise ValueError("num_samples must be >= 1")
    if W % 2 or W < MIN_WALKERS or W > MAX_WALKERS:
        raise ValueError(f"num_walkers = {W}: an even number in {MIN_WALKERS}..{MAX_WALKERS}")
    if int(burn_in) < 0:
        raise ValueError("burn_in must be >= 0")
    if int(thin) < 1:
        raise ValueError("thin must be >= 1")
    if int(num_init_samples) < W:
        raise ValueError(f"num_init_samples = {int(num_init_samples)} cannot fill num_walkers = {W} starts")


def plan_rows(condition, dims_to_sample, N: int, D: int, lo=None, hi=None, num_walkers: int = 64):
    """condition (N, D) or (D,), NaN = free in that row; ``dims_to_sample`` frees those dimensions in every row ->
    (values float32 [N, D], fixed int32 [N]): bit d of ``fixed`` set = coordinate d is fixed; ``fixed`` is -1 for a row
    that cannot be sampled (a fixed value that is not finite or lies outside the prior box: a NaN row), 0 for a row with
    nothing fixed.  Raises for a row without a free coordinate and for fewer walkers than 2 n_free + 2."""
    if D < 1 or D > DMAX:
        raise ValueError(f"D = {D}: the conditional sampler takes 1..{DMAX} parameters")
    c = np.array(condition, dtype=np.float32)
    if c.ndim == 1:
        c = np.broadcast_to(c[None, :], (N, c.shape[0])).copy()
    if c.shape != (N, D):
        raise ValueError(f"condition {tuple(np.shape(condition))} does not match (N = {N}, D = {D}) or (D = {D},)")
    if dims_to_sample is not None:
        dims = np.atleast_1d(np.asarray(dims_to_sample, dtype=np.int64))
        if dims.size and (dims.min() < -D or dims.max() >= D):
            raise ValueError(f"dims_to_sample {dims.tolist()} outside the D = {D} parameters")
        c[:, dims] = np.nan
    mask = ~np.isnan(c)
    n_free = D - mask.sum(1)
    if (n_free < 1).any():
        raise ValueError(f"row {int(np.flatnonzero(n_free < 1)[0])}: every parameter is fixed -- a conditional draw needs at "
                         "least one free coordinate")
    cond_rows = n_free < D
    W = int(num_walkers)
    if cond_rows.any() and W < 2 * int(n_free[cond_rows].max()) + 2:
        raise ValueError(f"num_walkers = {W} for {int(n_free[cond_rows].max())} free coordinates: the stretch move needs at "
                         f"least 2 n_free + 2 = {2 * int(n_free[cond_rows].max()) + 2} walkers")
    fixed = (mask.astype(np.int64) << np.arange(D)[None, :]).sum(1).astype(np.int32)
    dead = (mask & ~np.isfinite(c)).any(1)
    if lo is not None:
        lo32, hi32 = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
        with np.errstate(invalid="ignore"):
            dead |= (mask & ((c < lo32) | (c > hi32))).any(1)
    fixed[dead] = -1
    return c, fixed


def stretch_step(walkers, lp, fixed, lo, hi, lp_prop, prop, accepted, out, out_lp, collect: int, seed: int,
                 row_offset: int, half_step: int, resolve: bool, propose: bool, max_fixed: int,
                 trace_partner=None, trace_accept=None):
    """One half-step (sf_stretch_step) on contiguous device tensors: walkers [N, W, D], lp [N, W], fixed int32 [N],
    prop [N, W/2, D], lp_prop [N, W/2], accepted int32 [N], out [N, S, D] / out_lp [N, S] (``collect`` < 0: none)."""
    p = _lib.ptr
    N, W, D = walkers.shape
    S = 0 if out is None else out.shape[1]
    with torch.cuda.device(walkers.device):
        st = _lib.stream_ptr(walkers.device)
        _lib.check(_lib.load().sf_stretch_step(N, D, W, int(max_fixed), p(walkers), p(lp), p(fixed), p(lo), p(hi), p(lp_prop),
                                               p(prop), p(accepted), p(out), p(out_lp), S, int(collect),
                                               C.c_uint64(int(seed) & (2 ** 64 - 1)), int(row_offset), int(half_step),
                                               1 if resolve else 0, 1 if propose else 0, p(trace_partner), p(trace_accept), st))


class _Density:
    """log q for R points per context row: one flow, or the mixture logsumexp_e(log w_e + lp_e) (as map._Potential, without
    the gradient and for every flow kind)."""

    def __init__(self, posteriors: Sequence, weights: Optional[torch.Tensor], X):
        self.flows, self.ctx = [], []
        for p in posteriors:
            est = p.posterior_estimator
            self.ctx.append(p._embed(X))
            est._sync_params()
            self.flows.append(est.flow)
        self.logw = None
        if len(self.flows) > 1:
            self.logw = torch.log(torch.as_tensor(weights, dtype=torch.float32, device=self.ctx[0].device))[:, None]
        self._rep = {}

    def _one(self, e, theta, r0, r1, R):
        f, c = self.flows[e], self.ctx[e]
        if f.supports_log_prob_grad():
            return f.log_prob_grad(theta, c[r0:r1], R, True, False)[0]
        key = (e, r0, r1, R)     # the one-parameter NSF and the lampe kinds: repeated context rows, built once per block
        if key not in self._rep:
            self._rep = {k: v for k, v in self._rep.items() if k[0] != e}
            self._rep[key] = c[r0:r1].repeat_interleave(R, 0).contiguous()
        return f.log_prob(theta, self._rep[key])

    def __call__(self, theta, r0: int, r1: int, R: int):
        if self.logw is None:
            return self._one(0, theta, r0, r1, R)
        a = torch.stack([self._one(e, theta, r0, r1, R) for e in range(len(self.flows))], 0) + self.logw
        return torch.logsumexp(a, dim=0)


def n_steps(S: int, W: int, burn_in: int, thin: int) -> int:
    return int(burn_in) + (-(-int(S) // int(W))) * int(thin)


def _runs(flags: np.ndarray):
    """[a, b) blocks of consecutive True entries."""
    e = np.flatnonzero(np.diff(np.concatenate([[False], flags, [False]]).astype(np.int8)))
    return list(zip(e[0::2].tolist(), e[1::2].tolist()))


def conditional_catalogue(owner, posteriors, weights, X, condition, dims_to_sample=None, num_samples=1000, num_walkers=64,
                          burn_in=200, thin=5, num_init_samples=1000, seed=None, row_offset=0, return_log_prob=False,
                          _trace=False):
    """(samples [N, S, D], acceptance [N]) float32 device tensors (plus lp [N, S], the raw density at the draws, with
    ``return_log_prob``); ``owner`` draws the starts (``sample_catalogue``) and carries the prior box.  Rows with nothing
    fixed are ``sample_catalogue``'s exact draws with acceptance 1.  See FlowPosterior.sample_conditional_catalogue.
    ``_trace`` (tests): also a list with one dict per block and half-step -- the walkers and lp the proposals were made
    from, the proposals, their partners, their device lp and the accept flags."""
    check_conditional_args(num_samples, num_walkers, burn_in, thin, num_init_samples)
    D = posteriors[0].spec.D
    Xh = X if torch.is_tensor(X) else torch.as_tensor(np.asarray(X, dtype=np.float32))
    Xh = Xh[None, :] if Xh.dim() == 1 else Xh
    N = Xh.shape[0]
    prior = owner.prior
    lo_h = hi_h = None
    if prior is not None:
        lo_h, hi_h = prior.low.detach().cpu().float().numpy(), prior.high.detach().cpu().float().numpy()
    values, fixed = plan_rows(condition, dims_to_sample, N, D, lo_h, hi_h, num_walkers)
    dev = owner.device
    X = Xh.to(device=dev, dtype=torch.float32)
    S, W, R0 = int(num_samples), int(num_walkers), int(num_init_samples)
    W2 = W // 2
    seed = owner._next_seed(seed)
    init_seed = (seed + INIT_SEED_OFFSET) & (2 ** 63 - 1)
    samples = torch.full((N, S, D), float("nan"), dtype=torch.float32, device=dev)
    acceptance = torch.full((N,), float("nan"), dtype=torch.float32, device=dev)
    lp_out = torch.full((N, S), float("nan"), dtype=torch.float32, device=dev) if return_log_prob else None
    trace = [] if _trace else None
    pot = _Density(posteriors, weights, X)
    # ---- rows with nothing fixed: exact draws
    for a, b in _runs(fixed == 0):
        samples[a:b] = owner.sample_catalogue(X[a:b], S, seed=seed, row_offset=int(row_offset) + a)
        acceptance[a:b] = 1.0
        if return_log_prob:
            lp_out[a:b] = pot(samples[a:b].reshape((b - a) * S, D), a, b, S).reshape(b - a, S)
    # ---- conditioned rows (the dead ones among them travel along: the kernel skips them)
    if not (fixed != 0).any():
        return _result(samples, acceptance, lp_out, trace, return_log_prob, _trace)
    lo = hi = None
    if prior is not None:
        lo, hi = prior.low.to(dev).float().contiguous(), prior.high.to(dev).float().contiguous()
    bits = np.where(fixed > 0, fixed, 0)
    max_fixed = int(max(bin(int(v)).count("1") for v in np.unique(bits)))
    T = n_steps(S, W, burn_in, thin)
    rows_per = max(1, BLOCK_DRAWS // R0)
    for ra, rb in _runs(fixed != 0):
        for a in range(ra, rb, rows_per):
            b = min(rb, a + rows_per)
            n = b - a
            val = torch.as_tensor(values[a:b], device=dev)
            fx = torch.as_tensor(fixed[a:b], device=dev)
            fm = ((fx.clamp_min(0)[:, None] >> torch.arange(D, device=dev)[None, :]) & 1).bool()
            # ---- 1. starts: the W most probable of R0 unconditional draws moved onto the slice (NaN last, stable)
            draws = owner.sample_catalogue(X[a:b], R0, seed=init_seed, row_offset=int(row_offset) + a)
            draws = torch.where(fm[:, None, :], val[:, None, :], draws).contiguous()
            lp0 = pot(draws.reshape(n * R0, D), a, b, R0).reshape(n, R0)
            lp0 = torch.where(torch.isfinite(lp0), lp0, torch.full_like(lp0, float("-inf")))
            top = _stable_top(lp0, W)
            walkers = torch.gather(draws, 1, top[:, :, None].expand(n, W, D)).contiguous()
            lp = torch.gather(lp0, 1, top).contiguous()
            del draws, lp0
            alive = (fx > 0) & torch.isfinite(lp).all(1)
            fx = torch.where(alive, fx, torch.full_like(fx, -1)).contiguous()
            # ---- 2. the chain: call k resolves half-step k - 1, collects, proposes half-step k
            prop = torch.zeros((n, W2, D), dtype=torch.float32, device=dev)
            accepted = torch.zeros(n, dtype=torch.int32, device=dev)
            out, out_lp = samples[a:b], (lp_out[a:b] if return_log_prob else None)
            tp = ta = None
            if _trace:
                tp = torch.zeros((n, W2), dtype=torch.int32, device=dev)
                ta = torch.zeros((n, W2), dtype=torch.int32, device=dev)
            lp_prop = None
            for k in range(2 * T + 1):
                if k > 0:
                    lp_prop = pot(prop.reshape(n * W2, D), a, b, W2)
                done = k // 2
                collect = -1
                if k % 2 == 0 and done > burn_in and (done - burn_in) % int(thin) == 0:
                    collect = (done - burn_in) // int(thin) - 1
                stretch_step(walkers, lp, fx, lo, hi, lp_prop, prop, accepted, out, out_lp, collect, seed,
                             int(row_offset) + a, k, k > 0, k < 2 * T, max_fixed, tp, ta)
                if _trace:
                    if k > 0:
                        trace[-1].update(lp_prop=lp_prop.reshape(n, W2).clone(), accept=ta.clone())
                    if k < 2 * T:
                        trace.append(dict(row0=a, row1=b, half_step=k, walkers=walkers.clone(), lp=lp.clone(),
                                          prop=prop.clone(), partner=tp.clone(), fixed=fx.clone()))
            acceptance[a:b] = torch.where(alive, accepted.float() / float(max(T, 1) * W),
                                          torch.full((n,), float("nan"), device=dev))
    return _result(samples, acceptance, lp_out, trace, return_log_prob, _trace)


def _result(samples, acceptance, lp_out, trace, return_log_prob, _trace):
    res = (samples, acceptance) + ((lp_out,) if return_log_prob else ()) + ((trace,) if _trace else ())
    return res


def sample_conditional_one(self, sample_shape=(1,), x=None, condition=None, dims_to_sample=None, seed=None, **kw):
    """[UPSTREAM] the conditional-potential posterior's ``.sample(sample_shape, x=)`` for ONE observation ->
    (*sample_shape, D); ``condition`` is a (D,) vector (NaN = free), ``dims_to_sample`` frees those dimensions."""
    if x is None or condition is None:
        raise ValueError("sample_conditional() needs the observation x and the condition")
    shape = tuple(sample_shape)
    S = int(np.prod(shape)) if len(shape) else 1
    x = torch.as_tensor(x, dtype=torch.float32)
    x = x[None, :] if x.dim() == 1 else x
    if x.shape[0] != 1:
        raise ValueError("sample_conditional() takes ONE observation; use sample_conditional_catalogue() for a catalogue")
    cond = np.asarray(torch.as_tensor(condition).detach().cpu().numpy(), dtype=np.float32).reshape(-1)
    out, acc = self.sample_conditional_catalogue(x, cond, dims_to_sample=dims_to_sample, num_samples=S, seed=seed, **kw)
    self.last_conditional_acceptance = acc[0]
    return out[0].reshape(*shape, out.shape[-1])
