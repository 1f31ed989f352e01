"""Posterior mode (MAP) on the device: [UPSTREAM] sbi ``DirectPosterior.map`` / ``EnsemblePosterior.map`` ->
``gradient_ascent``, for whole catalogues.

Per catalogue row: ``num_init_samples`` accepted posterior draws, the ``num_to_optimize`` most probable of them
ascend ``log q(theta | x)`` for ``num_iter`` Adam steps in the unconstrained coordinates of the prior box, and the
best point seen is the row's mode.  One iteration is one ``sf_flow_log_prob_grad`` launch per ensemble member over
all rows x candidates (the candidates of a row share its context row: ``rows_per_x``) and one ``sf_map_step`` launch.
The algorithm is pinned by ``tests/map_model.py``; its deviation from upstream (the value computed for the step is
the value that is scored, plus one evaluation after the last step) is described in DESIGN.md, "Posterior mode".

Row blocks: a block holds at most ``MAP_BLOCK_DRAWS`` init draws (N_block x num_init_samples), so that the
``[N, num_init_samples, D]`` array of a large catalogue never exists at once (2^22 draws: 256 MiB at D = 16).  Rows
are independent and the random streams are keyed by the row's position in the whole catalogue, so the result does
not depend on the block size.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib

MAP_BLOCK_DRAWS = 1 << 22

_U_EPS = 1e-6   # [UPSTREAM] the box transform's clamp of (theta - lo) / (hi - lo)


def check_map_args(num_iter, num_to_optimize, learning_rate, init_method, num_init_samples, save_best_every):
    """Argument validation shared by map() / map_catalogue() / calculate_MAP (no GPU needed)."""
    if int(num_iter) < 0:
        raise ValueError("num_iter must be >= 0")
    if int(num_to_optimize) < 1:
        raise ValueError("num_to_optimize must be >= 1")
    if int(num_init_samples) < 1:
        raise ValueError("num_init_samples must be >= 1")
    if int(save_best_every) < 1:
        raise ValueError("save_best_every must be >= 1")
    if not float(learning_rate) > 0.0:
        raise ValueError("learning_rate must be > 0")
    if isinstance(init_method, str):
        if init_method not in ("posterior", "proposal"):
            raise ValueError(f"init_method '{init_method}': 'posterior', 'proposal' or an (N, R0, D) tensor of inits")
    elif not torch.is_tensor(init_method) or init_method.dim() != 3:
        raise ValueError("init_method must be 'posterior', 'proposal' or an (N, R0, D) tensor of inits")


def _stable_top(key: torch.Tensor, k: int) -> torch.Tensor:
    """Indices of the k largest entries per row, lower index first on ties."""
    return torch.sort(key, dim=1, descending=True, stable=True).indices[:, :k]


def map_step(theta, lp, g, phi, m, v, lo, hi, best_theta, best_lp, learning_rate: float, step: int, save_best: bool):
    """One fused ascent step (sf_map_step) on contiguous float32 device tensors; ``g`` None: score only."""
    p = _lib.ptr
    B, D = theta.shape
    with torch.cuda.device(theta.device):
        st = _lib.stream_ptr(theta.device)
        _lib.check(_lib.load().sf_map_step(B, D, p(phi), p(m), p(v), p(theta), p(lp), p(g), p(lo), p(hi), p(best_theta),
                                           p(best_lp), C.c_float(float(learning_rate)), int(step), 1 if save_best else 0, st))


class _Potential:
    """log q and its theta gradient for R candidates per context row: one flow, or the mixture
    logsumexp_e(log w_e + lp_e) with the softmax-weighted sum of the members' gradients."""

    def __init__(self, posteriors: Sequence, weights: Optional[torch.Tensor], X):
        self.flows, self.ctx = [], []
        for p in posteriors:
            est = p.posterior_estimator
            if not est.flow.supports_log_prob_grad():
                raise NotImplementedError(f"map: the flow kind '{est.spec.kind}' (D = {est.spec.D}) has no theta-gradient kernel "
                                          "(built: maf, and nsf with D >= 2)")
            self.ctx.append(p._embed(X))
            est._sync_params()
            self.flows.append(est.flow)
        self.logw = None
        if len(self.flows) > 1:
            self.logw = torch.log(torch.as_tensor(weights, dtype=torch.float32, device=self.ctx[0].device))[:, None]

    def __call__(self, theta, r0: int, r1: int, rows_per_x: int, want_grad: bool):
        if self.logw is None:
            return self.flows[0].log_prob_grad(theta, self.ctx[0][r0:r1], rows_per_x, True, want_grad)
        outs = [f.log_prob_grad(theta, c[r0:r1], rows_per_x, True, want_grad) for f, c in zip(self.flows, self.ctx)]
        a = torch.stack([o[0] for o in outs], 0) + self.logw
        lp = torch.logsumexp(a, dim=0)
        if not want_grad:
            return lp, None
        w = torch.softmax(a, dim=0)
        return lp, (w[:, :, None] * torch.stack([o[1] for o in outs], 0)).sum(0).contiguous()


def map_catalogue(owner, posteriors, weights, X, num_iter=1000, num_to_optimize=100, learning_rate=0.01,
                  init_method="posterior", num_init_samples=1000, save_best_every=10, seed=None, row_offset=0):
    """(theta_map [N, D], log_prob_map [N]) float32 device tensors; ``owner`` draws the inits (``sample_catalogue``) and
    carries the prior box.  See FlowPosterior.map_catalogue."""
    check_map_args(num_iter, num_to_optimize, learning_rate, init_method, num_init_samples, save_best_every)
    dev = owner.device
    X = torch.as_tensor(X, dtype=torch.float32, device=dev)
    X = X[None, :] if X.dim() == 1 else X
    N, D = X.shape[0], posteriors[0].spec.D
    explicit = torch.is_tensor(init_method)
    if explicit:
        inits = init_method.to(device=dev, dtype=torch.float32)
        if inits.shape[0] != N or inits.shape[2] != D:
            raise ValueError(f"init tensor {tuple(inits.shape)} does not match (N = {N}, R0, D = {D})")
        R0 = inits.shape[1]
    else:
        R0 = int(num_init_samples)
    R = min(int(num_to_optimize), R0)
    pot = _Potential(posteriors, weights, X)
    prior = owner.prior
    lo = hi = None
    if prior is not None:
        lo, hi = prior.low.to(dev).float().contiguous(), prior.high.to(dev).float().contiguous()
    if not explicit:
        seed = owner._next_seed(seed)
    theta_map = torch.full((N, D), float("nan"), dtype=torch.float32, device=dev)
    lp_map = torch.full((N,), float("nan"), dtype=torch.float32, device=dev)
    rows_per = max(1, MAP_BLOCK_DRAWS // max(R0, 1))
    ninf = float("-inf")
    for r0 in range(0, N, rows_per):
        r1 = min(N, r0 + rows_per)
        n = r1 - r0
        # ---- 1. inits: the R most probable of R0 draws (NaN last, lower index first on ties)
        if explicit:
            draws = inits[r0:r1].contiguous()
        else:
            draws = owner.sample_catalogue(X[r0:r1], R0, seed=seed, row_offset=int(row_offset) + r0)
        lp0, _ = pot(draws.reshape(n * R0, D), r0, r1, R0, False)
        lp0 = lp0.reshape(n, R0)
        lp0 = torch.where(torch.isfinite(lp0), lp0, torch.full_like(lp0, ninf))
        top = _stable_top(lp0, R)
        th0 = torch.gather(draws, 1, top[:, :, None].expand(n, R, D)).reshape(n * R, D)
        lp_init = torch.gather(lp0, 1, top).reshape(n * R)
        # ---- 2. unconstrained coordinates; the first iterate is theta(phi_0)
        if lo is not None:
            u = ((th0 - lo) / (hi - lo)).clamp(_U_EPS, 1.0 - _U_EPS)
            phi = (torch.log(u) - torch.log1p(-u)).contiguous()
            theta = (lo + (hi - lo) * torch.sigmoid(phi)).contiguous()
            inside = ((th0 >= lo) & (th0 <= hi)).all(-1)
        else:
            phi = th0.clone()
            theta = th0.clone()
            inside = torch.ones(n * R, dtype=torch.bool, device=dev)
        # a candidate starts with its init as its best (an init outside the box is only a starting point)
        keep = inside & torch.isfinite(lp_init)
        best_lp = torch.where(keep, lp_init, torch.full_like(lp_init, ninf)).contiguous()
        best_theta = torch.where(keep[:, None], th0, torch.full_like(th0, float("nan"))).contiguous()
        theta = torch.where(torch.isfinite(lp_init)[:, None], theta, torch.full_like(theta, float("nan"))).contiguous()
        m, v = torch.zeros_like(phi), torch.zeros_like(phi)
        # ---- 3. ascent
        for k in range(int(num_iter)):
            lp, g = pot(theta, r0, r1, R, True)
            map_step(theta, lp, g, phi, m, v, lo, hi, best_theta, best_lp, learning_rate, k + 1,
                     k % int(save_best_every) == 0)
        # ---- 4. the point after the last step, then the best candidate of the row (lowest index on ties)
        lp, _ = pot(theta, r0, r1, R, False)
        map_step(theta, lp, None, None, None, None, lo, hi, best_theta, best_lp, learning_rate, 1, True)
        best_lp = best_lp.reshape(n, R)
        j = _stable_top(best_lp, 1)
        lpj = torch.gather(best_lp, 1, j)[:, 0]
        thj = torch.gather(best_theta.reshape(n, R, D), 1, j[:, :, None].expand(n, 1, D))[:, 0]
        found = torch.isfinite(lpj)
        theta_map[r0:r1] = torch.where(found[:, None], thj, torch.full_like(thj, float("nan")))
        lp_map[r0:r1] = torch.where(found, lpj, torch.full_like(lpj, float("nan")))
    return theta_map, lp_map


def map_one(self, x=None, num_iter=1000, num_to_optimize=100, learning_rate=0.01, init_method="posterior",
            num_init_samples=1000, save_best_every=10, show_progress_bars=False, force_update=False, seed=None):
    """[UPSTREAM] ``posterior.map(x=...)`` for ONE observation -> theta [D]; ``show_progress_bars`` and
    ``force_update`` are accepted and ignored (nothing is cached)."""
    if torch.is_tensor(init_method) and init_method.dim() == 2:
        init_method = init_method[None]
    check_map_args(num_iter, num_to_optimize, learning_rate, init_method, num_init_samples, save_best_every)
    if x is None:
        raise ValueError("map() needs the observation x (this posterior keeps no default x)")
    x = torch.as_tensor(x, dtype=torch.float32)
    x = x[None, :] if x.dim() == 1 else x
    if x.shape[0] != 1:
        raise ValueError("map() takes ONE observation; use map_catalogue() for a catalogue")
    theta, lp = self.map_catalogue(x, num_iter, num_to_optimize, learning_rate, init_method, num_init_samples,
                                   save_best_every, seed)
    self.last_map_log_prob = lp[0]
    return theta[0]
