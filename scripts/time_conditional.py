"""Conditional-posterior timings.

Per shape (cfg1 MAF, cfg3 NSF; random weights), ``--rows`` catalogue rows x ``--draws`` conditional draws with the defaults
(64 walkers, burn_in 200, thin 5, 1000 starts), one coordinate fixed:

1. ``sample_conditional_catalogue`` end to end: HIP events around ``--rounds`` synchronised calls after one warm-up call of the
   same shape.
2. Where the time goes: ``sf_stretch_step`` (resolve + propose, the launch of an ordinary half-step) beside the density
   launch it alternates with, each on the chain's own shapes (rows x 64 walkers, rows x 32 proposals sharing their context
   row), HIP events around back-to-back calls.
3. The same chain with the step done in torch elementwise ops (gather, where, log, compare: ``torch_chain``) feeding the same
   density launches, for comparison.  It draws its random numbers from torch's generator, so it is the same amount of work,
   not the same draws.

    python scripts/time_conditional.py [--rows 1000] [--draws 1000] [--rounds 3] [--json PATH]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"maf_cfg1": ("maf", 5, 10, 50, 5, 10), "nsf_cfg3": ("nsf", 8, 20, 50, 5, 8)}
W, BURN, THIN, R0 = 64, 200, 5, 1000


def make(name, B, seed=0):
    from oracle import flows as OF
    from synference_amd.spec import FlowSpec
    kind, D, C, H, T, K = SHAPES[name]
    rng = np.random.default_rng(seed)
    perms = OF.random_perms(D, T, seed) if kind == "maf" else None
    st = dict(theta_mean=np.zeros(D, np.float32), theta_std=np.ones(D, np.float32), x_mean=np.zeros(C, np.float32),
              x_std=np.ones(C, np.float32))
    ospec = OF.FlowSpec(kind=kind, D=D, C=C, H=H, T=T, K=K, perms=perms, **{k: v.astype(np.float64) for k, v in st.items()})
    spec = FlowSpec(kind=kind, D=D, C=C, H=H, T=T, K=K, perms=perms, **st)
    flat = OF.init_params(ospec, seed + 1).astype(np.float32)
    return spec, flat, rng.normal(size=(B, C)).astype(np.float32)


def events(fn, rounds, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rounds):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / rounds


def torch_chain(flow, x, walkers, lp, free, lo, hi, n_free, steps):
    """``steps`` stretch-move steps on walkers [n, W, D] with torch elementwise ops; ``free`` [n, D] float mask."""
    n, Wk, D = walkers.shape
    W2 = Wk // 2
    for _ in range(steps):
        for h in (0, 1):
            act, oth = walkers[:, h::2], walkers[:, 1 - h::2]
            j = torch.randint(0, W2, (n, W2), device=walkers.device)
            tj = torch.gather(oth, 1, j[:, :, None].expand(n, W2, D))
            z = (torch.rand((n, W2), device=walkers.device) + 1.0) ** 2 * 0.5
            y = torch.where(free[:, None, :] > 0, tj + z[:, :, None] * (act - tj), act).contiguous()
            lpy = flow.log_prob_grad(y.reshape(n * W2, D), x, W2, True, False)[0].reshape(n, W2)
            inside = ((y >= lo) & (y <= hi)).all(-1)
            ok = inside & torch.isfinite(lpy) & (torch.log(torch.rand((n, W2), device=walkers.device))
                                                 < (n_free[:, None] - 1.0) * torch.log(z) + lpy - lp[:, h::2])
            walkers[:, h::2] = torch.where(ok[:, :, None], y, act)
            lp[:, h::2] = torch.where(ok, lpy, lp[:, h::2])
    return walkers, lp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_conditional.py measures on the GPU: no device visible")
    from synference_amd.conditional import n_steps, stretch_step
    from synference_amd.estimator import FlowEstimator
    from synference_amd.posterior import FlowPosterior
    from synference_amd.priors import CustomIndependentUniform
    out = {"device": torch.cuda.get_device_name(0), "rows": a.rows, "draws": a.draws, "rounds": a.rounds,
           "walkers": W, "burn_in": BURN, "thin": THIN}
    for name in SHAPES:
        spec, flat, x = make(name, a.rows)
        D, N, W2 = spec.D, a.rows, W // 2
        lo, hi = -4 * torch.ones(D), 4 * torch.ones(D)
        post = FlowPosterior(FlowEstimator(spec, torch.as_tensor(flat), device="cuda:0").to("cuda:0"),
                             CustomIndependentUniform(lo, hi, device="cuda:0"))
        flow = post.posterior_estimator.flow
        xs = torch.as_tensor(x).cuda()
        cond = np.full((N, D), np.nan, dtype=np.float32)
        cond[:, 0] = 0.25
        steps = n_steps(a.draws, W, BURN, THIN)
        call = lambda: post.sample_conditional_catalogue(xs, cond, num_samples=a.draws, seed=1)
        t_call = events(call, a.rounds, warm=1)
        _, acc = call()
        # ---- the two launches of a half-step on the chain's shapes
        walkers = post.sample_catalogue(xs, W, seed=2).contiguous()
        walkers[:, :, 0] = 0.25
        lp = flow.log_prob_grad(walkers.reshape(N * W, D), xs, W, True, False)[0].reshape(N, W).contiguous()
        fx = torch.ones(N, dtype=torch.int32, device="cuda:0")
        prop = walkers[:, ::2].clone().contiguous()
        accepted = torch.zeros(N, dtype=torch.int32, device="cuda:0")
        lo_d, hi_d = lo.cuda(), hi.cuda()
        lp_prop = flow.log_prob_grad(prop.reshape(N * W2, D), xs, W2, True, False)[0]
        t_step = events(lambda: stretch_step(walkers, lp, fx, lo_d, hi_d, lp_prop, prop, accepted, None, None, -1, 1, 0, 3,
                                             True, True, 1), 200)
        t_dens = events(lambda: flow.log_prob_grad(prop.reshape(N * W2, D), xs, W2, True, False), 200)
        # ---- the chain alone, kernel step against torch ops (the starts are not part of either)
        free = torch.ones((N, D), device="cuda:0")
        free[:, 0] = 0.0
        n_free = torch.full((N,), float(D - 1), device="cuda:0")

        def kernel_chain():
            for k in range(2 * steps + 1):
                lpp = flow.log_prob_grad(prop.reshape(N * W2, D), xs, W2, True, False)[0] if k > 0 else None
                stretch_step(walkers, lp, fx, lo_d, hi_d, lpp, prop, accepted, None, None, -1, 1, 0, k, k > 0, k < 2 * steps, 1)
        t_kchain = events(kernel_chain, a.rounds, warm=1)
        t_tchain = events(lambda: torch_chain(flow, xs, walkers, lp, free, lo_d, hi_d, n_free, steps), a.rounds, warm=1)
        row = dict(call_s=t_call, steps=steps, draws_per_s=N * a.draws / t_call, acceptance=float(acc.mean()),
                   stretch_step_us=t_step * 1e6, density_us=t_dens * 1e6, step_share=t_step / (t_step + t_dens),
                   kernel_chain_s=t_kchain, torch_chain_s=t_tchain)
        out[name] = row
        print(f"{name}: {N} rows x {a.draws} draws in {t_call * 1e3:.1f} ms ({row['draws_per_s']:.3e} draws/s, {steps} steps, "
              f"acceptance {row['acceptance']:.3f}); sf_stretch_step {t_step * 1e6:.1f} us beside the density launch "
              f"{t_dens * 1e6:.1f} us ({100 * row['step_share']:.1f} % of a half-step); the chain alone {t_kchain * 1e3:.1f} ms "
              f"against {t_tchain * 1e3:.1f} ms with the step in torch ops (x{t_tchain / t_kchain:.2f})", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
