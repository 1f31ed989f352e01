"""Posterior-mode timings ("Posterior mode").

1. ``log_prob_grad`` rows/s beside ``log_prob`` rows/s on the same shapes: cfg1 MAF, cfg3 NSF and the production NSF
   (H = 69, T = 15, K = 10), random weights, HIP events around ``--rounds`` back-to-back calls after a warm-up.
2. ``map_catalogue`` per row beside the only route without the gradient kernel: central finite differences through
   ``sf_flow_log_prob`` (2 D evaluations per gradient) feeding the same ``sf_map_step``, on the same GPU in the same run.
3. One object (N = 1): wall time per iteration = the launch overhead of the per-iteration design.
4. ``sf_map_step`` beside the ``log_prob_grad`` call it follows, on the candidates of the N-object run (HIP events).

    python scripts/time_map.py [--rows 262144] [--rounds 20] [--objects 256] [--num-iter 200] [--json PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"maf_cfg1": ("maf", 5, 10, 50, 5, 10), "nsf_cfg3": ("nsf", 8, 20, 50, 5, 8), "nsf_prod": ("nsf", 8, 20, 69, 15, 10)}


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
    theta = rng.normal(size=(B, D)).astype(np.float32)
    x = rng.normal(size=(B, C)).astype(np.float32)
    return spec, flat, theta, x


def events(fn, rounds):
    fn(); fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rounds):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / rounds


def fd_map(flow, x, inits, lo, hi, num_iter, lr, h=1e-3):
    """The ascent of map_catalogue (R candidates per row) with central differences through log_prob for the gradient."""
    from synference_amd.map import map_step
    n, R, D = inits.shape
    th0 = inits.reshape(n * R, D)
    xr = x.repeat_interleave(R, 0).contiguous()
    u = ((th0 - lo) / (hi - lo)).clamp(1e-6, 1 - 1e-6)
    phi = (torch.log(u) - torch.log1p(-u)).contiguous()
    theta = (lo + (hi - lo) * torch.sigmoid(phi)).contiguous()
    m, v = torch.zeros_like(phi), torch.zeros_like(phi)
    best_lp = torch.full((n * R,), float("-inf"), device=theta.device)
    best_th = torch.full_like(theta, float("nan"))
    eye = torch.eye(D, device=theta.device) * h
    for k in range(num_iter):
        lp = flow.log_prob(theta, xr)
        g = torch.empty_like(theta)
        for d in range(D):
            g[:, d] = (flow.log_prob(theta + eye[d], xr) - flow.log_prob(theta - eye[d], xr)) / (2 * h)
        map_step(theta, lp, g, phi, m, v, lo, hi, best_th, best_lp, lr, k + 1, k % 10 == 0)
    return best_th, best_lp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--num-iter", type=int, default=200)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from synference_amd.engine import HipFlow
    from synference_amd.estimator import FlowEstimator
    from synference_amd.posterior import FlowPosterior
    from synference_amd.priors import CustomIndependentUniform
    out = {"device": torch.cuda.get_device_name(0), "rows": a.rows, "rounds": a.rounds}
    for name in SHAPES:
        spec, flat, theta, x = make(name, a.rows)
        f = HipFlow(spec, "cuda:0")
        f.set_params(torch.as_tensor(flat))
        th, xs = torch.as_tensor(theta).cuda(), torch.as_tensor(x).cuda()
        t_lp = events(lambda: f.log_prob(th, xs), a.rounds)
        t_fw = events(lambda: f.log_prob_grad(th, xs, want_grad=False), a.rounds)
        t_g = events(lambda: f.log_prob_grad(th, xs), a.rounds)
        R = 100
        xs_r = xs[: (a.rows + R - 1) // R].contiguous()
        t_gr = events(lambda: f.log_prob_grad(th, xs_r, rows_per_x=R), a.rounds)
        row = dict(log_prob_rows_per_s=a.rows / t_lp, grad_forward_only_rows_per_s=a.rows / t_fw,
                   log_prob_grad_rows_per_s=a.rows / t_g, log_prob_grad_shared_x_rows_per_s=a.rows / t_gr, ratio=t_g / t_lp)
        out[name] = row
        print(f"{name}: log_prob {row['log_prob_rows_per_s']:.3e} rows/s, log_prob_grad {row['log_prob_grad_rows_per_s']:.3e} rows/s "
              f"(x{row['ratio']:.2f}), forward half {row['grad_forward_only_rows_per_s']:.3e}, rows_per_x=100 "
              f"{row['log_prob_grad_shared_x_rows_per_s']:.3e}", flush=True)
        # ---- map_catalogue per row against finite differences
        N = a.objects
        lo, hi = -4 * torch.ones(spec.D), 4 * torch.ones(spec.D)
        post = FlowPosterior(FlowEstimator(spec, torch.as_tensor(flat), device="cuda:0").to("cuda:0"),
                             CustomIndependentUniform(lo, hi, device="cuda:0"))
        kw = dict(num_iter=a.num_iter, num_to_optimize=100, num_init_samples=1000, seed=1)
        post.map_catalogue(xs[:8], **dict(kw, num_iter=5))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        post.map_catalogue(xs[:N], **kw)
        torch.cuda.synchronize()
        t_map = time.perf_counter() - t0
        inits = post.sample_catalogue(xs[:N], 100, seed=1)
        lo_d, hi_d = lo.cuda(), hi.cuda()
        fd_map(f, xs[:8], inits[:8], lo_d, hi_d, 2, 0.01)
        torch.cuda.synchronize()
        n_fd = max(1, a.num_iter // 10)
        t0 = time.perf_counter()
        fd_map(f, xs[:N], inits, lo_d, hi_d, n_fd, 0.01)
        torch.cuda.synchronize()
        t_fd = (time.perf_counter() - t0) * a.num_iter / n_fd
        t0 = time.perf_counter()
        post.map_catalogue(xs[:1], **kw)
        torch.cuda.synchronize()
        t_one = time.perf_counter() - t0
        # ---- the ascent step beside the gradient call it follows, on the batch of the N-object run (N x 100 candidates)
        from synference_amd.map import map_step
        Bc = min(N * 100, a.rows)
        thc = th[:Bc].clone()
        xc = xs[: (Bc + 99) // 100].contiguous()
        lpc, gc = f.log_prob_grad(thc, xc, rows_per_x=100)
        phi, mom1, mom2 = torch.zeros_like(thc), torch.zeros_like(thc), torch.zeros_like(thc)
        bth, blp = torch.zeros_like(thc), torch.full((Bc,), float("-inf"), device=thc.device)
        t_step = events(lambda: map_step(thc, lpc, gc, phi, mom1, mom2, lo_d, hi_d, bth, blp, 0.01, 1, True), a.rounds * 5)
        t_gradc = events(lambda: f.log_prob_grad(th[:Bc], xc, rows_per_x=100), a.rounds * 5)
        row.update(map_step_us=t_step * 1e6, log_prob_grad_same_batch_us=t_gradc * 1e6, step_batch=Bc)
        print(f"{name}: sf_map_step {t_step * 1e6:.1f} us beside log_prob_grad {t_gradc * 1e6:.1f} us on {Bc} candidates", flush=True)
        row.update(map_s_per_row=t_map / N, fd_map_s_per_row=t_fd / N, map_one_object_s=t_one,
                   one_object_us_per_iter=t_one / a.num_iter * 1e6, objects=N, num_iter=a.num_iter)
        print(f"{name}: map_catalogue {t_map / N * 1e3:.3f} ms/row ({N} rows, {a.num_iter} iterations, 100 candidates), finite "
              f"differences {t_fd / N * 1e3:.3f} ms/row (x{t_fd / t_map:.1f}; {n_fd} iterations timed, scaled); one object "
              f"{t_one * 1e3:.1f} ms = {t_one / a.num_iter * 1e6:.0f} us per iteration", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
