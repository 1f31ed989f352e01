"""Writes tests/golden/conditional/<case>.npz: what the distribution test of the conditional sampler
(tests/test_gpu_conditional.py) compares against -- needs no GPU.

Per case (a flow of tests/cases.py, one observation x, coordinate 0 fixed at a test-set value, the box of the tests):
  * the quadrature CDF of every free marginal of the ORACLE's conditional density q(theta_free | theta_fixed, x) restricted to
    the box: the density on a grid over the free coordinates (fp64 oracle), trapezoid sums;
  * the KS distances that the MODEL (tests/stretch_model.py, fp64, the oracle's density) reaches against that CDF with the
    default settings -- 16 rows of the same x pooled, W = 64, burn_in = 200, thin = 5, S = 1024, 1000 starts -- for 8 seeds,
    with its acceptance.  1.5 x the largest of the eight is the device's threshold.

    python tests/golden/make_conditional_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import stretch_model as SM  # noqa: E402
from cases import make_case, oracle_log_prob  # noqa: E402
from oracle import posterior as OP  # noqa: E402

CASES = {"maf_small": 4001, "nsf_d2": 4001, "maf_d3": 641}      # grid points per free coordinate
ROWS, W, BURN, THIN, S, R0 = 16, 64, 200, 5, 1024, 1000
SEEDS = tuple(range(101, 109))
FIXED_D = 0


def box(ospec):
    std, mean = np.asarray(ospec.theta_std, np.float64), np.asarray(ospec.theta_mean, np.float64)
    return mean - 4 * std, mean + 4 * std


def conditional_cdfs(ospec, flat, x_row, value, lo, hi, G):
    """(grids [n_free, G], cdfs [n_free, G]) of the free marginals of q(. | theta_FIXED_D = value, x) inside the box."""
    D = ospec.D
    free = [d for d in range(D) if d != FIXED_D]
    grids = np.stack([np.linspace(lo[d], hi[d], G) for d in free])
    mesh = np.meshgrid(*grids, indexing="ij")
    pts = np.empty((mesh[0].size, D))
    pts[:, FIXED_D] = value
    for k, d in enumerate(free):
        pts[:, d] = mesh[k].reshape(-1)
    lp = np.concatenate([oracle_log_prob(ospec, flat, pts[i:i + 65536], np.repeat(x_row[None], len(pts[i:i + 65536]), 0))
                         for i in range(0, len(pts), 65536)])
    dens = np.exp(lp - lp.max()).reshape(mesh[0].shape)
    cdfs = []
    for k in range(len(free)):
        m = dens
        for ax in reversed([a for a in range(len(free)) if a != k]):
            m = (getattr(np, "trapezoid", None) or np.trapz)(m, grids[ax], axis=ax)
        c = np.concatenate([[0.0], np.cumsum(0.5 * (m[1:] + m[:-1]) * np.diff(grids[k]))])
        cdfs.append(c / c[-1])
    return grids, np.stack(cdfs)


def main():
    os.makedirs(os.path.join(HERE, "conditional"), exist_ok=True)
    for name, G in CASES.items():
        ospec, spec, flat, theta, x = make_case(name, B=16)
        lo, hi = box(ospec)
        value = float(theta[0, FIXED_D])
        assert lo[FIXED_D] < value < hi[FIXED_D]
        x_row = x[0]
        grids, cdfs = conditional_cdfs(ospec, flat, x_row.astype(np.float64), value, lo, hi, G)
        free = [d for d in range(ospec.D) if d != FIXED_D]

        def pot(th, xx):
            return oracle_log_prob(ospec, flat, th, xx)
        xs = np.repeat(x_row[None], ROWS, 0)
        cond = np.full((ROWS, ospec.D), np.nan)
        cond[:, FIXED_D] = value
        mask, n_free, dead = SM.row_plan(cond, lo, hi)
        ks, acc = [], []
        for seed in SEEDS:
            draws, _ = OP.sample(ospec, torch.as_tensor(flat), xs, R0, seed + 1000, lo, hi, dtype=torch.float64)
            th0, lp0, enough = SM.select_starts(pot, xs, np.asarray(draws, np.float64), mask, np.nan_to_num(cond), W)
            out, _, a = SM.run(pot, xs, th0, lp0, mask, enough & ~dead, lo, hi, num_samples=S, burn_in=BURN, thin=THIN, seed=seed)
            ks.append([SM.ks_distance(out[:, :, d].reshape(-1), grids[k], cdfs[k]) for k, d in enumerate(free)])
            acc.append(a.mean())
            print(f"{name} seed {seed}: KS {ks[-1]} acceptance {acc[-1]:.3f}", flush=True)
        np.savez_compressed(os.path.join(HERE, "conditional", f"{name}.npz"), x_row=x_row, fixed_d=np.int64(FIXED_D),
                            value=np.float64(value), free=np.asarray(free), lo=lo, hi=hi, grids=grids, cdfs=cdfs,
                            model_ks=np.asarray(ks), model_acceptance=np.asarray(acc), seeds=np.asarray(SEEDS))
        print(f"{name}: largest model KS {np.max(ks):.4f}, threshold {1.5 * np.max(ks):.4f}, acceptance {np.mean(acc):.3f}")


if __name__ == "__main__":
    main()
