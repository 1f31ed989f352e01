"""Shapes, catalogues and boxes of tests/test_gpu_pipelined_passes.py, and the recorded oracle reference of its narrow box.

The fused fp32 16-row MAF sampler (sf_maf16.hip: one Philox call for the two tiles of a wave; sf_maf16_pass.h: sf_pass16g) on
NB = 1, 2 x D = 3, 4, 5 with the two widths per D that give m16_k3 = 0 and D - 1, each with the softplus and the sigmoid scale.

The narrow box is met by about one attempt in a thousand.  oracle/posterior.py walks the attempts one at a time (about 10 s for
150 slots), so its result is RECORDED: scripts/make_pipelined_passes_golden.py writes tests/golden/pipelined_passes/narrow.npz.
All galaxies of a narrow catalogue are the same context row, so that every one of them sees the box; a draw then depends on its
slot id alone (slot = galaxy * draws + index: the Philox counter), and ONE reference over slots 0 .. 149 serves every catalogue:
the draws of catalogue (M, S) are its first M * S rows, a galaxy's attempt count the sum over its S slots."""
import os

import numpy as np
import torch

import kstep_cases as KC
from oracle import posterior as OP

WIDTHS = {5: (52, 48), 4: (48, 36), 3: (32, 24)}   # D -> H with m16_k3 = 0, D - 1
T = 2
GRID = [(D, H, NB, sf) for D in (5, 4, 3) for H in WIDTHS[D] for NB in (1, 2) for sf in ("softplus", "sigmoid2")]
IDS = [f"D{D}-H{H}-NB{NB}-{sf}" for (D, H, NB, sf) in GRID]
# (galaxies, draws): one item; two tiles, the second with one item; 80 items = items 64 .. 79 in tile 1 of wave 0; 150 items
# = a second 128-item iteration, ragged; 129 = one item in it
CATALOGUES = [(1, 1), (1, 17), (2, 40), (3, 50), (1, 129)]
N_SLOTS = max(m * s for m, s in CATALOGUES)
SEED_WIDE, SEED_NARROW = 2025, 31
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipelined_passes", "narrow.npz")


def make(D, H, NB, sf, B):
    return KC.make(D, H, NB, T, sf, B=B)


def box(ospec, spec, flat, x0, q, n_free):
    """The q .. 1 - q quantiles per dimension of n_free unconstrained oracle draws of the context row x0."""
    free, _ = OP.sample(ospec, torch.as_tensor(flat), x0[None], n_free, 99, dtype=torch.float32)
    free = free.reshape(-1, spec.D)
    return np.quantile(free, q, axis=0).astype(np.float32), np.quantile(free, 1.0 - q, axis=0).astype(np.float32)


def narrow_q(D):
    """Central quantile range per dimension that a draw meets once in a thousand, were the dimensions independent."""
    return 0.5 * (1.0 - 1e-3 ** (1.0 / D))


def narrow_reference(D, H, NB, sf):
    """(lo, hi, draws [N_SLOTS, D], attempts used [N_SLOTS]) of oracle/posterior.py for slots 0 .. N_SLOTS - 1 of one context row."""
    ospec, spec, flat, _, x = make(D, H, NB, sf, B=1)
    lo, hi = box(ospec, spec, flat, x[0], narrow_q(D), 2000)
    th, used = OP.sample_slots(ospec, torch.as_tensor(flat), x[:1], np.arange(N_SLOTS), N_SLOTS, SEED_NARROW, lo, hi,
                               dtype=torch.float32)
    return lo, hi, th, used
