"""Shapes of the 16-row MAF sampler around the skipped k-step (csrc/sf_layout.cpp: a degree group of 12 or fewer units leaves
rows 3, 7, 11, 15 of its tile empty; SfDev::m16_k3 counts the trailing tiles of that kind; sf_pass16g issues three of the four
MFMA k-steps and three of the four tanh registers for them).

Degrees are dealt as unit % (D - 1), so the groups of a flow hold ceil(H / (D - 1)) or floor(H / (D - 1)) units, the larger ones
first: m16_k3 runs through 0 .. D - 1 as H falls from 13 (D - 1) to 12 (D - 1).  The small widths put every group into one tile
(no unrolled kernel, no skipping: the dispatching kernel and the parent's rows).

The weights are those of ``cases.make_case`` (initialisation plus a spread of half the mean magnitude: fitted-like)."""
import numpy as np

import cases

C = 7

# (D, H) -> (m16_k3, one degree group per hidden tile: the unrolled fused kernels serve the shape)
SHAPES = {
    (5, 52): (0, True), (5, 51): (1, True), (5, 50): (2, True), (5, 49): (3, True), (5, 48): (4, True),
    (5, 64): (0, True), (5, 36): (4, True), (5, 16): (0, False), (5, 4): (0, False),
    (4, 48): (0, True), (4, 37): (2, True), (4, 36): (3, True), (4, 9): (0, False),
    (3, 32): (0, True), (3, 25): (1, True), (3, 24): (2, True), (3, 5): (0, False),
}
MORE = [(5, 50), (5, 48), (4, 37), (3, 25)]   # also with one hidden block, with five transforms and with the sigmoid scale

# (D, H, NB, T, scale_fn)
GRID = [(D, H, 2, 2, "softplus") for (D, H) in SHAPES] + \
       [(D, H, NB, T, sf) for (D, H) in MORE for (NB, T, sf) in ((1, 2, "softplus"), (2, 5, "softplus"), (2, 2, "sigmoid2"))]
IDS = [f"D{D}-H{H}-NB{NB}-T{T}-{sf}" for (D, H, NB, T, sf) in GRID]


def expected_k3(D, H):
    return SHAPES[(D, H)][0]


def unrolled(D, H):
    return SHAPES[(D, H)][1]


def group_sizes(D, H):
    """Units per MADE degree 1 .. D - 1 (degree of unit j = j % (D - 1) + 1)."""
    return [len(range(g, H, D - 1)) for g in range(D - 1)]


def make(D, H, NB=2, T=2, scale_fn="softplus", B=37, seed=0):
    """(oracle spec, product spec, flat, theta, x) of ``cases.make_case`` for this shape."""
    name = f"kstep_d{D}_h{H}_nb{NB}_t{T}_{scale_fn}"
    extra = dict(NB=NB)
    if scale_fn != "softplus":
        extra["scale_fn"] = scale_fn
    cases.CASES.setdefault(name, ("maf", D, C, H, T, 10, extra))
    return cases.make_case(name, seed=seed, B=B)


def parent_rows(D, H):
    """The 16-row placement before the skipped register, restated: whole degree groups in order, a group that does not fit the
    rest of a tile starts the next one, units in rows used .. used + n - 1.  -> unit of every row [4 * 16] (-1: none), tiles."""
    rows = -np.ones(64, dtype=np.int64)
    tile = used = 0
    for g in range(D - 1):
        units = list(range(g, H, D - 1))
        if used + len(units) > 16:
            tile, used = tile + 1, 0
        assert tile < 4 and len(units) <= 16
        rows[tile * 16 + used:tile * 16 + used + len(units)] = units
        used += len(units)
    return rows, tile + 1


def skip_rows(D, H):
    """The placement with the skipped register: where every tile holds one group (D = 3..5), unit q of a group of n units sits in
    row 4 (q // KS) + q % KS with KS = max(3, ceil(n / 4)); every other shape keeps ``parent_rows``."""
    rows, nt = parent_rows(D, H)
    if not (3 <= D <= 5 and nt == D - 1):
        return rows, nt
    rows[:] = -1
    for g in range(D - 1):
        units = list(range(g, H, D - 1))
        ks = max(3, -(-len(units) // 4))
        for q, unit in enumerate(units):
            rows[g * 16 + 4 * (q // ks) + q % ks] = unit
    return rows, nt
