"""Model of the head-row region of the fused fp32 16-row MAF sampler (csrc/sf_layout.h: t16h_stride; sf_maf16_pass.h: sf_pass16g).

The fused passes take the (a, m) head rows as per-lane packed FMAs.  Behind the compact image of every transform sits one entry of
32 floats per (hidden tile ot, degree k >= ot + 2), tiles in order and per tile in DEGREE order; inside an entry the floats are
[g4][r][a|m]: row group g4, row r of the group (unit of tile row 4 g4 + r), a then m.  The packer gathers an entry from the o16_hv
rows of the physical slot that holds degree k in that transform -- the slot differs from transform to transform, so the table is
[T, t16h_stride].

Two halves, so that a test can set one against the other:
  ``logical_region``   every float from the flow's parameters alone (no slot anywhere: degree k of a transform IS its logical
                       dimension k - 1)
  ``table_from_slots`` the gather table from a degree -> slot table, as the packer builds it
"""
import numpy as np

import kstep_cases as KC
from oracle import flows as OF

# (D, H) with one degree group per hidden tile: m16_k3 runs through 0 .. D - 1
# (kstep_cases.py's widths, and D = 4, H = 38 for the one count they leave out: groups of 13, 13, 12 units, m16_k3 = 1)
SHAPES = [(D, H) for (D, H), (k3, unrolled) in KC.SHAPES.items() if unrolled and (D, H) not in ((5, 64), (5, 36))] + [(4, 38)]
GRID = [(D, H, NB, T) for (D, H) in SHAPES for NB in (1, 2) for T in (1, 2)]
IDS = [f"D{D}-H{H}-NB{NB}-T{T}" for (D, H, NB, T) in GRID]


def expected_k3(D, H):
    """Trailing tiles whose group holds 12 or fewer units (the larger groups come first)."""
    return sum(n <= 12 for n in KC.group_sizes(D, H))


def entry(D, ot, k):
    """Index of the entry of (tile ot, degree k), k = ot + 2 .. D (sf_hr16_entry)."""
    assert 0 <= ot <= D - 2 and ot + 2 <= k <= D
    return ot * (D - 1) - ot * (ot - 1) // 2 + (k - ot - 2)


def entries(D):
    return D * (D - 1) // 2


def stride(D):
    return (entries(D) * 32 + 255) // 256 * 256


def make(D, H, NB, T, B=16):
    """(oracle spec, product spec, flat, theta, x) with a non-identity permutation in front of the second transform."""
    case = KC.make(D, H, NB, T, "softplus", B=B)
    if T > 1:
        perms = np.asarray(case[0].perms)
        assert any(not np.array_equal(np.asarray(p), np.arange(D)) for p in perms), perms
    return case


def logical_region(ospec, flat, D, H):
    """[T, stride] from the parameters: entry (ot, k)[g4][r][ab] = Wf_t[2 (k - 1) + ab][unit of row 4 g4 + r of tile ot], zero where
    the row holds no unit (padding rows; rows 3, 7, 11, 15 of a tile whose fourth k-step is skipped) and in the padding behind the
    entries.  (The MADE mask lets every such weight through: a unit of tile ot has degree ot + 1 < k.)"""
    import torch
    rows, nt = KC.skip_rows(D, H)
    assert nt == D - 1
    P = OF.views(ospec, torch.as_tensor(np.asarray(flat, dtype=np.float64)))
    out = np.zeros((ospec.T, stride(D)))
    for t in range(ospec.T):
        Wf = P[f"t{t}.Wf"].numpy()
        for ot in range(D - 1):
            for k in range(ot + 2, D + 1):
                e = entry(D, ot, k)
                for g4 in range(4):
                    for r in range(4):
                        unit = rows[ot * 16 + 4 * g4 + r]
                        assert unit < 0 or unit % (D - 1) + 1 == ot + 1
                        for ab in range(2):
                            out[t, e * 32 + g4 * 8 + 2 * r + ab] = Wf[2 * (k - 1) + ab, unit] if unit >= 0 else 0.0
    return out


def slot_table(d):
    """[T, D]: physical slot of degree k = column + 1 in transform t (the constants image, c_dslot)."""
    cst = np.asarray(d["cst"])
    return np.array([[int(cst[d["c_dslot"] + t * 16 + q]) for q in range(d["D"])] for t in range(d["T"])])


def table_from_slots(d, slots):
    """The gather table [T, stride] as the packer builds it: the floats of an entry are the eight floats [r][a|m] of tile ot in
    row group g4 of the o16_hv rows ([slot][g4][tile (4)][r][a|m]) of the slot that holds the degree; -1 behind the entries."""
    D = d["D"]
    tab = -np.ones((d["T"], stride(D)), dtype=np.int64)
    for t in range(d["T"]):
        for ot in range(D - 1):
            for k in range(ot + 2, D + 1):
                e = entry(D, ot, k)
                for g4 in range(4):
                    src = d["o16_hv"] + int(slots[t][k - 1]) * 128 + g4 * 32 + ot * 8
                    tab[t, e * 32 + g4 * 8:e * 32 + g4 * 8 + 8] = src + np.arange(8)
    return tab


def gather(packed, d, tab):
    """The region [T, stride] that a table gathers from the packed 16-row image (k_maf_compact16's rule: -1 = zero)."""
    out = np.zeros(tab.shape)
    for t in range(d["T"]):
        full = packed[t * d["t16_stride"]:(t + 1) * d["t16_stride"]]
        out[t] = np.where(tab[t] >= 0, full[np.maximum(tab[t], 0)], 0.0)
    return out
