"""CPU: the 16-row MAF image with the skipped register (csrc/sf_layout.cpp).  Where every hidden tile holds one degree group
(D = 3..5), a group of 12 or fewer units leaves rows 3, 7, 11, 15 of its tile empty, so that the fourth k-step of every MFMA that
reads the tile and the fourth tanh register are structural zeros; ``m16_k3`` of describe() counts those (trailing) tiles and picks
the kernel instance.  Checked on the packer's own table (no GPU): the count, the placement against the rule restated in
kstep_cases.py, every block of the image against that placement, the zeros the kernels rely on, the parent's rows for groups of
13..16 units, and the wave-level simulation of the inverse over the new image against the fp64 oracle."""
import numpy as np
import pytest
import torch

import kstep_cases as KC
import wavesim as ws
from oracle import flows as OF


def _handle(D, H, NB, T, sf):
    from synference_amd.engine import HipFlow
    ospec, spec, flat, _, x = KC.make(D, H, NB, T, sf, B=16)
    return HipFlow(spec), ospec, flat, x   # creating a handle needs no GPU


def _deg(unit, D):
    return unit % (D - 1) + 1


def _rows_of_image(d, s1):
    """unit of every row of the hidden tiles, read off the first hidden block's bias rows of transform 0 (logical index = base +
    unit, and unit 0 always exists)."""
    NT = d["nT16"]
    b = np.asarray(s1[d["o16_bk0"]:d["o16_bk0"] + NT * 16], dtype=np.int64)
    rows = -np.ones(64, dtype=np.int64)
    rows[:NT * 16] = np.where(b >= 0, b - b[b >= 0].min(), -1)
    return rows


def _check_block(s1, off, OT, IT, orow, irow, in_dim, mask, what):
    """A weight block [ot][it][64 lanes][4] (lane l: out row ot*16 + (l & 15), in rows it*16 + 4 (l >> 4) + r) against the rows:
    entry = base + out * in_dim + in where both rows hold a unit and the mask lets the weight through, else -1."""
    blk = np.asarray(s1[off:off + OT * IT * 256], dtype=np.int64).reshape(OT, IT, 64, 4)
    base = None
    for ot in range(OT):
        for it in range(IT):
            for l in range(64):
                for r in range(4):
                    oo, ii = orow[ot * 16 + (l & 15)], irow[it * 16 + 4 * (l >> 4) + r]
                    on = oo >= 0 and ii >= 0 and mask(oo, ii)
                    e = blk[ot, it, l, r]
                    if not on:
                        assert e == -1, (what, ot, it, l, r)
                    else:
                        b = e - (oo * in_dim + ii)
                        base = b if base is None else base
                        assert e >= 0 and b == base, (what, ot, it, l, r)
    assert base is not None, what


@pytest.mark.parametrize("D,H,NB,T,sf", KC.GRID, ids=KC.IDS)
def test_placement_count_and_structural_zeros(D, H, NB, T, sf):
    hf, ospec, flat, x = _handle(D, H, NB, T, sf)
    d = hf.describe()
    assert d["m16_ok"]
    k3, unrolled = KC.expected_k3(D, H), KC.unrolled(D, H)
    assert d["m16_k3"] == k3, (d["m16_k3"], k3)
    NT = d["nT16"]
    assert (not d["m16_span"] and NT == D - 1) == unrolled
    s1, s2 = hf.pack_table16()
    rows = _rows_of_image(d, s1)
    want, nt = KC.skip_rows(D, H)
    assert nt == NT and np.array_equal(rows, want), (rows, want)
    assert sorted(rows[rows >= 0].tolist()) == list(range(H))   # a permutation of the units
    sizes = KC.group_sizes(D, H)
    if unrolled:
        assert k3 == sum(n <= 12 for n in sizes) and all(n <= 12 for n in sizes[NT - k3:]) and all(n > 12 for n in sizes[:NT - k3])
    k3_tile = [unrolled and ot >= NT - k3 for ot in range(NT)]
    # groups of 13..16 units, and every shape the unrolled kernels do not serve: the parent's rows -- every block of the image is
    # laid out from the rows by code this placement does not touch (checked block by block below), so the parent's image
    prow, pnt = KC.parent_rows(D, H)
    for ot in range(NT):
        if not k3_tile[ot]:
            assert np.array_equal(rows[ot * 16:ot * 16 + 16], prow[ot * 16:ot * 16 + 16]), ot
    if k3 == 0:
        assert pnt == NT and np.array_equal(rows, prow)
    stride = d["t16_stride"]
    hid = lambda j, i: _deg(j, D) >= _deg(i, D)
    packed = ws.pack(flat.astype(np.float64), s1, s2)
    for t in range(T):
        st = np.asarray(s1[t * stride:(t + 1) * stride], dtype=np.int64)
        img = packed[t * stride:(t + 1) * stride]
        for k in range(NB):
            _check_block(st, d[f"o16_wk{k}"], NT, NT, rows, rows, H, hid, f"wk{k}")
            b = st[d[f"o16_bk{k}"]:d[f"o16_bk{k}"] + NT * 16]
            assert np.array_equal(b >= 0, rows[:NT * 16] >= 0) and np.array_equal((b - b[b >= 0].min())[b >= 0], rows[:NT * 16][b >= 0])
        b0 = st[d["o16_b0"]:d["o16_b0"] + NT * 16]
        assert np.array_equal(b0 >= 0, rows[:NT * 16] >= 0)
        # the zeros the fused passes rely on: rows 3, 7, 11, 15 of a KS = 3 tile, as output rows and as input rows
        for ot in range(NT):
            if not k3_tile[ot]:
                continue
            assert (rows[ot * 16 + 3:ot * 16 + 16:4] == -1).all()
            lanes3 = [l for l in range(64) if (l & 15) % 4 == 3]
            w0 = st[d["o16_w0"]:d["o16_w0"] + NT * 256].reshape(NT, 64, 4)
            assert (w0[ot, lanes3] == -1).all() and (img[d["o16_w0"]:d["o16_w0"] + NT * 256].reshape(NT, 64, 4)[ot, lanes3] == 0).all()
            for name in ["o16_b0"] + [f"o16_bk{k}" for k in range(NB)]:
                bb = st[d[name]:d[name] + NT * 16].reshape(NT, 4, 4)
                assert (bb[ot, :, 3] == -1).all(), name
                assert (img[d[name]:d[name] + NT * 16].reshape(NT, 4, 4)[ot, :, 3] == 0).all(), name
            for k in range(NB):
                wk = st[d[f"o16_wk{k}"]:d[f"o16_wk{k}"] + NT * NT * 256].reshape(NT, NT, 64, 4)
                wv = img[d[f"o16_wk{k}"]:d[f"o16_wk{k}"] + NT * NT * 256].reshape(NT, NT, 64, 4)
                assert (wk[ot][:, lanes3] == -1).all() and (wv[ot][:, lanes3] == 0).all()   # output rows
                assert (wk[:, ot, :, 3] == -1).all() and (wv[:, ot, :, 3] == 0).all()         # input rows: the skipped k-step
            if d["o16_wh"] >= 0:
                wh = st[d["o16_wh"]:d["o16_wh"] + NT * 256].reshape(NT, 64, 4)
                assert (wh[ot, :, 3] == -1).all() and (img[d["o16_wh"]:d["o16_wh"] + NT * 256].reshape(NT, 64, 4)[ot, :, 3] == 0).all()
            hv = st[d["o16_hv"]:d["o16_hv"] + D * 128].reshape(D, 4, 4, 4, 2)   # [slot][g4][tile][r][a | m]
            assert (hv[:, :, ot, 3, :] == -1).all()
        if d["o16_wh"] >= 0:
            cst = np.asarray(d["cst"])
            sinv_rows = -np.ones(16, dtype=np.int64)   # head tile row 2 q + ab = logical head row 2 sinv[q] + ab
            hb = st[d["o16_bh"]:d["o16_bh"] + 16]
            sinv_rows[hb >= 0] = hb[hb >= 0] - hb[hb >= 0].min()
            assert (hb >= 0).sum() == 2 * D
            _check_block(st, d["o16_wh"], 1, NT, sinv_rows, rows, H, lambda oo, unit: (oo // 2 + 1) > _deg(unit, D), "wh")
        # W' = (W1 o M)(W0 o M0) as k_maf_fuse16 forms it from the image: its rows 3, 7, 11, 15 of a KS = 3 tile are exactly 0
        if d["o16_wp"] >= 0 and unrolled and NB >= 1:
            w1 = img[d["o16_wk0"]:d["o16_wk0"] + NT * NT * 256].reshape(NT, NT, 4, 16, 4)   # [ot][it][kk >> 2][row][kk & 3]
            w0i = img[d["o16_w0"]:d["o16_w0"] + NT * 256].reshape(NT, 4, 16, 4)             # [it][col >> 2][kk][col & 3]
            for ot in range(NT):
                W1 = w1[ot].transpose(2, 0, 1, 3).reshape(16, NT * 16)                       # [row][it * 16 + kk]
                W0 = w0i.transpose(0, 2, 1, 3).reshape(NT * 16, 16)                          # [it * 16 + kk][col]
                Wp = W1 @ W0
                if k3_tile[ot]:
                    assert (Wp[3::4] == 0).all(), ot
                assert np.abs(Wp[rows[ot * 16:ot * 16 + 16] >= 0]).max() > 0


@pytest.mark.parametrize("D,H,NB,T,sf", KC.GRID, ids=KC.IDS)
def test_wave_simulation_over_the_image_meets_the_oracle(D, H, NB, T, sf):
    hf, ospec, flat, x = _handle(D, H, NB, T, sf)
    d = hf.describe()
    s1, s2 = hf.pack_table16()
    packed = ws.pack(flat.astype(np.float64), s1, s2)
    z = np.random.default_rng(4).normal(size=(16, D))
    ref, _ = OF.inverse_transform(ospec, torch.as_tensor(flat, dtype=torch.float64), torch.as_tensor(z), torch.as_tensor(x).double())
    ref = ref.numpy()
    for hm in ([False, True] if d["o16_wh"] >= 0 and not d["m16_span"] else [False]):
        got = ws.maf_inverse16(d, packed, z, x.astype(np.float64), head_mfma=hm)
        assert np.abs(got - ref).max() < 5e-6 * max(1.0, np.abs(ref).max()), hm   # (fp32 constants image)


@pytest.mark.parametrize("D,H,NB,T,sf", [g for g in KC.GRID if g[2] == 2], ids=[i for g, i in zip(KC.GRID, KC.IDS) if g[2] == 2])
def test_training_image_keeps_the_rows_without_the_skipped_register(D, H, NB, T, sf):
    """The cooperative training kernel's image (sf_trainc.hip) is laid out from its own row table: units in rows 0 .. n - 1 as
    before the skipped register.  Another placement would reorder the sums of the training MFMAs, and thousands of Adam steps
    amplify that rounding into other fitted weights: a sampler optimisation must not move what a fit converges to."""
    hf, ospec, flat, x = _handle(D, H, NB, T, sf)
    s1, s2, gd, d, cst = hf.trainc_table()
    NT = d["NT"]
    b = np.asarray(s1[d["o_b1"]:d["o_b1"] + NT * 16], dtype=np.int64)   # first hidden block's bias rows of transform 0
    rows = -np.ones(64, dtype=np.int64)
    rows[:NT * 16] = np.where(b >= 0, b - b[b >= 0].min(), -1)
    want, nt = KC.parent_rows(D, H)
    assert nt == NT and np.array_equal(rows, want), (rows, want)
