"""CPU: the compact fused image of the fp32 16-row sampler (csrc/sf_layout.h: packed16c) as the packer lays it out -- one
contiguous block per transform with exactly what the fused passes read (second block's biases, head biases in both forms, head
tile, W', second block's fragments on and below the diagonal) -- for the six shapes of the unrolled fused kernels: its offsets
against the kernels' compile-time ones (SfFixC16, sf_maf16.hip; "c16_fix" of describe()) and against the layout rule restated
here, alignment, no overlap, whole 1 KiB wave-instructions, and every float against the full 16-row image it is gathered from."""
import numpy as np
import pytest

import wavesim as ws
from cases import make_case
from oracle import flows as OF
from synference_amd.spec import FlowSpec

SHAPES = {3: 24, 4: 36, 5: 50}   # D -> H: every degree group fills one 16-row tile


def _handle(D, NB, T=3, C=7, H=None):
    from synference_amd.engine import HipFlow
    seed = 10 * D + NB
    H = H or SHAPES[D]
    rng = np.random.default_rng(seed)
    st = dict(theta_mean=rng.normal(size=D).astype(np.float32), theta_std=rng.uniform(0.5, 2.0, size=D).astype(np.float32),
              x_mean=rng.normal(size=C).astype(np.float32), x_std=rng.uniform(0.5, 2.0, size=C).astype(np.float32))
    perms = OF.random_perms(D, T, seed)
    ospec = OF.FlowSpec(kind="maf", D=D, C=C, H=H, T=T, K=10, perms=perms, NB=NB,
                        **{k: v.astype(np.float64) for k, v in st.items()})
    spec = FlowSpec(kind="maf", D=D, C=C, H=H, T=T, K=10, perms=perms, NB=NB, **st)
    flat = OF.init_params(ospec, seed + 1).astype(np.float32)
    return HipFlow(spec), flat   # creating a handle needs no GPU


def _blocks(d):
    """(name, compact offset, floats, offset in the full image or None for the fragment list) in layout order."""
    D, NB, NT = d["D"], d["NB"], d["nT16"]
    ent = NT * (NT + 1) // 2
    return [("bk1", d["o16c_bk1"], NT * 16 if NB == 2 else 0, d["o16_bk1"]),
            ("hvb", d["o16c_hvb"], 2 * D, d["o16_hvb"]),
            ("bh", d["o16c_bh"], 16, d["o16_bh"]),
            ("wh", d["o16c_wh"], NT * 256, d["o16_wh"]),
            ("wp", d["o16c_wp"], ent * 16, d["o16_wp"]),
            ("blk", d["o16c_blk"], ent * 256 if NB == 2 else 0, None)]


@pytest.mark.parametrize("NB", [1, 2])
@pytest.mark.parametrize("D", [3, 4, 5])
def test_compact_image_layout_and_contents(D, NB):
    hf, flat = _handle(D, NB)
    d = hf.describe()
    NT = d["nT16"]
    assert d["m16_ok"] and not d["m16_span"] and NT == D - 1
    assert d["c16_fix"] == 1, d   # the packer's offsets are the compile-time ones of SfFixC16<NB, D>
    # the layout rule: sub-blocks in this order, each on a 16-byte boundary, the whole padded to 256 floats
    off = 0
    for name, o, n, _ in _blocks(d):
        assert o == off and o % 4 == 0, (name, o, off)
        off = (o + n + 3) // 4 * 4
    size = d["t16c_stride"]
    assert size == (off + 255) // 256 * 256 and size % 256 == 0
    if (D, NB) == (5, 2):
        assert size == 15 * 256   # 15 KiB instead of the 26 KiB of part A and the second block
    tab = hf.pack_table16c()
    assert len(tab) == size
    # every float against the full image
    s1, s2 = hf.pack_table16()
    stride = d["t16_stride"]
    packed = ws.pack(flat.astype(np.float64), s1, s2)
    covered = np.zeros(size, bool)
    for t in range(d["T"]):
        full = packed[t * stride:(t + 1) * stride]
        compact = np.where(tab >= 0, full[np.maximum(tab, 0)], 0.0)
        for name, o, n, src in _blocks(d):
            if src is not None:
                assert np.array_equal(tab[o:o + n], src + np.arange(n)), name
                assert np.array_equal(compact[o:o + n], full[src:src + n]), name
                covered[o:o + n] = True
            else:
                for ot in range(NT if n else 0):   # entry ot (ot + 1) / 2 + it <- block ot * NT + it of the second hidden block
                    for it in range(ot + 1):
                        e, b = ot * (ot + 1) // 2 + it, d["o16_wk1"] + (ot * NT + it) * 256
                        assert np.array_equal(tab[o + e * 256:o + (e + 1) * 256], b + np.arange(256)), (ot, it)
                        assert np.array_equal(compact[o + e * 256:o + (e + 1) * 256], full[b:b + 256]), (ot, it)
                        covered[o + e * 256:o + (e + 1) * 256] = True
            if name in ("bh", "wh", "blk") and n:
                assert np.abs(compact[o:o + n]).max() > 0, name   # (really parameters, not a block of zeros)
    assert (tab[~covered] == -1).all() and (tab[covered] >= 0).all()   # padding and nothing else outside the sub-blocks
    assert len(np.unique(tab[covered])) == covered.sum()                # no float taken twice


@pytest.mark.parametrize("D,H", [(6, 30), (8, 56), (5, 24)])
def test_aligned_shapes_the_fused_kernels_do_not_serve_have_no_compact_image(D, H):
    """Aligned placement with the head tile and W' in the image, but D > 5 or several degree groups per tile: no kernel would read
    a compact image, so none is laid out (and no buffer allocated, no gather launched: both hang on c16_fix == 1)."""
    hf, _ = _handle(D, 2, H=H)
    d = hf.describe()
    assert d["m16_ok"] and not d["m16_span"] and d["o16_wp"] >= 0
    assert d["t16c_stride"] == 0 and d["c16_fix"] == -1 and len(hf.pack_table16c()) == 0


def test_flows_without_the_fused_kernels_have_no_compact_image():
    from synference_amd.engine import HipFlow
    _, spec, _, _, _ = make_case("maf_span6")   # contiguous placement: degree groups straddle tiles
    hf = HipFlow(spec)
    d = hf.describe()
    assert d["m16_span"] and d["t16c_stride"] == 0 and d["c16_fix"] == -1
    assert len(hf.pack_table16c()) == 0
