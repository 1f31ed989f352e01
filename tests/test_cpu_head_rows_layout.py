"""CPU: the head-row region of the fused fp32 16-row MAF sampler as the packer lays it out (csrc/sf_layout.cpp: src16h,
t16h_stride; read by sf_pass16g as per-lane packed FMAs) against the model of head_rows_model.py, for D = 3, 4, 5 x one / two
hidden blocks x the widths that give m16_k3 = 0 .. D - 1 x one / two transforms (a permutation in front of the second one):

* every float of the region is the logical head weight of its (transform, degree, tile, row, a|m), zero where the row holds no
  unit and in the padding; the packer's table is the model's table built from that transform's degree -> slot table;
* the region's size is the compile-time one of the kernels (SfFixC16: "c16_fix" of describe());
* a planted defect -- two degrees' slots swapped in the second transform -- does not pass the comparison;
* the full 16-row image's head tile (o16_wh) and head rows (o16_hv), the compact image's table and the cooperative training
  tables are what they were before the region existed: digests recorded under tests/golden/.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import head_rows_model as HM
import wavesim as ws

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "head_rows_parent_tables.json")


def _handle(D, H, NB, T):
    from synference_amd.engine import HipFlow
    ospec, spec, flat, _, x = HM.make(D, H, NB, T)
    return HipFlow(spec), ospec, flat   # creating a handle needs no GPU


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=np.int32)).tobytes()).hexdigest()


def parent_digests(hf):
    """Digests of the tables that the head-row region must leave alone."""
    d = hf.describe()
    s1, s2 = hf.pack_table16()
    NT, D, T, st = d["nT16"], d["D"], d["T"], d["t16_stride"]
    out = {}
    for name, off, n in (("o16_wh", d["o16_wh"], NT * 256), ("o16_hv", d["o16_hv"], D * 128)):
        sl = np.concatenate([np.arange(t * st + off, t * st + off + n) for t in range(T)])
        out[name] = _digest(np.concatenate([np.asarray(s1)[sl], np.asarray(s2)[sl]]))
    out["compact"] = _digest(hf.pack_table16c())
    if d["NB"] == 2:
        t1, t2, gd, _, _ = hf.trainc_table()
        out["trainc"] = _digest(np.concatenate([np.asarray(t1).ravel(), np.asarray(t2).ravel(), np.asarray(gd).ravel()]))
    return out


@pytest.mark.parametrize("D,H,NB,T", HM.GRID, ids=HM.IDS)
def test_region_holds_the_logical_head_rows(D, H, NB, T):
    hf, ospec, flat = _handle(D, H, NB, T)
    d = hf.describe()
    assert d["m16_ok"] and not d["m16_span"] and d["nT16"] == D - 1
    assert d["m16_k3"] == HM.expected_k3(D, H)
    # the packer's sizes are the kernels' compile-time ones
    assert d["c16_fix"] == 1, d
    assert d["t16h_stride"] == HM.stride(D) and d["t16h_stride"] % 256 == 0
    if D == 5:
        assert HM.entries(D) == 10 and d["t16h_stride"] == 512   # 320 floats in place of the head tile's 1 040
    tab = hf.pack_table16h()
    assert tab.shape == (T, HM.stride(D))
    # ... built from THAT transform's slot table
    slots = HM.slot_table(d)
    assert sorted(slots[0].tolist()) == list(range(D))
    if T > 1:
        assert not np.array_equal(slots[0], slots[1])   # (the set-up: the slot of a degree differs between the transforms)
    want_tab = HM.table_from_slots(d, slots)
    assert np.array_equal(tab, want_tab)
    used = HM.entries(D) * 32
    assert (tab[:, used:] == -1).all() and (tab[:, :used] >= 0).all() and (tab[:, :used] < d["t16_stride"]).all()
    for t in range(T):
        assert len(np.unique(tab[t, :used])) == used   # no float taken twice
    # every float against the parameters
    s1, s2 = hf.pack_table16()
    packed = ws.pack(flat.astype(np.float64), s1, s2)
    got = HM.gather(packed, d, tab)
    want = HM.logical_region(ospec, flat, D, H)
    assert np.array_equal(got, want)
    assert np.abs(want[:, :used]).max() > 0
    # the zeros the passes rely on: r = 3 of every row group of a tile whose fourth k-step is skipped
    NT, k3 = D - 1, d["m16_k3"]
    reg = got[:, :used].reshape(T, HM.entries(D), 4, 4, 2)
    for ot in range(NT):
        for k in range(ot + 2, D + 1):
            e = HM.entry(D, ot, k)
            if ot >= NT - k3:
                assert (reg[:, e, :, 3, :] == 0).all(), (ot, k)
            assert np.abs(reg[:, e, :, :3, :]).max() > 0, (ot, k)


@pytest.mark.parametrize("D,H,NB", [(5, 50, 2), (4, 37, 1), (3, 25, 2)])
def test_swapped_slots_in_the_second_transform_do_not_pass(D, H, NB):
    """The planted defect: a table built with two degrees' slots exchanged in the second transform gathers other head rows, and
    the comparison with the parameters says so (in that transform only)."""
    hf, ospec, flat = _handle(D, H, NB, 2)
    d = hf.describe()
    s1, s2 = hf.pack_table16()
    packed = ws.pack(flat.astype(np.float64), s1, s2)
    want = HM.logical_region(ospec, flat, D, H)
    slots = HM.slot_table(d)
    assert np.array_equal(HM.gather(packed, d, HM.table_from_slots(d, slots)), want)
    bad = slots.copy()
    bad[1, D - 2], bad[1, D - 1] = slots[1, D - 1], slots[1, D - 2]
    got = HM.gather(packed, d, HM.table_from_slots(d, bad))
    assert np.array_equal(got[0], want[0])
    assert not np.array_equal(got[1], want[1])
    # one table for every transform (the first one's) is the same defect
    same = np.repeat(slots[:1], 2, axis=0)
    assert not np.array_equal(HM.gather(packed, d, HM.table_from_slots(d, same)), want)


@pytest.mark.parametrize("D,H,NB,T", HM.GRID, ids=HM.IDS)
def test_full_image_compact_table_and_training_tables_are_the_parents(D, H, NB, T):
    hf, _, _ = _handle(D, H, NB, T)
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    assert parent_digests(hf) == golden[f"D{D}-H{H}-NB{NB}-T{T}"]
