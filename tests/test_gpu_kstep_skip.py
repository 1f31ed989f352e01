"""GPU: the fused 16-row MAF sampler with the skipped k-step (sf_maf16_pass.h: sf_pass16g issues three of the four MFMA k-steps
and tanh registers for the hidden tiles whose rows 3, 7, 11, 15 are empty; SfDev::m16_k3 picks the instance of k_maf_samp16 /
k_maf_find16s) over the shapes of kstep_cases.py: every m16_k3 = 0 .. D - 1 at D = 3, 4, 5, and the small widths the dispatching
kernel serves.

Bars: given noise within 2e-4 of sigma of the fp64 oracle on every row (the inverse's bar of test_gpu_parity.py); catalogues draw
for draw against oracle/posterior.py under the rule of test_gpu_parity.py -- 1e-4 of the parameter scale on every draw, and a
galaxy may hold no more mismatching draws than its attempt count is off the oracle's (a candidate within rounding of the box edge
accepted by one side only moves that slot to a later attempt); everything else bit for bit."""
import functools

import numpy as np
import pytest
import torch

import kstep_cases as KC
from cases import oracle_inverse
from oracle import flows as OF
from oracle import philox
from oracle import posterior as OP

pytestmark = pytest.mark.gpu

M, S = 37, 24
CEILING = 4096


def _flow(spec, flat):
    from synference_amd.engine import HipFlow
    f = HipFlow(spec, "cuda:0")
    f.set_params(torch.as_tensor(flat))
    f.set_sample_time_limit(20)
    return f


def _oracle_first_accepted(ospec, flat, x, seed, lo, hi, ceiling, chunk=64):
    """oracle/posterior.py::sample_slots with a ceiling, ``chunk`` attempts of every open slot per call of the oracle's inverse:
    the same Philox stream (oracle/philox.py), the same flow (oracle/flows.py), the same box test, the lowest accepted attempt of
    every slot; slots that exhaust the ceiling are NaN rows.  (Attempt by attempt the oracle makes 4 096 calls on a handful of
    rows for a box that one attempt in 600 meets; test_chunked_oracle_is_the_oracle holds this form to it: the same attempt counts,
    the draws equal to the rounding of torch's fp32 products at another batch size.)"""
    n = len(x) * S
    slots = np.arange(n, dtype=np.uint64)
    out = np.full((n, ospec.D), np.nan)
    used = np.zeros(n, dtype=np.int64)
    pending = np.arange(n)
    ft = torch.as_tensor(flat).to(torch.float32)
    xs = np.asarray(x)
    for a0 in range(0, ceiling, chunk):
        if not len(pending):
            break
        na = min(chunk, ceiling - a0)
        sl = np.repeat(slots[pending], na)
        att = np.tile(np.arange(a0, a0 + na, dtype=np.uint32), len(pending))
        z = philox.normal(seed, sl, att, ospec.D)
        with torch.no_grad():
            th, _ = OF.inverse_transform(ospec, ft, torch.as_tensor(z), torch.as_tensor(xs[(sl // np.uint64(S)).astype(np.int64)]))
        ok = OP.in_box(th.numpy(), lo, hi).reshape(len(pending), na)
        hit = ok.any(1)
        first = ok.argmax(1)
        th = th.numpy().reshape(len(pending), na, ospec.D)
        out[pending[hit]] = th[hit, first[hit]]
        used[pending] += np.where(hit, first + 1, na)
        pending = pending[~hit]
    return out.reshape(len(x), S, ospec.D), used.reshape(len(x), S).sum(1)


@functools.lru_cache(maxsize=None)
def _reference(D, H, NB, T, sf):
    """Everything of a shape that does not need the device, computed once: the case, the boxes, the oracle's catalogues."""
    ospec, spec, flat, _, x = KC.make(D, H, NB, T, sf, B=M)
    # 37 near-identical galaxies, so that one box is narrow for all of them
    xs = (x[:1] * (1.0 + 0.002 * np.arange(M, dtype=np.float32))[:, None]).astype(np.float32)
    free, _ = OP.sample(ospec, torch.as_tensor(flat), xs[:1], 4000, 5, dtype=torch.float32)
    free = free.reshape(-1, D)
    box = {}
    for name, p in (("wide", 0.7), ("narrow", 1.0 / 600.0)):
        q = 0.5 * (1.0 - p ** (1.0 / D))   # central fraction p^(1/D) per dimension
        box[name] = (np.quantile(free, q, axis=0).astype(np.float32), np.quantile(free, 1.0 - q, axis=0).astype(np.float32))
    ref = {name: _oracle_first_accepted(ospec, flat, xs, 17, *box[name], CEILING) for name in box}
    rng = np.random.default_rng(7)
    z = rng.normal(size=(M, D)).astype(np.float32)
    rth, _ = oracle_inverse(ospec, flat, z, x, torch.float64)
    return dict(ospec=ospec, spec=spec, flat=flat, x=x, xs=xs, box=box, ref=ref, z=z, rth=rth)


def test_chunked_oracle_is_the_oracle():
    R = _reference(5, 50, 2, 2, "softplus")
    lo, hi = R["box"]["wide"]
    ref, rnd = OP.sample(R["ospec"], torch.as_tensor(R["flat"]), R["xs"], S, 17, lo, hi, max_attempts=CEILING, dtype=torch.float32)
    got, nd = R["ref"]["wide"]
    # the same accepted attempt of every slot; the draws to the rounding of torch's fp32 products at another batch size
    assert np.array_equal(nd, rnd), (nd, rnd)
    assert np.abs((got - ref) / np.asarray(R["ospec"].theta_std)).max() < 1e-5


@pytest.mark.parametrize("D,H,NB,T,sf", KC.GRID, ids=KC.IDS)
def test_given_noise_meets_the_oracle_and_a_nan_row_stays_alone(D, H, NB, T, sf):
    R = _reference(D, H, NB, T, sf)
    f = _flow(R["spec"], R["flat"])
    d = f.describe()
    assert d["m16_k3"] == KC.expected_k3(D, H)
    th, _ = f.inverse_sampler(R["z"], R["x"])
    assert f.last_sampler_rc == (3 if KC.unrolled(D, H) else 2), f.last_sampler_rc   # 3: the fused pass functions
    th = th.cpu().numpy()
    err = np.abs((th.astype(np.float64) - R["rth"]) / np.asarray(R["ospec"].theta_std)).max()
    print(f"D={D} H={H} NB={NB} T={T} {sf} k3={d['m16_k3']}: max |dtheta|/sigma {err:.2e}")
    assert np.isfinite(th).all() and err < 2e-4, err
    # a NaN context row in the middle of a tile: the other rows keep their bits (what the skipped register holds for that
    # sample -- the table row of a NaN context is NaN in the empty rows too -- is never an operand)
    x2 = R["x"].copy()
    x2[5] = np.nan
    th2, _ = f.inverse_sampler(R["z"], x2)
    th2 = th2.cpu().numpy()
    keep = np.arange(M) != 5
    assert np.array_equal(th2[keep], th[keep]) and not np.isfinite(th2[5]).any()


@pytest.mark.parametrize("D,H,NB,T,sf", KC.GRID, ids=KC.IDS)
def test_catalogue_draw_for_draw_wide_and_narrow_box(D, H, NB, T, sf):
    R = _reference(D, H, NB, T, sf)
    f = _flow(R["spec"], R["flat"])
    xt = torch.as_tensor(R["xs"], dtype=torch.float32, device="cuda:0").contiguous()
    f.prepare_context(xt)
    try:
        assert f.sampler_fused() == KC.unrolled(D, H)   # the fused kernels serve exactly the one-group-per-tile shapes
    finally:
        f.release_context()
    assert f.describe()["m16_k3"] == KC.expected_k3(D, H)
    scale = np.asarray(R["ospec"].theta_std)
    for name in ("wide", "narrow"):
        lo, hi = R["box"][name]
        ref, rnd = R["ref"][name]
        got, nd = f.sample(R["xs"], S, lo, hi, seed=17, max_attempts=CEILING, return_counts=True)
        got, nd = got.cpu().double().numpy(), nd.cpu().numpy().astype(np.int64)
        open_ref, open_got = np.isnan(ref[..., 0]), np.isnan(got[..., 0])
        both = ~open_ref & ~open_got
        err = np.where(both, np.abs((got - ref) / scale).max(-1), 0.0)
        bad_g = (err > 1e-4).sum(1) + (open_ref != open_got).sum(1)
        off_g = np.abs(nd - rnd)
        print(f"D={D} H={H} NB={NB} T={T} {sf} {name}: attempts per slot {nd.sum() / (M * S):.1f} (oracle {rnd.sum() / (M * S):.1f}), "
              f"unfilled {f.last_unfilled} (oracle {int(open_ref.sum())}), rounds {f.last_sample_stats['rounds']}, "
              f"max |dtheta|/sigma {err.max():.2e}, galaxies with another count {int((off_g > 0).sum())}")
        assert ((got[both] >= lo) & (got[both] <= hi)).all()
        assert (bad_g <= off_g).all(), (name, bad_g, off_g, err.max())
        assert off_g.sum() <= max(3, 0.01 * rnd.sum()), (name, off_g.sum())
        assert f.last_unfilled == int(open_got.sum())
        assert abs(f.last_unfilled - int(open_ref.sum())) <= int((open_ref != open_got).sum())
        if (off_g == 0).all():
            assert f.last_unfilled == int(open_ref.sum())
        if name == "narrow":
            assert rnd.sum() > 200 * M * S, rnd.sum()           # (the test's own set-up: about one attempt in 600)
            assert f.last_sample_stats["rounds"] >= 3, f.last_sample_stats   # the find / resolve launches ran


@pytest.mark.parametrize("D,H,NB,T,sf", KC.GRID, ids=KC.IDS)
def test_galaxy_alone_equals_its_place_in_a_ragged_catalogue(D, H, NB, T, sf):
    R = _reference(D, H, NB, T, sf)
    f = _flow(R["spec"], R["flat"])
    n_gal = 131   # 131 x 24 draws: not a whole number of 128-item iterations
    rng = np.random.default_rng(11)
    x = np.concatenate([R["x"]] * 4)[:n_gal] * (1.0 + 0.01 * rng.normal(size=(n_gal, 1)))
    x = x.astype(np.float32)
    lo, hi = R["box"]["wide"]
    whole, nd = f.sample(x, S, lo, hi, seed=23, max_attempts=CEILING, return_counts=True)
    whole, nd = whole.cpu().numpy(), nd.cpu().numpy()
    try:
        for g in (0, 64, 130):
            f.set_sample_row_offset(g)
            alone, nda = f.sample(x[g:g + 1], S, lo, hi, seed=23, max_attempts=CEILING, return_counts=True)
            assert np.array_equal(alone.cpu().numpy()[0], whole[g], equal_nan=True), g
            assert int(nda.cpu().numpy()[0]) == int(nd[g]), g
    finally:
        f.set_sample_row_offset(0)
