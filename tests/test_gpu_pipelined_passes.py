"""GPU: the fused fp32 16-row MAF sampler with ONE Philox call for the two tiles of a wave (sf_maf16.hip: k_maf_samp16, PREC 2;
lanes 0..31 draw tile 0's blocks, lanes 32..63 tile 1's, v_permlane32_swap hands them over) and its pass functions
(sf_maf16_pass.h: sf_pass16g), on the shapes of pipelined_passes_cases.py: NB = 1, 2 x D = 3, 4, 5 x the widths with m16_k3 = 0
and D - 1 x the softplus and the sigmoid scale (the arm of the finish's branch that the bench flow never takes).

Bars (those of test_gpu_head_rows.py): given noise against the fp64 oracle, 2e-4 of sigma on every row; catalogues against
oracle/posterior.py, 1e-4 of the box width on every draw and the oracle's attempt count in every galaxy; a galaxy alone against
its place in a ragged catalogue bit for bit.  The narrow box's oracle results are recorded (pipelined_passes_cases.py)."""
import numpy as np
import pytest
import torch

import pipelined_passes_cases as PC
from cases import oracle_inverse
from oracle import posterior as OP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(PC.GOLDEN) as d:
        return {k: d[k] for k in d.files}


def _flow(spec, flat, D, H):
    from synference_amd.engine import HipFlow
    f = HipFlow(spec, "cuda:0")
    d = f.describe()
    assert d["c16_fix"] == 1 and d["m16_k3"] == (0 if H == PC.WIDTHS[D][0] else D - 1), d
    f.set_params(torch.as_tensor(flat))
    f.set_sample_time_limit(20)
    return f


def _assert_fused(f, x):
    xt = torch.as_tensor(x, dtype=torch.float32, device="cuda:0").contiguous()
    f.prepare_context(xt)
    try:
        assert f.sampler_fused()
    finally:
        f.release_context()


def _check_catalogue(tag, f, x, S, seed, lo, hi, ref, rnd):
    """One catalogue draw for draw: every draw within 1e-4 of the box width of the oracle's, every galaxy the oracle's attempt count."""
    got, nd = f.sample(x, S, lo, hi, seed=seed, return_counts=True)
    got, nd = got.cpu().double().numpy(), nd.cpu().numpy()
    assert f.last_unfilled == 0 and np.isfinite(got).all(), tag
    assert ((got >= lo) & (got <= hi)).all(), tag
    err = np.abs((got - ref) / (hi - lo).astype(np.float64)).max(-1)
    rounds = f.last_sample_stats["rounds"]
    print(f"{tag} {len(x)} x {S}: max err / box {err.max():.2e}, attempts {nd.tolist()} oracle {np.asarray(rnd).tolist()}, rounds {rounds}")
    assert np.array_equal(nd, np.asarray(rnd)), (tag, nd, rnd)
    assert (err <= 1e-4).all(), (tag, err.max())
    return rounds


@pytest.mark.parametrize("D,H,NB,sf", PC.GRID, ids=PC.IDS)
def test_given_noise_meets_the_fp64_oracle(D, H, NB, sf):
    """k_maf_find16s in its given-noise mode (rc 3: the fused pass functions), 1 row and 390 rows."""
    ospec, spec, flat, _, x = PC.make(D, H, NB, sf, B=390)
    z = np.random.default_rng(7).normal(size=(390, D)).astype(np.float32)
    f = _flow(spec, flat, D, H)
    rth, _ = oracle_inverse(ospec, flat, z, x, torch.float64)
    scale = np.asarray(ospec.theta_std)
    for n in (1, 390):
        th, _ = f.inverse_sampler(z[:n], x[:n])
        assert f.last_sampler_rc == 3, f.last_sampler_rc
        th = th.cpu().numpy()
        assert np.isfinite(th).all()
        err = np.abs((th.astype(np.float64) - rth[:n]) / scale).max(-1)
        print(f"D={D} H={H} NB={NB} {sf} rows={n}: max |dtheta|/sigma {err.max():.2e}")
        assert (err < 2e-4).all(), err.max()


@pytest.mark.parametrize("D,H,NB,sf", PC.GRID, ids=PC.IDS)
def test_catalogues_in_a_wide_box_draw_for_draw(D, H, NB, sf):
    """k_maf_samp16 in the 3 % .. 97 % box of the first galaxy, where first attempts mostly pass: both tiles of a wave engaged
    and partly filled."""
    ospec, spec, flat, _, x = PC.make(D, H, NB, sf, B=3)
    lo, hi = PC.box(ospec, spec, flat, x[0], 0.03, 400)
    f = _flow(spec, flat, D, H)
    _assert_fused(f, x)
    for M, S in PC.CATALOGUES:
        ref, rnd = OP.sample(ospec, torch.as_tensor(flat), x[:M], S, PC.SEED_WIDE, lo, hi, dtype=torch.float32)
        _check_catalogue(f"D={D} H={H} NB={NB} {sf} wide", f, x[:M], S, PC.SEED_WIDE, lo, hi, ref, rnd)


@pytest.mark.parametrize("D,H,NB,sf", PC.GRID, ids=PC.IDS)
def test_catalogues_in_a_narrow_box_draw_for_draw(D, H, NB, sf, golden):
    """The same catalogues in a box that an attempt meets about once in a thousand: the open slots are retried with several
    attempts side by side (the queue widens a retry up to 64 attempts: inside a tile, across the wave's two tiles, across waves --
    the sampler reports no widths, so which ones a run reached is not asserted; a mis-keyed attempt at any width shows as another
    draw or attempt count), and the slots that use up the persistent launch's first window are filled by the find / resolve
    launches, which is asserted."""
    ospec, spec, flat, _, x = PC.make(D, H, NB, sf, B=1)
    name = PC.IDS[PC.GRID.index((D, H, NB, sf))]
    lo, hi = golden[name + " lo"], golden[name + " hi"]
    draws, used = golden[name + " draws"].astype(np.float64), golden[name + " used"].astype(np.int64)
    f = _flow(spec, flat, D, H)
    _assert_fused(f, x)
    rounds = 0
    for M, S in PC.CATALOGUES:
        xm = np.repeat(x[:1], M, axis=0)   # (the same galaxy M times: every one of them sees the box)
        ref, rnd = draws[:M * S].reshape(M, S, D), used[:M * S].reshape(M, S).sum(1)
        rounds = max(rounds, _check_catalogue(f"D={D} H={H} NB={NB} {sf} narrow", f, xm, S, PC.SEED_NARROW, lo, hi, ref, rnd))
    assert used.max() > 1024 and rounds >= 3   # the persistent launch and at least one find / resolve pair


@pytest.mark.parametrize("D,H,NB,sf", PC.GRID, ids=PC.IDS)
def test_a_galaxy_alone_equals_its_place_in_a_ragged_catalogue(D, H, NB, sf):
    """131 galaxies x 5 draws = 655 slots (five 128-item iterations and a ragged sixth; a tile of 16 draws holds three or four
    galaxies, a wave's pair of tiles six or seven): a galaxy sampled alone at its row offset equals its place in the catalogue
    bit for bit -- its Philox counters do not depend on which half of the wave draws them."""
    ospec, spec, flat, _, x = PC.make(D, H, NB, sf, B=131)
    lo, hi = PC.box(ospec, spec, flat, x[0], 0.01, 800)
    f = _flow(spec, flat, D, H)
    _assert_fused(f, x)
    whole = f.sample(x, 5, lo, hi, seed=17).cpu().numpy()
    try:
        for g in (0, 64, 130):
            f.set_sample_row_offset(g)
            alone = f.sample(x[g:g + 1], 5, lo, hi, seed=17).cpu().numpy()
            assert np.array_equal(alone[0], whole[g], equal_nan=True), g
    finally:
        f.set_sample_row_offset(0)
    assert np.isfinite(whole).mean() > 0.9
