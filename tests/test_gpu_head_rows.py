"""GPU: the fused fp32 16-row MAF sampler with the (a, m) head rows as per-lane packed FMAs (sf_maf16_pass.h: sf_pass16g reads the
head-row region behind the compact image; k_maf_samp16 / k_maf_find16s, PREC 2), on the shapes of head_rows_model.py: D = 3, 4, 5
x one / two hidden blocks x the widths that give m16_k3 = 0 .. D - 1 x one / two transforms.

Bars: given noise against the fp64 oracle at the inverse's bar of test_gpu_parity.py (2e-4 of sigma on every row); catalogues
against the oracle sampler under the rule of test_gpu_parity.py (1e-4 of the box width on every draw, except as many draws of a
galaxy as its attempt count is off the oracle's; counts off by at most max(3, 1 %) in all); everything else bit for bit."""
import numpy as np
import pytest
import torch

import head_rows_model as HM
from cases import oracle_inverse
from oracle import posterior as OP

pytestmark = pytest.mark.gpu

S = 130   # draws per galaxy: more than one 128-item iteration, and ragged


def _flow(spec, flat):
    from synference_amd.engine import HipFlow
    f = HipFlow(spec, "cuda:0")
    d = f.describe()
    assert d["c16_fix"] == 1 and d["t16h_stride"] == HM.stride(spec.D), d
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


@pytest.mark.parametrize("D,H,NB,T", HM.GRID, ids=HM.IDS)
def test_given_noise_meets_the_fp64_oracle_and_a_nan_row_stays_alone(D, H, NB, T):
    """k_maf_find16s in its given-noise mode (rc 3: the fused pass functions): 1 and 3 x 130 rows against the fp64 oracle; then one
    row of noise made NaN -- its draw is NaN and every other row keeps its bits (a row is one lane of each of the four row groups:
    nothing of it may reach the 15 other samples of the tile through the cross-lane sums or the accumulators)."""
    ospec, spec, flat, _, x = HM.make(D, H, NB, T, B=3 * S)
    z = np.random.default_rng(7).normal(size=(3 * S, D)).astype(np.float32)
    f = _flow(spec, flat)
    rth, _ = oracle_inverse(ospec, flat, z, x, torch.float64)
    scale = np.asarray(ospec.theta_std)
    whole = None
    for n in (1, 3 * S):
        th, _ = f.inverse_sampler(z[:n], x[:n])
        assert f.last_sampler_rc == 3, f.last_sampler_rc
        th = th.cpu().numpy()
        assert np.isfinite(th).all()
        err = np.abs((th.astype(np.float64) - rth[:n]) / scale).max(-1)
        print(f"D={D} H={H} NB={NB} T={T} rows={n}: max |dtheta|/sigma {err.max():.2e}")
        assert (err < 2e-4).all(), err.max()
        whole = th
    zn = z.copy()
    zn[37, D - 1] = np.nan
    th, _ = f.inverse_sampler(zn, x)
    assert f.last_sampler_rc == 3
    th = th.cpu().numpy()
    assert np.isnan(th[37]).any()
    keep = np.arange(3 * S) != 37
    assert np.array_equal(th[keep], whole[keep])


def _draw_for_draw(ospec, spec, flat, x, q, seed, n_free, S=S):
    """The rule of test_gpu_parity.py::_draw_for_draw in the box of the q .. 1 - q quantiles."""
    free, _ = OP.sample(ospec, torch.as_tensor(flat), x[:1], n_free, 99, dtype=torch.float32)
    free = free.reshape(-1, spec.D)
    lo, hi = np.quantile(free, q, axis=0).astype(np.float32), np.quantile(free, 1.0 - q, axis=0).astype(np.float32)
    f = _flow(spec, flat)
    _assert_fused(f, x)
    got, nd = f.sample(x, S, lo, hi, seed=seed, return_counts=True)
    got, nd = got.cpu().double().numpy(), nd.cpu().numpy()
    assert f.last_unfilled == 0 and np.isfinite(got).all()
    assert ((got >= lo) & (got <= hi)).all()
    ref, rnd = OP.sample(ospec, torch.as_tensor(flat), x, S, seed, lo, hi, dtype=torch.float32)
    rnd = np.asarray(rnd)
    err = np.abs((got - ref) / (hi - lo).astype(np.float64)).max(-1)
    bad_g, off_g = (err > 1e-4).sum(1), np.abs(nd - rnd)
    print(f"D={spec.D} H={spec.H} NB={spec.NB} T={spec.T} q={q:.3g}: max err / box {err.max():.2e}, draws over 1e-4 {bad_g.tolist()}, "
          f"attempts {nd.tolist()} oracle {rnd.tolist()}, rounds {f.last_sample_stats['rounds']}")
    assert (bad_g <= off_g).all(), (bad_g, off_g, err.max())
    assert off_g.sum() <= max(3, 0.01 * rnd.sum())
    return f, got, nd, lo, hi


@pytest.mark.parametrize("D,H,NB,T", HM.GRID, ids=HM.IDS)
def test_catalogue_in_a_wide_box_draw_for_draw(D, H, NB, T):
    """k_maf_samp16: 3 galaxies x 130 draws in the 3 % .. 97 % box."""
    ospec, spec, flat, _, x = HM.make(D, H, NB, T, B=3)
    _, _, nd, _, _ = _draw_for_draw(ospec, spec, flat, x, 0.03, 2025, 400)
    assert (nd >= S).all() and nd.sum() > S * len(x)   # the box really rejected something


@pytest.mark.parametrize("D,H,NB,T", HM.GRID, ids=HM.IDS)
def test_catalogue_in_a_narrow_box_reaches_find_and_resolve(D, H, NB, T):
    """A box that an attempt meets about once in a thousand: slots use up the persistent launch's first window and are filled by the
    find / resolve launches (k_maf_find16s in its best / att_list modes).  Two near-identical galaxies, so that both see the box."""
    ospec, spec, flat, _, x = HM.make(D, H, NB, T, B=1)
    x = np.concatenate([x, x * np.float32(1.01)]).astype(np.float32)
    q = 0.5 * (1.0 - 1e-3 ** (1.0 / D))
    # (40 draws per galaxy: about a third of the 80 slots outlive the first 1 024 attempts, and the oracle sampler stays quick)
    f, _, nd, _, _ = _draw_for_draw(ospec, spec, flat, x, q, 31, 2000, S=40)
    assert f.last_sample_stats["rounds"] >= 3   # the persistent launch and at least one find / resolve pair


@pytest.mark.parametrize("D,H,NB,T", HM.GRID, ids=HM.IDS)
def test_a_galaxy_alone_equals_its_place_in_a_ragged_catalogue(D, H, NB, T):
    """131 galaxies x 5 draws = 655 slots (five 128-item iterations and a ragged sixth; a tile of 16 draws holds three or four
    galaxies): a galaxy sampled alone at its row offset equals its place in the catalogue bit for bit."""
    ospec, spec, flat, _, x = HM.make(D, H, NB, T, B=131)
    free, _ = OP.sample(ospec, torch.as_tensor(flat), x[:4], 200, 5, dtype=torch.float32)
    free = free.reshape(-1, D)
    lo, hi = np.quantile(free, 0.01, axis=0).astype(np.float32), np.quantile(free, 0.99, axis=0).astype(np.float32)
    f = _flow(spec, flat)
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
