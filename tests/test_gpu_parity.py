"""GPU parity: HIP path (through the C ABI) vs the CPU oracle on identical seeded inputs.

Tolerances (north_star): |delta log_prob| < 1e-4 against the fp32 AND the fp64 oracle.
Samples: exact-from-given-noise within 2e-4 relative to the parameter scale; Philox sampler draw
for draw except for a tiny fraction of accept/reject flips at the box boundary.
"""
import numpy as np
import pytest
import torch

from cases import CASES, make_case, oracle_inverse, oracle_log_prob
from oracle import posterior as OP
from sweep_cases import compare_draws

pytestmark = pytest.mark.gpu

LOGP_TOL = 1e-4


def _flow(spec, flat):
    from synference_amd.engine import HipFlow
    f = HipFlow(spec, "cuda:0")
    f.set_params(torch.as_tensor(flat))
    return f


@pytest.mark.parametrize("name", list(CASES))
def test_log_prob_matches_oracle(name):
    ospec, spec, flat, theta, x = make_case(name, B=333)  # ragged: not a multiple of the tile
    f = _flow(spec, flat)
    got = f.log_prob(theta, x).cpu().double().numpy()
    ref64 = oracle_log_prob(ospec, flat, theta, x, torch.float64)
    ref32 = oracle_log_prob(ospec, flat, theta, x, torch.float32)
    assert np.isfinite(got).all()
    assert np.abs(got - ref64).max() < LOGP_TOL, np.abs(got - ref64).max()
    assert np.abs(got - ref32).max() < LOGP_TOL, np.abs(got - ref32).max()


@pytest.mark.parametrize("name", list(CASES))
def test_inverse_from_noise_matches_oracle(name):
    ospec, spec, flat, theta, x = make_case(name, B=130)
    rng = np.random.default_rng(5)
    z = rng.normal(size=theta.shape).astype(np.float32)
    f = _flow(spec, flat)
    th, ld = f.inverse(z, x)
    th, ld = th.cpu().double().numpy(), ld.cpu().double().numpy()
    rth, rld = oracle_inverse(ospec, flat, z, x, torch.float64)
    scale = np.asarray(ospec.theta_std)
    assert np.abs((th - rth) / scale).max() < 2e-4, np.abs((th - rth) / scale).max()
    assert np.abs(ld - rld).max() < 2e-4, np.abs(ld - rld).max()
    # round trip through the HIP density direction: log p(theta) = log N(z) - logdet_inverse
    lp = f.log_prob(torch.as_tensor(th, dtype=torch.float32), x).cpu().double().numpy()
    ref = -0.5 * (z.astype(np.float64) ** 2).sum(1) - 0.5 * spec.D * np.log(2 * np.pi) - ld
    assert np.abs(lp - ref).max() < 5e-4, np.abs(lp - ref).max()


@pytest.fixture
def sampler_mode():
    """Sets the process-wide arithmetic of the samplers' hidden blocks (sf_set_sampler_fp32: 1 fp32, 0 split bf16 x3, -1 the
    per-kind default: MAF fp32, NSF split) for one test and restores the default afterwards."""
    from synference_amd import _lib
    lib = _lib.load()
    yield lib.sf_set_sampler_fp32
    lib.sf_set_sampler_fp32(-1)


@pytest.mark.parametrize("name", ["maf_cfg1", "maf_span6", "maf_span_h64", "maf_d4", "maf_d3", "maf_nb1", "nsf_cfg3", "nsf_odd", "nsf_k16", "nsf_h69"])
def test_sampler_arithmetic_from_given_noise(name, sampler_mode):
    """The persistent sampler's OWN pass functions, fed GIVEN noise (sf_flow_inverse_from_noise_sampler), must meet the fp64
    oracle within 1e-4 of the parameter scale on EVERY row -- no exempt fraction, no Philox, no rejection in between -- in
    both arithmetic modes: the default of a MAF (round 5: every product on v_mfma_f32_16x16x4_f32, return code 2) and the
    split-bf16 x3 hidden blocks (the default of an NSF's sampler image and the opt-in fast mode of a MAF, return code 0).
    Measured (round 3, 4 099 rows): maf_cfg1 split 6.2e-5 / fp32 2.2e-5, maf_span6 1.8e-5 / 5.1e-6, maf_span_h64 8.3e-6 / 2.9e-6."""
    ospec, spec, flat, theta, x = make_case(name, B=4099)
    rng = np.random.default_rng(17)
    z = rng.normal(size=theta.shape).astype(np.float32)
    f = _flow(spec, flat)
    rth, _ = oracle_inverse(ospec, flat, z, x, torch.float64)
    scale = np.asarray(ospec.theta_std)
    errs = {}
    # return codes: 3 = the fp32 unrolled kernels with the fused first layer (aligned placement, D 3..5: cfg1, d4, d3, nb1),
    # 2 = the two-layer fp32 pass functions (span placements), 0 = split-bf16 x3, 1 = the generic fp32 path
    maf_rc = 3 if name in ("maf_cfg1", "maf_d4", "maf_d3", "maf_nb1") else 2
    for mode, want_rc in ((-1, maf_rc if name.startswith("maf") else 0), (0, 0), (1, maf_rc if name.startswith("maf") else 1)):
        sampler_mode(mode)
        th, _ = f.inverse_sampler(z, x)
        assert f.last_sampler_rc == want_rc, (name, mode, f.last_sampler_rc)
        errs[mode] = np.abs((th.cpu().double().numpy() - rth) / scale).max()
        assert errs[mode] <= 1e-4, (mode, errs[mode])
    # and the generic all-fp32 hook on the same rows
    th32, _ = f.inverse(z, x)
    err32 = np.abs((th32.cpu().double().numpy() - rth) / scale).max()
    assert err32 <= 1e-4, err32
    if name.startswith("maf"):   # the fp32 sampler is as close to the oracle as the density-side fp32 kernels
        assert errs[1] <= max(3.0 * err32, 2e-5), (errs, err32)
    print(f"{name}: max |dtheta|/sigma default {errs[-1]:.2e}, split-bf16 x3 {errs[0]:.2e}, fp32 {errs[1]:.2e}, generic fp32 hook {err32:.2e}")


def test_tiny_and_empty_batches():
    ospec, spec, flat, theta, x = make_case("maf_cfg1", B=3)
    f = _flow(spec, flat)
    got = f.log_prob(theta, x).cpu().double().numpy()
    assert np.abs(got - oracle_log_prob(ospec, flat, theta, x)).max() < LOGP_TOL
    got1 = f.log_prob(theta[:1], x[:1]).cpu().double().numpy()
    assert abs(got1[0] - got[0]) < 1e-6
    assert f.log_prob(theta[:0], x[:0]).numel() == 0


@pytest.mark.parametrize("name", ["maf_cfg1", "nsf_cfg3", "nsf_odd", "nsf_h69", "maf_span6", "maf_d2_span", "maf_d4", "maf_d3", "maf_sig2", "nsf_d1",
                                  "nsfar_cfg1", "nsfar_small", "nsfar_d1", "nsfar_wide", "nsfar_h180", "nsfar_k4", "nsfar_thin", "nsfar_two", "nsfar_33", "mafar_cfg1",
                                  "mafar_small"])
def test_sampler_matches_oracle_draw_for_draw(name):
    _draw_for_draw(name)


@pytest.mark.parametrize("name", ["maf_cfg1", "maf_span6", "maf_d2_span", "maf_d4", "maf_d3", "maf_sig2", "maf_nb1"])
def test_split_bf16_sampler_matches_oracle_draw_for_draw(name, sampler_mode):
    """The opt-in fast mode of a MAF (sf_set_sampler_fp32(0): hidden blocks as split-bf16 x3 products) under the same
    draw-for-draw bar as the default fp32 sampler."""
    sampler_mode(0)
    _draw_for_draw(name)


def _draw_for_draw(name, flat=None, case=make_case):
    """``case``: a make_case-shaped factory (name, B=, spread=) for other weights on the same shapes; ``flat``: other parameters for
    the factory's flow."""
    ospec, spec, flat0, theta, x = case(name, B=6, spread=0.2)
    flat = flat0 if flat is None else flat
    S, seed = 257, 2025
    # prior box from the 3%..97% quantiles of unbounded draws: ~60-75% acceptance, so the
    # rejection rounds are exercised for real
    free, _ = OP.sample(ospec, torch.as_tensor(flat), x, 400, 99, dtype=torch.float32)
    lo = np.quantile(free.reshape(-1, spec.D), 0.03, axis=0).astype(np.float32)
    hi = np.quantile(free.reshape(-1, spec.D), 0.97, axis=0).astype(np.float32)
    f = _flow(spec, flat)
    got, nd = f.sample(x, S, lo, hi, seed=seed, return_counts=True)
    got, nd = got.cpu().double().numpy(), nd.cpu().numpy()
    assert f.last_unfilled == 0
    ref, rnd = OP.sample(ospec, torch.as_tensor(flat), x, S, seed, lo, hi, dtype=torch.float32)
    # 1e-4 of the box width on EVERY draw; the only exemption is a boundary accept/reject flip, which the galaxy's attempt count
    # shows (the rule itself: sweep_cases.compare_draws, shared with tests/test_gpu_sweep_sampler.py)
    compare_draws(got, nd, ref, rnd, lo, hi, S)


def test_sampler_unbounded_and_acceptance():
    ospec, spec, flat, theta, x = make_case("maf_cfg1", B=4, spread=0.2)
    f = _flow(spec, flat)
    got = f.sample(x, 64, seed=7).cpu().double().numpy()
    ref, _ = OP.sample(ospec, torch.as_tensor(flat), x, 64, 7, dtype=torch.float32)
    # (unbounded: every slot is its first attempt, nothing is exempt; 1e-4 of the parameter scale)
    assert np.abs((got - ref) / np.asarray(ospec.theta_std)).max() <= 1e-4
    lo = (np.asarray(ospec.theta_mean) - 1.0 * np.asarray(ospec.theta_std)).astype(np.float32)
    hi = (np.asarray(ospec.theta_mean) + 1.0 * np.asarray(ospec.theta_std)).astype(np.float32)
    acc = f.acceptance(x, 4000, lo, hi, seed=11).cpu().numpy()
    racc = OP.acceptance(ospec, torch.as_tensor(flat), x, 4000, 11, lo, hi)
    assert np.abs(acc - racc).max() < 2e-3, (acc, racc)


def test_autoregressive_nsf_slots_acceptance_and_exhaustion():
    """The lampe-backend flow (sf_nsfar.hip) through the rest of the sampling ABI: listed slots reproduce the whole-catalogue
    draws, acceptance counts follow the oracle, and a box nothing falls into gives NaN rows + the attempt ceiling."""
    ospec, spec, flat, theta, x = make_case("nsfar_cfg1", B=5, spread=0.2)
    f = _flow(spec, flat)
    S = 96
    free = f.sample(x, 512, seed=3).cpu().double().numpy()
    ref_free, _ = OP.sample(ospec, torch.as_tensor(flat), x, 512, 3, dtype=torch.float32)
    assert np.abs((free - ref_free) / np.asarray(ospec.theta_std)).max() <= 1e-4
    lo = np.quantile(free.reshape(-1, spec.D), 0.05, axis=0).astype(np.float32)
    hi = np.quantile(free.reshape(-1, spec.D), 0.95, axis=0).astype(np.float32)
    whole = f.sample(x, S, lo, hi, seed=21)
    slots = torch.arange(0, len(x) * S, 7, dtype=torch.int32, device="cuda")
    part = torch.full_like(whole, float("nan"))
    assert f.sample_slots(x, S, slots, part, lo, hi, seed=21) == 0
    idx = slots.long()
    assert torch.equal(part.reshape(-1, spec.D)[idx], whole.reshape(-1, spec.D)[idx])
    acc = f.acceptance(x, 4000, lo, hi, seed=11).cpu().numpy()
    racc = OP.acceptance(ospec, torch.as_tensor(flat), x, 4000, 11, lo, hi)
    assert np.abs(acc - racc).max() < 2e-3, (acc, racc)
    # a long list (>= 4096 entries: walked across 4096 pieces, the cover has holes) against the whole-catalogue call
    xb = np.tile(x, (13, 1))[:64]
    big = f.sample(xb, 256, lo, hi, seed=33)
    lst = torch.arange(1, 64 * 256, 3, dtype=torch.int32, device="cuda")
    part = torch.full_like(big, float("nan"))
    assert f.sample_slots(xb, 256, lst, part, lo, hi, seed=33) == 0
    assert torch.equal(part.reshape(-1, spec.D)[lst.long()], big.reshape(-1, spec.D)[lst.long()])
    untouched = torch.ones(64 * 256, dtype=torch.bool, device="cuda")
    untouched[lst.long()] = False
    assert torch.isnan(part.reshape(-1, spec.D)[untouched]).all()
    far_lo, far_hi = (hi + 50.0).astype(np.float32), (hi + 51.0).astype(np.float32)
    got, nd = f.sample(x[:2], 8, far_lo, far_hi, seed=1, max_attempts=5, return_counts=True)
    assert torch.isnan(got).all() and f.last_unfilled == 16 and (nd.cpu().numpy() == 8 * 5).all()


def test_lampe_sampler_kernel_selection():
    """Which sampling kernel a lampe-backend flow takes (describe()): the 16-candidate register-tile kernels (sf_nsfar16.hip) for
    2 <= D <= 8 with at most 32 hidden units per type (one tile per type up to 16, two above) and D + C <= 32, the 64-sample LDS kernel
    otherwise; k-steps per hidden block = ceil(units per tile / 4)."""
    want = {"nsfar_cfg1": (1, 3, 1), "nsfar_small": (1, 2, 1), "nsfar_wide": (1, 2, 1), "nsfar_k4": (1, 4, 1), "nsfar_thin": (1, 2, 1),
            "mafar_cfg1": (1, 3, 1), "nsfar_h180": (1, 4, 2), "nsfar_two": (1, 3, 2), "nsfar_d1": (0, None, None), "nsfar_33": (0, None, None)}
    for name, (tiles16, ks, tpt) in want.items():
        ospec, spec, flat, theta, x = make_case(name, B=2)
        d = _flow(spec, flat).describe()
        assert d["sampler_tiles16"] == tiles16, (name, d["sampler_tiles16"])
        if tiles16:
            assert d["s16_ks"] == ks and d["s16_tpt"] == tpt and d["s16_nt"] == spec.D * tpt and d["s16_ni"] == (spec.D + spec.C + 15) // 16, (name, d)


def test_lampe_register_tile_sampler_equals_the_lds_sampler_on_a_full_chip(tmp_path):
    """A catalogue that fills the chip (2 000 rows x 256 draws, prior box, counts): the 16-candidate register-tile kernels
    (three workgroups per CU side by side) against the 64-sample LDS kernel of a child process (SF_AR_SAMP16=0) -- same seeds, so the
    same draws to rounding, except where a candidate within rounding of the box edge is accepted by one side only."""
    import os, subprocess, sys
    ospec, spec, flat, theta, x = make_case("nsfar_cfg1", B=2000, spread=0.2)
    f = _flow(spec, flat)
    S = 256
    free = f.sample(x[:64], 256, seed=3).reshape(-1, spec.D)
    lo = torch.quantile(free, 0.03, dim=0).cpu().numpy().astype(np.float32)
    hi = torch.quantile(free, 0.97, dim=0).cpu().numpy().astype(np.float32)
    got, nd = f.sample(x, S, lo, hi, seed=11, return_counts=True)
    assert f.describe()["sampler_tiles16"] == 1 and f.last_unfilled == 0
    got, nd = got.cpu().numpy(), nd.cpu().numpy()
    np.save(tmp_path / "lo.npy", lo); np.save(tmp_path / "hi.npy", hi)
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, numpy as np, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from cases import make_case; from synference_amd.engine import HipFlow\n"
            "ospec, spec, flat, theta, x = make_case('nsfar_cfg1', B=2000, spread=0.2)\n"
            "f = HipFlow(spec, 'cuda:0'); f.set_params(torch.as_tensor(flat).cuda())\n"
            "assert f.describe()['sampler_tiles16'] == 0\n"
            "o, nd = f.sample(x, 256, np.load(%r), np.load(%r), seed=11, return_counts=True)\n"
            "np.save(%r, o.cpu().numpy()); np.save(%r, nd.cpu().numpy())\n") % (
                os.path.dirname(here), here, str(tmp_path / "lo.npy"), str(tmp_path / "hi.npy"), str(tmp_path / "o.npy"), str(tmp_path / "nd.npy"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SF_AR_SAMP16="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    ref, rnd = np.load(tmp_path / "o.npy"), np.load(tmp_path / "nd.npy")
    assert np.isfinite(got).all() and ((got >= lo) & (got <= hi)).all()
    err = np.abs((got - ref) / np.asarray(ospec.theta_std, dtype=np.float32)).max(-1)      # (rows, draws)
    bad = err > 1e-4
    # a slot whose accepted attempt differs changes its row's attempt count: allow only count-explained mismatches, and few of them
    assert bad.sum() <= 8 and (bad.sum(1) <= np.abs(nd - rnd)).all(), (int(bad.sum()), np.abs(nd - rnd).sum())


def test_autoregressive_nsf_deep_tail_rounds_keep_the_lowest_accepted_attempt():
    """A box that accepts about one draw in a thousand: every slot outlives the persistent launch's 256-attempt window and is
    finished by the chip-wide FIND / RESOLVE rounds (sf_nsfar_sample) -- the draws and the attempt counts must still be the
    oracle's, which tries a slot's attempts one after the other and keeps the first accepted one."""
    ospec, spec, flat, theta, x = make_case("nsfar_small", B=3, spread=0.2)
    f = _flow(spec, flat)
    S, seed = 24, 77
    free, _ = OP.sample(ospec, torch.as_tensor(flat), x, 4000, 5, dtype=torch.float32)
    lo = np.quantile(free.reshape(-1, spec.D), 0.45, axis=0).astype(np.float32)
    hi = np.quantile(free.reshape(-1, spec.D), 0.55, axis=0).astype(np.float32)
    got, nd = f.sample(x, S, lo, hi, seed=seed, return_counts=True)
    got, nd = got.cpu().double().numpy(), nd.cpu().numpy()
    ref, rnd = OP.sample(ospec, torch.as_tensor(flat), x, S, seed, lo, hi, dtype=torch.float32)
    assert f.last_unfilled == 0 and np.isfinite(got).all() and ((got >= lo) & (got <= hi)).all()
    assert rnd.sum() > 300 * S * len(x)          # (the oracle really needed hundreds of attempts per slot)
    err = np.abs((got - ref) / (hi - lo).astype(np.float64)).max(-1)
    bad_g, off_g = (err > 1e-3).sum(1), np.abs(nd - rnd)
    # (a candidate within rounding of the box edge may be accepted by one side only: such a slot keeps another attempt and
    #  its row's attempt count differs; a narrow box has a long edge, so allow a few of the 72 slots)
    assert (bad_g <= np.minimum(off_g, 3)).all() and bad_g.sum() <= 4, (bad_g, off_g)


def test_autoregressive_nsf_deep_tail_rounds_on_the_lds_engine():
    """The deep-tail case on a shape that takes the 64-candidate LDS engine by itself (33 hidden units per type): the same
    persistent loop and FIND / RESOLVE rounds (sf_ar_sampler.h) around the other candidate routine, in-process.  Box: the
    45..55 % quantiles of the oracle's free draws; the oracle alone needs 59 073 attempts for the 72 slots of this seed (820 per
    slot, the assertion asks for more than 256), so most slots outlive the 256-attempt window.  Bars as in the register-tile test above."""
    ospec, spec, flat, theta, x = make_case("nsfar_33", B=3, spread=0.2)
    f = _flow(spec, flat)
    assert f.describe()["sampler_tiles16"] == 0
    S, seed = 24, 77
    free, _ = OP.sample(ospec, torch.as_tensor(flat), x, 4000, 5, dtype=torch.float32)
    lo = np.quantile(free.reshape(-1, spec.D), 0.45, axis=0).astype(np.float32)
    hi = np.quantile(free.reshape(-1, spec.D), 0.55, axis=0).astype(np.float32)
    got, nd = f.sample(x, S, lo, hi, seed=seed, return_counts=True)
    got, nd = got.cpu().double().numpy(), nd.cpu().numpy()
    ref, rnd = OP.sample(ospec, torch.as_tensor(flat), x, S, seed, lo, hi, dtype=torch.float32)
    assert f.last_unfilled == 0 and np.isfinite(got).all() and ((got >= lo) & (got <= hi)).all()
    assert rnd.sum() > 256 * S * len(x)          # (the rounds really ran)
    err = np.abs((got - ref) / (hi - lo).astype(np.float64)).max(-1)
    bad_g, off_g = (err > 1e-3).sum(1), np.abs(nd - rnd)
    assert (bad_g <= np.minimum(off_g, 3)).all() and bad_g.sum() <= 4, (bad_g, off_g)


@pytest.mark.parametrize("name", ["maf_cfg1", "nsf_cfg3", "nsf_odd", "maf_wide", "nsf_nb1", "maf_span6", "maf_span_h64"])
def test_context_table_round_equals_per_draw_round(name):
    """sf_flow_prepare_context only moves the context products out of the per-draw work: a dense round and a
    retry round over a slot list give the same draws and the same rejected set with and without the table.
    S = 7 puts several galaxies (and a ragged tail) inside every wave."""
    ospec, spec, flat, theta, x = make_case(name, B=37, spread=0.2)
    f = _flow(spec, flat)
    S, seed = 7, 31
    X = torch.as_tensor(x, dtype=torch.float32, device="cuda:0").contiguous()
    n = X.shape[0] * S
    free = f.sample(X, 300, seed=5).reshape(-1, spec.D).cpu().numpy()
    free = free[np.isfinite(free).all(-1)]
    lo = torch.as_tensor(np.quantile(free, 0.05, axis=0), dtype=torch.float32, device="cuda:0")
    hi = torch.as_tensor(np.quantile(free, 0.95, axis=0), dtype=torch.float32, device="cuda:0")

    def rounds(use_table):
        out = torch.full((X.shape[0], S, spec.D), float("nan"), dtype=torch.float32, device="cuda:0")
        rej = [torch.zeros(n, dtype=torch.int32, device="cuda:0") for _ in range(2)]
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        if use_table:
            f.prepare_context(X)
        f.sample_round(X, S, None, 0, n, 0, seed, lo, hi, out, rej[0], cnt)
        n0 = int(cnt.item())
        cnt.zero_()
        f.sample_round(X, S, rej[0], 0, n0, 1, seed, lo, hi, out, rej[1], cnt, attempts_per_slot=4)
        n1 = int(cnt.item())
        if use_table:
            f.release_context()
        return out.cpu().numpy(), set(rej[0][:n0].cpu().tolist()), set(rej[1][:n1].cpu().tolist())

    a, ra0, ra1 = rounds(False)
    b, rb0, rb1 = rounds(True)
    assert 0 < len(ra0) < n
    assert len(ra0 ^ rb0) <= 1 and len(ra1 ^ rb1) <= 1          # at most a boundary flip
    both = np.isfinite(a).all(-1) & np.isfinite(b).all(-1)
    assert both.sum() >= n - len(ra1) - 2
    scale = np.asarray(ospec.theta_std)
    assert np.abs((a[both] - b[both]) / scale).max() < 1e-4


def test_sampler_exhausted_attempts_give_nan_rows():
    ospec, spec, flat, theta, x = make_case("maf_small", B=2)
    f = _flow(spec, flat)
    lo = np.full(spec.D, 1e6, np.float32)
    hi = np.full(spec.D, 2e6, np.float32)        # unreachable box
    got = f.sample(x, 40, lo, hi, seed=1, max_attempts=3)
    assert f.last_unfilled == 80
    assert torch.isnan(got).all()


# ---------------------------------------------------------------------------------------------------
# opt-in bf16 mode (BASELINE configs[4]): hidden H x H layers with bf16 MFMA operands, fp32 accumulate
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["maf_cfg1", "nsf_cfg3", "nsf_odd", "maf_small", "maf_span_h64", "maf_span6"])
def test_bf16_hidden_mode_matches_bf16_emulating_oracle(name):
    """Tight: against the oracle with the SAME operand rounding (weights and hidden activations of the
    H x H layers rounded to bf16, wide accumulation).  Loose: the stated distance to the fp32 flow."""
    import dataclasses
    ospec, spec, flat, theta, x = make_case(name, B=150)
    spec_b = dataclasses.replace(spec, hidden_bf16=True)
    ospec_b = dataclasses.replace(ospec, hidden_bf16=True)
    f = _flow(spec_b, flat)
    got = f.log_prob(theta, x).cpu().double().numpy()
    ref_b = oracle_log_prob(ospec_b, flat, theta, x, torch.float64)
    ref_f = oracle_log_prob(ospec, flat, theta, x, torch.float64)
    # activations that sit on a bf16 rounding boundary can round differently (fp32 vs fp64 producer):
    # allow a small fraction of rows at the bf16 level, the rest must be tight
    err = np.abs(got - ref_b)
    assert np.median(err) < 2e-4 and (err > 5e-3).mean() < 0.05, (np.median(err), err.max())
    assert np.abs(got - ref_f).max() < 0.25, np.abs(got - ref_f).max()   # documented bf16-vs-fp32 tolerance
    assert np.abs(ref_b - ref_f).max() > 1e-5                             # the mode really changes arithmetic
    rng = np.random.default_rng(5)
    z = rng.normal(size=theta.shape).astype(np.float32)
    th, ld = f.inverse(z, x)
    rth, rld = oracle_inverse(ospec_b, flat, z, x, torch.float64)
    e2 = np.abs((th.cpu().double().numpy() - rth) / np.asarray(ospec.theta_std)).max(-1)
    assert np.median(e2) < 5e-4 and (e2 > 2e-2).mean() < 0.05, (np.median(e2), e2.max())
    # sampler runs and is reproducible in this mode
    s1 = f.sample(x[:4], 64, seed=3).cpu().numpy()
    assert np.isfinite(s1).all() and np.array_equal(s1, f.sample(x[:4], 64, seed=3).cpu().numpy())


def test_bf16_mode_leaves_training_in_fp32():
    import dataclasses
    from test_gpu_train import oracle_loss_grad
    ospec, spec, flat, theta, x = make_case("maf_cfg1", B=64)
    f = _flow(dataclasses.replace(spec, hidden_bf16=True), flat)
    loss, grad = f.loss_grad(torch.as_tensor(flat), theta, x, 1.0 / 64)
    rloss, rgrad = oracle_loss_grad(ospec, flat, theta, x)
    assert np.abs(loss.cpu().double().numpy() - rloss).max() < 1e-4
    assert np.abs(grad.cpu().double().numpy() - rgrad).max() < 2e-4 * np.abs(rgrad).max()


def test_get_params_round_trip_and_state_error():
    ospec, spec, flat, theta, x = make_case("nsf_odd", B=40)
    f = _flow(spec, flat)
    got = f.get_params().cpu().numpy()
    assert np.array_equal(got, np.asarray(flat, dtype=np.float32))
    f.loss_grad(torch.as_tensor(flat), theta, x, 1.0 / 40)
    with pytest.raises(RuntimeError, match="master copy"):
        f.get_params()
    f.set_params(torch.as_tensor(flat) * 0.5)
    assert np.allclose(f.get_params().cpu().numpy(), 0.5 * np.asarray(flat, dtype=np.float32))
