"""The samplers over the whole configuration sweep (tests/sweep_cases.py), against oracle.posterior: draw for draw under a prior
box, unbounded, the acceptance estimate, and the persistent sampler's own pass functions on given noise.

tests/test_gpu_random_configs.py checks density, inverse and gradients on these configs; the named cases of
tests/test_gpu_parity.py reach only the 16-row MAF sampler and the two-tile, two-block coupling NSF.  Here every config runs the
sampler its shape selects -- the 32-row MAF sampler (H > 64, NB = 3 / 4, the image streamed from L2), the NSF sampler with PT = 3,
NB = 1 / 3 / 4, D = 2 or D > 8, a staged image in 1 / 2 / 4 parts or none, the lampe kernels at D > 8 -- with the geometry ragged
against 16-, 32- and 64-wide tiles.  The bars are those of test_gpu_parity.py; tests/test_cpu_sweep_cases.py shows that the fp32
oracle itself stays a decade under them on every config.

A lampe config that the handle refuses for LDS (sweep_cases.flow_or_lds_refusal) has no sampler: skipped."""
import functools

import numpy as np
import pytest
import torch

import sharp_cases as SC
import sweep_cases as SW
from oracle import posterior as OP

pytestmark = pytest.mark.gpu

CONFIGS = SW.sweep_configs()
SEED = 2025
# Geometry of the main runs: 5 rows x 97 draws = 485 slots.  No config needs a smaller S: on an MI355X the slowest draw-for-draw
# case (the lampe flow with D = 15, T = 4) takes 0.4 s, nearly all of it the CPU oracle.
M_MAIN, S_MAIN = 5, 97


def _flow(cfg):
    c = SW.sweep_case(cfg)
    f = SW.flow_or_lds_refusal(c.spec)
    if f is None:
        pytest.skip("the handle refuses this lampe shape: its rows do not fit the LDS")
    f.set_params(torch.as_tensor(np.array(c.flat)))
    return c, f


def _draw_for_draw(cfg, M, S):
    c, f = _flow(cfg)
    x, flat = np.array(c.x[:M]), torch.as_tensor(np.array(c.flat))
    lo, hi = SW.case_box(cfg, M)
    got, nd = f.sample(x, S, lo, hi, seed=SEED, return_counts=True)
    got, nd = got.cpu().double().numpy(), nd.cpu().numpy()
    assert f.last_unfilled == 0
    ref, rnd = OP.sample(c.ospec, flat, x, S, SEED, lo, hi, dtype=torch.float32)
    worst, flips = SW.compare_draws(got, nd, ref, rnd, lo, hi, S)
    print(f"SWEEP {SW.config_id(cfg)} M={M} S={S}: worst draw error {worst:.2e} of the box width where the counts agree, "
          f"count difference {flips} in {int(rnd.sum())} attempts")


@pytest.mark.parametrize("cfg", CONFIGS, ids=SW.config_id)
def test_sampler_matches_oracle_draw_for_draw(cfg):
    _draw_for_draw(cfg, M_MAIN, S_MAIN)


@pytest.mark.parametrize("cfg", SW.DENSE_WAVE_CONFIGS, ids=SW.config_id)
def test_sampler_matches_oracle_draw_for_draw_with_several_galaxies_per_wave(cfg):
    _draw_for_draw(cfg, 37, 7)


@pytest.mark.parametrize("cfg", CONFIGS, ids=SW.config_id)
def test_unbounded_sampler_matches_oracle_on_every_element(cfg):
    """No box: every slot is its first attempt and nothing is exempt; 1e-4 of max(sigma, |theta_ref - mean|)."""
    c, f = _flow(cfg)
    M, S = M_MAIN, S_MAIN
    x = np.array(c.x[:M])
    got = f.sample(x, S, seed=SEED).cpu().double().numpy()
    ref, _ = OP.sample(c.ospec, torch.as_tensor(np.array(c.flat)), x, S, SEED, dtype=torch.float32)
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    err = np.abs(got - ref) / SC.theta_scale(c.ospec, ref)
    print(f"SWEEP {SW.config_id(cfg)} unbounded: worst {err.max():.2e} of max(sigma, |theta - mean|)")
    assert err.max() <= 1e-4, err.max()


@pytest.mark.parametrize("cfg", CONFIGS, ids=SW.config_id)
def test_acceptance_matches_oracle(cfg):
    c, f = _flow(cfg)
    lo, hi = SW.case_box(cfg, M_MAIN)
    x = np.array(c.x[:3])
    acc = f.acceptance(x, 4000, lo, hi, seed=11).cpu().numpy()
    racc = OP.acceptance(c.ospec, torch.as_tensor(np.array(c.flat)), x, 4000, 11, lo, hi)
    assert np.abs(acc - racc).max() < 2e-3, (acc, racc)


@pytest.fixture
def sampler_mode():
    """sf_set_sampler_fp32 (1 fp32, 0 split bf16 x3, -1 the per-kind default) for one test; the default afterwards."""
    from synference_amd import _lib
    lib = _lib.load()
    yield lib.sf_set_sampler_fp32
    lib.sf_set_sampler_fp32(-1)


@functools.lru_cache(maxsize=None)
def _inverse_budget(cfg):
    """The oracle's inverse of the 300 given-noise rows in fp64 and fp32."""
    c = SW.sweep_case(cfg, 300)
    b = SC.budget(c.ospec, c.flat, c.theta, c.x, c.z, "inverse")
    return b["f64"][0], b["f32"][0]


@pytest.mark.parametrize("mode", [-1, 1])
@pytest.mark.parametrize("cfg", CONFIGS, ids=SW.config_id)
def test_sampler_pass_functions_from_given_noise(cfg, mode, sampler_mode):
    """The persistent sampler's own pass functions on 300 rows of given noise (no Philox, no rejection), in the default mode and in
    fp32: 4 x the fp32 oracle's own error + 1e-4 of max(sigma, |theta - mean|), at the median, the 99th percentile and the maximum.
    (Split-bf16 x3 on a MAF: tests/test_gpu_sharp.py holds its recorded xfail; not swept here.)"""
    _, f = _flow(cfg)
    c = SW.sweep_case(cfg, 300)
    th64, th32 = _inverse_budget(cfg)
    sampler_mode(mode)
    th, _ = f.inverse_sampler(np.array(c.z), np.array(c.x))
    scale = SC.theta_scale(c.ospec, th64)
    label = f"{SW.config_id(cfg)} inverse_sampler mode {mode} (last_sampler_rc {f.last_sampler_rc})"
    SC.check_bar(label, (th.cpu().double().numpy() - th64) / scale, (th32 - th64) / scale, SC.THETA_FLOOR)
