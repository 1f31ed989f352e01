"""Conformance of the device flows far from the identity map: narrow bins, steep knots, linear tails, scales far from 1.

Every comparison is against the fp64 oracle under one rule (tests/sharp_cases.py, check_bar):

    quantile_q(|kernel - oracle64|) <= 4 * quantile_q(|oracle32 - oracle64|) + floor      for q in 0.5, 0.99, 1.0

with the reference's own fp32 error measured at run time on the same rows and the suite's near-identity bar as the floor.
tests/test_cpu_sharp_cases.py holds, on the reference alone, what keeps this from being vacuous: the fp32 oracle's error is capped
(a device defect of 4e-3 in log p on one row is always caught) and every bin, both tails, the narrow bins, the steep and flat
slopes and the extreme knot derivatives are really reached.

Every test prints the three ratios e_kernel / e_ref ("SHARP ..." lines; run with -s).  DESIGN.md section 0a has the table measured on
an MI355X."""
import numpy as np
import pytest
import torch

import sharp_cases as SC
from oracle import flows as OF

pytestmark = pytest.mark.gpu

SHARP = SC.SHARP      # one representative per kernel / template path
LD_FLOOR = 2e-4       # test_inverse_from_noise_matches_oracle: the log-determinant of the sampling direction


def _flow(c):
    from synference_amd.engine import HipFlow
    f = HipFlow(c.spec, "cuda:0")
    f.set_params(torch.as_tensor(np.array(c.flat)))
    return f


def _np(t):
    return t.cpu().double().numpy()


@pytest.mark.parametrize("name", SHARP)
def test_log_prob(name):
    c = SC.sharp_case(name)
    ref = SC.case_budget(name, "logp")
    got = _np(_flow(c).log_prob(np.array(c.theta), np.array(c.x)))
    assert np.isfinite(got).all(), np.flatnonzero(~np.isfinite(got))     # edge rows included
    SC.check_bar(f"{name} log_prob", got - ref["f64"], ref["f32"] - ref["f64"], SC.LOGP_FLOOR)


@pytest.mark.parametrize("name", SHARP)
def test_inverse_and_round_trip(name):
    c = SC.sharp_case(name)
    (th64, ld64, _), (th32, ld32, rt32) = (SC.case_budget(name, "inverse")[k] for k in ("f64", "f32"))
    f = _flow(c)
    th, ld = f.inverse(np.array(c.z), np.array(c.x))
    lp = _np(f.log_prob(th, np.array(c.x)))
    th, ld = _np(th), _np(ld)
    scale = SC.theta_scale(c.ospec, th64)
    SC.check_bar(f"{name} inverse theta", (th - th64) / scale, (th32 - th64) / scale, SC.THETA_FLOOR)
    SC.check_bar(f"{name} inverse logdet", ld - ld64, ld32 - ld64, LD_FLOOR)
    # log p(inverse(z)) = log N(z) - logdet through the device's two directions; budget: the fp32 oracle's own round trip
    SC.check_bar(f"{name} round trip", lp - (SC._std_normal_logp(c.z) - ld), rt32, SC.ROUNDTRIP_FLOOR)


@pytest.fixture
def sampler_mode():
    """sf_set_sampler_fp32 (1 fp32, 0 split bf16 x3, -1 the per-kind default) for one test; the default afterwards."""
    from synference_amd import _lib
    lib = _lib.load()
    yield lib.sf_set_sampler_fp32
    lib.sf_set_sampler_fp32(-1)


# the cases of test_sampler_arithmetic_from_given_noise that are in SHARP, with that test's return codes: 3 = the fp32 unrolled
# kernels with the fused first layer, 2 = the two-layer fp32 pass functions, 0 = split-bf16 x3, 1 = the generic fp32 path
_MAF_RC = {"maf_cfg1": 3, "maf_span6": 2}
_PASS_CASES = ["maf_cfg1", "maf_span6", "nsf_cfg3", "nsf_odd", "nsf_k16"]


# Measured on an MI355X: the opt-in split-bf16 x3 hidden blocks of a MAF's sampler (mode 0; the default of a MAF is fp32) are 20 - 50 x
# further from the fp64 oracle than the fp32 oracle is, with both fp32 modes inside the bar.  maf_span6 stays under the 1e-4 floor
# (7.0e-5); maf_cfg1 does not.  The NSF's split-bf16 default is level with its fp32 mode (ratios 1.1 / 1.0 / 0.8 on nsf_cfg3).
_SPLIT_MAF_CFG1 = pytest.mark.xfail(strict=True, reason="split-bf16 x3 MAF sampler on the sharp maf_cfg1: max |dtheta| / max(sigma, "
                                    "|theta - mean|) = 4.4e-4 = 35 x the fp32 oracle's 1.2e-5 (median 23 x, p99 30 x); bar 4 x + 1e-4")


@pytest.mark.parametrize("name,mode", [pytest.param(n, m, marks=_SPLIT_MAF_CFG1) if (n, m) == ("maf_cfg1", 0) else (n, m)
                                       for n in _PASS_CASES for m in (-1, 0, 1)])
def test_sampler_pass_functions(name, mode, sampler_mode):
    """The persistent sampler's own pass functions on given noise, in the default (-1), split-bf16 x3 (0) and fp32 (1) modes."""
    c = SC.sharp_case(name)
    (th64, _, _), (th32, _, _) = (SC.case_budget(name, "inverse")[k] for k in ("f64", "f32"))
    f = _flow(c)
    maf = name in _MAF_RC
    want_rc = {-1: _MAF_RC[name] if maf else 0, 0: 0, 1: _MAF_RC[name] if maf else 1}[mode]
    sampler_mode(mode)
    th, _ = f.inverse_sampler(np.array(c.z), np.array(c.x))
    assert f.last_sampler_rc == want_rc, (name, mode, f.last_sampler_rc)
    scale = SC.theta_scale(c.ospec, th64)
    label = {-1: "default", 0: "split-bf16 x3", 1: "fp32"}[mode]
    SC.check_bar(f"{name} inverse_sampler {label} (rc {want_rc})", (_np(th) - th64) / scale, (th32 - th64) / scale, SC.THETA_FLOOR)


def _grad_per_tensor(label, ospec, grad, g64, g32):
    """The bar on every tensor of the flat gradient, floor 2e-4 of max |g| as in test_gpu_train.py; prints the ratios over the whole
    vector and names the tensor with the largest max-ratio."""
    floor = SC.GRAD_FLOOR * np.abs(g64).max()
    worst, fails = ("", 0.0), []
    for n, s, o in OF.param_layout(ospec):
        k = int(np.prod(s))
        ek, er = np.abs(grad[o:o + k] - g64[o:o + k]), np.abs(g32[o:o + k] - g64[o:o + k])
        for q in SC.QUANTILES:
            a, b = np.quantile(ek, q), np.quantile(er, q)
            if not a <= SC.FACTOR * b + floor:
                fails.append((n, q, a, b))
        r = ek.max() / er.max() if er.max() > 0 else 0.0
        if r > worst[1] and ek.max() > 0.05 * floor:
            worst = (n, r)
    rs = SC.ratios(np.abs(grad - g64), np.abs(g32 - g64))
    print(f"SHARP {label}: ratio med/p99/max {rs[0]:.2f} {rs[1]:.2f} {rs[2]:.2f} | kernel max {np.abs(grad - g64).max():.3e} ref max "
          f"{np.abs(g32 - g64).max():.3e} floor {floor:.2e} (max |g| {np.abs(g64).max():.3e}) | worst tensor {worst[0]} x{worst[1]:.2f}")
    assert np.isfinite(grad).all(), label
    assert not fails, (label, fails[:5])
    return rs


@pytest.mark.parametrize("name", SHARP)
def test_loss_grad(name):
    """Loss rows and per-tensor parameter gradient of the training kernels; 512 rows, and 70 rows where that takes another kernel."""
    c = SC.sharp_case(name)
    from synference_amd.engine import HipFlow
    f = HipFlow(c.spec, "cuda:0")
    sizes = [512] + ([70] if f.train_path(70) != f.train_path(512) else [])
    flat = torch.as_tensor(np.array(c.flat))
    for B in sizes:
        ref = SC.case_budget(name, "grad", B)
        (l64, g64), (l32, g32) = ref["f64"], ref["f32"]
        loss, grad = f.loss_grad(flat, np.array(c.theta[:B]), np.array(c.x[:B]), 1.0 / B)
        loss, grad = _np(loss), _np(grad)
        tag = f"{name} loss_grad B={B} (path {f.train_path(B)})"
        SC.check_bar(tag + " loss", loss - l64, l32 - l64, SC.LOGP_FLOOR)
        _grad_per_tensor(tag + " grad", c.ospec, grad, g64, g32)


@pytest.mark.parametrize("name", ["nsf_cfg3", "maf_cfg1"])
@pytest.mark.parametrize("B", [70, 512])
def test_context_gradient(name, B):
    c = SC.sharp_case(name)
    from synference_amd.engine import HipFlow
    f = HipFlow(c.spec, "cuda:0")
    ref = SC.case_budget(name, "dctx", B)
    dctx = torch.empty(B, c.spec.C, device="cuda")
    f.loss_grad(torch.as_tensor(np.array(c.flat)), np.array(c.theta[:B]), np.array(c.x[:B]), 1.0, dctx_out=dctx)
    SC.check_bar(f"{name} dctx B={B} (path {f.train_path(B, True)})", _np(dctx) - ref["f64"], ref["f32"] - ref["f64"],
                 SC.GRAD_FLOOR * np.abs(ref["f64"]).max())


@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("name", [n for n in SHARP if n.startswith("maf_") or (n.startswith("nsf_") and n != "nsf_d1")])
def test_log_prob_grad(name, R):
    """d log p / d theta per row (the theta-gradient kernels), one context row per theta row and one per four."""
    c = SC.sharp_case(name)
    n = 512
    ref = SC.case_budget(name, "dtheta", n, R)
    (lp64, g64), (lp32, g32) = ref["f64"], ref["f32"]
    f = _flow(c)
    assert f.supports_log_prob_grad()
    lp, g = f.log_prob_grad(np.array(c.theta[:n]), np.array(c.x[:(n + R - 1) // R]), rows_per_x=R)
    std = np.asarray(c.ospec.theta_std)
    SC.check_bar(f"{name} log_prob_grad R={R} lp", _np(lp) - lp64, lp32 - lp64, SC.LOGP_FLOOR)
    SC.check_bar(f"{name} log_prob_grad R={R} dtheta", (_np(g) - g64) * std, (g32 - g64) * std, SC.GRAD_FLOOR * np.abs(g64 * std).max())


@pytest.mark.parametrize("name", ["nsfar_small", "nsfar_cfg1"])
def test_lampe_sampler_draw_for_draw(name):
    """The only route into the 16-candidate sampler's spline inverse (sf_nsfar16.hip): the Philox sampler draw for draw, under the
    unchanged rule of test_gpu_parity.py.  tests/test_cpu_sharp_cases.py confirms that the fp32 oracle meets the same rule against
    the fp64 oracle on these inputs."""
    from test_gpu_parity import _draw_for_draw
    c = SC.sharp_case(name, B=6, gain=SC.DRAW_GAINS[name], spread=0.2)
    assert _flow(c).describe()["sampler_tiles16"] == 1
    _draw_for_draw(name, case=SC.sharp_factory(SC.DRAW_GAINS[name]))
