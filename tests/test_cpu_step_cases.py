"""What keeps tests/test_gpu_step.py from passing vacuously, checked on the model and the case table alone (no GPU).

* the fp64 model of tests/step_model.py is torch.nn.utils.clip_grad_norm_ + torch.optim.Adam / AdamW in float64;
* the case table reaches every kernel path of sf_launch_adam with every hyper-parameter set and every clip regime, and the rule it
  sorts the cases by restates the source;
* the yardstick is usable: the float32 model stays within 2e-6 of a unit of the fp64 model on every case;
* a clip coefficient that is off by a part in a thousand -- which Adam's m / sqrt(v) hides from the parameters -- fails the bar on m
  and v.
"""
import os

import numpy as np
import pytest
import torch

import step_cases as SC
import step_model as SM
from cases import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARDSTICK_CAP = 2e-6


def _rel(a, b):
    """max over the elements of |a - b| / max(|b|, median |b|)."""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float((np.abs(a - b) / np.maximum(np.abs(b), np.median(np.abs(b)))).max())


@pytest.mark.parametrize("clip", ["active", "inactive"])
@pytest.mark.parametrize("hyper", list(SC.HYPERS))
def test_model_is_torch_adam_with_clip_grad_norm(hyper, clip):
    """Six steps in float64, the hyper-parameters those of the descriptor as doubles: 1e-12 relative on p, m, v and the norm.  torch
    keeps the bias corrections in double, so the model does too here (round_bc=False); what rounding them to float32 -- as
    sf_adam_apply does -- moves is bounded in the test below."""
    d = SC.HYPERS[hyper]
    lr, b1, b2, eps, wd = (float(t) for t in SM.desc_values(d))
    n = 1000
    p0 = SC.start_params(n, 11).astype(np.float64)
    pt = torch.nn.Parameter(torch.tensor(p0))
    opt = (torch.optim.AdamW if d.decoupled else torch.optim.Adam)([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0, np.zeros(n), np.zeros(n)
    for step in range(1, 7):
        g = SC.dense_gradient(n, (3.0, 0.01)[step % 2], 100 + step)
        gnorm = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
        max_norm = float(np.float32(gnorm / SC.ACTIVE_RATIO if clip == "active" else gnorm / SC.INACTIVE_RATIO))
        pt.grad = torch.tensor(g.astype(np.float64))
        tn = torch.nn.utils.clip_grad_norm_([pt], max_norm)
        opt.step()
        p, m, v, _, norm = SM.adam_step(p, g, m, v, step, d, max_norm, round_bc=False)
        st = opt.state[pt]
        assert abs(norm - tn.item()) <= 1e-12 * tn.item()
        assert _rel(p, pt.detach().numpy()) <= 1e-12, (step, _rel(p, pt.detach().numpy()))
        assert _rel(m, st["exp_avg"].numpy()) <= 1e-12 and _rel(v, st["exp_avg_sq"].numpy()) <= 1e-12
    assert np.abs(p - p0).max() > 1e-3                                   # the parameters really moved


@pytest.mark.parametrize("step", SC.STEPS)
def test_rounding_the_bias_corrections_moves_the_update_by_a_float32_rounding(step):
    d = SC.HYPERS["betas"]
    p = SC.start_params(500, 3)
    g = SC.dense_gradient(500, 1.0, 4)
    m, v = SM.warm_state(p, d, step, 5)
    a = SM.adam_step(p, g, m, v, step, d, 0.0)
    b = SM.adam_step(p, g, m, v, step, d, 0.0, round_bc=False)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])     # m and v do not see them
    assert (np.abs(a[3] - b[3]) <= 2.0 ** -23 * np.abs(b[3])).all()      # half an ulp each on bc1 and sqrt(bc2): 0.75 x 2^-23 at most
    bc = SM.bias_corrections(d, step)
    assert bc[0].dtype == np.float32 and bc[1].dtype == np.float32


def test_float32_model_rounds_every_operation():
    d = SC.HYPERS["adam_l2"]
    p, g = SC.start_params(300, 1), SC.dense_gradient(300, 3.0, 2)
    m, v = SM.warm_state(p, d, 2, 3)
    out = SM.adam_step(p, g, m, v, 2, d, 1.0, dtype=np.float32)
    assert all(np.asarray(a).dtype == np.float32 for a in out)
    # the descriptor's values, not the decimal ones: (1 - beta2) differs by 1.3e-5 relative between the two
    b2 = SM.desc_values(d)[2]
    assert b2 == np.float64(np.float32(0.999)) and abs((1 - b2) / (1 - 0.999) - 1) > 1e-5


# ---- the case table ---------------------------------------------------------------------------------------------------------
def test_path_rule_restates_the_source():
    src = open(os.path.join(ROOT, "synference_amd", "csrc", "sf_train.hip")).read()
    for line in ("if (n <= 131072 && ((uintptr_t)grad & 15) == 0) {",
                 "const bool vec = (n & 3) == 0 && (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) == 0;",
                 "const int nb = (int)((n + 4095) / 4096);",
                 "#define SF_ADAM_SHARES 256",
                 "const int blocks = (int)((n + 1023) / 1024 < SF_ADAM_SHARES ? (n + 1023) / 1024 : SF_ADAM_SHARES);"):
        assert src.count(line) == 1, line
    assert SC.FUSED_MAX == 131072 and SC.STRIDED_ABOVE == 256 * 1024


def test_table_covers_every_path_with_every_hyper_set_and_clip_regime():
    assert 35 <= len(SC.OPT_CASES) <= 45 and len(SC.OPT_BY_NAME) == len(SC.OPT_CASES)
    for path, shapes in SC.PATH_SHAPES.items():
        cs = [c for c in SC.OPT_CASES if c.path == path]
        assert len(cs) >= 3
        assert all(SC.path_of(c.n, c.offset) == path for c in cs), path
        assert {c.hyper for c in cs} == set(SC.HYPERS), path
        assert {c.regime for c in cs} == set(SC.REGIMES), path
        assert {c.step for c in cs} == set(SC.STEPS), path
        assert {(c.n, c.offset) for c in cs} == set(shapes), path
    want = {"fused_vec": {4, 4096, 4100, 131072}, "fused_scalar": {1, 3, 63, 4097, 10007, 131071}, "fused_scalar_align": {4096},
            "two_kernel": {131073, 131076, 300007}, "two_kernel_align": {4096}}
    assert {p: {n for n, _ in s} for p, s in SC.PATH_SHAPES.items()} == want
    assert {o for _, o in SC.PATH_SHAPES["fused_scalar_align"]} == {"p", "m", "v"}
    assert any(c.n > SC.STRIDED_ABOVE for c in SC.OPT_CASES if c.path == "two_kernel")
    for n, hyper, _ in SC.HANDLE_CASES:
        assert hyper in SC.HYPERS
    assert {SC.path_of(n, None) for n, _, _ in SC.HANDLE_CASES} == {"fused_vec", "two_kernel"}


@pytest.mark.parametrize("name", list(SC.OPT_BY_NAME))
def test_case_inputs_and_yardstick(name):
    """The inputs are what the case's name says, and the float32 model's error against the fp64 model is at most 2e-6 of a unit at the
    maximum (a few 1e-7 measured for m and v, 1e-8 relative for the norm): the bar 4 x e_ref + 2^-23 is never wide."""
    i = SC.opt_inputs(name)
    c = i.case
    g64 = i.g.astype(np.float64)
    norm = float(np.sqrt((g64 * g64).sum()))
    assert all(a.dtype == np.float32 and a.shape == (c.n,) for a in (i.p, i.g, i.m, i.v))
    assert np.isfinite(np.float32((g64 * g64).sum())) and np.isfinite(i.m).all() and (i.v >= 0).all()
    if c.regime in ("active", "sparse"):
        assert norm >= 1.5 * i.max_norm > 0
    elif c.regime == "inactive":
        assert 0 < norm <= 0.5 * i.max_norm
    elif c.regime == "zero":
        assert norm == 0 and i.max_norm > 0
    else:
        assert i.max_norm == {"off0": 0.0, "off_neg": -1.0}[c.regime] and norm > 0
    if c.regime == "sparse":
        k = max(1, c.n // 10)
        assert (i.g == 0).sum() >= k and (i.g == np.float32(1e-12)).sum() == k
    if c.n >= 63:
        assert 0.1 < (i.p == 0).mean() < 0.3
    assert ((i.m == 0).all() and (i.v == 0).all()) == (c.step == 1)
    ref = SC.opt_reference(name)
    assert all(np.isfinite(a).all() for a in (ref.p, ref.m, ref.v, ref.p32, ref.m32, ref.v32))
    zero = i.p == 0
    if not i.desc.decoupled:
        assert np.array_equal(ref.p[zero], -ref.update[zero])              # there the update itself is compared, in units of lr
    if c.regime == "zero" and c.step == 1 and i.desc.weight_decay == 0:
        assert np.array_equal(ref.p, i.p.astype(np.float64))               # parameters move only by decay
    yd = SM.yardstick(ref)
    worst = {k: float(e.max()) if e.size else 0.0 for k, e in yd.items()}
    nrel = abs(ref.norm32 - ref.norm) / ref.norm if ref.norm else 0.0
    print(f"{name}: float32 model max error in units m {worst['m']:.2e} v {worst['v']:.2e} p {worst['p']:.2e}; norm {nrel:.2e}")
    assert max(worst.values()) <= YARDSTICK_CAP and nrel <= YARDSTICK_CAP
    SM.check_step(name + " (float32 model)", ref.p32, ref.m32, ref.v32, ref)    # the yardstick passes its own bar


def test_wrong_clip_coefficient_fails_m_and_v_but_hides_in_the_parameters():
    """The defect the fused epoch could have: a clip norm taken from wrong shares.  A coefficient off by 1e-3 moves m by 1e-3 and v by
    2e-3 of a unit and fails the bar; in the parameters it is 1e-3 of eps / sqrt(v): the old comparison of parameters cannot see it."""
    name = next(c.name for c in SC.OPT_CASES if c.regime == "active" and c.step == 1 and c.n >= 4096 and c.hyper != "adam_l2")
    i, ref = SC.opt_inputs(name), SC.opt_reference(name)
    bad = SM.adam_step(i.p, i.g, i.m, i.v, i.case.step, i.desc, i.max_norm * 1.001, dtype=np.float32)
    with pytest.raises(AssertionError):
        SM.check_step("coefficient off by 1e-3", bad[0], bad[1], bad[2], ref)
    assert np.abs(bad[0].astype(np.float64) - ref.p).max() < 2e-6            # the bar of test_adam_step_matches_torch
    e_m = SM.unit_errors(bad[1], ref.m, ref.unit_m)
    assert 0.5e-3 < np.median(e_m) < 2e-3


def test_unit_zero_elements_must_be_exact():
    name = next(c.name for c in SC.OPT_CASES if c.regime == "zero" and c.step == 1)
    i, ref = SC.opt_inputs(name), SC.opt_reference(name)
    if i.desc.weight_decay == 0 or i.desc.decoupled:
        assert (ref.unit_m == 0).all() and (ref.unit_v == 0).all()
    m = np.array(ref.m32)
    m[0] = 1e-30
    if ref.unit_m[0] == 0:
        with pytest.raises(AssertionError, match="exactly"):
            SM.check_step("planted", ref.p32, m, ref.v32, ref)


# ---- the epoch cases ----------------------------------------------------------------------------------------------------------
def test_epoch_cases_are_the_gather_families():
    assert [(c.name, c.batch) for c in SC.EPOCH_CASES] == [
        ("maf_cfg1", 64), ("maf_t8", 96), ("maf_cli", 64), ("nsf_cfg3", 64), ("nsf_cfg3", 16416), ("nsf_h69", 64), ("maf_wide", 64),
        ("maf_wide", 600), ("nsf_d1", 64), ("nsfar_small", 64), ("mafar_small", 64)]
    assert all(c.name in CASES for c in SC.EPOCH_CASES)
    assert (16416 + 31) // 32 == 2 * 256 + 1                                  # one row tile past sf_nsfc_grid's cap on 256 CUs
    assert 600 > 512 and (600 + 31) // 32 > 16                                # the 32-row kernels leave per-tile replicas
    assert [SC.reproducible(c) for c in SC.EPOCH_CASES] == [True, True, True, True, False, True, True, False, True, False, False]
    assert SC.EPOCH_RUNS == [(0, 0.5), (5, 0.5), (0, 0.0)] and SC.EPOCH_DESC == SC.HYPERS["adamw"]
    assert set(SC.THREE_BATCH) | {SC.THREE_BATCH_LAMPE} <= {c.name for c in SC.EPOCH_CASES}


@pytest.mark.parametrize("case", [c for c in SC.EPOCH_CASES if c.batch <= 600], ids=lambda c: f"{c.name}-{c.batch}")
def test_epoch_inputs(case):
    for nb in (1, 3):
        i = SC.epoch_inputs(case.name, case.batch, nb)
        rows = case.batch + case.batch // 2
        assert i.theta.shape[0] == i.x.shape[0] == rows and i.order.shape == (nb * case.batch,) and i.order.dtype == np.int64
        assert 0 <= i.order.min() and i.order.max() < rows
        first = i.order[:case.batch]
        assert len(np.unique(first)) < case.batch                            # some rows repeated within one batch
    m, v = SC.epoch_warm_state(i.flat, 5)
    assert m.dtype == np.float32 and m.shape == i.flat.shape and (v > 0).all()
    m0, v0 = SC.epoch_warm_state(i.flat, 0)
    assert not m0.any() and not v0.any()
