"""The cooperative training kernels on every instantiation (k_maf_trainc<TS, NI, NT, NG, NFS>, k_nsf_trainc<NT, OTQ> with one to three
input tiles) and on the shapes just outside their envelope, against fp64 autograd of the oracle, through HipFlow and the C ABI.

Configs, references and the rule: tests/trainer_cases.py -- per-row loss inside 4 x the fp32 oracle's own error + 1e-4; the gradient,
PER TENSOR of the flat layout, inside 4 x the fp32 oracle's error on that tensor + 2e-4 of that tensor's own largest gradient.
tests/test_cpu_trainer_cases.py holds that the configs reach every family and that the fp32 oracle stays inside a quarter of that
floor.  Every call prints one "TRAINER ..." line (run with -s); DESIGN.md section 0e has the table measured on an MI355X."""
import numpy as np
import pytest
import torch

import sharp_cases as SC
import step_cases as STEP
import step_model as SM
import sweep_cases as SW
import trainer_cases as TC
from test_gpu_step import Guarded, _bits, _desc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _np(t):
    return t.detach().cpu().double().numpy()


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a), dtype=dtype, device=DEV).contiguous()


def _flow(cfg):
    from synference_amd.engine import HipFlow
    return HipFlow(SW.sweep_case(cfg).spec, DEV)


def _label(cfg, f, B, dctx=False, what=""):
    return f"{TC.config_id(cfg)} B={B}{what} path {f.train_path(B, dctx)} {TC.family(f, B)}"


def _loss_grad(cfg, B):
    """loss_grad of B rows without a context gradient: the dispatch, the rule, and the same bits from a second call (paths 0 - 3 sum
    per-workgroup partials in a fixed order at these sizes)."""
    c, ref = SW.sweep_case(cfg, B), TC.reference(cfg, B)
    f = _flow(cfg)
    assert f.train_path(B, False) == TC.expected_path(cfg, B), (cfg, B, f.train_path(B, False))
    flat, theta, x = _dev(c.flat), _dev(c.theta), _dev(c.x)
    loss, grad = f.loss_grad(flat, theta, x, 1.0 / B)
    torch.cuda.synchronize()
    TC.check_rule(_label(cfg, f, B), c.ospec, _np(loss), _np(grad), ref)
    loss_2, grad_2 = f.loss_grad(flat, theta, x, 1.0 / B)
    torch.cuda.synchronize()
    assert _bits(grad, grad_2) and _bits(loss, loss_2), (cfg, B, "not reproducible", float((grad - grad_2).abs().max()))


@pytest.mark.parametrize("B", TC.BATCHES)
@pytest.mark.parametrize("cfg", TC.ALL_CONFIGS, ids=TC.config_id)
def test_loss_grad(cfg, B):
    _loss_grad(cfg, B)


@pytest.mark.parametrize("cfg", TC.EIGHT_WAVE, ids=TC.config_id)
def test_loss_grad_eight_wave_workgroups(cfg):
    assert TC.expected_path(cfg, TC.B_EIGHT_WAVE) == 2
    _loss_grad(cfg, TC.B_EIGHT_WAVE)


@pytest.mark.parametrize("cfg", TC.ALL_CONFIGS, ids=TC.config_id)
def test_weighted_rows(cfg):
    """loss_grad_rows over 300 training rows, 70 batch rows with duplicates and out of order, signed weights with an all-zero tile:
    weights are read by batch position, theta / x by gathered row."""
    B = TC.B_MAIN
    wd = TC.weighted(cfg)
    c = wd.case
    f = _flow(cfg)
    assert f.train_path(B, False) == TC.expected_path(cfg, B)
    loss = torch.full((B,), float("nan"), device=DEV)
    grad = torch.full((c.flat.size,), float("nan"), device=DEV)
    f.loss_grad_rows(_dev(c.flat), _dev(c.theta), _dev(c.x), _dev(wd.rows, torch.int64), 1.0 / B, grad, loss_out=loss, weights=_dev(wd.w))
    torch.cuda.synchronize()
    TC.check_rule(_label(cfg, f, B, what=" weighted rows"), c.ospec, _np(loss), _np(grad), wd.ref)


@pytest.mark.parametrize("cfg", TC.CONFIGS, ids=TC.config_id)
def test_context_gradient_where_the_cooperative_kernel_has_one(cfg):
    """A context-gradient request keeps a MAF with one input tile on the cooperative kernel (path 1): dctx [B, C] and the flat gradient
    of that call.  Every other config goes to the 32-row kernels, which tests/test_gpu_random_configs.py covers."""
    B = TC.B_MAIN
    f = _flow(cfg)
    fam = TC.family(f, B)
    if not (cfg[0] == "maf" and fam.NI == 1):
        assert f.train_path(B, True) == 0, (cfg, f.train_path(B, True))
        return
    assert f.train_path(B, True) == 1, (cfg, f.train_path(B, True))
    c, ref = SW.sweep_case(cfg, B), TC.reference(cfg, B)
    d64, d32 = TC.dctx_reference(cfg, B)
    dctx = torch.full((B, c.spec.C), float("nan"), device=DEV)
    loss, grad = f.loss_grad(_dev(c.flat), _dev(c.theta), _dev(c.x), 1.0 / B, dctx_out=dctx)
    torch.cuda.synchronize()
    label = _label(cfg, f, B, True, " dctx")
    d = _np(dctx)
    assert np.isfinite(d).all(), label
    SC.check_bar(label, d - d64, d32 - d64, SC.GRAD_FLOOR * np.abs(d64).max())
    TC.check_rule(label, c.ospec, _np(loss), _np(grad), ref)


@pytest.mark.parametrize("cfg", TC.STEP_CONFIGS, ids=TC.config_id)
def test_one_epoch_step(cfg):
    """One train_epoch of a single batch of 70 rows: the gradient the call leaves is loss_grad's, bit for bit, and parameters and
    moments are the fp64 model of tests/step_model.py applied to it (the comparison of test_gpu_step.py)."""
    B = TC.B_MAIN
    c = SW.sweep_case(cfg, B)
    n = c.flat.size
    f = _flow(cfg)
    theta, x = _dev(c.theta), _dev(c.x)
    order = torch.arange(B, dtype=torch.int64, device=DEV)
    step0, max_norm = 0, 0.5
    m0, v0 = STEP.epoch_warm_state(c.flat, step0)
    flat, m, v = Guarded(c.flat), Guarded(m0), Guarded(v0)
    grad, scratch = Guarded(np.full(n, np.nan, np.float32)), Guarded(np.zeros(2, np.float32))
    loss_sum = torch.full((), STEP.LOSS_SUM_START, dtype=torch.float64, device=DEV)
    f.train_epoch(flat.t, theta, x, order, 1, B, 1.0 / B, m.t, v.t, _desc(STEP.EPOCH_DESC), step0, max_norm, scratch.t, grad.t, loss_sum)
    torch.cuda.synchronize()
    assert all(g.intact() for g in (flat, m, v, grad, scratch)), "a sentinel changed"
    loss_rows, g_own = _flow(cfg).loss_grad(_dev(c.flat), theta, x, 1.0 / B)
    torch.cuda.synchronize()
    label = _label(cfg, f, B, what=" epoch")
    assert _bits(grad.t, g_own), (label, float((grad.t - g_own).abs().max()))
    g_dev = grad.numpy()
    SM.check_norm(label, float(scratch.numpy()[1]), g_dev)
    SM.check_step(label, flat.numpy(), m.numpy(), v.numpy(), SM.reference(c.flat, g_dev, m0, v0, step0 + 1, STEP.EPOCH_DESC, max_norm))
    want, got = float(loss_rows.double().sum().item()), float(loss_sum.item()) - STEP.LOSS_SUM_START
    assert abs(got - want) <= B * STEP.LOSS_PER_ROW, (label, got, want)
