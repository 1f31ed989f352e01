"""Per-sample weights of the training kernels against fp64 autograd: sf_flow_loss_grad_weighted and sf_flow_loss_grad_rows with
weights [B] are the vector-Jacobian product behind every backward() of FlowEstimator.

Reference (tests/vjp_cases.py): oracle.flows.log_prob in float64, (-(lp * w).sum() * grad_scale) differentiated by autograd on the rows
the call names; budget: the same in float32.  The bar is the one rule of tests/sharp_cases.py,

    quantile_q(|kernel - g64|) <= 4 * quantile_q(|g32 - g64|) + 2e-4 * max |g64|      for q in 0.5, 0.99, 1.0

per tensor of the flat layout (test_gpu_sharp._grad_per_tensor) and on the context gradient.  tests/test_cpu_vjp_cases.py holds, on the
reference alone, that the bar never exceeds 1e-3 of the largest gradient while a kernel that read the weights from the wrong position
would be off by at least 2e-2 of it.

Every test prints what it measured ("VJP ..." lines; run with -s).  DESIGN.md section 0d has the table measured on an MI355X."""
import dataclasses

import numpy as np
import pytest
import torch

import sharp_cases as SC
import step_cases as STEP
import vjp_cases as VC
from oracle import flows as OF
from test_gpu_sharp import _grad_per_tensor

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _np(t):
    return t.detach().cpu().double().numpy()


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a), dtype=dtype, device=DEV).contiguous()


def _call(f, i, w, scale, rows_form, want_dctx, loss_sum=None):
    """One weighted call in either form -> (loss [B], grad [P], dctx [B, C] or None), device tensors of their own."""
    B = len(i.theta_b)
    wt = None if w is None else _dev(w)
    dctx = torch.full((B, i.spec.C), float("nan"), device=DEV) if want_dctx else None
    if not rows_form:
        loss, grad = f.loss_grad(_dev(i.flat), _dev(i.theta), _dev(i.x), scale, weights=wt, dctx_out=dctx)
    else:
        loss, grad = torch.full((B,), float("nan"), device=DEV), torch.full((i.flat.size,), float("nan"), device=DEV)
        f.loss_grad_rows(_dev(i.flat), _dev(i.theta), _dev(i.x), _dev(i.rows, torch.int64), scale, grad, loss_sum=loss_sum,
                         loss_out=loss, weights=wt, dctx_out=dctx)
    torch.cuda.synchronize()
    return loss, grad, dctx


def _bits(a, b) -> bool:
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _vjp_line(label, e_kernel, e_ref, gmax):
    rs = SC.ratios(np.abs(e_kernel).ravel(), np.abs(e_ref).ravel())
    print(f"VJP {label}: ratio med/p99/max {rs[0]:.2f} {rs[1]:.2f} {rs[2]:.2f} | kernel max {np.abs(e_kernel).max():.3e} "
          f"ref max {np.abs(e_ref).max():.3e} max |ref| {gmax:.3e}")


def _check_call(c, f, pattern, rows_form, sk):
    """Everything the issue asks of one weighted call."""
    i = VC.inputs(c.name, c.B, rows_form)
    w, scale = VC.weights(c.name, c.B, pattern), VC.grad_scale(c.B, sk)
    ref = VC.reference(c.name, c.B, rows_form, pattern, sk)
    label = f"{VC.case_id(c)} {pattern} {'rows' if rows_form else 'direct'} {sk} (path {f.train_path(c.B, c.dctx)})"
    loss_sum = torch.full((), STEP.LOSS_SUM_START, dtype=torch.float64, device=DEV) if rows_form else None
    loss, grad, dctx = _call(f, i, w, scale, rows_form, c.dctx, loss_sum)
    g = _np(grad)
    gmax = np.abs(ref.g64).max()
    _vjp_line(label + " grad", g - ref.g64, ref.g32 - ref.g64, gmax)
    if c.dctx:
        _vjp_line(label + " dctx", _np(dctx) - ref.dx64, ref.dx32 - ref.dx64, np.abs(ref.dx64).max())
    assert np.isfinite(g).all(), label
    # the loss rows are not weighted: the oracle's, and the bits of the same call without weights
    SC.check_bar(label + " loss", _np(loss) - ref.loss64, ref.loss32 - ref.loss64, SC.LOGP_FLOOR)
    loss_sum_0 = torch.full((), STEP.LOSS_SUM_START, dtype=torch.float64, device=DEV) if rows_form else None
    loss_0, _, _ = _call(f, i, None, scale, rows_form, c.dctx, loss_sum_0)
    assert _bits(loss, loss_0), (label, "the weights changed the loss rows")
    if rows_form:
        want = float(loss.double().sum().item())
        for ls in (loss_sum, loss_sum_0):
            got = float(ls.item()) - STEP.LOSS_SUM_START
            print(f"VJP {label}: loss sum {got:.9g} rows {want:.9g} diff {abs(got - want):.2e} bar {c.B * STEP.LOSS_PER_ROW:.2e}")
            assert abs(got - want) <= c.B * STEP.LOSS_PER_ROW, (label, got, want)
    if pattern == "zeros":
        assert not g.any(), (label, np.abs(g).max())
        if c.dctx:
            d = _np(dctx)
            assert np.isfinite(d).all() and not d.any(), label
        return
    _grad_per_tensor(label + " grad", i.ospec, g, ref.g64, ref.g32)
    if c.dctx:
        d = _np(dctx)
        assert np.isfinite(d).all(), label
        SC.check_bar(label + " dctx", d - ref.dx64, ref.dx32 - ref.dx64, SC.GRAD_FLOOR * np.abs(ref.dx64).max())
        assert not d[w == 0].any(), (label, "a row of weight 0 has a context gradient", np.flatnonzero(d[w == 0].any(1))[:5])
        assert d[w != 0].any(1).all(), label
    if STEP.reproducible(STEP.EpochCase(c.name, c.B, "")):
        loss_2, grad_2, dctx_2 = _call(f, i, w, scale, rows_form, c.dctx)
        assert _bits(grad, grad_2) and _bits(loss, loss_2) and (not c.dctx or _bits(dctx, dctx_2)), (label, "not reproducible")


@pytest.mark.parametrize("pattern", VC.PATTERNS)
@pytest.mark.parametrize("case", VC.SMALL, ids=VC.case_id)
def test_weighted_gradient(case, pattern):
    from synference_amd.engine import HipFlow
    i = VC.inputs(case.name, case.B, False)
    f = HipFlow(i.spec, DEV)
    path = f.train_path(case.B, case.dctx)
    if case.path is not None:
        assert path == case.path, (VC.case_id(case), path, "the dispatch changed: this row no longer reaches " + case.what)
    else:
        print(f"VJP {VC.case_id(case)}: train_path {path} ({case.what})")
    for rows_form in ((False, True) if pattern in VC.BOTH_FORMS else (False,)):
        for sk in VC.SCALES:
            _check_call(case, f, pattern, rows_form, sk)


@pytest.mark.parametrize("name", VC.NO_DCTX)
def test_context_gradient_is_refused_where_there_is_none(name):
    """The one-parameter and lampe engines have no context-gradient path: SF_ERR_INVALID with a message, in both forms, with weights."""
    from synference_amd.engine import HipFlow
    c = next(c for c in VC.SMALL if c.name == name)
    for rows_form in (False, True):
        i = VC.inputs(name, c.B, rows_form)
        f = HipFlow(i.spec, DEV)
        with pytest.raises(RuntimeError, match="no context-gradient path"):
            _call(f, i, VC.weights(name, c.B, "uniform"), 1.0, rows_form, True)
        # ... and the handle is as good as before
        _, grad, _ = _call(f, i, VC.weights(name, c.B, "uniform"), 1.0, rows_form, False)
        ref = VC.reference(name, c.B, rows_form, "uniform", "sum")
        _grad_per_tensor(f"{name} after the refusal", i.ospec, _np(grad), ref.g64, ref.g32)


@pytest.mark.parametrize("case", VC.LARGE, ids=VC.case_id)
def test_weighted_gradient_large_batch(case):
    """8-wave workgroups, and batches at which some persistent workgroups take a second chunk: the weight of row chunk * 64 + ..."""
    from synference_amd.engine import HipFlow
    i = VC.inputs(case.name, case.B, False)
    f = HipFlow(i.spec, DEV)
    assert f.train_path(case.B, False) == case.path, (VC.case_id(case), f.train_path(case.B, False))
    for sk in VC.SCALES:
        _check_call(case, f, "signed", False, sk)


# ---------------------------------------------------------------------------------------------------------------------------
# the estimator: a reduction whose grad_output varies from row to row
# ---------------------------------------------------------------------------------------------------------------------------
def _twin(spec):
    """The oracle's spec of an estimator's flow."""
    kw = {fld.name: getattr(spec, fld.name) for fld in dataclasses.fields(OF.FlowSpec) if hasattr(spec, fld.name)}
    for k in ("theta_mean", "theta_std", "x_mean", "x_std"):
        if kw.get(k) is not None:
            kw[k] = np.asarray(kw[k], dtype=np.float64)
    return OF.FlowSpec(**kw)


def _estimator_against_the_twin(label, est, emb, theta, x):
    """(losses ** 2).sum() / B through FlowEstimator against the same reduction on the oracle twin, in fp64 and (budget) fp32."""
    import copy
    B = len(theta)
    losses = est.loss(torch.as_tensor(theta).cuda(), torch.as_tensor(x).cuda())
    ((losses ** 2).sum() / B).backward()
    ospec = _twin(est.spec)
    ref = {}
    for key, dt in (("f64", torch.float64), ("f32", torch.float32)):
        p = est.flat.detach().cpu().to(dt).requires_grad_(True)
        xs = torch.as_tensor(x).to(dt)
        net = None
        if emb is not None:
            net = copy.deepcopy(emb).to(dt)
            xs = net((xs - est.x_mean_raw.cpu().to(dt)) / est.x_std_raw.cpu().to(dt))
        rl = -OF.log_prob(ospec, p, torch.as_tensor(theta).to(dt), xs)
        ((rl ** 2).sum() / B).backward()
        ref[key] = (rl.detach().double().numpy(), p.grad.double().numpy(),
                    [] if net is None else [(n, q.grad.double().numpy()) for n, q in net.named_parameters()])
    (l64, g64, e64), (l32, g32, e32) = ref["f64"], ref["f32"]
    gout = 2.0 * l64 / B
    print(f"VJP {label}: grad_output mean {gout.mean():.4f} spread over the rows {gout.std():.2e} (min {gout.min():.4f} max {gout.max():.4f})")
    assert gout.std() > 1e-3 * np.abs(gout).mean(), "grad_output does not vary from row to row"
    SC.check_bar(f"{label} losses", _np(losses) - l64, l32 - l64, SC.LOGP_FLOOR)
    g = _np(est.flat.grad)
    _vjp_line(f"{label} flat.grad", g - g64, g32 - g64, np.abs(g64).max())
    _grad_per_tensor(f"{label} flat.grad", ospec, g, g64, g32)
    if emb is not None:
        for (n, q), (_, r64), (_, r32) in zip(est.embedding_net.named_parameters(), e64, e32):
            _vjp_line(f"{label} embedding {n}", _np(q.grad) - r64, r32 - r64, np.abs(r64).max())
            SC.check_bar(f"{label} embedding {n}", _np(q.grad) - r64, r32 - r64, SC.GRAD_FLOOR * np.abs(r64).max())


def test_estimator_maf_squared_loss_reduction():
    from synference_amd.estimator import FlowEstimator
    i = VC.inputs("maf_cfg1", 70, False)
    est = FlowEstimator(i.spec, torch.as_tensor(np.array(i.flat)), device=DEV).to("cuda")
    assert not est.has_embedding and est.flow.train_path(70, False) == 1
    _estimator_against_the_twin("estimator maf_cfg1", est, None, np.array(i.theta), np.array(i.x))


def test_estimator_nsf_with_embedding_net_squared_loss_reduction():
    import copy
    from synference_amd.estimator import build_flow
    rng = np.random.default_rng(0)
    B, D, C = 96, 4, 12
    theta = rng.normal(size=(B, D)).astype(np.float32)
    x = (rng.normal(size=(B, C)) * 3 + 1).astype(np.float32)
    torch.manual_seed(0)
    emb = torch.nn.Sequential(torch.nn.Linear(C, 16), torch.nn.SiLU(), torch.nn.Linear(16, 6))
    est = build_flow("nsf", theta, x, hidden_features=24, num_transforms=2, num_bins=6, embedding_net=copy.deepcopy(emb), device=DEV,
                     generator=torch.Generator().manual_seed(1)).to("cuda")
    assert est.spec.C == 6 and est.has_embedding
    _estimator_against_the_twin("estimator nsf + embedding", est, emb, theta, x)


@pytest.mark.parametrize("B", [70, 96, 512])
def test_embedding_mlp_gradient_repeats_to_the_bit(B):
    """sf_mlp_backward -- the conditioner of the one-parameter engine and the FCN embedding -- up to 16 tiles of 32 rows: every tile adds
    into a gradient image of its own and the gather sums them in tile order, so that the same inputs give the same bits (one shared
    image and f32 atomics repeated only up to two tiles: three addends do not commute)."""
    from synference_amd.embedding import FCN
    g = torch.Generator().manual_seed(B)
    m = FCN([48, 40, 8], "SiLU", n_input=21, generator=g).to("cuda")
    x, gout = (torch.randn(B, 21, generator=g) * 2).cuda(), torch.randn(B, 8, generator=g).cuda()
    grads = []
    for _ in range(4):
        m.flat.grad = None
        (m(x) * gout).sum().backward()
        grads.append(m.flat.grad.clone())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grads[0]).all()) and bool(grads[0].any())
    differ = [k for k in range(1, 4) if not _bits(grads[0], grads[k])]
    print(f"VJP FCN backward B={B}: {4 - len(differ)} of 4 calls give the same bits")
    assert not differ, (B, differ, float((grads[0] - grads[differ[0]]).abs().max()))
