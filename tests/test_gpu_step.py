"""Training-step conformance: the clip + Adam kernels (sf_adam_apply, sf_adam_step) and the fused epoch (sf_flow_train_epoch) against
the fp64 model of tests/step_model.py, on the cases of tests/step_cases.py.

The bar on m, v and p is sharp_cases.check_bar: quantile_q(|kernel - model64| / unit) <= 4 x quantile_q(|model32 - model64| / unit) +
2^-23 at q = 0.5, 0.99, 1.0, with the float32 model evaluated on the same inputs at run time.  The fused epoch is fed its OWN gradient
(the buffer the call leaves) into the model, so that Adam's amplification of gradient rounding does not enter: what is pinned is
everything after the gradient -- the norm from the gather's shares, the clip, the moments, the update, the loss sum."""
import ctypes as C

import numpy as np
import pytest
import torch

import step_cases as SC
import step_model as SM
from synference_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 64                       # sentinel floats on both sides of every buffer (256 bytes: the 16-byte alignment is kept)
SENTINEL = -12345.6787109375    # a float32 value
INVALID = -1                    # SF_ERR_INVALID


class Guarded:
    """``a`` inside a larger allocation with SENT sentinel floats on both sides; ``offset`` = 1 starts it one float further in."""

    def __init__(self, a, offset: int = 0):
        a = torch.as_tensor(np.asarray(a), dtype=torch.float32)
        self.n, self.lo = a.numel(), SENT + offset
        self.buf = torch.full((self.lo + self.n + SENT,), SENTINEL, dtype=torch.float32, device=DEV)
        self.t = self.buf[self.lo:self.lo + self.n]
        self.t.copy_(a)
        assert self.buf.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == 4 * offset and self.t.is_contiguous()
        self.before = self.buf.clone()

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def intact(self) -> bool:
        return bool((self.buf[:self.lo] == SENTINEL).all() and (self.buf[self.lo + self.n:] == SENTINEL).all())

    def untouched(self) -> bool:
        return torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32))

    def numpy(self):
        return self.t.cpu().numpy()


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


def _desc(d):
    return _lib.sf_adam_desc(d.lr, d.beta1, d.beta2, d.eps, d.weight_decay, int(d.decoupled))


def _bits(a, b) -> bool:
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------
# sf_adam_apply, one test per case
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.OPT_BY_NAME))
def test_adam_apply_matches_the_fp64_model(name, lib):
    i, ref = SC.opt_inputs(name), SC.opt_reference(name)
    c = i.case
    b = {k: Guarded(a, 1 if c.offset == k else 0) for k, a in (("p", i.p), ("g", i.g), ("m", i.m), ("v", i.v))}
    scratch = Guarded(np.zeros(2, np.float32))
    d = _desc(i.desc)
    _lib.check(lib.sf_adam_apply(b["p"].ptr, b["g"].ptr, b["m"].ptr, b["v"].ptr, c.n, C.byref(d), c.step, C.c_float(i.max_norm),
                                 scratch.ptr, _stream()))
    torch.cuda.synchronize()
    assert all(x.intact() for x in b.values()) and scratch.intact(), "a sentinel changed"
    assert b["g"].untouched(), "the gradient changed"
    SM.check_norm(name, float(scratch.numpy()[1]), i.g)
    SM.check_step(name, b["p"].numpy(), b["m"].numpy(), b["v"].numpy(), ref)


# ---------------------------------------------------------------------------------------------------------------------------
# the handle, the Python optimiser's state, the refusals
# ---------------------------------------------------------------------------------------------------------------------------
def _device_floats(lib, ptr, n):
    """n floats at a device address the library owns, as float64 (exact)."""
    out = np.empty(n, dtype=np.float64)
    _lib.check(lib.sf_copy_to_host_f64(ptr, out.ctypes.data_as(C.c_void_p), n, _stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n,hyper,max_norm", SC.HANDLE_CASES)
def test_adam_step_on_a_handle_is_adam_apply_on_caller_state(n, hyper, max_norm, lib):
    d = _desc(SC.HYPERS[hyper])
    h = C.c_void_p()
    _lib.check(lib.sf_opt_create(n, C.byref(d), C.byref(h)))
    try:
        p0 = torch.as_tensor(SC.start_params(n, 21), device=DEV)
        pa, pb = p0.clone(), p0.clone()
        m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        na, scratch = torch.zeros(1, device=DEV), torch.zeros(2, device=DEV)
        for step in range(1, 5):
            g = torch.as_tensor(SC.dense_gradient(n, (3.0, 0.01)[step % 2], 30 + step), device=DEV)
            _lib.check(lib.sf_adam_step(h, _lib.ptr(pa), _lib.ptr(g), C.c_float(max_norm), _lib.ptr(na), _stream()))
            _lib.check(lib.sf_adam_apply(_lib.ptr(pb), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), n, C.byref(d), step, C.c_float(max_norm),
                                         _lib.ptr(scratch), _stream()))
            torch.cuda.synchronize()
            assert _bits(pa, pb) and _bits(na, scratch[1:]), step
        hm, hv, hs = C.c_void_p(), C.c_void_p(), C.POINTER(C.c_int64)()
        _lib.check(lib.sf_opt_state(h, C.byref(hm), C.byref(hv), C.byref(hs)))
        assert hs.contents.value == 4
        assert np.array_equal(_device_floats(lib, hm, n), m.cpu().double().numpy())
        assert np.array_equal(_device_floats(lib, hv, n), v.cpu().double().numpy())
        assert (pa != p0).any() and bool(torch.isfinite(pa).all())
    finally:
        lib.sf_opt_destroy(h)


def test_hipadam_state_dict_round_trip():
    """3 steps, save, load into a fresh HipAdam, 2 more steps on both: the same bits."""
    from synference_amd.runner import HipAdam
    n = 4100
    p0 = torch.as_tensor(SC.start_params(n, 5), device=DEV)
    pa = p0.clone()
    a = HipAdam(pa, lr=3e-3, weight_decay=0.01, decoupled=True)
    grads = [torch.as_tensor(SC.dense_gradient(n, 1.0, 40 + k), device=DEV) for k in range(5)]
    for g in grads[:3]:
        a.step(g, 0.5)
    sd = a.state_dict()
    assert sd["step"] == 3 and sd["exp_avg"].device.type == "cpu"
    pb = pa.clone()
    b = HipAdam(pb, lr=3e-3, weight_decay=0.01, decoupled=True)
    b.load_state_dict(sd)
    assert b.step_count == 3
    for g in grads[3:]:
        a.step(g, 0.5)
        b.step(g, 0.5)
    torch.cuda.synchronize()
    assert _bits(pa, pb) and _bits(a.exp_avg, b.exp_avg) and _bits(a.exp_avg_sq, b.exp_avg_sq) and a.step_count == b.step_count == 5
    assert a.last_grad_norm() == b.last_grad_norm() > 0.5


def test_refusals_leave_every_buffer_alone(lib):
    n = 1000
    b = {k: Guarded(SC.dense_gradient(n, 1.0, s)) for s, k in enumerate("pgmv")}
    scratch = Guarded(np.full(2, 7.0, np.float32))
    d = _desc(SC.HYPERS["adam"])

    def apply(n=n, step=1, desc=C.byref(d), **null):
        a = {k: (None if k in null else x.ptr) for k, x in list(b.items()) + [("s", scratch)]}
        return lib.sf_adam_apply(a["p"], a["g"], a["m"], a["v"], n, desc, step, C.c_float(1.0), a["s"], _stream())

    assert apply(n=0) == INVALID and lib.sf_last_error()
    assert apply(n=-5) == INVALID
    assert apply(step=0) == INVALID and apply(step=-1) == INVALID
    for k in "pgmvs":
        assert apply(**{k: True}) == INVALID, k
    assert apply(desc=None) == INVALID
    h = C.c_void_p()
    assert lib.sf_opt_create(0, C.byref(d), C.byref(h)) == INVALID and not h.value
    assert lib.sf_opt_create(n, None, C.byref(h)) == INVALID and not h.value
    assert lib.sf_adam_step(None, b["p"].ptr, b["g"].ptr, C.c_float(1.0), None, _stream()) == INVALID
    torch.cuda.synchronize()
    assert all(x.untouched() for x in b.values()) and scratch.untouched()
    assert apply() == 0                                                     # and the same call with nothing wrong goes through
    torch.cuda.synchronize()
    assert not b["p"].untouched() and b["g"].untouched() and all(x.intact() for x in b.values())


# ---------------------------------------------------------------------------------------------------------------------------
# the fused epoch
# ---------------------------------------------------------------------------------------------------------------------------
def _tensors(i):
    T = torch.as_tensor(i.theta, dtype=torch.float32, device=DEV).contiguous()
    X = torch.as_tensor(i.x, dtype=torch.float32, device=DEV).contiguous()
    return T, X, torch.as_tensor(i.order, device=DEV)


@pytest.mark.parametrize("case", SC.EPOCH_CASES, ids=lambda c: f"{c.name}-{c.batch}")
def test_epoch_step_matches_the_fp64_model_on_its_own_gradient(case):
    from synference_amd.engine import HipFlow
    i = SC.epoch_inputs(case.name, case.batch)
    T, X, order = _tensors(i)
    B, n = case.batch, i.flat.size
    d = _desc(SC.EPOCH_DESC)
    f = HipFlow(i.spec, DEV)                                                # one handle through the three runs
    for step0, max_norm in SC.EPOCH_RUNS:
        label = f"{case.name}-{B} step0={step0} max_norm={max_norm}"
        m0, v0 = SC.epoch_warm_state(i.flat, step0)
        flat, m, v = Guarded(i.flat), Guarded(m0), Guarded(v0)
        grad, scratch = Guarded(np.full(n, np.nan, np.float32)), Guarded(np.zeros(2, np.float32))
        loss_sum = torch.full((), SC.LOSS_SUM_START, dtype=torch.float64, device=DEV)
        f.train_epoch(flat.t, T, X, order, 1, B, 1.0 / B, m.t, v.t, d, step0, max_norm, scratch.t, grad.t, loss_sum)
        torch.cuda.synchronize()
        assert all(x.intact() for x in (flat, m, v, grad, scratch)), "a sentinel changed"
        g_dev = grad.numpy()
        assert np.isfinite(g_dev).all()
        # (a) the gradient the call leaves is the gradient of loss_grad_rows on a fresh handle
        fresh = HipFlow(i.spec, DEV)
        g_rows, loss_rows = torch.empty(n, device=DEV), torch.empty(B, device=DEV)
        fresh.loss_grad_rows(torch.as_tensor(i.flat, device=DEV), T, X, order, 1.0 / B, g_rows, loss_out=loss_rows)
        torch.cuda.synchronize()
        gmax = float(g_rows.abs().max())
        diff = float((grad.t - g_rows).abs().max())
        print(f"STEP {label}: max |g| {gmax:.3e} epoch against loss_grad_rows {diff:.3e} ({case.family})")
        if SC.reproducible(case):
            assert _bits(grad.t, g_rows), (label, diff)
        else:
            assert diff <= SC.GRAD_NOISE * max(1.0, gmax), (label, diff, gmax)
        # (b) the norm from the gather's shares against the fp64 norm of that buffer
        norm = SM.check_norm(label, float(scratch.numpy()[1]), g_dev)
        if max_norm > 0:
            assert norm > 1.25 * max_norm, (label, norm, "the clip does not bite")
        # (c) parameters and moments against the model applied to the start state and the device's own gradient
        ref = SM.reference(i.flat, g_dev, m0, v0, step0 + 1, SC.EPOCH_DESC, max_norm)
        SM.check_step(label, flat.numpy(), m.numpy(), v.numpy(), ref)
        # (d) the loss sum against the float64 sum of the per-row losses
        want = float(loss_rows.double().sum().item())
        got = float(loss_sum.item()) - SC.LOSS_SUM_START
        print(f"STEP {label}: loss sum {got:.9g} rows {want:.9g} diff {abs(got - want):.2e} bar {B * SC.LOSS_PER_ROW:.2e}")
        assert abs(got - want) <= B * SC.LOSS_PER_ROW, (label, got, want)


def _three(i, split: bool, snapshot=None):
    """Three Adam steps of batch 64 from zero state: one call with n_batches = 3, or three calls with step0 advanced."""
    from synference_amd.engine import HipFlow
    T, X, order = _tensors(i)
    B, n = 64, i.flat.size
    d = _desc(SC.EPOCH_DESC)
    f = HipFlow(i.spec, DEV)
    flat = torch.as_tensor(i.flat, device=DEV).clone()
    m, v, grad = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.empty(n, device=DEV)
    scratch = torch.zeros(2, device=DEV)
    loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)
    if split:
        for b in range(3):
            if b == 2 and snapshot is not None:
                torch.cuda.synchronize()
                snapshot.update(flat=flat.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy())
            f.train_epoch(flat, T, X, order[b * B:(b + 1) * B], 1, B, 1.0 / B, m, v, d, b, 0.5, scratch, grad, loss_sum)
    else:
        f.train_epoch(flat, T, X, order, 3, B, 1.0 / B, m, v, d, 0, 0.5, scratch, grad, loss_sum)
    torch.cuda.synchronize()
    f.set_params(flat)
    lp = f.log_prob(T, X)
    torch.cuda.synchronize()
    return dict(flat=flat, m=m, v=v, grad=grad, norm=scratch[1:].clone(), loss=float(loss_sum.item()), lp=lp)


@pytest.mark.parametrize("name", SC.THREE_BATCH)
def test_three_batches_in_one_call_equal_three_calls(name):
    """prep_lite (only the training image re-tiled between the steps of a call) and the step numbering step0 + b + 1."""
    i = SC.epoch_inputs(name, 64, 3)
    one, three = _three(i, False), _three(i, True)
    for k in ("flat", "m", "v", "grad", "norm", "lp"):
        assert _bits(one[k], three[k]), (name, k, float((one[k] - three[k]).abs().max()))
    print(f"STEP {name}: loss sums {one['loss']:.9g} {three['loss']:.9g}")
    assert abs(one["loss"] - three["loss"]) <= 3 * 64 * SC.LOSS_PER_ROW
    assert float((one["flat"] - torch.as_tensor(i.flat, device=DEV)).abs().max()) > 1e-3     # three steps of lr 1e-3 were taken
    assert bool(torch.isfinite(one["lp"]).all())


def test_three_batches_in_one_call_equal_three_calls_lampe():
    """The lampe flows add their hidden deltas in LDS in the hardware's order: the gradient to the suite's lampe bar (2e-6 x max |g|),
    parameters and moments to the optimiser bar -- against the fp64 model of the third step, applied to the state the three-call run
    had before it and to that run's third gradient."""
    name = SC.THREE_BATCH_LAMPE
    i = SC.epoch_inputs(name, 64, 3)
    snap = {}
    one, three = _three(i, False), _three(i, True, snap)
    gmax = float(three["grad"].abs().max())
    diff = float((one["grad"] - three["grad"]).abs().max())
    print(f"STEP {name}: max |g| {gmax:.3e} one call against three {diff:.3e}")
    assert diff <= SC.LAMPE_NOISE * gmax
    ref = SM.reference(snap["flat"], three["grad"].cpu().numpy(), snap["m"], snap["v"], 3, SC.EPOCH_DESC, 0.5)
    for run, r in (("three calls", three), ("one call", one)):
        SM.check_step(f"{name} {run}", r["flat"].cpu().numpy(), r["m"].cpu().numpy(), r["v"].cpu().numpy(), ref)
    assert abs(float(one["norm"]) - float(three["norm"])) <= SM.NORM_TOL * float(three["norm"])
    assert abs(one["loss"] - three["loss"]) <= 3 * 64 * SC.LOSS_PER_ROW
