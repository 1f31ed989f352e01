"""What a flow handle represents after every call that gives it a parameter vector.

A handle keeps up to ten derived images of one vector (density image, its transpose, the 16-row sampler image and its split-bf16 form, the
bf16 hidden blocks, the fused first layer, the compact fused image, the head-row table, the cooperative training image, the context table;
the one-parameter and lampe engines have copies of their own) and six flags that say which of them lag.  The rule under test:

    after a call that gives the handle the vector P, every consumer returns, bit for bit, what a fresh handle returns after
    set_params(P) on the same inputs in the same sampler mode

for the producers set_params, loss_grad (with and without dctx, and with B = 0), loss_grad_rows and train_epoch -- after which the images
are those of ``flat`` BEFORE the last update (include/synference_hip.h) -- and for a prepared context table, which every producer drops.
Bit equality is the expectation because both routes tile through sf_pack.h and the same fuse / compact kernels.

Every test prints what it compared ("STATE ..." lines; run with -s).  DESIGN.md section 0d lists the combinations measured on an MI355X."""
import dataclasses
import functools
import zlib

import numpy as np
import pytest
import torch

import step_cases as STEP
from cases import make_case
from synference_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_ROWS, N_EVAL, N_CTX, S, N_TRAIN_ROWS, N_ACC = 150, 70, 6, 64, 96, 512
MODES = (-1, 0, 1)
# (case, hidden_bf16)
FLOWS = [("maf_cfg1", False), ("maf_span6", False), ("maf_wide", False), ("maf_cfg1", True), ("nsf_cfg3", False), ("nsf_k16", False),
         ("nsf_d1", False), ("nsfar_small", False), ("mafar_small", False)]
OWN_ENGINE = ("nsf_d1", "nsfar_small", "mafar_small")      # no context table, no sample_round, no dctx
_flow_id = lambda fl: fl[0] + ("-bf16" if fl[1] else "")
flows = pytest.mark.parametrize("flow", FLOWS, ids=_flow_id)


@pytest.fixture
def sampler_mode():
    """sf_set_sampler_fp32 for one test; the per-kind default afterwards."""
    lib = _lib.load()
    yield lib.sf_set_sampler_fp32
    lib.sf_set_sampler_fp32(-1)


Inputs = dataclasses.make_dataclass("Inputs", "spec P0 P1 theta x z rows order".split())


@functools.lru_cache(maxsize=None)
def _inputs(flow):
    name, bf16 = flow
    _, spec, flat, theta, x = make_case(name, B=N_ROWS, spread=0.2)
    if bf16:
        spec = dataclasses.replace(spec, hidden_bf16=True)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    P1 = (flat + 0.02 * np.abs(flat).mean() * rng.normal(size=flat.shape)).astype(np.float32)
    z = rng.normal(size=(N_EVAL, spec.D)).astype(np.float32)
    rows = rng.integers(0, N_ROWS, size=N_TRAIN_ROWS).astype(np.int64)
    order = rng.integers(0, N_ROWS, size=3 * N_TRAIN_ROWS).astype(np.int64)
    for a in (flat, P1, theta, x, z, rows, order):
        a.setflags(write=False)
    return Inputs(spec, flat, P1, theta, x, z, rows, order)


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a), dtype=dtype, device=DEV).contiguous()


def _new(flow, P=None):
    from synference_amd.engine import HipFlow
    f = HipFlow(_inputs(flow).spec, DEV)
    if P is not None:
        f.set_params(_t(P))
    return f


@functools.lru_cache(maxsize=None)
def _box(flow):
    """The 3 % / 97 % quantiles of free draws at P0 (as in tests/test_gpu_parity.py): the box rejects a good share of the draws."""
    i = _inputs(flow)
    free = _new(flow, i.P0).sample(_t(i.x[:N_CTX]), 400, seed=99).reshape(-1, i.spec.D).cpu().numpy()
    free = free[np.isfinite(free).all(-1)]
    return np.quantile(free, 0.03, axis=0).astype(np.float32), np.quantile(free, 0.97, axis=0).astype(np.float32)


def _consumers(f, flow, set_mode, modes=MODES):
    """Every consumer of the handle's images on fixed inputs -> {name: cpu tensor}."""
    i = _inputs(flow)
    lo, hi = _box(flow)
    T, X, Z, X6 = _t(i.theta[:N_EVAL]), _t(i.x[:N_EVAL]), _t(i.z), _t(i.x[:N_CTX])
    slots = torch.arange(0, N_CTX * S, 3, dtype=torch.int32, device=DEV)
    out = {"log_prob": f.log_prob(T, X)}
    out["inverse theta"], out["inverse logdet"] = f.inverse(Z, X)
    try:
        for mode in modes:
            set_mode(mode)
            out[f"inverse_sampler[{mode}]"], _ = f.inverse_sampler(Z, X)
            out[f"inverse_sampler rc[{mode}]"] = torch.tensor([f.last_sampler_rc])
            out[f"sample[{mode}]"], out[f"n_drawn[{mode}]"] = f.sample(X6, S, lo, hi, seed=2025, return_counts=True)
            part = torch.full((N_CTX, S, i.spec.D), float("nan"), device=DEV)
            out[f"sample_slots unfilled[{mode}]"] = torch.tensor([f.sample_slots(X6, S, slots, part, lo, hi, seed=2025)])
            out[f"sample_slots[{mode}]"] = part
            out[f"acceptance[{mode}]"] = f.acceptance(X6, N_ACC, lo, hi, seed=11)
    finally:
        set_mode(-1)
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def _same(a, b) -> bool:
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


_FRESH = {}


def _fresh(flow, P, set_mode, modes=MODES):
    """The consumers of a fresh handle after set_params(P), once per (flow, vector, modes)."""
    key = (flow, modes, zlib.crc32(np.ascontiguousarray(P).tobytes()), len(P))
    if key not in _FRESH:
        _FRESH[key] = _consumers(_new(flow, P), flow, set_mode, modes)
    return _FRESH[key]


def _compare(label, got, want):
    assert set(got) == set(want)
    bad = []
    for k in want:
        if not _same(got[k], want[k]):
            a, b = got[k].double(), want[k].double()
            d = float((a - b).abs().nan_to_num(nan=0.0, posinf=float("inf")).max()) if a.shape == b.shape else float("nan")
            bad.append(f"{k} (max |diff| {d:.3e}, {int((a != b).sum()) if a.shape == b.shape else -1} elements)")
    finite = all(bool(torch.isfinite(want[k]).all()) for k in ("log_prob", "inverse theta") if k in want)
    print(f"STATE {label}: {len(want) - len(bad)} of {len(want)} consumers bit-equal to a fresh handle" + (": DIFFER " + "; ".join(bad) if bad else ""))
    assert finite, (label, "the fresh handle's own outputs are not finite")
    assert not bad, (label, bad)


def _check(label, f, flow, P, set_mode):
    _compare(label, _consumers(f, flow, set_mode), _fresh(flow, P, set_mode))


def _vectors_differ(flow, set_mode):
    """The perturbation is visible to every float consumer: a handle that kept P0 cannot pass for P1."""
    i = _inputs(flow)
    a, b = _fresh(flow, i.P0, set_mode), _fresh(flow, i.P1, set_mode)
    for k in ("log_prob", "inverse theta", "sample[-1]", "sample[0]", "sample[1]", "inverse_sampler[-1]"):
        assert not _same(a[k], b[k]), (flow, k, "P0 and P1 give the same bits")


def _holds_no_vector(f, flow):
    """After a training call the caller's vector is the master copy: get_params and log_prob_grad say so."""
    i = _inputs(flow)
    with pytest.raises(RuntimeError, match="no parameters held by the handle"):
        f.get_params()
    if f.supports_log_prob_grad():
        with pytest.raises(RuntimeError, match="no parameters held by the handle"):
            f.log_prob_grad(_t(i.theta[:8]), _t(i.x[:8]))


def _holds(f, flow, P):
    """After set_params(P) the handle holds P, and log_prob_grad (where the kind has it) is a fresh handle's to the bit."""
    i = _inputs(flow)
    assert np.array_equal(f.get_params().cpu().numpy(), np.asarray(P))
    if f.supports_log_prob_grad():
        T, X = _t(i.theta[:N_EVAL]), _t(i.x[:N_EVAL])
        lp, g = f.log_prob_grad(T, X)
        wlp, wg = _new(flow, P).log_prob_grad(T, X)
        assert bool(torch.isfinite(wlp).all() and torch.isfinite(wg).all())
        _compare(f"{_flow_id(flow)} log_prob_grad after set_params", {"lp": lp.cpu(), "dtheta": g.cpu()}, {"lp": wlp.cpu(), "dtheta": wg.cpu()})


def _at_p0(flow, set_mode):
    """A handle at P0 whose every image, lazily built ones included, has been used."""
    i = _inputs(flow)
    f = _new(flow, i.P0)
    _check(f"{_flow_id(flow)} set_params(P0)", f, flow, i.P0, set_mode)
    return f


# ---------------------------------------------------------------------------------------------------------------------------
# the producers
# ---------------------------------------------------------------------------------------------------------------------------
@flows
def test_set_params_then_set_params(flow, sampler_mode):
    i = _inputs(flow)
    _vectors_differ(flow, sampler_mode)
    f = _at_p0(flow, sampler_mode)
    _holds(f, flow, i.P0)
    f.set_params(_t(i.P1))
    _check(f"{_flow_id(flow)} set_params(P0), set_params(P1)", f, flow, i.P1, sampler_mode)
    _holds(f, flow, i.P1)


@flows
def test_loss_grad(flow, sampler_mode):
    i = _inputs(flow)
    T, X = _t(i.theta[:N_TRAIN_ROWS]), _t(i.x[:N_TRAIN_ROWS])
    f = _at_p0(flow, sampler_mode)
    variants = [False]
    if flow[0] not in OWN_ENGINE and f.train_path(N_TRAIN_ROWS, True) != f.train_path(N_TRAIN_ROWS, False):
        variants.append(True)
    for want_dctx in variants:
        f.set_params(_t(i.P0))
        dctx = torch.empty(N_TRAIN_ROWS, i.spec.C, device=DEV) if want_dctx else None
        loss, grad = f.loss_grad(_t(i.P1), T, X, 1.0 / N_TRAIN_ROWS, dctx_out=dctx)
        assert bool(torch.isfinite(loss).all() and torch.isfinite(grad).all()) and bool(grad.any())
        label = f"{_flow_id(flow)} set_params(P0), loss_grad(P1{', dctx' if want_dctx else ''}) path {f.train_path(N_TRAIN_ROWS, want_dctx)}"
        _check(label, f, flow, i.P1, sampler_mode)
        _holds_no_vector(f, flow)
    f.set_params(_t(i.P0))
    _holds(f, flow, i.P0)
    _check(f"{_flow_id(flow)} loss_grad(P1), set_params(P0)", f, flow, i.P0, sampler_mode)


@flows
def test_loss_grad_of_an_empty_batch(flow, sampler_mode):
    """B = 0: the images are those of P1 and the gradient is exactly zero."""
    i = _inputs(flow)
    f = _at_p0(flow, sampler_mode)
    grad = torch.full((i.P1.size,), float("nan"), device=DEV)
    loss, _ = f.loss_grad(_t(i.P1), torch.empty(0, i.spec.D, device=DEV), torch.empty(0, i.spec.C, device=DEV), 1.0, grad_out=grad)
    torch.cuda.synchronize()
    assert loss.numel() == 0 and not bool(grad.any()) and bool(torch.isfinite(grad).all())
    _check(f"{_flow_id(flow)} set_params(P0), loss_grad(P1, B = 0)", f, flow, i.P1, sampler_mode)
    _holds_no_vector(f, flow)


@flows
def test_loss_grad_rows(flow, sampler_mode):
    i = _inputs(flow)
    f = _at_p0(flow, sampler_mode)
    grad = torch.full((i.P1.size,), float("nan"), device=DEV)
    f.loss_grad_rows(_t(i.P1), _t(i.theta), _t(i.x), _t(i.rows, torch.int64), 1.0 / N_TRAIN_ROWS, grad)
    assert bool(torch.isfinite(grad).all()) and bool(grad.any())
    _check(f"{_flow_id(flow)} set_params(P0), loss_grad_rows(P1)", f, flow, i.P1, sampler_mode)
    _holds_no_vector(f, flow)


def _epoch(f, flow, start, n_batches):
    """sf_flow_train_epoch from zero optimiser state over the first n_batches x 96 rows of the order -> flat afterwards (numpy)."""
    i = _inputs(flow)
    n = i.P0.size
    d = _lib.sf_adam_desc(1e-3, 0.9, 0.999, 1e-8, 0.0, 0)
    flat = _t(start).clone()
    m, v, grad, scratch = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.empty(n, device=DEV), torch.zeros(2, device=DEV)
    loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)
    f.train_epoch(flat, _t(i.theta), _t(i.x), _t(i.order, torch.int64), n_batches, N_TRAIN_ROWS, 1.0 / N_TRAIN_ROWS, m, v, d, 0, 0.5,
                  scratch, grad, loss_sum)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss_sum.item())) and bool(torch.isfinite(flat).all())
    return flat.cpu().numpy()


# three batches on the reproducible families only: the gradients of the lampe flows repeat to rounding, so Q cannot be rebuilt to the bit
_EPOCHS = [(fl, 1) for fl in FLOWS] + [(fl, 3) for fl in FLOWS if STEP.reproducible(STEP.EpochCase(fl[0], N_TRAIN_ROWS, ""))]


@pytest.mark.parametrize("flow,n_batches", _EPOCHS, ids=[f"{_flow_id(fl)}-n{n}" for fl, n in _EPOCHS])
def test_train_epoch(flow, n_batches, sampler_mode):
    """After sf_flow_train_epoch the images are those of Q, the value of ``flat`` when the last step's gradient was taken: the start
    vector for one batch; for three, what a twin handle and a twin optimiser state hold after a two-batch call on the same order (the
    lampe flows run one batch only: their gradients repeat to rounding, not to the bit)."""
    i = _inputs(flow)
    f = _at_p0(flow, sampler_mode)
    after = _epoch(f, flow, i.P1, n_batches)
    Q = np.array(i.P1) if n_batches == 1 else _epoch(_new(flow), flow, i.P1, n_batches - 1)
    step = np.abs(after - Q).max()
    print(f"STATE {_flow_id(flow)} train_epoch n = {n_batches}: max |flat - Q| {step:.3e} (lr 1e-3)")
    assert 1e-4 < step < 5e-3, "the last update moved flat by about one learning rate"
    _check(f"{_flow_id(flow)} set_params(P0), train_epoch(P1, n = {n_batches}): images of flat before the last update", f, flow, Q, sampler_mode)
    _holds_no_vector(f, flow)
    # ... and not those of flat as it is returned
    got, ret = _consumers(f, flow, sampler_mode, (-1,)), _fresh(flow, after, sampler_mode, (-1,))
    assert not _same(got["log_prob"], ret["log_prob"])
    f.set_params(_t(after))
    _compare(f"{_flow_id(flow)} train_epoch(n = {n_batches}), set_params(flat)", _consumers(f, flow, sampler_mode, (-1,)), ret)


# ---------------------------------------------------------------------------------------------------------------------------
# the context table
# ---------------------------------------------------------------------------------------------------------------------------
def _table_consumers(f, flow, X):
    """inverse_sampler and one dense sample_round over the tensor X itself (the pointer a prepared table is keyed by)."""
    i = _inputs(flow)
    lo, hi = (_t(a) for a in _box(flow))
    n = N_CTX * S
    out = torch.full((N_CTX, S, i.spec.D), float("nan"), device=DEV)
    rej, cnt = torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    f.sample_round(X, S, None, 0, n, 0, 31, lo, hi, out, rej, cnt)      # first: the hook below may prepare a table of its own
    th, _ = f.inverse_sampler(_t(i.z[:N_CTX]), X)
    torch.cuda.synchronize()
    k = int(cnt.item())
    assert 0 < k < n
    return {"inverse_sampler": th.cpu(), "round draws": out.cpu(), "round rejected": torch.sort(rej[:k]).values.cpu(),
            "log_prob": f.log_prob(_t(i.theta[:N_CTX]), X).cpu(), "inverse theta": f.inverse(_t(i.z[:N_CTX]), X)[0].cpu()}


@pytest.mark.parametrize("flow", [fl for fl in FLOWS if fl[0] not in OWN_ENGINE], ids=_flow_id)
@pytest.mark.parametrize("producer", ["loss_grad", "set_params"])
def test_a_prepared_context_table_is_dropped(flow, producer):
    i = _inputs(flow)
    X = _t(i.x[:N_CTX])
    want = _table_consumers(_new(flow, i.P1), flow, _t(i.x[:N_CTX]))
    stale = _table_consumers(_new(flow, i.P0), flow, _t(i.x[:N_CTX]))
    assert not _same(want["round draws"], stale["round draws"]) and not _same(want["inverse_sampler"], stale["inverse_sampler"])
    f = _new(flow, i.P0)
    f.prepare_context(X)
    if producer == "loss_grad":
        f.loss_grad(_t(i.P1), _t(i.theta[:N_TRAIN_ROWS]), _t(i.x[:N_TRAIN_ROWS]), 1.0 / N_TRAIN_ROWS)
    else:
        f.set_params(_t(i.P1))
    _compare(f"{_flow_id(flow)} prepare_context(X), {producer}(P1): the table of P0 is not read", _table_consumers(f, flow, X), want)


@flows
def test_sample_reads_the_context_rows_of_this_call(flow):
    """sample(X), X changed in place (same pointer), sample(X) again: the second call draws for the new rows."""
    i = _inputs(flow)
    lo, hi = _box(flow)
    X, X2 = _t(i.x[:N_CTX]), _t(i.x[N_CTX:2 * N_CTX])
    f = _new(flow, i.P0)
    first = f.sample(X, S, lo, hi, seed=7).cpu()
    ptr = X.data_ptr()
    X.copy_(X2)
    assert X.data_ptr() == ptr
    second, nd = f.sample(X, S, lo, hi, seed=7, return_counts=True)
    want, wnd = _new(flow, i.P0).sample(X2, S, lo, hi, seed=7, return_counts=True)
    got = {"sample": second.cpu(), "n_drawn": nd.cpu()}
    ref = {"sample": want.cpu(), "n_drawn": wnd.cpu()}
    assert not _same(first, got["sample"])
    _compare(f"{_flow_id(flow)} sample(X), X.copy_(X2), sample(X)", got, ref)


# ---------------------------------------------------------------------------------------------------------------------------
# the sampler modes
# ---------------------------------------------------------------------------------------------------------------------------
@flows
def test_mode_sequence_on_one_handle(flow, sampler_mode):
    """Modes 1 -> 0 -> -1 on one handle: each equals a fresh handle that has seen that mode only."""
    i = _inputs(flow)
    f = _new(flow, i.P0)
    for mode in (1, 0, -1):
        got = _consumers(f, flow, sampler_mode, (mode,))
        want = _consumers(_new(flow, i.P0), flow, sampler_mode, (mode,))
        _compare(f"{_flow_id(flow)} mode {mode} in the sequence 1, 0, -1 on one handle", got, want)
