"""Conformance of the embedding MLP (k_mlp_fwd / k_mlp_bwd behind synference_amd.FCN, sf_mlp_forward, sf_mlp_backward): every
activation, tile edge and batch shape against tests/mlp_model.py in fp64 under the rule of tests/mlp_cases.py

    quantile_q(|kernel - ref64|) <= 4 * quantile_q(|ref32 - ref64|) + floor      for q in 0.5, 0.99, 1.0

with the floors of test_hip_fcn_forward_backward_match_torch (1e-4 of max(1, max |out|); per tensor 2e-4 of its own max |g|).
tests/test_cpu_mlp_cases.py holds on the reference alone that the bar is at most 1.1 floors, that the activation ranges are reached
and that a wrong derivative fails the rule.  Every comparison prints its ratios on an "MLP ..." line (run with -s); DESIGN.md
section 0b has the table measured on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import mlp_cases as MC
import mlp_model as MM
from oracle import flows as OF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _fcn(case):
    return MC.make_fcn(case).to(DEV)


class _Handle:
    """sf_mlp_* through the ABI: the only way to hand the kernel its standardisation constants."""

    def __init__(self, case, mean=None, std=None):
        from synference_amd import _lib
        self._lib, self.lib, self.case = _lib, _lib.load(), case
        keep = [None if a is None else np.ascontiguousarray(a.numpy(), dtype=np.float32) for a in (mean, std)]
        ptr = [None if a is None else a.ctypes.data_as(_lib.c_f32p) for a in keep]
        d = _lib.sf_mlp_desc(n_in=case.n_in, n_layers=len(case.widths),
                             widths=(C.c_int32 * 4)(*(list(case.widths) + [0] * 4)[:4]),
                             act={"silu": 0, "relu": 1, "tanh": 2}[case.act.lower()], x_mean=ptr[0], x_std=ptr[1])
        self.h = C.c_void_p()
        _lib.check(self.lib.sf_mlp_create(C.byref(d), C.byref(self.h)))   # (the constants are copied into the layout here)
        self.n = int(self.lib.sf_mlp_num_params(self.h))

    @staticmethod
    def _stream():
        return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def forward(self, flat, x):
        out = torch.full((x.shape[0], self.case.widths[-1]), float("nan"), device=DEV)
        self._lib.check(self.lib.sf_mlp_forward(self.h, C.c_void_p(flat.data_ptr()), C.c_void_p(x.data_ptr()), x.shape[0],
                                                C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def backward(self, flat, x, dout):
        grad = torch.full((self.n,), float("nan"), device=DEV)         # every element has to be written
        self._lib.check(self.lib.sf_mlp_backward(self.h, C.c_void_p(flat.data_ptr()), C.c_void_p(x.data_ptr()),
                                                 C.c_void_p(dout.data_ptr()), x.shape[0], C.c_void_p(grad.data_ptr()),
                                                 self._stream()))
        return grad

    def close(self):
        if self.h.value:
            self.lib.sf_mlp_destroy(self.h)
            self.h = C.c_void_p()


@pytest.fixture
def handles():
    made = []

    def make(case, mean=None, std=None):
        made.append(_Handle(case, mean, std))
        return made[-1]
    yield make
    torch.cuda.synchronize()
    for h in made:
        h.close()


def _cuda(*ts):
    return [t.to(DEV).contiguous() for t in ts]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. forward and backward of every case
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MC.ALL))
def test_forward_backward(name):
    b, ref = MC.build(name), MC.reference(name)
    m = _fcn(b.case)
    assert torch.equal(m.flat.detach().cpu(), b.flat)
    x, dout = _cuda(b.x, b.dout)
    out = m(x)
    (out * dout).sum().backward()
    assert out.shape == (b.case.B, b.case.widths[-1])
    assert torch.isfinite(out).all() and torch.isfinite(m.flat.grad).all()      # the saturated cases included
    MC.check_forward(name, out, ref)
    MC.check_grads(name, m.flat.grad, ref, b.case)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the forward is a function of the row alone
# ---------------------------------------------------------------------------------------------------------------------------
def test_forward_rows_do_not_depend_on_the_batch():
    """Every column of the MFMA accumulates on its own and in one order whatever the batch: bit for bit."""
    b = MC.build("B4099")
    m = _fcn(b.case)
    (x,) = _cuda(b.x)
    with torch.no_grad():
        full = m(x)
        assert torch.equal(m(x), full)
        assert torch.equal(m(x[:1]), full[:1])
        assert torch.equal(m(x[:33]), full[:33])
    MC.check_forward("B4099 rows", full, MC.reference("B4099"))


@pytest.mark.parametrize("B", [129, 4099])
@pytest.mark.parametrize("where", ["first", "last"])
def test_a_nan_row_stays_in_its_row(B, where):
    """Row 0, and the last row: the invalid lanes of the last wave read that row's data in its place."""
    b = MC.build("B4099")
    m = _fcn(b.case)
    (x,) = _cuda(b.x[:B])
    r = 0 if where == "first" else B - 1
    bad = x.clone()
    bad[r] = float("nan")
    with torch.no_grad():
        clean, got = m(x), m(bad)
    assert torch.isnan(got[r]).all()
    keep = torch.arange(B, device=DEV) != r
    assert torch.equal(got[keep], clean[keep])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. backward starts from zero
# ---------------------------------------------------------------------------------------------------------------------------
def test_backward_does_not_accumulate_and_the_stash_is_reused(handles):
    small, big = MC.build("B129"), MC.build("B4099")
    h = handles(small.case)
    (flat,) = _cuda(small.flat)
    xs, ds, xb, db = _cuda(small.x, small.dout, big.x, big.dout)
    first = h.backward(flat, xs, ds)
    second = h.backward(flat, xs, ds)
    MC.check_grads("B129 first backward", first, MC.reference("B129"), small.case)
    MC.check_grads("B129 second backward", second, MC.reference("B129"), small.case)       # not doubled
    MC.check_grads("B4099 after B129 (stash grows)", h.backward(flat, xb, db), MC.reference("B4099"), big.case)
    third = h.backward(flat, xs, ds)
    MC.check_grads("B129 after B4099 (stash reused)", third, MC.reference("B129"), small.case)
    # against each other, under the same per-tensor floors (the f32 atomics of five waves may arrive in any order)
    for label, g in (("second", second), ("third", third)):
        MC.check_grads(f"B129 {label} - first", g, MC.reference("B129"), small.case, other=first)


def test_two_handles_used_in_turn(handles):
    names = ("B129", "tanh_4l_wide")
    built = [MC.build(n) for n in names]
    hs = [handles(b.case) for b in built]
    dev = [_cuda(b.flat, b.x, b.dout) for b in built]
    alone = [h.backward(*d) for h, d in zip(hs, dev)]
    alone_out = [h.forward(d[0], d[1]) for h, d in zip(hs, dev)]
    for turn in range(2):
        for i in (0, 1):
            g = hs[i].backward(*dev[i])
            MC.check_grads(f"{names[i]} turn {turn}", g, MC.reference(names[i]), built[i].case)
            assert torch.equal(hs[i].forward(dev[i][0], dev[i][1]), alone_out[i])
    for i in (0, 1):
        MC.check_grads(f"{names[i]} alone", alone[i], MC.reference(names[i]), built[i].case)
        MC.check_forward(f"{names[i]} alone", alone_out[i], MC.reference(names[i]))


def test_one_wave_backward_is_bitwise_repeatable(handles):
    """B = 32 is one wave: every address of the gradient image receives one add."""
    b = MC.build("B32")
    h = handles(b.case)
    flat, x, dout = _cuda(b.flat, b.x, b.dout)
    g1 = h.backward(flat, x, dout)
    g2 = h.backward(flat, x, dout)
    assert torch.equal(g1, g2)
    MC.check_grads("B32 one wave", g1, MC.reference("B32"), b.case)


def test_empty_batch(handles):
    case = MC.ALL["B32"]
    m = _fcn(case)
    out = m(torch.empty(0, case.n_in, device=DEV))
    assert out.shape == (0, case.widths[-1])
    h = handles(case)
    (flat,) = _cuda(MC.build("B32").flat)
    g = h.backward(flat, torch.empty(0, case.n_in, device=DEV), torch.empty(0, case.widths[-1], device=DEV))
    assert torch.equal(g, torch.zeros_like(g))
    # ... also straight after a call that left a gradient in the image
    b = MC.build("B32")
    h.backward(*_cuda(b.flat, b.x, b.dout))
    g = h.backward(flat, torch.empty(0, case.n_in, device=DEV), torch.empty(0, case.widths[-1], device=DEV))
    assert torch.equal(g, torch.zeros_like(g))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. standardisation in the kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in", MC.STD_N_IN)
def test_standardisation_in_the_kernel(n_in, handles):
    b, ref = MC.build_std(n_in), MC.reference_std(n_in)
    flat, x, dout, mean, std = _cuda(b.flat, b.x, b.dout, b.mean, b.std)
    fused = handles(b.case, b.mean, b.std)
    MC.check_forward(f"std{n_in} fused", fused.forward(flat, x), ref)
    MC.check_grads(f"std{n_in} fused", fused.backward(flat, x, dout), ref, b.case)
    plain = handles(b.case)
    xs = ((x - mean) / std).contiguous()
    MC.check_forward(f"std{n_in} unfused", plain.forward(flat, xs), ref)
    MC.check_grads(f"std{n_in} unfused", plain.backward(flat, xs, dout), ref, b.case)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. HIP embedding in front of a HIP flow
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nsf", "maf"])
def test_hip_fcn_in_front_of_the_hip_flow_matches_the_fp64_twin(kind):
    """test_torch_embedding_net_trains_through_the_hip_flow with FCN([16, 6], "Tanh") as the embedding: losses, flow gradient and
    every embedding tensor's gradient against mlp_model in front of oracle.flows.log_prob, at that test's tolerances."""
    from synference_amd.embedding import FCN
    from synference_amd.estimator import build_flow
    rng = np.random.default_rng(0)
    B, D, Cx = 96, 4, 12
    theta = rng.normal(size=(B, D)).astype(np.float32)
    x = (rng.normal(size=(B, Cx)) * 3 + 1).astype(np.float32)
    emb = FCN([16, 6], "Tanh", generator=torch.Generator().manual_seed(0))
    est = build_flow(kind, theta, x, hidden_features=24, num_transforms=2, num_bins=6, embedding_net=emb, device=DEV,
                     generator=torch.Generator().manual_seed(1)).to("cuda")
    assert est.spec.C == 6 and est.has_embedding and est.embedding_net is emb and emb.n_input == Cx
    losses = est.loss(torch.as_tensor(theta).cuda(), torch.as_tensor(x).cuda())
    losses.mean().backward()
    s = est.spec
    ospec = OF.FlowSpec(kind=kind, D=D, C=6, H=24, T=2, K=6, perms=None if s.perms is None else np.asarray(s.perms),
                        theta_mean=s.theta_mean.astype(np.float64), theta_std=s.theta_std.astype(np.float64))
    p = est.flat.detach().cpu().double().requires_grad_(True)
    pe = emb.flat.detach().cpu().double().requires_grad_(True)
    xs = (torch.as_tensor(x).double() - est.x_mean_raw.cpu().double()) / est.x_std_raw.cpu().double()
    e64, hidden, _ = MM.forward(MM.tensors_of(pe, [16, 6], Cx), "Tanh", xs)
    assert hidden[0].abs().max() > 1.0                                  # the tanh is not in its linear range
    ref_loss = -OF.log_prob(ospec, p, torch.as_tensor(theta).double(), e64)
    ref_loss.mean().backward()
    e_loss = (losses.detach().cpu().double() - ref_loss.detach()).abs().max().item()
    g = est.flat.grad.cpu().double()
    e_flow = ((g - p.grad).abs().max() / p.grad.abs().max()).item()
    ge = emb.flat.grad.cpu().double()
    rows = []
    for name, shape, off in MM.layout([16, 6], Cx)[0]:
        k = int(np.prod(shape))
        r = pe.grad[off:off + k]
        rows.append((name, (ge[off:off + k] - r).abs().max().item(), max(r.abs().max().item(), 1e-9)))
    print(f"MLP joint {kind}: loss {e_loss:.2e} (bar 1e-4), flow gradient {e_flow:.2e} of max |g| (bar 2e-4), embedding "
          + ", ".join(f"{n} {e / m:.2e}" for n, e, m in rows) + " of the tensor's max |g| (bar 2e-4)")
    assert e_loss < 1e-4
    assert e_flow < 2e-4
    for n, e, m in rows:
        assert e < 2e-4 * m, n


def test_strided_input_and_leading_dimensions():
    """The module flattens leading dimensions and copies a strided view before the kernel reads it, in forward and in backward."""
    name = "nin33"
    b, ref = MC.build(name), MC.reference(name)
    x, dout = _cuda(b.x, b.dout)
    m = _fcn(b.case)
    with torch.no_grad():
        plain = m(x)
    wide = torch.zeros(b.case.B, 2 * b.case.n_in, device=DEV)
    wide[:, ::2] = x
    view = wide[:, ::2]
    assert not view.is_contiguous()
    out = m(view)
    assert torch.equal(out, plain)
    (out * dout).sum().backward()
    MC.check_grads(f"{name} strided input", m.flat.grad, ref, b.case)
    m.flat.grad = None
    out3 = m(x.reshape(7, 10, b.case.n_in))
    assert out3.shape == (7, 10, b.case.widths[-1]) and torch.equal(out3.reshape(70, -1), plain)
    (out3 * dout.reshape(7, 10, -1)).sum().backward()
    MC.check_grads(f"{name} leading dimensions", m.flat.grad, ref, b.case)
    with pytest.raises(ValueError, match="expected 33 input features, got 32"):
        m(x[:, :32])


# ---------------------------------------------------------------------------------------------------------------------------
# 6. a side stream
# ---------------------------------------------------------------------------------------------------------------------------
def test_side_stream():
    name = "edges_w"
    b, ref = MC.build(name), MC.reference(name)
    x, dout = _cuda(b.x, b.dout)
    m0 = _fcn(b.case)
    out0 = m0(x)
    (out0 * dout).sum().backward()
    torch.cuda.synchronize()
    m = _fcn(b.case)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = m(x)
        (out * dout).sum().backward()
    s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(out, out0)                                       # (the forward has no atomics)
    MC.check_forward(f"{name} side stream", out, ref)
    MC.check_grads(f"{name} side stream", m.flat.grad, ref, b.case)
    MC.check_grads(f"{name} default stream", m0.flat.grad, ref, b.case)
