"""What keeps tests/test_gpu_mlp.py from passing vacuously, checked on the reference alone (no GPU).

* the fp32 reference is so close to the fp64 one that the bar 4 x e_ref + floor is never wider than 1.1 floors;
* the inputs really reach the activation ranges the cases are named for, and no ReLU unit sits on its kink;
* a wrong activation derivative and a standardisation without its divide, planted in the reference's own functions, fail the rule;
* the hand-written backward of the reference is autograd's;
* the host-side refusals of sf_mlp_create and of FCN.__init__.

The tests print what they measure (run with -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mlp_cases as MC
import mlp_model as MM


def _hidden(name):
    return torch.cat([z.reshape(-1) for z in MC.reference(name)["f64"].z]).numpy()


@pytest.mark.parametrize("name", list(MC.ALL))
def test_fp32_reference_is_a_tenth_of_the_floor(name):
    """4 * max |ref32 - ref64| <= floor / 10 for the output and for every gradient tensor."""
    _check_reference_accuracy(name, MC.ALL[name], MC.reference(name))


@pytest.mark.parametrize("n_in", MC.STD_N_IN)
def test_fp32_reference_is_a_tenth_of_the_floor_standardised(n_in):
    _check_reference_accuracy(f"std{n_in}", MC.build_std(n_in).case, MC.reference_std(n_in))


def _check_reference_accuracy(name, case, ref):
    o64, o32 = ref["f64"].out.numpy(), ref["f32"].out.double().numpy()
    assert np.isfinite(o64).all() and np.isfinite(o32).all()
    worst = 4 * np.abs(o32 - o64).max() / MC.fwd_floor(o64)
    lay, _ = MM.layout(case.widths, case.n_in)
    for (tensor, _, _), g64, g32 in zip(lay, ref["f64"].grads, ref["f32"].grads):
        g64, g32 = g64.numpy(), g32.double().numpy()
        assert np.isfinite(g64).all() and np.isfinite(g32).all(), tensor
        assert np.abs(g64).max() > 1e-9, tensor                       # the 1e-9 guard of the floor is never what holds
        r = 4 * np.abs(g32 - g64).max() / (MC.GRAD_FLOOR * np.abs(g64).max())
        assert r <= 0.1, (name, tensor, r)
        worst = max(worst, r)
    print(f"{name}: 4 x e_ref / floor at most {worst:.3f}; max |out| {np.abs(o64).max():.3g}")
    assert worst <= 0.1, (name, worst)


def test_tanh_2l_reaches_the_curved_and_the_linear_range():
    z = np.abs(_hidden("tanh_2l"))
    print(f"tanh_2l: |z| > 3 {np.mean(z > 3):.4f}, |z| < 0.5 {np.mean(z < 0.5):.4f}")
    assert np.mean(z > 3) >= 0.005 and np.mean(z < 0.5) >= 0.10


@pytest.mark.parametrize("name", MC.SATURATED)
def test_saturated_cases_reach_past_the_exp2_range(name):
    """Beyond |z| = 44 the kernel's tanh has overflowed / flushed its exp2, beyond z = -88 its sigmoid has."""
    z = _hidden(name)
    print(f"{name}: |z| > 20 {np.mean(np.abs(z) > 20):.4f}, z > 88 {np.mean(z > 88):.4f}, z < -88 {np.mean(z < -88):.4f}, "
          f"z < -2 {np.mean(z < -2):.4f}")
    assert np.mean(np.abs(z) > 20) >= 0.20
    assert (z > 88).any() and (z < -88).any()
    if name == "sat_silu":
        assert np.mean(z < -2) >= 0.20
    ref = MC.reference(name)
    assert all(torch.isfinite(g).all() for k in ref for g in ref[k].grads) and all(torch.isfinite(ref[k].out).all() for k in ref)


@pytest.mark.parametrize("name", MC.RELU)
def test_relu_cases_stay_off_the_kink(name):
    b = MC.build(name)
    z = _hidden(name)
    neg = np.mean(z < 0)
    print(f"{name}: {b.redrawn} of {b.case.B} rows redrawn in {b.passes} pass(es); negative share {neg:.3f}, min |z| {np.abs(z).min():.2e}")
    assert 0.3 <= neg <= 0.7
    assert np.abs(z).min() >= MC.KINK
    assert b.redrawn <= 0.10 * b.case.B


def test_every_case_is_deterministic_and_of_the_stated_shape():
    for name, c in MC.ALL.items():
        b = MC.build(name)
        assert b.x.shape == (c.B, c.n_in) and b.dout.shape == (c.B, c.widths[-1]) and b.x.dtype == torch.float32
        assert b.flat.numel() == MM.layout(c.widths, c.n_in)[1]
    first = MC.build.__wrapped__("edges_w")
    again = MC.build.__wrapped__("edges_w")
    assert torch.equal(first.x, again.x) and torch.equal(first.flat, again.flat) and torch.equal(first.dout, again.dout)
    # the batch family is one net
    assert torch.equal(MC.build("B1").flat, MC.build("B4099").flat)


@pytest.mark.parametrize("name", ["tanh_2l", "silu_widen", "edges_w", "w1"])
def test_hand_written_backward_is_autograd(name):
    b = MC.build(name)
    c = b.case
    got = MM.flat_grad(MC.reference(name)["f64"])
    p = b.flat.double().requires_grad_(True)
    out, _, _ = MM.forward(MM.tensors_of(p, c.widths, c.n_in), c.act, b.x.double())
    (out * b.dout.double()).sum().backward()
    assert np.abs(got - p.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(got).max())
    # and the module form the existing device test uses
    mods, n_prev = [], c.n_in
    T = MM.tensors_of(b.flat.double(), c.widths, c.n_in)
    for l, w in enumerate(c.widths):
        lin = torch.nn.Linear(n_prev, w).double()
        lin.weight.data.copy_(T[f"layers.{l}.weight"]); lin.bias.data.copy_(T[f"layers.{l}.bias"])
        mods.append(lin)
        if l + 1 < len(c.widths):
            mods.append({"SiLU": torch.nn.SiLU(), "ReLU": torch.nn.ReLU(), "Tanh": torch.nn.Tanh()}[c.act])
        n_prev = w
    with torch.no_grad():
        assert (torch.nn.Sequential(*mods)(b.x.double()) - MC.reference(name)["f64"].out).abs().max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------------
# planted defects: the rule fails when the function under comparison is wrong (the fp64 reference with one function replaced
# stands in for the kernel)
# ---------------------------------------------------------------------------------------------------------------------------
def _defective(name, monkeypatch, table, key, fn):
    b = MC.build(name)
    monkeypatch.setitem(table, key, fn)
    try:
        return MM.run_flat(b.flat, b.case.widths, b.case.act, b.case.n_in, b.x, b.dout)
    finally:
        monkeypatch.undo()


@pytest.mark.parametrize("name,act,wrong", [("tanh_2l", "tanh", lambda z: torch.ones_like(z)),
                                            ("silu_widen", "silu", torch.sigmoid),
                                            # one percent of the curvature term: what the device's negative check used
                                            ("tanh_2l", "tanh", lambda z: 1 - 0.99 * torch.tanh(z) ** 2)],
                         ids=["tanh_d_is_1", "silu_d_is_sigmoid", "tanh_d_off_by_a_percent"])
def test_a_wrong_activation_derivative_fails_the_gradient_check(name, act, wrong, monkeypatch):
    ref, case = MC.reference(name), MC.ALL[name]
    MC.check_grads(f"{name} fp32 reference", MM.flat_grad(ref["f32"]), ref, case)              # the rule passes what is right
    bad = _defective(name, monkeypatch, MM.ACT_D, act, wrong)
    MC.check_forward(f"{name} planted d{act}", bad.out, ref)                                   # (the forward is untouched)
    with pytest.raises(AssertionError):
        MC.check_grads(f"{name} planted d{act}", MM.flat_grad(bad), ref, case)
    # the last layer sees no activation derivative: the defect has to be caught on an earlier tensor
    lay, _ = MM.layout(case.widths, case.n_in)
    L = len(case.widths)
    with pytest.raises(AssertionError):
        off, k = lay[0][2], int(np.prod(lay[0][1]))
        g64 = ref["f64"].grads[0].numpy().reshape(-1)
        MC.check(f"{name} planted d{act}, first weight", MM.flat_grad(bad)[off:off + k] - g64,
                 ref["f32"].grads[0].double().numpy().reshape(-1) - g64, MC.GRAD_FLOOR * np.abs(g64).max())
    assert torch.equal(bad.grads[2 * L - 1], ref["f64"].grads[2 * L - 1])


@pytest.mark.parametrize("n_in", MC.STD_N_IN)
def test_a_standardisation_without_its_divide_fails_the_forward_check(n_in, monkeypatch):
    b, ref = MC.build_std(n_in), MC.reference_std(n_in)
    MC.check_forward(f"std{n_in} fp32 reference", ref["f32"].out, ref)
    monkeypatch.setattr(MM, "standardise", lambda x, mean=None, std=None: x - mean)
    bad = MM.run_flat(b.flat, b.case.widths, b.case.act, n_in, b.x, b.dout, b.mean, b.std)
    monkeypatch.undo()
    with pytest.raises(AssertionError):
        MC.check_forward(f"std{n_in} planted no divide", bad.out, ref)
    # and the constants matter at all: the reference without them is far from the reference with them
    plain = MM.run_flat(b.flat, b.case.widths, b.case.act, n_in, b.x, b.dout)
    with pytest.raises(AssertionError):
        MC.check_forward(f"std{n_in} no constants", plain.out, ref)


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: sf_mlp_create only builds the layout, no device is needed
# ---------------------------------------------------------------------------------------------------------------------------
def _create(lib, n_in, widths, act=0):
    from synference_amd import _lib
    d = _lib.sf_mlp_desc(n_in=n_in, n_layers=len(widths), widths=(C.c_int32 * 4)(*(list(widths) + [0] * 4)[:4]), act=act,
                         x_mean=None, x_std=None)
    h = C.c_void_p()
    return lib.sf_mlp_create(C.byref(d), C.byref(h)), h


@pytest.mark.parametrize("n_in,widths,act,message", [
    (0, [8, 2], 0, b"n_in must be in 1..512"),
    (513, [8, 2], 0, b"n_in must be in 1..512"),
    (4, [], 0, b"n_layers must be in 1..4"),
    (4, [8, 0, 2], 0, b"layer widths must be in 1..128"),
    (4, [8, 129], 0, b"layer widths must be in 1..128"),
    (4, [8, 2], 3, b"unknown activation"),
    (4, [8, 2], -1, b"unknown activation"),
])
def test_sf_mlp_create_refuses_with_a_message(lib, n_in, widths, act, message):
    rc, h = _create(lib, n_in, widths, act)
    assert rc == -1 and not h.value                    # SF_ERR_INVALID
    assert lib.sf_last_error() == message, lib.sf_last_error()


def test_sf_mlp_create_refuses_five_layers(lib):
    from synference_amd import _lib
    d = _lib.sf_mlp_desc(n_in=4, n_layers=5, widths=(C.c_int32 * 4)(8, 8, 8, 2), act=0, x_mean=None, x_std=None)
    h = C.c_void_p()
    assert lib.sf_mlp_create(C.byref(d), C.byref(h)) == -1 and not h.value
    assert lib.sf_last_error() == b"n_layers must be in 1..4"
    assert lib.sf_mlp_create(None, C.byref(h)) == -1 and lib.sf_last_error() == b"null argument"


@pytest.mark.parametrize("n_in,widths", [(1, [1]), (512, [128, 128, 128, 128]), (37, [33, 65, 5])])
def test_sf_mlp_num_params_is_the_layout_count(lib, n_in, widths):
    rc, h = _create(lib, n_in, widths)
    assert rc == 0 and h.value
    try:
        assert lib.sf_mlp_num_params(h) == MM.layout(widths, n_in)[1]
        m = MC.make_fcn(MC.Case(tuple(widths), "SiLU", n_in, 1, 1.0))
        assert m.layout()[1] == m.flat.numel() == MM.layout(widths, n_in)[1]
        assert [(n, tuple(s), o) for n, s, o in m.layout()[0]] == MM.layout(widths, n_in)[0]
    finally:
        lib.sf_mlp_destroy(h)
    assert lib.sf_mlp_num_params(None) == 0


def test_fcn_constructor_refusals():
    from synference_amd.embedding import FCN
    with pytest.raises(ValueError, match="act_fn 'GELU' is not built on the HIP path; supported: SiLU, ReLU, Tanh"):
        FCN([8, 2], "GELU")
    with pytest.raises(ValueError, match=r"the HIP FCN supports 1\.\.4 layers of width <= 128"):
        FCN([8, 8, 8, 8, 2])
    with pytest.raises(ValueError, match=r"the HIP FCN supports 1\.\.4 layers of width <= 128"):
        FCN([129, 2])
    FCN([128, 128, 128, 128], "tanh")                   # the limits themselves are accepted, the activation in any case


def test_fcn_on_the_cpu_refuses_forward_by_name():
    m = MC.make_fcn(MC.ALL["tanh_2l"])
    with pytest.raises(RuntimeError, match="FCN parameters live on the CPU"):
        m(torch.zeros(3, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        with torch.no_grad():
            m(torch.zeros(3, 5))
