"""Cases and comparison rule of the embedding-MLP conformance tests (tests/test_gpu_mlp.py, tests/test_cpu_mlp_cases.py).

Helper module, no tests in it.  A case is (widths, activation, n_in, B, input scale): weights by torch's nn.Linear default
initialisation from a seeded generator (``FCN.initialize`` itself draws them, so the device module and the reference hold the same
numbers), inputs = seeded normal draws x scale, ``dout`` = seeded normal draws.

ReLU's kink: a hidden pre-activation within rounding of zero can fall on different sides in the kernel and in the fp64 reference,
which are then right about different functions.  For the ReLU cases every row whose fp64 hidden pre-activation has |z| < 1e-4 in any
unit is redrawn from the same generator until none is left -- decided on the reference alone.

The one rule of every comparison is sharp_cases.check_bar, unchanged:

    quantile_q(|kernel - ref64|) <= 4 * quantile_q(|ref32 - ref64|) + floor      for q in 0.5, 0.99, 1.0

with the floors test_hip_fcn_forward_backward_match_torch already asserts: 1e-4 * max(1, max |out64|) on the output and, per tensor,
2e-4 * max(max |g64 of that tensor|, 1e-9) on the gradient."""
from __future__ import annotations

import contextlib
import functools
import io
from collections import namedtuple

import numpy as np
import torch

import mlp_model as MM
import sharp_cases as SC

FWD_FLOOR = 1e-4              # of max(1, max |out64|)
GRAD_FLOOR = SC.GRAD_FLOOR    # 2e-4 of max(max |g64 of the tensor|, 1e-9)
KINK = 1e-4                   # ReLU rows with a hidden |z| below this are redrawn
WEIGHT_SEED = 0

Case = namedtuple("Case", "widths act n_in B scale")

CASES = {
    "tanh_2l": Case((24, 8), "Tanh", 5, 75, 2.0),                        # Tanh forward and derivative at all
    "tanh_4l_wide": Case((128, 128, 128, 16), "Tanh", 33, 200, 2.0),     # HT = 4, four layers, three stash levels
    "silu_widen": Case((8, 40, 128), "SiLU", 3, 130, 2.0),               # widening net, HT from the last layer
    "relu_out1": Case((64, 1), "ReLU", 9, 129, 2.0),                     # n_out = 1, one row in the fifth wave
    "in1": Case((16, 4), "SiLU", 1, 33, 2.0),                            # one input feature
    "w1": Case((1, 3), "SiLU", 4, 40, 2.0),                              # a hidden layer of one unit
    "edges_w": Case((33, 65, 97, 5), "ReLU", 20, 96, 2.0),               # every width one past a tile edge
    "relu4": Case((100, 64, 32, 12), "ReLU", 70, 513, 2.0),              # four-layer ReLU over five workgroups
    "in200": Case((64, 16), "SiLU", 200, 257, 2.0),                      # the spectra route's size
    "in512": Case((128, 64, 16), "SiLU", 512, 300, 2.0),                 # the packer's limit, 16 input tiles
    "sat_tanh": Case((32, 32, 8), "Tanh", 12, 70, 60.0),                 # pre-activations beyond +-88
    "sat_silu": Case((32, 32, 8), "SiLU", 12, 70, 60.0),                 # the same for the sigmoid
}
WIDTH_FAMILY = {f"nin{n}": Case((32, 8), "SiLU", n, 70, 2.0) for n in (8, 31, 32, 33, 64, 65, 127, 128, 129)}
# one net at every batch shape; 4099 rows are 129 waves in 33 workgroups
BATCH_FAMILY = {f"B{b}": Case((50, 12), "SiLU", 10, b, 2.0) for b in (1, 31, 32, 33, 127, 128, 129, 1000, 4099)}
ALL = {**CASES, **WIDTH_FAMILY, **BATCH_FAMILY}
SATURATED = ("sat_tanh", "sat_silu")
RELU = tuple(n for n, c in ALL.items() if c.act == "ReLU")

Built = namedtuple("Built", "case flat x dout redrawn passes")


def make_fcn(case: Case, seed: int = WEIGHT_SEED):
    """The FCN of a case on the CPU, weights drawn by FCN.initialize from a generator seeded with ``seed``."""
    from synference_amd.embedding import FCN
    return FCN(list(case.widths), case.act, n_input=case.n_in, generator=torch.Generator().manual_seed(seed))


def _kink_rows(case, flat, x):
    zs = MM.run_flat(flat, case.widths, case.act, case.n_in, x).z
    bad = torch.zeros(len(x), dtype=torch.bool)
    for z in zs:
        bad |= (z.abs() < KINK).any(1)
    return bad


@functools.lru_cache(maxsize=None)
def build(name: str) -> Built:
    """Weights (flat fp32), inputs [B, n_in] fp32 and dout [B, n_out] fp32 of a case; the same on every call."""
    case = ALL[name]
    flat = make_fcn(case).flat.detach().clone()
    # (the stable digest of the name, not hash(): the inputs must not depend on PYTHONHASHSEED)
    g = torch.Generator().manual_seed(1000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    x = torch.randn(case.B, case.n_in, generator=g) * case.scale
    redrawn = torch.zeros(case.B, dtype=torch.bool)
    passes = 0
    if case.act == "ReLU":
        while True:
            bad = _kink_rows(case, flat, x)
            if not bad.any():
                break
            passes += 1
            assert passes <= 20, name
            x[bad] = torch.randn(int(bad.sum()), case.n_in, generator=g) * case.scale
            redrawn |= bad
    dout = torch.randn(case.B, case.widths[-1], generator=g)
    return Built(case, flat, x, dout, int(redrawn.sum()), passes)


# the in-kernel standardisation (sf_mlp_desc.x_mean / x_std): at n_in = 33 and 5 the padded tail of the constant image,
# pad = 4 * ceil(n_in / 4), is not empty
STD_NET = ((48, 10), "SiLU", 90)
STD_N_IN = (37, 33, 5)
StdBuilt = namedtuple("StdBuilt", "case flat x dout mean std")


@functools.lru_cache(maxsize=None)
def build_std(n_in: int) -> StdBuilt:
    """Means 100 * normal, standard deviations log-uniform over 1e-3 .. 1e3, inputs mean + 1.5 * std * normal; all fp32."""
    widths, act, B = STD_NET
    case = Case(widths, act, n_in, B, None)
    flat = make_fcn(case).flat.detach().clone()
    g = torch.Generator().manual_seed(7000 + n_in)
    mean = 100.0 * torch.randn(n_in, generator=g)
    std = 10.0 ** (6.0 * torch.rand(n_in, generator=g) - 3.0)
    x = mean + 1.5 * std * torch.randn(B, n_in, generator=g)
    dout = torch.randn(B, widths[-1], generator=g)
    return StdBuilt(case, flat, x, dout, mean, std)


@functools.lru_cache(maxsize=None)
def reference_std(n_in: int):
    """The reference standardises with the same fp32 constants."""
    b = build_std(n_in)
    return both(b.flat, b.case, b.x, b.dout, b.mean, b.std)


def both(flat, case: Case, x, dout=None, mean=None, std=None):
    """{'f64': Result, 'f32': Result} of the reference on the same inputs."""
    return {k: MM.run_flat(flat, case.widths, case.act, case.n_in, x, dout, mean, std, dt)
            for k, dt in (("f64", torch.float64), ("f32", torch.float32))}


@functools.lru_cache(maxsize=None)
def reference(name: str):
    b = build(name)
    return both(b.flat, b.case, b.x, b.dout)


def _np(t):
    return torch.as_tensor(t).detach().cpu().double().numpy()


def check(label, e_kernel, e_ref, floor):
    """sharp_cases.check_bar with its report on an 'MLP ...' line; returns the three ratios."""
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            return SC.check_bar(label, e_kernel, e_ref, floor)
    finally:
        print("MLP " + buf.getvalue().strip().removeprefix("SHARP "))


def fwd_floor(out64):
    return FWD_FLOOR * max(1.0, float(np.abs(out64).max()))


def check_forward(label, out, ref):
    o64, o32 = _np(ref["f64"].out), _np(ref["f32"].out)
    out = _np(out)
    assert out.shape == o64.shape, (out.shape, o64.shape)
    return check(label + " out", out - o64, o32 - o64, fwd_floor(o64))


def check_grads(label, gflat, ref, case: Case, other=None):
    """The bar on every tensor of the flat gradient, each under the floor of its own maximum.  With ``other`` (a second device
    gradient of the same call) the two are held against each other instead: e_ref = 0, the floor alone."""
    gflat = _np(gflat)
    lay, n = MM.layout(case.widths, case.n_in)
    assert gflat.shape == (n,), gflat.shape
    out = {}
    for (name, shape, off), g64, g32 in zip(lay, ref["f64"].grads, ref["f32"].grads):
        g64, g32 = _np(g64).reshape(-1), _np(g32).reshape(-1)
        k = g64.size
        floor = GRAD_FLOOR * max(float(np.abs(g64).max()), 1e-9)
        if other is None:
            out[name] = check(f"{label} d {name}", gflat[off:off + k] - g64, g32 - g64, floor)
        else:
            out[name] = check(f"{label} d {name}", gflat[off:off + k] - _np(other)[off:off + k], np.zeros(k), floor)
    return out
