"""Reference of the embedding MLP (synference_amd.FCN): ili's FCN restated in plain torch, in any dtype.

    Linear(n_in, w0) -> act -> ... -> Linear(w_{L-2}, w_{L-1})        no activation after the last layer

with an optional standardisation (x - mean) / std in front.  Helper module, no tests in it.

``forward`` is differentiable torch (used as the fp64 twin in front of the oracle flow); ``run`` returns the output, the gradient of
sum(out * dout) with respect to every tensor in ``FCN.layout()`` order and the hidden pre-activations.  The backward of ``run`` is
written out by hand through ``ACT_F`` / ``ACT_D``, so that tests/test_cpu_mlp_cases.py can plant a wrong derivative in the reference
itself and see the comparison rule fail; the same module holds that the hand-written backward equals autograd.

Evaluated in float64 this is the reference; evaluated in float32 (weights rounded to fp32, the same inputs, fp32 arithmetic
throughout) it is the budget of the comparison rule in tests/mlp_cases.py."""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

ACT_F = {
    "silu": lambda z: z * torch.sigmoid(z),
    "relu": lambda z: torch.clamp(z, min=0),
    "tanh": torch.tanh,
}


def _d_silu(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


ACT_D = {
    "silu": _d_silu,
    "relu": lambda z: (z > 0).to(z.dtype),
    "tanh": lambda z: 1 - torch.tanh(z) ** 2,
}

Result = namedtuple("Result", "out grads z")   # out [B, n_out]; grads: one tensor per layout entry; z: hidden pre-activations


def layout(widths, n_in):
    """[(name, shape, offset)], total: the flat parameter layout of FCN.layout()."""
    out, off = [], 0
    for l, w in enumerate(widths):
        out.append((f"layers.{l}.weight", (w, n_in), off)); off += w * n_in
        out.append((f"layers.{l}.bias", (w,), off)); off += w
        n_in = w
    return out, off


def tensors_of(flat, widths, n_in):
    """name -> view of a flat vector (the dict FCN.named_tensors() returns)."""
    lay, n = layout(widths, n_in)
    assert flat.numel() == n, (flat.numel(), n)
    return {name: flat[o:o + int(np.prod(s))].view(*s) for name, s, o in lay}


def standardise(x, mean=None, std=None):
    if mean is not None:
        x = x - mean
    if std is not None:
        x = x / std
    return x


def forward(tensors, act, x, mean=None, std=None):
    """(out, hidden pre-activations, layer inputs) in the dtype of x; differentiable."""
    f = ACT_F[act.lower()]
    L = len(tensors) // 2
    h, zs, hs = standardise(x, mean, std), [], []
    for l in range(L):
        hs.append(h)
        z = h @ tensors[f"layers.{l}.weight"].T + tensors[f"layers.{l}.bias"]
        if l + 1 < L:
            zs.append(z)
            h = f(z)
    return z, zs, hs


def run(tensors, act, x, dout=None, mean=None, std=None, dtype=torch.float64) -> Result:
    """Everything cast to ``dtype`` first (float32: the weights ROUNDED to fp32 and fp32 arithmetic throughout)."""
    cast = lambda t: None if t is None else torch.as_tensor(t).detach().cpu().to(dtype)
    T = {k: cast(v) for k, v in tensors.items()}
    x, dout, mean, std = cast(x), cast(dout), cast(mean), cast(std)
    with torch.no_grad():
        out, zs, hs = forward(T, act, x, mean, std)
        grads = None
        if dout is not None:
            fd = ACT_D[act.lower()]
            L, d, g = len(T) // 2, dout, {}
            for l in range(L - 1, -1, -1):
                g[f"layers.{l}.weight"] = d.T @ hs[l]
                g[f"layers.{l}.bias"] = d.sum(0)
                if l > 0:
                    d = (d @ T[f"layers.{l}.weight"]) * fd(zs[l - 1])
            grads = [g[k] for k in T]          # dict order = layout order
    return Result(out, grads, zs)


def run_flat(flat, widths, act, n_in, x, dout=None, mean=None, std=None, dtype=torch.float64) -> Result:
    return run(tensors_of(torch.as_tensor(flat).detach().cpu(), widths, n_in), act, x, dout, mean, std, dtype)


def flat_grad(res: Result):
    """The gradient as one float64 numpy vector in layout order."""
    return np.concatenate([g.double().reshape(-1).numpy() for g in res.grads])
