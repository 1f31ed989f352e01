"""numpy model of one optimiser step: torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam / AdamW, as sf_adam_apply and the
fused epoch (sf_flow_train_epoch) carry it out.  Helper module, no tests in it.

    norm   = |g|_2
    coef   = min(max_norm / (norm + 1e-6), 1)           when max_norm > 0, else 1
    g_eff  = coef * g  (+ weight_decay * p   for Adam's L2 term: after the clip, the parameter before the update)
    p      = p * (1 - lr * weight_decay)                 AdamW only, first
    m      = beta1 * m + (1 - beta1) * g_eff
    v      = beta2 * v + (1 - beta2) * g_eff^2
    denom  = sqrt(v) / sqrt(bc2) + eps                   bc_k = 1 - beta_k^step
    update = lr / bc1 * m / denom
    p      = p - update

The hyper-parameters enter as the float32 values sf_adam_desc carries: the fp64 model computes with float64(float32(0.999)), not with
0.999 -- (1 - beta2) alone differs by 1.3e-5 relative between the two.  bc1 and bc2 are computed in double from those values and
rounded to float32, as sf_adam_apply does (``round_bc=False`` keeps them double: torch's own arithmetic, for the comparison with
torch.optim in tests/test_cpu_step_cases.py).  ``dtype=np.float32`` gives the same formulas with every operation rounded to float32:
the yardstick of the tolerances (``reference`` / ``check_step``).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from sharp_cases import check_bar

# the fields of sf_adam_desc (include/synference_hip.h), in its order
Desc = namedtuple("Desc", "lr beta1 beta2 eps weight_decay decoupled")

FLOOR = 2.0 ** -23       # of a unit (below): one float32 ulp of a value in [1, 2)
FACTOR = 4.0             # sharp_cases.check_bar: 3 for two fp32 evaluations in a different operation order, 1 for extreme quantiles
QUANTILES = (0.5, 0.99, 1.0)
NORM_TOL = 1e-5          # relative, on scratch[1]: the bar of test_adam_step_matches_torch


def desc_values(desc, dtype=np.float64):
    """(lr, beta1, beta2, eps, weight_decay) as the float32 values the descriptor carries, in ``dtype``; works on Desc and on
    _lib.sf_adam_desc alike."""
    return tuple(dtype(np.float32(getattr(desc, k))) for k in ("lr", "beta1", "beta2", "eps", "weight_decay"))


def bias_corrections(desc, step: int, rounded: bool = True):
    b1, b2 = np.float64(np.float32(desc.beta1)), np.float64(np.float32(desc.beta2))
    bc1, bc2 = 1.0 - b1 ** float(step), 1.0 - b2 ** float(step)
    return (np.float32(bc1), np.float32(bc2)) if rounded else (bc1, bc2)


def clip_coef(norm, max_norm, dtype=np.float64):
    mx = dtype(np.float32(max_norm))
    if not mx > 0:
        return dtype(1.0)
    # (1e-6f in the kernels, 1e-6 in torch: the two differ by 3e-14, far below either precision at any norm that clips)
    tiny = np.float32(1e-6) if dtype is np.float32 else np.float64(1e-6)
    return min(mx / (norm + tiny), dtype(1.0))


def effective_grad(p, g, desc, max_norm, dtype=np.float64):
    """(g_eff, norm): the clipped gradient plus the L2 term, and the norm before the clip."""
    lr, b1, b2, eps, wd = desc_values(desc, dtype)
    p, g = np.asarray(p).astype(dtype), np.asarray(g).astype(dtype)
    norm = np.sqrt(np.sum(g * g, dtype=dtype))
    ge = g * clip_coef(norm, max_norm, dtype)
    if not desc.decoupled and wd != 0:
        ge = ge + wd * p
    return ge, norm


def adam_step(p, g, m, v, step: int, desc, max_norm, dtype=np.float64, round_bc: bool = True):
    """One step; returns (p, m, v, update, norm), every array in ``dtype``."""
    assert step >= 1
    one = dtype(1.0)
    lr, b1, b2, eps, wd = desc_values(desc, dtype)
    p, m, v = (np.asarray(a).astype(dtype) for a in (p, m, v))
    ge, norm = effective_grad(p, g, desc, max_norm, dtype)
    if desc.decoupled:
        p = p * (one - lr * wd)
    bc1, bc2 = (dtype(b) for b in bias_corrections(desc, step, round_bc))
    m = b1 * m + (one - b1) * ge
    v = b2 * v + ((one - b2) * ge) * ge
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    update = (lr / bc1) * (m / denom)
    out = (p - update, m, v, update, norm)
    assert all(np.asarray(a).dtype == dtype for a in out)
    return out


def warm_state(p, desc, step: int, seed: int, scale: float = 1.0, max_steps: int = 8):
    """float32 (m, v) of an optimiser about to take step ``step``: the fp64 model run min(step - 1, max_steps) times on seeded
    gradients ~ scale * N(0, 1) at the parameters ``p`` (held fixed), so that m and v are consistent with each other.  Zeros at
    step 1."""
    p = np.asarray(p)
    m, v = np.zeros(p.shape), np.zeros(p.shape)
    rng = np.random.default_rng(seed)
    k = min(step - 1, max_steps)
    for t in range(step - k, step):
        _, m, v, _, _ = adam_step(p, (scale * rng.normal(size=p.shape)).astype(np.float32), m, v, t, desc, 0.0)
    return m.astype(np.float32), v.astype(np.float32)


Reference = namedtuple("Reference", "p m v update norm p32 m32 v32 norm32 unit_p unit_m unit_v")


def reference(p0, g, m0, v0, step: int, desc, max_norm) -> Reference:
    """The fp64 model, the float32 model and the units the errors are expressed in, element by element:
      m: |beta1 * m0| + |(1 - beta1) * g_eff|      v: beta2 * v0 + (1 - beta2) * g_eff^2      p: max(lr, |p_ref|)
    with g_eff the clipped gradient (plus the L2 term) of the fp64 model."""
    p, m, v, upd, norm = adam_step(p0, g, m0, v0, step, desc, max_norm)
    p32, m32, v32, _, n32 = adam_step(p0, g, m0, v0, step, desc, max_norm, dtype=np.float32)
    lr, b1, b2, _, _ = desc_values(desc)
    ge, _ = effective_grad(p0, g, desc, max_norm)
    m0, v0 = np.asarray(m0, dtype=np.float64), np.asarray(v0, dtype=np.float64)
    return Reference(p, m, v, upd, float(norm), p32, m32, v32, float(n32),
                     unit_p=np.maximum(lr, np.abs(p)), unit_m=np.abs(b1 * m0) + np.abs((1 - b1) * ge),
                     unit_v=b2 * v0 + (1 - b2) * ge * ge)


def unit_errors(got, ref64, unit):
    """|got - ref64| / unit where the unit is positive; where it is 0, got must equal the reference exactly (both are 0 there)."""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    pos = unit > 0
    assert np.array_equal(got[~pos], ref64[~pos]), "elements whose unit is 0 are not exactly equal"
    return np.abs(got[pos] - ref64[pos]) / unit[pos]


def yardstick(ref: Reference):
    """{'m' | 'v' | 'p': the float32 model's error against the fp64 model, in units}."""
    return {"m": unit_errors(ref.m32, ref.m, ref.unit_m), "v": unit_errors(ref.v32, ref.v, ref.unit_v),
            "p": unit_errors(ref.p32, ref.p, ref.unit_p)}


def check_step(label: str, p, m, v, ref: Reference):
    """m, v and p of a device step against the fp64 model: sharp_cases.check_bar with the float32 model's error on the same inputs as
    the reference error, factor 4, quantiles 0.5 / 0.99 / 1.0, floor 2^-23 of a unit.  Prints the ratios, returns them."""
    yd = yardstick(ref)
    out = {}
    for key, got, want, unit in (("m", m, ref.m, ref.unit_m), ("v", v, ref.v, ref.unit_v), ("p", p, ref.p, ref.unit_p)):
        got = np.asarray(got, dtype=np.float64)
        assert np.isfinite(got).all(), (label, key, "non-finite")
        e = unit_errors(got, want, unit)
        if e.size:
            out[key] = check_bar(f"{label} {key}", e, yd[key], FLOOR, FACTOR)
    return out


def check_norm(label: str, got: float, g):
    """scratch[1] against the fp64 norm of the float32 gradient: 1e-5 relative, exactly 0 for a zero gradient."""
    g = np.asarray(g, dtype=np.float64)
    want = float(np.sqrt((g * g).sum()))
    print(f"STEP {label}: norm {got:.9g} fp64 {want:.9g} rel {abs(got - want) / want if want else 0.0:.2e}")
    if want == 0:
        assert got == 0, (label, got)
    else:
        assert abs(got - want) <= NORM_TOL * want, (label, got, want)
    return want
