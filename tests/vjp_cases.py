"""Cases of the weighted-gradient conformance tests (tests/test_gpu_vjp.py; conditions held by tests/test_cpu_vjp_cases.py).  Helper
module, no tests in it; numpy and the oracle only.

sf_flow_loss_grad_weighted / sf_flow_loss_grad_rows take per-sample weights: grad = sum_b grad_scale * w_b * d loss_b / d flat, the
vector-Jacobian product behind every backward() of FlowEstimator.  Each training kernel reads w by BATCH position while theta / x are
gathered through ``rows``.  One case per kernel and accumulation form, four weight patterns each:

  uniform      U(0.5, 1.5): the control
  signed       N(0, 1), a seeded quarter of the entries exactly 0, one whole 32-row tile exactly 0, both signs in every other tile
               (a ragged tile of a single row, B = 513, has a nonzero weight)
  onehot_last  1 at b = B - 1 (in the ragged tile), 0 elsewhere: one sample's gradient
  zeros        all 0

Reference: oracle.flows.log_prob in float64, (-(lp * w).sum() * grad_scale) differentiated by autograd with respect to the flat vector
and the context rows; the budget of sharp_cases.check_bar is the same expression in float32 on the same inputs.  The forward graph is
built once per (case, form, precision) and differentiated once per weight vector.
"""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

import sharp_cases as SC
from cases import make_case
from oracle import flows as OF

TILE = 32                 # rows per tile of the 32-row kernels (and per half-chunk of the cooperative ones)
N_TRAIN = 300             # rows of the training arrays of the ``rows`` form
WRONG_FACTOR = 20.0       # a wrong reading of the weights differs by 20 x the bar's maximum ...
WRONG_MIN = WRONG_FACTOR * (1.0 + SC.FACTOR) * SC.GRAD_FLOOR     # ... = 0.02 of max |g64|, given condition 1 (5 floors)

VjpCase = namedtuple("VjpCase", "name B dctx path what")
# path: sf_flow_train_path(B, dctx) as the dispatch stands; None = whatever the library reports (engines of their own, no dctx)
SMALL = [
    VjpCase("maf_cfg1", 70, False, 1, "cooperative MAF, 4 waves"),
    VjpCase("maf_cfg1", 70, True, 1, "cooperative MAF, 4 waves, dctx form"),
    VjpCase("maf_cli", 70, False, 1, "cooperative MAF, two input tiles"),
    VjpCase("maf_cli", 70, True, 0, "32-row MAF for dctx"),
    VjpCase("maf_wide", 70, False, 0, "32-row MAF, HT = 3"),
    VjpCase("maf_wide", 513, False, 0, "32-row MAF, 17 tiles: f32-atomic gather"),
    VjpCase("maf_nb3", 70, True, 0, "32-row MAF, NB = 3"),
    VjpCase("nsf_cfg3", 70, False, 3, "cooperative NSF"),
    VjpCase("nsf_cfg3", 70, True, 0, "32-row NSF for dctx"),
    VjpCase("nsf_h69", 70, False, 3, "cooperative NSF, five-wave workgroups"),
    VjpCase("nsf_k16", 70, True, 0, "32-row NSF, PT = 3"),
    VjpCase("nsf_d1", 70, False, None, "one-parameter engine"),
    VjpCase("nsfar_small", 70, False, None, "lampe NSF"),
    VjpCase("nsfar_cfg1", 70, False, None, "lampe NSF, cfg1 shape"),
    VjpCase("mafar_small", 70, False, None, "lampe MAF"),
]
# signed weights, no rows
LARGE = [
    VjpCase("maf_cfg1", 8192 + 37, False, 2, "cooperative MAF, 8-wave workgroups"),
    VjpCase("maf_cfg1", 16384 + 64 + 5, False, 2, "cooperative MAF, second chunk on some persistent workgroups"),
    VjpCase("nsf_cfg3", 16384 + 37, False, 3, "cooperative NSF, second chunk, XCD replicas + f32 atomics"),
]
NO_DCTX = ("nsf_d1", "nsfar_small", "nsfar_cfg1", "mafar_small")    # kinds whose dctx request is refused (SF_ERR_INVALID)
LAMPE = ("nsfar_small", "nsfar_cfg1", "mafar_small")                # gradients repeat to rounding, not to the bit

PATTERNS = ("uniform", "signed", "onehot_last", "zeros")
BOTH_FORMS = ("uniform", "signed")          # through loss_grad(weights=) and through loss_grad_rows with weights
SCALES = ("mean", "sum")                    # grad_scale 1 / B and 1.0


def case_id(c: VjpCase) -> str:
    return f"{c.name}-{c.B}{'-dctx' if c.dctx else ''}"


def grad_scale(B: int, key: str) -> float:
    return {"mean": 1.0 / B, "sum": 1.0}[key]


def _seed(text: str) -> int:
    return zlib.crc32(text.encode())


def tiles(B: int):
    return [slice(t * TILE, min(B, (t + 1) * TILE)) for t in range((B + TILE - 1) // TILE)]


def zero_tile(B: int) -> int:
    """The tile of the signed pattern whose weights are all 0: the middle full tile."""
    return (B // TILE) // 2


def _both_signs(w) -> bool:
    """Both signs among the weights of a tile; a ragged tile of one row (B = 513) can only be asked for a nonzero weight."""
    return bool((w > 0).any() and (w < 0).any()) if len(w) > 1 else bool(w[0] != 0)


@functools.lru_cache(maxsize=None)
def weights(name: str, B: int, pattern: str) -> np.ndarray:
    """float32 [B], read-only."""
    seed = _seed(f"{name}-{B}-{pattern}")
    if pattern == "uniform":
        w = np.random.default_rng(seed).uniform(0.5, 1.5, size=B)
    elif pattern == "signed":
        zt = zero_tile(B)
        for s in range(seed, seed + 1000):       # the first seed at which every other tile keeps both signs (ragged ones have few rows)
            rng = np.random.default_rng(s)
            w = rng.normal(size=B)
            w[rng.permutation(B)[:(B + 3) // 4]] = 0.0
            w[tiles(B)[zt]] = 0.0
            if all(t == zt or _both_signs(w[sl]) for t, sl in enumerate(tiles(B))):
                break
        else:
            raise AssertionError("no seed gives both signs in every tile")
    elif pattern == "onehot_last":
        w = np.zeros(B)
        w[B - 1] = 1.0
    elif pattern == "zeros":
        w = np.zeros(B)
    else:
        raise ValueError(pattern)
    w = w.astype(np.float32)
    w.setflags(write=False)
    return w


def wrong_readings(w: np.ndarray, rows=None) -> dict:
    """The weights as a kernel with a wrong index would see them."""
    B = len(w)
    out = {"ones": np.ones_like(w), "rolled": np.roll(w, 1)}
    r = B - B % TILE
    if r < B:
        ragged = w.copy()
        ragged[r:] = w[:B - r]
        out["ragged_from_first"] = ragged
    if rows is not None:
        out["by_gathered_row"] = w[np.asarray(rows) % B]
    return out


Inputs = namedtuple("Inputs", "ospec spec flat theta x rows theta_b x_b")


@functools.lru_cache(maxsize=None)
def inputs(name: str, B: int, rows_form: bool) -> Inputs:
    """make_case(name); without rows the B rows of the call; with rows N_TRAIN training rows and ``rows`` int64 [B], seeded, with
    duplicates, not monotone.  theta_b / x_b: the rows the call names, batch-indexed."""
    if not rows_form:
        ospec, spec, flat, theta, x = make_case(name, B=B)
        rows, theta_b, x_b = None, theta, x
    else:
        ospec, spec, flat, theta, x = make_case(name, B=N_TRAIN)
        rows = np.random.default_rng(_seed(f"{name}-{B}-rows")).integers(0, N_TRAIN, size=B).astype(np.int64)
        rows[B - 1] = rows[0]                       # a duplicate whatever the draw
        rows[1], rows[2] = max(rows[1], rows[2]), min(rows[1], rows[2])
        theta_b, x_b = theta[rows], x[rows]
        rows.setflags(write=False)
    for a in (flat, theta, x, theta_b, x_b):
        a.setflags(write=False)
    return Inputs(ospec, spec, flat, theta, x, rows, theta_b, x_b)


_DT = {"f64": torch.float64, "f32": torch.float32}


@functools.lru_cache(maxsize=6)
def _graph(name: str, B: int, rows_form: bool, key: str):
    """(flat, x_b, lp) of the oracle in one precision, with the autograd graph kept."""
    i = inputs(name, B, rows_form)
    dt = _DT[key]
    p = torch.as_tensor(np.array(i.flat)).to(dt).requires_grad_(True)
    th = torch.as_tensor(np.array(i.theta_b)).to(dt)
    xb = torch.as_tensor(np.array(i.x_b)).to(dt).requires_grad_(True)
    return p, xb, OF.log_prob(i.ospec, p, th, xb)


def grads_for(name: str, B: int, rows_form: bool, w, scale: float, key: str = "f64"):
    """(d / d flat [P], d / d x_b [B, C]) of -(lp * w).sum() * scale as float64 numpy; w: float32 weights, cast to the precision."""
    p, xb, lp = _graph(name, B, rows_form, key)
    wt = torch.as_tensor(np.array(w, dtype=np.float32)).to(lp.dtype)
    gp, gx = torch.autograd.grad(-(lp * wt).sum() * scale, [p, xb], retain_graph=True, allow_unused=True)
    gp = torch.zeros_like(p) if gp is None else gp
    gx = torch.zeros_like(xb) if gx is None else gx
    return gp.double().numpy(), gx.double().numpy()


Ref = namedtuple("Ref", "loss64 loss32 g64 g32 dx64 dx32")


@functools.lru_cache(maxsize=None)
def reference(name: str, B: int, rows_form: bool, pattern: str, scale_key: str) -> Ref:
    """The fp64 reference and the fp32 budget of one weighted call, once per session."""
    w, s = weights(name, B, pattern), grad_scale(B, scale_key)
    g64, dx64 = grads_for(name, B, rows_form, w, s, "f64")
    g32, dx32 = grads_for(name, B, rows_form, w, s, "f32")
    loss = [-_graph(name, B, rows_form, k)[2].detach().double().numpy() for k in ("f64", "f32")]
    out = Ref(loss[0], loss[1], g64, g32, dx64, dx32)
    for a in out:
        a.setflags(write=False)
    return out


def per_sample_gradient(name: str, B: int, rows_form: bool, b: int, scale: float) -> np.ndarray:
    """d (-log p_b * scale) / d flat in float64 from a forward pass over that one row."""
    i = inputs(name, B, rows_form)
    p = torch.as_tensor(np.array(i.flat)).double().requires_grad_(True)
    lp = OF.log_prob(i.ospec, p, torch.as_tensor(np.array(i.theta_b[b:b + 1])).double(), torch.as_tensor(np.array(i.x_b[b:b + 1])).double())
    (g,) = torch.autograd.grad(-lp.sum() * scale, [p])
    return g.numpy()


def tensor_max(ospec, d) -> dict:
    """max |d| per tensor of the flat layout."""
    return {n: float(np.abs(d[o:o + int(np.prod(s))]).max()) for n, s, o in OF.param_layout(ospec)}
