"""The trainer sweep: configs that reach every instantiation of the two cooperative training kernels (k_maf_trainc<TS, NI, NT, NG, NFS>,
csrc/sf_trainc.hip; k_nsf_trainc<NT, OTQ> with one to three input tiles, csrc/sf_nsfc.hip), the shapes just outside their envelope,
the family a handle reports on the host, the fp64 / fp32 oracle references and the one comparison rule.

Helper module, no tests in it; numpy, torch and the oracle only.  tests/test_cpu_trainer_cases.py holds which families the list
reaches and the conditions on the reference alone, tests/test_gpu_trainer_sweep.py the comparisons with the kernels.

A config is the 8-tuple sweep_cases.build_case takes: (kind, D, C, H, T, K, NB = 2, seed).  CONFIGS is a fixed list: 500 MAF and 400
NSF shapes drawn inside the cooperative envelope (numpy default_rng(4242) / default_rng(4243), seeds 1000.. / 2000.. in drawing
order: D in 2 .. 8, MAF C in 1 .. 24, H in 1 .. 64, T in 1 .. 8; NSF C in 1 .. 40, H in 17 .. 80, T in 1, 2, 3, 5, K in 2 .. 11),
thinned greedily to the ones that add a family or a required shape and whose fp32 oracle meets the reference conditions with 40 % to
spare, then corners by hand (seeds 1500.. and 2500..).  It is not regenerated at import.

The rule (``check_rule``), per call:

    per-row loss     quantile_q |loss + lp64|  <=  4 * quantile_q |lp32 - lp64| + 1e-4                q in 0.5, 0.99, 1
    gradient         max |g_t - g64_t|         <=  4 * max |g32_t - g64_t| + 2e-4 * max |g64_t|       per tensor t of OF.param_layout

g32 / lp32: the fp32 oracle on the same inputs, never the kernel.  Factor and floors are sharp_cases.FACTOR, LOGP_FLOOR, GRAD_FLOOR; the
scale of the gradient floor is the TENSOR's own maximum, not the vector's.  A tensor whose fp64 gradient is exactly 0 must come out
exactly 0.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np
import torch

import sharp_cases as SC
import sweep_cases as SW
import vjp_cases as VC
from oracle import flows as OF

BATCHES = (1, 33, 70)        # one live row of a 32-row chunk; a chunk plus one row; two chunks plus six rows, several workgroups
B_EIGHT_WAVE = 8192 + 37     # 8-wave workgroups (above 8 192 rows): 64-row chunks, the last fills group 0 and leaves 5 rows in group 1
B_MAIN = 70                  # the weighted, context-gradient and epoch calls; the reference conditions
N_TRAIN = VC.N_TRAIN         # training rows of the ``rows`` form

# ---------------------------------------------------------------------------------------------------------------------------
# the configs
# ---------------------------------------------------------------------------------------------------------------------------
MAF_CONFIGS = [
    ("maf", 2, 6, 45, 2, 10, 2, 1001),      # NI 1 NT 3 TS 5 NFS 8
    ("maf", 7, 9, 16, 2, 10, 2, 1002),      # NI 1 NT 1 TS 5 NFS 5
    ("maf", 2, 8, 61, 2, 10, 2, 1003),      # NI 1 NT 4 TS 5 NFS 8
    ("maf", 8, 14, 60, 8, 10, 2, 1004),     # NI 2 NT 4 TS 8 NFS 8; four-wave workgroups only
    ("maf", 2, 11, 34, 7, 10, 2, 1005),     # NI 1 NT 3 TS 8 NFS 8
    ("maf", 7, 14, 41, 5, 10, 2, 1006),     # NI 2 NT 3 TS 5 NFS 5
    ("maf", 5, 22, 64, 6, 10, 2, 1008),     # NI 2 NT 4 TS 6 NFS 5
    ("maf", 6, 18, 19, 3, 10, 2, 1010),     # NI 2 NT 2 TS 5 NFS 5
    ("maf", 4, 6, 60, 8, 10, 2, 1011),      # NI 1 NT 4 TS 8 NFS 8; four-wave workgroups only
    ("maf", 6, 20, 6, 3, 10, 2, 1012),      # NI 2 NT 1 TS 5 NFS 5
    ("maf", 7, 24, 17, 6, 10, 2, 1013),     # NI 2 NT 2 TS 6 NFS 5
    ("maf", 2, 4, 17, 3, 10, 2, 1015),      # NI 1 NT 2 TS 5 NFS 5
    ("maf", 3, 24, 61, 5, 10, 2, 1016),     # NI 2 NT 4 TS 5 NFS 8
    ("maf", 5, 10, 36, 2, 10, 2, 1017),     # NI 1 NT 4 TS 5 NFS 5
    ("maf", 6, 7, 35, 6, 10, 2, 1018),      # NI 1 NT 3 TS 6 NFS 5
    ("maf", 6, 21, 29, 6, 10, 2, 1023),     # NI 2 NT 3 TS 6 NFS 5
    ("maf", 7, 18, 16, 7, 10, 2, 1027),     # NI 2 NT 1 TS 8 NFS 5
    ("maf", 4, 7, 34, 3, 10, 2, 1031),      # NI 1 NT 3 TS 5 NFS 5
    ("maf", 2, 13, 30, 7, 10, 2, 1032),     # NI 1 NT 2 TS 8 NFS 5
    ("maf", 6, 12, 11, 6, 10, 2, 1037),     # NI 2 NT 1 TS 6 NFS 5
    ("maf", 4, 5, 38, 7, 10, 2, 1044),      # NI 1 NT 3 TS 8 NFS 5
    ("maf", 8, 8, 1, 6, 10, 2, 1050),       # NI 1 NT 1 TS 6 NFS 5
    ("maf", 7, 20, 22, 7, 10, 2, 1053),     # NI 2 NT 2 TS 8 NFS 5
    ("maf", 4, 16, 63, 6, 10, 2, 1062),     # NI 2 NT 4 TS 6 NFS 8
    ("maf", 8, 17, 55, 2, 10, 2, 1079),     # NI 2 NT 4 TS 5 NFS 5
    ("maf", 2, 23, 47, 2, 10, 2, 1089),     # NI 2 NT 3 TS 5 NFS 8
    ("maf", 4, 18, 28, 7, 10, 2, 1106),     # NI 2 NT 3 TS 8 NFS 5
    ("maf", 2, 8, 63, 6, 10, 2, 1130),      # NI 1 NT 4 TS 6 NFS 8
    ("maf", 5, 23, 36, 8, 10, 2, 1143),     # NI 2 NT 4 TS 8 NFS 5; four-wave workgroups only
    ("maf", 8, 6, 51, 6, 10, 2, 1152),      # NI 1 NT 4 TS 6 NFS 5
    ("maf", 4, 1, 6, 8, 10, 2, 1188),       # NI 1 NT 1 TS 8 NFS 5
    ("maf", 2, 23, 39, 6, 10, 2, 1217),     # NI 2 NT 3 TS 6 NFS 8
    ("maf", 2, 12, 39, 6, 10, 2, 1333),     # NI 1 NT 3 TS 6 NFS 8
    ("maf", 2, 2, 17, 6, 10, 2, 1350),      # NI 1 NT 2 TS 6 NFS 5
    ("maf", 5, 11, 40, 7, 10, 2, 1359),     # NI 1 NT 4 TS 8 NFS 5; four-wave workgroups only
    # by hand: the one family the draws missed; the largest C of one input tile (D + C = 16) at D = 2 and at D = 8 with H = 64
    ("maf", 2, 20, 33, 8, 10, 2, 1500),       # NI 2 NT 3 TS 8 NFS 8
    ("maf", 2, 14, 17, 4, 10, 2, 1501),       # NI 1 NT 2 TS 5 NFS 5
    ("maf", 8, 8, 64, 5, 10, 2, 1502),        # NI 1 NT 4 TS 5 NFS 8
]
NSF_CONFIGS = [
    ("nsf", 4, 20, 33, 5, 4, 2, 2000),      # NT 3 OTQ 6 NI 2, 4 padding slots
    ("nsf", 7, 12, 35, 3, 10, 2, 2002),     # NT 3 OTQ 8 NI 2, 1 padding slots
    ("nsf", 8, 40, 32, 1, 7, 2, 2008),      # NT 2 OTQ 6 NI 3, 1 padding slots
    ("nsf", 8, 22, 50, 2, 10, 2, 2011),     # NT 4 OTQ 8 NI 2, 1 padding slots
    ("nsf", 5, 21, 57, 5, 4, 2, 2014),      # NT 4 OTQ 6 NI 2, 4 padding slots
    ("nsf", 6, 40, 37, 3, 5, 2, 2015),      # NT 3 OTQ 6 NI 3, 3 padding slots
    ("nsf", 3, 25, 62, 2, 9, 2, 2016),      # NT 4 OTQ 8 NI 3, 2 padding slots
    ("nsf", 5, 10, 30, 1, 3, 2, 2017),      # NT 2 OTQ 6 NI 2, 5 padding slots
    ("nsf", 3, 8, 42, 3, 9, 2, 2021),       # NT 3 OTQ 8 NI 1, 2 padding slots
    ("nsf", 5, 2, 63, 5, 4, 2, 2023),       # NT 4 OTQ 6 NI 1, 4 padding slots
    ("nsf", 4, 1, 27, 3, 9, 2, 2028),       # NT 2 OTQ 8 NI 1, 2 padding slots
    ("nsf", 6, 17, 23, 1, 10, 2, 2034),     # NT 2 OTQ 8 NI 2, 1 padding slots
    ("nsf", 4, 8, 33, 2, 4, 2, 2041),       # NT 3 OTQ 6 NI 1, 4 padding slots
    ("nsf", 7, 40, 65, 1, 8, 2, 2045),      # NT 5 OTQ 6 NI 3, 0 padding slots
    ("nsf", 6, 28, 64, 5, 8, 2, 2046),      # NT 4 OTQ 6 NI 3, 0 padding slots
    ("nsf", 6, 24, 71, 3, 10, 2, 2048),     # NT 5 OTQ 8 NI 2, 1 padding slots
    ("nsf", 3, 1, 69, 3, 6, 2, 2050),       # NT 5 OTQ 6 NI 1, 2 padding slots
    ("nsf", 4, 3, 78, 5, 9, 2, 2055),       # NT 5 OTQ 8 NI 1, 2 padding slots
    ("nsf", 2, 3, 17, 2, 5, 2, 2062),       # NT 2 OTQ 6 NI 1, 3 padding slots
    ("nsf", 2, 3, 58, 5, 11, 2, 2082),      # NT 4 OTQ 8 NI 1, 0 padding slots
    ("nsf", 5, 27, 45, 2, 10, 2, 2102),     # NT 3 OTQ 8 NI 3, 1 padding slots
    ("nsf", 6, 25, 20, 5, 11, 2, 2154),     # NT 2 OTQ 8 NI 3, 0 padding slots
    ("nsf", 5, 9, 69, 1, 2, 2, 2245),       # NT 5 OTQ 6 NI 2, 6 padding slots
    ("nsf", 6, 25, 80, 3, 9, 2, 2314),      # NT 5 OTQ 8 NI 3, 2 padding slots
    # by hand: the smallest and the largest shape of the envelope; odd D with a full second input tile and a full 8-slot head
    ("nsf", 2, 1, 17, 1, 2, 2, 2500),         # NT 2 OTQ 6 NI 1, 6 padding slots
    ("nsf", 8, 40, 80, 5, 11, 2, 2504),       # NT 5 OTQ 8 NI 3, 0 padding slots
    ("nsf", 3, 24, 65, 1, 8, 2, 2502),        # NT 5 OTQ 6 NI 2, 0 padding slots
]
CONFIGS = MAF_CONFIGS + NSF_CONFIGS

# One config just outside each edge of the envelope (train_path 0: the 32-row kernels): MAF D = 1 (no autoregressive input), D = 9 (a
# second input tile of theta alone is no cooperative shape), T = 9 (beyond the deepest stash), H = 65 (five hidden tiles); NSF D = 9,
# K = 12 (a three-tile head), H = 16 (one hidden tile), H = 81 (six), C = 41 (four input tiles).
NEIGHBOURS = [
    ("maf", 1, 5, 20, 3, 10, 2, 3000), ("maf", 9, 5, 40, 3, 10, 2, 3001), ("maf", 4, 6, 33, 9, 10, 2, 3002),
    ("maf", 4, 6, 65, 3, 10, 2, 3003),
    ("nsf", 9, 6, 40, 2, 6, 2, 3010), ("nsf", 4, 6, 40, 2, 12, 2, 3011), ("nsf", 4, 6, 16, 2, 6, 2, 3012),
    ("nsf", 4, 6, 81, 2, 6, 2, 3013), ("nsf", 4, 41, 40, 2, 6, 2, 3014),
]
ALL_CONFIGS = CONFIGS + NEIGHBOURS

config_id = SW.config_id


def by_seed(seed: int):
    return next(c for c in ALL_CONFIGS if c[-1] == seed)


# ---------------------------------------------------------------------------------------------------------------------------
# families, from what the library reports on the host
# ---------------------------------------------------------------------------------------------------------------------------
MafFamily = namedtuple("MafFamily", "NI NT TS NFS NG")
NsfFamily = namedtuple("NsfFamily", "NT OTQ NI pad")


def trc_ts(T: int) -> int:
    """Stash depth of the instantiation a MAF of T transforms runs (csrc/sf_trainc.h, sf_trc_ts)."""
    return 5 if T <= 5 else 6 if T <= 6 else 8


def trc_slots_needed(d: dict) -> int:
    """Fragment slots per masked layer and wave (csrc/sf_trainc.h, sf_trc_slots_needed): a wave holds the fragments of hidden tiles p
    and NT - 1 - p; forward the input tiles 0 .. kend, backward the output tiles kbeg .. NT - 1."""
    NT, mx = d["NT"], 0
    for p in range((NT + 1) // 2):
        a, b = p, NT - 1 - p
        nf = d[f"kend{a}"] + 1 + (d[f"kend{b}"] + 1 if b > a else 0)
        nb = NT - d[f"kbeg{a}"] + (NT - d[f"kbeg{b}"] if b > a else 0)
        mx = max(mx, nf, nb)
    return mx


def family(hf, B: int):
    """The kernel instantiation ``loss_grad`` of B rows (no context gradient) runs on this handle: MafFamily / NsfFamily, or None
    where the library reports train_path 0.  Host only: trainc_table()[3], train_path and spec.T."""
    path = hf.train_path(B, False)
    if path == 0:
        return None
    d = hf.trainc_table()[3]
    if hf.spec.kind == "maf":
        assert path in (1, 2), path
        return MafFamily(d["NI"], d["NT"], trc_ts(hf.spec.T), 8 if trc_slots_needed(d) > 5 else 5, path)
    assert hf.spec.kind == "nsf" and path == 3, (hf.spec.kind, path)
    return NsfFamily(d["NT"], d["OTQ"], d["NI"], d["KM"] - hf.spec.K)


def handle(cfg):
    """A HipFlow of the config (creating one needs no GPU)."""
    from synference_amd.engine import HipFlow
    return HipFlow(SW.sweep_case(cfg).spec)


def expected_path(cfg, B: int) -> int:
    """train_path(B, no context gradient) as the dispatch stands: 0 for the neighbours, 3 for an NSF, 1 or 2 for a MAF."""
    if cfg in NEIGHBOURS:
        return 0
    if cfg[0] == "nsf":
        return 3
    return 2 if B > 8192 and cfg in EIGHT_WAVE else 1


# MAF (NI, NT, TS, NFS) -> the config that runs it with 8-wave workgroups at B_EIGHT_WAVE (every family but NT = 4, TS = 8, whose stash
# leaves LDS for one group of four waves only); by seed.
_EIGHT_WAVE_SEEDS = (
    1001, 1002, 1003, 1005, 1006, 1008, 1010, 1012, 1013, 1015, 1016, 1017, 1018, 1023, 1027, 1031,
    1032, 1037, 1044, 1050, 1053, 1062, 1079, 1089, 1106, 1130, 1152, 1188, 1217, 1333, 1350, 1500,
)
EIGHT_WAVE = [c for c in MAF_CONFIGS if c[-1] in _EIGHT_WAVE_SEEDS]
# one config per (kind, NI) for the epoch step: MAF NI 1, 2; NSF NI 1, 2, 3
_STEP_SEEDS = (
    1031, 1010, 2021, 2011, 2015,
)
STEP_CONFIGS = [c for c in CONFIGS if c[-1] in _STEP_SEEDS]


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
Ref = namedtuple("Ref", "loss64 loss32 g64 g32")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def reference(cfg, B: int) -> Ref:
    """Loss rows and d mean(-log p) / d flat of sweep_case(cfg, B) by the oracle's autograd, in fp64 and (budget) in fp32."""
    c = SW.sweep_case(cfg, B)
    b = SC.budget(c.ospec, c.flat, c.theta, c.x, None, "grad")
    return Ref(*_frozen(b["f64"][0], b["f32"][0], b["f64"][1], b["f32"][1]))


@functools.lru_cache(maxsize=None)
def dctx_reference(cfg, B: int):
    """(fp64, fp32) d mean(-log p) / d x [B, C]."""
    c = SW.sweep_case(cfg, B)
    b = SC.budget(c.ospec, c.flat, c.theta, c.x, None, "dctx")
    return _frozen(b["f64"] / B, b["f32"] / B)


Weighted = namedtuple("Weighted", "case rows w ref")


@functools.lru_cache(maxsize=None)
def weighted(cfg) -> Weighted:
    """The weighted call of the sweep: N_TRAIN training rows, B_MAIN seeded batch rows (duplicates, not monotone: the construction of
    vjp_cases.inputs), the signed weights of vjp_cases (both signs, a quarter exactly 0, one whole 32-row tile 0), and the reference
    -(lp * w).sum() / B by autograd on the gathered rows in both precisions.  The loss rows are not weighted."""
    B, name = B_MAIN, config_id(cfg)
    c = SW.sweep_case(cfg, N_TRAIN)
    rows = np.random.default_rng(VC._seed(f"{name}-{B}-rows")).integers(0, N_TRAIN, size=B).astype(np.int64)
    rows[B - 1] = rows[0]
    rows[1], rows[2] = max(rows[1], rows[2]), min(rows[1], rows[2])
    w = VC.weights(name, B, "signed")
    out = {}
    for key, dt in (("f64", torch.float64), ("f32", torch.float32)):
        p = torch.as_tensor(np.array(c.flat)).to(dt).requires_grad_(True)
        lp = OF.log_prob(c.ospec, p, torch.as_tensor(c.theta[rows]).to(dt), torch.as_tensor(c.x[rows]).to(dt))
        (-(lp * torch.as_tensor(np.array(w)).to(dt)).sum() / B).backward()
        out[key] = (-lp.detach().double().numpy(), p.grad.double().numpy())
    _frozen(rows)
    return Weighted(c, rows, w, Ref(*_frozen(out["f64"][0], out["f32"][0], out["f64"][1], out["f32"][1])))


# ---------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------
def tensor_errors(ospec, grad, ref: Ref):
    """[(tensor name, max |grad_t - g64_t|, max |g32_t - g64_t|, max |g64_t|)] over OF.param_layout."""
    out = []
    for name, shape, off in OF.param_layout(ospec):
        s = slice(off, off + int(np.prod(shape)))
        out.append((name, float(np.abs(grad[s] - ref.g64[s]).max()), float(np.abs(ref.g32[s] - ref.g64[s]).max()),
                    float(np.abs(ref.g64[s]).max())))
    return out


def check_rule(label: str, ospec, loss, grad, ref: Ref, factor: float = SC.FACTOR, grad_floor: float = SC.GRAD_FLOOR):
    """The rule of the module docstring on one call's loss rows [B] and flat gradient [P] (numpy); ``label`` names config, batch,
    path and family.  No allowance beyond the rule is taken anywhere (DESIGN.md 0e has the measured margins).
    Prints ONE line -- the worst tensor under the rule with its ratio to its bar, and the largest ratio the same errors have to
    the bar whose floor is 2e-4 of the whole vector's maximum -- then asserts.  Returns (worst tensor, its ratio, global-scale ratio)."""
    loss, grad = np.asarray(loss, dtype=np.float64), np.asarray(grad, dtype=np.float64)
    assert loss.shape == ref.loss64.shape and grad.shape == ref.g64.shape, (label, loss.shape, grad.shape)
    e_loss, e_ref = np.abs(loss - ref.loss64), np.abs(ref.loss32 - ref.loss64)
    loss_ratio, loss_fail = 0.0, []
    for q in SC.QUANTILES:
        k, bar = np.quantile(e_loss, q), factor * np.quantile(e_ref, q) + SC.LOGP_FLOOR
        loss_ratio = max(loss_ratio, float(k / bar)) if np.isfinite(k) else float("inf")
        if not k <= bar:
            loss_fail.append((q, float(k), float(bar)))
    gmax = float(np.abs(ref.g64).max())
    worst, old, fails = ("-", 0.0), 0.0, []
    for name, ek, er, gm in tensor_errors(ospec, grad, ref):
        if gm == 0.0:
            if ek != 0.0:
                fails.append((name, ek, "the fp64 gradient of this tensor is exactly 0"))
            continue
        bar = factor * er + grad_floor * gm
        r = ek / bar if np.isfinite(ek) else float("inf")
        if r > worst[1]:
            worst = (name, r)
        old = max(old, ek / (factor * er + grad_floor * gmax))
        if not ek <= bar:
            fails.append((name, ek, bar))
    print(f"TRAINER {label}: loss x{loss_ratio:.3f} of its bar | worst tensor {worst[0]} x{worst[1]:.3f} of its bar | "
          f"global-scale rule x{old:.3f} | max |g| {gmax:.3e}")
    assert np.isfinite(loss).all() and np.isfinite(grad).all(), (label, "non-finite kernel output")
    assert not loss_fail, (label, "loss rows", loss_fail)
    assert not fails, (label, fails[:6])
    return worst[0], worst[1], old
