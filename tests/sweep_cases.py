"""The configuration sweep: randomised shapes (fixed seeds) of every flow kind plus hand-picked corners, the per-config case builder,
the prior box of the sampler sweep and the draw-for-draw comparison rule.

Helper module, no tests in it.  tests/test_gpu_random_configs.py holds the density / inverse / gradient assertions over these
configs, tests/test_gpu_sweep_sampler.py the sampler ones, tests/test_cpu_sweep_cases.py the conditions on the reference alone and
on which kernel families the union of the configs reaches.

A config is a tuple: ("maf" | "nsf", D, C, H, T, K, NB, seed) for the two tile engines, (kind, D, C, H, T, K, seed) for the flows
outside them (the lampe backend's autoregressive flows and sbi's one-parameter NSF)."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import flows as OF
from oracle import posterior as OP
from synference_amd.spec import FlowSpec


def _configs():
    rng = np.random.default_rng(2026)
    out = []
    for i in range(28):
        kind = "maf" if i % 2 == 0 else "nsf"
        D = int(rng.integers(1 if kind == "maf" else 2, 17))
        C = int(rng.choice([1, 3, 8, 9, 31, 32, 33, 64, 70, 130]))
        H = int(rng.choice([4, 17, 32, 33, 50, 64, 65, 96, 100, 128]))
        T = int(rng.integers(1, 5))
        K = int(rng.integers(2, 17))
        NB = int(rng.choice([1, 2, 2, 2, 3, 4]))
        out.append((kind, D, C, H, T, K, NB, i))
    # corner cases by hand
    out += [("maf", 16, 512, 128, 1, 10, 2, 100), ("nsf", 16, 257, 128, 1, 16, 1, 101), ("nsf", 2, 1, 1, 3, 2, 2, 102),
            ("maf", 2, 1, 1, 2, 10, 2, 103), ("maf", 9, 20, 8, 2, 10, 2, 104)]
    return out


def _configs_other_kinds():
    """The flows outside the two tile engines: the autoregressive NSF of the lampe backend (csrc/sf_nsfar.hip: hidden rows sorted
    by type and padded, ragged H mod D, one parameter, 16 parameters, K = 2 .. 8) and sbi's one-parameter NSF (csrc/sf_nsf1.hip)."""
    rng = np.random.default_rng(2027)
    out = []
    for i in range(14):
        D = int(rng.integers(1, 17))
        C = int(rng.choice([1, 3, 8, 9, 31, 64, 70]))
        H = int(max(D, rng.choice([4, 17, 32, 33, 50, 64, 100, 128])))
        out.append(("nsf_ar", D, C, H, int(rng.integers(1, 5)), int(rng.integers(2, 9)), 200 + i))
    for i in range(6):
        out.append(("nsf", 1, int(rng.choice([1, 3, 8, 33, 70])), int(rng.choice([4, 17, 50, 64, 128])), int(rng.integers(1, 7)),
                    int(rng.integers(2, 17)), 300 + i))
    out += [("nsf_ar", 16, 64, 128, 1, 8, 400), ("nsf_ar", 2, 1, 2, 3, 2, 401), ("nsf_ar", 3, 5, 192, 1, 8, 402)]
    # zuko.flows.MAF (backend="lampe", model "maf"): the same engine with the affine univariate map
    out += [("maf_ar", 5, 10, 50, 5, 8, 500), ("maf_ar", 1, 3, 16, 2, 8, 501), ("maf_ar", 16, 31, 100, 2, 8, 502), ("maf_ar", 7, 9, 33, 3, 8, 503)]
    return out


def _configs_by_hand():
    """Sampler families neither random draw reaches (tests/test_cpu_sweep_cases.py names a family that the union loses):
    the 32-row MAF sampler with one hidden block; a one-parameter MAF; the 16-row MAF sampler with NB = 1 on the contiguous
    placement, beyond the unrolled kernels' D <= 5; a three-parameter MAF that four hidden blocks send to the 32-row sampler; a
    two-parameter NSF with the three-tile spline head (K > 11), three blocks and a two-part image."""
    return [("maf", 7, 9, 100, 2, 10, 1, 600), ("maf", 1, 4, 8, 2, 10, 2, 601), ("maf", 7, 12, 60, 2, 10, 1, 602),
            ("maf", 3, 5, 40, 2, 10, 4, 603), ("nsf", 2, 33, 64, 2, 14, 3, 604)]


def sweep_configs():
    """Every config of the sampler sweep."""
    return _configs() + _configs_by_hand() + _configs_other_kinds()


# One config per sampler family (by seed, the last field), for the second geometry of the draw-for-draw test: M = 37 rows x S = 7
# draws puts several galaxies and a ragged tail inside every wave.  MAF 32-row: 601 (HT 1, one parameter), 603 (HT 2, NB 4), 4 (HT 3),
# 10 (HT 4, NB 3, image streamed from L2), 600 (HT 4, NB 1); MAF 16-row: 14 (contiguous placement), 18 (aligned, D = 14 in one hidden
# tile), 6 (aligned, D = 3); NSF: 101 (PT 3, NB 1, D = 16, no sampler image), 19 (PT 2, NB 3, D = 16, 4 parts), 3 (PT 3, NB 4), 13 (D = 2,
# NB 2), 604 (D = 2, PT 3, 2 parts); lampe: 206 (the 64-sample kernel at D = 14), 207 (register tiles); 300 (sbi's one-parameter NSF).
_DENSE_WAVE_SEEDS = (601, 603, 4, 10, 600, 14, 18, 6, 101, 19, 3, 13, 604, 206, 207, 300)
DENSE_WAVE_CONFIGS = [c for c in sweep_configs() if c[-1] in _DENSE_WAVE_SEEDS]
assert len(DENSE_WAVE_CONFIGS) == len(_DENSE_WAVE_SEEDS)


def config_id(cfg) -> str:
    return "-".join(str(v) for v in cfg)


Case = namedtuple("Case", "ospec spec flat theta x z st")


def build_case(cfg, B: int | None = None) -> Case:
    """Standardisation ~ N(0, 1) means / U(0.5, 2) widths, the oracle's and the product's spec, the oracle's initial parameters
    perturbed by 0.4 of their mean magnitude, and B rows of theta, x and given noise z (default: 45 rows for the tile engines, 77 --
    two waves of the thread-per-sample kernels, the second ragged -- for the other kinds).  The spec and the parameters do not
    depend on B."""
    tile = len(cfg) == 8
    if tile:
        kind, D, C, H, T, K, NB, seed = cfg
    else:
        kind, D, C, H, T, K, seed = cfg
    rng = np.random.default_rng(seed)
    st = dict(theta_mean=rng.normal(size=D).astype(np.float32), theta_std=rng.uniform(0.5, 2, size=D).astype(np.float32),
              x_mean=rng.normal(size=C).astype(np.float32), x_std=rng.uniform(0.5, 2, size=C).astype(np.float32))
    if tile:
        extra = dict(NB=NB, perms=OF.random_perms(D, T, seed) if kind == "maf" else None)
    else:
        extra = dict(tail_bound=5.0, ar_slope=float(rng.choice([1e-3, 1e-2]))) if kind in ("nsf_ar", "maf_ar") else {}
    ospec = OF.FlowSpec(kind=kind, D=D, C=C, H=H, T=T, K=K, **extra, **{k: v.astype(np.float64) for k, v in st.items()})
    spec = FlowSpec(kind=kind, D=D, C=C, H=H, T=T, K=K, **extra, **st)
    flat = OF.init_params(ospec, seed + 1)
    flat = (flat + 0.4 * rng.normal(size=flat.shape) * np.abs(flat).mean()).astype(np.float32)
    B = B or (45 if tile else 77)
    theta = (rng.normal(size=(B, D)) * st["theta_std"] * 1.2 + st["theta_mean"]).astype(np.float32)
    x = (rng.normal(size=(B, C)) * st["x_std"] + st["x_mean"]).astype(np.float32)
    z = rng.normal(size=(B, D)).astype(np.float32)
    return Case(ospec, spec, flat, theta, x, z, st)


@functools.lru_cache(maxsize=None)
def sweep_case(cfg, B: int | None = None) -> Case:
    """build_case, once per session and read-only."""
    c = build_case(cfg, B)
    for a in (c.flat, c.theta, c.x, c.z):
        a.setflags(write=False)
    return c


def lampe_lds_refused(spec) -> bool:
    """Whether the handle refuses this autoregressive flow at creation: a wave's rows must fit the CU's LDS."""
    if spec.kind not in ("nsf_ar", "maf_ar"):
        return False
    D, C, H = spec.D, spec.C, spec.H
    Hp = sum((len(range(r, H, D)) + 7) // 8 * 8 for r in range(D))
    Hp = (Hp + 15) // 16 * 16
    rows = (D + C + 15) // 16 * 16 + 2 * Hp + 2 * D          # (two hidden buffers; + the head rows of one wave)
    need = max((rows + 32) * 65 * 4, (rows + 24) * 65 * 4 + 4 * Hp * 4)   # density / sampling kernels, training kernel (+ its tables)
    return need > 160 * 1024 - 1024


def flow_or_lds_refusal(spec, device="cuda:0"):
    """The handle of ``spec`` -- or None after the handle refused, by name, a lampe shape whose rows do not fit the LDS."""
    from synference_amd.engine import HipFlow
    if lampe_lds_refused(spec):
        with pytest.raises(RuntimeError, match="LDS"):
            HipFlow(spec, device)
        return None
    return HipFlow(spec, device)


def sweep_tail(D: int) -> float:
    """Per-dimension tail mass of the sweep box: (1 - 0.65^(1/D)) / 2, so that independent dimensions would accept 0.65 at every D
    (the 3 % / 97 % box of test_gpu_parity._draw_for_draw gives 0.94^16 = 0.37 at D = 16)."""
    return (1.0 - 0.65 ** (1.0 / D)) / 2.0


def sweep_box(ospec, flat, x):
    """(lo, hi) float32 [D]: the ``tail`` and ``1 - tail`` quantiles, per dimension, of 400 unbounded fp32-oracle draws per row of x
    (seed 99)."""
    free, _ = OP.sample(ospec, torch.as_tensor(np.array(flat)), np.asarray(x), 400, 99, dtype=torch.float32)
    free = free.reshape(-1, ospec.D)
    assert np.isfinite(free).all()
    tail = sweep_tail(ospec.D)
    return np.quantile(free, tail, axis=0).astype(np.float32), np.quantile(free, 1.0 - tail, axis=0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_box(cfg, M: int):
    """sweep_box of the first M context rows of sweep_case(cfg), once per session."""
    c = sweep_case(cfg)
    lo, hi = sweep_box(c.ospec, c.flat, c.x[:M])
    lo.setflags(write=False)
    hi.setflags(write=False)
    return lo, hi


DRAW_BAR = 1e-4          # of the box width, on every draw


def compare_draws(got, nd, ref, rnd, lo, hi, S: int):
    """The draw-for-draw rule (tests/test_gpu_parity.py::_draw_for_draw): ``got`` [M, S, D] with attempt counts ``nd`` [M] against
    the reference's ``ref``, ``rnd`` under the box (lo, hi).

    All draws finite and inside the box; 1e-4 of the box width on EVERY draw.  The only exemption: a candidate that lands within
    rounding of the box edge can be accepted by one implementation and rejected by the other; that slot then keeps a later attempt
    and the galaxy's attempt count differs -- so a galaxy whose count equals the reference's has no exempt draw at all, and one whose
    count differs may have as many mismatching draws as its count is off (a flip moves the count by at least one).  The counts may
    differ by max(3, 1 %) of the reference's attempts in total, and the box must really have rejected something.

    Returns (largest error over the box width among the galaxies whose counts agree, sum of the count differences)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    nd, rnd = np.asarray(nd).astype(np.int64), np.asarray(rnd).astype(np.int64)
    assert np.isfinite(got).all()
    assert ((got >= lo) & (got <= hi)).all()
    scale = (hi - lo).astype(np.float64)
    err = np.abs((got - ref) / scale).max(-1)
    bad_g = (err > DRAW_BAR).sum(1)
    off_g = np.abs(nd - rnd)
    assert (bad_g <= off_g).all(), (bad_g, off_g, err.max())
    assert off_g.sum() <= max(3, 0.01 * rnd.sum())
    assert (nd >= S).all() and nd.sum() > S * len(nd)  # the box really rejected something
    same = off_g == 0
    return (float(err[same].max()) if same.any() else 0.0), int(off_g.sum())
