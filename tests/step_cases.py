"""Cases of the training-step conformance tests (tests/test_gpu_step.py; conditions held by tests/test_cpu_step_cases.py).  Helper
module, no tests in it.

Optimiser cases: (n, which buffer starts one float into a larger allocation, hyper-parameters, step, clip regime).  n and the
alignment select the kernel as sf_launch_adam does (``path_of`` restates its rule):

  fused_vec          k_adam_fused, float4 branch with the has_own prefetch: n % 4 == 0, n <= 131072, everything 16-byte aligned
  fused_scalar       k_adam_fused, scalar branch: n % 4 != 0
  fused_scalar_align k_adam_fused, scalar branch because p, m or v is not 16-byte aligned
  two_kernel         k_sqnorm (one share of |g|^2 per block) + k_adam: n > 131072; 300007 > 256 x 1024, so the strided loops run
  two_kernel_align   the same path at a small n because the gradient is not 16-byte aligned

Every input is seeded.  A case at step t > 1 gets m and v from the fp64 model run min(t - 1, 8) times on seeded gradients
(step_model.warm_state); a fifth of the parameters start at exactly 0, so that there p_new = -update and the update itself is compared.

Epoch cases: names of tests/cases.py with a batch size, one per gather family of sf_train_loss_grad.
"""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import numpy as np

import step_model as SM
from cases import make_case

FUSED_MAX = 131072                 # sf_launch_adam: n <= 131072 -> k_adam_fused
STRIDED_ABOVE = 256 * 1024         # sf_launch_adam: at most 256 blocks of (256 threads x 4) / k_adam_fused: 4096 per block

HYPERS = {
    "adam": SM.Desc(1e-3, 0.9, 0.999, 1e-8, 0.0, 0),
    "adam_l2": SM.Desc(1e-3, 0.9, 0.999, 1e-8, 0.01, 0),       # weight_decay != 0 && !decoupled: gi += wd * pi
    "adamw": SM.Desc(1e-3, 0.9, 0.999, 1e-8, 0.01, 1),         # what train_flow(optimizer_choice="AdamW") builds
    "betas": SM.Desc(3e-3, 0.8, 0.99, 1e-6, 0.0, 0),
}
STEPS = (1, 2, 1000)
# clip regime -> gradient kind.  active: |g| = 2 max_norm; inactive: |g| = max_norm / 4; off0 / off_neg: max_norm 0 / -1; zero: an
# all-zero gradient under max_norm 1 (coef = min(1 / 1e-6, 1)); sparse: a tenth of the entries exactly 0, a tenth at 1e-12, clip active
REGIMES = {"active": "dense", "inactive": "dense", "off0": "dense", "off_neg": "dense", "zero": "zero", "sparse": "sparse"}
ACTIVE_RATIO, INACTIVE_RATIO = 2.0, 0.25        # |g| / max_norm; the table asks for >= 1.5 and <= 0.5

# path -> [(n, offset buffer)]
PATH_SHAPES = {
    "fused_vec": [(4, None), (4096, None), (4100, None), (131072, None)],
    "fused_scalar": [(1, None), (3, None), (63, None), (4097, None), (10007, None), (131071, None)],
    "fused_scalar_align": [(4096, "p"), (4096, "m"), (4096, "v")],
    "two_kernel": [(131073, None), (131076, None), (300007, None)],
    "two_kernel_align": [(4096, "g")],
}
_ORDER = ["active", "inactive", "off0", "off_neg", "zero", "sparse", "active", "inactive"]

OptCase = namedtuple("OptCase", "name path n offset hyper step regime scale")


def path_of(n: int, offset) -> str:
    """The kernel sf_launch_adam picks (csrc/sf_train.hip)."""
    if n <= FUSED_MAX and offset != "g":
        if offset in ("p", "m", "v"):
            return "fused_scalar_align"
        return "fused_vec" if n % 4 == 0 else "fused_scalar"
    return "two_kernel_align" if n <= FUSED_MAX else "two_kernel"


def _table():
    out = []
    hy = list(HYPERS)
    for k, (path, shapes) in enumerate(PATH_SHAPES.items()):
        for i, regime in enumerate(_ORDER):
            n, off = shapes[i % len(shapes)]
            if regime == "sparse" and n < 20:      # a tenth of the entries must be at least one
                n, off = shapes[(i + 1) % len(shapes)]
            hyper, step = hy[(i + k) % len(hy)], STEPS[(i + k) % len(STEPS)]
            # the two gradient magnitudes of test_adam_step_matches_torch; under L2 the large one only (opt_inputs)
            scale = 3.0 if hyper == "adam_l2" else (3.0, 0.01)[i % 2]
            name = f"{path}-n{n}{'-off_' + off if off else ''}-{hyper}-t{step}-{regime}"
            out.append(OptCase(name, path, n, off, hyper, step, regime, scale))
    return out


OPT_CASES = _table()
OPT_BY_NAME = {c.name: c for c in OPT_CASES}
# one fused and one two-kernel case for the handle-against-caller-state test
HANDLE_CASES = [(4100, "adam_l2", 0.7), (131076, "adamw", 50.0)]

OptInputs = namedtuple("OptInputs", "case desc p g m v max_norm")


def _seed(name: str) -> int:
    return zlib.crc32(name.encode())


def dense_gradient(n: int, scale: float, seed: int, floor: float = 0.0) -> np.ndarray:
    """scale * N(0, 1); with ``floor``, scale * +-(floor + |N(0, 1)|): no entry near zero."""
    z = np.random.default_rng(seed).normal(size=n)
    return (scale * (np.sign(z) * (floor + np.abs(z)) if floor else z)).astype(np.float32)


def start_params(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    p = rng.normal(size=n).astype(np.float32)
    p[rng.random(n) < 0.2] = 0.0
    return p


@functools.lru_cache(maxsize=4)
def opt_inputs(name: str) -> OptInputs:
    c = OPT_BY_NAME[name]
    seed = _seed(name)
    desc = HYPERS[c.hyper]
    p = start_params(c.n, seed)
    # Under L2 the gradient is kept away from -weight_decay * p: where the two cancel, g_eff -- the unit of m and v -- is small against
    # the roundings of its addends and NO fp32 evaluation is within 2e-6 of a unit (at n = 300007 some twenty elements of N(0, 3^2)
    # draws are not).  |g| >= 0.3 against |weight_decay * p| <= 0.05: opposite signs still meet, cancelling a sixth at the most.
    g = dense_gradient(c.n, c.scale, seed + 1, floor=0.1 if c.hyper == "adam_l2" else 0.0)
    kind = REGIMES[c.regime]
    if kind == "zero":
        g[:] = 0.0
    elif kind == "sparse":
        perm = np.random.default_rng(seed + 2).permutation(c.n)
        k = max(1, c.n // 10)
        g[perm[:k]] = 0.0
        g[perm[k:2 * k]] = 1e-12
    norm = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
    assert np.isfinite(np.float32((g.astype(np.float64) ** 2).sum()))      # the sum of squares stays finite in float32
    max_norm = {"active": norm / ACTIVE_RATIO, "sparse": norm / ACTIVE_RATIO, "inactive": norm / INACTIVE_RATIO,
                "off0": 0.0, "off_neg": -1.0, "zero": 1.0}[c.regime]
    max_norm = float(np.float32(max_norm))                                  # (the ABI takes a float)
    m, v = SM.warm_state(p, desc, c.step, seed + 3, c.scale)
    for a in (p, g, m, v):
        a.setflags(write=False)
    return OptInputs(c, desc, p, g, m, v, max_norm)


@functools.lru_cache(maxsize=4)
def opt_reference(name: str) -> SM.Reference:
    i = opt_inputs(name)
    return SM.reference(i.p, i.g, i.m, i.v, i.case.step, i.desc, i.max_norm)


# ---------------------------------------------------------------------------------------------------------------------------
# the fused epoch
# ---------------------------------------------------------------------------------------------------------------------------
EpochCase = namedtuple("EpochCase", "name batch family")
EPOCH_CASES = [
    EpochCase("maf_cfg1", 64, "cooperative MAF"),
    EpochCase("maf_t8", 96, "cooperative MAF, T = 8 stash"),
    EpochCase("maf_cli", 64, "cooperative MAF"),
    EpochCase("nsf_cfg3", 64, "cooperative NSF, one chunk per workgroup"),
    # 513 row tiles: one past one chunk per workgroup on a 256-CU part (sf_nsfc_grid caps at 512) -> sf_nsfc_acc_mode = 2
    EpochCase("nsf_cfg3", 16416, "cooperative NSF, f32 atomic replicas summed by k_gather_c2"),
    EpochCase("nsf_h69", 64, "cooperative NSF, five-wave kernel"),
    EpochCase("maf_wide", 64, "32-row kernels"),
    EpochCase("maf_wide", 600, "32-row kernels, f32 atomic replicas"),
    EpochCase("nsf_d1", 64, "one-parameter NSF"),
    EpochCase("nsfar_small", 64, "lampe flow"),
    EpochCase("mafar_small", 64, "lampe flow"),
]
LAMPE = ("nsfar_small", "mafar_small")
THREE_BATCH = ["maf_cfg1", "nsf_cfg3", "maf_wide", "nsf_d1"]       # bit for bit
THREE_BATCH_LAMPE = "nsfar_small"                                   # to the suite's lampe bar
EPOCH_DESC = SM.Desc(1e-3, 0.9, 0.999, 1e-8, 0.01, 1)               # AdamW 0.01
EPOCH_RUNS = [(0, 0.5), (5, 0.5), (0, 0.0)]                         # (step0, max_norm); state warmed where step0 > 0
LOSS_SUM_START = 123.5
LOSS_PER_ROW = 1e-6                # the loss parts are added on a 2^-20 grid: at most 2^-21 = 4.8e-7 per row
GRAD_NOISE = 1e-5                  # x max(1, max |g|): test_large_batch_gradient_path_matches_autograd, accumulation-order noise
LAMPE_NOISE = 2e-6                 # x max |g|: test_lampe_gradient_partials_and_atomics_agree

EpochInputs = namedtuple("EpochInputs", "spec flat theta x order")


def reproducible(case: EpochCase) -> bool:
    """Whether the gradient of the case is the same bits call after call: per-tile replicas summed in a fixed order up to batch 512,
    f32 atomics above; the lampe flows add hidden deltas in LDS in the hardware's order."""
    return case.batch <= 512 and case.name not in LAMPE


@functools.lru_cache(maxsize=4)
def epoch_inputs(name: str, batch: int, n_batches: int = 1) -> EpochInputs:
    """Training arrays of 1.5 x batch rows and ``order``: a seeded choice of n_batches x batch of them, some rows repeated."""
    rows = batch + batch // 2
    _, spec, flat, theta, x = make_case(name, B=rows)
    order = np.random.default_rng(_seed(f"{name}-{batch}")).integers(0, rows, size=n_batches * batch).astype(np.int64)
    for a in (flat, theta, x, order):
        a.setflags(write=False)
    return EpochInputs(spec, flat, theta, x, order)


def epoch_warm_state(flat, step0: int):
    """float32 (m, v) before step step0 + 1."""
    return SM.warm_state(flat, EPOCH_DESC, step0 + 1, _seed("epoch") + step0, 0.05)
