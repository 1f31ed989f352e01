"""Named inputs for the conformance tests of csrc/sf_post.hip (tests/test_cpu_post_cases.py holds them to what they claim,
tests/test_gpu_post.py runs the kernels on them).  Helper module, no tests in it.  Each case is the smallest at which the code
path it is named for can still go wrong; every array is built once per session and handed out read-only.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

# The block caps of the grid-stride kernels, restated from csrc/sf_post.hip (tests/test_cpu_post_cases.py greps the source for the
# very lines, so a changed cap fails there instead of silently shrinking a "large" case to one pass):
AB_MAX_BLOCKS = 2048        # sf_flux_to_abmag:   blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);   x 256 threads x 4 floats
ASINH_MAX_BLOCKS = 4096     # sf_flux_to_asinh:   blocks = blocks > 4096 ? 4096 : blocks;                      x 256 threads
SCATTER_MAX_BLOCKS = 8192   # sf_scatter_depths:  blocks = blocks > 8192 ? 8192 : blocks;                      x 256 threads, 4 bands each
CAP_LINES = {"AB": "blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);", "ASINH": "blocks = blocks > 4096 ? 4096 : blocks;",
             "SCATTER": "blocks = blocks > 8192 ? 8192 : blocks;"}
THREADS = 256
SORT_MAX_S = 8192           # sf_quantiles: S > 8192 is refused (the sort lives in LDS)

F32 = np.float32
INF = F32(np.inf)
MODE = 50.0                 # the two modes of the bimodal family sit at +-MODE, sigma 1


def _ro(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---------------------------------------------------------------------------------------------------------------------------
# quantiles
# ---------------------------------------------------------------------------------------------------------------------------
QCase = namedtuple("QCase", "name x q kernels")     # x [N, S, D] float32, q [Q] float32, kernels: subset of ("sort", "large")

Q_BY_COUNT = {
    1: [0.5],
    3: [0.16, 0.5, 0.84],
    5: [0.0, 0.001, 0.5, 0.999, 1.0],
    9: [0.0, 0.001, 0.0275, 0.16, 0.5, 0.84, 0.9725, 0.999, 1.0],       # crosses the 8-rank batches of the large kernel
    256: list(np.linspace(0.0, 1.0, 256)),                               # ... and fills the 256-thread output loop of both
}
# (S, N, D, Q): every S of the list, every D in {1, 3, 16}, N in {1, 5} and Q in {1, 3, 5, 9, 256} at least once
SIZES_SORT = [(1, 1, 1, 5), (2, 5, 3, 3), (3, 1, 16, 9), (255, 5, 1, 1), (256, 1, 3, 256), (257, 5, 16, 5), (1023, 1, 1, 9),
              (1025, 5, 3, 1), (4097, 1, 16, 3), (8191, 5, 1, 256), (8192, 1, 3, 5)]
SIZES_LARGE_ONLY = [(8193, 5, 3, 9), (70000, 1, 3, 9), (70000, 1, 16, 256)]
FAMILY_S = (257, 4097, 8192)                                             # odd, more than one pass of 256 threads, the LDS limit
BIMODAL_S = (1023, 4097, 8191, 8192)
INT_S = (257, 1025, 4097)                                                # S - 1 a power of two: q = k / (S - 1) is exact in fp32
Q3 = [0.16, 0.5, 0.84]


def _q(vals):
    return np.asarray(vals, dtype=np.float64).astype(F32)


def _pos_lo(n, q32):
    return int(np.floor((n - 1) * float(F32(q32))))


def bimodal_columns(S, q):
    """[S, 3 len(q)]: column 3 j + k has lo + k draws ~ N(-MODE, 1) and the rest ~ N(+MODE, 1), lo = floor((S - 1) q_j): with
    k = 1 the two order statistics around quantile q_j are the top of the low mode and the bottom of the high one (the value lies
    in the gap and the position error is multiplied by it), with k = 0 / 2 the split is one rank to either side."""
    rng = np.random.default_rng(S)
    cols = []
    for qq in _q(q):
        lo = _pos_lo(S, qq)
        for k in (0, 1, 2):
            n_low = min(max(lo + k, 0), S)
            col = np.concatenate([rng.normal(-MODE, 1.0, n_low), rng.normal(MODE, 1.0, S - n_low)])
            cols.append(rng.permutation(col))
    return np.stack(cols, 1).astype(F32)


def _family(name, S):
    """x [N, S, D] of one value family."""
    rng = np.random.default_rng([S, sum(map(ord, name))])
    if name == "cauchy":
        return rng.standard_cauchy(size=(2, S, 3)).astype(F32)
    if name == "all_equal":
        return np.broadcast_to(np.array([3.25, -1e-30, 0.0], F32), (1, S, 3)).copy()
    if name == "two_values":
        return np.where(rng.uniform(size=(2, S, 3)) < 0.3, F32(-2.5), F32(7.0)).astype(F32)
    if name == "low_byte":            # equal but for the lowest mantissa byte: the last radix pass, and a sort that compares all 32 bits
        return (np.uint32(0x3F800000) + rng.integers(0, 256, size=(1, S, 3)).astype(np.uint32)).view(F32)
    if name == "signs_zero_denormal":
        pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.17549435e-38, -1.17549435e-38, 1.0, -1.0, 3e38, -3e38], F32)
        return pool[rng.integers(0, len(pool), size=(1, S, 3))]
    if name == "leading_nan":         # n differs per column of one launch: k leading NaN, k in {0, 1, S - 1, S}
        x = rng.normal(size=(2, S, 4)).astype(F32)
        for d, k in enumerate((0, 1, S - 1, S)):
            x[:, :k, d] = np.nan
        return x
    if name == "inf":
        # columns: +inf at the top; -inf at the bottom; both ends; every draw +inf; every draw -inf; -inf and +inf only;
        # one +inf and NaN besides (n counts the +inf); a single +inf among finite draws
        x = rng.normal(size=(1, S, 8)).astype(F32)
        m = max(1, S // 50)
        x[0, :m, 0] = INF
        x[0, :m, 1] = -INF
        x[0, :m, 2], x[0, m:2 * m, 2] = INF, -INF
        x[0, :, 3], x[0, :, 4] = INF, -INF
        x[0, :, 5] = np.where(np.arange(S) % 3 == 0, -INF, INF)
        x[0, ::2, 6] = np.nan
        x[0, 1, 6] = INF
        x[0, S // 2, 7] = INF
        for d in range(8):
            x[0, :, d] = rng.permutation(x[0, :, d])
        return x
    raise KeyError(name)


FAMILIES = ("cauchy", "all_equal", "two_values", "low_byte", "signs_zero_denormal", "leading_nan", "inf")


@functools.lru_cache(maxsize=None)
def quantile_cases():
    out = []
    for S, N, D, Q in SIZES_SORT + SIZES_LARGE_ONLY:
        x = np.random.default_rng([S, N, D]).normal(size=(N, S, D)).astype(F32)
        kernels = ("sort", "large") if S <= SORT_MAX_S else ("large",)
        out.append(QCase(f"gauss_S{S}_N{N}_D{D}_Q{Q}", x, _q(Q_BY_COUNT[Q]), kernels))
    for S in BIMODAL_S:
        out.append(QCase(f"bimodal_S{S}", bimodal_columns(S, Q3)[None], _q(Q3), ("sort", "large")))
    for fam in FAMILIES:
        for S in FAMILY_S:
            out.append(QCase(f"{fam}_S{S}", _family(fam, S), _q([0.0, 0.001, 0.16, 0.5, 0.84, 0.999, 1.0]), ("sort", "large")))
    for S in INT_S:
        # exact integer positions: the Gaussian row, and the +-inf columns beside which 0 * inf would be NaN
        m = max(1, S // 50)                                                # the +-inf columns hold m infinite draws at an end
        ks = np.array([0, 1, m - 1, m, (S - 1) // 4, (S - 1) // 2, S - 1 - m, S - 3, S - 2, S - 1], np.float64)
        x = np.concatenate([np.random.default_rng(S).normal(size=(1, S, 3)).astype(F32), _family("inf", S)[:, :, :3]], 2)
        out.append(QCase(f"integer_S{S}", x, _q(ks / (S - 1)), ("sort", "large")))
    for c in out:
        _ro(c.x, c.q)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def quantile_case(name):
    return next(c for c in quantile_cases() if c.name == name)


SORT_NAMES = [c.name for c in quantile_cases() if "sort" in c.kernels]
LARGE_NAMES = [c.name for c in quantile_cases() if "large" in c.kernels]


# ---------------------------------------------------------------------------------------------------------------------------
# PIT
# ---------------------------------------------------------------------------------------------------------------------------
PIT_S = (1, 63, 64, 65, 300)                     # one wave reads 64 draws per trip
PIT_ND = ((1, 1), (1, 3), (3, 3), (37, 4))       # N D = 1, 3, 9, 148: the last 256-thread block holds 1, 3, 1 or 4 waves
TRUTH_KINDS = ("equal_to_a_draw", "below_all", "above_all", "plus_inf", "minus_inf", "nan", "ordinary")
DRAW_KINDS = ("plain", "some_nan", "all_nan", "some_inf", "all_plus_inf", "all_minus_inf", "nan_and_inf")


def pit_kinds(S, N, D):
    """(truth kind, draw kind) index of every (row, dim): the truth kind cycles, the draw kind moves on once per cycle, so that all
    49 pairs turn up over the 148 columns of the largest case; the offset S makes the one-column cases differ from each other."""
    w = np.arange(N * D) + S
    return (w % len(TRUTH_KINDS)).reshape(N, D), ((w // len(TRUTH_KINDS)) % len(DRAW_KINDS)).reshape(N, D)


@functools.lru_cache(maxsize=None)
def pit_case(S, N, D):
    """(s [N, S, D], t [N, D]) float32.  Draws on a grid of 1/8 (ties among the draws; equality with the truth is exact)."""
    rng = np.random.default_rng([S, N, D])
    s = (np.round(rng.normal(size=(N, S, D)) * 8) / 8).astype(F32)
    t = (np.round(rng.normal(size=(N, D)) * 8) / 8 + 1 / 16).astype(F32)          # ordinary: between grid points
    tk, dk = pit_kinds(S, N, D)
    for g in range(N):
        for d in range(D):
            col, kind = s[g, :, d], DRAW_KINDS[dk[g, d]]
            if kind in ("some_nan", "nan_and_inf"):
                col[rng.uniform(size=S) < 0.3] = np.nan
            if kind in ("some_inf", "nan_and_inf"):
                r = rng.uniform(size=S)
                col[r < 0.15], col[r > 0.85] = -INF, INF
            if kind == "all_nan":
                col[:] = np.nan
            if kind == "all_plus_inf":
                col[:] = INF
            if kind == "all_minus_inf":
                col[:] = -INF
            fin = col[np.isfinite(col)]
            lo, hi = (fin.min(), fin.max()) if fin.size else (F32(0), F32(0))
            t[g, d] = {"equal_to_a_draw": fin[len(fin) // 2] if fin.size else F32(0), "below_all": lo - 1, "above_all": hi + 1,
                       "plus_inf": INF, "minus_inf": -INF, "nan": np.nan, "ordinary": t[g, d]}[TRUTH_KINDS[tk[g, d]]]
    return _ro(s, t)


PIT_CASES = [(S, N, D) for S in PIT_S for N, D in PIT_ND]


# ---------------------------------------------------------------------------------------------------------------------------
# AB magnitudes
# ---------------------------------------------------------------------------------------------------------------------------
AB_N = (1, 2, 3, 4, 5, 7, 1023, 1025)            # every n % 4 tail, fewer than four elements, more than one block
AB_LIMITS = (30.0, 50.0, 99.0)
AB_BIG_N = AB_MAX_BLOCKS * THREADS * 4 + 3       # the grid-stride loop runs a second time and ends in the scalar tail


def ab_boundary(lim):
    """(f_in, f_out) float32 neighbours: f_in is the smallest positive flux whose fp64 magnitude is still <= lim."""
    f = F32(1000.0 * 10.0 ** ((23.9 - lim) / 2.5))
    mag = lambda v: -2.5 * np.log10(np.float64(v) / 1000.0) + 23.9
    while mag(f) <= lim:
        f = np.nextafter(f, F32(0))
    while mag(f) > lim:
        f = np.nextafter(f, INF)
    return f, np.nextafter(f, F32(0))


def ab_specials(lim):
    f_in, f_out = ab_boundary(lim)
    return np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-40, -5.0, f_in, f_out, 1e-30, 3e38, 1.17549435e-38], F32)


@functools.lru_cache(maxsize=None)
def ab_case(n, lim, with_err):
    """(flux [n], err [n] or None) float32: log-uniform fluxes over 1e-3 .. 1e5 nJy with the special values written over the first
    elements (rotated by n, so that the short cases see different ones) and, in the long cases, over the last ones too (the tail)."""
    rng = np.random.default_rng([n, int(lim)])
    f = (10 ** rng.uniform(-3, 5, size=n)).astype(F32)
    sp = np.roll(ab_specials(lim), n)
    k = min(n, len(sp))
    f[:k] = sp[:k]
    if n > 2 * len(sp):
        f[-len(sp):] = sp
    e = (0.1 * np.abs(np.where(np.isfinite(f), f, 1.0)) + 1).astype(F32) if with_err else None
    return _ro(f, e)


AB_CASES = [(n, AB_LIMITS[i % 3], bool(i % 2)) for i, n in enumerate(AB_N)] + [(1025, 30.0, True), (1023, 99.0, False),
                                                                               (AB_BIG_N, 50.0, True)]


# ---------------------------------------------------------------------------------------------------------------------------
# asinh magnitudes
# ---------------------------------------------------------------------------------------------------------------------------
ASINH_C = (1, 3, 7, 9)
# The second trip of the grid-stride loop starts at element 4096 * 256, which is no multiple of 7: i % C must be taken of the element
# index, not of the trip's offset.  4096 * 256 + 5 elements with C = 7 is not a whole number of rows; the next whole number is taken
# (149798 rows = 4096 * 256 + 10 elements).
ASINH_BIG = (-(-(ASINH_MAX_BLOCKS * THREADS + 5) // 7), 7)


@functools.lru_cache(maxsize=None)
def asinh_case(N, C):
    """(flux [N, C], f_b [C], err [N, C]) float32: |f / 2 f_b| log-uniform over 1e-8 .. 1e8 in both signs; row 0 holds f = 0 and the
    ends of the range in both signs."""
    rng = np.random.default_rng([N, C])
    fb = (10 ** rng.uniform(0, 2, size=C)).astype(F32)
    r = 10 ** rng.uniform(-8, 8, size=(N, C)) * rng.choice([-1.0, 1.0], size=(N, C))
    ends = np.array([0.0, 1e-8, -1e-8, 1e8, -1e8, 1.0, -1.0], np.float64)
    r.reshape(-1)[:min(len(ends), r.size)] = ends[:min(len(ends), r.size)]
    if r.size > 2 * len(ends):
        r.reshape(-1)[-len(ends):] = ends
    f = (r * 2 * fb.astype(np.float64)).astype(F32)
    e = (0.1 * np.abs(f) + 1).astype(F32)
    return _ro(f, fb, e)


ASINH_CASES = [(64, C) for C in ASINH_C] + [(1, 1), ASINH_BIG]


# ---------------------------------------------------------------------------------------------------------------------------
# depth scatter
# ---------------------------------------------------------------------------------------------------------------------------
SCATTER_C = (1, 3, 4, 5, 17)
# (N, C, n_scatters, sigma rows, min_flux_pc_error): 0.01 % leaves the depth as sigma everywhere, 60 % makes |f| win nearly everywhere
SCATTER_CASES = [(33, C, ns, rows, pc) for C in SCATTER_C for ns, rows in ((1, 1), (3, 1), (3, 3)) for pc in (0.01, 60.0)]
# N n_scatters ceil(C / 4) = 349600 * 3 * 2 work items > 8192 * 256: output row 8192 * 256 / 2 is the first of the second trip
SCATTER_BIG = (349600, 5, 3, 3, 1.5)
SCATTER_BIG_BOUNDARY_ROW = SCATTER_MAX_BLOCKS * THREADS // 2


@functools.lru_cache(maxsize=None)
def scatter_case(N, C, n_scatters, sigma_rows, pc):
    """(flux [N, C], sigma [sigma_rows, C]) float32; a third of the fluxes negative."""
    rng = np.random.default_rng([N, C, n_scatters, sigma_rows])
    f = rng.uniform(-100, 200, size=(N, C)).astype(F32)
    sigma = rng.uniform(0.2, 6.0, size=(sigma_rows, C)).astype(F32)
    return _ro(f, sigma)


def scatter_big_rows():
    """Output rows checked in the big case: either side of the grid-stride boundary, the first and the last rows."""
    N, C, ns, _, _ = SCATTER_BIG
    b, last = SCATTER_BIG_BOUNDARY_ROW, N * ns
    return np.concatenate([np.arange(0, 64), np.arange(b - 100, b + 100), np.arange(last - 100, last)])
