"""What keeps tests/test_gpu_post.py from passing vacuously, checked on the reference alone (no GPU).

* the model's quantiles are numpy's on every case without +-inf, its PIT ranks the reference's np.mean(s < y);
* the cases reach what they are named for: the bimodal quantile lies in the gap, the integer positions are integers, the AB boundary
  pair straddles the limit, the large cases need a second grid pass;
* the defects the device code once had, planted in the model, fail the GPU test's own comparison functions -- and only on the cases
  that were built for them;
* the fp32 evaluation of the magnitude formulas is far inside the floors of the bar 4 x e_ref + floor;
* the host-side refusals of the ABI and of the Python wrappers, on the loaded library without a device.
"""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import post_cases as PC
import post_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB_FLOOR, ASINH_FLOOR = 2e-5, 5e-5          # the bars of test_flux_to_abmag_matches_reference_formula / test_flux_to_asinh_matches_oracle


def _has_inf(x):
    return bool(np.isinf(x).any())


# ---- the model against numpy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in PC.quantile_cases() if not _has_inf(c.x)])
def test_model_quantiles_are_numpys(name):
    """4 fp64 ulp, taken at the larger of the two knots: numpy's lerp (a + t (b - a), or b - (b - a)(1 - t) from t = 0.5 on) and the
    rule's v[lo] + f (v[hi] - v[lo]) round differently, each by about an ulp of the knots, not of a result that may be near zero."""
    c = PC.quantile_case(name)
    det = PM.quantiles_detail(c.x, c.q)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        want = np.nanquantile(c.x.astype(np.float64), c.q.astype(np.float64), axis=1, method="linear").transpose(1, 2, 0)
    assert np.array_equal(np.isnan(det.value), np.isnan(want))
    ok = ~np.isnan(want)
    bar = 4 * np.spacing(np.maximum(np.abs(det.vlo[ok]), np.abs(det.vhi[ok])))
    assert (np.abs(det.value[ok] - want[ok]) <= bar).all()
    assert np.array_equal(det.n, (~np.isnan(c.x)).sum(1))


def test_model_quantiles_on_infinite_draws():
    x = np.array([-np.inf, 1.0, 2.0, 3.0, np.inf, np.nan], np.float32).reshape(1, 6, 1)      # n = 5
    v = PM.quantiles(x, [0.0, 0.125, 0.25, 0.5, 0.75, 0.875, 1.0])[0, 0]
    # above a -inf knot the expression is -inf + f * (+inf): inf - inf, NaN; below a +inf knot it is finite + f * inf = +inf
    assert np.array_equal(v, [-np.inf, np.nan, 1.0, 2.0, 3.0, np.inf, np.inf], equal_nan=True)
    both = np.array([-np.inf, np.inf], np.float32).reshape(1, 2, 1)
    v = PM.quantiles(both, [0.0, 0.5, 1.0])[0, 0]
    assert v[0] == -np.inf and np.isnan(v[1]) and v[2] == np.inf                              # inf - inf is the only NaN
    assert np.isnan(PM.quantiles(np.full((1, 4, 1), np.nan, np.float32), [0.5])).all()


@pytest.mark.parametrize("shape", [(1, 1, 1), (65, 3, 3), (300, 37, 4)])
def test_model_pit_is_the_reference_definition(shape):
    S, N, D = shape
    s = np.random.default_rng(S).normal(size=(N, S, D)).astype(np.float32)
    y = np.random.default_rng(S + 1).normal(size=(N, D)).astype(np.float32)
    want = np.array([np.mean(s[i] < y[i], axis=0) for i in range(N)])                         # sbi_runner.py:7153-7158
    assert np.array_equal(PM.pit_ranks(s, y), want)
    from oracle import features as OF
    assert np.array_equal(OF.pit_ranks(s, y), want)


@pytest.mark.parametrize("case", PC.PIT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_oracle_pit_is_the_model_and_stays_in_the_unit_interval(case):
    from oracle import features as OF
    s, t = PC.pit_case(*case)
    a, b = OF.pit_ranks(s, t), PM.pit_ranks(s, t)
    assert np.array_equal(a, b, equal_nan=True)
    assert ((b[~np.isnan(b)] >= 0) & (b[~np.isnan(b)] <= 1)).all()


# ---- the cases reach what they claim ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", PC.BIMODAL_S)
def test_bimodal_quantiles_lie_in_the_gap(S):
    c = PC.quantile_case(f"bimodal_S{S}")
    det = PM.quantiles_detail(c.x, c.q)
    for j in range(len(c.q)):
        mid = 3 * j + 1                                                    # the column split AT quantile j
        assert det.vlo[0, mid, j] < -PC.MODE + 6 and det.vhi[0, mid, j] > PC.MODE - 6
        if det.f[0, mid, j] > 0:
            assert abs(det.value[0, mid, j]) < PC.MODE - 6
        assert det.vhi[0, mid - 1, j] - det.vlo[0, mid - 1, j] < 6          # one rank to either side: both knots in one mode
        assert det.vhi[0, mid + 1, j] - det.vlo[0, mid + 1, j] < 6
        assert det.vlo[0, mid - 1, j] > 0 > det.vhi[0, mid + 1, j]
    # at least one quantile of the case has a fraction away from 0: the position error has something to multiply
    assert (np.minimum(det.f[0, 1::3], 1 - det.f[0, 1::3]).max() > 0.05)


@pytest.mark.parametrize("S", PC.INT_S)
def test_integer_positions_are_integers(S):
    c = PC.quantile_case(f"integer_S{S}")
    pos = (S - 1) * c.q.astype(np.float64)
    assert np.array_equal(pos, np.round(pos)) and len(set(pos)) == len(pos) and pos.max() == S - 1
    det = PM.quantiles_detail(c.x, c.q)
    gauss = det.f[0, 0]
    assert (gauss == 0).all()
    # ... and some of them sit beside an infinite draw (where v[lo] + 0 * inf would be NaN)
    assert (np.isfinite(det.vlo) & np.isinf(det.vhi) & (det.f == 0)).any()
    assert (np.isinf(det.vlo) & (det.f == 0)).any()


def test_case_lists_cover_the_shapes():
    cs = PC.quantile_cases()
    gauss = [c for c in cs if c.name.startswith("gauss")]
    assert {c.x.shape[1] for c in gauss if "sort" in c.kernels} == {1, 2, 3, 255, 256, 257, 1023, 1025, 4097, 8191, 8192}
    assert {c.x.shape[1] for c in gauss if c.kernels == ("large",)} == {8193, 70000}
    assert {c.x.shape[2] for c in gauss} == {1, 3, 16} and {c.x.shape[0] for c in gauss} == {1, 5}
    assert {len(c.q) for c in gauss} == {1, 3, 5, 9, 256}
    assert all(c.x.dtype == np.float32 and c.q.dtype == np.float32 for c in cs)
    for S in PC.FAMILY_S:
        x = PC.quantile_case(f"leading_nan_S{S}").x
        assert [int(np.isnan(x[0, :, d]).sum()) for d in range(4)] == [0, 1, S - 1, S]
        x = PC.quantile_case(f"low_byte_S{S}").x
        assert len(np.unique(x.view(np.uint32) >> 8)) == 1 and len(np.unique(x)) > 100
        x = PC.quantile_case(f"signs_zero_denormal_S{S}").x
        assert (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any() and ((x != 0) & (np.abs(x) < 1e-38)).any()
    tk = {(int(a), int(b)) for a, b in zip(*map(np.ravel, PC.pit_kinds(300, 37, 4)))}
    assert len(tk) == len(PC.TRUTH_KINDS) * len(PC.DRAW_KINDS)            # every truth kind meets every draw kind
    s, t = PC.pit_case(300, 37, 4)
    assert (s == t[:, None, :]).any()                                        # a truth equal to a draw: the strict <


@pytest.mark.parametrize("lim", PC.AB_LIMITS)
def test_ab_boundary_pair_straddles_the_limit(lim):
    f_in, f_out = PC.ab_boundary(lim)
    mag = lambda v: -2.5 * np.log10(np.float64(v) / 1000.0) + 23.9
    assert f_in.dtype == np.float32 and f_out == np.nextafter(f_in, np.float32(0)) and f_out > 0
    assert mag(f_in) <= lim < mag(f_out)
    assert PM.abmag(np.array([f_in, f_out]), None, lim)[1] == lim
    for n, l, _ in PC.AB_CASES:
        if n >= 1023 and l == lim:
            assert f_in in PC.ab_case(n, l, False)[0] and f_out in PC.ab_case(n, l, False)[0]


def test_large_cases_need_a_second_grid_pass():
    src = open(os.path.join(ROOT, "synference_amd", "csrc", "sf_post.hip")).read()
    for line in PC.CAP_LINES.values():
        assert src.count(line) == 1, line                                   # the caps next to the cases restate the source
    one_pass = PC.AB_MAX_BLOCKS * PC.THREADS * 4
    assert one_pass < PC.AB_BIG_N < 2 * one_pass and PC.AB_BIG_N % 4 == 3
    assert any(n == PC.AB_BIG_N for n, _, _ in PC.AB_CASES)
    N, Cb = PC.ASINH_BIG
    one_pass = PC.ASINH_MAX_BLOCKS * PC.THREADS
    assert N * Cb >= one_pass + 5 and one_pass % Cb != 0 and PC.ASINH_BIG in PC.ASINH_CASES
    N, Cb, ns, _, _ = PC.SCATTER_BIG
    items, one_pass = N * ns * ((Cb + 3) // 4), PC.SCATTER_MAX_BLOCKS * PC.THREADS
    rows = PC.scatter_big_rows()
    b = PC.SCATTER_BIG_BOUNDARY_ROW
    assert items > one_pass and b * ((Cb + 3) // 4) == one_pass
    assert {b - 1, b, N * ns - 1, 0} <= set(rows.tolist()) and rows.max() == N * ns - 1 and len(rows) < 500
    assert {c[1] for c in PC.SCATTER_CASES} == {1, 3, 4, 5, 17}


def test_scatter_cases_reach_both_sides_of_the_max():
    for case in PC.SCATTER_CASES:
        f, sigma = PC.scatter_case(*case[:4], case[4])
        _, s = PM.scatter_depths(f, sigma, case[2], case[4], 1)
        depth_wins = s == sigma[(np.arange(len(s)) % case[2]) % len(sigma)]
        if case[4] < 1:
            assert depth_wins.all()
        else:
            assert depth_wins.mean() < 0.1
        assert (f < 0).any() or f.size < 4


def test_scatter_rows_are_the_full_run():
    f, sigma = PC.scatter_case(33, 5, 3, 3, 60.0)
    full = PM.scatter_depths(f, sigma, 3, 60.0, 9)
    rows = np.array([0, 5, 98, 31, 32])
    part = PM.scatter_depths(f, sigma, 3, 60.0, 9, rows=rows)
    assert np.array_equal(part[0], full[0][rows]) and np.array_equal(part[1], full[1][rows])


# ---- planted defects ------------------------------------------------------------------------------------------------------------
def _rejected(label, got, det):
    with pytest.raises(AssertionError) as e:
        PM.check_quantiles(label, got.astype(np.float32), det)
    return str(e.value)


def test_fp32_position_fails_the_bimodal_case():
    c = PC.quantile_case("bimodal_S8192")
    det = PM.quantiles_detail(c.x, c.q)
    bad = PM.quantiles(c.x, c.q, position_dtype=np.float32)
    msg = _rejected("fp32 position", bad, det)
    assert "ulp at the knots" in msg                                        # the tolerance, not a NaN pattern or an exact value
    err = np.abs(bad - det.value).max()
    print(f"fp32 position on bimodal_S8192: worst error {err:.3e} = {err / (2 * PC.MODE):.2e} of the mode separation, "
          f"{err / PM.ulp32(PC.MODE):.0f} fp32 ulp at the modes")
    assert err > 100 * PM.ulp32(PC.MODE)
    PM.check_quantiles("the rule itself", det.value.astype(np.float32), det)
    # the same defect on Gaussian draws is the few ulp the old suite could not see
    g = PC.quantile_case("gauss_S1023_N1_D1_Q9")
    assert np.abs(PM.quantiles(g.x, g.q, position_dtype=np.float32) - PM.quantiles(g.x, g.q)).max() < 1e-5


def test_dropped_plus_inf_fails_the_inf_case():
    c = PC.quantile_case("inf_S257")
    det = PM.quantiles_detail(c.x, c.q)
    bad = PM.quantiles(c.x, c.q, drop_pos_inf=True)
    msg = _rejected("+inf dropped", bad, det)
    assert "NaN pattern" in msg or "not exact" in msg
    PM.check_quantiles("the rule itself", det.value.astype(np.float32), det)
    g = PC.quantile_case("cauchy_S257")                                     # no infinite draw: the defect is invisible
    assert np.array_equal(PM.quantiles(g.x, g.q, drop_pos_inf=True), PM.quantiles(g.x, g.q))


def test_missing_guard_fails_the_integer_positions_beside_inf():
    c = PC.quantile_case("integer_S257")
    det = PM.quantiles_detail(c.x, c.q)
    bad = PM.quantiles(c.x, c.q, guard=False)
    assert "NaN pattern" in _rejected("no f == 0 guard", bad, det)
    fin = PC.quantile_case("gauss_S257_N5_D16_Q5")
    assert np.array_equal(PM.quantiles(fin.x, fin.q, guard=False), PM.quantiles(fin.x, fin.q))


def test_pit_defects_fail_the_pit_comparison():
    s, t = PC.pit_case(300, 37, 4)
    want = PM.pit_ranks(s, t)
    PM.check_pit("the rule itself", want.astype(np.float32), want)
    with pytest.raises(AssertionError, match="ulp"):
        PM.check_pit("<=", PM.pit_ranks(s, t, strict=False).astype(np.float32), want)
    with np.errstate(all="ignore"):
        fin = PM.pit_ranks(s, t, finite_denominator=True)
    assert np.nanmax(fin) > 1                                                # the old oracle: above 1 on -inf draws
    with pytest.raises(AssertionError):
        PM.check_pit("finite denominator", fin.astype(np.float32), want)
    # on draws without +-inf and truths that meet no draw, both defects are invisible
    sp, tp = np.array(s), np.array(t)
    keep = np.isfinite(sp).all(1) & ~(sp == tp[:, None, :]).any(1)
    assert keep.sum() >= 5
    assert np.array_equal(PM.pit_ranks(sp, tp, strict=False)[keep], want[keep])
    assert np.array_equal(PM.pit_ranks(sp, tp, finite_denominator=True)[keep], want[keep])


# ---- the fp32 reference is far inside the floors ------------------------------------------------------------------------------
def _finite_err(a32, a64):
    ok = np.isfinite(a64)
    assert np.array_equal(np.isnan(a32), np.isnan(a64)) and np.array_equal(a32[~ok & ~np.isnan(a64)], a64[~ok & ~np.isnan(a64)])
    return np.abs(a32[ok].astype(np.float64) - a64[ok])


@pytest.mark.parametrize("case", PC.AB_CASES, ids=lambda c: f"{c[0]}-{c[1]:g}-{c[2]}")
def test_fp32_abmag_is_far_inside_its_floor(case):
    """max |abmag32 - abmag64| <= 4 x floor / 10: with it the bar 4 e_ref + floor is never wider than 2.6 floors.  (4 e_ref <=
    floor / 10, the MLP condition, cannot be met by any fp32 evaluation here: half an ulp at 30 mag is 9.5e-7 > 5e-7.)"""
    n, lim, with_err = case
    f, _ = PC.ab_case(n, lim, with_err)
    e = _finite_err(PM.abmag(f, None, lim, np.float32), PM.abmag(f, None, lim))
    print(f"abmag n={n} lim={lim}: max |m32 - m64| {e.max() if e.size else 0:.2e} (floor {AB_FLOOR:.0e})")
    assert e.size == 0 or e.max() <= 0.4 * AB_FLOOR


@pytest.mark.parametrize("case", PC.ASINH_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_fp32_asinh_is_far_inside_its_floor(case):
    f, fb, _ = PC.asinh_case(*case)
    m64 = PM.asinh_mag(f, fb)
    e = np.abs(PM.asinh_mag(f, fb, None, np.float32).astype(np.float64) - m64)
    r = np.abs(f.astype(np.float64) / (2 * fb.astype(np.float64)))
    print(f"asinh {case}: max |m32 - m64| {e.max():.2e} (floor {ASINH_FLOOR:.0e}); largest |f / 2 f_b| {r.max():.1e}")
    assert np.isfinite(m64).all() and e.max() <= 0.4 * ASINH_FLOOR
    if f.size > 14:
        assert r[r > 0].min() <= 1.01e-8 and r.max() >= 0.99e8 and (f == 0).any() and (f < 0).any() and (f > 0).any()


def test_magnitude_model_is_the_oracle_and_the_old_test_formula():
    from oracle import features as OF
    f, fb, e = PC.asinh_case(64, 9)
    a, b = PM.asinh_mag(f, fb, e), OF.flux_to_asinh(f, fb, e)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    fl, er = PC.ab_case(1025, 50.0, True)
    with np.errstate(all="ignore"):
        ref = -2.5 * np.log10(fl.astype(np.float64) / 1000.0) + 23.9      # test_flux_to_abmag_matches_reference_formula
        ref[fl < 0] = 50.0
        ref[ref > 50.0] = 50.0
        rerr = 2.5 * er.astype(np.float64) / (np.log(10) * fl.astype(np.float64))
    m, me = PM.abmag(fl, er, 50.0)
    assert np.array_equal(m, ref, equal_nan=True) and np.array_equal(me, rerr, equal_nan=True)
    sp = dict(zip(["nan", "inf", "-inf", "0", "-0"], PM.abmag(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], np.float32), None, 30.0)))
    assert np.isnan(sp["nan"]) and sp["inf"] == -np.inf and sp["-inf"] == 30.0 and sp["0"] == 30.0 and sp["-0"] == 30.0


# ---- host-side refusals -------------------------------------------------------------------------------------------------------
def test_abi_refuses_bad_arguments(lib):
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)          # never dereferenced: the argument checks come first

    def qs(N=2, S=100, D=3, Q=3, samples=p, q=p, out=p):
        return lib.sf_quantiles(samples, N, S, D, q, Q, out, None)
    for kw in (dict(S=0), dict(S=8193), dict(D=0), dict(Q=0), dict(Q=257), dict(samples=None), dict(q=None), dict(out=None)):
        assert qs(**kw) == -1, kw                                           # SF_ERR_INVALID
        assert lib.sf_last_error()
    assert qs(S=8193) == -1 and b"8192" in lib.sf_last_error()
    assert qs(N=0) == 0                                                      # nothing to do is not an error

    def ql(N=2, S=100, D=3, Q=3, samples=p, q=p, out=p):
        return lib.sf_quantiles_large(samples, N, S, D, q, Q, out, None)
    for kw in (dict(S=0), dict(S=2 ** 24 + 1), dict(Q=257), dict(samples=None), dict(q=None), dict(out=None)):
        assert ql(**kw) == -1, kw

    f = C.c_float
    assert lib.sf_pit_ranks(None, p, 2, 10, 3, p, None) == -1 and lib.sf_pit_ranks(p, None, 2, 10, 3, p, None) == -1
    assert lib.sf_pit_ranks(p, p, 2, 10, 3, None, None) == -1 and lib.sf_pit_ranks(p, p, 2, 0, 3, p, None) == -1
    assert lib.sf_pit_ranks(p, p, 2, 10, 0, p, None) == -1 and lib.sf_pit_ranks(p, p, 0, 10, 3, p, None) == 0
    assert lib.sf_flux_to_abmag(None, None, 8, f(50), p, None, None) == -1 and lib.sf_flux_to_abmag(p, None, 8, f(50), None, None, None) == -1
    assert lib.sf_flux_to_abmag(p, p, 8, f(50), p, None, None) == -1         # errors in, nowhere to put them
    mis = C.c_void_p(p.value + 4)
    assert lib.sf_flux_to_abmag(mis, None, 8, f(50), p, None, None) == -1 and b"aligned" in lib.sf_last_error()
    assert lib.sf_flux_to_abmag(p, None, 0, f(50), p, None, None) == 0
    assert lib.sf_flux_to_asinh(None, None, 2, 3, p, p, None, None) == -1 and lib.sf_flux_to_asinh(p, None, 2, 3, None, p, None, None) == -1
    assert lib.sf_flux_to_asinh(p, None, 2, 0, p, p, None, None) == -1 and lib.sf_flux_to_asinh(p, None, 0, 3, p, p, None, None) == 0
    sd = lambda flux=p, N=2, Cb=3, sigma=p, rows=1, ns=3, out=p: lib.sf_scatter_depths(flux, N, Cb, sigma, rows, ns, f(0), C.c_uint64(1),
                                                                                      out, None, None)
    for kw in (dict(flux=None), dict(sigma=None), dict(out=None), dict(Cb=0), dict(ns=0), dict(rows=2)):
        assert sd(**kw) == -1, kw
    assert sd(N=0) == 0 and sd(rows=3, N=0) == 0


@pytest.mark.parametrize("fn", ["device_quantiles", "device_quantiles_large"])
@pytest.mark.parametrize("q", [[-0.01], [0.5, 1.0000001], [float("nan")], [0.16, float("nan"), 0.84], [float("inf")], 2.0])
def test_wrappers_refuse_q_outside_the_unit_interval(fn, q):
    """numpy's refusal and numpy's message, before any device work: the draws here are on the CPU, which a valid q is refused for."""
    import torch
    from synference_amd import posterior
    with pytest.raises(ValueError) as numpys:
        np.quantile(np.zeros(4), q)
    with pytest.raises(ValueError) as ours:
        getattr(posterior, fn)(torch.zeros(2, 10, 3), q)
    assert str(ours.value) == str(numpys.value) == "Quantiles must be in the range [0, 1]"
    with pytest.raises(RuntimeError, match="GPU"):
        getattr(posterior, fn)(torch.zeros(2, 10, 3), [0.0, 0.5, 1.0])
