"""The six entry points of csrc/sf_post.hip against the fp64 model (tests/post_model.py) on the named cases of tests/post_cases.py,
through the public wrappers and straight through the C ABI with sentinel-filled outputs.

Bars (tests/test_cpu_post_cases.py shows that each rejects the defect it was made for):
  quantiles   PM.check_quantiles: NaN pattern exact, order statistics at integer positions and infinite values exact, else 1 fp32
              ulp of the larger knot; both kernels against the model and against each other;
  PIT         PM.check_pit: NaN pattern exact, 1 fp32 ulp of the fp64 ratio;
  magnitudes  sharp_cases.check_bar, factor 4 on the fp32 model's own error, floors 2e-5 (AB) and 5e-5 (asinh) mag; magnitude errors per
              element to 4 fp32 ulp; special values exactly;
  scatter     sigma to 1 fp32 ulp, draws to 2e-4 max(1, sigma / 6, |out| / 200).
Every test prints its worst error over its bar ("POST ..." lines): the table in DESIGN.md 0c is filled from them.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import post_cases as PC
import post_model as PM
from sharp_cases import check_bar

pytestmark = pytest.mark.gpu

AB_FLOOR, ASINH_FLOOR = 2e-5, 5e-5
SENT = -7.5


def _dev(a):
    return torch.tensor(np.array(a)).cuda()


@functools.lru_cache(maxsize=None)
def _detail(name):
    c = PC.quantile_case(name)
    return PM.quantiles_detail(c.x, c.q)


def _quant(kernel, x, q):
    from synference_amd.posterior import device_quantiles, device_quantiles_large
    fn = device_quantiles if kernel == "sort" else device_quantiles_large
    return fn(_dev(x), np.array(q)).cpu().numpy()


# ---- quantiles --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.SORT_NAMES)
def test_quantiles_sort_kernel_against_the_model(name):
    c = PC.quantile_case(name)
    got = _quant("sort", c.x, c.q)
    worst = PM.check_quantiles(name, got, _detail(name))
    print(f"POST quantiles sort {name}: worst |difference| / (ulp at the knots) {worst:.3f}")


@pytest.mark.parametrize("name", PC.LARGE_NAMES)
def test_quantiles_large_kernel_against_the_model(name):
    c = PC.quantile_case(name)
    got = _quant("large", c.x, c.q)
    worst = PM.check_quantiles(name, got, _detail(name))
    print(f"POST quantiles large {name}: worst |difference| / (ulp at the knots) {worst:.3f}")


@pytest.mark.parametrize("name", PC.SORT_NAMES)
def test_the_two_quantile_kernels_agree(name):
    """Under the same bar, with the large kernel's result in the model's place (same NaN pattern, exact where the position is an
    integer or the value infinite, one ulp of the larger knot elsewhere)."""
    c = PC.quantile_case(name)
    det = _detail(name)
    a, b = _quant("sort", c.x, c.q), _quant("large", c.x, c.q)
    worst = PM.check_quantiles(name, a, det._replace(value=b.astype(np.float64)))
    print(f"POST quantiles sort vs large {name}: worst |difference| / (ulp at the knots) {worst:.3f}")


def test_quantiles_through_the_abi_leave_the_rest_alone():
    """Raw ABI call with a q vector and an output that sit inside larger sentinel-filled buffers; two launches back to back on
    different shapes (the second, shorter row must not see the first one's LDS); a side stream."""
    from synference_amd import _lib
    lib = _lib.load()
    big, small = PC.quantile_case("inf_S4097"), PC.quantile_case("gauss_S3_N1_D16_Q9")
    side = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(side):
        for fn in (lib.sf_quantiles, lib.sf_quantiles_large):
            for c in (big, small):
                x, q = _dev(c.x), _dev(c.q)
                N, S, D = c.x.shape
                buf = torch.full((N * D * len(c.q) + 16,), SENT, device="cuda")
                out = buf[8:-8]
                assert fn(C.c_void_p(x.data_ptr()), N, S, D, C.c_void_p(q.data_ptr()), len(c.q), C.c_void_p(out.data_ptr()),
                          C.c_void_p(side.cuda_stream)) == 0
                outs.append((c, buf))
    side.synchronize()
    for c, buf in outs:
        h = buf.cpu().numpy()
        assert (h[:8] == SENT).all() and (h[-8:] == SENT).all()
        N, S, D = c.x.shape
        PM.check_quantiles(c.name, h[8:-8].reshape(N, D, len(c.q)), _detail(c.name))


def test_quantile_wrappers_take_strided_and_non_float32_draws():
    from synference_amd.posterior import device_quantiles, device_quantiles_large
    c = PC.quantile_case("gauss_S257_N5_D16_Q5")
    x64 = _dev(c.x).double()
    strided = _dev(np.concatenate([c.x, c.x], 2))[:, :, ::2]                 # every other column of a wider cube
    want = PM.quantiles_detail(np.concatenate([c.x, c.x], 2)[:, :, ::2], c.q)
    for fn in (device_quantiles, device_quantiles_large):
        PM.check_quantiles("float64 draws", fn(x64, list(map(float, c.q))).cpu().numpy(), PM.quantiles_detail(c.x, c.q))
        assert not strided.is_contiguous()
        PM.check_quantiles("strided draws", fn(strided, c.q).cpu().numpy(), want)
        assert tuple(fn(_dev(c.x)[:0], [0.5, 0.9]).shape) == (0, 16, 2)      # N = 0
        with pytest.raises(ValueError, match=r"Quantiles must be in the range \[0, 1\]"):
            fn(_dev(c.x), [0.5, 1.5])


# ---- PIT ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.PIT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_pit_ranks_against_the_model(case):
    from synference_amd.features import pit_ranks
    s, t = PC.pit_case(*case)
    got = pit_ranks(_dev(s), _dev(t)).cpu().numpy()
    worst = PM.check_pit(str(case), got, PM.pit_ranks(s, t))
    print(f"POST pit {case}: worst |difference| / ulp {worst:.3f}")


def test_pit_ranks_other_inputs():
    from synference_amd.features import pit_ranks
    s, t = PC.pit_case(65, 3, 3)
    want = PM.pit_ranks(s, t)
    PM.check_pit("float64, truth on the host", pit_ranks(_dev(s).double(), torch.tensor(np.array(t)).double()).cpu().numpy(), want)
    wide = _dev(np.concatenate([s, s], 2))[:, :, ::2]
    PM.check_pit("strided", pit_ranks(wide, _dev(np.concatenate([t, t], 1))[:, ::2]).cpu().numpy(),
                 PM.pit_ranks(np.concatenate([s, s], 2)[:, :, ::2], np.concatenate([t, t], 1)[:, ::2]))
    assert tuple(pit_ranks(_dev(s)[:0], _dev(t)[:0]).shape) == (0, 3)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a = pit_ranks(_dev(s), _dev(t))
        s2, t2 = PC.pit_case(1, 37, 4)
        b = pit_ranks(_dev(s2), _dev(t2))
    side.synchronize()
    PM.check_pit("side stream", a.cpu().numpy(), want)
    PM.check_pit("side stream, second shape", b.cpu().numpy(), PM.pit_ranks(s2, t2))


# ---- AB magnitudes ----------------------------------------------------------------------------------------------------------------
def _check_ab(label, f, e, lim, mag, merr):
    m64, m32 = PM.abmag(f, None, lim), PM.abmag(f, None, lim, np.float32).astype(np.float64)
    got = np.asarray(mag, dtype=np.float64)
    # special values exactly: NaN stays NaN, +inf flux gives -inf, +-0 / negative / -inf / too faint give the limit itself
    assert np.array_equal(np.isnan(got), np.isnan(m64)), (label, "NaN pattern")
    assert np.array_equal(got == -np.inf, m64 == -np.inf) and not (got == np.inf).any(), (label, "infinite magnitudes")
    with np.errstate(all="ignore"):                                         # (the boundary pair is one fp32 rounding from the limit:
        faint = -2.5 * np.log10(f.astype(np.float64) / 1000.0) + 23.9       #  it is held to the bar; a floor beyond it, to the value)
    clipped = (f < 0) | (f == 0) | ((f > 0) & (faint > lim + AB_FLOOR))
    assert (got[clipped] == lim).all(), (label, "the limit value itself")
    assert (got[~np.isnan(got)] <= lim).all(), (label, "nothing fainter than the limit")
    fin = np.isfinite(m64)
    rs = check_bar(f"POST abmag {label}", got[fin] - m64[fin], m32[fin] - m64[fin], AB_FLOOR)
    if e is not None:
        _, e64 = PM.abmag(f, e, lim)
        worst = PM.check_ulps(f"abmag error {label}", merr, e64, 4.0)
        print(f"POST abmag error {label}: worst |difference| / ulp {worst:.3f}")
    return rs


@pytest.mark.parametrize("case", PC.AB_CASES, ids=lambda c: f"{c[0]}-{c[1]:g}-{c[2]}")
def test_flux_to_abmag_against_the_model(case):
    from synference_amd.features import flux_to_abmag
    n, lim, with_err = case
    f, e = PC.ab_case(n, lim, with_err)
    out = flux_to_abmag(_dev(f), None if e is None else _dev(e), lim)
    mag, merr = (out if with_err else (out, None))
    _check_ab(f"n={n} lim={lim:g}", f, e, lim, mag.cpu().numpy(), None if merr is None else merr.cpu().numpy())


def test_flux_to_abmag_other_inputs():
    from synference_amd.features import flux_to_abmag
    f, e = PC.ab_case(1025, 50.0, True)
    base = _dev(np.concatenate([[0.0], f]).astype(np.float32))
    mis = base[1:]                                                            # contiguous, 4 bytes off a 16-byte boundary: copied
    assert mis.data_ptr() % 16 != 0
    ref = flux_to_abmag(_dev(f), None, 50.0).cpu().numpy()
    assert np.array_equal(flux_to_abmag(mis, None, 50.0).cpu().numpy(), ref, equal_nan=True)
    strided = _dev(np.stack([f, f], 1))[:, 0]
    assert not strided.is_contiguous()
    assert np.array_equal(flux_to_abmag(strided, None, 50.0).cpu().numpy(), ref, equal_nan=True)
    m, me = flux_to_abmag(_dev(f).double(), _dev(e).double(), 50.0)
    _check_ab("float64 input", f, e, 50.0, m.cpu().numpy(), me.cpu().numpy())
    assert tuple(flux_to_abmag(_dev(f.reshape(205, 5))[:0], None, 50.0).shape) == (0, 5)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a = flux_to_abmag(_dev(f), None, 50.0)
        f2, _ = PC.ab_case(7, 99.0, False)
        b = flux_to_abmag(_dev(f2), None, 99.0)
    side.synchronize()
    assert np.array_equal(a.cpu().numpy(), ref, equal_nan=True)
    _check_ab("side stream, second shape", f2, None, 99.0, b.cpu().numpy(), None)


# ---- asinh magnitudes ---------------------------------------------------------------------------------------------------------------
def _check_asinh(label, f, fb, e, mag, merr):
    m64, e64 = PM.asinh_mag(f, fb, e) if e is not None else (PM.asinh_mag(f, fb), None)
    m32 = PM.asinh_mag(f, fb, None, np.float32).astype(np.float64)
    rs = check_bar(f"POST asinh {label}", np.asarray(mag, np.float64) - m64, m32 - m64, ASINH_FLOOR)
    if merr is not None:
        worst = PM.check_ulps(f"asinh error {label}", merr, e64, 4.0)
        print(f"POST asinh error {label}: worst |difference| / ulp {worst:.3f}")
    return rs


@pytest.mark.parametrize("case", PC.ASINH_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_flux_to_asinh_against_the_model(case):
    from synference_amd.features import flux_to_asinh
    f, fb, e = PC.asinh_case(*case)
    mag, merr = flux_to_asinh(_dev(f), _dev(fb), _dev(e))
    _check_asinh(f"{case[0]}x{case[1]}", f, fb, e, mag.cpu().numpy(), merr.cpu().numpy())
    only = flux_to_asinh(_dev(f), fb)                                         # softening from the host, no errors
    assert np.array_equal(only.cpu().numpy(), mag.cpu().numpy())


def test_flux_to_asinh_other_inputs():
    from synference_amd.features import flux_to_asinh
    f, fb, e = PC.asinh_case(64, 7)
    wide = _dev(np.concatenate([f, f], 1))[:, :7]
    assert not wide.is_contiguous()
    m, me = flux_to_asinh(wide.double(), _dev(fb).double(), _dev(e).double())
    _check_asinh("strided float64", f, fb, e, m.cpu().numpy(), me.cpu().numpy())
    assert tuple(flux_to_asinh(_dev(f)[:0], fb).shape) == (0, 7)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a = flux_to_asinh(_dev(f), fb)
        f2, fb2, _ = PC.asinh_case(64, 3)
        b = flux_to_asinh(_dev(f2), fb2)
    side.synchronize()
    _check_asinh("side stream", f, fb, None, a.cpu().numpy(), None)
    _check_asinh("side stream, second shape", f2, fb2, None, b.cpu().numpy(), None)


# ---- depth scatter ------------------------------------------------------------------------------------------------------------------
def _check_scatter(label, out, err, ref_out, ref_sigma):
    worst_s = PM.check_ulps(f"scatter sigma {label}", err, ref_sigma, 1.0)
    d = np.abs(np.asarray(out, np.float64) - ref_out) / PM.draw_bar(ref_out, ref_sigma)
    print(f"POST scatter {label}: sigma worst |difference| / ulp {worst_s:.3f}; draws worst |difference| / bar {d.max():.3f}")
    assert np.isfinite(out).all() and d.max() <= 1.0, (label, float(d.max()))


def _abi_scatter(f, sigma, ns, pc, seed, stream=None):
    from synference_amd import _lib
    N, Cb = f.shape
    fd, sd = _dev(f), _dev(sigma)
    out, err = torch.full((N * ns, Cb), SENT, device="cuda"), torch.full((N * ns, Cb), SENT, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    assert _lib.load().sf_scatter_depths(p(fd), N, Cb, p(sd), sigma.shape[0], ns, C.c_float(pc), C.c_uint64(seed), p(out), p(err),
                                         C.c_void_p(stream.cuda_stream if stream is not None else 0)) == 0
    return out, err


@pytest.mark.parametrize("case", PC.SCATTER_CASES, ids=lambda c: "-".join(map(str, c)))
def test_scatter_depths_against_the_model(case):
    """Through the ABI: sigma rows are its input as they stand (the wrapper divides the depths by depth_sigma before the call)."""
    N, Cb, ns, rows, pc = case
    f, sigma = PC.scatter_case(N, Cb, ns, rows, pc)
    out, err = _abi_scatter(f, sigma, ns, pc, seed=77 + Cb)
    torch.cuda.synchronize()
    ro, rs = PM.scatter_depths(f, sigma, ns, float(np.float32(pc)), 77 + Cb)   # (the ABI carries min_flux_pc_error as float32)
    _check_scatter("-".join(map(str, case)), out.cpu().numpy(), err.cpu().numpy(), ro, rs)


def test_scatter_depths_second_grid_pass():
    N, Cb, ns, rows, pc = PC.SCATTER_BIG
    f, sigma = PC.scatter_case(N, Cb, ns, rows, pc)
    out, err = _abi_scatter(f, sigma, ns, pc, seed=5)
    torch.cuda.synchronize()
    pick = PC.scatter_big_rows()
    ro, rs = PM.scatter_depths(f, sigma, ns, pc, 5, rows=pick)
    idx = torch.as_tensor(pick).cuda()
    _check_scatter("second grid pass", out[idx].cpu().numpy(), err[idx].cpu().numpy(), ro, rs)
    assert bool((out != SENT).all()) and bool((err != SENT).all())            # every element of every row was written


def test_scatter_depths_wrapper_and_other_inputs():
    from synference_amd.features import scatter_depths
    f, sigma = PC.scatter_case(33, 5, 3, 1, 60.0)
    depths = (sigma[0] * np.float32(5.0)).astype(np.float32)
    sg = (depths / np.float32(5.0)).astype(np.float32)[None]                 # what the wrapper hands to the ABI
    ro, rs = PM.scatter_depths(f, sg, 3, 60.0, 11)
    wide = _dev(np.concatenate([f, f], 1))[:, :5]
    assert not wide.is_contiguous()
    out, err = scatter_depths(wide.double(), depths, n_scatters=3, depth_sigma=5.0, min_flux_pc_error=60.0, seed=11, return_errors=True)
    _check_scatter("wrapper, strided float64", out.cpu().numpy(), err.cpu().numpy(), ro, rs)
    assert tuple(scatter_depths(_dev(f)[:0], depths, n_scatters=3).shape) == (0, 5)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a = scatter_depths(_dev(f), depths, n_scatters=3, depth_sigma=5.0, min_flux_pc_error=60.0, seed=11)
        f2, s2 = PC.scatter_case(33, 17, 1, 1, 0.01)
        b, be = _abi_scatter(f2, s2, 1, 0.01, seed=3, stream=side)
    side.synchronize()
    assert np.array_equal(a.cpu().numpy(), out.cpu().numpy())
    r2, rs2 = PM.scatter_depths(f2, s2, 1, 0.01, 3)
    _check_scatter("side stream, second shape", b.cpu().numpy(), be.cpu().numpy(), r2, rs2)
