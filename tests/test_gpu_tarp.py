"""TARP coverage on the device (csrc/sf_tarp.hip) against the numpy model (tests/tarp_model.py).

The device evaluates the distances in float32, the model in float64 on the same float32 inputs, so a count may differ
where a draw's distance lies within float32 rounding of the truth's: every cell must lie inside the model's band
[k_lo, k_hi] (tarp_model.TAU).  Everything after the counts is integer or float64 arithmetic and must agree to 1e-12:
the resampled rows exactly, the curve recomputed from the RETURNED counts, and, in every pass whose counts equal the
model's, the np.histogram form of the curve and its edges."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import tarp_model as TM

pytestmark = pytest.mark.gpu

# (N, S, D, B): S not a multiple of 64 / D = 1, three bins / one bin, widest D / LDS tiling / many occurrences per row
SHAPES = [(64, 100, 5, 8), (37, 257, 1, 4), (10, 64, 16, 3), (12, 8192, 16, 2), (300, 1000, 3, 8)]
METRICS = ["euclidean", "manhattan"]
SEED = 0x1234_5678_9ABC


@functools.lru_cache(maxsize=None)
def _data(shape):
    N, S, D, B = shape
    x, theta = TM.gaussian_case(N, S, D, seed=1000 + N + S)
    x.setflags(write=False); theta.setflags(write=False)
    return x, theta


@functools.lru_cache(maxsize=None)
def _model(shape, metric, norm_axis):
    """One model evaluation per case, shared by the tests below."""
    N, S, D, B = shape
    x, theta = _data(shape)
    return TM.tarp_coverage(x, theta, metric=metric, norm=norm_axis >= 0, bootstrap=True, num_bootstrap=B,
                            num_alpha_bins=max(1, N // 10), seed=SEED, norm_axis=max(norm_axis, 0), band=True)


def _buffers(x, theta, B=0, n=None, references=None):
    """Device copies of the inputs and sentinel-filled outputs of one call."""
    N, S, D = x.shape
    n = n if n is not None else max(1, N // 10)
    rows = max(B, 1)
    return dict(x=torch.tensor(x).cuda(), theta=torch.tensor(theta).cuda(),     # (copies: the cached inputs are read-only)
                refs=None if references is None else torch.tensor(np.asarray(references, dtype=np.float32)).cuda(),
                ecp=torch.full((rows, n + 1), -7.0, dtype=torch.float64, device="cuda"),
                alpha=torch.full((n + 1,), -7.0, dtype=torch.float64, device="cuda"),
                counts=torch.full((rows, N), -7, dtype=torch.int32, device="cuda"),
                bidx=torch.full((rows, N), -7, dtype=torch.int32, device="cuda"), B=B, n=n)


def _queue(buf, metric="euclidean", norm_axis=0, seed=SEED, lib=None):
    """The call on torch's current stream, straight through the C ABI; nothing waits for it."""
    from synference_amd import _lib
    lib = lib or _lib.load()
    N, S, D = buf["x"].shape
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    _lib.check(lib.sf_tarp_coverage(p(buf["x"]), p(buf["theta"]), N, S, D, p(buf["refs"]), METRICS.index(metric), norm_axis,
                                    buf["B"], buf["n"], C.c_uint64(seed), p(buf["ecp"]), p(buf["alpha"]), p(buf["counts"]),
                                    p(buf["bidx"]) if buf["B"] else None, C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def _host(buf):
    return (buf["ecp"].cpu().numpy(), buf["alpha"].cpu().numpy(), buf["counts"].cpu().numpy().astype(np.int64),
            buf["bidx"].cpu().numpy().astype(np.int64))


def _device(x, theta, metric="euclidean", norm_axis=0, B=0, n=None, seed=SEED, references=None, lib=None):
    """Straight through the C ABI with counts and boot_idx returned."""
    buf = _buffers(x, theta, B, n, references)
    _queue(buf, metric, norm_axis, seed, lib)
    torch.cuda.synchronize()
    return _host(buf)


def _check_against_model(ecp, alpha, counts, m, S, n):
    """The requirements of every case; returns the number of passes whose counts equal the model's."""
    lo_ok, hi_ok = m["k_lo"] <= counts, counts <= m["k_hi"]
    print(f"cells {counts.size}: differ from the float64 count {int((counts != m['counts']).sum())}, "
          f"band loose in {int((m['k_lo'] != m['k_hi']).sum())}, outside the band {int((~lo_ok).sum() + (~hi_ok).sum())}")
    assert lo_ok.all() and hi_ok.all()                                # EVERY cell
    same = 0
    for b in range(counts.shape[0]):
        e_c, a_c = TM.curve_counts(counts[b], S, n)
        assert np.abs(ecp[b] - e_c).max() < 1e-12
        if np.array_equal(counts[b], m["counts"][b]):
            e_h, a_h = TM.curve_histogram(m["counts"][b], S, n)
            assert np.abs(ecp[b] - e_h).max() < 1e-12
            if b == counts.shape[0] - 1:
                assert np.array_equal(alpha, a_h)
            same += 1
    e_c, a_c = TM.curve_counts(counts[-1], S, n)
    assert np.array_equal(alpha, a_c)                                 # alpha: the edges of the last pass
    return same


@pytest.mark.parametrize("norm_axis", [-1, 0, 1])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_counts_and_curves_match_the_model(shape, metric, norm_axis):
    N, S, D, B = shape
    x, theta = _data(shape)
    m = _model(shape, metric, norm_axis)
    n = max(1, N // 10)
    ecp, alpha, counts, bidx = _device(x, theta, metric, norm_axis, B)
    assert np.array_equal(bidx, m["idx"])                             # the row resample: exactly
    assert counts.min() >= 0 and counts.max() <= S
    same = _check_against_model(ecp, alpha, counts, m, S, n)
    print(f"passes with the model's counts: {same} of {B}")


# N = 1, and N around and beyond the 1024 threads of the row-count scan: a thread owns one count, then several
SCAN_SHAPES = [(N, 8, 1, 2) for N in (1, 1023, 1024, 1025, 2500)]


@pytest.mark.parametrize("shape", SCAN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_row_scan_beyond_one_count_per_thread(shape):
    N, S, D, B = shape
    x, theta = _data(shape)
    m = _model(shape, "euclidean", 0)
    n = max(1, N // 10)
    ecp, alpha, counts, bidx = _device(x, theta, "euclidean", 0, B)
    assert np.array_equal(bidx, m["idx"])                             # the row resample: exactly
    assert counts.min() >= 0 and counts.max() <= S
    _check_against_model(ecp, alpha, counts, m, S, n)


def test_scratch_reuse_across_sizes():
    """Small, large, small again: the scratch grows, serves a smaller layout from the larger buffer, then one of equal size."""
    small, large = (37, 257, 1, 4), (300, 1000, 3, 8)
    first = _device(*_data(small), "euclidean", 0, small[3])
    ecp, alpha, counts, bidx = _device(*_data(large), "euclidean", 0, large[3])
    third = _device(*_data(small), "euclidean", 0, small[3])
    for u, v in zip(first, third):
        assert u.tobytes() == v.tobytes()
    m = _model(large, "euclidean", 0)
    assert np.array_equal(bidx, m["idx"]) and counts.min() >= 0 and counts.max() <= large[1]
    _check_against_model(ecp, alpha, counts, m, large[1], max(1, large[0] // 10))
    m = _model(small, "euclidean", 0)
    assert np.array_equal(first[3], m["idx"])
    _check_against_model(*first[:3], m, small[1], max(1, small[0] // 10))


def test_two_calls_on_two_streams():
    """Two calls queued back to back on two streams, with no host synchronisation in between; different data and a different
    N, so that the second call carves the shared scratch differently.  Each result must equal that call's result when it
    runs alone.  This walks the wait-and-record path of the scratch (the second call's stream waits for the event the first
    call recorded).  It is not a detector: a lost ordering would not fail reliably, and the test must never be looped to
    make it fail."""
    cases = [((64, 100, 5, 8), "euclidean"), ((37, 257, 1, 4), "manhattan")]
    alone = [_device(*_data(shape), metric, 0, shape[3]) for shape, metric in cases]
    bufs = [_buffers(*_data(shape), shape[3]) for shape, _ in cases]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for buf, st, (_, metric) in zip(bufs, streams, cases):
        with torch.cuda.stream(st):
            _queue(buf, metric, 0)
    for st in streams:
        st.synchronize()
    for buf, want in zip(bufs, alone):
        for u, v in zip(_host(buf), want):
            assert u.tobytes() == v.tobytes()


def test_explicit_references_and_the_non_bootstrap_call():
    shape = (64, 100, 5, 8)
    N, S, D, B = shape
    x, theta = _data(shape)
    n = 6
    # no bootstrap: one pass over the rows in order, reference points of pass 0
    m = TM.tarp_coverage(x, theta, norm=True, num_alpha_bins=n, seed=SEED, band=True)
    ecp, alpha, counts, _ = _device(x, theta, "euclidean", 0, 0, n)
    assert ecp.shape == (1, n + 1)
    _check_against_model(ecp, alpha, counts, m, S, n)
    # explicit references: used by position in every pass, not resampled
    refs = np.random.default_rng(3).uniform(size=(N, D)).astype(np.float32)
    for B_ in (0, 3):
        m = TM.tarp_coverage(x, theta, references=refs, metric="manhattan", norm=True, bootstrap=B_ > 0, num_bootstrap=B_,
                             num_alpha_bins=n, seed=SEED, band=True)
        ecp, alpha, counts, bidx = _device(x, theta, "manhattan", 0, B_, n, references=refs)
        if B_:
            assert np.array_equal(bidx, m["idx"])
        _check_against_model(ecp, alpha, counts, m, S, n)
    assert not np.array_equal(_device(x, theta, "manhattan", 0, 0, n)[2], counts[:1])   # ... and they are used


def test_all_nan_row_counts_zero():
    shape = (64, 100, 5, 8)
    N, S, D, B = shape
    x, theta = _data(shape)
    x = x.copy()
    x[7] = np.nan
    x[9, ::3, 2] = np.nan
    m = TM.tarp_coverage(x, theta, norm=True, bootstrap=True, num_bootstrap=B, num_alpha_bins=6, seed=SEED, band=True)
    ecp, alpha, counts, bidx = _device(x, theta, "euclidean", 0, B, 6)
    assert (bidx == 7).any() and (counts[bidx == 7] == 0).all() and (m["counts"][m["idx"] == 7] == 0).all()
    _check_against_model(ecp, alpha, counts, m, S, 6)


def test_all_counts_equal_takes_the_half_unit_range():
    N, S, D = 30, 70, 2
    theta = np.zeros((N, D), np.float32)
    refs = np.full((N, D), 0.25, np.float32)
    for far, k in ((True, 0), (False, S)):
        # every draw farther from / nearer to the reference point than the truth: all counts 0 / S
        x = np.full((N, S, D), 5.0 if far else 0.25, np.float32)
        ecp, alpha, counts, _ = _device(x, theta, "euclidean", -1, 0, 4, references=refs)
        assert (counts == k).all()
        e_h, a_h = TM.curve_histogram(counts[0], S, 4)
        assert alpha[0] == k / S - 0.5 and alpha[-1] == k / S + 0.5 and np.array_equal(alpha, a_h)
        assert np.abs(ecp[0] - e_h).max() < 1e-12 and ecp[0, 0] == 0.0 and ecp[0, -1] == 1.0


def test_two_calls_are_bitwise_equal():
    shape = (300, 1000, 3, 8)
    x, theta = _data(shape)
    a = _device(x, theta, "euclidean", 0, 8)
    torch.empty(1 << 20, device="cuda").normal_()                     # other work in between
    b = _device(x, theta, "euclidean", 0, 8)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    c = _device(x, theta, "euclidean", 0, 8, seed=SEED + 1)
    assert not np.array_equal(a[3], c[3])


def test_features_wrapper_matches_the_abi():
    from synference_amd.features import tarp_coverage
    shape = (64, 100, 5, 8)
    x, theta = _data(shape)
    xd = torch.tensor(x).cuda()
    ecp, alpha, counts, bidx = tarp_coverage(xd, theta, norm=True, bootstrap=True, num_bootstrap=8, seed=SEED, return_counts=True)
    e0, a0, c0, i0 = _device(x, theta, "euclidean", 0, 8, 6)
    assert ecp.shape == (8, 7) and ecp.dtype == np.float64 and np.array_equal(ecp, e0) and np.array_equal(alpha, a0)
    assert np.array_equal(counts, c0) and np.array_equal(bidx, i0)
    e1, a1 = tarp_coverage(xd, theta, norm=True, seed=SEED)          # no bootstrap: one curve, N // 10 bins
    assert e1.shape == (7,) and np.array_equal(e1, _device(x, theta, "euclidean", 0, 0, 6)[0][0])
    e2, _ = tarp_coverage(xd, theta, norm=True, norm_axis=1, seed=SEED)
    assert np.array_equal(e2, _device(x, theta, "euclidean", 1, 0, 6)[0][0])
    with pytest.raises(ValueError, match="at least 10 rows"):
        tarp_coverage(xd[:9], theta[:9])
    with pytest.raises(ValueError, match="metric"):
        tarp_coverage(xd, theta, metric="chebyshev")


@pytest.fixture(scope="module")
def fitter():
    from synference_amd import SBI_Fitter
    return SBI_Fitter("tarp", ["a", "b", "c"], device="cuda")


def test_fitter_known_answer_calibrated_and_shifted(fitter):
    """The thresholds of tests/test_cpu_tarp.py on the device: exact conjugate posterior below 0.03, shifted by 0.8 sigma
    above 0.10 (N = 400, S = 200, D = 3, 16 passes, axis 0; seed 4 of that test, see its docstring on the seeds)."""
    x, theta = TM.gaussian_case(400, 200, 3, seed=4)
    good = fitter.calculate_TARP(None, theta, num_bootstrap=16, samples=x.transpose(1, 0, 2), seed=104)
    assert isinstance(good, torch.Tensor) and good.dim() == 0 and good.dtype == torch.float64 and good.device.type == "cuda"
    want = TM.tarp_value(TM.tarp_coverage(x, theta, norm=True, bootstrap=True, num_bootstrap=16, seed=104)["ecp"])
    xs, _ = TM.gaussian_case(400, 200, 3, seed=4, shift=0.8)
    bad = fitter.calculate_TARP(None, theta, num_bootstrap=16, samples=torch.as_tensor(xs.transpose(1, 0, 2)), seed=104)
    print(f"calibrated {float(good):.4f} (model {want:.4f}) shifted {float(bad):.4f}")
    assert float(good) < 0.03 and float(bad) > 0.10
    assert abs(float(good) - want) < 2e-3                            # a band cell moves ecp by 1 / N per pass at most
    assert float(fitter.calculate_TARP(None, theta, num_bootstrap=16, samples=x.transpose(1, 0, 2), seed=104)) == float(good)


def test_evaluate_model_carries_the_key_on_request(fitter):
    x, theta = TM.gaussian_case(400, 200, 3, seed=0)
    m = fitter.evaluate_model(X_test=None, y_test=theta, num_samples=200, samples=x, tarp=True, seed=100)
    assert isinstance(m["tarp"], list) and len(m["tarp"]) == 1 and 0.0 <= m["tarp"][0] < 0.03
    assert "tarp" not in fitter.evaluate_model(X_test=None, y_test=theta, num_samples=200, samples=x)


def test_fitter_refuses_more_than_8192_draws(fitter):
    x = np.zeros((9000, 12, 2), np.float32)                          # (S, N, D)
    with pytest.raises(RuntimeError, match="1 <= S <= 8192"):
        fitter.calculate_TARP(None, np.zeros((12, 2), np.float32), samples=x, num_bootstrap=2, seed=1)
