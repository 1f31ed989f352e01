"""Missing-band imputation, host side: the numpy model (tests/impute_model.py) pinned against scipy's gaussian_kde, the
threshold ladder on hand-built chi2 values, the margins that the shared fixtures must have for the GPU test to demand exact
selections, and the C entry points refusing bad arguments before they touch a device."""
import ctypes as C
import inspect

import numpy as np
import pytest

import impute_model as IM


def _neighbour_set(duplicate):
    rng = np.random.default_rng(3)
    tb = (25.0 + rng.normal(size=(60, 4))).astype(np.float32)
    y = tb[17].copy() if duplicate else (tb[17] + np.float32(0.01)).astype(np.float32)
    miss = np.array([0, 0, 1, 0], bool)
    rows = np.arange(60)
    return tb, y, miss, rows


@pytest.mark.parametrize("duplicate", [False, True], ids=["ordinary", "duplicate"])
def test_kde_moments_are_scipys(duplicate):
    stats = pytest.importorskip("scipy.stats")
    tb, y, miss, rows = _neighbour_set(duplicate)
    w = IM.neighbour_weights(tb, y, miss, rows)
    assert (w.max() == 1e10) == duplicate                              # dist == 0 -> 1e-10
    x = tb[rows, 2].astype(np.float64)
    wn, neff, cov = IM.kde_moments(x, w, 0.2)
    kde = stats.gaussian_kde(x, bw_method=0.2, weights=w)
    print(f"neff {neff!r} scipy {kde.neff!r} cov {cov!r} scipy {kde.covariance[0, 0]!r}")
    np.testing.assert_allclose(wn, kde.weights, rtol=1e-12, atol=0)
    np.testing.assert_allclose(neff, kde.neff, rtol=1e-12, atol=0)
    np.testing.assert_allclose(cov, kde.covariance[0, 0], rtol=1e-12, atol=0)
    if duplicate:
        assert 0.0 < neff - 1.0 < 1e-5                                 # the cancellation the fp64 moments exist for


def test_threshold_ladder_on_hand_built_chi2():
    thr = IM.thresholds()
    assert thr.dtype == np.float32 and np.array_equal(thr, np.arange(5, 51, 5, dtype=np.float32))
    big = np.full(500, 1e3, np.float32)
    # 29 rows <= 5 and one more <= 10: threshold 10, 30 neighbours
    c = big.copy(); c[10:39] = 1.0; c[400] = 7.5
    sel, used, n, fb = IM.select(c)
    assert used == 10.0 and n == 30 and not fb and np.array_equal(sel, np.r_[10:39, 400])
    # no row <= 50: the 100 smallest, ties to the lowest row
    c = np.full(500, 80.0, np.float32); c[300:360] = 60.0
    sel, used, n, fb = IM.select(c)
    assert fb and n == 100 and used == 50.0 and np.array_equal(sel, np.r_[0:40, 300:360])
    # 8 rows <= 50: a failure (the set is not empty, so no fallback)
    c = big.copy(); c[3:11] = 49.0
    sel, used, n, fb = IM.select(c)
    assert n == -1 and not fb and len(sel) == 0 and used == 50.0
    # fewer rows than min_neighbours in the whole library
    sel, used, n, fb = IM.select(np.full(20, 1e3, np.float32))
    assert n == -1 and fb
    # exactly at a threshold counts (<=)
    c = big.copy(); c[:30] = 5.0
    assert IM.select(c)[1:3] == (5.0, 30)


def test_nan_training_value_contributes_zero():
    tb = np.array([[1.0, 2.0, 3.0], [1.0, np.nan, 3.0]], np.float32)
    y = np.array([0.0, 0.0, np.nan], np.float32)
    sig = np.array([0.5, 1.0, 1.0], np.float32)
    miss = np.array([0, 0, 1], bool)
    for f in (IM.chi2_f32, IM.chi2_f64):
        c = f(tb, y, sig, miss)
        assert np.array_equal(c, [(4.0 + 4.0) / 2, 4.0 / 2])           # dof counts the finite OBSERVED values
    # an observed band whose value is NaN: its terms vanish and dof drops
    y2 = np.array([0.0, np.nan, 0.0], np.float32)
    assert np.array_equal(IM.chi2_f32(tb, y2, sig, np.zeros(3, bool)), [(4.0 + 9.0) / 2, (4.0 + 9.0) / 2])


@pytest.mark.parametrize("shape", IM.SHAPES, ids=lambda s: "x".join(map(str, s[:5])))
def test_shared_fixtures_have_margins(shape):
    """Conditions on the INPUTS of tests/test_gpu_impute.py: no row within TAU of a threshold, the fallback boundary wider
    than TAU, every index uniform farther than 1e-9 of the total weight from a CDF boundary, every kind on its path."""
    NT, F, B, M, nmc, with_err = shape
    cs, mods = IM.case_and_model(shape)
    thr = IM.thresholds()
    for m, (kind, mod) in enumerate(zip(cs["kinds"], mods)):
        tb, y = cs["train"][:, cs["band_col"]], cs["obs"][m][cs["band_col"]]
        c64 = IM.chi2_f64(tb, y, cs["sigma"][m], cs["missing"][m])
        assert len(IM.loose_rows(c64, thr)) == 0, (m, kind)
        sel64 = IM.select(c64, thr)
        assert np.array_equal(sel64[0], mod["rows"]) and sel64[2] == mod["n_used"]     # float32 and float64 agree
        if kind == "fallback":
            s = np.sort(c64)
            assert mod["fallback"] and mod["n_used"] == min(100, NT) and (s[100] - s[99]) > IM.TAU * s[99]
        elif kind == "fail":
            assert mod["n_used"] == -1 and not mod["fallback"] and 1 <= int((c64 <= 50).sum()) <= 29
        elif kind == "mid_ladder":
            assert mod["thr"] == 20.0 and mod["n_used"] >= 30
        else:
            assert mod["thr"] == 5.0 and mod["n_used"] >= 30 and not mod["fallback"]
        if kind == "two_missing" and B >= 3:
            assert cs["missing"][m][0] and cs["missing"][m][-1] and cs["missing"][m].sum() == 2
        if kind == "duplicate":
            assert mod["w"].max() == 1e10
        if mod["n_used"] > 0:
            assert mod["u_margin"] > 1e-9, (m, kind, mod["u_margin"])
    assert {"ordinary", "fallback", "fail"} <= set(cs["kinds"])


def test_draws_do_not_depend_on_the_grouping():
    cs, mods = IM.case_and_model(IM.SHAPES[3])
    a = IM.philox_blocks(IM.SEED, IM.ROW_OFFSET + 2, 4, 2)
    b = IM.philox_blocks(IM.SEED, IM.ROW_OFFSET + 2, 9, 2)
    assert all(np.array_equal(x, y[:4]) for x, y in zip(a, b))
    assert not np.array_equal(a[0], IM.philox_blocks(IM.SEED, IM.ROW_OFFSET + 1, 4, 2)[0])


def test_abi_refuses_bad_arguments(lib):
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)          # never dereferenced: the argument checks come first
    cols = (C.c_int32 * 40)(*range(40))

    def imp(NT=100, F=8, B=4, bc=cols, M=3, nmc=4, train=p, obs=p, sigma=p, missing=p, imputed=p, recon=p, n_used=p,
            step=5.0, nbr=None, cap=0):
        return lib.sf_impute_missing(train, NT, F, bc, None, B, obs, sigma, missing, M, 0, 5.0, step, 50.0, 30, 100, 0.2, nmc, 1,
                                     imputed, recon, n_used, None, None, nbr, cap, None, None)
    bad_col = (C.c_int32 * 4)(0, 1, 2, 8)
    for kw in (dict(B=0), dict(B=33, F=40), dict(F=3), dict(F=65), dict(nmc=0), dict(bc=bad_col), dict(NT=0), dict(step=0.0),
               dict(train=None), dict(obs=None), dict(sigma=None), dict(missing=None), dict(imputed=None), dict(recon=None),
               dict(n_used=None), dict(bc=None), dict(nbr=p, cap=0)):
        assert imp(**kw) == -1, kw                                    # SF_ERR_INVALID
        assert b"sf_impute_missing" in lib.sf_last_error()

    def ql(N=2, S=100, D=3, Q=3, samples=p, q=p, out=p):
        return lib.sf_quantiles_large(samples, N, S, D, q, Q, out, None)
    for kw in (dict(S=0), dict(S=2 ** 24 + 1), dict(D=0), dict(Q=0), dict(Q=257), dict(samples=None), dict(q=None), dict(out=None)):
        assert ql(**kw) == -1, kw
        assert b"sf_quantiles_large" in lib.sf_last_error()
    assert ql(N=0) == 0 and imp(M=0) == 0                              # nothing to do is not an error


def test_public_surface_without_a_gpu():
    import torch
    from synference_amd import SBI_Fitter
    from synference_amd.missing import MissingPhotometryHandler
    from synference_amd.posterior import device_quantiles_large
    sig = inspect.signature(SBI_Fitter.fit_catalogue).parameters
    assert sig["missing_data_mcmc"].default is False and sig["missing_data_mcmc_params"].default is None
    assert sig["missing_data_sigma"].default is None
    h = MissingPhotometryHandler(np.zeros((40, 3), np.float32), None, run_params={"ini_chi": 7.0, "nmc": 5})
    assert h.run_params["ini_chi2"] == 7.0 and "ini_chi" not in h.run_params and h.run_params["nmc"] == 5
    assert h.run_params["max_chi2"] == 50.0 and h.run_params["nposterior"] == 1000 and h.run_params["tmax_all"] == 10
    for name in ("init_from_synference", "generate_imputations", "sample_posterior", "process_observation", "process_catalogue"):
        assert callable(getattr(MissingPhotometryHandler, name))
    with pytest.raises(RuntimeError, match="GPU"):
        device_quantiles_large(torch.zeros(2, 10, 3), [0.5])
