"""Missing-band imputation on the device (csrc/sf_impute.hip, sf_quantiles_large in csrc/sf_post.hip) against the numpy
model (tests/impute_model.py), straight through the C ABI with sentinel-filled outputs.

The shared fixtures have margins (tests/test_cpu_impute.py asserts them): no training row lies within TAU of a threshold, so
the float32 device selection must equal the model's exactly -- n_used, the threshold and the whole neighbour list; the
moments are compared on the RETURNED list (fp64, rtol 1e-6: the duplicate object's 1 - sum w^2 ~ 1e-7 costs about 1e-7);
every index uniform is farther than 1e-9 of the total weight from a CDF boundary, so draw_idx must be exact; a value may differ
from the float32 model by 2 ulp plus 1e-5 sqrt(var) (ten times the |dz| ~ 1e-6 of the hardware Box-Muller against libm that
csrc/sf_rng.h states)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import impute_model as IM

pytestmark = pytest.mark.gpu

SENT_F, SENT_I = -7.5, -77
IDS = ["x".join(map(str, s[:5])) for s in IM.SHAPES]


def _device(shape, lo=0, hi=None, nbr_cap=None, seed=IM.SEED, budget=None):
    """Objects [lo, hi) of the shape's case in one call.  Returns a dict of numpy arrays."""
    from synference_amd import _lib
    lib = _lib.load()
    NT, F, B, M, nmc, with_err = shape
    cs, _ = IM.case_and_model(shape)
    hi = M if hi is None else hi
    m = hi - lo
    cap = NT if nbr_cap is None else nbr_cap
    dev = "cuda"
    train = torch.tensor(cs["train"]).to(dev)
    obs = torch.tensor(cs["obs"][lo:hi]).to(dev)
    sigma = torch.tensor(cs["sigma"][lo:hi]).to(dev)
    missing = torch.tensor(cs["missing"][lo:hi]).to(dev)
    out = dict(imputed=torch.full((m, nmc, F), SENT_F, device=dev), recon=torch.full((m, B), SENT_F, device=dev),
               n_used=torch.full((m,), SENT_I, dtype=torch.int32, device=dev), thr=torch.full((m,), SENT_F, device=dev),
               kde_var=torch.full((m, B), SENT_F, dtype=torch.float64, device=dev),
               nbr_idx=torch.full((m, cap), SENT_I, dtype=torch.int32, device=dev),
               draw_idx=torch.full((m, nmc, B), SENT_I, dtype=torch.int32, device=dev))
    bc = (C.c_int32 * B)(*[int(c) for c in cs["band_col"]])
    ec = (C.c_int32 * B)(*[int(c) for c in cs["err_col"]]) if with_err else None
    p = lambda t: C.c_void_p(t.data_ptr())
    old = os.environ.get("SF_IMPUTE_SCRATCH_BYTES")
    if budget is not None:
        os.environ["SF_IMPUTE_SCRATCH_BYTES"] = str(budget)
    try:
        _lib.check(lib.sf_impute_missing(p(train), NT, F, bc, ec, B, p(obs), p(sigma), p(missing), m, IM.ROW_OFFSET + lo,
                                         5.0, 5.0, 50.0, 30, 100, 0.2, nmc, C.c_uint64(seed), p(out["imputed"]), p(out["recon"]),
                                         p(out["n_used"]), p(out["thr"]), p(out["kde_var"]), p(out["nbr_idx"]), cap,
                                         p(out["draw_idx"]), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    finally:
        if budget is not None:
            if old is None:
                del os.environ["SF_IMPUTE_SCRATCH_BYTES"]
            else:
                os.environ["SF_IMPUTE_SCRATCH_BYTES"] = old
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _run(shape):
    return _device(shape)


def _check_selection(shape, d):
    NT, F, B, M, nmc, with_err = shape
    cs, mods = IM.case_and_model(shape)
    for m, mod in enumerate(mods):
        print(f"object {m} {cs['kinds'][m]}: n_used {d['n_used'][m]} (model {mod['n_used']}) thr {d['thr'][m]} (model {mod['thr']})")
        assert d["n_used"][m] == mod["n_used"] and d["thr"][m] == mod["thr"]
        n = max(int(mod["n_used"]), 0)
        assert np.array_equal(d["nbr_idx"][m, :n], mod["rows"])
        assert (d["nbr_idx"][m, n:] == SENT_I).all()                  # nothing past the object's list
        if mod["n_used"] < 0:                                         # a failure: NaN outputs
            assert np.isnan(d["imputed"][m]).all() and np.isnan(d["recon"][m]).all() and (d["draw_idx"][m] == -1).all()


def test_a_short_neighbour_buffer_is_respected():
    shape = IM.SHAPES[0]
    _, mods = IM.case_and_model(shape)
    d = _device(shape, nbr_cap=7)
    for m, mod in enumerate(mods):
        k = min(7, max(int(mod["n_used"]), 0))
        assert np.array_equal(d["nbr_idx"][m, :k], mod["rows"][:k]) and (d["nbr_idx"][m, k:] == SENT_I).all()
    assert np.array_equal(d["imputed"], _run(shape)["imputed"], equal_nan=True)


def _check_moments(shape, d):
    NT, F, B, M, nmc, with_err = shape
    cs, mods = IM.case_and_model(shape)
    worst = 0.0
    for m in range(M):
        n = int(d["n_used"][m])
        miss = cs["missing"][m].astype(bool)
        assert np.isnan(d["kde_var"][m][~miss]).all()
        if n <= 0:
            continue
        mod = IM.impute_object(cs["train"], cs["band_col"], cs["err_col"], cs["obs"][m], cs["sigma"][m], miss, IM.ROW_OFFSET + m,
                               IM.SEED, nmc, rows=d["nbr_idx"][m, :n])
        rel = np.abs(d["kde_var"][m][miss] / mod["var"][miss] - 1.0).max()
        worst = max(worst, rel)
        assert rel < 1e-6, (m, cs["kinds"][m], rel)
    print(f"kde_var: worst relative difference {worst:.2e}")


def _check_draws(shape, d):
    NT, F, B, M, nmc, with_err = shape
    cs, mods = IM.case_and_model(shape)
    bc, ec = cs["band_col"], cs["err_col"]
    worst = 0.0
    for m, mod in enumerate(mods):
        if mod["n_used"] < 0:
            continue
        miss = cs["missing"][m].astype(bool)
        assert np.array_equal(d["draw_idx"][m], mod["draw_idx"])      # exactly (observed bands: -1)
        repl = np.zeros(F, bool)
        repl[bc[miss]] = True
        if with_err:
            repl[ec[miss]] = True
        want = np.broadcast_to(cs["obs"][m], (nmc, F))
        assert d["imputed"][m][:, ~repl].tobytes() == want[:, ~repl].tobytes()          # observed columns: bit for bit
        for b in np.where(miss)[0]:
            got, ref = d["imputed"][m][:, bc[b]].astype(np.float64), mod["imputed"][:, bc[b]].astype(np.float64)
            tol = 2 * np.spacing(np.abs(mod["imputed"][:, bc[b]])).astype(np.float64) + 1e-5 * float(mod["sd"][b])
            worst = max(worst, float((np.abs(got - ref) / tol).max()))
            assert (np.abs(got - ref) <= tol).all(), (m, b)
            if with_err:
                assert np.array_equal(d["imputed"][m][:, ec[b]], cs["train"][d["draw_idx"][m][:, b], ec[b]])
            mean = d["imputed"][m][:, bc[b]].astype(np.float64).mean()
            assert abs(d["recon"][m, b] - mean) <= 1e-6 * abs(mean)
        assert np.isnan(d["recon"][m][~miss]).all()
    print(f"imputed values: worst |difference| / tolerance {worst:.3f}")


@pytest.mark.parametrize("shape", IM.SHAPES, ids=IDS)
def test_selection_is_the_models(shape):
    _check_selection(shape, _run(shape))


@pytest.mark.parametrize("shape", IM.SHAPES, ids=IDS)
def test_moments_on_the_returned_list(shape):
    _check_moments(shape, _run(shape))


@pytest.mark.parametrize("shape", IM.SHAPES, ids=IDS)
def test_draws_are_the_models(shape):
    _check_draws(shape, _run(shape))


def test_scratch_reuse_across_sizes():
    """Small, large, small again: both scratch regions grow, serve a smaller layout from the larger buffers, then one of equal
    size."""
    small, large = IM.SHAPES[3], IM.SHAPES[0]
    first, second, third = _device(small), _device(large), _device(small)
    for k in first:
        assert first[k].tobytes() == third[k].tobytes(), k
    for shape, d in ((small, first), (large, second)):
        _check_selection(shape, d)
        _check_moments(shape, d)
        _check_draws(shape, d)


def test_reproducible_and_independent_of_the_grouping():
    shape = IM.SHAPES[0]
    NT, F, B, M, nmc, with_err = shape
    a = _run(shape)
    torch.empty(1 << 20, device="cuda").normal_()                     # other work in between
    b = _device(shape)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    # two calls over halves with row_offset
    h1, h2 = _device(shape, 0, M // 2), _device(shape, M // 2, M)
    for k in a:
        assert np.concatenate([h1[k], h2[k]]).tobytes() == a[k].tobytes(), k
    # a scratch budget of 2000 bytes = 100 list entries: several object groups (one object alone may exceed it)
    c = _device(shape, budget=2000)
    for k in a:
        assert c[k].tobytes() == a[k].tobytes(), k
    other = _device(shape, seed=IM.SEED + 1)
    assert not np.array_equal(other["draw_idx"], a["draw_idx"]) and np.array_equal(other["nbr_idx"], a["nbr_idx"])


# ---- sf_quantiles_large -------------------------------------------------------------------------------------------------------
QSHAPES = [(3, 8193, 1), (2, 20000, 5), (2, 100000, 16), (4, 100, 3)]
QS = np.array([0.16, 0.5, 0.84, 0.0, 1.0, 0.0275], np.float32)


def _ql(x, q):
    from synference_amd.posterior import device_quantiles_large
    return device_quantiles_large(torch.tensor(x).cuda(), q).cpu().numpy()


@pytest.mark.parametrize("shape", QSHAPES, ids=lambda s: "x".join(map(str, s)))
def test_quantiles_large_against_numpy(shape):
    N, S, D = shape
    rng = np.random.default_rng(S)
    x = (rng.normal(size=shape) * np.array([1.0, 1e-3, 1e3, 1.0][: min(D, 4)] + [1.0] * max(0, D - 4))).astype(np.float32)
    x[rng.uniform(size=shape) < 0.01] = np.nan                        # NaN draws sprinkled in
    x[0, :, D - 1] = np.nan                                           # ... and one all-NaN row
    x[N - 1, : S // 2, 0] = x[N - 1, 0, 0]                            # ... and many equal draws
    got = _ql(x, QS)
    assert got.shape == (N, D, len(QS))
    with np.errstate(all="ignore"):
        want = np.nanquantile(x.astype(np.float64), QS.astype(np.float64), axis=1).transpose(1, 2, 0)
    assert np.isnan(got[0, D - 1]).all() and np.isnan(want[0, D - 1]).all()
    ok = ~np.isnan(want)
    # the device interpolates in float64 and rounds once: half an ulp of the result, plus numpy's own float64 rounding
    tol = np.spacing(np.abs(want[ok]).astype(np.float32)).astype(np.float64)
    err = np.abs(got[ok].astype(np.float64) - want[ok])
    print(f"worst |difference| / ulp {float((err / tol).max()):.3f}")
    assert np.isfinite(got[ok]).all() and (err <= tol).all()


def test_quantiles_large_integer_positions_are_order_statistics():
    S, n = 10050, 10001                                                # 10001 finite draws: (n - 1) q is an integer
    rng = np.random.default_rng(1)
    x = np.full((2, S, 3), np.nan, np.float32)
    for g in range(2):
        for d in range(3):
            x[g, rng.permutation(S)[:n], d] = rng.normal(size=n).astype(np.float32)
    got = _ql(x, np.array([0.0, 0.5, 1.0], np.float32))
    for g in range(2):
        for d in range(3):
            s = np.sort(x[g, :, d][~np.isnan(x[g, :, d])])
            assert np.array_equal(got[g, d], [s[0], s[5000], s[-1]])


def test_quantiles_large_agrees_with_the_lds_sort():
    from synference_amd.posterior import device_quantiles
    import post_model as PM
    x = torch.tensor(np.random.default_rng(2).normal(size=(5, 4096, 5)).astype(np.float32)).cuda()
    a, b = device_quantiles(x, [0.16, 0.5, 0.84]).cpu().numpy(), _ql(x.cpu().numpy(), [0.16, 0.5, 0.84])
    assert np.abs(a - b).max() < 1e-5
    # both kernels form the position and the interpolation in fp64 and round once: one fp32 ulp of the larger knot (the bar of
    # tests/test_gpu_post.py, with the other kernel's result in the model's place)
    det = PM.quantiles_detail(x.cpu().numpy(), [0.16, 0.5, 0.84])
    PM.check_quantiles("sort against select", a, det._replace(value=b.astype(np.float64)))


# ---- the Python surface ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    """A small trained-shape MAF (random weights are enough: the test is about the plumbing) on a synthetic library."""
    from cases import make_case
    from synference_amd import SBI_Fitter
    from synference_amd.estimator import FlowEstimator
    from synference_amd.posterior import EnsemblePosterior, FlowPosterior
    from synference_amd.priors import CustomIndependentUniform
    ospec, spec, flat, theta, x = make_case("maf_small", B=400)
    names = [f"p{i}" for i in range(spec.D)]
    fit = SBI_Fitter("impute", names, device="cuda")
    fit.feature_array = np.asarray(x, np.float32)
    fit.feature_names = [f"f{i}" for i in range(spec.C)]
    est = FlowEstimator(spec, torch.as_tensor(flat), device="cuda:0").to("cuda:0")
    lo = (np.asarray(theta).min(0) - 50.0).astype(np.float32)
    hi = (np.asarray(theta).max(0) + 50.0).astype(np.float32)
    fit.posteriors = EnsemblePosterior([FlowPosterior(est, CustomIndependentUniform(lo, hi, names, device="cuda:0"), seed=1)])
    fit.fitted_parameter_names = names
    fit.simple_fitted_parameter_names = names
    return fit, np.asarray(x, np.float32)


def test_fit_catalogue_marginalises_flagged_rows(fitted):
    fit, x = fitted
    C_ = x.shape[1]
    cat = x[:12].copy() + np.float32(0.01)
    cat[3, 1] = np.nan
    cat[7, 0] = np.nan
    cat[7, C_ - 1] = np.nan
    params = {"nmc": 6, "nposterior": 50, "ini_chi": 5.0}
    base = fit.fit_catalogue(cat, num_samples=64, seed=5, missing_data_flag=np.nan)
    with pytest.raises(ValueError, match="missing_data_sigma"):
        fit.fit_catalogue(cat, num_samples=64, seed=5, missing_data_flag=np.nan, missing_data_mcmc=True)
    tab = fit.fit_catalogue(cat, num_samples=64, seed=5, missing_data_flag=np.nan, missing_data_mcmc=True,
                            missing_data_mcmc_params=params, missing_data_sigma=0.5)
    qcols = [c for c in base.columns if c[:1] == "p"]
    complete = np.ones(12, bool)
    complete[[3, 7]] = False
    assert np.isnan(base.loc[~complete, qcols].to_numpy()).all()
    assert base.loc[complete, qcols].to_numpy().tobytes() == tab.loc[complete, qcols].to_numpy().tobytes()   # bit-identical
    assert list(tab["has_missing_data"]) == list(~complete)
    assert np.isfinite(tab.loc[~complete, qcols].to_numpy()).all()
    h = fit.missing_handler
    assert h.run_params["nmc"] == 6 and h.run_params["nposterior"] == 50            # the caller's settings are applied
    assert {"predicted_f0", "predicted_f1", f"predicted_f{C_ - 1}"} == {c for c in tab.columns if c.startswith("predicted_")}
    assert np.isfinite(tab["predicted_f1"][3]) and np.isnan(np.delete(tab["predicted_f1"].to_numpy(), 3)).all()
    # the same seed gives the same table; the pooled draws are nmc * nposterior long and their quantiles are the table's
    tab2, samples = fit.fit_catalogue(cat, num_samples=64, seed=5, missing_data_flag=np.nan, missing_data_mcmc=True,
                                      missing_data_mcmc_params=params, missing_data_sigma=0.5, return_samples=True)
    assert tab2.loc[~complete, qcols].to_numpy().tobytes() == tab.loc[~complete, qcols].to_numpy().tobytes()
    assert samples.shape[:2] == (12, 64) and np.isnan(samples[~complete]).all() and np.isfinite(samples[complete]).all()
    pooled = fit.missing_handler.last_posterior_samples
    assert tuple(pooled.shape) == (2, 300, len(qcols) // 3)
    want = np.quantile(pooled.cpu().numpy().astype(np.float64), [0.16, 0.5, 0.84], axis=1)      # (Q, 2, D)
    got = tab.loc[~complete, qcols].to_numpy().reshape(2, -1, 3)
    want = want.transpose(1, 2, 0)
    assert (np.abs(got - want) <= 1e-6 * (1.0 + np.abs(want))).all()                           # float32 results
    # an object too far from the library in its observed bands fails: NaN quantiles, still flagged
    far = cat.copy()
    far[3, [c for c in range(C_) if c != 1]] += 1e4
    tab3 = fit.fit_catalogue(far, num_samples=64, seed=5, missing_data_flag=np.nan, missing_data_mcmc=True,
                             missing_data_mcmc_params=dict(params, fallback_k=10), missing_data_sigma=0.5)
    assert np.isnan(tab3.loc[3, qcols].to_numpy(dtype=float)).all() and bool(tab3["has_missing_data"][3])


def test_handler_chunks_give_the_same_draws(fitted):
    from synference_amd.missing import MissingPhotometryHandler
    fit, x = fitted
    B = x.shape[1]
    rows = x[20:26].copy()
    miss = np.zeros((6, B), bool)
    miss[np.arange(6), np.arange(6) % B] = True
    rows[miss] = np.nan
    sig = np.full((6, B), 0.5, np.float32)
    rp = {"nmc": 4, "nposterior": 32}
    h = MissingPhotometryHandler.init_from_synference(fit, run_params=rp)
    a = h.process_catalogue(rows, sig, miss, seed=9)
    small = MissingPhotometryHandler.init_from_synference(fit, run_params=rp, draw_budget_bytes=1)     # one object per chunk
    b = small.process_catalogue(rows, sig, miss, seed=9)
    assert a["success"].all() and np.array_equal(a["quantiles"], b["quantiles"])
    assert np.array_equal(a["reconstructed_photometry"], b["reconstructed_photometry"], equal_nan=True)
    one = h.process_observation({"mags_sbi": rows[2], "mags_unc_sbi": sig[2], "missing_mask": miss[2]}, seed=9)
    assert one["success"] and one["posterior_samples"].shape == (4 * 32, a["quantiles"].shape[1]) and one["count"] == 4
    assert one["imputed_vectors"].shape == (4, B) and np.isfinite(one["reconstructed_photometry"]).all()
    late = MissingPhotometryHandler.init_from_synference(fit, run_params=dict(rp, tmax_all=1e-9))
    c = late.process_catalogue(rows, sig, miss, seed=9)
    assert c["timeout"][1:].all() and not c["success"][1:].any()
