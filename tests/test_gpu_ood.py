"""The out-of-distribution check on the device (csrc/sf_ood.hip, synference_amd/ood.py, SBI_Fitter.test_in_distribution*,
fit_catalogue(check_out_of_distribution=True)) against the numpy model (tests/ood_model.py) and the values scikit-learn and
scipy recorded (tests/golden/ood/ood_*.npz).

sf_knn goes through the C ABI with sentinel-filled outputs: rows and distance BITS must equal the model's.  sf_kde_logsumexp
is compared on the same whitened float32 inputs with |delta| <= 2e-5 (v_exp_f32: (|a| + 2) 2^-23 per term, terms beyond
|a| = 30 weigh below 1e-13; ordered fp64 sums).  At the Python level scores carry rtol 1e-5, a KDE log-density the bound above
plus the input-rounding term, and masks must be equal except on rows the model marks undecidable (tests/test_cpu_ood.py
asserts that the fixtures have at most 5 % of those)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import ood_model as OM

pytestmark = pytest.mark.gpu

SENT_F, SENT_I = -7.5, -77
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ood")


def _p(t):
    return C.c_void_p(t.data_ptr())


def _knn_raw(base, query, k, exclude_self=0, self_offset=0, check=True):
    from synference_amd import _lib
    lib = _lib.load()
    b, q = torch.tensor(base).cuda(), torch.tensor(query).cuda()
    M = len(query)
    d2 = torch.full((M, max(k, 1)), SENT_F, device="cuda")
    idx = torch.full((M, max(k, 1)), SENT_I, dtype=torch.int32, device="cuda")
    rc = lib.sf_knn(_p(b), base.shape[0], base.shape[1], _p(q), M, k, exclude_self, self_offset, _p(d2), _p(idx),
                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    if check:
        _lib.check(rc)
    return rc, d2.cpu().numpy(), idx.cpu().numpy()


def _kde_raw(base_w, query_w):
    from synference_amd import _lib
    lib = _lib.load()
    b, q = torch.tensor(base_w).cuda(), torch.tensor(query_w).cuda()
    out = torch.full((len(query_w),), SENT_F, dtype=torch.float64, device="cuda")
    _lib.check(lib.sf_kde_logsumexp(_p(b), base_w.shape[0], base_w.shape[1], _p(q), len(query_w), _p(out),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(N, Cn, M, k, kind):
    base, query = OM.make_case(N, Cn, M, seed=N + Cn)
    if kind == "self":
        query = base.copy()
    if kind == "ties":      # 40 duplicated base rows, 10 queries that are base rows, one base row with a NaN
        base[100:140] = base[600:640]
        query[5:15] = base[[7, 100, 600, 101, 601, 1030, 0, 333, 139, 639]]
        base[500, 3] = np.nan
    return base, query


KNN_CASES = [(2500, 7, 70, 20, "plain"), (300, 3, 33, 5, "plain"), (257, 1, 1, 1, "plain"), (21, 20, 21, 20, "self"),
             (64, 64, 5, 64, "plain"), (1031, 20, 130, 32, "ties")]


@functools.lru_cache(maxsize=None)
def _knn_pair(case):
    N, Cn, M, k, kind = case
    base, query = _case(*case)
    ex = 1 if kind == "self" else 0
    return _knn_raw(base, query, k, ex)[1:], OM.knn_f32(base, query, k, ex)


@pytest.mark.parametrize("case", KNN_CASES, ids=["x".join(map(str, c)) for c in KNN_CASES])
def test_knn_is_the_models_bit_for_bit(case):
    (d2, idx), (md2, midx) = _knn_pair(case)
    assert np.array_equal(idx, midx)
    assert np.array_equal(d2.view(np.uint32), md2.view(np.uint32))


@pytest.mark.parametrize("case", KNN_CASES, ids=["x".join(map(str, c)) for c in KNN_CASES])
def test_knn_pairs_are_consistent_without_the_selection_model(case):
    N, Cn, M, k, kind = case
    base, query = _case(*case)
    (d2, idx), _ = _knn_pair(case)
    assert ((idx >= 0) & (idx < N)).all()
    full = OM.d2_f32(query, base)
    assert np.array_equal(np.take_along_axis(full, idx.astype(np.int64), 1).view(np.uint32), d2.view(np.uint32))
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    assert (key[:, 1:] > key[:, :-1]).all() and all(len(set(r)) == k for r in idx.tolist())
    if kind == "self":
        assert (idx != np.arange(M)[:, None]).all()
    if kind == "ties":
        assert (d2[5:15, 0] == 0).all() and idx[5:15, 0].tolist() == [7, 100, 100, 101, 101, 1030, 0, 333, 139, 139]
        assert not (idx == 500).any()


def test_knn_scratch_reuse_across_sizes():
    """Small, large, small again: the scratch grows, serves a smaller layout from the larger buffer, then one of equal size."""
    small, large = KNN_CASES[2], KNN_CASES[0]
    first, second, third = (_knn_raw(*_case(*c), c[3])[1:] for c in (small, large, small))
    for u, v in zip(first, third):
        assert u.tobytes() == v.tobytes()
    for case, (d2, idx) in ((small, first), (large, second)):
        md2, midx = _knn_pair(case)[1]
        assert np.array_equal(idx, midx) and np.array_equal(d2.view(np.uint32), md2.view(np.uint32))


def test_knn_two_calls_on_two_streams():
    """Two sf_knn calls queued back to back on two streams, with no host synchronisation in between; different data and
    shapes, so that the second call carves the shared scratch differently.  Each result must equal that call's result when it
    runs alone.  This walks the wait-and-record path of the scratch (the second call's stream waits for the event the first
    call recorded).  It is not a detector: a lost ordering would not fail reliably, and the test must never be looped to
    make it fail."""
    from synference_amd import _lib
    lib = _lib.load()
    cases = [KNN_CASES[0], KNN_CASES[5]]
    alone = [_knn_pair(c)[0] for c in cases]
    bufs = []
    for c in cases:
        base, query = _case(*c)
        bufs.append((torch.tensor(base).cuda(), torch.tensor(query).cuda(), torch.full((c[2], c[3]), SENT_F, device="cuda"),
                     torch.full((c[2], c[3]), SENT_I, dtype=torch.int32, device="cuda")))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for c, (b, q, d2, idx), st in zip(cases, bufs, streams):
        with torch.cuda.stream(st):
            _lib.check(lib.sf_knn(_p(b), c[0], c[1], _p(q), c[2], c[3], 0, 0, _p(d2), _p(idx), C.c_void_p(st.cuda_stream)))
    for st in streams:
        st.synchronize()
    for (b, q, d2, idx), (ad2, aidx) in zip(bufs, alone):
        assert np.array_equal(idx.cpu().numpy(), aidx) and d2.cpu().numpy().tobytes() == ad2.tobytes()


def test_knn_does_not_depend_on_the_split_over_queries():
    case = KNN_CASES[0]
    base, query = _case(*case)
    (d2, idx), _ = _knn_pair(case)
    for lo, hi in ((0, 17), (17, 70)):
        _, pd2, pidx = _knn_raw(base, query[lo:hi], case[3])
        assert np.array_equal(pidx, idx[lo:hi]) and np.array_equal(pd2.view(np.uint32), d2[lo:hi].view(np.uint32))


def test_knn_self_mode_split_with_self_offset():
    base, _ = _case(*KNN_CASES[1])
    _, d2, idx = _knn_raw(base, base, 5, 1)
    md2, midx = OM.knn_f32(base, base, 5, 1)
    assert np.array_equal(idx, midx) and np.array_equal(d2.view(np.uint32), md2.view(np.uint32))
    for lo, hi in ((0, 129), (129, 300)):
        _, pd2, pidx = _knn_raw(base, base[lo:hi], 5, 1, lo)
        assert np.array_equal(pidx, idx[lo:hi]) and np.array_equal(pd2.view(np.uint32), d2[lo:hi].view(np.uint32))


def test_knn_many_queries_against_a_long_base():
    """More than one query tile and more than one split of the base in the same call."""
    rng = np.random.default_rng(5)
    base = (25 + rng.normal(size=(9000, 5))).astype(np.float32)
    query = (25 + rng.normal(size=(300, 5))).astype(np.float32)
    for k in (3, 17, 40):                                  # the three workgroup sizes
        _, d2, idx = _knn_raw(base, query, k)
        md2, midx = OM.knn_f32(base, query, k)
        assert np.array_equal(idx, midx) and np.array_equal(d2.view(np.uint32), md2.view(np.uint32))


def test_knn_every_row_at_the_bound_distance():
    """40 000 identical base rows: every split's list is full of rows at the bound distance, so the combine kernel has more
    real entries than it packs into LDS and takes its binary-search path; ties go to the lowest rows."""
    base = np.full((40000, 2), 25.0, np.float32)
    base[::7, 1] = 25.5                                     # two distances, interleaved over all splits
    query = np.array([[25.0, 25.0], [25.0, 25.5], [24.0, 26.0]], np.float32)
    _, d2, idx = _knn_raw(base, query, 64)
    md2, midx = OM.knn_f32(base, query, 64)
    assert np.array_equal(idx, midx) and np.array_equal(d2.view(np.uint32), md2.view(np.uint32))
    assert idx[1].tolist() == list(range(0, 64 * 7, 7))


def test_knn_refusals_leave_the_outputs_alone():
    base, query = _case(*KNN_CASES[1])
    wide = np.zeros((10, 65), np.float32)
    for b, q, k, ex in ((base, query, 0, 0), (base, query, 65, 0), (wide, wide, 3, 0), (base[:4], query, 5, 0),
                        (base[:5], base[:5], 5, 1)):
        rc, d2, idx = _knn_raw(b, q, k, ex, check=False)
        assert rc == -1 and (d2 == SENT_F).all() and (idx == SENT_I).all()


@pytest.mark.parametrize("name", list(OM.CASES))
def test_kde_logsumexp_against_the_fp64_model(name):
    g = np.load(os.path.join(GOLD, f"ood_{name}.npz"))
    bw, qw, _, _ = OM.kde_whiten(g["base"], g["query"])
    for b, q in ((bw, qw), (bw, bw[:257])):
        dev = _kde_raw(b, q)
        err = np.abs(dev - OM.kde_logsumexp(q, b)).max()
        print(f"{name}: sf_kde_logsumexp max |device - fp64 model| = {err:.3g} over {len(q)} rows")
        assert err <= OM.KDE_ATOL
        assert np.array_equal(dev, _kde_raw(b, q))         # two calls: the same bits


def test_kde_logsumexp_long_base_and_nan_row():
    rng = np.random.default_rng(9)
    b = rng.normal(size=(20000, 4)).astype(np.float32)     # several splits
    q = (2.0 * rng.normal(size=(40, 4))).astype(np.float32)
    dev = _kde_raw(b, q)
    assert np.abs(dev - OM.kde_logsumexp(q, b)).max() <= OM.KDE_ATOL and np.array_equal(dev, _kde_raw(b, q))
    b2 = b.copy()
    b2[77, 1] = np.nan                                     # a NaN row is a zero term
    keep = np.ones(len(b), bool)
    keep[77] = False
    assert np.abs(_kde_raw(b2, q) - OM.kde_logsumexp(q, b[keep])).max() <= OM.KDE_ATOL


# ---- Python level -----------------------------------------------------------------------------------------------------------
def _gold(name):
    g = np.load(os.path.join(GOLD, f"ood_{name}.npz"))
    return g, g["base"], g["query"], int(g["k"])


def _same_masks(dev_mask, model_mask, und, what):
    diff = np.asarray(dev_mask) != np.asarray(model_mask)
    print(f"{what}: {int(diff.sum())} masks differ, {int(np.asarray(und).sum())} rows undecidable")
    assert not (diff & ~und).any()


@pytest.mark.parametrize("name", list(OM.CASES))
def test_detect_outliers_against_model_and_recorded_values(name):
    from synference_amd import ood
    g, base, query, k = _gold(name)
    fb = ood.FittedBase(base)
    for method in ("mahalanobis", "hotelling_t2", "pca", "lof"):
        thr = float(g["f_ppf"]) if method == "hotelling_t2" else None
        nc = base.shape[1] - 1                   # (all components, the default, reconstruct exactly: scores of rounding noise)
        mod = OM.detect_outliers(base, query, method, contamination=0.1, n_neighbors=k, threshold=thr, n_components=nc)
        dev = ood.detect_outliers(fb, query, method=method, contamination=0.1, n_neighbors=k, n_components=nc, plot=False)
        for key in ("outlier_mask", "scores", "threshold_used", "method_info"):
            assert key in dev
        ref = mod["scores"] if method != "lof" else -(mod["decision"] + mod["offset"])     # LOF itself, not its small difference
        got = dev["scores"] if method != "lof" else dev["scores"] - mod["offset"]
        rel = np.abs(got / ref - 1).max()
        print(f"{name} {method}: scores max rel {rel:.3g}, threshold {dev['threshold_used']} (model {mod['threshold_used']})")
        assert rel <= OM.RTOL
        assert abs(dev["threshold_used"] - mod["threshold_used"]) <= 1e-6 * abs(mod["threshold_used"])
        _same_masks(dev["outlier_mask"], mod["outlier_mask"], OM.fixture_undecidable(base, query, method, k, n_components=nc, threshold=thr),
                    f"{name} {method}")
    dev = ood.detect_outliers(fb, query, method="lof", contamination=0.1, n_neighbors=k, plot=False)
    assert np.abs((dev["scores"] - float(g["lof_offset"])) / (g["lof_decision"] + float(g["lof_offset"])) + 1).max() <= OM.RTOL
    assert ("lof", k) in fb._cache and ("knn", k) in fb._cache            # the base side is kept


@pytest.mark.parametrize("name", list(OM.CASES))
def test_detect_outliers_kde(name):
    from synference_amd import ood
    g, base, query, k = _gold(name)
    mod = OM.detect_outliers(base, query, "kde")
    dev = ood.detect_outliers(base, query, method="kde", plot=False)
    bw, qw, _, _ = OM.kde_whiten(base, query)
    bound = OM.KDE_ATOL + OM.kde_input_term(qw, bw)
    # scores = -log(density + 1e-10): |d score| <= |d log density|, so the log-density bound holds for the scores of ALL rows
    # (the inflated rows' densities lie below the 1e-10 floor and cannot be taken back out of their scores)
    for what, ref in (("model", mod["density"]), ("scipy", g["kde_density"])):
        err = np.abs(dev["scores"] + np.log(ref + 1e-10))
        print(f"{name} kde score against {what}: max {err.max():.3g}, max err / bound {np.max(err / bound):.3g}")
        assert (err <= bound + 1e-9).all()
    assert abs(dev["method_info"]["kde_bandwidth"] - float(g["kde_factor"])) < 1e-12
    assert abs(np.log(dev["threshold_used"]) - np.log(float(g["kde_base_percentile"]))) <= 2e-4
    _same_masks(dev["outlier_mask"], mod["outlier_mask"], OM.fixture_undecidable(base, query, "kde", k), f"{name} kde")


@pytest.mark.parametrize("name", list(OM.CASES))
def test_detect_outliers_pyod(name):
    from synference_amd import ood
    g, base, query, k = _gold(name)
    fb = ood.FittedBase(base)
    res = ood.detect_outliers_pyod(fb, query, methods=["knn", "lof", "kde"], combination="none", return_scores=True,
                                   contamination=0.1)
    masks = []
    for j, m in enumerate(("knn", "lof", "kde")):
        sc, thr, fragile = OM.pyod_scores(base, query, m, 0.1)
        if m == "kde":
            bw, qw, _, _ = OM.kde_whiten(base, query, 1.0)
            err = np.abs(res["scores"][:, j] - sc)
            print(f"{name} pyod kde: max |score - model| {err.max():.3g}")
            assert (err <= OM.KDE_ATOL + OM.kde_input_term(qw, bw) + 1e-9).all()
        else:
            rel = np.abs(res["scores"][:, j] / sc - 1).max()
            print(f"{name} pyod {m}: scores max rel {rel:.3g}")
            assert rel <= OM.RTOL
        masks.append(sc > thr)
        _same_masks(res["outlier_mask"][:, j], masks[-1], OM.fixture_undecidable(base, query, m, None, 0.1, pyod=True),
                    f"{name} pyod {m}")
    masks = np.stack(masks, 1)
    if np.array_equal(res["outlier_mask"], masks):
        for comb in ("majority", "any", "all"):
            assert np.array_equal(ood.detect_outliers_pyod(fb, query, combination=comb, contamination=0.1), OM.combine(masks, comb))
    with pytest.raises(ValueError, match="n_neighbors"):
        ood.detect_outliers_pyod(fb, query, methods="knn", n_neighbors=65)


# ---- fitter level -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitter(tmp_path_factory):
    from synference_amd import SBI_Fitter
    from synference_amd.synthetic import make_catalogue
    x, theta, names = make_catalogue(1500, 6, 3, seed=1)
    f = SBI_Fitter("ood", names, [f"F{i}" for i in range(6)], feature_array=x, parameter_array=theta)
    f.run_single_sbi(model_type="maf", hidden_features=32, num_transforms=2, training_batch_size=256, learning_rate=2e-3,
                     stop_after_epochs=2, max_num_epochs=4, random_seed=3, out_dir=str(tmp_path_factory.mktemp("models")),
                     verbose=False, name_append="t", evaluate_model=False, save_model=False)
    obs = make_catalogue(40, 6, 3, seed=2)[0]
    planted = [3, 17, 31]       # every feature within 1.5 sigma of the library's mean, the combination far from its rows
    signs = np.array([[1, -1, 1, -1, 1, -1], [-1, 1, 1, -1, -1, 1], [1, 1, -1, -1, 1, -1]])
    obs[planted] = (x.mean(0) + 1.5 * x.std(0) * signs).astype(np.float32)
    return f, obs, planted


def test_test_in_distribution_both_directions(fitter):
    from synference_amd import ood
    f, obs, planted = fitter
    r = f.test_in_distribution(obs, method="lof", plot=False)
    assert r["outlier_mask"].shape == (40,) and r["outlier_mask"][planted].all() and r["threshold_used"] == 0
    mod = OM.detect_outliers(f.feature_array, obs, "lof")
    assert np.abs((r["scores"] - mod["offset"]) / (mod["decision"] + mod["offset"]) + 1).max() <= OM.RTOL
    base = f._ood_base()
    assert f._ood_base() is base and ("lof", 20) in base._cache
    out = f.test_in_distribution(obs, method="mahalanobis", direction="out", plot=False)
    assert out["outlier_mask"].shape == (1500,)
    assert np.allclose(out["scores"], OM.detect_outliers(obs, f.feature_array, "mahalanobis")["scores"], rtol=1e-6)
    m_in = f.test_in_distribution_pyod(obs, contamination=0.01)
    assert m_in.shape == (40,) and m_in.dtype == bool and m_in[planted].all()
    assert np.array_equal(m_in, ood.detect_outliers_pyod(f.feature_array, obs, contamination=0.01))
    assert f.test_in_distribution_pyod(obs, direction="out", methods=["knn"], contamination=0.05).shape == (1500,)
    f.feature_array = f.feature_array.copy()                        # a replaced array drops the fitted base side
    assert f._ood_base() is not base


@pytest.mark.parametrize("device_quantiles", [True, False])
def test_fit_catalogue_with_the_check(fitter, device_quantiles):
    f, obs, planted = fitter
    kw = dict(num_samples=64, seed=11, append_to_input=False, device_quantiles=device_quantiles)
    off = f.fit_catalogue(obs, **kw)
    on = f.fit_catalogue(obs, check_out_of_distribution=True, **kw)
    assert "is_outlier" not in off.columns and "is_outlier" in on.columns
    flag = on["is_outlier"].to_numpy(dtype=bool)
    assert flag[planted].all() and flag.sum() < 10
    qcols = [c for c in off.columns if c != "ID"]
    assert len(qcols) == 9
    assert np.isnan(on[qcols].to_numpy()[flag]).all()
    assert np.array_equal(on[qcols].to_numpy()[~flag], off[qcols].to_numpy()[~flag]) and np.isfinite(off[qcols].to_numpy()).all()
    fa, mask = f.fit_catalogue(obs, return_feature_array=True, check_out_of_distribution=True)
    assert fa.shape == obs.shape and np.array_equal(mask, flag)
    knn_only = f.fit_catalogue(obs, check_out_of_distribution=True, outlier_methods=["knn"], **kw)
    assert knn_only["is_outlier"].to_numpy(dtype=bool)[planted].all()


def test_fit_catalogue_check_with_missing_data_mcmc(fitter):
    f, obs, planted = fitter
    o = obs.copy()
    o[5, 2] = -99.0
    t = f.fit_catalogue(o, num_samples=64, seed=11, append_to_input=False, check_out_of_distribution=True,
                        missing_data_mcmc=True, missing_data_sigma=0.1,
                        missing_data_mcmc_params=dict(nmc=4, nposterior=32, min_neighbours=5))
    flag = t["is_outlier"].to_numpy(dtype=bool)
    assert flag[planted].all() and not flag[5] and bool(t["has_missing_data"][5])
