"""The out-of-distribution check without a GPU: the numpy model (tests/ood_model.py) against what scikit-learn and scipy
recorded on the same inputs (tests/golden/ood/ood_*.npz, written by tests/golden/make_ood_golden.py), the margins of the shared
fixtures, and every refusal that comes before the device is touched."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import ood_model as OM

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ood")


def _gold(name):
    g = np.load(os.path.join(GOLD, f"ood_{name}.npz"))
    return g, g["base"], g["query"], int(g["k"])


@pytest.mark.parametrize("name", list(OM.CASES))
def test_fixture_is_the_generators(name):
    g, base, query, k = _gold(name)
    N, Cn, M, kk = OM.CASES[name]
    assert base.shape == (N, Cn) and query.shape == (M, Cn) and k == kk and base.dtype == np.float32
    assert abs(float(base.mean()) - 25.0) < 0.5


@pytest.mark.parametrize("name", list(OM.CASES))
def test_lof_model_is_sklearns(name):
    g, base, query, k = _gold(name)
    r = OM.detect_outliers(base, query, "lof", contamination=0.1, n_neighbors=k)
    err = np.abs(r["decision"] - g["lof_decision"]).max()
    print(f"{name}: LOF decision max |model - sklearn| = {err:.3g}, offset {r['offset']} (sklearn {float(g['lof_offset'])})")
    assert err <= 1e-6 and abs(r["offset"] - float(g["lof_offset"])) <= 1e-6
    assert np.allclose(OM.lof_fit(base, k)["nof"][:64], g["lof_nof_head"], rtol=0, atol=1e-6)
    assert np.array_equal(r["outlier_mask"], g["lof_decision"] < 0) and np.array_equal(r["scores"], -r["decision"])


@pytest.mark.parametrize("name", list(OM.CASES))
def test_neighbour_models_are_sklearns(name):
    g, base, query, k = _gold(name)
    d64, idx64, _ = OM.knn_f64(base, query, k)
    assert np.allclose(d64, g["nn_dist"], rtol=1e-9, atol=0)
    d2, idx = OM.knn_f32(base, query, k)
    assert np.array_equal(idx, idx64)                     # these fixtures have no float32 near-ties
    assert np.allclose(np.sqrt(d2.astype(np.float64)), g["nn_dist"], rtol=2e-6, atol=0)
    assert (np.diff(d2, axis=1) >= 0).all()
    ds, _, _ = OM.knn_f64(base, base, k, exclude_self=True)
    assert np.allclose(ds[:, -1], g["nn_self_kth"], rtol=1e-9, atol=0)
    d2s, idxs = OM.knn_f32(base[:200], base[:50], 3, exclude_self=1)
    assert (idxs != np.arange(50)[:, None]).all()
    part = OM.knn_f32(base[:200], base[20:50], 3, exclude_self=1, self_offset=20)
    assert np.array_equal(part[1], idxs[20:]) and np.array_equal(part[0].view(np.uint32), d2s[20:].view(np.uint32))


def test_neighbour_model_ties_and_nan():
    base = np.array([[1.0], [np.nan], [1.0], [3.0], [1.0]], np.float32)
    d2, idx = OM.knn_f32(base, np.array([[1.0]], np.float32), 5)
    assert idx.tolist() == [[0, 2, 4, 3, 1]] and d2[0, :3].tolist() == [0, 0, 0] and np.isinf(d2[0, 4])


@pytest.mark.parametrize("name", list(OM.CASES))
def test_kde_model_is_scipys(name):
    g, base, query, k = _gold(name)
    bw, qw, lognorm, factor = OM.kde_whiten(base, query, None, np.float64)
    err = np.abs(OM.kde_logsumexp(qw, bw) - lognorm - np.log(g["kde_density"])).max()
    print(f"{name}: log-density max |model - scipy| = {err:.3g}")
    assert err <= 1e-9 and abs(factor - float(g["kde_factor"])) < 1e-15
    r = OM.detect_outliers(base, query, "kde")
    assert abs(r["threshold_used"] / float(g["kde_base_percentile"]) - 1) < 1e-4
    # rounding the whitened rows to float32 (what the device is given) stays inside the stated input term
    bw32, qw32, _, _ = OM.kde_whiten(base, query)
    assert (np.abs(OM.kde_logsumexp(qw32, bw32) - OM.kde_logsumexp(qw, bw)) <= OM.kde_input_term(qw32, bw32)).all()


@pytest.mark.parametrize("name", list(OM.CASES))
def test_fixture_margins(name):
    g, base, query, k = _gold(name)
    for pyod, methods in ((False, ("lof", "kde", "mahalanobis", "pca")), (True, ("knn", "lof", "kde"))):
        for m in methods:
            und = OM.fixture_undecidable(base, query, m, None, pyod=True) if pyod else \
                OM.fixture_undecidable(base, query, m, k, n_components=base.shape[1] - 1)
            print(f"{name} {'pyod ' if pyod else ''}{m}: {int(und.sum())} of {len(und)} rows undecidable")
            assert und.mean() <= 0.05


@pytest.mark.parametrize("name", list(OM.CASES))
def test_quantile_functions(name):
    from synference_amd import ood
    g, base, _, _ = _gold(name)
    N, Cn = base.shape
    assert abs(ood.chi2_ppf(0.95, Cn) / float(g["chi2_ppf"]) - 1) < 1e-10
    assert abs(ood.f_ppf(0.95, Cn, N - Cn) / float(g["f_ppf"]) - 1) < 1e-10
    assert abs(OM._chi2_ppf(0.95, Cn) / float(g["chi2_ppf"]) - 1) < 1e-10


def test_combination_rules():
    m = np.array([[1, 0, 0], [1, 1, 0], [1, 1, 1], [0, 0, 0]], bool)
    assert OM.combine(m, "majority").tolist() == [False, True, True, False]
    assert OM.combine(m[:, :2], "majority").tolist() == [True, True, True, False]      # sum >= len / 2: one of two is enough
    assert OM.combine(m, "any").tolist() == [True, True, True, False] and OM.combine(m, "all").tolist() == [False, False, True, False]


def test_abi_refuses_bad_arguments(lib):
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)          # never dereferenced: the argument checks come first

    def knn(N=100, Cn=8, M=3, k=5, ex=0, off=0, base=p, query=p, d2=p, idx=p):
        return lib.sf_knn(base, N, Cn, query, M, k, ex, off, d2, idx, None)
    for kw in (dict(k=0), dict(k=65), dict(Cn=0), dict(Cn=65), dict(N=4), dict(N=5, ex=1), dict(N=0), dict(N=2 ** 31), dict(M=-1),
               dict(ex=2), dict(ex=1, off=98), dict(off=-1), dict(base=None), dict(query=None), dict(d2=None), dict(idx=None)):
        assert knn(**kw) == -1, kw                                    # SF_ERR_INVALID
        assert b"sf_knn" in lib.sf_last_error()

    def kde(N=100, Cn=8, M=3, base=p, query=p, out=p):
        return lib.sf_kde_logsumexp(base, N, Cn, query, M, out, None)
    for kw in (dict(Cn=0), dict(Cn=65), dict(N=0), dict(N=2 ** 31), dict(M=-1), dict(base=None), dict(query=None), dict(out=None)):
        assert kde(**kw) == -1, kw
        assert b"sf_kde_logsumexp" in lib.sf_last_error()
    assert knn(M=0) == 0 and kde(M=0) == 0                             # nothing to do is not an error


def test_python_refusals_come_before_the_device():
    from synference_amd import SBI_Fitter, ood
    base, obs = np.zeros((30, 3), np.float32), np.zeros((4, 3), np.float32)
    for m in ood.NOT_BUILT:
        with pytest.raises(ValueError, match="mahalanobis.*lof"):
            ood.detect_outliers(base, obs, method=m)
    with pytest.raises(ValueError, match="Unknown method"):
        ood.detect_outliers(base, obs, method="nope")
    with pytest.raises(ValueError, match="same number of features"):
        ood.detect_outliers(base, obs[:, :2], method="lof")
    with pytest.raises(ValueError, match="knn.*lof.*kde"):
        ood.detect_outliers_pyod(base, obs, methods=["ecod"])
    with pytest.raises(ValueError, match="Combination"):
        ood.detect_outliers_pyod(base, obs, methods="knn", combination="most")
    with pytest.raises(ValueError, match="same number of features"):
        ood.detect_outliers_pyod(base, obs[:, :2])
    f = SBI_Fitter("ood", ["a"], feature_array=base, feature_names=["x", "y", "z"], parameter_array=np.zeros((30, 1)))
    with pytest.raises(ValueError, match="feature_breakdown"):
        f.test_in_distribution(obs, feature_breakdown=True)
    with pytest.raises(ValueError, match="not built"):
        f.test_in_distribution(obs, method="robust_mahalanobis")
    with pytest.raises(TypeError):
        f.test_in_distribution(obs.tolist(), method="lof")
    with pytest.raises(TypeError):
        f.test_in_distribution_pyod(obs.tolist())
    with pytest.raises(AssertionError):
        f.test_in_distribution(obs, method="lof", direction="sideways")
    with pytest.raises(ValueError, match="knn.*lof.*kde"):
        f.test_in_distribution_pyod(obs, methods=["lof", "isolation_forest"])
    sig = inspect.signature(SBI_Fitter.fit_catalogue).parameters
    assert sig["check_out_of_distribution"].default is False and sig["outlier_methods"].default is None
    sig = inspect.signature(ood.detect_outliers).parameters
    assert [sig[n].default for n in ("method", "contamination", "n_neighbors", "threshold", "confidence", "n_components", "plot")] \
        == ["mahalanobis", 0.1, 20, None, 0.95, None, True]
    sig = inspect.signature(ood.detect_outliers_pyod).parameters
    assert sig["combination"].default == "majority" and sig["return_scores"].default is False


def test_no_cpu_fallback():
    import torch
    from synference_amd import ood
    x = torch.zeros((30, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ood.knn(x, x[:4], 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ood.kde_logsumexp(x, x[:4])
