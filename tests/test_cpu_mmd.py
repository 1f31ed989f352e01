"""The MMD misspecification test without a GPU: the numpy model (tests/mmd_model.py) against itself -- the row-sum identity
against the direct three blocks --, the decidability of the named cases (tests/mmd_cases.py), the keyed subsets, the bandwidth,
and every refusal that comes before the device is touched."""
import ctypes as C
import inspect

import numpy as np
import pytest

import mmd_cases as MC
import mmd_model as MM


def test_identity_is_the_direct_evaluation():
    z, z_obs, n_shuffle, seed = MC.make_case("edge")
    N, M = len(z), len(z_obs)
    K, _ = MM.kernel(z, z, MC.scale("edge"))
    worst = 0.0
    for S in MC.subsets("edge").astype(np.int64):
        T = np.setdiff1d(np.arange(N), S)
        direct = MM.mmd2(*MM.mmd2_blocks(K, S, T), M, N - M)
        ident = MM.mmd2(*MM.identity_blocks(K, S), M, N - M)
        worst = max(worst, abs(direct - ident))
    print(f"edge: max |identity - direct| over {n_shuffle} shuffles = {worst:.3g}")
    assert worst <= 1e-12


@pytest.mark.parametrize("name", list(MC.CASES))
def test_cases_are_decidable(name):
    """No null value lies within (its bound + the observed bound) of the observed statistic, so the device's p-value -- any
    device inside the bounds -- equals the model's."""
    m = MC.model(name)
    z, z_obs, n_shuffle, _ = MC.make_case(name)
    N, Cn, M = MC.CASES[name][:3]
    assert z.shape == (N, Cn) and z_obs.shape == (M, Cn) and z.dtype == np.float32 and len(m["null"]) == n_shuffle
    print(f"{name}: p_value {m['p_value']:.3f}  mmd2 {m['mmd2']:.4g}  negative null squares {np.mean(m['null'] < 0):.3f}  "
          f"smallest gap {m['smallest_gap']:.3g}  largest combined bound {m['largest_bound']:.3g}")
    assert m["undecidable"] == 0
    assert (m["null_b"] > 0).all() and m["mmd2_b"] > 0


def test_dups_case_is_by_position():
    z, z_obs, _, _ = MC.make_case("dups")
    assert np.array_equal(z[250:], z[:50]) and np.array_equal(z_obs[:10], z[100:110])
    m = MC.model("dups")
    K, _ = MM.kernel(z, z, MC.scale("dups"))
    assert K[0, 250] == 1.0 and abs(m["r"][0] - (K[0].sum() - 1.0)) < 1e-12      # the copy counts, the row itself does not


def test_counting_case_on_the_model():
    m = MC.model("edge", True)
    N, _, M = MC.CASES["edge"][:3]
    assert np.abs(m["r"] - (N - 1)).max() <= (N - 1) * 2.0 ** -22
    assert np.abs(m["pair"] - M * (M - 1)).max() <= M * (M - 1) * 2.0 ** -22
    assert abs(m["Cx_o"] - M * N) <= M * N * 2.0 ** -22 and abs(m["A_o"] - M * (M - 1)) <= M * (M - 1) * 2.0 ** -22


def test_keyed_subsets():
    from synference_amd import misspecification as MS
    from synference_amd.lc2st import _mix
    for N, m in ((333, 41), (130, 2), (17, 17), (4097, 100)):
        s = MS.mmd_subsets(7, 5, N, m)
        assert s.shape == (5, m) and s.dtype == np.int32 and s.min() >= 0 and s.max() < N
        assert all(len(np.unique(row)) == m for row in s)
        assert not np.array_equal(s, MS.mmd_subsets(8, 5, N, m))
        assert np.array_equal(s[2:4], MS.mmd_subsets(7, 2, N, m, first=2))
        # the first-m shortcut is the first m entries of the full bijection, written out on its own here
        key = MS._set_keys(7, [3])[:, 0]
        hb = MS._half_bits(N)
        full = np.empty(N, np.int64)
        for j in range(N):
            x = j
            while True:
                L, R = x >> hb, x & ((1 << hb) - 1)
                for r in range(4):
                    with np.errstate(over="ignore"):
                        L, R = R, L ^ (int(_mix(np.uint32(R) ^ key[r])) & ((1 << hb) - 1))
                x = (L << hb) | R
                if x < N:
                    break
            full[j] = x
        assert sorted(full.tolist()) == list(range(N)) and np.array_equal(full[:m], s[3])
    with pytest.raises(ValueError):
        MS.mmd_subsets(0, 1, 10, 11)


def test_rbf_scale_is_the_median_of_the_models_distances():
    from synference_amd import misspecification as MS
    for name in ("edge", "wide", "one"):
        z, _, _, seed = MC.make_case(name)
        got = MS.rbf_scale(z, seed)
        assert abs(got / MC.scale(name) - 1) <= 1e-12, (name, got, MC.scale(name))
    rng = np.random.default_rng(0)
    big = rng.normal(size=(2100, 2)).astype(np.float32)                      # more than 2048 rows: the keyed first 2048
    pick = MS.mmd_subsets(5, 1, 2100, 2048, first=MS.SET_SCALE)[0]
    assert abs(MS.rbf_scale(big, 5) / MM.scale_model(big, pick) - 1) <= 1e-12
    assert MS.c2_of(2.0) == float(np.float32(-0.125 * 1.4426950408889634))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            MS.c2_of(bad)


def test_abi_refuses_bad_arguments(lib):
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)          # never dereferenced: the argument checks come first

    def rowsum(N=100, Cn=8, M=3, c2=-1.0, ex=0, off=0, base=p, query=p, out=p):
        return lib.sf_rbf_rowsum(base, N, Cn, query, M, c2, ex, off, out, None)
    for kw in (dict(Cn=0), dict(Cn=65), dict(N=0), dict(N=2 ** 31), dict(M=-1), dict(ex=2), dict(ex=-1), dict(ex=1, off=98),
               dict(off=-1), dict(c2=1e-3), dict(c2=float("nan")), dict(c2=float("-inf")), dict(c2=float("inf")),
               dict(base=None), dict(query=None), dict(out=None)):
        assert rowsum(**kw) == -1, kw                                    # SF_ERR_INVALID
        assert b"sf_rbf_rowsum" in lib.sf_last_error()

    def subset(N=100, Cn=8, n_sets=3, m=5, c2=-1.0, rows=p, idx=p, rowsum=p, pair=p, picked=p):
        return lib.sf_rbf_subset_sums(rows, N, Cn, idx, n_sets, m, c2, rowsum, pair, picked, None)
    for kw in (dict(Cn=0), dict(Cn=65), dict(N=0), dict(N=2 ** 31), dict(n_sets=-1), dict(m=1), dict(m=0), dict(m=101),
               dict(c2=1e-3), dict(c2=float("nan")), dict(c2=float("-inf")), dict(rows=None), dict(idx=None), dict(pair=None),
               dict(rowsum=None), dict(picked=None)):                       # (rowsum without picked_rowsum and the reverse)
        assert subset(**kw) == -1, kw
        assert b"sf_rbf_subset_sums" in lib.sf_last_error()
    assert all(v == 0.0 for v in buf)                                     # the outputs stay untouched
    assert rowsum(M=0) == 0 and subset(n_sets=0) == 0                    # nothing to do is not an error
    assert subset(n_sets=0, rowsum=None, picked=None) == 0


def test_python_refusals_come_before_the_device():
    from synference_amd import SBI_Fitter
    from synference_amd import misspecification as MS
    x, xo = np.zeros((30, 3), np.float32), np.ones((4, 3), np.float32)
    with pytest.raises(ValueError, match="M >= 2"):
        MS.calc_misspecification_mmd(None, xo[:1], x)
    with pytest.raises(ValueError, match="M >= 2"):
        MS.calc_misspecification_mmd(None, x[:29], x)                      # N < M + 2
    with pytest.raises(ValueError, match="features"):
        MS.calc_misspecification_mmd(None, xo[:, :2], x)
    bad = xo.copy()
    bad[1, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        MS.calc_misspecification_mmd(None, bad, x)
    with pytest.raises(ValueError, match="non-finite"):
        MS.calc_misspecification_logprob(x, bad, None)
    with pytest.raises(ValueError, match="mode"):
        MS.calc_misspecification_mmd(None, xo, x, mode="latent")
    with pytest.raises(ValueError, match="embedding"):
        MS.calc_misspecification_mmd(None, xo, x, mode="embedding")
    with pytest.raises(ValueError, match="at most 64"):
        MS.calc_misspecification_mmd(None, np.zeros((4, 65), np.float32), np.zeros((30, 65), np.float32))
    with pytest.raises(ValueError, match="two-dimensional"):
        MS.calc_misspecification_mmd(None, xo[0], x)
    with pytest.raises(ValueError, match="NSF"):
        MS.MarginalTrainer(density_estimator="MDN")
    with pytest.raises(ValueError, match="D <= 16.*mmd"):
        MS.MarginalTrainer().append_samples(np.zeros((10, 17), np.float32))
    with pytest.raises(ValueError, match="append_samples"):
        MS.MarginalTrainer().train()
    f = SBI_Fitter("mis", ["a"], feature_array=x, feature_names=["x", "y", "z"], parameter_array=np.zeros((30, 1)))
    with pytest.raises(ValueError, match="No training data found. Please set the training data first."):
        f.detect_misspecification(xo)
    with pytest.raises(ValueError, match="Unknown method"):
        f.detect_misspecification(xo, X_train=x, method="c2st")
    with pytest.raises(ValueError, match="D <= 16.*mmd"):
        f.detect_misspecification(np.zeros((4, 17), np.float32), X_train=np.zeros((30, 17), np.float32))
    with pytest.raises(ValueError, match="embedding"):
        f.detect_misspecification(xo, X_train=x, method="mmd", mode="embedding")
    assert f.last_misspecification is None and f.marginal_trainer_est is None


def test_no_cpu_fallback(monkeypatch):
    import torch
    from synference_amd import misspecification as MS
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # (host tensors below: nothing reaches a device)
    x, xo = np.random.default_rng(0).normal(size=(30, 3)).astype(np.float32), np.ones((4, 3), np.float32)
    t = torch.as_tensor(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MS.rbf_rowsum(t, t[:4], -1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MS.rbf_subset_sums(t, torch.zeros((2, 3), dtype=torch.int32), -1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MS.mmd2_unbiased(t, t[:4], 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MS.calc_misspecification_mmd(None, xo, x)
    tr = MS.MarginalTrainer().append_samples(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.train()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MS.calc_misspecification_logprob(x, xo, None)


def test_signature_defaults():
    from synference_amd import SBI_Fitter
    from synference_amd import misspecification as MS
    sig = inspect.signature(MS.calc_misspecification_mmd).parameters
    assert list(sig)[:5] == ["inference", "x_obs", "x", "mode", "n_shuffle"]
    assert [sig[n].default for n in ("mode", "n_shuffle", "scale", "z_score", "max_train", "seed", "alpha", "return_details")] \
        == ["x_space", 1000, None, True, None, 0, 0.05, False]
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("scale", "z_score", "max_train", "seed", "alpha",
                                                                       "return_details"))
    sig = inspect.signature(MS.calc_misspecification_logprob).parameters
    assert list(sig) == ["x_train", "x_o", "estimator", "alpha"] and sig["alpha"].default == 0.05
    assert inspect.signature(MS.MarginalTrainer.__init__).parameters["density_estimator"].default == "NSF"
    assert MS.MarginalTrainer().build_kwargs == dict(backend="lampe", num_transforms=5, hidden_features=50)
    sig = inspect.signature(MS.MarginalTrainer.train).parameters
    assert [sig[n].default for n in ("training_batch_size", "learning_rate", "validation_fraction", "stop_after_epochs",
                                     "max_num_epochs", "clip_max_norm", "seed")] == [200, 5e-4, 0.1, 20, 2 ** 31 - 1, 5.0, None]
    assert inspect.signature(MS.rbf_scale).parameters["seed"].default == 0
    sig = inspect.signature(SBI_Fitter.detect_misspecification).parameters
    assert list(sig)[:4] == ["self", "x_obs", "X_train", "retrain"]
    assert [sig[n].default for n in ("X_train", "retrain", "method", "alpha", "seed", "plot")] == [None, False, "logprob", 0.05,
                                                                                                 None, False]
