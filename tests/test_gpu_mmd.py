"""sf_rbf_rowsum / sf_rbf_subset_sums and calc_misspecification_mmd on the device against the float64 model
(tests/mmd_model.py) on the named cases (tests/mmd_cases.py), at the model's derived bounds: every sum within the sum of its
terms' bounds, every MMD^2 within the same linear combination, and -- the cases being decidable (tests/test_cpu_mmd.py) -- the
p-value equal to the model's."""
import numpy as np
import pytest
import torch

import mmd_cases as MC
import mmd_model as MM

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(name):
    z, z_obs, n_shuffle, seed = MC.make_case(name)
    return torch.tensor(z).to(DEV), torch.tensor(z_obs).to(DEV), n_shuffle, seed


def _ratio(got, want, bound):
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / bound))


def _sums(name, scale):
    from synference_amd import misspecification as MS
    z, zo, n_shuffle, seed = _dev(name)
    c2 = MS.c2_of(scale)
    idx = torch.as_tensor(np.array(MC.subsets(name))).to(DEV)
    r = MS.rbf_rowsum(z, z, c2, exclude_self=True)
    pair, picked = MS.rbf_subset_sums(z, idx, c2, r)
    return dict(r=r.cpu().numpy(), row_o=MS.rbf_rowsum(zo, zo, c2, exclude_self=True).cpu().numpy(),
                row_x=MS.rbf_rowsum(z, zo, c2).cpu().numpy(), pair=pair.cpu().numpy(), picked=picked.cpu().numpy())


@pytest.mark.parametrize("name", list(MC.CASES))
def test_sums_within_the_derived_bound(name):
    m, d = MC.model(name), _sums(name, MC.scale(name))
    ratios = {k: _ratio(d[k], m[k], m[k + "_b"]) for k in ("r", "row_o", "row_x", "pair", "picked")}
    print(f"{name}: worst |device - model| / bound: " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (name, k, v)
    assert abs(d["row_o"].sum() - m["A_o"]) <= m["row_o_b"].sum() and abs(d["row_x"].sum() - m["Cx_o"]) <= m["row_x_b"].sum()


@pytest.mark.parametrize("name", list(MC.CASES))
def test_mmd2_within_bound_and_p_value_is_the_models(name):
    """(z_score=False: the rows of the cases are what the model sees; test_z_score_is_the_training_rows' covers the step)"""
    from synference_amd import misspecification as MS
    m = MC.model(name)
    z, z_obs, n_shuffle, seed = MC.make_case(name)
    out = MS.calc_misspecification_mmd(None, z_obs, z, "x_space", n_shuffle, z_score=False, seed=seed, return_details=True)
    assert abs(out["scale"] / MC.scale(name) - 1) <= 1e-12
    print(f"{name}: p_value {out['p_value']} (model {m['p_value']})  mmd2 {out['mmd2']:.6g} (model {m['mmd2']:.6g})  worst "
          f"|device - model| / bound: observed {abs(out['mmd2'] - m['mmd2']) / m['mmd2_b']:.3f}  null "
          f"{_ratio(out['null_mmd2'], m['null'], m['null_b']):.3f}")
    assert abs(out["mmd2"] - m["mmd2"]) <= m["mmd2_b"]
    assert (np.abs(out["null_mmd2"] - m["null"]) <= m["null_b"]).all()
    assert out["p_value"] == m["p_value"] and out["reject"] == (m["p_value"] < 0.05)
    p, (base, mmd) = MS.calc_misspecification_mmd(None, z_obs, z, "x_space", n_shuffle, z_score=False, seed=seed)
    assert p == out["p_value"] and mmd == np.sqrt(max(out["mmd2"], 0.0))
    assert np.array_equal(base, np.sqrt(np.maximum(out["null_mmd2"], 0.0))) and np.array_equal(base, out["mmds_baseline"])
    got = MS.mmd2_unbiased(torch.tensor(z_obs).to(DEV), torch.tensor(z).to(DEV), out["scale"])
    assert abs(got - m["mmd2"]) <= m["mmd2_b"]


def test_counting_case():
    m, d = MC.model("edge", True), _sums("edge", MC.COUNT_SCALE)
    N, _, M = MC.CASES["edge"][:3]
    assert np.abs(d["r"] - (N - 1)).max() <= (N - 1) * 2.0 ** -22
    assert np.abs(d["pair"] - M * (M - 1)).max() <= M * (M - 1) * 2.0 ** -22
    assert np.abs(d["picked"] - M * (N - 1)).max() <= M * (N - 1) * 2.0 ** -22
    assert abs(d["row_x"].sum() - M * N) <= M * N * 2.0 ** -22 and abs(d["row_o"].sum() - M * (M - 1)) <= M * (M - 1) * 2.0 ** -22
    assert _ratio(d["pair"], m["pair"], m["pair_b"]) <= 1.0


def test_counting_on_many_tiles():
    """m = 16 640 positions are 65 tile rows, more than a tile row has workgroups: two tiles per workgroup.  With every term 1
    the sum is the number of ordered pairs -- a tile visited twice or not at all moves it by at least 256."""
    from synference_amd import misspecification as MS
    m = 16640
    rows = torch.as_tensor(np.random.default_rng(0).normal(size=(m + 5, 1)).astype(np.float32)).to(DEV)
    idx = torch.stack([torch.arange(m, dtype=torch.int32), torch.arange(m + 4, 4, -1, dtype=torch.int32)]).to(DEV)
    rowsum = torch.ones(m + 5, dtype=torch.float64, device=DEV)
    pair, picked = MS.rbf_subset_sums(rows, idx, MS.c2_of(MC.COUNT_SCALE), rowsum)
    assert (np.abs(pair.cpu().numpy() - m * (m - 1)) <= m * (m - 1) * 2.0 ** -22).all(), pair
    assert picked.cpu().tolist() == [float(m), float(m)]


def test_explicit_subsets_across_tiles():
    """600 positions of `tile`: three tile rows, diagonal and doubled tiles, a last tile of 88 rows."""
    from synference_amd import misspecification as MS
    z, _, _, _ = MC.make_case("tile")
    scale = MC.scale("tile")
    K, E = MM.kernel(z, z, scale)
    rng = np.random.default_rng(9)
    sets = np.stack([rng.permutation(len(z))[:600] for _ in range(3)]).astype(np.int32)
    pair = MS.rbf_subset_sums(torch.tensor(z).to(DEV), torch.as_tensor(sets).to(DEV), MS.c2_of(scale)).cpu().numpy()
    for s, S in enumerate(sets.astype(np.int64)):
        want, bound = MM.offdiag_sum(K[np.ix_(S, S)]), MM.offdiag_sum(E[np.ix_(S, S)])
        print(f"set {s}: |device - model| / bound = {abs(pair[s] - want) / bound:.3f}")
        assert abs(pair[s] - want) <= bound
    with pytest.raises(ValueError, match="outside"):
        MS.rbf_subset_sums(torch.tensor(z).to(DEV), torch.as_tensor(sets + 500).to(DEV), -1.0)
    with pytest.raises(ValueError, match="int32"):
        MS.rbf_subset_sums(torch.tensor(z).to(DEV), torch.as_tensor(sets.astype(np.int64)).to(DEV), -1.0)


@pytest.mark.parametrize("name", ["edge", "tile"])
def test_two_calls_give_the_same_bits(name):
    a, b = _sums(name, MC.scale(name)), _sums(name, MC.scale(name))
    for k in a:
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k


def test_rowsum_in_two_pieces():
    from synference_amd import misspecification as MS
    for name, cut in (("tile", 300), ("edge", 7)):       # (these shapes have one split of the base: row for row the same bits)
        z, _, _, _ = _dev(name)
        c2 = MS.c2_of(MC.scale(name))
        whole = MS.rbf_rowsum(z, z, c2, exclude_self=True)
        parts = torch.cat([MS.rbf_rowsum(z, z[:cut], c2, exclude_self=True),
                           MS.rbf_rowsum(z, z[cut:], c2, exclude_self=True, self_offset=cut)])
        assert torch.equal(whole, parts)
        assert not torch.equal(whole[cut:], MS.rbf_rowsum(z, z[cut:], c2, exclude_self=True))     # the offset matters
    # a long base is cut into splits by the number of query tiles: the pieces add in another order, the sums agree to fp64 rounding
    big = torch.as_tensor(np.random.default_rng(3).normal(size=(20000, 4)).astype(np.float32)).to(DEV)
    whole = MS.rbf_rowsum(big, big, -0.2, exclude_self=True)
    parts = torch.cat([MS.rbf_rowsum(big, big[:9000], -0.2, exclude_self=True),
                       MS.rbf_rowsum(big, big[9000:], -0.2, exclude_self=True, self_offset=9000)])
    assert float(((whole - parts).abs() / whole).max()) <= 1e-13
    ref = torch.exp2(torch.cdist(big[:64].double(), big.double()) ** 2 * -0.2).sum(1) - 1.0
    assert float(((whole[:64] - ref).abs() / ref).max()) <= 1e-5


def test_device_subsets_are_the_definition():
    from synference_amd import misspecification as MS
    for N, m, first in ((333, 41, 0), (1030, 257, 5), (130, 2, 0), (70000, 300, MS.SET_TRAIN)):
        got = MS._subsets_device(11, first, 6, N, m, DEV).cpu().numpy()
        assert np.array_equal(got, MS.mmd_subsets(11, 6, N, m, first=first))


def test_max_train_and_scale_are_honoured():
    from synference_amd import misspecification as MS
    z, z_obs, n_shuffle, seed = MC.make_case("edge")
    kw = dict(z_score=False, seed=seed, return_details=True)
    sub = MS.calc_misspecification_mmd(None, z_obs, z, "x_space", n_shuffle, max_train=200, **kw)
    keep = MS.mmd_subsets(seed, 1, len(z), 200, first=MS.SET_TRAIN)[0]
    same = MS.calc_misspecification_mmd(None, z_obs, z[keep], "x_space", n_shuffle, **kw)
    full = MS.calc_misspecification_mmd(None, z_obs, z, "x_space", n_shuffle, **kw)
    assert sub["mmd2"] == same["mmd2"] and np.array_equal(sub["null_mmd2"], same["null_mmd2"]) and sub["scale"] == same["scale"]
    assert sub["mmd2"] != full["mmd2"]
    wide = MS.calc_misspecification_mmd(None, z_obs, z, "x_space", n_shuffle, scale=3.5, **kw)
    assert wide["scale"] == 3.5 and wide["mmd2"] != full["mmd2"]
    want = MS.mmd2_unbiased(torch.tensor(z_obs).to(DEV), torch.tensor(z).to(DEV), 3.5)
    assert abs(wide["mmd2"] - want) <= 1e-12
    K, _ = MM.kernel(z_obs, z, 3.5)
    assert abs(wide["mmd2"] - MM.mmd2(MM.offdiag_sum(MM.kernel(z_obs, z_obs, 3.5)[0]), MM.offdiag_sum(MM.kernel(z, z, 3.5)[0]),
                                      float(K.sum()), len(z_obs), len(z))) <= 1e-6


def test_z_score_is_the_training_rows():
    from synference_amd import misspecification as MS
    z, z_obs, n_shuffle, seed = MC.make_case("edge")
    x, xo = z * np.float32(3.0) + np.float32(25.0), z_obs * np.float32(3.0) + np.float32(25.0)
    t = torch.as_tensor(x).to(DEV)
    mean, std = t.mean(0), t.std(0, unbiased=True).clamp_min(1e-7)
    zz, zzo = ((t - mean) / std).cpu().numpy(), ((torch.as_tensor(xo).to(DEV) - mean) / std).cpu().numpy()
    a = MS.calc_misspecification_mmd(None, xo, x, "x_space", n_shuffle, seed=seed, return_details=True)
    b = MS.calc_misspecification_mmd(None, zzo, zz, "x_space", n_shuffle, z_score=False, seed=seed, return_details=True)
    assert a["mmd2"] == b["mmd2"] and np.array_equal(a["null_mmd2"], b["null_mmd2"]) and a["p_value"] == b["p_value"]
    assert a["reject"] and a["p_value"] == 0.0                            # every feature shifted by 0.3 sigma over 41 rows


def test_embedding_mode_is_x_space_on_the_embedded_rows():
    from synference_amd import misspecification as MS
    from synference_amd.embedding import FCN
    from synference_amd.estimator import build_flow
    from synference_amd.posterior import EnsemblePosterior, FlowPosterior
    rng = np.random.default_rng(0)
    x = (rng.normal(size=(400, 12)) * 3 + 1).astype(np.float32)
    xo = (rng.normal(size=(50, 12)) * 3 + 1.5).astype(np.float32)
    theta = rng.normal(size=(400, 3)).astype(np.float32)
    emb = FCN([16, 6], "Tanh", generator=torch.Generator().manual_seed(0))
    est = build_flow("maf", theta, x, hidden_features=24, num_transforms=2, embedding_net=emb, device="cuda:0",
                     generator=torch.Generator().manual_seed(1)).to("cuda")
    with torch.no_grad():
        e, eo = est.embed(x).cpu().numpy(), est.embed(xo).cpu().numpy()
    assert e.shape == (400, 6)
    want = MS.calc_misspecification_mmd(None, eo, e, "x_space", 40, z_score=False, seed=3, return_details=True)
    post = FlowPosterior(est)
    for inference in (est, post, EnsemblePosterior([post])):
        got = MS.calc_misspecification_mmd(inference, xo, x, "embedding", 40, seed=3, return_details=True)
        assert got["mmd2"] == want["mmd2"] and np.array_equal(got["null_mmd2"], want["null_mmd2"])
        assert got["scale"] == want["scale"] and got["p_value"] == want["p_value"]
