"""Latents on the device: sf_flow_to_noise against the fp64 oracle (oracle.flows.forward_transform) for every flow kind, its
consistency with log_prob and inverse, the edges of the call, sf_latent_summary against the numpy model of
tests/latent_model.py, and the fitter surface (calculate_latent_residuals, evaluate_model(latent=True))."""
import functools

import numpy as np
import pytest
import torch

import latent_model as LM
from cases import CASES, make_case, oracle_inverse

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 333                       # ragged against the 32-row tiles of the register engine and the 64-row blocks of the AR engine
LOG_2PI = float(np.log(2.0 * np.pi))
EDGE_CASES = ["maf_cfg1", "nsf_cfg3", "nsf_d1", "nsfar_small", "mafar_small"]


@functools.lru_cache(maxsize=None)
def _run(name):
    """One handle per case, its parity rows through to_noise / log_prob, and the oracle's fp64 answer (computed once)."""
    from oracle import flows as OF
    from synference_amd.engine import HipFlow
    ospec, spec, flat, theta, x = make_case(name, B=B)
    f = HipFlow(spec, DEV)
    f.set_params(torch.as_tensor(flat))
    lp0 = f.log_prob(theta, x).cpu().numpy()
    z, lad = f.to_noise(theta, x)
    lp1 = f.log_prob(theta, x).cpu().numpy()
    with torch.no_grad():
        zr, lr = OF.forward_transform(ospec, torch.as_tensor(flat).double(), torch.as_tensor(theta).double(),
                                      torch.as_tensor(x).double())
    return dict(ospec=ospec, spec=spec, flat=flat, theta=theta, x=x, f=f, z=z.cpu().numpy(), lad=lad.cpu().numpy(), lp0=lp0, lp1=lp1,
                z_ref=zr.numpy(), lad_ref=lr.numpy())


@pytest.mark.parametrize("name", list(CASES))
def test_to_noise_matches_the_oracle(name):
    r = _run(name)
    assert r["z"].shape == (B, r["spec"].D) and r["z"].dtype == np.float32 and r["lad"].shape == (B,)
    ez = float(np.abs(r["z"].astype(np.float64) - r["z_ref"]).max())
    el = float(np.abs(r["lad"].astype(np.float64) - r["lad_ref"]).max())
    print(f"{name}: |dz|max={ez:.2e} |dlogabsdet|max={el:.2e}")
    assert ez < 2e-4 and el < 2e-4


@pytest.mark.parametrize("name", list(CASES))
def test_to_noise_is_consistent_with_log_prob(name):
    """-0.5 |z|^2 - 0.5 D log(2 pi) + logabsdet in fp64 from the fp32 outputs against the kernel's own fp32 evaluation of the same
    expression: D products, D + 1 additions and the final rounding, each 2^-24 relative to a partial sum that the three
    magnitudes bound -- 2^-23 (D + 3) (0.5 |z|^2 + 0.5 D log(2 pi) + |logabsdet|) per row."""
    r = _run(name)
    D = r["spec"].D
    z, lad = r["z"].astype(np.float64), r["lad"].astype(np.float64)
    half = 0.5 * (z * z).sum(1)
    want = -half - 0.5 * D * LOG_2PI + lad
    bound = 2.0 ** -23 * (D + 3) * (half + 0.5 * D * LOG_2PI + np.abs(lad))
    err = np.abs(r["lp0"].astype(np.float64) - want)
    print(f"{name}: max err / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert np.array_equal(r["lp0"], r["lp1"])            # log_prob before and after a to_noise call on the handle: same bits


@pytest.mark.parametrize("name", EDGE_CASES)
def test_round_trip_through_inverse(name):
    r = _run(name)
    th, _ = r["f"].inverse(torch.as_tensor(r["z"]), r["x"])
    err = float(np.abs((th.cpu().double().numpy() - r["theta"]) / np.asarray(r["ospec"].theta_std)).max())
    print(f"{name}: round trip rel err {err:.2e}")
    assert err < 2e-4


def _abi(r, theta, x, want_z=True, want_lad=True, z_buf=None):
    from synference_amd import _lib
    lib = _lib.load()
    n, D = theta.shape[0], r["spec"].D
    z = (torch.full((n, D), 7.0, device=DEV) if z_buf is None else z_buf) if want_z else None
    lad = torch.full((n,), 7.0, device=DEV) if want_lad else None
    _lib.check(lib.sf_flow_to_noise(r["f"].handle, _lib.ptr(theta), _lib.ptr(x), n, _lib.ptr(z), _lib.ptr(lad), _lib.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    return z, lad


@pytest.mark.parametrize("name", EDGE_CASES)
def test_edges_of_the_call(name):
    r = _run(name)
    f, D, Cx = r["f"], r["spec"].D, r["spec"].C
    z0, l0 = f.to_noise(np.zeros((0, D), np.float32), np.zeros((0, Cx), np.float32))          # B = 0: a no-op
    assert z0.shape == (0, D) and l0.shape == (0,)
    for n in (1, 3):
        z, lad = f.to_noise(r["theta"][:n], r["x"][:n])
        assert np.abs(z.cpu().double().numpy() - r["z_ref"][:n]).max() < 2e-4
        assert np.abs(lad.cpu().double().numpy() - r["lad_ref"][:n]).max() < 2e-4
    theta, x = torch.as_tensor(r["theta"]).to(DEV), torch.as_tensor(r["x"]).to(DEV)
    z_only, none = _abi(r, theta, x, want_lad=False)
    none2, lad_only = _abi(r, theta, x, want_z=False)
    assert none is None and none2 is None
    assert np.array_equal(z_only.cpu().numpy(), r["z"]) and np.array_equal(lad_only.cpu().numpy(), r["lad"])
    # a z that starts off a 16-byte boundary takes the dword stores: the same bits, nothing outside the rows
    buf = torch.full((B * D + 8,), 7.0, device=DEV)
    zv, _ = _abi(r, theta, x, z_buf=buf[1:1 + B * D].view(B, D))
    assert zv.data_ptr() % 16 == 4 and np.array_equal(zv.cpu().numpy(), r["z"])
    assert float(buf[0]) == 7.0 and (buf[1 + B * D:] == 7.0).all()
    # a NaN row of theta: a NaN row of z, the neighbours keep their bits
    bad = r["theta"].copy()
    bad[7] = np.nan
    zb, lb = f.to_noise(bad, r["x"])
    zb, lb = zb.cpu().numpy(), lb.cpu().numpy()
    assert np.isnan(zb[7]).all()
    keep = np.arange(B) != 7
    assert np.array_equal(zb[keep], r["z"][keep]) and np.array_equal(lb[keep], r["lad"][keep])
    with pytest.raises(ValueError):
        f.to_noise(r["theta"][:, :-1] if D > 1 else np.zeros((B, 2), np.float32), r["x"])


# ---- the summary ---------------------------------------------------------------------------------------------------
def _raw(z, nb):
    from synference_amd import _lib
    lib = _lib.load()
    zd = torch.as_tensor(z).to(DEV).contiguous()
    N, D = zd.shape
    n2 = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    psum = torch.full((4, D), -1.0, dtype=torch.float64, device=DEV)
    cross = torch.full((D, D), -1.0, dtype=torch.float64, device=DEV)
    pit = torch.full((D, nb), -1, dtype=torch.int64, device=DEV)
    rad = torch.full((nb,), -1, dtype=torch.int64, device=DEV)
    _lib.check(lib.sf_latent_summary(_lib.ptr(zd), N, D, nb, _lib.ptr(n2), _lib.ptr(psum), _lib.ptr(cross), _lib.ptr(pit), _lib.ptr(rad),
                                     _lib.stream_ptr(torch.device(DEV))))
    return [t.cpu().numpy() for t in (n2, psum, cross, pit, rad)]


def _summary_input(N, D):
    z = np.random.default_rng(1000 * N + D).standard_normal((N, D)).astype(np.float32)
    if N >= 63:
        z[3] = np.nan                      # a NaN row
        z[5, D // 2] = np.inf if D % 2 else -np.inf
        z[7] = 12.0                        # Phi saturates: the last bin
        z[11] = 0.0
    return z


@pytest.mark.parametrize("N,D,nb", [(1, 1, 1), (63, 5, 3), (64, 16, 100), (65, 16, 1024), (257, 3, 7), (20011, 16, 100)])
def test_summary_matches_the_model(N, D, nb):
    from synference_amd.features import latent_summary
    z = _summary_input(N, D)
    m = LM.raw_sums(z, nb)
    assert m["edge_rows"] == 0             # no value of the seeded inputs lies within 1e-9 of a bin edge: counts must be equal
    n2, psum, cross, pit, rad = _raw(z, nb)
    assert (int(n2[0]), int(n2[1])) == (m["n"], m["n_bad"]) and m["n_bad"] == (2 if N >= 63 else 0)
    ep = float((np.abs(psum - m["psum"]) / np.maximum(m["psum_abs"], 1e-300)).max())
    ec = float((np.abs(cross - m["cross"]) / np.maximum(m["cross_abs"], 1e-300)).max())
    print(f"N={N} D={D} nb={nb}: psum err / sum|terms| = {ep:.2e}, cross {ec:.2e}")
    assert (np.abs(psum - m["psum"]) <= 1e-12 * m["psum_abs"]).all()
    assert (np.abs(cross - m["cross"]) <= 1e-12 * m["cross_abs"]).all()
    assert np.array_equal(pit, m["pit_counts"]) and np.array_equal(rad, m["radial_counts"])
    again = _raw(z, nb)
    for a, b in zip((n2, psum, cross, pit, rad), again):
        assert a.tobytes() == b.tobytes()
    # the Python surface: the derived statistics (float64 on the host) against the model's direct ones
    s = latent_summary(torch.as_tensor(z).to(DEV), nb)
    ref = LM.latent_summary(z, nb)
    assert s["n"] == ref["n"] and s["n_bad"] == ref["n_bad"]
    assert np.array_equal(s["pit_counts"], ref["pit_counts"]) and np.array_equal(s["radial_counts"], ref["radial_counts"])
    assert np.array_equal(s["alpha"], ref["alpha"]) and np.allclose(s["ecp"], ref["ecp"], rtol=0, atol=1e-15)
    assert np.allclose(s["ks"], ref["ks"], rtol=0, atol=1e-15) and abs(s["radial_ks"] - ref["radial_ks"]) <= 1e-15
    if ref["n"] >= 50:   # raw-moment formulas: cancellation against moments of order 12^4 / n at the most
        for k in ("mean", "cov", "skew", "excess_kurtosis"):
            assert np.allclose(s[k], ref[k], rtol=1e-9, atol=1e-9), k


def test_summary_of_no_rows_and_null_outputs():
    from synference_amd import _lib
    from synference_amd.features import latent_summary
    n2, psum, cross, pit, rad = _raw(np.zeros((0, 4), np.float32), 10)
    assert n2.tolist() == [0, 0] and not psum.any() and not cross.any() and not pit.any() and not rad.any()
    s = latent_summary(torch.zeros((0, 4), device=DEV), 10)
    assert s["n"] == 0 and np.isnan(s["mean"]).all() and np.isnan(s["radial_ks"])
    lib = _lib.load()
    z = torch.as_tensor(_summary_input(257, 3)).to(DEV)
    rad = torch.zeros(7, dtype=torch.int64, device=DEV)
    _lib.check(lib.sf_latent_summary(_lib.ptr(z), 257, 3, 7, None, None, None, None, _lib.ptr(rad), _lib.stream_ptr(torch.device(DEV))))
    assert np.array_equal(rad.cpu().numpy(), LM.raw_sums(_summary_input(257, 3), 7)["radial_counts"])
    with pytest.raises(RuntimeError, match="sf_latent_summary: need 1 <= D <= 16"):
        latent_summary(torch.zeros((8, 17), device=DEV))


# ---- the fitter ----------------------------------------------------------------------------------------------------
def _fitter_with(members, weights=None):
    from synference_amd import SBI_Fitter
    from synference_amd.estimator import FlowEstimator
    from synference_amd.posterior import EnsemblePosterior, FlowPosterior
    spec0 = members[0][0]
    fit = SBI_Fitter("latent", [f"p{i}" for i in range(spec0.D)], device="cuda")
    posts = [FlowPosterior(FlowEstimator(s, torch.as_tensor(fl), device=DEV).to(DEV), None) for s, fl in members]
    fit.posteriors = EnsemblePosterior(posts, weights=weights)
    return fit


def test_fitter_tells_an_exact_sample_from_a_rescaled_flow():
    import dataclasses
    ospec, spec, flat, _, x = make_case("maf_cfg1", B=4096)
    z0 = np.random.default_rng(7).standard_normal((4096, spec.D)).astype(np.float32)
    theta, _ = oracle_inverse(ospec, flat, z0, x)                       # an exact sample of the flow, row by row
    theta = theta.astype(np.float32)
    wide = dataclasses.replace(spec, theta_std=spec.theta_std * 2)       # the same flow believing theta twice as wide
    fit = _fitter_with([(spec, flat)])
    res, lat = fit.calculate_latent_residuals(X=x, y=theta, return_latents=True)
    assert set(res) == {"members", "weights"} and len(res["members"]) == 1 and res["weights"] == [1.0]
    good = res["members"][0]
    assert lat[0].shape == (4096, spec.D) and lat[0].dtype == np.float64 and np.abs(lat[0] - z0).max() < 5e-4
    bad = _fitter_with([(wide, flat)]).calculate_latent_residuals(X=x, y=theta)["members"][0]
    print(f"radial_ks exact {good['radial_ks']:.4f} (ks max {good['ks'].max():.4f}), theta_std doubled {bad['radial_ks']:.4f}")
    assert good["n"] == 4096 and good["n_bad"] == 0
    assert good["radial_ks"] < 0.03 and bad["radial_ks"] > 0.3
    two = _fitter_with([(spec, flat), (wide, flat)], weights=[0.25, 0.75]).calculate_latent_residuals(X=x, y=theta)
    assert len(two["members"]) == 2 and np.allclose(two["weights"], [0.25, 0.75])
    assert two["members"][0]["radial_ks"] == good["radial_ks"] and two["members"][1]["radial_ks"] == bad["radial_ks"]


def test_evaluate_model_adds_exactly_the_two_keys(tmp_path):
    from synference_amd import SBI_Fitter
    from synference_amd.synthetic import make_catalogue
    x, theta, names = make_catalogue(3000, 10, 5, seed=1)
    f = SBI_Fitter("latent_e2e", names, [f"F{i}" for i in range(10)], feature_array=x, parameter_array=theta)
    post, _ = f.run_single_sbi(model_type="maf", hidden_features=50, num_transforms=5, n_nets=1, training_batch_size=256,
                               learning_rate=2e-3, stop_after_epochs=3, max_num_epochs=6, random_seed=3, save_model=False,
                               out_dir=str(tmp_path), verbose=False, evaluate_model=False)

    def run(**kw):   # the same seed state for both calls: the posteriors' call counters key the seeds nobody passes
        for p in [post] + list(post.posteriors):
            p._calls = 0
        return f.evaluate_model(posteriors=post, num_samples=100, seed=5, **kw)
    plain, with_latent = run(), run(latent=True)
    assert set(with_latent) - set(plain) == {"latent_radial_ks", "latent_ks_max"} and "latent_radial_ks" not in plain
    assert {k: with_latent[k] for k in plain} == plain
    res = f.calculate_latent_residuals(posteriors=post)                 # the stored test split
    assert with_latent["latent_radial_ks"] == res["members"][0]["radial_ks"]
    assert with_latent["latent_ks_max"] == float(res["members"][0]["ks"].max())
    assert 0.0 <= with_latent["latent_radial_ks"] <= 1.0 and res["members"][0]["n"] == len(f._X_test)
