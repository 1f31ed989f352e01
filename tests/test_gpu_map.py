"""Posterior mode on the device: the theta-gradient kernels (csrc/sf_gradtheta_kernels.h), the fused ascent step and
map_catalogue / map / calculate_MAP against the model (tests/map_model.py) and fp64 autograd through the oracle.

The tests print what they measure (errors, deficits) before they assert: run with ``-s`` to see the figures."""
import functools

import numpy as np
import pytest
import torch

import map_model as MM
from cases import make_case, oracle_log_prob

pytestmark = pytest.mark.gpu

LOGP_TOL = 1e-4      # tests/test_gpu_parity.py: fp32 device log-density against the fp64 oracle
GRAD_REL = 2e-4      # tests/test_gpu_parity.py: the project's gradient bound for the same arithmetic

GRAD_CASES = ["maf_small", "maf_cfg1", "maf_d1", "maf_sig2", "maf_nb3", "maf_nb1", "maf_wide", "maf_t8",
              "nsf_d2", "nsf_odd", "nsf_nb1", "nsf_k16", "nsf_h69", "nsf_cfg3"]


def _flow(spec, flat):
    from synference_amd.engine import HipFlow
    f = HipFlow(spec, "cuda:0")
    f.set_params(torch.as_tensor(flat))
    return f


@functools.lru_cache(maxsize=None)
def _case(name, B=333):
    ospec, spec, flat, theta, x = make_case(name, B=B)
    for a in (flat, theta, x):
        a.setflags(write=False)
    return ospec, spec, flat, theta, x


@functools.lru_cache(maxsize=None)
def _ref(name, B=333):
    """fp64 autograd of the oracle, once per case."""
    ospec, spec, flat, theta, x = _case(name, B)
    lp, g = MM.flow_potential(ospec, flat, torch.float64)(theta, x)
    lp.setflags(write=False); g.setflags(write=False)
    return lp, g


def _check_grad(name, lp, g, ref_lp, ref_g, std):
    e_lp = np.abs(lp - ref_lp).max()
    e_g = np.abs((g - ref_g) * std).max()
    scale = np.abs(ref_g * std).max()
    print(f"{name}: |dlp|max={e_lp:.3e} grad err={e_g:.3e} rel={e_g / scale:.3e}")
    assert e_lp < LOGP_TOL, (name, e_lp)
    assert e_g <= GRAD_REL * scale, (name, e_g, scale)


# ---- 1. gradient parity -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAD_CASES)
def test_gradient_parity(name):
    ospec, spec, flat, theta, x = _case(name)
    ref_lp, ref_g = _ref(name)
    std = np.asarray(ospec.theta_std)
    f = _flow(spec, flat)
    lp, g = f.log_prob_grad(theta, x)
    lp, g = lp.cpu().double().numpy(), g.cpu().double().numpy()
    _check_grad(name, lp, g, ref_lp, ref_g, std)
    # ragged sub-batches (one row, one tile + one row) against the same reference rows
    for B in (1, 33):
        lpb, gb = f.log_prob_grad(theta[:B], x[:B])
        _check_grad(f"{name}[B={B}]", lpb.cpu().double().numpy(), gb.cpu().double().numpy(), ref_lp[:B], ref_g[:B], std)
    # one output at a time: the same numbers
    lp_only, none_g = f.log_prob_grad(theta, x, want_grad=False)
    none_lp, g_only = f.log_prob_grad(theta, x, want_lp=False)
    assert none_g is None and none_lp is None
    assert np.array_equal(lp_only.cpu().double().numpy(), lp) and np.array_equal(g_only.cpu().double().numpy(), g)


@pytest.mark.parametrize("name", ["maf_cfg1", "nsf_cfg3", "nsf_odd"])
def test_rows_per_x_is_the_repeated_context(name):
    ospec, spec, flat, theta, x = _case(name)
    f = _flow(spec, flat)
    R = 7
    nx = (len(theta) + R - 1) // R
    xs = torch.as_tensor(x[:nx].copy())
    lp1, g1 = f.log_prob_grad(theta, xs, rows_per_x=R)
    lp2, g2 = f.log_prob_grad(theta, xs.repeat_interleave(R, 0)[:len(theta)].contiguous())
    assert torch.equal(lp1, lp2) and torch.equal(g1, g2)
    assert torch.isfinite(lp1).all() and torch.isfinite(g1).all()


# Above 256 MiB of stash a call runs as several launches over consecutive tiles (maf_cfg1: 1872 tiles = 59904 rows); a wide
# flow's launch is widened to one tile per SIMD first (nsf_cfg3: 819 tiles in 256 MiB, 1024 on an MI355X = 32768 rows).
@pytest.mark.parametrize("name,B", [("maf_cfg1", 70001), ("nsf_cfg3", 40001)])
def test_stash_bounded_launches_are_the_small_calls(name, B):
    ospec, spec, flat, theta, x = make_case(name, B=B)
    f = _flow(spec, flat)
    th, xs = torch.as_tensor(theta).cuda(), torch.as_tensor(x).cuda()
    lp, g = f.log_prob_grad(th, xs)
    for r0 in range(0, B, 8192):
        lpc, gc = f.log_prob_grad(th[r0:r0 + 8192], xs[r0:r0 + 8192])
        assert torch.equal(lp[r0:r0 + 8192], lpc) and torch.equal(g[r0:r0 + 8192], gc), r0
    assert torch.isfinite(lp).all() and torch.isfinite(g).all()


# ---- 2. nothing else moves --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["maf_cfg1", "nsf_cfg3"])
def test_other_calls_unchanged_by_a_gradient_call(name):
    ospec, spec, flat, theta, x = _case(name)
    fl = torch.as_tensor(flat).cuda()

    def snapshot(f):
        lp = f.log_prob(theta, x).clone()
        s = f.sample(x[:8], 64, seed=3).clone()
        loss, grad = f.loss_grad(fl, theta, x, 1.0 / len(theta))
        return lp, s, loss.clone(), grad.clone()

    f = _flow(spec, flat)
    before = snapshot(f)
    f.set_params(fl)                      # (loss_grad left the caller's vector as the master copy)
    f.log_prob_grad(theta, x)
    after = snapshot(f)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    # after loss_grad the handle holds no vector of its own: the documented state error, then set_params repairs it
    with pytest.raises(RuntimeError, match="master copy"):
        f.log_prob_grad(theta, x)
    f.set_params(fl * 0.5)
    lp_half, g_half = f.log_prob_grad(theta, x)
    f2 = _flow(spec, np.asarray(flat) * 0.5)
    lp2, g2 = f2.log_prob_grad(theta, x)
    assert torch.equal(lp_half, lp2) and torch.equal(g_half, g2)     # the image follows set_params


# ---- 3. unsupported kinds ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,word", [("nsf_d1", "one-parameter NSF"), ("nsfar_small", "nsf_ar"), ("mafar_small", "maf_ar")])
def test_unsupported_kinds_raise(name, word):
    ospec, spec, flat, theta, x = make_case(name, B=8)
    f = _flow(spec, flat)
    assert not f.supports_log_prob_grad()
    with pytest.raises(RuntimeError, match=word):
        f.log_prob_grad(theta, x)


def test_unsupported_kind_keeps_theta_out_of_autograd():
    """theta.requires_grad alone on a kind without the kernel: no graph, as before the theta gradient existed, so a
    backward() raises instead of leaving theta.grad at None."""
    from synference_amd.estimator import FlowEstimator
    ospec, spec, flat, theta, x = make_case("nsf_d1", B=8)
    est = FlowEstimator(spec, torch.as_tensor(flat), device="cuda:0").to("cuda:0")
    est.flat.requires_grad_(False)
    th = torch.as_tensor(theta).cuda().requires_grad_(True)
    lp = est.log_prob(th, context=torch.as_tensor(x).cuda())
    assert not lp.requires_grad and lp.grad_fn is None
    with pytest.raises(RuntimeError):
        lp.sum().backward()


# ---- 4. autograd ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["maf_cfg1", "nsf_odd"])
def test_autograd_theta_gradient(name):
    from synference_amd.estimator import FlowEstimator
    ospec, spec, flat, theta, x = _case(name)
    est = FlowEstimator(spec, torch.as_tensor(flat), device="cuda:0").to("cuda:0")
    th = torch.as_tensor(theta).cuda()
    xs = torch.as_tensor(x).cuda()
    est.log_prob(th, context=xs).sum().backward()
    flat_grad = est.flat.grad.clone()
    est.flat.grad = None
    thg = th.clone().requires_grad_(True)
    est.log_prob(thg, context=xs).sum().backward()
    _, g = _flow(spec, flat).log_prob_grad(theta, x)
    assert torch.equal(thg.grad, g)
    assert torch.equal(est.flat.grad, flat_grad)
    # theta alone
    est.flat.requires_grad_(False)
    thg2 = th.clone().requires_grad_(True)
    (2.0 * est.log_prob(thg2, context=xs)).sum().backward()
    assert torch.equal(thg2.grad, 2.0 * g)


# ---- 5. the step kernel against the model -----------------------------------------------------------------------------
def _device_ascent(f, x, inits, lo, hi, num_iter, lr, save_best_every=10):
    """The loop of synference_amd.map.map_catalogue for R = 1, driven by hand so that the last iterate is visible."""
    from synference_amd.map import map_step
    dev = "cuda:0"
    th0 = torch.as_tensor(inits, dtype=torch.float32, device=dev)
    lo_t, hi_t = torch.as_tensor(lo, dtype=torch.float32, device=dev), torch.as_tensor(hi, dtype=torch.float32, device=dev)
    xs = torch.as_tensor(x, device=dev)
    u = ((th0 - lo_t) / (hi_t - lo_t)).clamp(1e-6, 1 - 1e-6)
    phi = (torch.log(u) - torch.log1p(-u)).contiguous()
    theta = (lo_t + (hi_t - lo_t) * torch.sigmoid(phi)).contiguous()
    m, v = torch.zeros_like(phi), torch.zeros_like(phi)
    best_lp = torch.full((len(th0),), float("-inf"), device=dev)
    best_th = torch.full_like(th0, float("nan"))
    for k in range(num_iter):
        lp, g = f.log_prob_grad(theta, xs)
        map_step(theta, lp, g, phi, m, v, lo_t, hi_t, best_th, best_lp, lr, k + 1, k % save_best_every == 0)
    return theta.cpu().double().numpy()


@pytest.mark.parametrize("name", ["maf_cfg1", "nsf_odd"])
def test_step_kernel_follows_the_model(name):
    ospec, spec, flat, theta, x = _case(name, 64)
    std, mean = np.asarray(ospec.theta_std), np.asarray(ospec.theta_mean)
    lo, hi = mean - 4 * std, mean + 4 * std
    inits = np.clip(theta, lo + 0.05 * std, hi - 0.05 * std)
    ref = MM.gradient_ascent(MM.flow_potential(ospec, flat, torch.float64), x, inits[:, None, :], lo, hi, num_iter=100,
                             num_to_optimize=1, learning_rate=0.01)
    got = _device_ascent(_flow(spec, flat), x, inits, lo, hi, 100, 0.01)
    err = np.abs((got - ref["theta_last"][:, 0]) / std).max(-1)
    print(f"{name}: median={np.median(err):.3e} max={err.max():.3e}")
    assert np.median(err) < 2e-4 and (err > 5e-3).mean() < 0.05, (np.median(err), err.max())
    moved = np.abs((ref["theta_last"][:, 0] - inits) / std).max(-1)
    assert np.median(moved) > 0.01      # (the comparison is about iterates that went somewhere)


# ---- 6. known answer --------------------------------------------------------------------------------------------------
def _posterior(spec, flat, lo=None, hi=None, seed=5):
    from synference_amd.estimator import FlowEstimator
    from synference_amd.posterior import FlowPosterior
    from synference_amd.priors import CustomIndependentUniform
    est = FlowEstimator(spec, torch.as_tensor(flat), device="cuda:0").to("cuda:0")
    prior = None
    if lo is not None:
        prior = CustomIndependentUniform(torch.as_tensor(lo, dtype=torch.float32), torch.as_tensor(hi, dtype=torch.float32),
                                         device="cuda:0")
    return FlowPosterior(est, prior, seed=seed)


@pytest.mark.parametrize("shift", [0.0, 1.0])
def test_known_answer_zero_maf(shift):
    ospec, spec, flat, theta, x = make_case("maf_small", B=6)
    std, mean = np.asarray(ospec.theta_std, np.float64), np.asarray(ospec.theta_mean, np.float64)
    sig = MM.zero_maf_sigma(ospec)
    lo = mean - 4 * std if shift == 0.0 else mean + shift * sig      # shift 1: the mean lies one sigma below the box
    hi = lo + 8 * std
    lr = 0.01
    post = _posterior(spec, np.zeros_like(flat), lo, hi)
    th, lp = post.map_catalogue(x, num_iter=1000, num_to_optimize=8, learning_rate=lr, num_init_samples=64, seed=17)
    th = th.cpu().double().numpy()
    tol = lr * (hi - lo) / 4
    if shift == 0.0:
        assert (np.abs(th - mean) <= tol).all(), np.abs(th - mean).max(0) / tol
    else:
        lo32 = lo.astype(np.float32).astype(np.float64)       # (the face as the device holds it)
        assert ((th >= lo32) & (th - lo32 <= tol + 1e-6 * (hi - lo))).all(), ((th - lo32) / tol).max(0)
    assert torch.isfinite(lp).all()


# ---- 7. end to end ----------------------------------------------------------------------------------------------------
E2E = dict(num_iter=100, num_to_optimize=8, learning_rate=0.01, num_init_samples=64, save_best_every=10)


def _box(ospec):
    std, mean = np.asarray(ospec.theta_std, np.float64), np.asarray(ospec.theta_mean, np.float64)
    return mean - 4 * std, mean + 4 * std


def _e2e_checks(post, pot_grad, x, D, monkeypatch):
    """7(a)-(c) for a posterior whose potential on the device is ``pot_grad(theta, x_rows) -> lp``."""
    import synference_amd.map as M
    N = len(x)
    th, lp = post.map_catalogue(x, seed=23, **E2E)
    assert th.shape == (N, D) and lp.shape == (N,) and th.dtype == torch.float32 and lp.dtype == torch.float32
    assert torch.isfinite(th).all() and torch.isfinite(lp).all()
    # (a) never below the best init, exactly
    inits = post.sample_catalogue(x, E2E["num_init_samples"], seed=23)
    R0 = inits.shape[1]
    p0 = pot_grad(inits.reshape(N * R0, D), torch.as_tensor(x).cuda().repeat_interleave(R0, 0)).reshape(N, R0)
    assert (lp >= p0.max(1).values).all()
    assert (lp > p0.max(1).values).float().mean() > 0.5          # ... and the ascent went somewhere
    # (b) the value is the density at the returned point
    assert (pot_grad(th, torch.as_tensor(x).cuda()) - lp).abs().max() < 1e-5
    # (c) the same seed twice; one block against row blocks of 5
    th2, lp2 = post.map_catalogue(x, seed=23, **E2E)
    assert torch.equal(th, th2) and torch.equal(lp, lp2)
    monkeypatch.setattr(M, "MAP_BLOCK_DRAWS", 5 * E2E["num_init_samples"])
    th3, lp3 = post.map_catalogue(x, seed=23, **E2E)
    assert torch.equal(th, th3) and torch.equal(lp, lp3)
    monkeypatch.undo()
    return th, lp, inits


@pytest.mark.parametrize("name", ["maf_small", "nsf_d2"])
def test_map_catalogue_end_to_end(name, monkeypatch):
    ospec, spec, flat, theta, x = _case(name, 16)
    lo, hi = _box(ospec)
    post = _posterior(spec, flat, lo, hi)
    flow = post.posterior_estimator.flow
    th, lp, inits = _e2e_checks(post, lambda t, xx: flow.log_prob(t, xx), x, spec.D, monkeypatch)
    # (d) deficit against the fp64 model on the device's own inits, everything scored by the fp64 oracle
    ini = inits.cpu().numpy()
    thd, _ = post.map_catalogue(x, init_method=torch.as_tensor(ini), **E2E)
    kw = dict(num_iter=E2E["num_iter"], num_to_optimize=E2E["num_to_optimize"], learning_rate=E2E["learning_rate"],
              save_best_every=E2E["save_best_every"])
    m64 = MM.gradient_ascent(MM.flow_potential(ospec, flat, torch.float64), x, ini, lo, hi, **kw)
    m32 = MM.gradient_ascent(MM.flow_potential(ospec, flat, torch.float32), x, ini, lo, hi, dtype=np.float32, **kw)
    s64 = oracle_log_prob(ospec, flat, m64["theta_map"], x)
    s32 = oracle_log_prob(ospec, flat, m32["theta_map"], x)
    sdev = oracle_log_prob(ospec, flat, thd.cpu().double().numpy(), x)
    d32, ddev = float((s64 - s32).max()), float((s64 - sdev).max())
    print(f"{name}: deficit fp32 model {d32:.3e}, device {ddev:.3e}")
    assert ddev <= max(4 * d32, LOGP_TOL), (ddev, d32)


# ---- 8. ensemble ------------------------------------------------------------------------------------------------------
def test_ensemble_gradient_and_map(monkeypatch):
    from synference_amd.map import _Potential
    from synference_amd.posterior import EnsemblePosterior
    ospec, spec, flat, theta, x = _case("nsf_odd", 333)
    _, _, flat_b, _, _ = make_case("nsf_odd", seed=1, B=4)
    flat_b = flat_b.astype(np.float32)
    lo, hi = _box(ospec)
    w = [0.3, 0.7]
    ens = EnsemblePosterior([_posterior(spec, flat, lo, hi), _posterior(spec, flat_b, lo, hi)], weights=w, seed=3)
    pot = _Potential(ens.posteriors, ens.weights, torch.as_tensor(x))
    lp, g = pot(torch.as_tensor(theta).cuda(), 0, len(x), 1, True)
    ref_lp, ref_g = MM.ensemble_potential([ospec, ospec], [flat, flat_b], w, torch.float64)(theta, x)
    _check_grad("ensemble nsf_odd", lp.cpu().double().numpy(), g.cpu().double().numpy(), ref_lp, ref_g,
                np.asarray(ospec.theta_std))
    xs = x[:16]
    _e2e_checks(ens, lambda t, xx: ens.log_prob_catalogue(t, xx, norm_posterior=False), xs, spec.D, monkeypatch)


# ---- 9. fitter --------------------------------------------------------------------------------------------------------
def test_fitter_calculate_map_and_fit_catalogue():
    from synference_amd.fitter import SBI_Fitter
    from synference_amd.posterior import EnsemblePosterior
    ospec, spec, flat, theta, x = _case("maf_small", 16)
    lo, hi = _box(ospec)
    fit = SBI_Fitter("map_test", parameter_names=[f"p{i}" for i in range(spec.D)])
    fit.feature_names = [f"f{i}" for i in range(spec.C)]
    fit.fitted_parameter_names = list(fit.parameter_names)
    fit.simple_fitted_parameter_names = list(fit.parameter_names)
    fit.posteriors = EnsemblePosterior([_posterior(spec, flat, lo, hi)], seed=9)
    fit._X_test = x
    kw = dict(num_iter=30, num_to_optimize=4, num_init_samples=32)
    th = fit.calculate_MAP(seed=4, **kw)
    assert th.shape == (16, spec.D) and th.dtype == np.float64
    assert ((th >= lo - 1e-6) & (th <= hi + 1e-6)).all()
    assert fit.last_map_log_prob.shape == (16,) and np.isfinite(fit.last_map_log_prob).all()
    assert np.array_equal(th, fit.calculate_MAP(x, seed=4, **kw))
    obs = x.copy()
    obs[3, 1] = np.nan                       # a masked row
    plain = fit.fit_catalogue(obs, num_samples=64, seed=11, append_to_input=False)
    both = fit.fit_catalogue(obs, num_samples=64, seed=11, append_to_input=False, map_estimate=True, map_kwargs=kw)
    for c in plain.columns:
        assert np.array_equal(plain[c].to_numpy(), both[c].to_numpy(), equal_nan=True), c
    new = [c for c in both.columns if c not in plain.columns]
    assert new == [f"p{i}_map" for i in range(spec.D)] + ["map_log_prob"]
    vals = both[new].to_numpy()
    assert np.isnan(vals[3]).all() and np.isfinite(np.delete(vals, 3, axis=0)).all()
    # an init tensor through map_kwargs is indexed by table row: the masked row's block is skipped, the others are used
    inits = fit.posteriors.sample_catalogue(torch.as_tensor(x), 32, seed=2)
    t1 = fit.fit_catalogue(obs, num_samples=64, seed=11, append_to_input=False, map_estimate=True,
                           map_kwargs=dict(kw, init_method=inits))
    ref_th = fit.calculate_MAP(np.delete(x, 3, axis=0), init_method=torch.cat([inits[:3], inits[4:]]), **kw)
    assert np.array_equal(np.delete(t1[new[:-1]].to_numpy(), 3, axis=0), ref_th) and np.isnan(t1[new].to_numpy()[3]).all()
    with pytest.raises(ValueError, match="init_method"):
        fit.fit_catalogue(obs, num_samples=64, seed=11, append_to_input=False, map_estimate=True,
                          map_kwargs=dict(kw, init_method=inits[:5]))
