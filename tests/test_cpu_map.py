"""The model of the posterior-mode search (tests/map_model.py) and the argument checks of map / map_catalogue /
calculate_MAP: everything here runs without a GPU."""
import numpy as np
import pytest
import torch

import map_model as MM
from cases import make_case, oracle_log_prob


# ---- the model's gradient ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["maf_small", "nsf_d2"])
def test_model_gradient_against_central_differences(name):
    ospec, spec, flat, theta, x = make_case(name, B=24)
    theta = theta.astype(np.float64)
    lp, g = MM.flow_potential(ospec, flat, torch.float64)(theta, x)
    assert np.abs(lp - oracle_log_prob(ospec, flat, theta, x)).max() < 1e-12
    h = 1e-6
    fd = np.empty_like(g)
    for d in range(spec.D):
        e = np.zeros(spec.D); e[d] = h
        fd[:, d] = (oracle_log_prob(ospec, flat, theta + e, x) - oracle_log_prob(ospec, flat, theta - e, x)) / (2 * h)
    assert np.abs(fd - g).max() <= 1e-6 * np.abs(g).max(), np.abs(fd - g).max() / np.abs(g).max()


# ---- selection, clamp, schedule, ties ---------------------------------------------------------------------------------
def test_select_inits_order_ties_and_nan():
    p0 = np.array([[1.0, 3.0, np.nan, 3.0, -np.inf, 2.0],
                   [np.nan, np.nan, np.nan, np.nan, np.nan, np.nan]])
    idx = MM.select_inits(p0, 4)
    assert idx[0].tolist() == [1, 3, 5, 0]          # ties: lower index first; NaN / -inf last
    assert idx[1].tolist() == [0, 1, 2, 3]


def test_box_transform_clamp_and_round_trip():
    lo, hi = np.array([-1.0, 0.0]), np.array([3.0, 10.0])
    th = np.array([[-1.0, 10.0], [1.0, 5.0], [-5.0, 20.0]])
    phi = MM.to_phi(th, lo, hi)
    lim = np.log(1e-6) - np.log1p(-1e-6)
    assert np.allclose(phi[0], [lim, -lim]) and np.allclose(phi[2], [lim, -lim]) and np.allclose(phi[1], 0.0)
    assert np.allclose(MM.to_theta(phi, lo, hi)[1], th[1])
    assert np.array_equal(MM.to_phi(th, None, None), th) and np.array_equal(MM.to_theta(th, None, None), th)


def _recording(fn):
    calls = []

    def wrapped(theta, x):
        calls.append(np.array(theta, copy=True))
        return fn(theta, x)
    return wrapped, calls


def test_schedule_scores_iterates_0_s_2s_and_the_last():
    # the potential's VALUE is the evaluation count (so every later evaluation would win if it were scored), its gradient
    # pushes every coordinate up: the best must be the last scored iterate, and it is scored only on the schedule
    state = {"n": 0}

    def pot(theta, x):
        state["n"] += 1
        return np.full(len(theta), float(state["n"])), np.ones_like(theta)
    pot, calls = _recording(pot)
    x = np.zeros((1, 1))
    out = MM.gradient_ascent(pot, x, np.zeros((1, 1, 2)), num_iter=25, num_to_optimize=1, learning_rate=0.1,
                             save_best_every=10)
    assert len(calls) == 1 + 25 + 1                       # inits, one per step, one after the last step
    assert out["log_prob_map"][0] == 27.0                 # the evaluation after the last step
    assert np.array_equal(out["theta_map"][0], calls[-1][0])
    # an oscillating ascent (Adam's first step is the learning rate, twice the distance to the optimum): the result is the
    # best of the init and the iterates 0, 10, 20 and 25 -- iterates off the schedule, however good, are not seen
    f = lambda t, xx: (-np.abs(t).sum(-1), -np.sign(t))
    pot, calls = _recording(f)
    out = MM.gradient_ascent(pot, x, np.full((1, 1, 2), 0.05), num_iter=25, num_to_optimize=1, learning_rate=0.1,
                             save_best_every=10)
    seen = [calls[0][0], calls[1][0], calls[11][0], calls[21][0], calls[26][0]]
    vals = [float(f(t[None], None)[0][0]) for t in seen]
    assert out["log_prob_map"][0] == max(vals) and np.array_equal(out["theta_map"][0], seen[int(np.argmax(vals))])
    every = [float(f(c, None)[0][0]) for c in calls]
    assert max(every) > max(vals)                         # (an unscored iterate was better: the schedule is what is tested)


def test_strict_improvement_and_lowest_index_on_ties():
    # a flat potential: nothing ever improves strictly, every candidate keeps its init, the row takes candidate 0
    inits = np.arange(12, dtype=np.float64).reshape(2, 3, 2)
    out = MM.gradient_ascent(lambda t, xx: (np.zeros(len(t)), np.zeros_like(t)), np.zeros((2, 1)), inits, num_iter=5,
                             num_to_optimize=3)
    assert np.array_equal(out["theta_map"], inits[:, 0]) and np.array_equal(out["log_prob_map"], [0.0, 0.0])


def test_rows_without_a_finite_init_and_frozen_candidates():
    def pot(theta, x):
        p = -(theta ** 2).sum(-1)
        p = np.where(theta[:, 0] > 5.0, np.nan, p)           # a region where the density is not finite
        return p, -2 * theta
    inits = np.array([[[6.0, 0.0], [7.0, 0.0]], [[1.0, 1.0], [6.0, 0.0]]])
    out = MM.gradient_ascent(pot, np.zeros((2, 1)), inits, num_iter=20, num_to_optimize=2, learning_rate=0.05)
    assert np.isnan(out["theta_map"][0]).all() and np.isnan(out["log_prob_map"][0])
    assert np.isfinite(out["theta_map"][1]).all() and out["log_prob_map"][1] > -2.0
    assert out["init_idx"][1].tolist() == [0, 1]


# ---- known answer -----------------------------------------------------------------------------------------------------
def test_zero_maf_is_the_gaussian_of_the_model():
    ospec, spec, flat, theta, x = make_case("maf_small", B=12)
    sig = MM.zero_maf_sigma(ospec)
    lp = oracle_log_prob(ospec, np.zeros_like(flat), theta, x)
    ref, _ = MM.gaussian_potential(ospec.theta_mean, sig)(theta, x)
    assert np.abs(lp - ref).max() < 1e-10


@pytest.mark.parametrize("shift", [0.0, 1.0])
def test_known_answer_model(shift):
    ospec, spec, flat, theta, x = make_case("maf_small", B=6)
    std, mean = np.asarray(ospec.theta_std, np.float64), np.asarray(ospec.theta_mean, np.float64)
    sig = MM.zero_maf_sigma(ospec)
    lo = mean - 4 * std if shift == 0.0 else mean + shift * sig      # shift 1: the mean lies one sigma below the box
    hi = lo + 8 * std
    rng = np.random.default_rng(3)
    inits = np.empty((6, 64, spec.D))
    for i in range(6):                                     # accepted draws of N(mean, sig) inside the box
        acc = np.empty((0, spec.D))
        while len(acc) < 64:
            d = mean + sig * rng.normal(size=(4096, spec.D))
            acc = np.concatenate([acc, d[((d >= lo) & (d <= hi)).all(1)]])
        inits[i] = acc[:64]
    lr = 0.01
    out = MM.gradient_ascent(MM.gaussian_potential(mean, sig), x, inits, lo, hi, num_iter=1000, num_to_optimize=8,
                             learning_rate=lr)
    th = out["theta_map"]
    tol = lr * (hi - lo) / 4
    if shift == 0.0:
        assert (np.abs(th - mean) <= tol).all(), (np.abs(th - mean) / tol).max()
    else:
        assert ((th >= lo) & (th - lo <= tol + 1e-6 * (hi - lo))).all(), ((th - lo) / tol).max()
    assert (out["log_prob_map"] >= out["init_lp"].max(1)).all()


# ---- argument validation (no GPU) -------------------------------------------------------------------------------------
def _cpu_posterior():
    from synference_amd.estimator import FlowEstimator
    from synference_amd.posterior import EnsemblePosterior, FlowPosterior
    ospec, spec, flat, theta, x = make_case("maf_small", B=4)
    post = FlowPosterior(FlowEstimator(spec, torch.as_tensor(flat), device="cuda:0"))
    return post, EnsemblePosterior([post]), x


@pytest.mark.parametrize("kw,msg", [(dict(num_iter=-1), "num_iter"), (dict(num_to_optimize=0), "num_to_optimize"),
                                    (dict(num_init_samples=0), "num_init_samples"), (dict(save_best_every=0), "save_best_every"),
                                    (dict(learning_rate=0.0), "learning_rate"), (dict(init_method="prior"), "init_method"),
                                    (dict(init_method=torch.zeros(3)), "init_method")])
def test_map_argument_validation(kw, msg):
    post, ens, x = _cpu_posterior()
    for p in (post, ens):
        with pytest.raises(ValueError, match=msg):
            p.map_catalogue(x, **kw)
        with pytest.raises(ValueError, match=msg):
            p.map(x[0], **kw)


def test_map_takes_one_observation_and_needs_x():
    post, ens, x = _cpu_posterior()
    for p in (post, ens):
        with pytest.raises(ValueError, match="ONE observation"):
            p.map(x)
        with pytest.raises(ValueError, match="needs the observation"):
            p.map()
        p_kw = dict(show_progress_bars=True, force_update=True)       # accepted (and ignored): the error is the next check
        with pytest.raises(ValueError, match="ONE observation"):
            p.map(x, **p_kw)


def test_calculate_map_argument_validation():
    from synference_amd.fitter import SBI_Fitter
    post, ens, x = _cpu_posterior()
    fit = SBI_Fitter("t", parameter_names=["a", "b"])
    fit.posteriors = ens
    with pytest.raises(ValueError, match="X must be provided"):
        fit.calculate_MAP()
    with pytest.raises(TypeError, match="unknown keyword"):
        fit.calculate_MAP(x, num_steps=3)
    with pytest.raises(ValueError, match="num_iter"):
        fit.calculate_MAP(x, num_iter=-2)
    with pytest.raises(ValueError, match="init_method"):
        fit.calculate_MAP(x, init_method="sir")
