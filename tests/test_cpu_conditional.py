"""Conditional posteriors without a GPU: the model of the ensemble sampler (tests/stretch_model.py) on an analytic target,
its partner indices and stretch factors, and the argument validation of the whole Python surface."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stretch_model as SM


# ---- 1. the model on an analytic target -------------------------------------------------------------------------------
MEAN = np.array([0.3, -1.0, 2.0])
SIG = np.array([1.0, 0.5, 2.0])
CORR = np.array([[1.0, 0.6, -0.3], [0.6, 1.0, 0.4], [-0.3, 0.4, 1.0]])
COV = CORR * SIG[:, None] * SIG[None, :]
LO, HI = MEAN - 8 * SIG, MEAN + 8 * SIG      # (the box cuts off < 1e-14 of the mass: the closed form holds)


def test_model_recovers_a_gaussian_conditional():
    N, W, S, R0, fixed_d, value = 16, 64, 1024, 1000, 1, -0.6
    rng = np.random.default_rng(5)
    pot = SM.gaussian_potential(MEAN, COV)
    cond = np.full((N, 3), np.nan)
    cond[:, fixed_d] = value
    mask, n_free, dead = SM.row_plan(cond, LO, HI)
    assert not dead.any() and (n_free == 2).all()
    draws = rng.multivariate_normal(MEAN, COV, size=(N, R0))
    x = np.zeros((N, 1))
    theta0, lp0, enough = SM.select_starts(pot, x, draws, mask, np.nan_to_num(cond), W)
    assert enough.all() and (theta0[:, :, fixed_d] == value).all()
    out, out_lp, acc = SM.run(pot, x, theta0, lp0, mask, enough & ~dead, LO, HI, num_samples=S, burn_in=200, thin=5, seed=11)
    assert out.shape == (N, S, 3) and np.isfinite(out).all()
    assert ((out >= LO) & (out <= HI)).all()
    assert (out[:, :, fixed_d] == value).all()
    assert np.array_equal(out_lp.reshape(-1), pot(out.reshape(-1, 3), None))
    u, cmean, ccov = SM.gaussian_conditional(MEAN, COV, [fixed_d], [value])
    row_means = out[:, :, u].mean(1)                       # [N, 2]
    se = row_means.std(0, ddof=1) / np.sqrt(N)             # between-row scatter of independent chains
    dev = np.abs(row_means.mean(0) - cmean) / se
    print(f"conditional mean {cmean}, pooled {row_means.mean(0)}, se {se}, |dev|/se {dev}, acceptance {acc.mean():.3f}")
    assert (dev <= 5.0).all(), dev
    # (the spread, for orientation: the pooled variance against the closed form, within 10 %)
    var = out[:, :, u].reshape(-1, 2).var(0)
    assert np.allclose(var, np.diag(ccov), rtol=0.1), (var, np.diag(ccov))
    assert ((acc > 0.3) & (acc < 1.0)).all()


def test_model_dead_rows_and_slot_dropping():
    pot = SM.gaussian_potential(MEAN, COV)
    N, W, S = 3, 8, 21                     # 3 collecting points, the last one keeps 5 of its 8 walkers
    cond = np.full((N, 3), np.nan)
    cond[:, 0] = [0.0, LO[0] - 1.0, np.inf]
    mask, n_free, dead = SM.row_plan(cond, LO, HI)
    assert dead.tolist() == [False, True, True]
    draws = np.random.default_rng(1).multivariate_normal(MEAN, COV, size=(N, 50))
    theta0, lp0, enough = SM.select_starts(pot, np.zeros((N, 1)), draws, mask, np.nan_to_num(cond, posinf=0.0), W)
    tr = []
    out, out_lp, acc = SM.run(pot, np.zeros((N, 1)), theta0, lp0, mask, enough & ~dead, LO, HI, num_samples=S, burn_in=4,
                              thin=2, seed=3, trace=tr)
    assert len(tr) == 2 * SM.n_steps(S, W, 4, 2) == 2 * (4 + 3 * 2)
    assert np.isfinite(out[0]).all() and np.isnan(out[1:]).all() and np.isnan(acc[1:]).all() and np.isfinite(acc[0])


# ---- 2. partner indices and stretch factors ---------------------------------------------------------------------------
@pytest.mark.parametrize("W", [4, 30, 64])
def test_partner_uniform_over_the_other_half(W):
    n_rows = 2000
    pos = (1 << 33) + np.arange(n_rows)          # positions past 2^32: both counter words in use
    for hs in (0, 1, 6, 7):
        h = hs & 1
        r = SM.words(12345, pos, hs, W)
        j = SM.partner(r[0][:, h::2], W, h)
        assert ((j % 2) == 1 - h).all() and (j >= 0).all() and (j < W).all()      # never in the active half
        n = j.size
        counts = np.bincount(j.reshape(-1) // 2, minlength=W // 2)
        expect = n / (W // 2)
        sd = np.sqrt(expect * (1 - 2.0 / W))
        assert (np.abs(counts - expect) < 5 * sd).all(), (W, hs, counts)
        z = SM.stretch_z(r[1])
        assert (z >= 1 / SM.A).all() and (z <= SM.A).all()
        # g(z) ~ 1 / sqrt(z) on [1/a, a]: E z = (a + 1 + 1/a) / 3
        assert abs(z.mean() - (SM.A + 1 + 1 / SM.A) / 3) < 5 * z.std() / np.sqrt(z.size)
    # the words are those of the sampler's stream with the stretch key
    from oracle import philox
    r = SM.words(7 + (9 << 32), [5], 3, 4)
    ref = philox.philox4x32_10(np.uint32(5), np.uint32(0), np.uint32(3), np.uint32(2), 7, 9 ^ SM.STREAM_STRETCH)
    assert [int(a[0, 2]) for a in r] == [int(a) for a in ref]


def test_proposal_copies_fixed_coordinates():
    rng = np.random.default_rng(0)
    theta = rng.normal(size=(6, 10, 4))
    mask = np.zeros((6, 4), bool)
    mask[:, 2] = True
    mask[3:, 0] = True
    for hs in (0, 1):
        y, j, z = SM.propose(theta, mask, 3, np.arange(6), hs)
        act = theta[:, (hs & 1)::2]
        assert np.array_equal(y[:, :, 2], act[:, :, 2]) and np.array_equal(y[3:, :, 0], act[3:, :, 0])
        tj = np.take_along_axis(theta, j[:, :, None], 1)
        assert np.allclose(y[:, :, 1], tj[:, :, 1] + z * (act[:, :, 1] - tj[:, :, 1]), rtol=0, atol=1e-15)


# ---- 3. argument validation -------------------------------------------------------------------------------------------
def test_plan_rows_and_walker_checks():
    from synference_amd import conditional as CD
    assert CD.STREAM_STRETCH == SM.STREAM_STRETCH
    lo, hi = np.zeros(5, np.float32), np.ones(5, np.float32)
    cond = np.full((4, 5), np.nan)
    cond[0, 1] = 0.5
    cond[1, [0, 4]] = [0.25, 0.75]
    cond[2, 3] = 1.5                          # outside the box: a NaN row
    vals, fixed = CD.plan_rows(cond, None, 4, 5, lo, hi, 64)
    assert fixed.tolist() == [2, 17, -1, 0] and vals.dtype == np.float32
    mask, n_free, dead = SM.row_plan(cond, lo, hi)
    assert dead.tolist() == [False, False, True, False] and n_free.tolist() == [4, 3, 4, 5]
    cond[3, 0] = -np.inf                      # not finite where the mask says fixed
    assert CD.plan_rows(cond, None, 4, 5, lo, hi, 64)[1].tolist() == [2, 17, -1, -1]
    # a (D,) condition is every row's; dims_to_sample frees dimensions
    v, f = CD.plan_rows(np.array([0.1, 0.2, 0.3, 0.4, 0.5]), [0, 2, 3], 3, 5, lo, hi, 64)
    assert f.tolist() == [18, 18, 18] and np.isnan(v[:, [0, 2, 3]]).all()
    with pytest.raises(ValueError, match="at least one free"):
        CD.plan_rows(np.array([0.1, 0.2, 0.3, 0.4, 0.5]), None, 3, 5, lo, hi, 64)
    with pytest.raises(ValueError, match="2 n_free \\+ 2 = 10"):
        CD.plan_rows(cond[:1], None, 1, 5, lo, hi, 8)       # 4 free coordinates need 10 walkers
    assert CD.plan_rows(cond[:1], None, 1, 5, lo, hi, 10)[1].tolist() == [2]
    with pytest.raises(ValueError, match="does not match"):
        CD.plan_rows(cond[:, :4], None, 4, 5, lo, hi, 64)
    with pytest.raises(ValueError, match="dims_to_sample"):
        CD.plan_rows(cond, [5], 4, 5, lo, hi, 64)
    for W in (3, 7, 63, 2, 66, 0):
        with pytest.raises(ValueError, match="num_walkers"):
            CD.check_conditional_args(100, W, 10, 1, 1000)
    for bad in (dict(num_samples=0), dict(burn_in=-1), dict(thin=0), dict(num_init_samples=10)):
        kw = dict(num_samples=100, num_walkers=16, burn_in=10, thin=1, num_init_samples=100)
        kw.update(bad)
        with pytest.raises(ValueError):
            CD.check_conditional_args(**kw)
    assert CD.n_steps(1000, 64, 200, 5) == SM.n_steps(1000, 64, 200, 5) == 280


def test_conditional_catalogue_checks_before_any_device_work():
    from synference_amd.conditional import conditional_catalogue
    owner = SimpleNamespace(prior=SimpleNamespace(low=torch.zeros(5), high=torch.ones(5)))
    posts = [SimpleNamespace(spec=SimpleNamespace(D=5))]
    X = np.zeros((2, 3), np.float32)
    cond = np.full((2, 5), np.nan)
    cond[:, 0] = 0.5
    with pytest.raises(ValueError, match="num_walkers = 7"):
        conditional_catalogue(owner, posts, None, X, cond, num_walkers=7)
    with pytest.raises(ValueError, match="2 n_free \\+ 2"):
        conditional_catalogue(owner, posts, None, X, cond, num_walkers=8)
    with pytest.raises(ValueError, match="at least one free"):
        conditional_catalogue(owner, posts, None, X, np.full((2, 5), 0.5))


def _fitter():
    from synference_amd.fitter import SBI_Fitter
    fit = SBI_Fitter("conditional_test", parameter_names=["redshift", "log_mass", "tau_v"])
    fit.feature_names = ["f0", "f1"]
    fit.fitted_parameter_names = list(fit.parameter_names)
    fit.simple_fitted_parameter_names = list(fit.parameter_names)
    fit.posteriors = SimpleNamespace()          # never reached: every check below fires first
    return fit


def test_fitter_validation():
    fit = _fitter()
    X = np.zeros((4, 2), np.float32)
    with pytest.raises(ValueError, match="redshift.*log_mass.*tau_v"):
        fit.sample_conditional_posterior(X, {"z_spec": 1.0})
    with pytest.raises(ValueError, match="redshift.*log_mass.*tau_v"):
        fit.fit_catalogue(X, fixed_parameters={"mass": 1.0})
    with pytest.raises(ValueError, match="missing_data_mcmc"):
        fit.fit_catalogue(X, fixed_parameters={"redshift": 1.0}, missing_data_mcmc=True)
    with pytest.raises(ValueError, match="num_walkers"):
        fit.sample_conditional_posterior(X, {"redshift": 1.0}, num_walkers=9)
    with pytest.raises(ValueError, match="array"):
        fit.sample_conditional_posterior(X, {"redshift": np.ones(3)})
    with pytest.raises(ValueError, match="not a column"):
        fit.fit_catalogue({"f0": np.zeros(4), "f1": np.zeros(4)}, fixed_parameters={"redshift": "z_spec"})
    with pytest.raises(TypeError, match="unknown keyword"):
        fit.sample_conditional_posterior(X, {"redshift": 1.0}, walkers=8)
    c = fit._fixed_condition({"redshift": 2.0, "tau_v": [0.1, np.nan, 0.3, 0.4]}, 4)
    assert c.shape == (4, 3) and (c[:, 0] == 2.0).all() and np.isnan(c[:, 1]).all() and np.isnan(c[1, 2])
    # routing through sample_method is out of scope: the name keeps raising
    with pytest.raises(ValueError, match="Invalid sample method"):
        fit.sample_posterior(X, sample_method="emcee")
