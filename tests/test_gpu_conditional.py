"""Conditional posteriors on the device: the step kernel (csrc/sf_stretch.hip) against the model (tests/stretch_model.py),
the whole pipeline along the device's own trajectory against the fp64 oracle, the distribution of the draws against the
quadrature CDF of the oracle's conditional density (tests/golden/conditional/), the invariances and the fitter surface.

The tests print what they measure before they assert: run with ``-s`` to see the figures."""
import functools
import os

import numpy as np
import pytest
import torch

import map_model as MM
import stretch_model as SM
from cases import make_case, oracle_log_prob

pytestmark = pytest.mark.gpu

LOGP_TOL = 1e-4      # tests/test_gpu_parity.py: fp32 device log-density against the fp64 oracle
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conditional")


def _box(ospec):
    std, mean = np.asarray(ospec.theta_std, np.float64), np.asarray(ospec.theta_mean, np.float64)
    return mean - 4 * std, mean + 4 * std


def _posterior(spec, flat, lo=None, hi=None, seed=5):
    from synference_amd.estimator import FlowEstimator
    from synference_amd.posterior import FlowPosterior
    from synference_amd.priors import CustomIndependentUniform
    est = FlowEstimator(spec, torch.as_tensor(flat), device=DEV).to(DEV)
    prior = None
    if lo is not None:
        prior = CustomIndependentUniform(torch.as_tensor(lo, dtype=torch.float32), torch.as_tensor(hi, dtype=torch.float32),
                                         device=DEV)
    return FlowPosterior(est, prior, seed=seed)


@functools.lru_cache(maxsize=None)
def _case(name, B=16):
    ospec, spec, flat, theta, x = make_case(name, B=B)
    for a in (flat, theta, x):
        a.setflags(write=False)
    return ospec, spec, flat, theta, x


def _mask_of(fixed, D):
    return ((np.maximum(fixed, 0)[:, None] >> np.arange(D)[None, :]) & 1).astype(bool)


# ---- the rules shared by tests 4 and 5 --------------------------------------------------------------------------------
def _check_proposals(tag, walkers, mask, live, seed, pos, hs, prop, partner):
    """The proposals of half-step ``hs`` follow from ``walkers`` (the device's state, fp32) as the model says."""
    w64 = walkers.astype(np.float64)
    y, j, z = SM.propose(w64, mask, seed, pos, hs)
    assert np.array_equal(partner[live], j[live]), tag
    act = w64[:, (hs & 1)::2]
    tj = np.take_along_axis(w64, j[:, :, None], axis=1)
    bound = 8 * 2.0 ** -24 * (np.abs(tj) + z[:, :, None] * np.abs(act - tj))
    err = np.abs(prop.astype(np.float64) - y)
    assert (err[live] <= bound[live]).all(), (tag, float((err[live] / np.maximum(bound[live], 1e-300)).max()))
    fixed_sel = np.broadcast_to(mask[:, None, :], prop.shape) & live[:, None, None]
    assert np.array_equal(prop[fixed_sel], walkers[:, (hs & 1)::2][fixed_sel]), tag      # copied, bit for bit
    return z


def _check_flags(lp_w, lp_y, z, n_free, prop, lo32, hi32, live, seed, pos, hs, W, flags):
    """(mismatches, excluded, total) of the accept flags against the model's rule on the given numbers; a near tie --
    |margin| < 1e-5 (1 + |lp| + |lp_y| + |(n - 1) log z|) -- is excluded."""
    lp_w, lp_y = lp_w.astype(np.float64), lp_y.astype(np.float64)
    m = SM.accept_margin(lp_w, lp_y, z, n_free, seed, pos, hs, W)
    inside = ((prop >= lo32) & (prop <= hi32)).all(-1)          # on the device's own numbers, in its precision
    finite = np.isfinite(lp_y)
    expect = inside & finite & (m > 0)
    with np.errstate(invalid="ignore"):
        eps = 1e-5 * (1 + np.abs(lp_w) + np.abs(lp_y) + np.abs((n_free[:, None] - 1.0) * np.log(z)))
        tie = inside & finite & (np.abs(m) < eps)
    sel = live[:, None] & ~tie
    return int((flags.astype(bool) != expect)[sel].sum()), int((tie & live[:, None]).sum()), int(live.sum() * flags.shape[1])


# ---- 4. one-step parity of sf_stretch_step, no flow -------------------------------------------------------------------
@pytest.mark.parametrize("W", [4, 30, 64])
@pytest.mark.parametrize("D", [1, 2, 5, 16])
def test_step_kernel_one_step_parity(D, W):
    from synference_amd.conditional import stretch_step
    N, S, seed, off, W2 = 37, 2 * W - 3, 0x1234567890ABCDEF, (1 << 32) + 11, W // 2
    rng = np.random.default_rng(1000 * D + W)
    lo32 = rng.uniform(-3.0, -2.0, D).astype(np.float32)
    hi32 = rng.uniform(1.5, 3.0, D).astype(np.float32)
    fixed = np.zeros(N, np.int32)
    for i in range(N):                       # mixed masks: 0 .. D - 1 fixed coordinates, every row keeps a free one
        k = rng.integers(0, D)
        fixed[i] = sum(1 << int(d) for d in rng.choice(D, size=k, replace=False))
    fixed[5] = -1                            # a NaN row: nothing of it is read or written
    mask, live = _mask_of(fixed, D), fixed >= 0
    n_free = D - mask.sum(1)
    walkers = rng.uniform(lo32, hi32, (N, W, D)).astype(np.float32)
    values = rng.uniform(lo32, hi32, (N, D)).astype(np.float32)
    walkers = np.where(mask[:, None, :], values[:, None, :], walkers)
    lp = (-100.0 * rng.random((N, W)) ** 2).astype(np.float32)
    pos = off + np.arange(N)
    t = lambda a: torch.as_tensor(a).to(DEV).contiguous()
    d_w, d_lp, d_fx, d_lo, d_hi = t(walkers), t(lp), t(fixed), t(lo32), t(hi32)
    d_prop = torch.full((N, W2, D), 7.5, device=DEV)
    d_acc = torch.zeros(N, dtype=torch.int32, device=DEV)
    d_out = torch.full((N, S, D), -9.0, device=DEV)
    d_olp = torch.full((N, S), -9.0, device=DEV)
    d_tp = torch.full((N, W2), -1, dtype=torch.int32, device=DEV)
    d_ta = torch.full((N, W2), -1, dtype=torch.int32, device=DEV)
    max_fixed = max(D - 1, 0)
    mism = excl = total = 0
    hs0 = 6
    for k, hs in enumerate((hs0, hs0 + 1, hs0 + 2)):          # propose h = 0 | resolve it, propose h = 1 | resolve it, collect
        resolve, propose = k > 0, k < 2
        state, state_lp = d_w.cpu().numpy(), d_lp.cpu().numpy()
        if resolve:
            prev = hs - 1
            prop_prev = d_prop.cpu().numpy()
            z_prev = SM.stretch_z(SM.words(seed, pos, prev, W)[1][:, (prev & 1)::2])
            lp_w = state_lp[:, (prev & 1)::2]
            lp_y = (lp_w + rng.normal(size=(N, W2)) * rng.choice([0.5, 3.0, 60.0], size=(N, W2))).astype(np.float32)
            lp_y = np.clip(lp_y, -100.0, 100.0)
            lp_y[rng.random((N, W2)) < 0.03] = -np.inf
            lp_y[rng.random((N, W2)) < 0.02] = np.nan
            d_lpy = t(lp_y)
        else:
            d_lpy = None
        stretch_step(d_w, d_lp, d_fx, d_lo, d_hi, d_lpy, d_prop, d_acc, d_out, d_olp, 1 if k == 2 else -1, seed, off, hs,
                     resolve, propose, max_fixed, d_tp, d_ta)
        torch.cuda.synchronize()
        after, after_lp = d_w.cpu().numpy(), d_lp.cpu().numpy()
        if resolve:
            flags = d_ta.cpu().numpy()
            a, b, c = _check_flags(lp_w, lp_y, z_prev, n_free, prop_prev, lo32, hi32, live, seed, pos, prev, W, flags)
            mism, excl, total = mism + a, excl + b, total + c
            fl = flags.astype(bool) & live[:, None]
            exp_w, exp_lp = state.copy(), state_lp.copy()
            exp_w[:, (prev & 1)::2] = np.where(fl[:, :, None], prop_prev, state[:, (prev & 1)::2])
            exp_lp[:, (prev & 1)::2] = np.where(fl, lp_y, lp_w)
            assert np.array_equal(after, exp_w) and np.array_equal(after_lp, exp_lp)
            assert (~fl | ((prop_prev >= lo32) & (prop_prev <= hi32)).all(-1)).all()       # outside the box: rejected
        else:
            assert np.array_equal(after, state) and np.array_equal(after_lp, state_lp)
        if propose:
            _check_proposals((D, W, hs), after, mask, live, seed, pos, hs, d_prop.cpu().numpy(), d_tp.cpu().numpy())
    print(f"D={D} W={W}: {total} flags, {mism} mismatches, {excl} near ties excluded ({excl / total:.4f})")
    assert mism == 0 and excl / total < 0.01
    # the accept counter, the collecting point (slots [W, 2 W - 3): the last three walkers dropped) and the NaN row
    flags_total = d_acc.cpu().numpy()
    assert flags_total[5] == 0 and (flags_total[live] <= W).all() and flags_total[live].sum() > 0
    out, olp = d_out.cpu().numpy(), d_olp.cpu().numpy()
    fin, fin_lp = d_w.cpu().numpy(), d_lp.cpu().numpy()
    assert (out[:, :W] == -9.0).all() and (olp[:, :W] == -9.0).all()
    assert np.array_equal(out[live, W:], fin[live, :W - 3]) and np.array_equal(olp[live, W:], fin_lp[live, :W - 3])
    assert (out[5] == -9.0).all() and (d_prop[5] == 7.5).all() and np.array_equal(fin[5], walkers[5])
    assert (d_tp[5] == -1).all() and (d_ta[5] == -1).all()


def test_step_kernel_refuses_bad_arguments():
    from synference_amd.conditional import stretch_step
    w = torch.zeros((3, 8, 2), device=DEV)
    lp, fx = torch.zeros((3, 8), device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV)
    prop, acc = torch.zeros((3, 4, 2), device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="free set"):
        stretch_step(w, lp, fx, None, None, None, prop, acc, None, None, -1, 1, 0, 0, False, True, 2)
    with pytest.raises(RuntimeError, match="walkers"):
        stretch_step(torch.zeros((3, 7, 2), device=DEV), lp, fx, None, None, None, prop, acc, None, None, -1, 1, 0, 0, False,
                     True, 0)
    with pytest.raises(RuntimeError, match="resolving"):
        stretch_step(w, lp, fx, None, None, None, prop, acc, None, None, -1, 1, 0, 1, True, True, 0)


# ---- 5. local parity along the device's own trajectory ----------------------------------------------------------------
TRAJ = dict(num_samples=75, num_walkers=16, burn_in=10, thin=2, num_init_samples=200)      # 10 + 5 * 2 = 20 steps


def _trajectory_checks(tag, post, oracle_lp, x, cond, D, seed=31, row_offset=3):
    N, W = len(x), TRAJ["num_walkers"]
    s, acc, lp, trace = post.sample_conditional_catalogue(x, cond, seed=seed, row_offset=row_offset, return_log_prob=True,
                                                           _trace=True, **TRAJ)
    assert len(trace) == 2 * 20 and s.shape == (N, 75, D)
    lo32, hi32 = post.prior.low.cpu().numpy(), post.prior.high.cpu().numpy()
    pos = row_offset + np.arange(N)
    fixed = trace[0]["fixed"].cpu().numpy()
    live, mask = fixed > 0, _mask_of(fixed, D)
    assert live.all()
    n_free = D - mask.sum(1)
    props = np.stack([r["prop"].cpu().numpy() for r in trace])                     # [40, N, W/2, D]
    ref = oracle_lp(props.reshape(-1, D).astype(np.float64),
                    np.tile(np.repeat(np.asarray(x, np.float64), W // 2, axis=0), (len(trace), 1))).reshape(props.shape[:3])
    mism = excl = total = 0
    worst = 0.0
    for k, r in enumerate(trace):
        assert r["half_step"] == k
        walkers, lp_state = r["walkers"].cpu().numpy(), r["lp"].cpu().numpy()
        prop, lp_prop, flags = props[k], r["lp_prop"].cpu().numpy(), r["accept"].cpu().numpy()
        z = _check_proposals((tag, k), walkers, mask, live, seed, pos, k, prop, r["partner"].cpu().numpy())
        both = np.isfinite(ref[k]) & np.isfinite(lp_prop)
        assert (np.isfinite(ref[k]) == np.isfinite(lp_prop)).all()
        worst = max(worst, float(np.abs(lp_prop - ref[k])[both].max()))
        a, b, c = _check_flags(lp_state[:, (k & 1)::2], lp_prop, z, n_free, prop, lo32, hi32, live, seed, pos, k, W, flags)
        mism, excl, total = mism + a, excl + b, total + c
        if k + 1 < len(trace):              # the next state is this one with the accepted proposals in place
            nxt = walkers.copy()
            nxt[:, (k & 1)::2] = np.where(flags.astype(bool)[:, :, None], prop, walkers[:, (k & 1)::2])
            assert np.array_equal(trace[k + 1]["walkers"].cpu().numpy(), nxt)
    print(f"{tag}: |lp_prop - oracle|max={worst:.3e}; {total} flags, {mism} mismatches, {excl} near ties; "
          f"acceptance {acc.cpu().numpy()}")
    assert worst < LOGP_TOL, worst
    assert mism == 0 and excl / total < 0.01
    a = acc.cpu().numpy()
    assert ((a > 0) & (a < 1)).all()
    return s, acc, lp


def _cond_for(theta, fixed_dims, N, lo, hi):
    """The test set's values of ``fixed_dims`` (moved into the inner 80 % of the box where they lie outside it), NaN elsewhere."""
    cond = np.full((N, theta.shape[1]), np.nan, dtype=np.float32)
    inner = np.clip(theta[:N], lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo)).astype(np.float32)
    cond[:, fixed_dims] = inner[:, fixed_dims]
    return cond


@pytest.mark.parametrize("name,fixed_dims", [("maf_small", [1]), ("nsf_odd", [0, 3]), ("nsfar_small", [2])])
def test_pipeline_follows_the_model_along_its_own_trajectory(name, fixed_dims):
    ospec, spec, flat, theta, x = _case(name)
    lo, hi = _box(ospec)
    post = _posterior(spec, flat, lo, hi)
    N = 5
    _trajectory_checks(name, post, lambda th, xx: oracle_log_prob(ospec, flat, th, xx), x[:N],
                       _cond_for(theta, fixed_dims, N, lo, hi), spec.D)


def test_one_parameter_flow_has_nothing_to_sample():
    ospec, spec, flat, theta, x = _case("maf_d1")
    lo, hi = _box(ospec)
    post = _posterior(spec, flat, lo, hi)
    with pytest.raises(ValueError, match="at least one free"):
        post.sample_conditional_catalogue(x[:5], _cond_for(theta, [0], 5, lo, hi), seed=1, **TRAJ)


def test_ensemble_runs_on_the_mixture_potential():
    from synference_amd.posterior import EnsemblePosterior
    ospec, spec, flat, theta, x = _case("nsf_odd")
    _, _, flat_b, _, _ = make_case("nsf_odd", seed=1, B=4)
    flat_b = flat_b.astype(np.float32)
    lo, hi = _box(ospec)
    w = [0.3, 0.7]
    ens = EnsemblePosterior([_posterior(spec, flat, lo, hi), _posterior(spec, flat_b, lo, hi)], weights=w, seed=3)
    pot = MM.ensemble_potential([ospec, ospec], [flat, flat_b], w, torch.float64)
    _trajectory_checks("ensemble nsf_odd", ens, lambda th, xx: pot(th, xx)[0], x[:5], _cond_for(theta, [0, 3], 5, lo, hi), spec.D)


# ---- 6. distribution --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["maf_small", "nsf_d2", "maf_d3"])
def test_draws_follow_the_conditional_density(name):
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    ospec, spec, flat, theta, x = _case(name)
    assert np.array_equal(g["x_row"], x[0]) and float(g["value"]) == float(theta[0, int(g["fixed_d"])])
    post = _posterior(spec, flat, g["lo"], g["hi"])
    rows = 16
    xs = np.repeat(x[:1], rows, axis=0)
    cond = np.full((rows, spec.D), np.nan, dtype=np.float32)
    cond[:, int(g["fixed_d"])] = g["value"]
    s, acc = post.sample_conditional_catalogue(xs, cond, num_samples=1024, seed=2024)
    s = s.cpu().double().numpy()
    assert np.isfinite(s).all() and (s[:, :, int(g["fixed_d"])] == np.float32(g["value"])).all()
    thr = 1.5 * float(g["model_ks"].max())
    ks = [SM.ks_distance(s[:, :, d].reshape(-1), g["grids"][k], g["cdfs"][k]) for k, d in enumerate(g["free"])]
    print(f"{name}: KS {ks} against threshold {thr:.4f} (model: {g['model_ks'].max(0)}); acceptance "
          f"{float(acc.mean()):.3f} (model {float(g['model_acceptance'].mean()):.3f})")
    assert max(ks) <= thr, (ks, thr)


# ---- 7. invariances ---------------------------------------------------------------------------------------------------
SMALL = dict(num_samples=40, num_walkers=16, burn_in=10, thin=2, num_init_samples=64)


def test_invariances(monkeypatch):
    import synference_amd.conditional as CD
    ospec, spec, flat, theta, x = _case("maf_small")
    lo, hi = _box(ospec)
    post = _posterior(spec, flat, lo, hi)
    N = 8
    cond = _cond_for(theta, [0], N, lo, hi)
    cond[2] = np.nan                          # nothing fixed: the exact sampler
    cond[6] = np.nan
    cond[4, 0] = hi[0] + 1.0                  # outside the box: a NaN row
    xs = x[:N]
    s, acc, lp = post.sample_conditional_catalogue(xs, cond, seed=77, return_log_prob=True, **SMALL)
    assert s.shape == (N, 40, spec.D) and s.dtype == torch.float32 and acc.shape == (N,) and lp.shape == (N, 40)
    # the same seed, the same bits
    s2, acc2, lp2 = post.sample_conditional_catalogue(xs, cond, seed=77, return_log_prob=True, **SMALL)
    assert torch.equal(s.nan_to_num(9e9), s2.nan_to_num(9e9)) and torch.equal(acc.nan_to_num(-1), acc2.nan_to_num(-1))
    assert torch.equal(lp.nan_to_num(9e9), lp2.nan_to_num(9e9))
    # two row blocks with row_offset, and small internal blocks: the bits of the single call
    sa, acca = post.sample_conditional_catalogue(xs[:3], cond[:3], seed=77, **SMALL)
    sb, accb = post.sample_conditional_catalogue(xs[3:], cond[3:], seed=77, row_offset=3, **SMALL)
    assert torch.equal(torch.cat([sa, sb]).nan_to_num(9e9), s.nan_to_num(9e9))
    assert torch.equal(torch.cat([acca, accb]).nan_to_num(-1), acc.nan_to_num(-1))
    monkeypatch.setattr(CD, "BLOCK_DRAWS", 2 * SMALL["num_init_samples"])
    s3, acc3 = post.sample_conditional_catalogue(xs, cond, seed=77, **SMALL)
    monkeypatch.undo()
    assert torch.equal(s3.nan_to_num(9e9), s.nan_to_num(9e9)) and torch.equal(acc3.nan_to_num(-1), acc.nan_to_num(-1))
    # rows with an empty mask are sample_catalogue's draws, bit for bit
    plain = post.sample_catalogue(xs, 40, seed=77)
    assert torch.equal(s[2], plain[2]) and torch.equal(s[6], plain[6]) and acc[2] == 1 and acc[6] == 1
    free_all, acc_all = post.sample_conditional_catalogue(xs, np.full((N, spec.D), np.nan), seed=77, **SMALL)
    assert torch.equal(free_all, plain) and (acc_all == 1).all()
    # the NaN row, and nothing else
    assert torch.isnan(s[4]).all() and torch.isnan(acc[4]) and torch.isnan(lp[4]).all()
    ok = [i for i in range(N) if i != 4]
    assert torch.isfinite(s[ok]).all() and torch.isfinite(lp[ok]).all()
    a = acc[[0, 1, 3, 5, 7]]
    assert ((a > 0) & (a < 1)).all()
    # inside the box, on the slice, and lp is the raw density at the draws
    lo_t, hi_t = post.prior.low, post.prior.high
    assert ((s[ok] >= lo_t) & (s[ok] <= hi_t)).all()
    for i in (0, 1, 3, 5, 7):
        assert (s[i, :, 0] == float(cond[i, 0])).all()
    ref = post.log_prob_catalogue(s[ok].reshape(-1, spec.D), torch.as_tensor(xs[ok]).repeat_interleave(40, 0),
                                  norm_posterior=False).reshape(len(ok), 40)
    err = float((ref - lp[ok]).abs().max())
    print(f"|lp - log_prob_catalogue|max = {err:.3e}")
    assert err < LOGP_TOL
    # the sbi-style single call
    chain_kw = {k: v for k, v in SMALL.items() if k != "num_samples"}
    one = post.sample_conditional((3, 5), x=xs[0], condition=cond[0], dims_to_sample=[1], seed=5, **chain_kw)
    assert one.shape == (3, 5, spec.D) and (one[..., 0] == float(cond[0, 0])).all()


# ---- 8. end to end ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted(tmp_path_factory):
    from synference_amd import SBI_Fitter
    from synference_amd.synthetic import make_catalogue
    x, theta, names = make_catalogue(3000, 8, 4, seed=2)
    f = SBI_Fitter("cond", names, [f"F{i}" for i in range(8)], feature_array=x, parameter_array=theta)
    out = tmp_path_factory.mktemp("models")
    f.run_single_sbi(model_type="maf", hidden_features=32, num_transforms=3, n_nets=1, training_batch_size=256,
                     learning_rate=2e-3, stop_after_epochs=3, max_num_epochs=8, random_seed=3, out_dir=str(out), verbose=False,
                     name_append="t", evaluate_model=False)
    return f


def test_fitter_end_to_end(fitted):
    import pandas as pd
    f = fitted
    N = 12
    X, y = f._X_test[:N].copy(), f._y_test[:N]
    name = f.simple_fitted_parameter_names[1]
    col = np.asarray(y[:, 1], dtype=np.float32).astype(np.float64)
    col[N // 2:] = np.nan                     # the second half has no fixed value
    X[2, 3] = np.nan                          # a masked row among the fixed ones
    df = pd.DataFrame(X, columns=f.feature_names)
    df["spec"] = col
    ckw = dict(num_walkers=16, burn_in=20, thin=2, num_init_samples=100)
    plain = f.fit_catalogue(df, num_samples=64, seed=9)
    table = f.fit_catalogue(df, num_samples=64, seed=9, fixed_parameters={name: "spec"}, conditional_kwargs=ckw)
    qcols = [f"{p}_{q}" for p in f.simple_fitted_parameter_names for q in (16, 50, 84)]
    free_rows = np.arange(N) >= N // 2
    for c in qcols:
        assert np.array_equal(plain[c].to_numpy()[free_rows], table[c].to_numpy()[free_rows]), c
    fixed_rows = np.array([i for i in range(N // 2) if i != 2])
    for q in (16, 50, 84):
        assert np.array_equal(table[f"{name}_{q}"].to_numpy()[fixed_rows], col[fixed_rows])
    acc = table["conditional_acceptance"].to_numpy()
    print("conditional_acceptance", acc)
    assert ((acc[fixed_rows] > 0) & (acc[fixed_rows] < 1)).all() and np.isnan(acc[free_rows]).all() and np.isnan(acc[2])
    assert np.isnan(table[qcols].to_numpy()[2]).all()
    others = [c for c in qcols if not c.startswith(name + "_")]
    assert np.isfinite(table[others].to_numpy()[fixed_rows]).all()
    assert not np.array_equal(table[others].to_numpy()[fixed_rows], plain[others].to_numpy()[fixed_rows])
    assert [c for c in table.columns if c not in plain.columns] == ["conditional_acceptance"]
    # a dict of arrays says the same as the column name
    t2 = f.fit_catalogue(df, num_samples=64, seed=9, fixed_parameters={name: col}, conditional_kwargs=ckw)
    assert all(np.array_equal(t2[c].to_numpy(), table[c].to_numpy(), equal_nan=True) for c in table.columns)
    s = f.sample_conditional_posterior(X[:2], {name: col[:2]}, num_samples=50, seed=4, **ckw)
    assert s.shape == (2, 50, len(f.fitted_parameter_names)) and s.dtype == np.float64 and np.isfinite(s).all()
    assert (s[:, :, 1] == col[:2, None]).all() and f.last_conditional_acceptance.shape == (2,)
    with pytest.raises(ValueError, match="Invalid sample method"):
        f.sample_posterior(X[:2], sample_method="emcee")
