"""L-C2ST on the device (csrc/sf_lc2st.hip, synference_amd/lc2st.py) against the numpy model (tests/lc2st_model.py), whose
classifier arithmetic tests/test_cpu_lc2st.py pins to sklearn.  Tolerances are multiples of the gap between the model in
float32 and the model in float64 on the same case, computed here -- never a number taken from the device.  Every test prints
what it measures before it asserts."""
import numpy as np
import pytest
import torch

import lc2st_model as LM

pytestmark = pytest.mark.gpu

# (name, D, C, W, N, data seed, test seed): a ragged last minibatch (599 training rows), a partial 32-row sub-chunk and widths
# that are no multiple of 4 / 16; the LDS limit; less than one minibatch.
# The seeds were chosen on the CPU with the model: over the 5 epochs no validation row of any of the 4 classifiers has
# |logit| < 1e-4 (the smallest the model meets: 1.3e-3, 2.3e-3 and 0.22; asserted again in test_validation_scores).
CASES = [("ragged", 3, 4, 30, 333, 1, 9), ("lds_limit", 16, 64, 128, 150, 2, 11), ("tiny", 1, 1, 10, 17, 3, 7)]
N_CLS, EPOCHS = 4, 5


def make_data(D, C, N, seed):
    rng = np.random.default_rng(seed)
    th = rng.standard_normal((N, D))
    A = rng.standard_normal((D, C)) / np.sqrt(D)
    xs = th @ A + 0.5 * rng.standard_normal((N, C))
    ps = 0.6 * th + 0.3 + 0.8 * rng.standard_normal((N, D))      # a posterior that is visibly off
    return th, xs, ps


def device_test(case, **kw):
    from synference_amd.lc2st import LC2ST
    name, D, C, W, N, dseed, seed = case
    th, xs, ps = make_data(D, C, N, dseed)
    args = dict(seed=seed, num_trials_null=N_CLS - 1, hidden_width=W, max_iter=EPOCHS, n_iter_no_change=None)
    args.update(kw)
    return LC2ST(th, xs, ps, **args), (th, xs, ps)


def model_inputs(t, data, seed):
    """The model's own labels, split and init; the rows are the device's float32 rows (checked against the model's z-score)."""
    rows64, stats = LM.zscore(*data)
    rows = t.rows.cpu().numpy()
    assert np.abs(rows - rows64).max() <= 4e-7 * max(1.0, np.abs(rows64).max())
    N = len(data[0])
    lab = [LM.labels_for(seed, c, N) for c in range(t.n_cls)]
    vm = [LM.validation_mask(seed, c, lab[c]) for c in range(t.n_cls)]
    w0 = [LM.glorot_init(seed, c, t.n_in, t.W) for c in range(t.n_cls)]
    assert np.array_equal(np.stack(lab), t.labels.cpu().numpy()) and np.array_equal(np.stack(vm), t.vmask.cpu().numpy())
    return rows, lab, vm, w0, stats


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def trained(request):
    """Device and model (float64, float32) after 5 epochs without early stopping: computed once per case."""
    case = request.param
    t, data = device_test(case)
    t.train_all()
    rows, lab, vm, w0, stats = model_inputs(t, data, case[6])
    m64 = [LM.train(rows.astype(np.float64), lab[c], vm[c], w0[c], case[6], c, max_iter=EPOCHS) for c in range(N_CLS)]
    m32 = [LM.train(rows, lab[c], vm[c], w0[c], case[6], c, max_iter=EPOCHS, dtype=np.float32) for c in range(N_CLS)]
    return case, t, t.training_state(), m64, m32, stats, data


def test_training_parity(trained):
    case, t, st, m64, m32, _, _ = trained
    assert (st["n_iter"] == EPOCHS).all() and st["done"].all() and (st["best_iter"] == EPOCHS).all()
    for c in range(N_CLS):
        ref = m64[c]["weights"]
        scale = np.abs(ref).max()
        gap32 = float(np.abs(m32[c]["weights"].astype(np.float64) - ref).max() / scale)
        gap = float(np.abs(st["weights"][c].astype(np.float64) - ref).max() / scale)
        moved = float(np.abs(ref - LM.glorot_init(case[6], c, t.n_in, t.W)).max() / scale)
        print(f"{case[0]} clf {c}: device gap {gap:.3e}  float32-model gap {gap32:.3e}  bound {8 * gap32:.3e}  moved {moved:.3e}")
        assert moved > 100 * gap32                    # the comparison is about training, not about the initial weights
        assert gap <= 8 * gap32


def test_validation_scores(trained):
    case, t, st, m64, _, _, _ = trained
    for c in range(N_CLS):
        near = m64[c]["min_abs_val_logit"]
        print(f"{case[0]} clf {c}: device counts {st['validation_counts'][c, :EPOCHS]} model {m64[c]['counts']} "
              f"n_val {m64[c]['n_val']} smallest model |logit| {near:.3e}")
        assert near >= 1e-4                           # the seeds keep every validation row away from the decision boundary
        assert st["n_val"][c] == m64[c]["n_val"] and st["n_train"][c] == 2 * case[4] - m64[c]["n_val"]
        assert np.array_equal(st["validation_scores"][c, :EPOCHS], m64[c]["scores"])
        assert np.isnan(st["validation_scores"][c, EPOCHS:]).all()


STOP_SEED, STOP_W = 28, 6


def stop_test(**kw):
    """R = 2 x 400 rows of a one-dimensional threshold problem, not z-scored and scaled by 7, width 6: the decision boundary
    sweeps slowly through the rows, so the observed classifier finds a better validation accuracy at least every fourth
    epoch for the whole run.  Chosen on the CPU with the model (float64 and float32 agree): n_iter (60, 5, 5, 8), best_iter
    (59, 1, 1, 4) -- classifier 0 runs to max_iter, the null classifiers stop early."""
    from synference_amd.lc2st import LC2ST
    rng = np.random.default_rng(4)
    th = 7.0 * rng.uniform(0, 1, (400, 1))
    ps = -7.0 * rng.uniform(0, 1, (400, 1))
    xs = 0.7 * rng.standard_normal((400, 1))
    return LC2ST(th, xs, ps, seed=STOP_SEED, z_score=False, num_trials_null=N_CLS - 1, hidden_width=STOP_W, **kw)


def test_stopping_rule_on_the_device():
    """n_iter and best_iter follow from the device's own score log by the model's rule; the result is the best-score snapshot:
    bit-equal to a run without early stopping that ends at best_iter; one classifier runs to max_iter, others stop early."""
    t = stop_test(max_iter=60, n_iter_no_change=3)
    t.train_all()
    st = t.training_state()
    print("n_iter", st["n_iter"], "best_iter", st["best_iter"], "counts of classifier 0", st["validation_counts"][0])
    for c in range(N_CLS):
        n_iter, best_iter, _ = LM.apply_rule(st["validation_scores"][c], 3, 60)
        assert (st["n_iter"][c], st["best_iter"][c]) == (n_iter, best_iter)
    assert (st["n_iter"] < 60).any() and (st["n_iter"] == 60).any() and st["done"].all()
    for b in sorted(set(st["best_iter"].tolist())):
        t2 = stop_test(max_iter=int(b), n_iter_no_change=None)
        t2.train_all()
        w2 = t2.training_state()["weights"]
        for c in np.flatnonzero(st["best_iter"] == b):
            assert np.array_equal(w2[c], st["weights"][c]), (c, b)


def test_determinism_and_launch_split():
    case = CASES[0]
    th_o = np.random.default_rng(9).standard_normal((200, case[1]))

    def run(**kw):
        t, data = device_test(case, max_iter=12, n_iter_no_change=2, **kw)
        t.train_all()
        st = t.training_state()
        return st["weights"], st["validation_counts"], t.get_scores(th_o, data[1][0], trained_clfs=range(N_CLS)), t.p_value(th_o, data[1][0])
    a, b, one, other = run(), run(), run(epochs_per_launch=1), run(seed=case[6] + 1)
    print("p-values", a[3], b[3], one[3], other[3])
    for x, y, z in zip(a, b, one):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert not np.array_equal(a[0], other[0]) and not np.array_equal(a[2], other[2])


@pytest.mark.parametrize("S", [1000, 33])
def test_scores(trained, S):
    case, t, st, _, _, stats, data = trained
    rng = np.random.default_rng(S)
    th_o, x_o = rng.standard_normal((S, case[1])), data[1][1]
    probs, stat = t.get_scores(th_o, x_o, return_probs=True, trained_clfs=range(N_CLS))
    rows_o = LM.rows_at(th_o, x_o, stats)
    for c in range(N_CLS):
        w = st["weights"][c]
        p64, s64 = LM.scores(w, rows_o, t.n_in, t.W)
        p32, s32 = LM.scores(w, rows_o.astype(np.float32), t.n_in, t.W, dtype=np.float32)
        gp, gs = float(np.abs(p32 - p64).max()), abs(s32 - s64)
        dp, ds = float(np.abs(probs[c] - p64).max()), abs(stat[c] - s64)
        print(f"{case[0]} S={S} clf {c}: probs device {dp:.3e} float32-model {gp:.3e} | statistic device {ds:.3e} float32-model {gs:.3e}")
        assert dp <= 8 * gp and ds <= 8 * gs
    # the same numbers through every door
    assert np.array_equal(t.get_scores(th_o, x_o), stat[:1])
    assert np.array_equal(t.get_scores(th_o, x_o[None, :], trained_clfs=[2]), stat[2:3])
    assert np.array_equal(t.get_scores(th_o, x_o, trained_clfs=[3, 1]), stat[[3, 1]])
    assert t.get_statistic_on_observed_data(th_o, x_o) == stat[0]
    pn, sn = t.get_statistics_under_null_hypothesis(th_o, x_o, return_probs=True)
    assert np.array_equal(pn, probs[1:]) and np.array_equal(sn, stat[1:])
    x3 = data[1][[1, 5, 1]]
    p3, s3 = t.get_scores(np.stack([th_o, th_o[::-1], th_o]), x3, return_probs=True, trained_clfs=range(N_CLS))
    assert p3.shape == (3, N_CLS, S) and s3.shape == (3, N_CLS)
    assert np.array_equal(p3[0], probs) and np.array_equal(p3[2], probs) and np.array_equal(s3[0], stat)
    p5, s5 = t.get_scores(th_o[::-1], data[1][5], return_probs=True, trained_clfs=range(N_CLS))
    assert np.array_equal(p3[1], p5) and np.array_equal(s3[1], s5)
    assert t.p_value(th_o, x_o) == LM.p_value(stat[0], stat[1:]) and t.reject_test(th_o, x_o) == (t.p_value(th_o, x_o) < 0.05)


# ---- the decision on a toy with a known posterior ----------------------------------------------------------------------------
TOY_SEED = 2
TOY_KW = dict(num_trials_null=40, max_iter=100, n_iter_no_change=10)


def toy(shift):
    """theta ~ N(0, I_2), x = theta + 0.5 eps: the posterior is N(0.8 x, 0.2 I)."""
    rng = np.random.default_rng(100)
    N, S = 1000, 2000
    th = rng.standard_normal((N, 2))
    xs = th + 0.5 * rng.standard_normal((N, 2))
    sd = np.sqrt(0.2)
    ps = 0.8 * xs + sd * rng.standard_normal((N, 2)) + shift * sd
    x_o = np.array([0.5, -0.3])
    th_o = 0.8 * x_o + sd * rng.standard_normal((S, 2)) + shift * sd
    return th, xs, ps, th_o, x_o


@pytest.mark.parametrize("shift,model_p", [(0.0, 0.925), (1.0, 0.0)], ids=["exact", "shifted"])
def test_decision_on_a_known_posterior(shift, model_p):
    """``model_p``: the p-value of the numpy model run on the CPU with these seeds and settings (exact posterior 0.925, mean
    shifted by one posterior sigma 0.0; the device gave 0.9 and 0.0)."""
    from synference_amd.lc2st import LC2ST
    th, xs, ps, th_o, x_o = toy(shift)
    t = LC2ST(th, xs, ps, seed=TOY_SEED, **TOY_KW)
    t.train_all()
    p = float(t.p_value(th_o, x_o))
    print(f"shift {shift}: model p_value {model_p}  device p_value {p}  statistic {t.get_statistic_on_observed_data(th_o, x_o)}  n_iter {t.training_state()['n_iter']}")
    if shift == 0.0:
        assert p >= 0.05 and not t.reject_test(th_o, x_o)
    else:
        assert p < 0.05 and t.reject_test(th_o, x_o)


# ---- fitter level -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitter(tmp_path_factory):
    from synference_amd import SBI_Fitter
    from synference_amd.synthetic import make_catalogue
    x, theta, names = make_catalogue(3000, 6, 3, seed=1)
    f = SBI_Fitter("lc2st", names, [f"F{i}" for i in range(6)], feature_array=x, parameter_array=theta)
    f.run_single_sbi(model_type="maf", hidden_features=32, num_transforms=2, training_batch_size=256, learning_rate=2e-3,
                     stop_after_epochs=2, max_num_epochs=4, random_seed=3, out_dir=str(tmp_path_factory.mktemp("models")),
                     verbose=False, name_append="t", evaluate_model=False, save_model=False)
    return f, x, theta


def test_fitter_lc2st(fitter):
    f, x, theta = fitter
    kw = dict(X_test=x[:500], y_test=theta[:500], num_trials_null=20, num_posterior_samples=1000, seed=11, max_iter=30,
              n_iter_no_change=5)
    obs = x[600:603]
    r = f.lc2st(obs[0], **kw)
    assert f.last_lc2st is r
    print("p_value", r["p_value"], "statistic", r["statistic"], "n_iter", r["n_iter"])
    assert set(r) == {"p_value", "reject", "statistic", "null_statistics", "probs_data", "probs_null", "n_iter"}
    assert r["null_statistics"].shape == (20,) and r["probs_data"].shape == (1000,) and r["probs_null"].shape == (20, 1000)
    assert r["n_iter"].shape == (21,) and 0.0 <= r["p_value"] <= 1.0 and r["reject"] == (r["p_value"] < 0.05)
    assert r["statistic"] == np.mean((r["probs_data"].astype(np.float64) - 0.5) ** 2) or abs(
        r["statistic"] - np.mean((r["probs_data"].astype(np.float64) - 0.5) ** 2)) < 1e-9
    r2 = f.lc2st(obs[0][None, :], **kw)
    for k in r:
        assert np.array_equal(np.asarray(r[k]), np.asarray(r2[k])), k
    rm = f.lc2st(obs, **kw)
    assert f.last_lc2st is rm and rm["probs_null"].shape == (3, 20, 1000) and rm["p_value"].shape == (3,)
    for m in range(3):
        single = r if m == 0 else f.lc2st(obs[m], **kw)
        for k in single:
            assert np.array_equal(np.asarray(single[k]), rm[k][m]), (k, m)
