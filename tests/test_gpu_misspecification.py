"""The marginal-flow half of the misspecification tests on the device: MarginalTrainer / MarginalEstimator,
calc_misspecification_logprob and SBI_Fitter.detect_misspecification with both methods."""
import pickle
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _gaussian(n, seed=0):
    rng = np.random.default_rng(seed)
    A = np.array([[1.0, 0.0, 0.0], [0.8, 0.6, 0.0], [-0.5, 0.3, 0.4]])
    return (np.array([3.0, -1.0, 10.0]) + rng.normal(size=(n, 3)) @ A.T * np.array([2.0, 0.5, 5.0])).astype(np.float32)


@pytest.fixture(scope="module")
def trained():
    from synference_amd import misspecification as MS
    x = _gaussian(1024)
    trainer = MS.MarginalTrainer().append_samples(x)
    est = trainer.train(training_batch_size=128, max_num_epochs=5, seed=4)
    return trainer, est, x


def test_marginal_trainer(trained):
    from synference_amd import misspecification as MS
    trainer, est, x = trained
    s = est.summary
    print(f"kind {est.estimator.spec.kind}: loss before training {s['initial_loss']:.4f}, validation {s['validation_loss']}")
    assert isinstance(est, MS.MarginalEstimator) and trainer.estimator is est and est.n_features == 3
    assert est.estimator.spec.kind == "nsf_ar" and est.estimator.spec.C == 1 and est.estimator.spec.T == 5 and est.estimator.spec.H == 50
    assert s["best_validation_loss"][0] < s["initial_loss"] and len(s["validation_loss"]) >= 5
    xd = torch.as_tensor(x).cuda()
    with torch.no_grad():
        want = est.estimator.log_prob(xd, torch.zeros((len(x), 1), device="cuda"))
    got = est.log_prob(x)
    assert got.shape == (1024,) and torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert est.log_prob(x[5]).shape == (1,) and abs(float(est.log_prob(x[5])[0] - got[5])) < 1e-4
    draws = est.sample((64,), seed=3)
    assert draws.shape == (64, 3) and bool(torch.isfinite(draws).all())
    assert torch.equal(draws, est.sample((64,), seed=3)) and not torch.equal(draws, est.sample((64,), seed=4))
    with pytest.raises(ValueError):
        est.log_prob(x[:, :2])


def test_logprob_test_is_the_formula(trained):
    from synference_amd import misspecification as MS
    _, est, x = trained
    lp = est.log_prob(x).double().cpu().numpy()
    far = x[:4] + 10.0 * x.std(0)
    p, rej = MS.calc_misspecification_logprob(x, far[0], est)
    assert p == 0.0 and rej is True
    pm, rm = MS.calc_misspecification_logprob(x, far, est)
    lpf = est.log_prob(far).double().cpu().numpy()
    assert pm.shape == (4,) and np.array_equal(pm, (lp[None, :] < lpf[:, None]).mean(1)) and rm.all()
    mid = int(np.argsort(lp)[len(lp) // 2])                          # a training row at the median log-prob
    p, rej = MS.calc_misspecification_logprob(x, x[mid], est)
    assert p == float(np.mean(lp < lp[mid])) and abs(p - 0.5) < 0.01 and rej is False
    p2, rej2 = MS.calc_misspecification_logprob(x, x[mid], est, alpha=0.9)
    assert p2 == p and rej2 is True


@pytest.mark.parametrize("kind,backend", [("MAF", "lampe"), ("NSF", "sbi"), ("MAF", "sbi")])
def test_other_density_estimators_train(kind, backend):
    from synference_amd import misspecification as MS
    x = _gaussian(512, 1)
    est = MS.MarginalTrainer(kind, backend=backend).append_samples(x).train(training_batch_size=128, learning_rate=5e-3,
                                                                            max_num_epochs=5, seed=1)
    want = {("MAF", "lampe"): "maf_ar", ("NSF", "sbi"): "nsf", ("MAF", "sbi"): "maf"}[(kind, backend)]
    assert est.estimator.spec.kind == want
    tl = est.summary["training_loss"]
    print(f"{kind} {backend}: loss before training {est.summary['initial_loss']:.4f}, training loss per epoch {tl}")
    assert tl[-1] < tl[0] and tl[-1] < est.summary["initial_loss"]     # (training rows: the 51 validation rows are too few to rank)
    assert bool(torch.isfinite(est.log_prob(x)).all())


def test_one_feature_trains():
    from synference_amd import misspecification as MS
    x = _gaussian(512, 2)[:, :1]
    est = MS.MarginalTrainer().append_samples(x).train(training_batch_size=128, learning_rate=5e-3, max_num_epochs=5, seed=1)
    tl = est.summary["training_loss"]
    assert tl[-1] < tl[0] and tl[-1] < est.summary["initial_loss"] and est.sample((8,)).shape == (8, 1)


@pytest.fixture(scope="module")
def fitter():
    from synference_amd import SBI_Fitter
    from synference_amd.synthetic import make_catalogue
    x, theta, names = make_catalogue(1500, 6, 3, seed=1)
    f = SBI_Fitter("mis", names, [f"F{i}" for i in range(6)], feature_array=x, parameter_array=theta)
    f._X_train = np.asarray(x[:1200], dtype=np.float32)
    return f, np.asarray(x, dtype=np.float32)


def _state_bytes(f, tmp_path, tag, monkeypatch):
    monkeypatch.setattr(time, "strftime", lambda *a: "20000101_000000")
    with open(f.save_state(str(tmp_path), tag, save_method="pickle"), "rb") as fh:
        return fh.read()


def test_detect_misspecification(fitter, tmp_path, monkeypatch):
    f, x = fitter
    before = _state_bytes(f, tmp_path, "a", monkeypatch)
    obs = x[1200:1260]
    kw = dict(training_batch_size=128, max_num_epochs=3)
    r = f.detect_misspecification(obs[0], seed=5, **kw)
    assert f.last_misspecification is r and set(r) == {"method", "p_value", "reject", "log_prob_obs", "log_prob_train"}
    assert r["method"] == "logprob" and 0.0 <= r["p_value"] <= 1.0 and r["reject"] == (r["p_value"] < 0.05)
    assert r["log_prob_train"].shape == (1200,) and r["p_value"] == float(np.mean(r["log_prob_train"] < r["log_prob_obs"]))
    est = f.marginal_trainer_est
    assert est is not None and f.marginal_trainer.estimator is est
    r2 = f.detect_misspecification(obs[0], seed=6, **kw)                       # retrain=False: the kept flow, whatever the seed
    assert f.marginal_trainer_est is est and r2["p_value"] == r["p_value"] and r2["log_prob_obs"] == r["log_prob_obs"]
    rm = f.detect_misspecification(obs[:5], **kw)
    assert rm["p_value"].shape == (5,) and abs(rm["p_value"][0] - r["p_value"]) <= 2 / 1200 and rm["log_prob_obs"].shape == (5,)
    assert abs(rm["log_prob_obs"][0] - r["log_prob_obs"]) < 1e-4 and rm["reject"].shape == (5,)
    r3 = f.detect_misspecification(obs[0], retrain=True, seed=6, plot=True, **kw)
    assert f.marginal_trainer_est is not est and f.last_misspecification is r3
    shifted = f.detect_misspecification(obs[0] + 10.0 * x.std(0), **kw)
    assert shifted["p_value"] == 0.0 and shifted["reject"] is True

    g = f.detect_misspecification(obs, method="mmd", n_shuffle=50, seed=5)
    assert f.last_misspecification is g
    assert set(g) == {"method", "p_value", "reject", "mmd", "mmds_baseline", "mmd2", "null_mmd2", "scale"}
    assert g["method"] == "mmd" and g["null_mmd2"].shape == (50,) and g["mmds_baseline"].shape == (50,) and g["scale"] > 0
    assert g["p_value"] == float(np.mean(g["null_mmd2"] > g["mmd2"])) and g["reject"] == (g["p_value"] < 0.05)
    assert g["p_value"] >= 0.05                                                  # rows of the same catalogue
    g2 = f.detect_misspecification(obs, method="mmd", n_shuffle=50, seed=5)
    assert g2["mmd2"] == g["mmd2"] and np.array_equal(g2["null_mmd2"], g["null_mmd2"])
    far = f.detect_misspecification(obs + 0.5 * x.std(0), method="mmd", n_shuffle=50, seed=5)
    assert far["p_value"] == 0.0 and far["reject"] and far["mmd"] > g["mmd"]
    assert _state_bytes(f, tmp_path, "a", monkeypatch) == before                # save_state writes what it wrote before
    assert not any("marginal" in k or "misspec" in k for k in pickle.loads(before))
