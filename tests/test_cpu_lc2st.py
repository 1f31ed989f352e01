"""L-C2ST, host side: the numpy model (tests/lc2st_model.py) against sklearn's MLPClassifier -- the one place where this code
base can be pinned to the real upstream --, the stopping rule against sklearn's, the keyed order / labels / split as stated,
the product's own stream functions against the model's, and the public surface without a GPU."""
import ctypes as C
import inspect
import warnings

import numpy as np
import pytest
import torch

import lc2st_model as LM


def _problem(n=300, n_in=5, seed=0, noise=0.5):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, n_in))
    y = ((X[:, 0] + 0.5 * X[:, 1] ** 2 + noise * rng.standard_normal(n)) > 0.3).astype(np.uint8)
    return X, y


def test_model_training_loop_is_sklearns():
    """Warm-start injection (public API only): fit once with max_iter=1, overwrite coefs_ / intercepts_, fit again -- the
    second fit builds a fresh Adam and keeps the injected weights.  Full batch, no shuffle, 7 epochs."""
    sk = pytest.importorskip("sklearn.neural_network")
    n, n_in, W, epochs = 300, 5, 16, 7
    X, y = _problem(n, n_in)
    w0 = LM.glorot_init(3, 0, n_in, W).astype(np.float64)
    clf = sk.MLPClassifier(hidden_layer_sizes=(W, W), activation="relu", solver="adam", alpha=1e-4, batch_size=n,
                           learning_rate_init=1e-3, max_iter=1, shuffle=False, warm_start=True, tol=0.0, n_iter_no_change=10 ** 6,
                           early_stopping=False, random_state=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf.fit(X, y)
        coefs, intercepts = LM.unpack(w0, n_in, W)
        for dst, src in zip(clf.coefs_ + clf.intercepts_, coefs + intercepts):
            dst[...] = src
        clf.set_params(max_iter=epochs)
        clf.fit(X, y)
    res = LM.train(X, y, np.zeros(n, dtype=np.uint8), w0, 0, 0, max_iter=epochs, batch=n, shuffle=False)
    got = LM.pack(clf.coefs_, clf.intercepts_)
    err = float(np.abs(got - res["weights"]).max())
    print("max |w_model - w_sklearn| after", epochs, "epochs:", err)
    assert np.abs(got - w0).max() > 1e-3                     # the weights did move
    assert err < 1e-12
    p0 = 1.0 - LM.sigmoid(LM.logits(res["weights"], X, n_in, W)[0])
    perr = float(np.abs(clf.predict_proba(X)[:, 0] - p0).max())
    print("max |p_model - predict_proba[:, 0]|:", perr)
    assert perr < 1e-12


def test_stopping_rule_is_sklearns():
    sk = pytest.importorskip("sklearn.neural_network")
    X, y = _problem(400, 4, seed=5, noise=2.0)
    clf = sk.MLPClassifier(hidden_layer_sizes=(8, 8), early_stopping=True, n_iter_no_change=5, max_iter=300, random_state=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf.fit(X, y)
    n_iter, best_iter, best = LM.apply_rule(clf.validation_scores_, 5, 300)
    print("sklearn n_iter_", clf.n_iter_, "model", n_iter, "best", clf.best_validation_score_, best, "at", best_iter)
    assert clf.n_iter_ < 300                                 # the case does stop early
    assert n_iter == clf.n_iter_ == len(clf.validation_scores_)
    assert best == clf.best_validation_score_
    assert clf.validation_scores_[best_iter - 1] == best


@pytest.mark.parametrize("R", [1, 2, 199, 200, 201, 513])
def test_keyed_order_is_a_permutation(R):
    from synference_amd.lc2st import keyed_order
    a, b = LM.keyed_order(11, 3, 0, R), LM.keyed_order(11, 3, 1, R)
    assert sorted(a.tolist()) == list(range(R)) and sorted(b.tolist()) == list(range(R))
    if R >= 199:
        assert (a != b).any() and (a != np.arange(R)).any()
        assert (LM.keyed_order(11, 4, 0, R) != a).any() and (LM.keyed_order(12, 3, 0, R) != a).any()
    for e in (0, 1, 7):
        assert np.array_equal(keyed_order(11, 3, e, R), LM.keyed_order(11, 3, e, R))     # product == model


def test_labels_split_and_init_streams():
    from synference_amd import lc2st as P
    N, seed, n_cls = 123, 2 ** 40 + 17, 4
    lab = P.make_labels(seed, n_cls, N)
    vm = P.make_validation_mask(seed, lab)
    init = P.make_init(seed, n_cls, 7, 30)
    assert lab.dtype == np.uint8 and vm.dtype == np.uint8 and init.dtype == np.float32
    assert (lab[0, :N] == 0).all() and (lab[0, N:] == 1).all()
    for t in range(n_cls):
        assert np.array_equal(lab[t], LM.labels_for(seed, t, N))
        assert np.array_equal(vm[t], LM.validation_mask(seed, t, lab[t]))
        assert np.array_equal(init[t], LM.glorot_init(seed, t, 7, 30))
        assert int((lab[t] == 0).sum()) == N                                          # exactly N zeros
        for k in (0, 1):                                                              # stratified at 10 %
            assert int(vm[t][lab[t] == k].sum()) == (N + 5) // 10 == 12
    assert (lab[1] != lab[2]).any() and (vm[1] != vm[2]).any() and (lab[1] != lab[0]).any()
    o_b1, o_w2, o_b2, o_w3, o_b3, NP = LM.offsets(7, 30)
    assert init.shape == (n_cls, NP) == (n_cls, P.num_params(7, 30))
    for lo, hi, fan in ((0, o_w2, 7 + 30), (o_w2, o_w3, 60), (o_w3, NP, 31)):
        b = np.sqrt(6.0 / fan)
        assert np.abs(init[:, lo:hi]).max() <= b and np.abs(init[:, lo:hi]).max() > 0.8 * b


def test_float32_model_is_close_to_float64_model():
    """The device tolerances are multiples of this gap; it has to be small and not zero."""
    X, y = _problem(240, 6, seed=2)
    w0, vm = LM.glorot_init(1, 0, 6, 20), LM.validation_mask(1, 0, y)
    a = LM.train(X, y, vm, w0, 1, 0, max_iter=3)
    b = LM.train(X.astype(np.float32), y, vm, w0, 1, 0, max_iter=3, dtype=np.float32)
    gap = float(np.abs(a["weights"] - b["weights"]).max() / np.abs(a["weights"]).max())
    print("float32 / float64 model gap:", gap)
    assert b["weights"].dtype == np.float32 and 0 < gap < 1e-3


def _toy(N=40, D=2, Cx=3):
    rng = np.random.default_rng(0)
    return rng.standard_normal((N, D)), rng.standard_normal((N, Cx)), rng.standard_normal((N, D))


def test_argument_errors_and_limits():
    from synference_amd.lc2st import LC2ST
    th, xs, ps = _toy()
    sig = inspect.signature(LC2ST.__init__)
    assert [(k, v.default) for k, v in sig.parameters.items()][4:11] == [
        ("seed", 1), ("num_folds", 1), ("num_ensemble", 1), ("classifier", "mlp"), ("z_score", True), ("num_trials_null", 100),
        ("permutation", True)]
    for name in ("hidden_width", "max_iter", "n_iter_no_change", "timeout_seconds"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    for m in ("train_on_observed_data", "train_under_null_hypothesis", "get_scores", "get_statistic_on_observed_data",
              "get_statistics_under_null_hypothesis", "p_value", "reject_test"):
        assert callable(getattr(LC2ST, m))
    assert inspect.signature(LC2ST.reject_test).parameters["alpha"].default == 0.05
    with pytest.raises(ValueError, match="only 'mlp'"):
        LC2ST(th, xs, ps, classifier="random_forest")
    with pytest.raises(ValueError, match="only num_ensemble=1"):
        LC2ST(th, xs, ps, num_ensemble=5)
    with pytest.raises(ValueError, match="only num_folds=1"):
        LC2ST(th, xs, ps, num_folds=2)
    with pytest.raises(ValueError, match="permutation"):
        LC2ST(th, xs, ps, permutation=False)
    with pytest.raises(ValueError, match="W <= 128"):
        LC2ST(th, xs, ps, hidden_width=129)
    with pytest.raises(ValueError, match="n_in <= 80"):
        LC2ST(th, np.zeros((40, 79)), ps)
    with pytest.raises(ValueError, match="D <= 16"):
        LC2ST(np.zeros((40, 17)), xs, np.zeros((40, 17)))
    with pytest.raises(ValueError, match="do not agree"):
        LC2ST(th, xs[:-1], ps)
    t = LC2ST(np.zeros((40, 16)), xs, np.zeros((40, 16)))
    assert t.W == 128 and t.n_in == 19                                   # 10 D capped at 128
    assert LC2ST(th, xs, ps).W == 20


def test_no_cpu_fallback(monkeypatch):
    from synference_amd.lc2st import LC2ST
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    th, xs, ps = _toy()
    t = LC2ST(th, xs, ps, num_trials_null=2)
    for call in (t.train_on_observed_data, t.train_under_null_hypothesis, t.train_all):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="not trained"):
        t.get_statistic_on_observed_data(ps, xs[0])


def test_fitter_messages_are_the_references():
    from synference_amd import SBI_Fitter
    sig = inspect.signature(SBI_Fitter.lc2st)
    assert list(sig.parameters)[:5] == ["self", "x_obs", "posterior", "X_test", "y_test"]
    assert all(sig.parameters[k].default is None for k in ("posterior", "X_test", "y_test"))
    kw = {k: v.default for k, v in sig.parameters.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
    assert kw == {"num_posterior_samples": 10000, "num_trials_null": 100, "alpha": 0.05, "seed": None}

    class Bare:
        _X_train = _y_train = posteriors = None
    f = Bare()
    x = np.zeros(3, dtype=np.float32)
    with pytest.raises(ValueError) as e:
        SBI_Fitter.lc2st(f, x)
    assert str(e.value) == "No training data found. Please set the training data first."
    with pytest.raises(ValueError) as e:
        SBI_Fitter.lc2st(f, x, X_test=np.zeros((8, 3)))
    assert str(e.value) == "No training labels found. Please set the training labels first."
    with pytest.raises(ValueError) as e:
        SBI_Fitter.lc2st(f, x, X_test=np.zeros((8, 3)), y_test=np.zeros((8, 2)))
    assert str(e.value) == "No posterior found. Please set the posterior first."


def test_abi_refuses_bad_arguments(lib):
    from synference_amd._lib import sf_c2st_desc
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value            # never dereferenced: the checks come first

    def call(**kw):
        d = dict(n_in=5, width=16, n_cls=2, max_iter=10, n_iter_no_change=5, early_stopping=1, batch=200, R=100, seed=1,
                 lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, alpha=1e-4, tol=1e-4, rows=p, labels=p, vmask=p, init_weights=p)
        d.update(kw)
        h = C.c_void_p()
        return lib.sf_c2st_create(C.byref(sf_c2st_desc(**d)), C.byref(h), None)
    for kw in (dict(n_in=0), dict(n_in=81), dict(width=0), dict(width=129), dict(R=0), dict(R=2 ** 31), dict(n_cls=0),
               dict(max_iter=0), dict(batch=0), dict(rows=None), dict(labels=None), dict(vmask=None), dict(init_weights=None)):
        assert call(**kw) == -1, kw                                       # SF_ERR_INVALID
        assert b"sf_c2st_create" in lib.sf_last_error()
    assert call(n_in=81) == -1 and b"n_in must be 1 .. 80" in lib.sf_last_error()
    assert call(width=129) == -1 and b"hidden width must be 1 .. 128" in lib.sf_last_error()
    assert lib.sf_c2st_train(None, 0, 1, 1, 0, None, None) == -1
    assert lib.sf_c2st_scores(None, 0, 1, None, 1, None, None, None) == -1
    assert lib.sf_c2st_get(None, None, None, None, None) == -1
    if not torch.cuda.is_available():
        assert call() == -3 and b"no CPU fallback" in lib.sf_last_error()   # SF_ERR_NO_DEVICE


def test_product_does_not_import_the_test_side():
    src = (inspect.getsourcefile(__import__("synference_amd.lc2st", fromlist=["x"])))
    text = open(src).read()
    assert "import oracle" not in text and "from oracle" not in text and "import sklearn" not in text and "from sklearn" not in text
