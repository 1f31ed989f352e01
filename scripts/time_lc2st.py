"""Developer probe: the L-C2ST classifiers (`sf_c2st_train`, csrc/sf_lc2st.hip) at the reference's size -- N = 10 000
calibration pairs, D = 6 parameters, C = 20 features, 1 + 100 classifiers of width 60 with sbi's settings (up to 1000 epochs,
early stopping after 50 epochs without improvement).

    python scripts/time_lc2st.py [--n 10000] [--trials 100] [--max-iter 1000] [--json PATH] [--no-host]

Reports the wall time of `LC2ST.train_all()` (host preparation of labels, splits and initial weights apart), the epochs run,
Adam steps per second per classifier (all classifiers run side by side, one workgroup each), the time of the scores at
S = 10 000 draws, and -- where scikit-learn is importable -- one `MLPClassifier.fit` on the same rows with the same settings
on the host, times the number of classifiers, as the cost of the reference path.  Needs a GPU: no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000)
    ap.add_argument("--trials", type=int, default=100)
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    from synference_amd.lc2st import BATCH, LC2ST
    D, C, N = 6, 20, a.n
    rng = np.random.default_rng(0)
    th = rng.standard_normal((N, D))
    xs = th @ (rng.standard_normal((D, C)) / np.sqrt(D)) + 0.5 * rng.standard_normal((N, C))
    ps = th + 0.35 * rng.standard_normal((N, D)) + 0.05           # a posterior that is slightly off
    t = LC2ST(th, xs, ps, seed=1, num_trials_null=a.trials, max_iter=a.max_iter)
    t0 = time.perf_counter()
    t._ensure()
    torch.cuda.synchronize()
    t_prep = time.perf_counter() - t0
    t0 = time.perf_counter()
    t.train_all()
    torch.cuda.synchronize()
    t_train = time.perf_counter() - t0
    st = t.training_state()
    steps = st["n_iter"].astype(np.int64) * (-(-st["n_train"] // BATCH))
    th_o = torch.as_tensor(rng.standard_normal((10_000, D)), device="cuda")
    t.p_value(th_o, xs[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p = t.p_value(th_o, xs[0])
    torch.cuda.synchronize()
    t_score = time.perf_counter() - t0
    out = {"N": N, "D": D, "C": C, "width": t.W, "classifiers": t.n_cls, "prepare_s": t_prep, "train_s": t_train,
           "epochs_total": int(st["n_iter"].sum()), "epochs_min": int(st["n_iter"].min()), "epochs_max": int(st["n_iter"].max()),
           "epochs_observed": int(st["n_iter"][0]), "adam_steps_total": int(steps.sum()),
           "steps_per_s_per_classifier": float(steps.max() / t_train), "steps_per_s_all": float(steps.sum() / t_train),
           "scores_s": t_score, "p_value": float(p)}
    if not a.no_host:
        try:
            from sklearn.neural_network import MLPClassifier
        except ImportError:
            MLPClassifier = None
        if MLPClassifier is not None:
            rows, lab = t.rows.cpu().numpy().astype(np.float64), t.labels[0].cpu().numpy()
            clf = MLPClassifier(hidden_layer_sizes=(t.W, t.W), activation="relu", solver="adam", max_iter=a.max_iter,
                                early_stopping=True, n_iter_no_change=50, random_state=1)
            t0 = time.perf_counter()
            clf.fit(rows, lab)
            t_host = time.perf_counter() - t0
            out.update({"host_one_fit_s": t_host, "host_one_fit_epochs": int(clf.n_iter_),
                        "host_all_fits_s": t_host * t.n_cls, "host_threads": torch.get_num_threads()})
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
