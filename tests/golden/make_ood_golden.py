"""Writes tests/golden/ood/ood_<case>.npz (a directory of their own: tests/test_golden.py takes every tests/golden/*.npz for a
flow fixture): the inputs of the out-of-distribution fixtures (tests/ood_model.py ``make_case``; stored,
because default_rng streams are not a contract) and what scikit-learn and scipy give on them -- LocalOutlierFactor decision
values and offset, NearestNeighbors distances, gaussian_kde densities, the chi-square and F quantiles of the two statistical
thresholds.  Needs scikit-learn and scipy (written with 1.7 / 1.15); the tests need neither.

    python tests/golden/make_ood_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import ood_model as OM  # noqa: E402

CONTAMINATION = 0.1
CONFIDENCE = 0.95


def main():
    import scipy
    import sklearn
    from scipy import stats
    from sklearn.neighbors import LocalOutlierFactor, NearestNeighbors
    for name, (N, C, M, k) in OM.CASES.items():
        base, query = OM.make_case(N, C, M, seed=sum(map(ord, name)))
        b64, q64 = base.astype(np.float64), query.astype(np.float64)
        lof = LocalOutlierFactor(n_neighbors=k, novelty=True, contamination=CONTAMINATION).fit(b64)
        nn = NearestNeighbors(n_neighbors=k, algorithm="brute").fit(b64)
        kde = stats.gaussian_kde(b64.T)
        out = dict(base=base, query=query, k=np.int64(k),
                   lof_decision=lof.decision_function(q64), lof_offset=np.float64(lof.offset_),
                   lof_nof_head=lof.negative_outlier_factor_[:64],
                   nn_dist=nn.kneighbors(q64)[0], nn_self_kth=nn.kneighbors()[0][:, -1],
                   kde_density=kde(q64.T), kde_base_density_head=kde(b64[:64].T), kde_factor=np.float64(kde.factor),
                   chi2_ppf=np.float64(stats.chi2.ppf(CONFIDENCE, C)), f_ppf=np.float64(stats.f.ppf(CONFIDENCE, C, N - C)),
                   kde_base_percentile=np.float64(np.percentile(kde(b64.T), (1 - CONFIDENCE) * 100)),
                   versions=np.array([sklearn.__version__, scipy.__version__]))
        # the fixtures' margins: at most 5 % of the rows may be undecidable (asserted again by tests/test_cpu_ood.py)
        for method in ("lof", "kde"):
            frac = OM.fixture_undecidable(base, query, method, k).mean()
            assert frac <= 0.05, (name, method, frac)
        os.makedirs(os.path.join(HERE, "ood"), exist_ok=True)
        path = os.path.join(HERE, "ood", f"ood_{name}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 200_000


if __name__ == "__main__":
    main()
