"""Shared inputs of the noise-model tests (TEST INFRASTRUCTURE): a mock observed catalogue, the five bands of the
draw-for-draw comparison, the three regimes of the distribution tests, and the tolerance of the comparison -- measured on
the CPU (tests/test_cpu_noise_model.py) as the float32 evaluation of tests/noise_model.py against its float64 one."""
import numpy as np

from synference_amd.noise_models import (AsinhEmpiricalUncertaintyModel, GeneralEmpiricalUncertaintyModel, band_fields,
                                         pack_models)

N_ROWS, N_SCATTERS, SEED = 257, 3, 20251
BINS = (2, 7, 20, 33, 20)
# max over the 5 x 771 elements of |float32 model - float64 model| in units of each element's own scale (sigma for the
# flux, ss for the error), measured on these inputs with this seed (2.601e-2 sigma in band 0, whose sampled sigma comes as
# low as 6e-5 mag at a magnitude of 23, one float32 ulp of which is 1.9e-6; 3.26e-5 ss); the device bounds are 4x that: the
# margin covers hardware log / ncdfinv / sqrt forms that differ from libm by a few ulp
TOL_FLUX_MEASURED, TOL_ERR_MEASURED = 2.61e-2, 3.3e-5
TOL_FLUX_BOUND, TOL_ERR_BOUND = 4 * TOL_FLUX_MEASURED, 4 * TOL_ERR_MEASURED
SNR_MARGIN = 1e-5            # elements whose model SNR lies this close (relative) to the threshold may be left out ...
SNR_MAX_EXCLUDED = 2         # ... at most this many per band


def mock_catalogue(n=3000, seed=1):
    """(flux, error) in Jy: errors of about 0.1 uJy with a 25 % log-normal spread and a weak flux dependence."""
    rng = np.random.default_rng(seed)
    f = 10 ** rng.uniform(-1.0, 2.5, n) * 1e-6
    e = (0.1e-6 * np.exp(0.25 * rng.normal(size=n)) + 0.01 * f)
    f_obs = f + e * rng.normal(size=n)
    return f_obs, e


def ab_of(f_jy, e_jy):
    with np.errstate(invalid="ignore", divide="ignore"):
        return -2.5 * np.log10(f_jy) + 8.9, np.abs(2.5 / np.log(10) * e_jy / f_jy)


def five_models():
    f, e = mock_catalogue(6000, seed=2)
    m, me = ab_of(f, e)
    return [
        GeneralEmpiricalUncertaintyModel(m, me, flux_unit="AB", num_bins=2, log_bins=False, return_noise=True),
        GeneralEmpiricalUncertaintyModel(f * 1e6, e * 1e6, flux_unit="uJy", num_bins=7, sigma_clip=3.0, error_type="observed",
                                         min_samples_per_bin=1, return_noise=True),
        GeneralEmpiricalUncertaintyModel(m, me, flux_unit="AB", flux_bins=np.linspace(*np.nanquantile(m, [0.01, 0.99]), 21),
                                         upper_limits=True, treat_as_upper_limits_below=3.0,
                                         upper_limit_flux_behaviour="scatter_limit", upper_limit_flux_err_behaviour="sig_3",
                                         return_noise=True),
        AsinhEmpiricalUncertaintyModel(f, e, num_bins=33, log_bins=False, min_samples_per_bin=1, return_noise=True),
        AsinhEmpiricalUncertaintyModel(f, e, num_bins=20, log_bins=False, interpolation_flux_unit="nJy",
                                       error_type="empirical", min_samples_per_bin=1, return_noise=True),
    ]


FIVE_UNITS = (("nJy", "AB"), ("nJy", "uJy"), ("nJy", "AB"), ("nJy", "asinh"), ("nJy", "asinh"))


def five_bands():
    """The packed form of the five models, each with its own (input, output) unit, and the library fluxes in nJy."""
    models = five_models()
    bands, table = pack_models(models, [u[0] for u in FIVE_UNITS], [u[1] for u in FIVE_UNITS])
    rng = np.random.default_rng(7)
    flux = (10 ** rng.uniform(1.3, 5.3, size=(N_ROWS, 5))).astype(np.float32)
    flux[11, 0], flux[12, 0] = 0.0, -40.0
    return models, bands, table, flux


def regimes():
    """name -> (model, constant flux, mu, ss): the sigma distribution N(mu, ss) truncated to sigma >= 0."""
    mk = lambda c, med, std, **kw: GeneralEmpiricalUncertaintyModel(            # noqa: E731
        np.array(c, float), None, flux_unit="uJy", already_binned=True, bin_median_errors=np.array(med, float),
        bin_std_errors=np.array(std, float), sigma_clip=3.0, return_noise=True, **kw)
    return {
        "ratio_0.5": (mk([1.0, 100.0], [0.5, 0.5], [1.0, 1.0]), 50.0, 0.5, 1.0),
        "ratio_8": (mk([1.0, 100.0], [2.0, 2.0], [0.25, 0.25]), 50.0, 2.0, 0.25),
        "extrapolated": (mk([10.0, 20.0], [1.0, 0.5], [0.2, 0.2], extrapolate=True), 32.0, -0.1, 0.2),
    }


REGIME_SEEDS = {"ratio_0.5": 1, "ratio_8": 2, "extrapolated": 5}    # float64 model: every p-value above 1e-2
KS_ROWS = 20000


def ks_pvalues(model, flux0, mu, ss, y, s):
    """KS p-values of the returned errors against the truncated normal of p(sigma | flux), and of the noise in units of the
    error against a normal truncated to +-3."""
    from scipy import stats
    a = -mu / ss
    p_sigma = stats.kstest(np.asarray(s, np.float64), stats.truncnorm(a, np.inf, loc=mu, scale=ss).cdf).pvalue
    z = (np.asarray(y, np.float64) - flux0) / np.asarray(s, np.float64)
    p_noise = stats.kstest(z, stats.truncnorm(-3, 3).cdf).pvalue
    return p_sigma, p_noise


def compare(got_y, got_s, ref, label=""):
    """got (device or float32 model) against the float64 model's dict of one band: the NaN / inf pattern is identical; the
    largest error in units of each element's own scale, with at most SNR_MAX_EXCLUDED elements near the SNR threshold left
    out.  Returns (flux figure, error figure, elements left out)."""
    near = ref["margin"] < SNR_MARGIN
    assert near.sum() <= SNR_MAX_EXCLUDED, (label, int(near.sum()))
    out = []
    for got, want, scale in ((got_y, ref["y"], ref["flux_scale"]), (got_s, ref["s"], ref["err_scale"])):
        got, want = np.asarray(got, np.float64)[~near], np.asarray(want, np.float64)[~near]
        assert np.array_equal(np.isnan(got), np.isnan(want)), (label, "NaN pattern")
        inf = np.isinf(want)
        assert np.array_equal(got[inf], want[inf]), (label, "inf pattern")
        ok = np.isfinite(want)
        assert np.isfinite(got[ok]).all(), (label, "finite pattern")
        sc = scale[~near][ok]
        assert (sc > 0).all(), (label, "scale")
        out.append(float(np.max(np.abs(got[ok] - want[ok]) / sc)) if ok.any() else 0.0)
    return out[0], out[1], int(near.sum())
