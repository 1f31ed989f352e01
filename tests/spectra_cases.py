"""Shared inputs of the spectra tests (TEST INFRASTRUCTURE): small library spectra, redshifts, observed grids and resolution
curves from fixed seeds, the float64 model's answers (computed once per process), and the tolerance of the device comparison
-- measured on the CPU (tests/test_cpu_spectra_model.py) as the float32 evaluation of tests/spectra_model.py against its
float64 one.

Condition on every case (checked by the CPU suite): each pixel's float64 ``trunc * sigma`` lies at least ``TIE_MARGIN`` from
an integer and each ``sigma`` at least ``TIE_MARGIN`` from 0.01, so that a device that keeps the widths in fp64 takes the
same half-width and the same copy / convolve branch as the model on every pixel: no pixel is left out of a comparison."""
import functools

import numpy as np

import spectra_model as SM

TIE_MARGIN = 1e-6
# max over every case, row and output pixel of |float32 model - float64 model| / max|row of the float64 model| (output in
# nJy), measured on these inputs: 4.38e-7, stored rounded up so that another host's float32 exp can move it a little (the
# CPU suite asserts the measurement lies in [TOL_MEASURED / 1.5, TOL_MEASURED]): the float32 weights and tap sums of the
# convolution and the float32 products of the rebinning.  The device bound is 4x that, the margin the noise-model tests use
# for the same kind of comparison: the device exp is the fast intrinsic and its sums run in another order.
TOL_MEASURED = 4.5e-7
TOL_BOUND = 4 * TOL_MEASURED
Z_MAIN = (0.0, 0.5, 2.0, 3.7, 6.0)


def _spectra(rng, wave, n):
    """Positive continua (power laws with a break) with a few emission and absorption lines, in nJy, float32."""
    x = np.log(wave / wave[0]) / np.log(wave[-1] / wave[0])
    rows = []
    for _ in range(n):
        f = 10 ** rng.uniform(2.0, 4.0) * (0.3 + x) ** rng.uniform(-1.5, 2.0)
        f = f * (1.0 + 0.8 / (1.0 + np.exp(-(x - rng.uniform(0.2, 0.6)) * 60.0)))
        for _k in range(6):
            c, s, a = rng.uniform(0, 1), rng.uniform(0.002, 0.03), rng.uniform(-0.6, 3.0)
            f = f * (1.0 + a * np.exp(-0.5 * ((x - c) / s) ** 2))
        rows.append(f)
    return np.asarray(rows, np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(wave [L], flux [N, L] float32, z [N], observed [M], curve_wave, curve_r, theory_r)."""
    out = {}
    rng = np.random.default_rng(20260)
    wave = np.geomspace(0.1, 2.0, 301)
    observed = np.linspace(0.6, 5.0, 37)
    cw = np.array([0.5, 0.9, 1.4, 2.0, 2.7, 3.5, 4.4, 5.3])
    cr = np.array([30.0, 38.0, 55.0, 80.0, 120.0, 170.0, 230.0, 300.0])
    flux = _spectra(rng, wave, len(Z_MAIN))
    for tr in (np.inf, 100.0):
        out[f"main_r{tr:g}"] = dict(wave=wave, flux=flux, z=np.array(Z_MAIN), observed=observed, curve_wave=cw, curve_r=cr,
                                    theory_r=tr)
    wave2 = np.geomspace(0.1, 2.0, 1000)
    obs2 = np.concatenate([np.linspace(1.0, 1.05, 26), np.linspace(1.2, 4.8, 13)])    # bins inside one old bin; bins over dozens
    out["fine"] = dict(wave=wave2, flux=_spectra(rng, wave2, 3), z=np.array([0.5, 2.0, 3.7]), observed=obs2,
                       curve_wave=np.array([0.1, 1.0, 3.0, 9.0]), curve_r=np.array([10.0, 17.0, 33.0, 60.0]), theory_r=np.inf)
    out["l2"] = dict(wave=np.array([0.8, 1.3]), flux=np.array([[3.0, 5.0], [7.0, 2.0]], np.float32), z=np.array([0.0, 0.4]),
                     observed=np.linspace(0.7, 1.6, 5), curve_wave=cw, curve_r=cr, theory_r=np.inf)
    out["outside"] = dict(wave=wave, flux=flux[:2], z=np.array([0.0, 0.3]), observed=np.linspace(3.0, 5.0, 9), curve_wave=cw,
                          curve_r=cr, theory_r=np.inf)
    out["theory_r_array"] = dict(wave=wave, flux=flux[1:4], z=np.array([0.5, 2.0, 3.7]), observed=observed, curve_wave=cw,
                                 curve_r=cr, theory_r=np.linspace(60.0, 400.0, len(wave)))
    return out


def sigmas(case):
    """float64 sigma in pixels, [N, L]."""
    return np.stack([SM.sigma_pixels(case["wave"], z, case["curve_wave"], case["curve_r"], case["theory_r"]) for z in case["z"]])


@functools.lru_cache(maxsize=None)
def model(name, dtype=np.float64):
    """The model's transform_spectrum of every row of a case: [N, M] in ``dtype`` (computed once, do not modify)."""
    c = cases()[name]
    rows = [SM.transform_spectrum(c["wave"], c["flux"][i], c["z"][i], c["observed"], c["curve_wave"], c["curve_r"], c["theory_r"],
                                  dtype=dtype)[1] for i in range(len(c["z"]))]
    out = np.stack(rows)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model_convolved(name, dtype=np.float64):
    """The model's convolution alone of every row, with the case's float64 sigmas: [N, L]."""
    c = cases()[name]
    sg = sigmas(c)
    out = np.stack([SM.convolve(c["flux"][i], sg[i], 4.0, dtype) for i in range(len(c["z"]))])
    out.setflags(write=False)
    return out


def fitter_library(n=600, L=200, seed=5):
    """The end-to-end library: (grid (L, n) nJy, wave [L], parameters (n, 3): redshift, log mass, slope) whose spectra depend
    on the parameters, so that a flow has something to learn."""
    rng = np.random.default_rng(seed)
    wave = np.geomspace(0.1, 2.0, L)
    z = rng.uniform(0.5, 4.0, n)
    mass = rng.uniform(8.0, 11.0, n)
    slope = rng.uniform(-1.0, 1.5, n)
    x = np.log(wave / wave[0]) / np.log(wave[-1] / wave[0])
    grid = 10 ** (mass[None, :] - 7.0) * (0.3 + x[:, None]) ** slope[None, :] * \
        (1.0 + 0.8 / (1.0 + np.exp(-(x[:, None] - 0.35) * 60.0)))
    return grid.astype(np.float32), wave, np.stack([z, mass, slope], axis=1)
