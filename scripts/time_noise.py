"""Developer probe: `sf_scatter_empirical` (csrc/sf_noise.hip) timed with HIP events at a library of 1e6 rows x 5 scatters x
20 bands (1e8 output elements, two float32 arrays written) beside the numpy + scipy form of the same algorithm on this
machine's CPU -- `scipy.stats.truncnorm.rvs` for the sigma draw, `numpy.random` for the noise, per band, as the reference
does it (noise_models.py:383-390, 818-880) -- on `--cpu-rows` library rows, scaled to the whole library.

    python scripts/time_noise.py [--rows 1000000] [--scatters 5] [--bands 20] [--rounds 5] [--cpu-rows 20000] [--write]

The one claim to check is that the device time is a small multiple of the time to write 8 bytes per output element at the
HBM rate (`--hbm-tbs`, default 8.0 TB/s, the MI355X's peak); the multiple found is printed.  `--write` rewrites the lines of
DESIGN.md section 13 between the `noise-timing` markers.  Needs a GPU: no fallback."""
import argparse
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def catalogue(n, seed):
    rng = np.random.default_rng(seed)
    f = 10 ** rng.uniform(-1.0, 2.5, n) * 1e-6
    e = 0.1e-6 * np.exp(0.25 * rng.normal(size=n)) + 0.01 * f
    return f + e * rng.normal(size=n), e


def cpu_scatter(model, flux_njy, n_scatters, rng):
    """The General AB model of the reference on the host: sigma from scipy's truncated normal, Gaussian scatter."""
    from scipy import stats
    f = np.repeat(flux_njy.astype(np.float64), n_scatters)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = -2.5 * np.log10(f * 1e-9) + 8.9
    mu, ss = model._mu_sigma_interpolator(x), model._sigma_sigma_interpolator(x)
    a = -mu / np.where(ss > 1e-9, ss, 1)
    s = stats.truncnorm.rvs(a=a, b=np.inf, loc=mu, scale=ss, size=len(x), random_state=rng)
    return x + rng.normal(size=len(x)) * s, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--scatters", type=int, default=5)
    ap.add_argument("--bands", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cpu-rows", type=int, default=20000)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    from synference_amd.features import scatter_empirical
    from synference_amd.noise_models import GeneralEmpiricalUncertaintyModel, pack_models
    models = []
    for c in range(a.bands):
        f, e = catalogue(5000, c)
        with np.errstate(invalid="ignore", divide="ignore"):
            m, me = -2.5 * np.log10(f) + 8.9, np.abs(2.5 / np.log(10) * e / f)
        models.append(GeneralEmpiricalUncertaintyModel(m, me, flux_unit="AB", num_bins=20, return_noise=True))
    packed = pack_models(models, "nJy", "AB")
    rng = np.random.default_rng(0)
    flux = torch.as_tensor((10 ** rng.uniform(1.5, 5.0, size=(a.rows, a.bands))).astype(np.float32)).cuda()
    scatter_empirical(flux[:1000], packed, n_scatters=a.scatters, seed=1)          # warm-up: module load, scratch
    torch.cuda.synchronize()
    ms = []
    for r in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = torch.empty((a.rows * a.scatters, a.bands), dtype=torch.float32, device="cuda")   # (allocation outside the events)
        del out
        e0.record()
        y, s = scatter_empirical(flux, packed, n_scatters=a.scatters, seed=r)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
        del y, s
    dev_ms = float(np.median(ms))
    elements = a.rows * a.scatters * a.bands
    floor_ms = elements * 8 / (a.hbm_tbs * 1e12) * 1e3
    t0 = time.perf_counter()
    host = flux[:a.cpu_rows].cpu().numpy()
    for c in range(a.bands):
        cpu_scatter(models[c], host[:, c], a.scatters, rng)
    cpu_s = (time.perf_counter() - t0) * a.rows / a.cpu_rows
    line = (f"`sf_scatter_empirical`, {a.rows} rows x {a.scatters} scatters x {a.bands} bands ({elements:.2e} elements, General AB "
            f"models, 20 bins): {dev_ms:.2f} ms on the device (median of {a.rounds} HIP-event timings, min {min(ms):.2f}, output "
            f"allocation included) = {dev_ms / floor_ms:.1f}x the {floor_ms:.2f} ms that writing 8 bytes per element takes at "
            f"{a.hbm_tbs:g} TB/s; numpy + scipy (`truncnorm.rvs`) on the host CPU, one thread: {cpu_s:.1f} s (measured on "
            f"{a.cpu_rows} rows, scaled).")
    print(line)
    if a.write:
        path = os.path.join(ROOT, "DESIGN.md")
        text = open(path).read()
        text = re.sub(r"(<!-- noise-timing -->\n).*?(\n<!-- /noise-timing -->)", lambda m_: m_.group(1) + line + m_.group(2), text,
                      flags=re.S)
        open(path, "w").write(text)


if __name__ == "__main__":
    main()
