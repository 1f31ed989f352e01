"""Developer probe: `sf_spectra_transform` (csrc/sf_spectra.hip) timed with HIP events on a library shaped like the
reference's spectral example -- N = 20 000 spectra of L = 8192 pixels (0.1 - 2 um, logarithmic), rebinned onto M = 1000
observed pixels (0.6 - 5.3 um) behind a prism-like resolution curve, R from 30 to 300 -- beside the numpy model of the
test-suite (tests/spectra_model.py, float64, one spectrum at a time as the reference's loop goes) on this machine's CPU.

    python scripts/time_spectra.py [--rows 20000] [--pixels 8192] [--out-pixels 1000] [--rounds 5] [--cpu-rows 2] [--write]

Prints ms per call (median and minimum of `--rounds` timings after a warm-up call at the same shape), spectra / s, Gaussian taps
/ s -- taps = sum over pixels of 2 ceil(4 sigma) + 1, counted on the host from the float64 widths of a sample of rows -- and the
model's seconds per spectrum.  `--write` rewrites the lines of DESIGN.md between the `spectra-timing` markers.  Needs a GPU:
no fallback."""
import argparse
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--pixels", type=int, default=8192)
    ap.add_argument("--out-pixels", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cpu-rows", type=int, default=2)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    import spectra_model as SM
    from synference_amd.spectra import spectra_features
    rng = np.random.default_rng(0)
    wave = np.geomspace(0.1, 2.0, a.pixels)
    observed = np.linspace(0.6, 5.3, a.out_pixels)
    curve_wave = np.linspace(0.5, 5.5, 11)
    curve_r = np.array([40.0, 32.0, 30.0, 36.0, 50.0, 75.0, 110.0, 155.0, 205.0, 255.0, 300.0])    # prism-like
    z = rng.uniform(0.5, 8.0, a.rows)
    x = torch.linspace(0.0, 1.0, a.pixels, device="cuda")
    flux = (torch.rand((a.rows, 1), device="cuda") * 1e3 + 10.0) * (0.3 + x) ** 1.5 * (1.0 + 0.2 * torch.rand((a.rows, a.pixels), device="cuda"))
    kw = dict(z=z, observed_wave=observed, resolution_curve_wave=curve_wave, resolution_curve_r=curve_r)
    out = torch.empty((a.rows, a.out_pixels), dtype=torch.float32, device="cuda")
    spectra_features(flux, wave, out=out, **kw)                                           # warm-up at the timed shape
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        spectra_features(flux, wave, out=out, **kw)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    dev_ms = float(np.median(ms))
    sample = rng.choice(a.rows, size=min(a.rows, 200), replace=False)
    taps = float(np.mean([np.sum(2 * np.ceil(4.0 * SM.sigma_pixels(wave, z[i], curve_wave, curve_r)) + 1) for i in sample])) * a.rows
    host = flux[:a.cpu_rows].cpu().numpy()
    t0 = time.perf_counter()
    rows = [SM.transform_spectrum(wave, host[i], z[i], observed, curve_wave, curve_r)[1] for i in range(a.cpu_rows)]
    cpu_s = (time.perf_counter() - t0) / a.cpu_rows
    got = out[:a.cpu_rows].cpu().numpy()
    err = max(float(np.abs(got[i] - rows[i]).max() / np.abs(rows[i]).max()) for i in range(a.cpu_rows))
    line = (f"`sf_spectra_transform`, {a.rows} spectra x {a.pixels} pixels -> {a.out_pixels} pixels, R 30 - 300 ({taps:.2e} taps, "
            f"{taps / a.rows / a.pixels:.0f} per pixel): {dev_ms:.1f} ms on the device (median of {a.rounds} HIP-event timings after a "
            f"warm-up call, min {min(ms):.1f}; the upload of the redshifts and of the small tables included) = "
            f"{a.rows / dev_ms * 1e3:.3g} spectra / s, {taps / dev_ms * 1e3:.3g} taps / s; the numpy model on the host CPU, one thread: "
            f"{cpu_s:.2f} s per spectrum (measured on {a.cpu_rows}); device against that model on those rows: {err:.1e} of the row "
            f"maximum.")
    print(line)
    if a.write:
        path = os.path.join(ROOT, "DESIGN.md")
        text = open(path).read()
        text = re.sub(r"(<!-- spectra-timing -->\n).*?(\n<!-- /spectra-timing -->)", lambda m_: m_.group(1) + line + m_.group(2), text,
                      flags=re.S)
        open(path, "w").write(text)


if __name__ == "__main__":
    main()
