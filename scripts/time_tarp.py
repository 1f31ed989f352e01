"""Developer probe: `sf_tarp_coverage` (csrc/sf_tarp.hip) timed with HIP events beside the numpy model of the test-suite
(tests/tarp_model.py) on the same machine's CPU, at the reference's own comment shape (200 rows x 1 000 draws x 6
parameters, sbi_runner.py:6618) and at the bench catalogue's shape (2 000 x 1 000 x 5), 200 bootstrap passes each.

    python scripts/time_tarp.py [--rounds 20] [--cpu-passes 2] [--write]

Per shape: the median and the minimum of `--rounds` calls bracketed by events on the call's stream (after warm-up calls
that also grow the scratch buffer), the bytes and operations the algorithm needs (the draws once, B N S (3 D + 1)
operations) and the model's time for `--cpu-passes` passes scaled to B.  `--write` puts the JSON under profiles/ and
rewrites the two rows of DESIGN.md section 3 between the `tarp-timing` markers.  Needs a GPU: no fallback."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [("reference comment shape", 200, 1000, 6), ("bench catalogue", 2000, 1000, 5)]
B = 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--cpu-passes", type=int, default=2)
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_tarp.py needs a GPU")
    import tarp_model as TM
    from synference_amd.features import tarp_coverage
    rows = []
    for name, N, S, D in SHAPES:
        x, theta = TM.gaussian_case(N, S, D, seed=7)
        xd, td = torch.as_tensor(x).cuda(), torch.as_tensor(theta).cuda()
        for k in range(3):
            tarp_coverage(xd, td, norm=True, bootstrap=True, num_bootstrap=B, seed=k)
        torch.cuda.synchronize()
        ms = []
        for k in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ecp, _ = tarp_coverage(xd, td, norm=True, bootstrap=True, num_bootstrap=B, seed=10 + k)   # ends in a D2H copy
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        value = float(abs(ecp[:, ecp.shape[1] // 2].mean() - 0.5))
        t0 = time.perf_counter()
        m = TM.tarp_coverage(x, theta, norm=True, bootstrap=True, num_bootstrap=args.cpu_passes, seed=10 + args.rounds - 1)
        cpu_pass = (time.perf_counter() - t0) / args.cpu_passes
        e_dev, _, c_dev, _ = tarp_coverage(xd, td, norm=True, bootstrap=True, num_bootstrap=args.cpu_passes,
                                           seed=10 + args.rounds - 1, return_counts=True)
        row = {"shape": name, "N": N, "S": S, "D": D, "num_bootstrap": B, "device_ms_median": float(np.median(ms)),
               "device_ms_min": float(np.min(ms)), "rounds": args.rounds, "tarp_value": value,
               "bytes_draws": 4 * N * S * D, "operations": B * N * S * (3 * D + 1),
               "cpu_model_s_per_pass": cpu_pass, "cpu_model_s_scaled_to_B": cpu_pass * B,
               "cells_off_the_float64_count": int((c_dev != m["counts"]).sum()), "cells": int(c_dev.size)}
        row["gop_per_s"] = row["operations"] / (row["device_ms_median"] * 1e-3) / 1e9
        rows.append(row)
        print(json.dumps(row))
    if args.write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "tarp_timing.json"), "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        table = "\n".join(
            f"| `sf_tarp_coverage` {r['N']} x {r['S']} x {r['D']}, {B} passes ({r['shape']}) | {r['device_ms_median']:.3f} ms "
            f"(min {r['device_ms_min']:.3f}) | {r['cpu_model_s_scaled_to_B']:.1f} s | {r['gop_per_s']:.0f} Gop/s |" for r in rows)
        p = os.path.join(ROOT, "DESIGN.md")
        s = open(p).read()
        s2 = re.sub(r"(<!-- tarp-timing -->\n)(.*?)(\n<!-- /tarp-timing -->)", lambda mo: mo.group(1) + table + mo.group(3), s,
                    flags=re.S)
        if s2 == s and table not in s:
            raise SystemExit("DESIGN.md has no tarp-timing markers")
        open(p, "w").write(s2)


if __name__ == "__main__":
    main()
