"""Developer probe: what the latents cost.

    python scripts/time_latent.py [--parent-lib PATH] [--repeats 5] [--iters 20] [--write]

1. ``to_noise`` against ``log_prob`` of the same handle at the bench shape (``maf_cfg1``, 2e6 rows) and at ``nsf_cfg3`` (1e6
   rows): per repeat the mean of ``--iters`` calls between two device events, after a warm-up call; ``--repeats`` repeats,
   median and spread (max - min).  With ``--parent-lib`` (a libsynference_hip.so built from the parent commit) the same
   ``log_prob`` timing runs in fresh child processes on that library and on this one, alternating, so that the parent's own
   run-to-run spread stands beside the difference.  The z store adds B D 4 bytes of writes: its time at the device-to-device
   copy bandwidth measured here is printed next to the difference.
2. ``latent_summary`` at 1e6 x 16, 100 bins.
3. TARP at 1000 draws per row as the comparison: ``sample_catalogue`` + ``tarp_coverage`` on ``--tarp-rows`` rows of the
   ``maf_cfg1`` catalogue (the (N, 1000, D) draw set of 1e6 rows would not fit), reported per row.
Needs a GPU: no fallback.  ``--write`` puts the JSON lines into profiles/latent_measurements.txt."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [("maf_cfg1", 2_000_000), ("nsf_cfg3", 1_000_000)]
NEW = ("sf_flow_to_noise", "sf_latent_summary")


def timed(fn, iters, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "spread_ms": float(np.max(ms) - np.min(ms)),
            "repeats_ms": [round(float(v), 4) for v in ms]}


def flows(args, with_to_noise):
    import torch
    from cases import make_case
    from synference_amd.engine import HipFlow
    rows = []
    for name, B in SHAPES:
        ospec, spec, flat, theta, x = make_case(name, B=B)
        f = HipFlow(spec, "cuda:0")
        f.set_params(torch.as_tensor(flat))
        td, xd = torch.as_tensor(theta).cuda(), torch.as_tensor(x).cuda()
        row = {"case": name, "rows": B, "D": spec.D, "log_prob": stats(timed(lambda: f.log_prob(td, xd), args.iters, args.repeats))}
        if with_to_noise:
            row["to_noise"] = stats(timed(lambda: f.to_noise(td, xd), args.iters, args.repeats))
            row["log_prob_again"] = stats(timed(lambda: f.log_prob(td, xd), args.iters, args.repeats))
            big = torch.empty(B * spec.D, dtype=torch.float32, device="cuda")
            cp = np.median(timed(lambda: big.clone(), args.iters, args.repeats))
            row["copy_gb_per_s"] = 2 * big.numel() * 4 / (cp * 1e-3) / 1e9
            row["z_store_ms_at_copy_bandwidth"] = big.numel() * 4 / (row["copy_gb_per_s"] * 1e9) * 1e3
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tarp-rows", type=int, default=20000)
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--log-prob-only", action="store_true", help="child mode: log_prob of the library in SYNFERENCE_HIP_LIB")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_latent.py needs a GPU")
    if args.log_prob_only:
        from synference_amd import _lib
        for n in NEW:                                   # (a library of the parent commit does not export them)
            _lib.PROTOTYPES.pop(n, None)
        print("CHILD " + json.dumps(flows(args, False)))
        return
    lines = []
    if args.parent_lib:
        for k in range(4):                              # parent, this, parent, this
            env = dict(os.environ)
            which = "parent" if k % 2 == 0 else "this"
            if which == "parent":
                env["SYNFERENCE_HIP_LIB"] = os.path.abspath(args.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--log-prob-only", "--repeats", str(args.repeats),
                                "--iters", str(args.iters)], env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise SystemExit(f"child ({which}) failed with {p.returncode}:\n{p.stderr[-2000:]}")
            got = [l for l in p.stdout.splitlines() if l.startswith("CHILD ")][-1][6:]
            lines.append({"what": f"log_prob, library of {which} commit, child {k}", "rows": json.loads(got)})
            print(json.dumps(lines[-1]), flush=True)
    lines.append({"what": "log_prob / to_noise / log_prob of one handle, this commit", "rows": flows(args, True)})
    print(json.dumps(lines[-1]), flush=True)

    from synference_amd.features import latent_summary, tarp_coverage
    z = torch.randn((1_000_000, 16), device="cuda")
    lines.append({"what": "latent_summary 1e6 x 16, 100 bins (ends in the copies of the results to the host)",
                  **stats(timed(lambda: latent_summary(z, 100), max(2, args.iters // 4), args.repeats)), "bytes_read": z.numel() * 4})
    print(json.dumps(lines[-1]), flush=True)

    from cases import make_case
    from synference_amd.estimator import FlowEstimator
    from synference_amd.posterior import FlowPosterior
    N = args.tarp_rows
    ospec, spec, flat, theta, x = make_case("maf_cfg1", B=N)
    post = FlowPosterior(FlowEstimator(spec, torch.as_tensor(flat), device="cuda:0").to("cuda:0"), None)
    td, xd = torch.as_tensor(theta).cuda(), torch.as_tensor(x).cuda()

    def tarp():
        sd = post.sample_catalogue(xd, 1000, seed=3)
        tarp_coverage(sd, td, norm=True, bootstrap=True, num_bootstrap=200, seed=4)

    def latent():
        zz, _ = post.to_noise_catalogue(td, xd)
        latent_summary(zz, 100)
    t_tarp = stats(timed(tarp, 1, args.repeats))
    t_lat = stats(timed(latent, max(2, args.iters // 4), args.repeats))
    lines.append({"what": f"maf_cfg1, {N} rows: 1000 draws per row + TARP (200 bootstrap passes) against to_noise + latent_summary",
                  "tarp": t_tarp, "latent": t_lat, "tarp_us_per_row": t_tarp["median_ms"] * 1e3 / N,
                  "latent_us_per_row": t_lat["median_ms"] * 1e3 / N})
    print(json.dumps(lines[-1]), flush=True)
    if args.write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "latent_measurements.txt"), "w") as fh:
            fh.write(f"# scripts/time_latent.py on {torch.cuda.get_device_name(0)}: --repeats {args.repeats} --iters {args.iters}\n")
            for l in lines:
                fh.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
