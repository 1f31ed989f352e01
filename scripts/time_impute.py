"""Developer probe: the missing-band path (`sf_impute_missing`, csrc/sf_impute.hip; `MissingPhotometryHandler.process_catalogue`,
synference_amd/missing.py) timed with HIP events, on the bench MAF (C = 10, D = 5) and a synthetic library of 1e5 and of 1e6
rows: 1 000 objects with one and with three missing bands, nmc = 100, nposterior = 1000 (1e5 pooled draws per object).

    python scripts/time_impute.py [--rounds 3] [--objects 1000] [--cpu-objects 3] [--write]

Per case: the imputation stage alone; the whole `process_catalogue` (imputation, 1e8 posterior draws, pooled quantiles, the
small read-backs); the floor the new stages add to -- plain `sample_catalogue` over the same M * nmc context rows in the same
chunks -- and the numpy model of the test-suite (tests/impute_model.py) on `--cpu-objects` objects, scaled to M.  The
reference publishes 1.9 / 2.2 / 2.8 s per object for this procedure ("MC NSF").  `--write` puts the JSON
under profiles/ and rewrites the rows of DESIGN.md section 3 between the `impute-timing` markers.  Needs a GPU: no fallback."""
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

B = 10
RUN = {"nmc": 100, "nposterior": 1000}


def library(NT, M, n_missing, seed):
    """A two-parameter manifold with 0.05 mag scatter (the shape of tests/impute_model.make_case); objects are library
    rows moved by 0.03 mag, sigma 0.1 mag."""
    rng = np.random.default_rng(seed)
    a, c = rng.uniform(size=NT), rng.uniform(size=NT)
    lam = np.linspace(0.0, 1.0, B)
    train = (24.0 + 3.0 * a[:, None] + 2.0 * c[:, None] * lam[None, :] + 0.5 * np.sin(3.0 * lam[None, :] + 2.0 * a[:, None])
             + 0.05 * rng.normal(size=(NT, B))).astype(np.float32)
    obs = (train[rng.integers(NT, size=M)] + 0.03 * rng.normal(size=(M, B))).astype(np.float32)
    miss = np.zeros((M, B), bool)
    for m in range(M):
        miss[m, rng.choice(B, n_missing, replace=False)] = True
    obs[miss] = np.nan
    return train, obs, np.full((M, B), 0.1, np.float32), miss


def timed(fn, rounds):
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--objects", type=int, default=1000)
    ap.add_argument("--cpu-objects", type=int, default=3)
    ap.add_argument("--libraries", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_impute.py needs a GPU")
    import impute_model as IM
    from cases import make_case
    from synference_amd.estimator import FlowEstimator
    from synference_amd.missing import MissingPhotometryHandler
    from synference_amd.posterior import FlowPosterior
    from synference_amd.priors import CustomIndependentUniform
    ospec, spec, flat, theta, _ = make_case("maf_cfg1")
    est = FlowEstimator(spec, torch.as_tensor(flat), device="cuda:0").to("cuda:0")
    lo = (np.asarray(ospec.theta_mean) - 50.0 * np.asarray(ospec.theta_std)).astype(np.float32)
    hi = (np.asarray(ospec.theta_mean) + 50.0 * np.asarray(ospec.theta_std)).astype(np.float32)
    post = FlowPosterior(est, CustomIndependentUniform(lo, hi, [f"p{i}" for i in range(spec.D)], device="cuda:0"))
    M, nmc, S = args.objects, RUN["nmc"], RUN["nposterior"]
    rows = []
    for NT in args.libraries:
        for n_missing in (1, 3):
            train, obs, sigma, miss = library(NT, M, n_missing, seed=NT + n_missing)
            h = MissingPhotometryHandler(train, post, run_params=RUN)
            od, sd = torch.as_tensor(obs).cuda(), torch.as_tensor(sigma).cuda()
            h.impute(od, sd, miss, seed=1)                                     # warm-up: uploads the library, grows the scratch
            imp_med, imp_min, imp = timed(lambda: h.impute(od, sd, miss, seed=2), args.rounds)
            n_used = imp["n_used"].cpu().numpy()
            h.process_catalogue(obs[:8], sigma[:8], miss[:8], seed=3)
            all_med, all_min, res = timed(lambda: h.process_catalogue(obs, sigma, miss, seed=4), args.rounds)
            ctx = imp["imputed"].reshape(M * nmc, B)
            ctx = torch.where(torch.isfinite(ctx), ctx, torch.as_tensor(train[0]).cuda()[None, :])
            per = max(1, h.draw_budget_bytes // (4 * nmc * (S * spec.D + B)))

            def floor():
                for a in range(0, M, per):
                    post.sample_catalogue(ctx[a * nmc:(a + per) * nmc], S, 4, row_offset=a * nmc)
            floor_med, floor_min, _ = timed(floor, args.rounds)
            t0 = time.perf_counter()
            for m in range(args.cpu_objects):
                IM.impute_object(train, np.arange(B), None, obs[m], sigma[m], miss[m], m, 2, nmc)
            cpu = (time.perf_counter() - t0) / max(1, args.cpu_objects)
            row = {"library_rows": NT, "objects": M, "missing_bands": n_missing, "nmc": nmc, "nposterior": S,
                   "impute_ms_median": imp_med, "impute_ms_min": imp_min, "process_catalogue_ms_median": all_med,
                   "process_catalogue_ms_min": all_min, "plain_sampling_ms_median": floor_med, "plain_sampling_ms_min": floor_min,
                   "ms_per_object": all_med / M, "rounds": args.rounds, "neighbours_median": float(np.median(n_used[n_used > 0]))
                   if (n_used > 0).any() else 0.0, "neighbours_max": int(n_used.max()), "failed_objects": int((n_used <= 0).sum()),
                   "succeeded": int(res["success"].sum()), "cpu_model_imputation_s_per_object": cpu,
                   "cpu_model_imputation_s_scaled_to_M": cpu * M, "reference_published_s_per_object": 2.2}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "impute_timing.json"), "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        table = "\n".join(
            f"| {r['library_rows']:.0e} rows, {r['objects']} objects, {r['missing_bands']} missing | {r['impute_ms_median']:.2f} ms "
            f"(min {r['impute_ms_min']:.2f}) | {r['process_catalogue_ms_median']:.0f} ms | {r['plain_sampling_ms_median']:.0f} ms | "
            f"{r['ms_per_object']:.3f} ms | {r['cpu_model_imputation_s_scaled_to_M']:.0f} s |" for r in rows)
        p = os.path.join(ROOT, "DESIGN.md")
        s = open(p).read()
        s2 = re.sub(r"(<!-- impute-timing -->\n)(.*?)(\n<!-- /impute-timing -->)", lambda mo: mo.group(1) + table + mo.group(3), s,
                    flags=re.S)
        if s2 == s and table not in s:
            raise SystemExit("DESIGN.md has no impute-timing markers")
        open(p, "w").write(s2)


if __name__ == "__main__":
    main()
