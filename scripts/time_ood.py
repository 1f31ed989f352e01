"""Developer probe: the two all-pairs kernels of the out-of-distribution check (`sf_knn`, `sf_kde_logsumexp`, csrc/sf_ood.hip)
timed with HIP events at the workload's shapes -- library N = 1e5 and 1e6 rows, C = 10 and 20 features, catalogue M = 2 000
and 1e5 rows, k = 20 -- beside what plumbing alone does on the same GPU in the same run: chunked `torch.cdist` + `topk`
(and `logsumexp`), and, where scikit-learn is importable, NearestNeighbors(algorithm="brute") on the host for M = 2 000.

    python scripts/time_ood.py [--budget 3.0] [--quick] [--json PATH] [--from-json PATH] [--write]

Per shape and path: one warm-up call (which also grows the scratch buffer), then as many timed calls as fit `--budget`
seconds (at least 3, at most 20), each bracketed by events on the call's stream; the median, the minimum and the spread
(max / min) are reported, and 3 N M C lane operations per second against the packed-fp32 VALU peak (CUs x 64 lanes x 2 x
clock).  `--json` keeps the rows; `--write` (with this run's rows or `--from-json`) rewrites the table of DESIGN.md section 3
between the `ood-timing` markers.  Needs a GPU: no fallback."""
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

K = 20
SHAPES = [(N, C, M) for N in (100_000, 1_000_000) for C in (10, 20) for M in (2_000, 100_000)]
CHUNK_ELEMS = 1 << 28     # distances per chunk of the torch baseline (1 GiB of float32)


def timed(fn, budget):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    rounds = int(min(20, max(3, budget / max(time.perf_counter() - t0, 1e-6))))
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "spread": float(np.max(ms) / np.min(ms)),
            "rounds": rounds}


def torch_knn(base, query):
    step = max(1, CHUNK_ELEMS // base.shape[0])
    out = [torch.cdist(query[a:a + step], base).topk(K, dim=1, largest=False) for a in range(0, query.shape[0], step)]
    return torch.cat([o.values for o in out]), torch.cat([o.indices for o in out])


def torch_kde(base, query):
    step = max(1, CHUNK_ELEMS // base.shape[0])
    return torch.cat([torch.logsumexp(-0.5 * torch.cdist(query[a:a + step], base) ** 2, dim=1)
                      for a in range(0, query.shape[0], step)])


def table(rows):
    head = ("| N x C, M | `sf_knn` k=20 | cdist + topk | `sf_kde_logsumexp` | cdist + logsumexp | Top/s knn / kde (% of peak) | sklearn brute, host |\n"
            "|---|---|---|---|---|---|---|\n")
    lines = []
    for r in rows:
        sk = f"{r['sklearn_knn_s']:.2f} s" if r.get("sklearn_knn_s") is not None else "-"
        lines.append(f"| {r['N']:.0e} x {r['C']}, {r['M']:.0e} | {r['knn']['ms_median']:.2f} ms (min {r['knn']['ms_min']:.2f}, spread "
                     f"{r['knn']['spread']:.2f}) | {r['torch_knn']['ms_median']:.1f} ms | {r['kde']['ms_median']:.2f} ms (min "
                     f"{r['kde']['ms_min']:.2f}, spread {r['kde']['spread']:.2f}) | {r['torch_kde']['ms_median']:.1f} ms | "
                     f"{r['knn_tops']:.1f} / {r['kde_tops']:.1f} ({100 * r['knn_tops'] / r['peak_tops']:.0f} % / "
                     f"{100 * r['kde_tops'] / r['peak_tops']:.0f} %) | {sk} |")
    return head + "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--budget", type=float, default=3.0)
    ap.add_argument("--quick", action="store_true", help="the N = 1e5 shapes only")
    ap.add_argument("--json")
    ap.add_argument("--from-json")
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    if args.from_json:
        doc = json.load(open(args.from_json))
    else:
        if not torch.cuda.is_available():
            raise SystemExit("time_ood.py needs a GPU")
        from synference_amd import ood
        props = torch.cuda.get_device_properties(0)
        clock_khz = getattr(props, "clock_rate", 2_400_000)      # MI355X: 2.4 GHz peak engine clock where torch does not say
        peak = props.multi_processor_count * 64 * 2 * clock_khz * 1e3 / 1e12
        try:
            from sklearn.neighbors import NearestNeighbors
        except ImportError:
            NearestNeighbors = None
        rows = []
        g = torch.Generator(device="cuda").manual_seed(3)
        for N, C, M in SHAPES:
            if args.quick and N > 100_000:
                continue
            base = 25 + torch.randn((N, C), device="cuda", generator=g)
            query = 25 + torch.randn((M, C), device="cuda", generator=g)
            bw, qw = (base - 25).contiguous(), (query - 25).contiguous()
            row = {"N": N, "C": C, "M": M, "k": K, "peak_tops": peak,
                   "knn": timed(lambda: ood.knn(base, query, K), args.budget),
                   "torch_knn": timed(lambda: torch_knn(base, query), args.budget),
                   "kde": timed(lambda: ood.kde_logsumexp(bw, qw), args.budget),
                   "torch_kde": timed(lambda: torch_kde(bw, qw), args.budget)}
            ops = 3.0 * N * M * C
            row["knn_tops"] = ops / (row["knn"]["ms_median"] * 1e-3) / 1e12
            row["kde_tops"] = ops / (row["kde"]["ms_median"] * 1e-3) / 1e12
            # the same neighbours as the baseline on the first rows (the baseline's distances are not exact: rows only)
            ti = torch_knn(base, query[:64])[1]
            row["rows_equal_to_torch"] = float((ood.knn(base, query[:64], K)[1].long() == ti).float().mean())
            row["kde_max_abs_diff_to_torch"] = float((ood.kde_logsumexp(bw, qw[:64]) - torch_kde(bw, qw[:64]).double()).abs().max())
            row["sklearn_knn_s"] = None
            if NearestNeighbors is not None and M <= 2_000:
                b, q = base.cpu().numpy(), query.cpu().numpy()
                t0 = time.perf_counter()
                NearestNeighbors(n_neighbors=K, algorithm="brute").fit(b).kneighbors(q)
                row["sklearn_knn_s"] = time.perf_counter() - t0
            rows.append(row)
            print(json.dumps(row), flush=True)
            del base, query, bw, qw
        doc = {"device": torch.cuda.get_device_name(0), "rows": rows}
        if args.json:
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            json.dump(doc, open(args.json, "w"), indent=1)
    print(table(doc["rows"]))
    if args.write:
        p = os.path.join(ROOT, "DESIGN.md")
        s = open(p).read()
        s2 = re.sub(r"(<!-- ood-timing -->\n)(.*?)(\n<!-- /ood-timing -->)", lambda mo: mo.group(1) + table(doc["rows"]) + mo.group(3),
                    s, flags=re.S)
        if s2 == s and table(doc["rows"]) not in s:
            raise SystemExit("DESIGN.md has no ood-timing markers")
        open(p, "w").write(s2)


if __name__ == "__main__":
    main()
