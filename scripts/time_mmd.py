"""Developer probe: the MMD misspecification test (`misspecification.calc_misspecification_mmd`; `sf_rbf_rowsum`,
`sf_rbf_subset_sums`, csrc/sf_mmd.hip) timed at the headline shape -- N = 1e5 training rows, C = 20, M = 1e4 observed rows,
n_shuffle = 1000: 1e10 pair terms for the row sums and 1000 x 1e8 ordered pairs (half of them visited) for the null -- beside the
same statistic through chunked `torch.cdist` + `exp` with the same identity on the same GPU in the same run, and beside ONE
upstream-style shuffle (all three blocks of a fresh split evaluated again with torch), extrapolated to n_shuffle.

    python scripts/time_mmd.py [--n 100000] [--c 20] [--m 10000] [--shuffles 1000] [--budget 3.0] [--json PATH]

Per path: one warm-up call (which also grows the scratch buffer), then as many timed calls as fit `--budget` seconds (at least
3, at most 20), each bracketed by events on the call's stream; the median, the minimum and the spread (max / min) are
reported.  The parts (`rowsum` N x N, `subset_sums`, the device index generation) are timed on their own too.  The two paths'
results are compared (largest relative difference of the null's sums).  Needs a GPU: no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK_ELEMS = 1 << 27     # kernel values per chunk of the torch path (1 GiB of float64)


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


def torch_rowsum(base, query, c2, exclude_diag):
    """sum_i exp2(|q - b_i|^2 c2) per query through cdist, fp32 distances and fp64 sums; the diagonal term (1) taken off."""
    step = max(1, CHUNK_ELEMS // base.shape[0])
    out = [torch.exp2(torch.cdist(query[a:a + step], base) ** 2 * c2).sum(1, dtype=torch.float64)
           for a in range(0, query.shape[0], step)]
    out = torch.cat(out)
    return out - 1.0 if exclude_diag else out


def torch_subset_sums(z, idx, c2, r):
    pair = torch.empty(idx.shape[0], dtype=torch.float64, device=z.device)
    for s in range(idx.shape[0]):
        g = z[idx[s].long()]
        pair[s] = torch_rowsum(g, g, c2, True).sum()
    return pair, r[idx.long()].sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--c", type=int, default=20)
    ap.add_argument("--m", type=int, default=10_000)
    ap.add_argument("--shuffles", type=int, default=1000)
    ap.add_argument("--budget", type=float, default=3.0)
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mmd.py needs a GPU")
    from synference_amd import misspecification as MS
    N, Cn, M, S = args.n, args.c, args.m, args.shuffles
    g = torch.Generator(device="cuda").manual_seed(3)
    z = torch.randn((N, Cn), device="cuda", generator=g)
    zo = torch.randn((M, Cn), device="cuda", generator=g) + 0.02
    scale = MS.rbf_scale(z, 0)
    c2 = MS.c2_of(scale)
    doc = {"device": torch.cuda.get_device_name(0), "N": N, "C": Cn, "M": M, "n_shuffle": S, "scale": scale}

    r = MS.rbf_rowsum(z, z, c2, exclude_self=True)
    idx = MS._subsets_device(0, 0, S, N, M, "cuda")
    doc["hip_total"] = timed(lambda: MS.calc_misspecification_mmd(None, zo, z, "x_space", S, scale=scale, z_score=False,
                                                                   return_details=True), args.budget)
    doc["hip_rowsum_NxN"] = timed(lambda: MS.rbf_rowsum(z, z, c2, exclude_self=True), args.budget)
    doc["hip_subset_sums"] = timed(lambda: MS.rbf_subset_sums(z, idx, c2, r, check=False), args.budget)
    doc["device_index_generation"] = timed(lambda: MS._subsets_device(0, 0, S, N, M, "cuda"), args.budget)
    doc["bandwidth"] = timed(lambda: MS.rbf_scale(z, 0), args.budget)

    # the same identity through torch: the N x N row sums once, then one M x M block per shuffle
    n_t = min(S, 20)                                  # (the per-shuffle cost is constant: a few are timed, the rest scaled)
    doc["torch_rowsum_NxN"] = timed(lambda: torch_rowsum(z, z, c2, True), args.budget)
    doc["torch_subset_sums_per_shuffle"] = timed(lambda: torch_subset_sums(z, idx[:n_t], c2, r), args.budget)
    for k in ("ms_median", "ms_min"):
        doc["torch_subset_sums_per_shuffle"][k] /= n_t
    doc["torch_identity_total_ms"] = doc["torch_rowsum_NxN"]["ms_median"] + S * doc["torch_subset_sums_per_shuffle"]["ms_median"]

    # one upstream-style shuffle: the same split of the training rows, all three blocks evaluated again
    def upstream_one():
        x = z[idx[0].long()]
        mask = torch.ones(N, dtype=torch.bool, device="cuda")
        mask[idx[0].long()] = False
        y = z[mask]
        A = torch_rowsum(x, x, c2, True).sum()
        B = torch_rowsum(y, y, c2, True).sum()
        Cx = torch_rowsum(y, x, c2, False).sum()
        return A / (M * (M - 1)) + B / ((N - M) * (N - M - 1)) - 2 * Cx / (M * (N - M))
    doc["upstream_style_one_shuffle"] = timed(upstream_one, args.budget)
    doc["upstream_style_extrapolated_s"] = doc["upstream_style_one_shuffle"]["ms_median"] * S / 1e3

    # the two paths compute the same thing
    hp, hk = MS.rbf_subset_sums(z, idx[:4], c2, r, check=False)
    tp, tk = torch_subset_sums(z, idx[:4], c2, r)
    doc["max_rel_diff_pair_sum"] = float(((hp - tp).abs() / tp).max())
    doc["max_rel_diff_rowsum"] = float(((r[:4096] - torch_rowsum(z, z[:4096], c2, True)).abs() / r[:4096]).max())
    doc["hip_over_torch"] = doc["hip_total"]["ms_median"] / doc["torch_identity_total_ms"]
    pairs = float(N) * N + S * float(M) * M
    doc["pair_terms_per_s"] = pairs / (doc["hip_total"]["ms_median"] * 1e-3)
    print(json.dumps(doc, indent=1))
    print(f"HIP path {doc['hip_total']['ms_median'] / 1e3:.3f} s (rowsum {doc['hip_rowsum_NxN']['ms_median']:.1f} ms, subset sums "
          f"{doc['hip_subset_sums']['ms_median']:.1f} ms, indices {doc['device_index_generation']['ms_median']:.1f} ms); torch with the "
          f"same identity {doc['torch_identity_total_ms'] / 1e3:.3f} s; upstream-style full re-evaluation "
          f"{doc['upstream_style_extrapolated_s']:.1f} s for {S} shuffles")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(doc, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
