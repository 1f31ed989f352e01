#!/usr/bin/env python
"""Do two builds of the library compute the same sampler results, byte for byte?

    python scripts/compare_sampler_builds.py [--family maf|lampe] LIB_A LIB_B [--timeout SECONDS]

For each library in turn: two fresh child processes with SYNFERENCE_HIP_LIB set, one with the default environment and one with the
family's switch set (maf: SF_PERSIST_MIN=1, lampe: SF_AR_SAMP16=0 -- read once per process), one after the other, each under its
own time limit.  A child that exits non-zero or runs out of time ends the script: nothing more is started on the GPU after it.
Every child runs a fixed list of calls on small shapes (M = 37 contexts x S = 24 draws: partly filled tiles, two galaxies in one
tile), and the results of the two libraries are compared as bytes: one line per call.
--family maf (default): the 16-row MAF flows of tests/cases.py in both sampler arithmetics; the second child runs the narrow box only.
Compared: the draws, n_unfilled, the acceptance counts, the given-noise hook's output -- what does not depend on the schedule.
n_drawn is printed, not compared.  Exit status 0: every call identical.

--family lampe: the same call list over the autoregressive flows of the lampe backend (sf_nsfar.hip / sf_nsfar16.hip: the shapes
of both candidate engines), one arithmetic (sf_set_sampler_fp32 does not apply); the second child runs the whole list with
SF_AR_SAMP16=0, which puts the 64-candidate engine on the tile-eligible shapes.  Two more calls reach the interleaved walk of the
persistent loop: a whole catalogue of M x 128 >= 4096 slots, and a list of >= 4096 slots (the 4096-piece cover, with holes).
Observed on an MI355X: all four children of this family together take about 15 s, well inside the per-child limit.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOWS = ["maf_cfg1", "maf_d4", "maf_d3", "maf_nb1", "maf_sig2", "maf_small", "maf_span6", "maf_d2_span", "maf_span_h64"]
MODES = [-1, 0]          # sf_set_sampler_fp32: the per-kind default (MAF: fp32) and split bf16 x3
# KS 3 / 2 / 4 (two input tiles) with one tile per type, two tiles per type, the affine map; D = 1 and 33 units per type: 64-candidate engine
LAMPE_FLOWS = ["nsfar_cfg1", "nsfar_small", "nsfar_k4", "nsfar_two", "mafar_cfg1", "nsfar_d1", "nsfar_33"]
S_WALK, S_LIST = 128, 384   # M x S_WALK >= 4096: the catalogue is walked across its rows; every third slot of M x S_LIST: >= 4096 listed slots
M, S = 37, 24
NARROW_ACCEPT = 1.0 / 600.0   # per attempt: about one slot in six is still open after 1 024 attempts
NARROW_CAP = 4096             # ... and the ceiling ends the call


def child(out_path, narrow_only, family):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from cases import make_case
    from oracle import posterior as OP      # only to place the boxes: the same for both libraries
    from synference_amd import _lib
    from synference_amd.engine import HipFlow

    lib = _lib.load()
    res = {}
    lampe = family == "lampe"
    for name in (LAMPE_FLOWS if lampe else FLOWS):
        ospec, spec, flat, _, x = make_case(name, B=M, spread=0.2)
        D = spec.D
        free, _ = OP.sample(ospec, torch.as_tensor(flat), x[:16], 2000, 5, dtype=torch.float32)
        free = free.reshape(-1, D)

        def box(accept):   # central quantile range per dimension, `accept` of the draws inside were the dimensions independent
            q = 0.5 * (1.0 - accept ** (1.0 / D))
            return np.quantile(free, q, axis=0).astype(np.float32), np.quantile(free, 1.0 - q, axis=0).astype(np.float32)

        half, narrow = box(0.5), box(NARROW_ACCEPT)
        z = np.random.default_rng(3).normal(size=(M * S, D)).astype(np.float32)
        xz = np.repeat(x, S, axis=0)
        for mode in ([None] if lampe else MODES):
            if mode is not None:
                lib.sf_set_sampler_fp32(mode)
            f = HipFlow(spec, "cuda:0")
            f.set_params(torch.as_tensor(flat))
            f.set_sample_time_limit(60.0)
            key = "%s %s" % (name, "" if lampe else "mode=%d " % mode)
            leg = ""          # the second child's calls carry its switch in their names
            if lampe and os.environ.get("SF_AR_SAMP16") == "0":
                leg = " SF_AR_SAMP16=0"
            elif narrow_only:
                leg = " SF_PERSIST_MIN=1"

            def put(call, arr, unfilled=None, nd=None):
                res[key + call] = arr.cpu().numpy()
                if unfilled is not None:
                    res[key + call + " #unfilled"] = np.int64(unfilled)
                if nd is not None:
                    res[key + call + " #n_drawn"] = np.int64(nd.cpu().numpy().astype(np.int64).sum())

            got, nd = f.sample(x, S, narrow[0], narrow[1], seed=11, max_attempts=NARROW_CAP, return_counts=True)
            put("sample narrow box" + leg, got, f.last_unfilled, nd)
            if narrow_only:
                continue
            got, nd = f.sample(x, S, half[0], half[1], seed=7, return_counts=True)
            put("sample half box" + leg, got, f.last_unfilled, nd)
            out = torch.zeros((M, S, D), dtype=torch.float32, device="cuda:0")
            slots = torch.arange(0, M * S, 3, dtype=torch.int32, device="cuda:0")
            put("sample_slots every third" + leg, out, f.sample_slots(x, S, slots, out, half[0], half[1], seed=7))
            put("acceptance" + leg, f.acceptance(x, S, half[0], half[1], seed=5))
            th, _ = f.inverse_sampler(z, xz)
            put("inverse_from_noise_sampler rc=%d" % f.last_sampler_rc + leg, th)
            if lampe:
                got, nd = f.sample(x, S_WALK, half[0], half[1], seed=9, return_counts=True)
                put("sample half box %d x %d (walk across rows)" % (M, S_WALK) + leg, got, f.last_unfilled, nd)
                out = torch.zeros((M, S_LIST, D), dtype=torch.float32, device="cuda:0")
                slots = torch.arange(0, M * S_LIST, 3, dtype=torch.int32, device="cuda:0")
                put("sample_slots every third of %d x %d (%d slots)" % (M, S_LIST, len(slots)) + leg, out,
                    f.sample_slots(x, S_LIST, slots, out, half[0], half[1], seed=9))
    if not lampe:
        lib.sf_set_sampler_fp32(-1)
    torch.cuda.synchronize()
    np.savez(out_path, **res)


def run_children(lib_path, tmp, tag, timeout, family):
    """The two children of one library; returns their results, or None after a failure (nothing else may start then)."""
    res = {}
    switch = "SF_AR_SAMP16" if family == "lampe" else "SF_PERSIST_MIN"
    for leg, extra in (("default", {}), ("second", {switch: "0" if family == "lampe" else "1"})):
        out = os.path.join(tmp, "%s_%s.npz" % (tag, leg))
        env = dict(os.environ, SYNFERENCE_HIP_LIB=os.path.abspath(lib_path), **extra)
        if not extra:
            env.pop(switch, None)   # (the default leg must not inherit the switch)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", out, "--family", family] + (["--narrow-only"] if extra and family == "maf" else [])
        try:
            r = subprocess.run(cmd, env=env, timeout=timeout)
        except subprocess.TimeoutExpired:
            print("STOP: %s (%s leg) did not finish in %d s" % (lib_path, leg, timeout))
            return None
        if r.returncode != 0:
            print("STOP: %s (%s leg) exited with status %d" % (lib_path, leg, r.returncode))
            return None
        with np.load(out) as d:
            res.update({k: d[k] for k in d.files})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("libs", nargs="*", metavar="LIB")
    ap.add_argument("--family", choices=("maf", "lampe"), default="maf", help="flow family: the 16-row MAF flows (default) or the lampe backend's autoregressive flows")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--child", metavar="OUT.npz", help=argparse.SUPPRESS)
    ap.add_argument("--narrow-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.narrow_only, a.family)
        return 0
    if len(a.libs) != 2:
        ap.error("two libraries to compare")
    for p in a.libs:
        if not os.path.isfile(p):
            ap.error("no such library: " + p)
    with tempfile.TemporaryDirectory() as tmp:
        ra = run_children(a.libs[0], tmp, "a", a.timeout, a.family)
        rb = run_children(a.libs[1], tmp, "b", a.timeout, a.family) if ra is not None else None
    if ra is None or rb is None:
        return 2
    n_diff = 0
    for k in [k for k in ra if " #" not in k]:
        va, vb = ra[k], rb.get(k)
        same = vb is not None and va.shape == vb.shape and va.tobytes() == vb.tobytes()
        note = ""
        if k + " #unfilled" in ra:
            ua, ub = int(ra[k + " #unfilled"]), int(rb.get(k + " #unfilled", -1))
            same = same and ua == ub
            note += "  n_unfilled %d / %d" % (ua, ub)
        if k + " #n_drawn" in ra:
            note += "  n_drawn %d / %d (not compared)" % (int(ra[k + " #n_drawn"]), int(rb.get(k + " #n_drawn", -1)))
        if same:
            print("identical  %s (%d bytes)%s" % (k, va.nbytes, note))
        else:
            n_diff += 1
            nb = -1 if vb is None or va.shape != vb.shape else int((va.view(np.uint8) != vb.view(np.uint8)).sum())
            print("DIFFERENT  %s (%d of %d bytes differ)%s" % (k, nb, va.nbytes, note))
    missing = [k for k in rb if k not in ra]
    for k in missing:
        print("DIFFERENT  %s (only the second library ran it)" % k)
    n_diff += len(missing)
    print("%d calls compared, %d differ" % (len([k for k in ra if " #" not in k]), n_diff))
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
