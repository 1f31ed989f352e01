#!/usr/bin/env python
"""Record oracle/posterior.py's draws and attempt counts in the narrow box of tests/test_gpu_pipelined_passes.py.

    python scripts/make_pipelined_passes_golden.py [--jobs N]

No GPU.  Writes tests/golden/pipelined_passes/narrow.npz: per shape of tests/pipelined_passes_cases.py the box (lo, hi), the
draws of slots 0 .. 149 and the attempts each slot used.  About 10 s per shape (the oracle walks the attempts one by one)."""
import argparse
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def one(shape):
    import torch
    torch.set_num_threads(1)
    import pipelined_passes_cases as PC
    lo, hi, th, used = PC.narrow_reference(*shape)
    assert np.isfinite(th).all() and (used >= 1).all()
    # (the oracle computes in float32 and returns float64: the cast back is exact)
    assert np.array_equal(th.astype(np.float32).astype(np.float64), th)
    return lo, hi, th.astype(np.float32), used.astype(np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    import pipelined_passes_cases as PC
    with mp.get_context("spawn").Pool(a.jobs) as pool:
        res = pool.map(one, PC.GRID)
    out = {}
    for name, (lo, hi, th, used) in zip(PC.IDS, res):
        out[name + " lo"], out[name + " hi"], out[name + " draws"], out[name + " used"] = lo, hi, th, used
        print(name, "attempts per slot: median %d, max %d" % (np.median(used), used.max()))
    os.makedirs(os.path.dirname(PC.GOLDEN), exist_ok=True)
    np.savez_compressed(PC.GOLDEN, **out)
    print(PC.GOLDEN, os.path.getsize(PC.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
