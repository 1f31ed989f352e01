#!/usr/bin/env python
"""Do two builds of the library compute the same loss and gradient in the cooperative training kernels, byte for byte?

    python scripts/compare_trainer_builds.py LIB_A LIB_B [--timeout SECONDS]

For every row of ROWS and each library in turn: one fresh child process (tests/helpers/trc_child.py: one loss_grad call, writes
loss, gradient and the training path) with SYNFERENCE_HIP_LIB set and the row's switches in its environment -- the library reads
them once per process -- under its own time limit.  A child that exits non-zero or runs out of time ends the script: nothing more
is started on the GPU after it.  The .npz arrays of the two libraries are compared as bytes, one line per row.

The rows are the smallest that reach every store mode of the weight-gradient finish and every instantiation family of
k_maf_trainc / k_nsf_trainc: B = 37 is one ragged workgroup, 2 085 many workgroups (store mode 0: plain stores into the
workgroup's partial), 16 384 + 37 a workgroup's second chunk (mode 1: add to the partial), SF_GRAD_ACC=fix mode 3 (fixed-point
atomics), SF_TRC_NG=2 the 8-wave form.  The f32-atomic mode 2 depends on the order of the adds and is not compared by bits
(tests/test_gpu_train_bench_shapes.py checks it against the oracle).  Exit status 0: every row identical.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "helpers", "trc_child.py")
SWITCHES = ("SF_TRC_NG", "SF_GRAD_ACC", "SF_DETERMINISTIC")
BIG = 16384 + 37
ROWS = [({}, name, B) for name in ("maf_cfg1", "maf_span6", "maf_cli", "maf_t8", "maf_d4") for B in (37, 2085)]
ROWS += [({"SF_TRC_NG": "2"}, "maf_cfg1", 2085), ({}, "maf_cfg1", BIG), ({"SF_GRAD_ACC": "fix"}, "maf_cfg1", 2085)]
ROWS += [({}, name, B) for name in ("nsf_cfg3", "nsf_k10", "nsf_h69") for B in (37, 2085)]
ROWS += [({"SF_GRAD_ACC": "fix"}, "nsf_cfg3", 2085), ({"SF_GRAD_ACC": "partial"}, "nsf_cfg3", BIG)]


def label(row):
    extra, name, B = row
    return "%s B=%d%s" % (name, B, "".join(" %s=%s" % kv for kv in sorted(extra.items())))


def run_rows(lib_path, tmp, tag, timeout):
    """One child per row; returns {label: {array name: array}}, or None after a failure (nothing else may start then)."""
    res = {}
    for n, row in enumerate(ROWS):
        extra, name, B = row
        out = os.path.join(tmp, "%s_%d.npz" % (tag, n))
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}   # (a row must not inherit a switch)
        env.update(extra, SYNFERENCE_HIP_LIB=os.path.abspath(lib_path))
        try:
            r = subprocess.run([sys.executable, CHILD, name, str(B), out], env=env, timeout=timeout)
        except subprocess.TimeoutExpired:
            print("STOP: %s, %s did not finish in %d s" % (lib_path, label(row), timeout))
            return None
        if r.returncode != 0:
            print("STOP: %s, %s exited with status %d" % (lib_path, label(row), r.returncode))
            return None
        with np.load(out) as d:
            res[label(row)] = {k: d[k] for k in d.files}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("libs", nargs=2, metavar="LIB")
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child process")
    a = ap.parse_args()
    for p in a.libs:
        if not os.path.isfile(p):
            ap.error("no such library: " + p)
    with tempfile.TemporaryDirectory() as tmp:
        ra = run_rows(a.libs[0], tmp, "a", a.timeout)
        rb = run_rows(a.libs[1], tmp, "b", a.timeout) if ra is not None else None
    if ra is None or rb is None:
        return 2
    n_diff = 0
    for k, va in ra.items():
        vb = rb[k]
        bad = [n for n in ("loss", "grad", "path") if va[n].shape != vb[n].shape or va[n].tobytes() != vb[n].tobytes()]
        n_diff += 1 if bad else 0
        print("%s  %s (path %d, loss %d bytes, grad %d bytes)%s" % ("DIFFERENT" if bad else "identical ", k, int(va["path"]),
                                                                   va["loss"].nbytes, va["grad"].nbytes,
                                                                   "  differ: " + ", ".join(bad) if bad else ""), flush=True)
    print("%d rows compared, %d differ" % (len(ra), n_diff))
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
