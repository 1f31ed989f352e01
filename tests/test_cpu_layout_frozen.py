"""No GPU: the layout builder's output is frozen.  synference_amd/csrc/layout_dump_main.cpp, built with the host compiler against
the tree's sf_layout.cpp, prints one digest per shape over every descriptor byte and every table of sf_build_layout /
sf_build_mlp_layout (and the error strings of invalid descs); the output must equal tests/golden/layout_digests.txt line for line.
The golden file is recorded by scripts/make_layout_golden.py -- rerun it after an INTENDED change of the layout.  The summary line
counts the placements and images the matrix reaches; a count of zero means the matrix no longer covers that path."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "synference_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "layout_digests.txt")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path_factory.mktemp("layout_dump") / "layout_dump")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I" + CSRC, os.path.join(CSRC, "layout_dump_main.cpp"),
                    os.path.join(CSRC, "sf_layout.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def lines(dump):
    return subprocess.run([dump], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()


def test_every_table_and_descriptor_equals_the_recorded_digest(dump, lines):
    with open(GOLDEN) as fh:
        want = fh.read().splitlines()
    for i, (got, exp) in enumerate(zip(lines, want)):
        if got == exp:
            continue
        key, moved = exp.split(" ", 1)[0], ""
        if got.split(" ", 1)[0] == key and not key.startswith(("mlp", "summary")):
            # the last field holds one hex digit per table, in the order of --tables
            tables = subprocess.run([dump, "--tables", key], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()[1:]
            sig_got, sig_exp = got.split()[-1], exp.split()[-1]
            assert len(tables) == len(sig_got) == len(sig_exp), (tables, sig_got, sig_exp)
            moved = "\n".join(f"{t}   {'MOVED (recorded ' + e + '...)' if g != e else ''}" for t, g, e in zip(tables, sig_got, sig_exp))
        pytest.fail(f"line {i + 1} differs from {GOLDEN}\n  recorded: {exp}\n  built:    {got}\ntables of the built layout:\n{moved}")
    assert len(lines) == len(want), (len(lines), len(want))


def test_the_matrix_reaches_every_placement_and_image(lines):
    assert lines[-1].startswith("summary ")
    counts = dict(f.split("=") for f in lines[-1].split()[1:])
    print(counts)
    assert len(counts) >= 35, counts
    for name, n in counts.items():
        assert int(n) >= 1, (name, counts)
