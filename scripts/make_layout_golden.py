"""Record tests/golden/layout_digests.txt: the output of synference_amd/csrc/layout_dump_main.cpp (one digest per flow / MLP shape
over every table and descriptor that sf_build_layout / sf_build_mlp_layout produce), compiled against the sf_layout.cpp and
sf_layout.h of the commit to record.  After an intended layout change, record the working tree:

    python scripts/make_layout_golden.py synference_amd/csrc tests/golden/layout_digests.txt

To repeat the provenance of a golden file from another commit, extract that commit's layout source first:

    mkdir /tmp/parent && git show <commit>:synference_amd/csrc/sf_layout.cpp > /tmp/parent/sf_layout.cpp \
        && git show <commit>:synference_amd/csrc/sf_layout.h > /tmp/parent/sf_layout.h
    python scripts/make_layout_golden.py /tmp/parent tests/golden/layout_digests.txt

(include/synference_hip.h is taken from this checkout either way: the dump program fills today's sf_flow_desc.)
"""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "synference_amd", "csrc")


def build_dump(layout_dir, out_dir):
    """Compile the dump program against layout_dir's sf_layout.{cpp,h}; returns the binary's path."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        raise RuntimeError("no host C++ compiler found")
    # staged like the tree, so that every quoted include resolves to the recorded commit's header and not to this checkout's
    src = os.path.join(out_dir, "synference_amd", "csrc")
    os.makedirs(src)
    os.makedirs(os.path.join(out_dir, "include"))
    shutil.copy(os.path.join(CSRC, "layout_dump_main.cpp"), src)
    shutil.copy(os.path.join(layout_dir, "sf_layout.cpp"), src)
    shutil.copy(os.path.join(layout_dir, "sf_layout.h"), src)
    shutil.copy(os.path.join(ROOT, "include", "synference_hip.h"), os.path.join(out_dir, "include"))
    exe = os.path.join(out_dir, "layout_dump")
    subprocess.run([cxx, "-O2", "-std=c++17", os.path.join(src, "layout_dump_main.cpp"), os.path.join(src, "sf_layout.cpp"),
                    "-o", exe], check=True)
    return exe


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        text = subprocess.run([build_dump(sys.argv[1], tmp)], check=True, stdout=subprocess.PIPE, text=True).stdout
    with open(sys.argv[2], "w") as fh:
        fh.write(text)
    print(len(text.splitlines()) - 1, "cases;", text.splitlines()[-1])
