"""No GPU: the registers of the fused fp32 16-row MAF kernels, read from the BUILT library (the gfx950 code objects' metadata).

The head rows as per-lane packed FMAs fit the 128 VGPRs of four workgroups per CU only because the off-chain FMAs are pinned in the
pass that computes them (sf_maf16_pass.h: the empty asm statements on SfPass16G::ham / pre); the flagship has one register to
spare and four instances none, so another compiler version may spill without any test of the results noticing.  Bar (DESIGN.md
§3, "head rows off the matrix pipe"), for every PREC 2 instance of k_maf_samp16 and k_maf_find16s, NB = 1, 2 x D = 3 .. 5 x K3 = 0 .. D - 1:
no scratch, no spilled register, at most 128 VGPRs and no AGPR (256-thread workgroups, four per CU: 16 waves per CU, 4 per SIMD,
512 / 4 registers)."""
import os
import re
import shutil
import subprocess

import pytest

from synference_amd import _lib

# k_maf_samp16<NB, SPAN, HM, DD, PREC = 2, K3> / k_maf_find16s<NB, DD, PREC = 2, K3>: groups (NB, DD, K3)
SAMP = re.compile(r"^_Z12k_maf_samp16ILi([12])ELb0ELb1ELi([345])ELi2ELi(\d)EE")
FIND = re.compile(r"^_Z13k_maf_find16sILi([12])ELi([345])ELi2ELi(\d)EE")
FIELDS = ("private_segment_fixed_size", "vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count")


def _tool(name):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    for p in (os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", name),
              os.path.join(os.path.dirname(os.path.realpath(hipcc)), name), shutil.which(name) or ""):
        if p and os.path.isfile(p):
            return p
    raise AssertionError(f"{name} of the ROCm toolchain that built the library was not found")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled name: {field: int}} of every kernel in the library's gfx950 code objects."""
    lib = _lib.load()._name
    tmp = tmp_path_factory.mktemp("codeobj")
    link = tmp / "lib.so"
    os.symlink(os.path.abspath(lib), link)   # llvm-objdump writes the bundles next to the path it is given
    subprocess.run([_tool("llvm-objdump"), "--offloading", str(link)], check=True, cwd=tmp, stdout=subprocess.DEVNULL)
    objs = sorted(p for p in tmp.iterdir() if p.name.endswith("gfx950"))
    assert objs, "no gfx950 code object in " + lib
    out = {}
    for o in objs:
        notes = subprocess.run([_tool("llvm-readelf"), "--notes", str(o)], check=True, stdout=subprocess.PIPE, text=True).stdout
        blocks = []
        for line in notes.splitlines():
            m = re.match(r"^  (- | {2})\.(\w+): +(\S+)", line)   # a kernel's own keys ("- " opens the list item); its arguments' lie deeper
            if not m:
                continue
            if m.group(1) == "- ":
                blocks.append({})
            if blocks:
                blocks[-1][m.group(2)] = m.group(3)
        for b in blocks:
            if "name" in b and "vgpr_count" in b:
                out[b["name"]] = {k: int(b[k]) for k in FIELDS if k in b}
    return out


def _instances(kernels, pat):
    return {pat.match(k).groups(): v for k, v in kernels.items() if pat.match(k)}


@pytest.mark.parametrize("pat", [SAMP, FIND], ids=["k_maf_samp16", "k_maf_find16s"])
def test_every_fused_fp32_instance_is_built_and_fits_four_workgroups_per_cu(kernels, pat):
    inst = _instances(kernels, pat)
    want = {(str(NB), str(D), str(K3)) for D in (3, 4, 5) for NB in (1, 2) for K3 in range(D)}
    assert set(inst) == want, sorted(want ^ set(inst))
    for key, r in sorted(inst.items()):
        print(pat.pattern[3:20], key, r)
        assert set(r) == set(FIELDS), (key, r)
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (key, r)
        assert r["vgpr_count"] <= 128 and r["agpr_count"] == 0, (key, r)
