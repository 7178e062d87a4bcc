"""Compile-time guard on the PPO + ICM kernel (ppo_icm_segment_kernel in ppo_rn_inner_loop.hip), with tests/test_ppo_build.py's recipe: the file
is compiled to gfx950 assembly with the Makefile's own flags (hipcc cross-compiles without a GPU).  The kernel must be there once per continuous
real env, its static LDS plus the largest dynamic carve-up the library's layout accepts must fit the 160 KiB of a CU, and its scratch frame is
reported.  The module adds no dynamic LDS: the carve-up is the ICM-less kernels'.  (What the generated code of the shared body may not contain
is tests/test_ppo_build.py's to check: it reads the same assembly file.)"""
import os
import re
import subprocess

import pytest

from test_ppo_build import CSRC, HIPCC, ROOT, SRC, _largest_accepted_dynamic_lds, _makefile_flags

KERNEL = "ppo_icm_segment_kernel"


def test_kernel_name_and_source_rules():
    assert "ppo_rn_inner_kernel" not in KERNEL              # tests/test_ppo_build.py counts the kernels that carry that name
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert SRC + ".hip" in re.search(r"^SRCS = (.*)$", text, re.M).group(1).split()
    for name in (SRC + ".hip", "ppo_rn_inner_kernel.inc", "lenv_icm.cuh"):
        src = open(os.path.join(CSRC, name)).read()
        assert "asm" not in re.sub(r"//.*", "", src), name
        assert "getenv" not in src, name
    assert KERNEL in open(os.path.join(CSRC, SRC + ".hip")).read()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.timeout(900)
def test_ppo_icm_kernel_resources(tmp_path):
    out = str(tmp_path / (SRC + ".s"))
    subprocess.check_call([HIPCC] + _makefile_flags("_build/%s.o" % SRC) + ["-I", os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                                                                             os.path.join(CSRC, SRC + ".hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    kernels, cur = {}, None
    for line in open(out).read().splitlines():
        m = re.match(r"^(_ZN[A-Za-z0-9_]*):", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
        if cur is not None:
            for key, pat in (("scratch", r"; ScratchSize: (\d+)"), ("lds", r"; LDSByteSize: (\d+)"), ("vgpr", r"; NumVgprs: (\d+)"), ("sgpr", r"; NumSgprs: (\d+)")):
                m2 = re.search(pat, line)
                if m2:
                    cur[key] = int(m2.group(1))
    icm = {n: k for n, k in kernels.items() if "%d%s" % (len(KERNEL), KERNEL) in n}
    assert len(icm) == 3, sorted(kernels)                  # Pendulum-v0, MountainCarContinuous-v0, the HalfCheetah stand-in
    assert len([n for n in kernels if "19ppo_rn_inner_kernel" in n]) == 3 and len([n for n in kernels if "21ppo_rn_segment_kernel" in n]) == 3
    dyn = _largest_accepted_dynamic_lds()
    for name, k in sorted(icm.items()):
        print("%s: ScratchSize %s B/lane, static LDS %s B (+ at most %d B dynamic), %s VGPRs, %s SGPRs" % (name, k.get("scratch"), k.get("lds"), dyn, k.get("vgpr"), k.get("sgpr")))
        assert k.get("lds") is not None and k["lds"] + dyn <= 160 * 1024
        assert k.get("scratch") is not None
