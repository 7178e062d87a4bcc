"""Compile-time guard on agent_test_population.hip, in the style of test_ppo_build.py: the file is part of the library build, holds no inline
assembly and no environment knobs, compiles to gfx950 with the Makefile's own flags (hipcc cross-compiles without a GPU), its static LDS plus
the largest dynamic carve-up the entry can ask for fits the 160 KiB of a CU, and the scratch frame is reported."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "learning_environments_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SRC = "agent_test_population"


def _makefile_flags(obj):
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS = (.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    for m in re.finditer(r"^(.*?): EXTRA \+= (.*)$", text, re.M):
        if obj in m.group(1).split():
            flags += m.group(2).split()
    return [f for f in flags if f not in ("-fPIC", "-Wall", "-Wno-unused-parameter")]


def _constant(src, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


def _largest_dynamic_lds(src):
    """The entry's dynamic LDS (the layout at the top of the source file): two activation buffers [rows][W] and, with the shared LayerNorm,
    [rows][H | 1], rows = min(T, AT_TB); the parameters are staged only where they fit below the limit the source states.  Largest over the
    admitted envelope: either the limit itself (a staged launch) or the widest unstaged shape."""
    tb = _constant(src, "AT_TB")
    limit = re.search(r"AT_LDS_LIMIT = (\d+) \* 1024 - (\d+);", src)
    limit = int(limit.group(1)) * 1024 - int(limit.group(2))
    widest = 0
    for H in (1, 511, 512):
        for F in (0, 128):
            W = max((H + 3) & ~3, 2 * ((F + 3) & ~3))
            widest = max(widest, 4 * (2 * tb * W + tb * (H | 1)))
    assert widest <= limit, (widest, limit)            # the widest admitted shape runs without staged parameters
    return limit


def test_source_is_part_of_the_library_build():
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert SRC + ".hip" in re.search(r"^SRCS = (.*)$", text, re.M).group(1).split()
    src = open(os.path.join(CSRC, SRC + ".hip")).read()
    assert "asm" not in re.sub(r"//.*", "", src), "no inline assembly beyond what the shared headers hold"
    assert "getenv" not in src, "no environment knobs"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.timeout(600)
def test_agent_test_kernel_resources(tmp_path):
    out = str(tmp_path / (SRC + ".s"))
    subprocess.check_call([HIPCC] + _makefile_flags("_build/%s.o" % SRC) + ["-I", os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                                                                             os.path.join(CSRC, SRC + ".hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_ZN[A-Za-z0-9_]*):", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
        if cur is not None:
            for key, pat in (("scratch", r"; ScratchSize: (\d+)"), ("lds", r"; LDSByteSize: (\d+)"), ("vgpr", r"; NumVgprs: (\d+)"), ("sgpr", r"; NumSgprs: (\d+)")):
                m2 = re.search(pat, line)
                if m2:
                    cur[key] = int(m2.group(1))
    mine = {n: k for n, k in kernels.items() if "28agent_test_population_kernel" in n}
    assert len(mine) == 2, sorted(kernels)                # parameters staged in LDS / read from global memory
    dyn = _largest_dynamic_lds(open(os.path.join(CSRC, SRC + ".hip")).read())
    for name, k in mine.items():
        print("%s: ScratchSize %s B/lane, static LDS %s B (+ at most %d B dynamic), %s VGPRs, %s SGPRs" % (name, k.get("scratch"), k.get("lds"), dyn, k.get("vgpr"), k.get("sgpr")))
        assert k.get("lds") is not None and k["lds"] + dyn <= 160 * 1024
        assert k.get("scratch") is not None
