"""Compile-time guard on actor_test_population.hip, in the style of test_ppo_build.py: the file is part of the library build, holds no
environment knobs, compiles to gfx950 with the Makefile's own flags (hipcc cross-compiles without a GPU), its static LDS plus the largest
dynamic carve-up the entry can ask for fits the 160 KiB of a CU, and VGPRs, scratch and LDS of every instantiation are printed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "learning_environments_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SRC = "actor_test_population"


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
    """The entry's dynamic LDS (the layout at the top of the source file): two activation buffers [rows][W] and, with a TD3 actor's shared
    LayerNorm, [rows][H | 1], rows = min(T, AC_TB); the actor is staged only where all of it fits below the limit the source states, half a
    CU's LDS less the static arrays.  Largest over the admitted envelope: the limit itself (a staged launch) or the widest unstaged shape."""
    tb = _constant(src, "AC_TB")
    limit = re.search(r"AC_LDS_LIMIT = (\d+) \* 1024 - (\d+);", src)
    limit = int(limit.group(1)) * 1024 - int(limit.group(2))
    widest = max(4 * (2 * tb * ((H + 3) & ~3) + tb * (H | 1)) for H in (1, 511, 512))
    return limit, max(limit, widest)


def test_source_is_part_of_the_library_build():
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert SRC + ".hip" in re.search(r"^SRCS = (.*)$", text, re.M).group(1).split()
    src = open(os.path.join(CSRC, SRC + ".hip")).read()
    assert "getenv" not in src, "no environment knobs"
    for header in ("lenv_actor_params.cuh", "lenv_at_layer.cuh"):
        assert header in re.search(r"^_build/%\.o: (.*)$", text, re.M).group(1).split(), header


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.timeout(600)
def test_actor_test_kernel_resources(tmp_path):
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
    mine = {n: k for n, k in kernels.items() if "28actor_test_population_kernel" in n}
    assert len(mine) == 6, sorted(kernels)                # three envs x (actor staged in LDS / read from global memory)
    staged_dyn, dyn = _largest_dynamic_lds(open(os.path.join(CSRC, SRC + ".hip")).read())
    for name, k in sorted(mine.items()):
        print("%s: ScratchSize %s B/lane, static LDS %s B (+ at most %d B dynamic, %d B with a staged actor), %s VGPRs, %s SGPRs"
              % (name, k.get("scratch"), k.get("lds"), dyn, staged_dyn, k.get("vgpr"), k.get("sgpr")))
        assert k.get("lds") is not None and k["lds"] + dyn <= 160 * 1024
        assert k["lds"] + staged_dyn <= 80 * 1024, "a staged launch leaves room for a second workgroup on the CU"
        assert k.get("scratch") is not None
        assert k.get("vgpr") is not None and k["vgpr"] <= 128, "__launch_bounds__(512, 4): two workgroups of 8 waves per CU"
