"""What the compile-time guards of the test-population entries share (test_agent_test_population_build.py, test_actor_test_population_build.py,
test_discrete_actor_test_population_build.py): the Makefile's own flags, the resource figures of every kernel of a source file compiled to
gfx950 device assembly, and the constants the kernels share through lenv_at_layer.cuh."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "learning_environments_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SHARED_HEADER = "lenv_at_layer.cuh"
LAYOUT_HEADER = "lenv_tp_layout.h"      # TP_TB and the dynamic-LDS layout, read by the kernels and by the host's launch plan


def source(name):
    return open(os.path.join(CSRC, name)).read()


def makefile_flags(obj):
    text = source("Makefile")
    flags = re.search(r"^FLAGS = (.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    for m in re.finditer(r"^(.*?): EXTRA \+= (.*)$", text, re.M):
        if obj in m.group(1).split():
            flags += m.group(2).split()
    return [f for f in flags if f not in ("-fPIC", "-Wall", "-Wno-unused-parameter")]


def kernels(tmp_path, src):
    """{mangled name: dict(scratch, lds, vgpr, sgpr)} of every kernel of csrc/<src>.hip"""
    out = str(tmp_path / (src + ".s"))
    subprocess.check_call([HIPCC] + makefile_flags("_build/%s.o" % src) + ["-I", os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                                                                            os.path.join(CSRC, src + ".hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    found, cur = {}, None
    for line in open(out).read().splitlines():
        m = re.match(r"^(_ZN[A-Za-z0-9_]*):", line)
        if m:
            cur = found.setdefault(m.group(1), {})
        if cur is not None:
            for key, pat in (("scratch", r"; ScratchSize: (\d+)"), ("lds", r"; LDSByteSize: (\d+)"), ("vgpr", r"; NumVgprs: (\d+)"), ("sgpr", r"; NumSgprs: (\d+)")):
                m2 = re.search(pat, line)
                if m2:
                    cur[key] = int(m2.group(1))
    return found


def episodes_per_workgroup(src_name):
    """TP_TB, defined once in the layout header (a dependency of every object) and in no kernel file"""
    assert not re.search(r"constexpr int \w*_TB =", source(src_name + ".hip")), "the episodes of a workgroup are TP_TB of " + LAYOUT_HEADER
    assert LAYOUT_HEADER in re.search(r"^_build/%\.o: (.*)$", source("Makefile"), re.M).group(1).split()
    return int(re.search(r"constexpr int TP_TB = (\d+);", source(LAYOUT_HEADER)).group(1))


def lds_limit(src_name, prefix):
    """<prefix>_LDS_LIMIT of csrc/<src_name>.hip in bytes"""
    m = re.search(r"%s_LDS_LIMIT = (\d+) \* 1024 - (\d+);" % prefix, source(src_name + ".hip"))
    return int(m.group(1)) * 1024 - int(m.group(2))
