"""Compile-time guard on the 256-wide DDQN wave-chain kernel (ddqn_wavechain_wide.hip), in the style of test_kernel_resources.py: the file is
compiled to gfx950 assembly with the Makefile's own flags (hipcc cross-compiles without a GPU).  Its kernel must be there, its out-of-line
phase routines must keep LLVM's no-callee-saved-registers treatment (no save / restore blocks through scratch memory), and the kernel's frame
must stay small."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "learning_environments_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SRC = "ddqn_wavechain_wide"
ROUTINES = ("ww_forward", "ww_backward", "ww_update", "ww_update_small", "ww_thin", "ww_test_steps")


def _makefile_flags(obj):
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS = (.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    for m in re.finditer(r"^(.*?): EXTRA \+= (.*)$", text, re.M):
        if obj in m.group(1).split():
            flags += m.group(2).split()
    return [f for f in flags if f not in ("-fPIC", "-Wall", "-Wno-unused-parameter")]


def test_source_is_part_of_the_library_build():
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert SRC + ".hip" in re.search(r"^SRCS = (.*)$", text, re.M).group(1).split()
    assert "-fno-optimize-sibling-calls" in _makefile_flags("_build/%s.o" % SRC)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.timeout(900)
def test_wide_wavechain_routines_keep_no_callee_saved_registers(tmp_path):
    out = str(tmp_path / (SRC + ".s"))
    subprocess.check_call([HIPCC] + _makefile_flags("_build/%s.o" % SRC) + ["-I", os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                                                                             os.path.join(CSRC, SRC + ".hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    funcs, cur = {}, None
    for line in open(out):
        m = re.match(r"^(_ZN[A-Za-z0-9_]*):", line)
        if m:
            cur = funcs.setdefault(m.group(1), {"st": 0, "ld": 0, "scratch": None})
        if cur is not None:
            cur["st"] += "scratch_store" in line
            cur["ld"] += "scratch_load" in line
            m2 = re.search(r"; ScratchSize: (\d+)", line)
            if m2:
                cur["scratch"] = int(m2.group(1))
    kernels = [n for n in funcs if "26ddqn_wavechain_wide_kernel" in n]
    assert len(kernels) == 1, sorted(funcs)
    k = funcs[kernels[0]]
    assert k["scratch"] is not None and k["scratch"] <= 300, "%s: ScratchSize %s B/lane" % (kernels[0], k["scratch"])
    for r in ROUTINES:
        names = [n for n in funcs if re.search(r"L?%d%sE" % (len(r), r), n)]
        assert len(names) == 1, (r, sorted(funcs))
        f = funcs[names[0]]
        assert f["st"] <= 8 and f["ld"] <= 8, "%s: %d scratch stores / %d loads (callee-saved registers are being saved again?)" % (names[0], f["st"], f["ld"])
