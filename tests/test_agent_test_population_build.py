"""Compile-time guard on agent_test_population.hip, in the style of test_ppo_build.py: the file is part of the library build, holds no inline
assembly and no environment knobs, compiles to gfx950 with the Makefile's own flags (hipcc cross-compiles without a GPU), its static LDS plus
the largest dynamic carve-up the entry can ask for fits the 160 KiB of a CU, and the scratch frame is reported."""
import os
import re

import pytest

from population_build_common import HIPCC, SHARED_HEADER, episodes_per_workgroup, kernels, lds_limit, source

SRC = "agent_test_population"


def _largest_dynamic_lds():
    """The entry's dynamic LDS (the layout at the top of the source file): two activation buffers [rows][W] and, with the shared LayerNorm,
    [rows][H | 1], rows = min(T, TP_TB); the parameters are staged only where they fit below the limit the source states.  Largest over the
    admitted envelope: either the limit itself (a staged launch) or the widest unstaged shape."""
    tb, limit = episodes_per_workgroup(SRC), lds_limit(SRC, "AT")
    widest = 0
    for H in (1, 511, 512):
        for F in (0, 128):
            W = max((H + 3) & ~3, 2 * ((F + 3) & ~3))
            widest = max(widest, 4 * (2 * tb * W + tb * (H | 1)))
    assert widest <= limit, (widest, limit)            # the widest admitted shape runs without staged parameters
    return limit


def test_source_is_part_of_the_library_build():
    text = source("Makefile")
    assert SRC + ".hip" in re.search(r"^SRCS = (.*)$", text, re.M).group(1).split()
    assert SHARED_HEADER in re.search(r"^_build/%\.o: (.*)$", text, re.M).group(1).split()
    src = source(SRC + ".hip")
    assert "asm" not in re.sub(r"//.*", "", src), "no inline assembly beyond what the shared headers hold"
    assert "getenv" not in src, "no environment knobs"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.timeout(600)
def test_agent_test_kernel_resources(tmp_path):
    found = kernels(tmp_path, SRC)
    mine = {n: k for n, k in found.items() if "28agent_test_population_kernel" in n}
    assert len(mine) == 2, sorted(found)                # parameters staged in LDS / read from global memory
    dyn = _largest_dynamic_lds()
    for name, k in mine.items():
        print("%s: ScratchSize %s B/lane, static LDS %s B (+ at most %d B dynamic), %s VGPRs, %s SGPRs" % (name, k.get("scratch"), k.get("lds"), dyn, k.get("vgpr"), k.get("sgpr")))
        assert k.get("lds") is not None and k["lds"] + dyn <= 160 * 1024
        assert k.get("scratch") is not None
