"""Compile-time guard on actor_test_population.hip, in the style of test_ppo_build.py: the file is part of the library build, holds no
environment knobs, compiles to gfx950 with the Makefile's own flags (hipcc cross-compiles without a GPU), its static LDS plus the largest
dynamic carve-up the entry can ask for fits the 160 KiB of a CU, and VGPRs, scratch and LDS of every instantiation are printed."""
import os
import re

import pytest

from population_build_common import HIPCC, SHARED_HEADER, episodes_per_workgroup, kernels, lds_limit, source

SRC = "actor_test_population"


def _largest_dynamic_lds():
    """The entry's dynamic LDS (the layout at the top of the source file): two activation buffers [rows][W] and, with a TD3 actor's shared
    LayerNorm, [rows][H | 1], rows = min(T, TP_TB); the actor is staged only where all of it fits below the limit the source states, half a
    CU's LDS less the static arrays.  Largest over the admitted envelope: the limit itself (a staged launch) or the widest unstaged shape."""
    tb, limit = episodes_per_workgroup(SRC), lds_limit(SRC, "AC")
    widest = max(4 * (2 * tb * ((H + 3) & ~3) + tb * (H | 1)) for H in (1, 511, 512))
    return limit, max(limit, widest)


def test_source_is_part_of_the_library_build():
    text = source("Makefile")
    assert SRC + ".hip" in re.search(r"^SRCS = (.*)$", text, re.M).group(1).split()
    src = source(SRC + ".hip")
    assert "getenv" not in src, "no environment knobs"
    for header in ("lenv_actor_params.cuh", SHARED_HEADER):
        assert header in re.search(r"^_build/%\.o: (.*)$", text, re.M).group(1).split(), header


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.timeout(600)
def test_actor_test_kernel_resources(tmp_path):
    found = kernels(tmp_path, SRC)
    mine = {n: k for n, k in found.items() if "28actor_test_population_kernel" in n}
    assert len(mine) == 6, sorted(found)                # three envs x (actor staged in LDS / read from global memory)
    staged_dyn, dyn = _largest_dynamic_lds()
    for name, k in sorted(mine.items()):
        print("%s: ScratchSize %s B/lane, static LDS %s B (+ at most %d B dynamic, %d B with a staged actor), %s VGPRs, %s SGPRs"
              % (name, k.get("scratch"), k.get("lds"), dyn, staged_dyn, k.get("vgpr"), k.get("sgpr")))
        assert k.get("lds") is not None and k["lds"] + dyn <= 160 * 1024
        assert k["lds"] + staged_dyn <= 80 * 1024, "a staged launch leaves room for a second workgroup on the CU"
        assert k.get("scratch") is not None
        assert k.get("vgpr") is not None and k["vgpr"] <= 128, "__launch_bounds__(512, 4): two workgroups of 8 waves per CU"
