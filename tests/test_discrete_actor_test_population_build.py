"""Compile-time guard on discrete_actor_test_population.hip and ql_test_population.hip, in the style of test_actor_test_population_build.py:
the files are part of the library build, hold no environment knobs and no inline assembly, compile to gfx950 with the Makefile's own flags
(hipcc cross-compiles without a GPU), the static LDS plus the largest dynamic carve-up the entry can ask for fits the 160 KiB of a CU, a staged
launch leaves room for a second workgroup on the CU, and VGPRs, scratch and LDS of every instantiation are printed.  The kernel is compiled
under __launch_bounds__(512, 4): the staging rule wants two workgroups of 8 waves on a CU, i.e. at most 128 VGPRs (unbounded the
instantiations take 135..142), at the price of a small scratch frame, which is bounded here too."""
import os
import re

import pytest

from population_build_common import HIPCC, SHARED_HEADER, episodes_per_workgroup, kernels, lds_limit, source

SRC = "discrete_actor_test_population"
QL_SRC = "ql_test_population"


def _largest_dynamic_lds():
    """The entry's dynamic LDS (the layout at the top of the source file): two activation buffers [rows][W] and, with the shared LayerNorm,
    [rows][H | 1], rows = min(T, TP_TB); the actor is staged only where all of it fits below the limit the source states.  Largest over the
    admitted envelope: the limit itself (a staged launch) or the widest unstaged shape."""
    tb, limit = episodes_per_workgroup(SRC), lds_limit(SRC, "DA")
    widest = max(4 * (2 * tb * ((H + 3) & ~3) + tb * (H | 1)) for H in (1, 511, 512))
    return limit, max(limit, widest)


def test_sources_are_part_of_the_library_build():
    text = source("Makefile")
    srcs = re.search(r"^SRCS = (.*)$", text, re.M).group(1).split()
    deps = re.search(r"^_build/%\.o: (.*)$", text, re.M).group(1).split()
    for s in (SRC, QL_SRC):
        assert s + ".hip" in srcs
        src = source(s + ".hip")
        assert "getenv" not in src, "no environment knobs"
        assert "asm" not in src.replace("same", ""), "no inline assembly"
    for header in ("lenv_td3d_actor.cuh", "lenv_ql_policy.cuh", SHARED_HEADER):
        assert header in deps, header
    # the shared pieces live in the headers alone: the fused kernels include them and define none of them
    fused = source("td3_discrete_inner_loop.hip")
    assert '#include "lenv_td3d_actor.cuh"' in fused
    for name in ("float det_gumbel(", "float td3d_temperature(", "int argmax_first(", "void gumbel_softmax_row(", "void dmlp_off(", "STREAM_TD3D_GUMBEL_TEST ="):
        assert name not in fused and name in source("lenv_td3d_actor.cuh"), name
        assert name not in source(SRC + ".hip"), name
    ql = source("ql_rn_inner_loop.hip")
    assert '#include "lenv_ql_policy.cuh"' in ql and "int ql_argmax_f32(" not in ql
    assert "int ql_argmax_f32(" in source("lenv_ql_policy.cuh")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.timeout(600)
def test_discrete_actor_test_kernel_resources(tmp_path):
    found = kernels(tmp_path, SRC)
    mine = {n: k for n, k in found.items() if "37discrete_actor_test_population_kernel" in n}
    assert len(mine) == 6, sorted(found)                # three envs x (actor staged in LDS / read from global memory)
    src = source(SRC + ".hip")
    staged_dyn, dyn = _largest_dynamic_lds()
    assert "__launch_bounds__(DNT, 4)" in src
    for name, k in sorted(mine.items()):
        print("%s: ScratchSize %s B/lane, static LDS %s B (+ at most %d B dynamic, %d B with a staged actor), %s VGPRs, %s SGPRs"
              % (name, k.get("scratch"), k.get("lds"), dyn, staged_dyn, k.get("vgpr"), k.get("sgpr")))
        assert k.get("lds") is not None and k["lds"] + dyn <= 160 * 1024
        assert k["lds"] + staged_dyn <= 80 * 1024, "a staged launch leaves room for a second workgroup on the CU"
        assert k.get("scratch") is not None and k["scratch"] <= 64, "the frame the bound costs stays a few registers per lane"
        assert k.get("vgpr") is not None and k["vgpr"] <= 128, "__launch_bounds__(512, 4): two workgroups of 8 waves per CU"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.timeout(600)
def test_ql_test_kernel_resources(tmp_path):
    found = kernels(tmp_path, QL_SRC)
    mine = {n: k for n, k in found.items() if "25ql_test_population_kernel" in n}
    assert len(mine) == 1, sorted(found)
    for name, k in mine.items():
        print("%s: ScratchSize %s B/lane, static LDS %s B, %s VGPRs, %s SGPRs" % (name, k.get("scratch"), k.get("lds"), k.get("vgpr"), k.get("sgpr")))
        assert k.get("lds") == 0 and k.get("scratch") == 0
        assert k.get("vgpr") is not None and k["vgpr"] <= 128
