"""Compile-time guard on se_fit.hip, in the style of test_agent_test_population_build.py: the file is part of the library build, holds no inline
assembly and no environment knobs, compiles to gfx950 with the Makefile's own flags (hipcc cross-compiles without a GPU), its static LDS plus
the largest dynamic carve-up the entry can ask for fits the 160 KiB of a CU, and the scratch frame is reported."""
import os
import re

import pytest

from population_build_common import HIPCC, kernels, lds_limit, source

SRC = "se_fit"


def _largest_dynamic_lds():
    """sf_layout of the source file: idx [batch] | xT [in][ld] | eT [out][ld] | act [layers][hidden][ld], every piece rounded to 4 floats,
    ld = min(batch, SF_RC) | 1; the parameters, moments and gradient follow only where all of it stays below the limit the source states.
    Largest over the admitted envelope: either the limit itself (a resident launch) or the widest shape without them."""
    limit = lds_limit(SRC, "SF")
    rc = int(re.search(r"constexpr int SF_RC = (\d+);", source(SRC + ".hip")).group(1))
    r4 = lambda n: (n + 3) & ~3
    widest = 0
    for batch in (1, rc, 256):
        ld = min(batch, rc) | 1
        widest = max(widest, 4 * (r4(batch) + r4(32 * ld) + r4(32 * ld) + r4(2 * 128 * ld)))
    assert widest <= limit, (widest, limit)              # the widest admitted shape runs with its gradient in the workspace
    return limit


def test_source_is_part_of_the_library_build():
    text = source("Makefile")
    assert SRC + ".hip" in re.search(r"^SRCS = (.*)$", text, re.M).group(1).split()
    deps = re.search(r"^_build/%\.o: (.*)$", text, re.M).group(1).split()
    assert "lenv_gemm.cuh" in deps and "lenv_device.cuh" in deps
    src = source(SRC + ".hip")
    assert "asm" not in re.sub(r"//.*", "", src), "no inline assembly beyond what the shared headers hold"
    assert "getenv" not in src, "no environment knobs"
    assert "adam_elem" in src and "STREAM_SE_FIT_BATCH" in src


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.timeout(600)
def test_se_fit_kernel_resources(tmp_path):
    found = kernels(tmp_path, SRC)
    mine = {n: k for n, k in found.items() if "13se_fit_kernel" in n}
    assert len(mine) == 2, sorted(found)                 # parameters resident in LDS / parameters in the caller's arrays, gradient in the workspace
    dyn = _largest_dynamic_lds()
    for name, k in mine.items():
        print("%s: ScratchSize %s B/lane, static LDS %s B (+ at most %d B dynamic), %s VGPRs, %s SGPRs" % (name, k.get("scratch"), k.get("lds"), dyn, k.get("vgpr"), k.get("sgpr")))
        assert k.get("lds") is not None and k["lds"] + dyn <= 160 * 1024
        assert k.get("scratch") is not None
