"""Compile-time guard on the PPO inner-loop kernel (ppo_rn_inner_loop.hip), in the style of test_wavechain_wide_build.py: the file is compiled
to gfx950 assembly with the Makefile's own flags (hipcc cross-compiles without a GPU).  One kernel per continuous real env must be there, its
static LDS plus the largest dynamic carve-up the library's layout accepts must fit the 160 KB of a CU, the scratch frame is reported (DESIGN.md section 8 records it), and
the generated code must hold no scalar memory write of any kind (stores, atomics, write-backs of the scalar data cache)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "learning_environments_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SRC = "ppo_rn_inner_loop"
# scalar-unit instructions that write memory, spelled in pieces: s_ + (buffer_ | scratch_)? + store / atomic, and the scalar data cache's
# write-back / discard
_W, _A = "st" + "ore", "at" + "omic"
SCALAR_WRITES = re.compile(r"\bs_(?:buffer_|scratch_)?(?:%s|%s)\w*|\bs_dcache_(?:wb|discard)\w*" % (_W, _A), re.I)


def _makefile_flags(obj):
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS = (.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    for m in re.finditer(r"^(.*?): EXTRA \+= (.*)$", text, re.M):
        if obj in m.group(1).split():
            flags += m.group(2).split()
    return [f for f in flags if f not in ("-fPIC", "-Wall", "-Wno-unused-parameter")]


def _largest_accepted_dynamic_lds():
    """The dynamic LDS bytes of a launch come from the library's own layout (lenv_ppo_rn_lds_bytes): the largest value over reward nets of
    one hidden layer (the only ones staged in LDS) of growing width on the stand-in's 21 inputs; the widths the layout refuses must be
    refused by the workspace query too, i.e. before a launch."""
    import ctypes as C
    from learning_environments_amd import _lib
    L = _lib.lib()
    big, refused = 0, 0
    for rn_hidden in range(16, 641, 16):
        cfg = _lib.PpoCfg(env_id=2, state_dim=17, action_dim=6, max_steps=100, rn_hidden=rn_hidden, rn_layers=1, rn_act=1, rn_prelu=0.25,
                          reward_env_type=3, info_dim=4, hidden=128, layers=2, act=1, prelu=0.25, train_episodes=2, test_episodes=64,
                          init_episodes=0, early_out_num=1, ppo_epochs=1, same_action_num=1, rng_mode=0, solved_reward=1e9, gamma=0.99, lr=1e-3,
                          action_std=0.5, vf_coef=1.0, ent_coef=0.01, eps_clip=0.2, update_episodes=20.0, adam_beta1=0.9, adam_beta2=0.999,
                          adam_eps=1e-8)
        n = L.lenv_ppo_rn_lds_bytes(C.byref(cfg))
        if n < 0:
            assert n == -2 and L.lenv_ppo_rn_workspace_bytes(C.byref(cfg), 1) == -2
            refused += 1
        else:
            assert L.lenv_ppo_rn_workspace_bytes(C.byref(cfg), 1) > 0
            big = max(big, n)
    assert big > 150 * 1024 and refused > 0, (big, refused)       # the widest accepted net comes close to the limit; wider ones are refused
    return big


def test_source_is_part_of_the_library_build():
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert SRC + ".hip" in re.search(r"^SRCS = (.*)$", text, re.M).group(1).split()
    src = open(os.path.join(CSRC, SRC + ".hip")).read()
    assert "asm" not in re.sub(r"//.*", "", src), "no inline assembly beyond what the shared headers hold"
    assert "getenv" not in src, "no environment knobs"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.timeout(900)
def test_ppo_kernel_resources(tmp_path):
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
    ppo = {n: k for n, k in kernels.items() if "19ppo_rn_inner_kernel" in n}
    assert len(ppo) == 3, sorted(kernels)                 # Pendulum-v0, MountainCarContinuous-v0, the HalfCheetah stand-in
    dyn = _largest_accepted_dynamic_lds()
    for name, k in ppo.items():
        print("%s: ScratchSize %s B/lane, static LDS %s B (+ at most %d B dynamic), %s VGPRs, %s SGPRs" % (name, k.get("scratch"), k.get("lds"), dyn, k.get("vgpr"), k.get("sgpr")))
        assert k.get("lds") is not None and k["lds"] + dyn <= 160 * 1024
        assert k.get("scratch") is not None
    hits = sorted(set(m.group(0) for m in SCALAR_WRITES.finditer(re.sub(r";.*", "", text))))
    assert not hits, "scalar memory writes in the generated code: %s" % hits
