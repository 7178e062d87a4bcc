"""The chunk-aligned forward deal of the early-gradient DDQN instantiation (`lenv_ddqn_se_forward_deal`, host only) and a compile-time
guard on the register and scratch budget of `ddqn_se_inner_loop.hip`.

The deal decides which thread of the 768-thread workgroup runs which (pass, sample) forward item of the published CartPole shape
(B = 199, gradient chunks of 17) and which waves' "forward done" tags the gradient of a chunk waits for: a wrong mask is a data race
on the GPU, so the masks are recomputed here from the lanes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "learning_environments_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NT, B, CHUNK, N_CHUNKS, FULL_LANES, SPILL = 768, 199, 17, 12, 512, 85


def _deal(cfg):
    from learning_environments_amd import _lib
    item = (C.c_int32 * NT)(*([-7] * NT))
    mask = (C.c_int32 * 16)(*([-7] * 16))
    rc = _lib.lib().lenv_ddqn_se_forward_deal(C.byref(cfg), item, mask)
    return rc, np.array(item[:]), np.array(mask[:])


def _published_cfg():
    from learning_environments_amd import configs
    from learning_environments_amd.config import ddqn_cfg_from_config
    cfg = ddqn_cfg_from_config(configs.cartpole_syn_env_ddqn(4))
    assert (cfg.batch_size, cfg.grad_chunk, cfg.q_hidden) == (B, CHUNK, 57)
    return cfg


def test_deal_is_a_bijection_with_pass2_spill_slots_and_exact_wave_masks():
    rc, item, mask = _deal(_published_cfg())
    assert rc == N_CHUNKS
    # 597 (pass, sample) items on 512 full-item lanes + 85 spill slots, nothing behind them
    assert (item[:FULL_LANES + SPILL] >= 0).all() and (item[FULL_LANES + SPILL:] == -1).all()
    assert sorted(item[:FULL_LANES + SPILL].tolist()) == list(range(3 * B))
    # every spill slot holds a pass-2 item
    assert (item[FULL_LANES:FULL_LANES + SPILL] // B == 2).all()
    # chunk_wave_mask[c] names exactly the waves that hold an item of chunk c
    want = [0] * N_CHUNKS
    for t in range(FULL_LANES + SPILL):
        want[(int(item[t]) % B) // CHUNK] |= 1 << (t // 64)
    assert mask[:N_CHUNKS].tolist() == want and (mask[N_CHUNKS:] == -7).all()
    # the two groups of four full-item waves: whichever of them finishes last, at least five chunks do not depend on it
    for late in (0x0f, 0xf0):
        assert sum(1 for m in want if m & late == 0) >= 5, (hex(late), [hex(m) for m in want])
    # a chunk's three passes of a sample all sit on the chunk's waves (the TD error reads all three)
    for c, m in enumerate(want):
        assert 0 < bin(m).count("1") <= 5, (c, hex(m))


def test_other_cfgs_report_no_early_gradient():
    from learning_environments_amd import _lib, configs
    from learning_environments_amd.config import ddqn_cfg_from_config
    base = _published_cfg()
    cases = {}
    cfgd = configs.cartpole_syn_env_ddqn(4)                 # SHAPE 2: default_config_cartpole.yaml
    cfgd["envs"]["CartPole-v0"].update(hidden_size=128)
    cfgd["agents"]["ddqn"].update(hidden_size=64, batch_size=32, activation_fn="relu", test_episodes=1)
    cases["shape 2"] = ddqn_cfg_from_config(cfgd)
    for name, field, value in (("test_mode 1", "test_mode", 1), ("NO_EARLY_GRAD", "kernel_variant", _lib.VARIANT_NO_EARLY_GRAD),
                               ("GENERIC", "kernel_variant", _lib.VARIANT_GENERIC), ("tape rng", "rng_mode", 1), ("batch 198", "batch_size", 198)):
        c = _lib.DdqnCfg.from_buffer_copy(base)
        setattr(c, field, value)
        cases[name] = c
    for name, c in cases.items():
        rc, item, mask = _deal(c)
        assert rc == 0 and (item == -7).all() and (mask == -7).all(), name
    L = _lib.lib()
    assert L.lenv_ddqn_se_forward_deal(None, (C.c_int32 * NT)(), (C.c_int32 * 16)()) == -1
    assert L.lenv_ddqn_se_forward_deal(C.byref(base), None, (C.c_int32 * 16)()) == -1
    # the split the deal builds on is the pinned one
    items, parts = C.c_int32(), C.c_int32()
    assert L.lenv_ddqn_se_forward_split(C.byref(base), C.byref(items), C.byref(parts)) == 0 and (items.value, parts.value) == (SPILL, 3)


# ---- compile guard (the helpers' pattern of tests/test_kernel_resources.py) ----
def _makefile_flags(obj):
    """FLAGS of the Makefile + the target-specific EXTRA of `obj` (so the test compiles what the product compiles)."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS = (.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    for m in re.finditer(r"^(.*?): EXTRA \+= (.*)$", text, re.M):
        if obj in m.group(1).split():
            flags += m.group(2).split()
    return [f for f in flags if f not in ("-fPIC", "-Wall", "-Wno-unused-parameter")]


def _resources_by_instantiation(src, tmp_path):
    """{template arguments (ENV, S, A, QACT, PPT, SHAPE, TEAM, TWIDE, RENV, EGRAD): {"vgpr": n, "scratch": bytes}} of ddqn_se_inner_kernel."""
    out = str(tmp_path / (src + ".s"))
    subprocess.check_call([HIPCC] + _makefile_flags("_build/%s.o" % src) + ["-I", os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                                                                             os.path.join(CSRC, src + ".hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    funcs, cur = {}, None
    for line in open(out):
        m = re.match(r"^_ZN4lenv20ddqn_se_inner_kernelI([A-Za-z0-9_]*?)EEvNS_9InnerArgsE:", line)
        if m:
            args = tuple(int(x) for x in re.findall(r"L[ib](\d+)E", m.group(1) + "E"))
            cur = funcs.setdefault(args, {"vgpr": None, "scratch": None})
        if cur is not None:
            for key, field in (("NumVgprs", "vgpr"), ("ScratchSize", "scratch")):
                m2 = re.search(r"; %s: (\d+)" % key, line)
                if m2 and cur[field] is None:
                    cur[field] = int(m2.group(1))
    return funcs


# ScratchSize (bytes per lane) of every instantiation of the parent commit c505a79 ("Give the four test-population entries one shared
# skeleton"), read once from its source with the Makefile's flags; key = (ENV, S, A, QACT, PPT, SHAPE, TEAM, TWIDE, RENV)
PARENT_SCRATCH = {
    (0,4,2,3,1,1,1,0,0): 20, (0,4,2,1,1,0,1,0,0): 36, (0,4,2,2,1,0,1,0,0): 36, (0,4,2,3,1,0,1,0,0): 36, (0,4,2,0,1,0,1,0,0): 36,
    (0,4,2,1,2,0,1,0,0): 44, (0,4,2,2,2,0,1,0,0): 44, (0,4,2,3,2,0,1,0,0): 64, (0,4,2,0,2,0,1,0,0): 44, (1,6,3,1,1,0,1,0,0): 92,
    (1,6,3,2,1,0,1,0,0): 92, (1,6,3,3,1,0,1,0,0): 148, (1,6,3,0,1,0,1,0,0): 100, (1,6,3,1,2,0,1,0,0): 116, (1,6,3,2,2,0,1,0,0): 116,
    (1,6,3,3,2,0,1,0,0): 164, (1,6,3,0,2,0,1,0,0): 124, (0,4,2,3,1,1,1,1,0): 40, (0,4,2,1,1,0,1,1,0): 24, (0,4,2,2,1,0,1,1,0): 24,
    (0,4,2,3,1,0,1,1,0): 24, (0,4,2,0,1,0,1,1,0): 24, (0,4,2,1,2,0,1,1,0): 60, (0,4,2,2,2,0,1,1,0): 60, (0,4,2,3,2,0,1,1,0): 60,
    (0,4,2,0,2,0,1,1,0): 60, (1,6,3,1,1,0,1,1,0): 140, (1,6,3,2,1,0,1,1,0): 140, (1,6,3,3,1,0,1,1,0): 140, (1,6,3,0,1,0,1,1,0): 140,
    (1,6,3,1,2,0,1,1,0): 176, (1,6,3,2,2,0,1,1,0): 176, (1,6,3,3,2,0,1,1,0): 176, (1,6,3,0,2,0,1,1,0): 180, (0,4,2,1,1,0,0,0,1): 36,
    (0,4,2,2,1,0,0,0,1): 36, (0,4,2,3,1,0,0,0,1): 76, (0,4,2,0,1,0,0,0,1): 36, (0,4,2,1,2,0,0,0,1): 72, (0,4,2,2,2,0,0,0,1): 72,
    (0,4,2,3,2,0,0,0,1): 96, (0,4,2,0,2,0,0,0,1): 64, (1,6,3,1,1,0,0,0,1): 104, (1,6,3,2,1,0,0,0,1): 104, (1,6,3,3,1,0,0,0,1): 156,
    (1,6,3,0,1,0,0,0,1): 104, (1,6,3,1,2,0,0,0,1): 140, (1,6,3,2,2,0,0,0,1): 140, (1,6,3,3,2,0,0,0,1): 184, (1,6,3,0,2,0,0,0,1): 140,
    (0,4,2,1,1,0,0,0,0): 12, (0,4,2,2,1,0,0,0,0): 20, (0,4,2,3,1,0,0,0,0): 24, (0,4,2,0,1,0,0,0,0): 12, (0,4,2,1,2,0,0,0,0): 48,
    (0,4,2,2,2,0,0,0,0): 36, (0,4,2,3,2,0,0,0,0): 52, (0,4,2,0,2,0,0,0,0): 48, (1,6,3,1,1,0,0,0,0): 96, (1,6,3,2,1,0,0,0,0): 96,
    (1,6,3,3,1,0,0,0,0): 136, (1,6,3,0,1,0,0,0,0): 96, (1,6,3,1,2,0,0,0,0): 116, (1,6,3,2,2,0,0,0,0): 116, (1,6,3,3,2,0,0,0,0): 164,
    (1,6,3,0,2,0,0,0,0): 124, (0,4,2,3,1,1,0,0,0): 8, (0,4,2,1,1,2,0,0,0): 0, (1,6,3,2,2,3,0,0,0): 84,
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.timeout(900)
def test_ddqn_kernel_register_and_scratch_budget(tmp_path):
    """Both instantiations of the published CartPole shape on one workgroup per chain (with and without the early gradient) stay at
    <= 168 VGPRs -- the cap of a 12-wave workgroup -- and <= 8 B of scratch per lane; no other instantiation's scratch
    grows beyond the parent commit's."""
    assert "-fno-slp-vectorize" in _makefile_flags("_build/ddqn_se_inner_loop.o")
    funcs = _resources_by_instantiation("ddqn_se_inner_loop", tmp_path)
    shape1 = [funcs.get((0, 4, 2, 3, 1, 1, 0, 0, 0, eg)) for eg in (0, 1)]
    assert all(f is not None for f in shape1), "the two SHAPE 1 instantiations were not found (name mangling changed?): %r" % sorted(funcs)
    for eg, f in enumerate(shape1):
        assert f["vgpr"] is not None and f["vgpr"] <= 168, (eg, f)
        assert f["scratch"] is not None and f["scratch"] <= 8, (eg, f)
    seen = 0
    for args, f in funcs.items():
        if args[:9] == (0, 4, 2, 3, 1, 1, 0, 0, 0):
            continue
        assert args[9] == 0 and args[:9] in PARENT_SCRATCH, "an instantiation the parent commit does not have: %r" % (args,)
        assert f["scratch"] is not None and f["scratch"] <= PARENT_SCRATCH[args[:9]], (args, f, PARENT_SCRATCH[args[:9]])
        seen += 1
    assert seen == len(PARENT_SCRATCH) - 1, (seen, len(PARENT_SCRATCH))
