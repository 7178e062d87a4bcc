"""lenv_dueling_se_inner_loop_segment, host side (no GPU): the binding, the header, and the refusals, which return before anything
touches a device."""
import ctypes as C
import os
import re

from learning_environments_amd import _lib, configs
from learning_environments_amd.config import ddqn_cfg_from_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lenv_dueling_se_inner_loop_segment"


def test_the_function_is_bound_and_declared_and_the_abi_is_still_version_7():
    assert NAME in _lib.EXPORTS
    L = _lib.lib()
    assert L.lenv_abi_version() == 7
    assert L.lenv_struct_size(len(_lib.ABI_STRUCTS)) == -1                    # a function only: no new ABI struct
    assert len(_lib.ABI_STRUCTS) == 17
    with open(os.path.join(ROOT, "include", "lenv_hip.h")) as f:
        header = f.read()
    m = re.search(r"#define LENV_DUELING_RESUME_WORDS (\d+)", header)
    assert m and int(m.group(1)) == _lib.DUELING_RESUME_WORDS == 32
    decl = re.sub(r"/\*.*?\*/", "", re.search(r"int %s\((.*?)\);" % NAME, header, re.S).group(1), flags=re.S)
    assert len(decl.split(",")) == len(_lib.SIGNATURES[NAME][1])              # the ctypes argument list follows the header's
    assert _lib.SIGNATURES[NAME][1][:-4] == _lib.SIGNATURES["lenv_dueling_se_inner_loop_icm"][1][:-1]


def _call(cfg, begin, end, resume, icm=None, agent_init=1, out_score=1, hp=None):
    """A launch of ZERO chains: every refusal below is checked in front of the `chains == 0` return, so it shows as LENV_ERR_INVALID, and a
    check that went missing would show as LENV_OK -- never as a kernel started on these (host) addresses."""
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    out = _lib.InnerOut(*[p.value if f == "score" and out_score else None if t is C.c_void_p else 0 for f, t in _lib.InnerOut._fields_])
    return _lib.lib().lenv_dueling_se_inner_loop_segment(C.byref(cfg), hp, icm, p, None, None, None, p if agent_init else None, p, None, 0, p,
                                                         C.c_size_t(0), C.byref(out), begin, end, p if resume else None, None)


def _cfg():
    cfgd = configs.fixed_work(configs.cartpole_syn_env_ddqn(num_workers=2), 7)
    cfg = ddqn_cfg_from_config(cfgd)
    assert cfg.train_episodes == 7
    return cfg


def test_refusals_happen_on_the_host():
    cfg = _cfg()
    assert _call(cfg, 0, 7, True) == 0 and _call(cfg, 3, 4, True) == 0        # LENV_OK: nothing to do for zero chains
    for begin, end in ((3, 3), (5, 2), (-1, 3), (0, 8), (7, 8), (7, 7)):
        assert _call(cfg, begin, end, True) == -1, (begin, end)               # LENV_ERR_INVALID
    assert _call(cfg, 0, 7, False) == -1                                      # resume == NULL
    # what lenv_dueling_se_inner_loop_icm refuses, the same way
    assert _call(cfg, 0, 7, True, agent_init=0) == -1
    assert _call(cfg, 0, 7, True, out_score=0) == -1
    assert _call(cfg, 0, 7, True, hp=C.byref(_lib.ChainHp(None, None, None, None))) == -1      # a lenv_chain_hp without its arrays
    icm_cfg = _lib.DdqnCfg.from_buffer_copy(cfg)
    icm_cfg.icm_enabled, icm_cfg.icm_feature_dim, icm_cfg.icm_hidden = 1, 8, 16
    assert _call(icm_cfg, 0, 7, True, icm=None) == -1                         # an ICM cfg without lenv_icm_io
    tape_cfg = _lib.DdqnCfg.from_buffer_copy(cfg)
    tape_cfg.rng_mode = _lib.RNG_TAPE
    assert _call(tape_cfg, 0, 7, True) == -1                                  # tape mode without tapes
