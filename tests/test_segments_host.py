"""lenv_td3_rn_inner_loop_segment, lenv_dueling_se_inner_loop_segment and lenv_ppo_rn_inner_loop_segment, host side (no GPU): the binding,
the header, and the refusals, which return before anything touches a device.  (engine.PpoInnerLoop needs a device to be constructed: its
argument checks are in tests/test_ppo_segments_gpu.py.)"""
import ctypes as C
import os
import re

import pytest

from learning_environments_amd import _lib, configs
from learning_environments_amd.config import ddqn_cfg_from_config, td3_cfg_from_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = 7


def _ppo_cfg(**over):
    kw = dict(env_id=_lib.ENV["Pendulum-v0"], state_dim=3, action_dim=1, max_steps=12, rn_hidden=16, rn_layers=1, rn_act=_lib.ACT["tanh"], rn_prelu=0.25,
              reward_env_type=2, info_dim=0, hidden=64, layers=2, act=_lib.ACT["relu"], prelu=0.25, train_episodes=E, test_episodes=2, init_episodes=0,
              early_out_num=3, ppo_epochs=3, same_action_num=1, rng_mode=_lib.RNG_COUNTER, solved_reward=1e9, gamma=0.99, lr=3e-3, action_std=0.5,
              vf_coef=1.0, ent_coef=0.01, eps_clip=0.2, update_episodes=2.5, adam_beta1=0.9, adam_beta2=0.999, adam_eps=1e-8)
    kw.update(over)
    return _lib.PpoCfg(**kw)


# per family: the segment entry and the entry it continues, the name of its record width, its output struct, whether hp / icm stand behind the
# cfg, and a cfg of seven training episodes
FAMILIES = {
    "td3": dict(name="lenv_td3_rn_inner_loop_segment", old="lenv_td3_rn_inner_loop_icm", words="TD3_RESUME_WORDS", Out=_lib.Td3Out, prefix=True,
                cfg=lambda: td3_cfg_from_config(configs.fixed_work(configs.cmc_reward_env_td3(16), E))),
    "dueling": dict(name="lenv_dueling_se_inner_loop_segment", old="lenv_dueling_se_inner_loop_icm", words="DUELING_RESUME_WORDS", Out=_lib.InnerOut,
                    prefix=True, cfg=lambda: ddqn_cfg_from_config(configs.fixed_work(configs.cartpole_syn_env_ddqn(num_workers=2), E))),
    "ppo": dict(name="lenv_ppo_rn_inner_loop_segment", old="lenv_ppo_rn_inner_loop", words="PPO_RESUME_WORDS", Out=_lib.PpoOut, prefix=False,
                cfg=_ppo_cfg),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_function_is_bound_and_declared_and_the_abi_is_still_version_7(family):
    f = FAMILIES[family]
    name = f["name"]
    assert name in _lib.EXPORTS
    L = _lib.lib()
    assert L.lenv_abi_version() == 7
    assert L.lenv_struct_size(len(_lib.ABI_STRUCTS)) == -1                    # a function only: no new ABI struct
    if family == "dueling":
        assert len(_lib.ABI_STRUCTS) == 17
    with open(os.path.join(ROOT, "include", "lenv_hip.h")) as fh:
        header = fh.read()
    m = re.search(r"#define LENV_%s (\d+)" % f["words"], header)
    assert m and int(m.group(1)) == getattr(_lib, f["words"]) == 32
    decl = re.sub(r"/\*.*?\*/", "", re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1), flags=re.S)
    assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1])              # the ctypes argument list follows the header's
    assert _lib.SIGNATURES[name][1][:-4] == _lib.SIGNATURES[f["old"]][1][:-1]
    if family == "ppo":
        assert _lib.SIGNATURES[name][1][-4:] == [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]


def _call(family, cfg, begin, end, resume=True, icm=None, agent_init=1, out_score=1, hp=None, segment=True):
    """A launch of ZERO chains: every refusal below is checked in front of the `chains == 0` return, so it shows as LENV_ERR_INVALID, and a
    check that went missing would show as LENV_OK -- never as a kernel started on these (host) addresses."""
    f = FAMILIES[family]
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    out = f["Out"](*[p.value if n == "score" and out_score else None if t is C.c_void_p else 0 for n, t in f["Out"]._fields_])
    head = (C.byref(cfg),) + ((hp, icm) if f["prefix"] else ()) + (p, None, None, None, p if agent_init else None, p, None, 0, p, C.c_size_t(0),
                                                                   C.byref(out))
    if not segment:
        return getattr(_lib.lib(), f["old"])(*head, None)
    return getattr(_lib.lib(), f["name"])(*head, begin, end, p if resume else None, None)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_refusals_happen_on_the_host(family):
    cfg = FAMILIES[family]["cfg"]()
    assert cfg.train_episodes == E
    call = lambda *a, **kw: _call(family, *a, **kw)
    assert call(cfg, 0, E, segment=False) == 0                                # the cfg is one the old entry takes
    for begin, end in ((0, E), (3, 4), (0, 1), (E - 1, E)):
        assert call(cfg, begin, end) == 0, (begin, end)                       # LENV_OK: nothing to do for zero chains
    for begin, end in ((3, 3), (5, 2), (-1, 3), (0, E + 1), (E, E + 1), (E, E)):
        assert call(cfg, begin, end) == -1, (begin, end)                      # LENV_ERR_INVALID
    assert call(cfg, 0, E, resume=False) == -1                                # resume == NULL
    # what the old entry refuses, the same way
    assert call(cfg, 0, E, agent_init=0) == -1 == call(cfg, 0, E, agent_init=0, segment=False)
    assert call(cfg, 0, E, out_score=0) == -1 == call(cfg, 0, E, out_score=0, segment=False)
    if family == "ppo":
        wide = _ppo_cfg(hidden=129)
        old = call(wide, 0, E, segment=False)
        assert old != 0 and call(wide, 0, E) == old                           # an unsupported cfg: the old entry's own code
        assert call(_ppo_cfg(train_episodes=0), 0, 1) == -1                   # no training episode: no segment to run
        return
    if family == "dueling":
        assert call(cfg, 0, E, hp=C.byref(_lib.ChainHp(None, None, None, None))) == -1      # a lenv_chain_hp without its arrays
        tape_cfg = _lib.DdqnCfg.from_buffer_copy(cfg)
        tape_cfg.rng_mode = _lib.RNG_TAPE
        assert call(tape_cfg, 0, E) == -1                                     # tape mode without tapes
    icm_cfg = type(cfg).from_buffer_copy(cfg)
    icm_cfg.icm_enabled, icm_cfg.icm_feature_dim, icm_cfg.icm_hidden = 1, 8, 16
    assert call(icm_cfg, 0, E, icm=None) == -1                                # an ICM cfg without lenv_icm_io
