"""lenv_ppo_rn_inner_loop_segment, host side (no GPU): the binding, the header, and the refusals, which return before anything touches
a device.  (engine.PpoInnerLoop needs a device to be constructed: its argument checks are in tests/test_ppo_segments_gpu.py.)"""
import ctypes as C
import os
import re

from learning_environments_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lenv_ppo_rn_inner_loop_segment"
E = 7


def test_the_function_is_bound_and_declared_and_the_abi_is_still_version_7():
    assert NAME in _lib.EXPORTS
    L = _lib.lib()
    assert L.lenv_abi_version() == 7
    assert L.lenv_struct_size(len(_lib.ABI_STRUCTS)) == -1                    # a function only: no new ABI struct
    with open(os.path.join(ROOT, "include", "lenv_hip.h")) as f:
        header = f.read()
    m = re.search(r"#define LENV_PPO_RESUME_WORDS (\d+)", header)
    assert m and int(m.group(1)) == _lib.PPO_RESUME_WORDS == 32
    decl = re.sub(r"/\*.*?\*/", "", re.search(r"int %s\((.*?)\);" % NAME, header, re.S).group(1), flags=re.S)
    assert len(decl.split(",")) == len(_lib.SIGNATURES[NAME][1])              # the ctypes argument list follows the header's
    assert _lib.SIGNATURES[NAME][1][:-4] == _lib.SIGNATURES["lenv_ppo_rn_inner_loop"][1][:-1]
    assert _lib.SIGNATURES[NAME][1][-4:] == [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]


def _cfg(**over):
    kw = dict(env_id=_lib.ENV["Pendulum-v0"], state_dim=3, action_dim=1, max_steps=12, rn_hidden=16, rn_layers=1, rn_act=_lib.ACT["tanh"], rn_prelu=0.25,
              reward_env_type=2, info_dim=0, hidden=64, layers=2, act=_lib.ACT["relu"], prelu=0.25, train_episodes=E, test_episodes=2, init_episodes=0,
              early_out_num=3, ppo_epochs=3, same_action_num=1, rng_mode=_lib.RNG_COUNTER, solved_reward=1e9, gamma=0.99, lr=3e-3, action_std=0.5,
              vf_coef=1.0, ent_coef=0.01, eps_clip=0.2, update_episodes=2.5, adam_beta1=0.9, adam_beta2=0.999, adam_eps=1e-8)
    kw.update(over)
    return _lib.PpoCfg(**kw)


def _call(cfg, begin, end, resume=1, agent_init=1, out_score=1, segment=True):
    """A launch of ZERO chains: every refusal below is checked in front of the `chains == 0` return, so it shows as LENV_ERR_INVALID, and a
    check that went missing would show as LENV_OK -- never as a kernel started on these (host) addresses."""
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    out = _lib.PpoOut(*[p.value if f == "score" and out_score else None if t is C.c_void_p else 0 for f, t in _lib.PpoOut._fields_])
    head = (C.byref(cfg), p, None, None, None, p if agent_init else None, p, None, 0, p, C.c_size_t(0), C.byref(out))
    if not segment:
        return _lib.lib().lenv_ppo_rn_inner_loop(*head, None)
    return _lib.lib().lenv_ppo_rn_inner_loop_segment(*head, begin, end, p if resume else None, None)


def test_refusals_happen_on_the_host():
    cfg = _cfg()
    assert _call(cfg, 0, E, segment=False) == 0                               # the cfg is one the old entry takes
    for begin, end in ((0, E), (3, 4), (0, 1), (E - 1, E)):
        assert _call(cfg, begin, end) == 0, (begin, end)                      # LENV_OK: nothing to do for zero chains
    for begin, end in ((3, 3), (5, 2), (-1, 3), (0, E + 1), (E, E + 1), (E, E)):
        assert _call(cfg, begin, end) == -1, (begin, end)                     # LENV_ERR_INVALID
    assert _call(cfg, 0, E, resume=0) == -1                                   # resume == NULL
    # what lenv_ppo_rn_inner_loop refuses, the same way
    assert _call(cfg, 0, E, agent_init=0) == -1 == _call(cfg, 0, E, agent_init=0, segment=False)
    assert _call(cfg, 0, E, out_score=0) == -1 == _call(cfg, 0, E, out_score=0, segment=False)
    wide = _cfg(hidden=129)
    old = _call(wide, 0, E, segment=False)
    assert old != 0 and _call(wide, 0, E) == old                              # an unsupported cfg: the old entry's own code
    assert _call(_cfg(train_episodes=0), 0, 1) == -1                          # no training episode: no segment to run
