"""lenv_td3d_inner_loop_segment and lenv_td3d_rn_inner_loop_segment, host side (no GPU): the binding, the header, and the refusals, which
return before anything touches a device -- the checks of tests/test_segments_host.py for the TD3_discrete_vary pair."""
import ctypes as C
import os
import re

import pytest

from learning_environments_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = 7

# the segment entry, the entry it continues, whether a lenv_td3d_rn_cfg stands in front of hp
ENTRIES = {"se": ("lenv_td3d_inner_loop_segment", "lenv_td3d_inner_loop", False),
           "rn": ("lenv_td3d_rn_inner_loop_segment", "lenv_td3d_rn_inner_loop", True)}


def _cfg(**over):
    kw = dict(env_id=_lib.ENV["CartPole-v0"], state_dim=4, action_dim=2, max_steps=12, se_hidden=16, se_layers=1, se_act=_lib.ACT["leakyrelu"],
              se_prelu=0.25, hidden=40, layers=3, act=_lib.ACT["tanh"], prelu=0.25, use_layer_norm=0, gumbel_hard=1, batch_size=20, rb_size=40,
              train_episodes=E, test_episodes=2, init_episodes=2, early_out_num=50, policy_delay=2, rng_mode=_lib.RNG_COUNTER, solved_reward=1e9,
              gamma=0.99, lr=1e-3, tau=0.01, action_std=0.1, policy_std=0.2, policy_std_clip=0.5, max_action=1.0, gumbel_temp=1.0,
              adam_beta1=0.9, adam_beta2=0.999, adam_eps=1e-8, step_budget=0, se_layer_norm=0, test_mode=0, early_out_virtual_diff=0.01)
    kw.update(over)
    return _lib.Td3dCfg(**kw)


def _rn(**over):
    kw = dict(synthetic_env_type=1, reward_env_type=2, rn_hidden=16, rn_layers=1, rn_act=_lib.ACT["tanh"], rn_prelu=0.25, rn_layer_norm=0)
    kw.update(over)
    return _lib.Td3dRnCfg(**kw)


@pytest.mark.parametrize("which", sorted(ENTRIES))
def test_the_functions_are_bound_and_declared_and_the_abi_is_still_version_7(which):
    name, old, _ = ENTRIES[which]
    assert name in _lib.EXPORTS
    L = _lib.lib()
    assert L.lenv_abi_version() == 7
    assert len(_lib.ABI_STRUCTS) == 17 and L.lenv_struct_size(17) == -1          # functions only: no new ABI struct
    with open(os.path.join(ROOT, "include", "lenv_hip.h")) as fh:
        header = fh.read()
    m = re.search(r"#define LENV_TD3D_RESUME_WORDS (\d+)", header)
    assert m and int(m.group(1)) == _lib.TD3D_RESUME_WORDS == 32
    decl = re.sub(r"/\*.*?\*/", "", re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1), flags=re.S)
    assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1])                 # the ctypes argument list follows the header's
    assert _lib.SIGNATURES[name][1][:-4] == _lib.SIGNATURES[old][1][:-1]         # the continued entry's arguments in front of ...
    assert _lib.SIGNATURES[name][1][-4:] == [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]      # episode_begin, episode_end, resume, stream
    assert "`%s`" % name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _call(which, cfg, begin, end, rn=None, resume=True, agent_init=1, out_score=1, hp=None, segment=True, chains=0):
    """A launch of ZERO chains: every refusal below is checked in front of the `chains == 0` return, so it shows as its error code, and a
    check that went missing would show as LENV_OK -- never as a kernel started on these (host) addresses."""
    name, old, has_rn = ENTRIES[which]
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    out = _lib.Td3Out(*[p.value if n == "score" and out_score else None if t is C.c_void_p else 0 for n, t in _lib.Td3Out._fields_])
    head = (C.byref(cfg),) + ((C.byref(rn if rn is not None else _rn()),) if has_rn else ()) + (
        hp, p, None, None, None, p if agent_init else None, p, None, chains, p, C.c_size_t(0), C.byref(out))
    if not segment:
        return getattr(_lib.lib(), old)(*head, None)
    return getattr(_lib.lib(), name)(*head, begin, end, p if resume else None, None)


@pytest.mark.parametrize("which", sorted(ENTRIES))
def test_refusals_happen_on_the_host(which):
    cfg = _cfg()
    call = lambda *a, **kw: _call(which, *a, **kw)
    assert call(cfg, 0, E, segment=False) == 0                                # the cfg is one the old entry takes
    for begin, end in ((0, E), (3, 4), (0, 1), (E - 1, E)):
        assert call(cfg, begin, end) == 0, (begin, end)                       # LENV_OK: nothing to do for zero chains
    for begin, end in ((3, 3), (5, 2), (-1, 3), (0, E + 1), (E, E + 1), (E, E)):
        assert call(cfg, begin, end) == -1, (begin, end)                      # LENV_ERR_INVALID
    assert call(cfg, 0, E, resume=False) == -1                                # resume == NULL
    # what the old entry refuses, the same way
    assert call(cfg, 0, E, agent_init=0) == -1 == call(cfg, 0, E, agent_init=0, segment=False)
    assert call(cfg, 0, E, out_score=0) == -1 == call(cfg, 0, E, out_score=0, segment=False)
    assert call(cfg, 0, E, hp=C.byref(_lib.ChainHp(None, None, None, None))) == -1      # a lenv_chain_hp without its arrays
    tape_cfg = _cfg(rng_mode=_lib.RNG_TAPE)
    assert call(tape_cfg, 0, E) == -1 == call(tape_cfg, 0, E, segment=False)  # tape mode without tapes


def _old_code(which, cfg, rn=None):
    """The code with which the continued entry refuses an unsupported cfg.  It looks at the cfg once there is a chain to run, so the call asks
    for one chain -- after the parameter count (host only) has confirmed that the cfg is refused and no kernel can start."""
    L = _lib.lib()
    if which == "se":
        probe = L.lenv_td3d_num_params(C.byref(cfg), None, None)
    else:
        probe = L.lenv_td3d_rn_num_params(C.byref(cfg), C.byref(rn if rn is not None else _rn()))
    assert probe < 0
    old = _call(which, cfg, 0, E, rn=rn, segment=False, chains=1)
    assert old == probe
    return old


@pytest.mark.parametrize("which", sorted(ENTRIES))
def test_a_cfg_the_old_entry_refuses_is_refused_with_its_code(which):
    prelu = _cfg(act=_lib.ACT["prelu"])                                       # the agent nets' trained PReLU slope
    assert _call(which, prelu, 0, E) == _old_code(which, prelu) == -2
    wide = _cfg(hidden=513)
    assert _call(which, wide, 0, E) == _old_code(which, wide) == -2
    if which == "rn":
        for bad in (_rn(reward_env_type=3), _rn(synthetic_env_type=0), _rn(rn_layers=4)):
            assert _call(which, cfg=_cfg(), begin=0, end=E, rn=bad) == _old_code(which, _cfg(), rn=bad) == -2
        name = ENTRIES[which][0]
        assert getattr(_lib.lib(), name)(C.byref(_cfg()), None, *([None] * 8), 0, None, 0, None, 0, E, None, None) == -1       # rn == NULL


def test_same_action_num_2_is_refused_in_front_of_both_entry_pairs():
    """lenv_td3d_cfg has no same_action_num: the config reader refuses it (NotImplementedError) for the VirtualEnv and the RewardEnv launch alike,
    so neither the single launch nor a segment is ever built for it."""
    from learning_environments_amd.config import td3d_cfg_from_config
    from learning_environments_amd.configs import cartpole_syn_env_td3_discrete
    for syn in (0, 1):
        cfgd = cartpole_syn_env_td3_discrete(num_workers=2, max_iterations=1)
        cfgd["agents"]["gtn"]["synthetic_env_type"] = syn
        td3d_cfg_from_config(cfgd)
        cfgd["agents"]["td3_discrete_vary"]["same_action_num"] = 2
        with pytest.raises(NotImplementedError):
            td3d_cfg_from_config(cfgd)


def test_the_engine_class_states_both_entry_pairs():
    from learning_environments_amd import engine
    assert issubclass(engine.Td3DiscreteInnerLoop, engine._SegmentedInnerLoop)
    assert engine.Td3DiscreteInnerLoop.resume_words == 32
