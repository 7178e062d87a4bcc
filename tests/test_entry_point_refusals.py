"""CPU suite: what the fused inner loops' entry points refuse, and what their layout queries answer -- both before any device call, so no GPU
is needed.  Each case changes ONE thing of a launch that would otherwise go through and names the code the library answers; no call here gets
as far as a launch.  The expected codes and byte counts are literals, taken from the library before its host-side launch path was folded into
csrc/lenv_host.h: the pin that the fold changed no refusal and moved no buffer."""
import ctypes as C

import pytest

from learning_environments_amd import _lib, config, configs
from learning_environments_amd.agents import vary
from learning_environments_amd.envs.gridworld import transition_tables

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
_BUF = (C.c_char * 64)()
P = C.addressof(_BUF)                    # a non-null host pointer: these calls never get as far as reading through it
BIG = 1 << 40
ACT_PRELU = _lib.ACT["prelu"]


def _copy(cfg, **over):
    c = type(cfg).from_buffer_copy(cfg)
    for k, v in over.items():
        setattr(c, k, v)
    return c


def _small(cfgd, episodes=3):
    return configs.fixed_work(cfgd, episodes)


def _ddqn_cfg(**over):
    return config.ddqn_cfg_from_config(_small(configs.cartpole_syn_env_ddqn(2)), **over)


def _dueling_cfg(**over):
    return config.ddqn_cfg_from_config(_small(configs.acrobot_syn_env_duelingddqn(2)), **dict(dict(q_hidden=16, feature_dim=16, batch_size=8), **over))


def _td3_cfg(**over):
    return config.td3_cfg_from_config(_small(configs.pendulum_reward_env_td3(2)), **dict(dict(hidden=16, batch_size=8, rn_hidden=16), **over))


def _td3d_cfg(**over):
    return config.td3d_cfg_from_config(_small(configs.cartpole_syn_env_td3_discrete(2)), **dict(dict(hidden=16, batch_size=8), **over))


def _td3d_rn():
    cfgd = configs.cartpole_syn_env_td3_discrete(2)
    cfgd["agents"]["gtn"]["synthetic_env_type"] = 1
    cfgd["envs"]["CartPole-v0"].update(reward_env_type=2)
    return config.td3d_rn_cfg_from_config(cfgd)


def _ppo_cfg(**over):
    return config.ppo_cfg_from_config(_small(configs.pendulum_reward_env_ppo(2)), **over)


def _ql_rn_cfg(**over):
    return config.ql_cfg_from_config(_small(configs.cliff_reward_env_ql(2)), transition_tables("Cliff"), **over)


def _ql_se_cfg(**over):
    return config.ql_se_cfg_from_config(_small(configs.cliff_syn_env_ql(2)), transition_tables("Cliff"), **over)


class Call:
    """One entry point: its parameter names in order and a launch that would go through.  run(**changes) calls it with some arguments replaced;
    `cfg`, `rn`, `hp`, `icm`, `tapes` and `out` take a ctypes struct (passed by reference) or None."""
    STRUCTS = ("cfg", "rn", "hp", "icm", "tapes", "out")

    def __init__(self, name, params, **good):
        self.name, self.params, self.good = name, params.split(), good

    def run(self, **changes):
        unknown = set(changes) - set(self.params)
        assert not unknown, (self.name, unknown)
        args = dict(self.good, **changes)
        keep = [args[p] for p in self.params]          # the structs stay referenced for the duration of the call
        return getattr(_lib.lib(), self.name)(*[C.byref(v) if p in self.STRUCTS and v is not None else v for p, v in zip(self.params, keep)])


POP = "theta eps worker sign agent_init rng_keys tapes chains workspace workspace_bytes out"
SEG = " episode_begin episode_end resume stream"


def _good(cfg, out_cls, **more):
    return dict(dict(cfg=cfg, hp=None, icm=None, theta=P, eps=None, worker=None, sign=None, agent_init=P, rng_keys=P, tapes=None, chains=2, workspace=P,
                     workspace_bytes=BIG, out=out_cls(score=P), stream=None, episode_begin=0, episode_end=1, resume=P), **more)


def _calls():
    dd, du, t3, td, pp = _ddqn_cfg(), _dueling_cfg(), _td3_cfg(), _td3d_cfg(), _ppo_cfg()
    ql = dict(cfg=None, alpha=None, gamma=None, theta=P, eps=None, worker=None, sign=None, shaped_override=None, next_state=P, reward=P, done=P, rng_keys=P,
              tapes=None, chains=2, out=_lib.QlOut(score=P), stream=None, trace_se=None, workspace=P, workspace_bytes=BIG)
    init = dict(hp=None, rng_keys=P, chains=2, agent_init=P, stream=None)
    calls = [
        Call("lenv_ddqn_se_inner_loop", "cfg " + POP + " stream", **_good(dd, _lib.InnerOut)),
        Call("lenv_dueling_se_inner_loop", "cfg " + POP + " stream", **_good(du, _lib.InnerOut)),
        Call("lenv_dueling_se_inner_loop_hp", "cfg hp " + POP + " stream", **_good(du, _lib.InnerOut)),
        Call("lenv_dueling_se_inner_loop_icm", "cfg hp icm " + POP + " stream", **_good(du, _lib.InnerOut)),
        Call("lenv_dueling_se_inner_loop_segment", "cfg hp icm " + POP + SEG, **_good(du, _lib.InnerOut)),
        Call("lenv_td3_rn_inner_loop", "cfg " + POP + " stream", **_good(t3, _lib.Td3Out)),
        Call("lenv_td3_rn_inner_loop_hp", "cfg hp " + POP + " stream", **_good(t3, _lib.Td3Out)),
        Call("lenv_td3_rn_inner_loop_icm", "cfg hp icm " + POP + " stream", **_good(t3, _lib.Td3Out)),
        Call("lenv_td3_rn_inner_loop_segment", "cfg hp icm " + POP + SEG, **_good(t3, _lib.Td3Out)),
        Call("lenv_td3d_inner_loop", "cfg hp " + POP + " stream", **_good(td, _lib.Td3Out)),
        Call("lenv_td3d_rn_inner_loop", "cfg rn hp " + POP + " stream", **_good(td, _lib.Td3Out, rn=_td3d_rn())),
        Call("lenv_ppo_rn_inner_loop", "cfg " + POP + " stream", **_good(pp, _lib.PpoOut)),
        Call("lenv_ppo_rn_inner_loop_segment", "cfg " + POP + SEG, **_good(pp, _lib.PpoOut)),
        Call("lenv_ql_rn_inner_loop", "cfg theta eps worker sign shaped_override next_state reward done rng_keys tapes chains out stream",
             **dict(ql, cfg=_ql_rn_cfg())),
        Call("lenv_ql_rn_inner_loop_hp", "cfg alpha gamma theta eps worker sign shaped_override next_state reward done rng_keys tapes chains out stream",
             **dict(ql, cfg=_ql_rn_cfg())),
        Call("lenv_ql_se_inner_loop", "cfg theta eps worker sign next_state reward done rng_keys tapes chains out trace_se workspace workspace_bytes stream",
             **dict(ql, cfg=_ql_se_cfg())),
        Call("lenv_dueling_agent_init_hp", "cfg hp rng_keys chains agent_init stream", **dict(init, cfg=du)),
        Call("lenv_td3_agent_init_hp", "cfg hp rng_keys chains agent_init stream", **dict(init, cfg=t3)),
        Call("lenv_td3d_agent_init", "cfg hp rng_keys chains agent_init stream", **dict(init, cfg=td)),
    ]
    return {c.name: c for c in calls}


CALLS = _calls()
FUSED = [n for n in CALLS if "agent_init" not in n and "_ql_" not in n]          # the launches with agent_init / workspace / out->score
HP = [n for n in FUSED if " hp " in " " + " ".join(CALLS[n].params) + " "]
ICM = [n for n in FUSED if "icm" in CALLS[n].params]
SEGMENT = [n for n in CALLS if n.endswith("_segment")]
TABULAR = [n for n in CALLS if "_ql_" in n]
AGENT_INIT = [n for n in CALLS if "agent_init" in n]
TAPES = {_lib.DdqnCfg: _lib.Tapes, _lib.Td3Cfg: _lib.Td3Tapes, _lib.Td3dCfg: _lib.Td3dTapes, _lib.PpoCfg: _lib.PpoTapes, _lib.QlCfg: _lib.Tapes}
# a cfg the family's layout refuses with LENV_ERR_UNSUPPORTED
BAD_CFG = {_lib.DdqnCfg: dict(q_act=ACT_PRELU), _lib.Td3Cfg: dict(act=ACT_PRELU), _lib.Td3dCfg: dict(act=ACT_PRELU), _lib.PpoCfg: dict(act=ACT_PRELU),
           _lib.QlCfg: dict(rn_layers=5)}


def _bad_cfg(call):
    cfg = call.good["cfg"]
    return _copy(cfg, **BAD_CFG[type(cfg)])


@pytest.mark.parametrize("name", sorted(CALLS))
def test_null_cfg_and_negative_chains(name):
    assert CALLS[name].run(cfg=None) == INVALID
    assert CALLS[name].run(chains=-1) == INVALID


@pytest.mark.parametrize("name", FUSED)
def test_null_buffers_of_the_fused_launches(name):
    call = CALLS[name]
    assert call.run(agent_init=None) == INVALID
    assert call.run(out=None) == INVALID
    assert call.run(out=type(call.good["out"])()) == INVALID              # out->score null
    assert call.run(workspace=None) == INVALID


@pytest.mark.parametrize("name", FUSED)
def test_theta_rule_of_each_family(name):
    """DDQN, DuelingDDQN and TD3_discrete need theta; TD3 and PPO need it unless reward_env_type is 0 (the real env itself: nothing to evaluate)."""
    call = CALLS[name]
    assert call.run(theta=None) == INVALID
    if isinstance(call.good["cfg"], (_lib.Td3Cfg, _lib.PpoCfg)):
        assert call.good["cfg"].reward_env_type != 0
        assert call.run(theta=None, cfg=_copy(call.good["cfg"], reward_env_type=0), chains=0) == OK
        assert call.run(theta=None, chains=0) == INVALID


@pytest.mark.parametrize("name", FUSED + TABULAR)
def test_eps_needs_worker_and_sign(name):
    assert CALLS[name].run(eps=P, worker=None, sign=P) == INVALID
    assert CALLS[name].run(eps=P, worker=P, sign=None) == INVALID
    assert CALLS[name].run(eps=P, worker=P, sign=P, chains=0) == OK


@pytest.mark.parametrize("name", FUSED + TABULAR)
def test_rng_mode_needs_its_source(name):
    call = CALLS[name]
    assert call.run(cfg=_copy(call.good["cfg"], rng_mode=_lib.RNG_TAPE), tapes=None) == INVALID
    assert call.run(rng_keys=None) == INVALID                              # counter mode without keys
    # tape mode needs no keys
    tapes = TAPES[type(call.good["cfg"])](**{k: P for k in TAPES[type(call.good["cfg"])].keys})
    assert call.run(cfg=_copy(call.good["cfg"], rng_mode=_lib.RNG_TAPE), tapes=tapes, rng_keys=None, chains=0) == OK


@pytest.mark.parametrize("name", HP)
@pytest.mark.parametrize("member", ["lr", "batch_size", "q_hidden", "q_layers"])
def test_hp_with_a_null_member(name, member):
    hp = _lib.ChainHp(lr=P, batch_size=P, q_hidden=P, q_layers=P)
    assert CALLS[name].run(hp=hp, chains=0) == OK
    setattr(hp, member, None)
    assert CALLS[name].run(hp=hp) == INVALID
    assert CALLS[name].run(hp=hp, chains=0) == INVALID


@pytest.mark.parametrize("name", ICM)
def test_icm_agent_needs_its_io(name):
    call = CALLS[name]
    cfg = _copy(call.good["cfg"], icm_enabled=1, icm_feature_dim=8, icm_hidden=8)
    assert call.run(cfg=cfg, icm=None) == INVALID
    assert call.run(cfg=cfg, icm=_lib.IcmIo()) == INVALID                   # icm_init null
    assert call.run(cfg=cfg, icm=_lib.IcmIo(icm_init=P), chains=0) == OK
    assert call.run(icm=None, chains=0) == OK                               # no ICM: icm is not read
    # ... and with a null hp member or a null cfg next to it
    assert call.run(cfg=None, icm=None) == INVALID
    assert call.run(cfg=cfg, icm=None, hp=_lib.ChainHp()) == INVALID


@pytest.mark.parametrize("name", ["lenv_dueling_se_inner_loop", "lenv_dueling_se_inner_loop_hp", "lenv_td3_rn_inner_loop", "lenv_td3_rn_inner_loop_hp"])
def test_icm_cfg_through_an_entry_without_icm(name):
    call = CALLS[name]
    cfg = _copy(call.good["cfg"], icm_enabled=1, icm_feature_dim=8, icm_hidden=8)
    assert call.run(cfg=cfg) == INVALID
    assert call.run(cfg=cfg, chains=0) == INVALID


def test_ddqn_kernel_refuses_icm_as_unsupported():
    call = CALLS["lenv_ddqn_se_inner_loop"]
    assert call.run(cfg=_copy(call.good["cfg"], icm_enabled=1, icm_feature_dim=8, icm_hidden=8)) == UNSUPPORTED


@pytest.mark.parametrize("name", SEGMENT)
def test_segment_range(name):
    call = CALLS[name]
    n = call.good["cfg"].train_episodes
    assert n == 3
    assert call.run(episode_begin=-1) == INVALID
    assert call.run(episode_begin=1, episode_end=1) == INVALID
    assert call.run(episode_begin=2, episode_end=1) == INVALID
    assert call.run(episode_begin=0, episode_end=n + 1) == INVALID
    assert call.run(resume=None) == INVALID
    assert call.run(episode_begin=0, episode_end=n, chains=0) == OK
    assert call.run(episode_begin=n - 1, episode_end=n, chains=0) == OK
    assert call.run(episode_begin=n, episode_end=n + 1, chains=0) == INVALID


WORKSPACE_QUERY = {"lenv_ddqn": ("lenv_ddqn_se_workspace_bytes", 0), "lenv_dueling": ("lenv_dueling_se_workspace_bytes", 256),
                   "lenv_td3_": ("lenv_td3_rn_workspace_bytes", 256), "lenv_td3d_inner": ("lenv_td3d_workspace_bytes", 256),
                   "lenv_td3d_rn": ("lenv_td3d_rn_workspace_bytes", 256), "lenv_ppo": ("lenv_ppo_rn_workspace_bytes", 256)}


@pytest.mark.parametrize("name", FUSED)
def test_workspace_one_byte_short(name):
    """The queries of the arena families answer 256 bytes more than the launch insists on; the DDQN launch insists on its query's answer."""
    call = CALLS[name]
    query, slack = next(v for k, v in WORKSPACE_QUERY.items() if name.startswith(k))
    lead = [C.byref(call.good["cfg"])] + ([C.byref(call.good["rn"])] if "rn" in call.params else [])
    need = getattr(_lib.lib(), query)(*lead, 2) - slack
    assert need > 0
    assert call.run(workspace_bytes=need - 1) == WORKSPACE
    assert call.run(workspace_bytes=0) == WORKSPACE


def test_workspace_of_the_gridworld_virtual_env_loop():
    call = CALLS["lenv_ql_se_inner_loop"]
    assert call.run(workspace=None, workspace_bytes=0, chains=0) == OK       # the staged theta fits LDS: no workspace
    cfg = _ql_se_cfg(rn_hidden=128, rn_layers=2)
    need = _lib.lib().lenv_ql_se_workspace_bytes(C.byref(cfg), 2)
    assert need > 0
    assert call.run(cfg=cfg, workspace_bytes=need - 1) == WORKSPACE
    assert call.run(cfg=cfg, workspace=None, workspace_bytes=need) == WORKSPACE
    assert call.run(cfg=cfg, workspace=None, workspace_bytes=need, chains=0) == OK


@pytest.mark.parametrize("name", sorted(CALLS))
def test_unsupported_cfg_and_zero_chains(name):
    """An unsupported cfg is refused by every launch; with zero chains the launchers return before they look at the cfg's shapes -- but for PPO
    and the gridworld VirtualEnv loop, which run their layout / check first."""
    call = CALLS[name]
    assert call.run(chains=0) == OK
    assert call.run(cfg=_bad_cfg(call)) == UNSUPPORTED
    layout_first = name.startswith("lenv_ppo") or name == "lenv_ql_se_inner_loop"
    assert call.run(cfg=_bad_cfg(call), chains=0) == (UNSUPPORTED if layout_first else OK)


def test_family_rules_of_ppo():
    for name in ("lenv_ppo_rn_inner_loop", "lenv_ppo_rn_inner_loop_segment"):
        call = CALLS[name]
        tape_cfg = _copy(call.good["cfg"], rng_mode=_lib.RNG_TAPE)
        for k in _lib.PpoTapes.keys:
            tapes = _lib.PpoTapes(**{j: P for j in _lib.PpoTapes.keys if j != k})
            assert call.run(cfg=tape_cfg, tapes=tapes, chains=0) == INVALID
        assert call.run(cfg=_copy(call.good["cfg"], rng_mode=2)) == INVALID
        assert call.run(cfg=_copy(call.good["cfg"], rng_mode=2), tapes=_lib.PpoTapes(**{j: P for j in _lib.PpoTapes.keys}), chains=0) == INVALID
        for k in ("trace_action", "trace_state", "trace_next_state"):
            out = _lib.PpoOut(score=P, trace_cap=4, trace_reward=P, trace_action=P, trace_state=P, trace_next_state=P)
            assert call.run(out=out, chains=0) == OK
            setattr(out, k, None)
            assert call.run(out=out, chains=0) == INVALID
            out.trace_cap = 0
            assert call.run(out=out, chains=0) == OK
        assert call.run(cfg=_copy(call.good["cfg"], reserved=1), chains=0) == UNSUPPORTED


def test_family_rules_of_td3_discrete_on_a_reward_env():
    call = CALLS["lenv_td3d_rn_inner_loop"]
    assert call.run(rn=None) == INVALID
    assert call.run(rn=None, chains=0) == INVALID
    assert call.run(rn=_copy(call.good["rn"], reward_env_type=3)) == UNSUPPORTED
    assert call.run(rn=_copy(call.good["rn"], synthetic_env_type=0)) == UNSUPPORTED
    assert call.run(rn=_copy(call.good["rn"], reward_env_type=3), chains=0) == OK


def test_family_rules_of_the_tabular_loops():
    for name in ("lenv_ql_rn_inner_loop", "lenv_ql_rn_inner_loop_hp", "lenv_ql_se_inner_loop"):
        call = CALLS[name]
        for k in ("next_state", "reward", "done", "out"):
            assert call.run(**{k: None}) == INVALID
        assert call.run(out=_lib.QlOut()) == INVALID
    for name in ("lenv_ql_rn_inner_loop", "lenv_ql_rn_inner_loop_hp"):
        call = CALLS[name]
        assert call.run(theta=None) == INVALID
        assert call.run(theta=None, shaped_override=P, chains=0) == OK
        assert call.run(cfg=_copy(call.good["cfg"], reward_env_type=3)) == UNSUPPORTED
        assert call.run(cfg=_copy(call.good["cfg"], n_states=1 << 20)) == UNSUPPORTED      # the tables do not fit LDS
        assert call.run(cfg=_copy(call.good["cfg"], agent_kind=2)) == UNSUPPORTED
    call = CALLS["lenv_ql_se_inner_loop"]
    assert call.run(theta=None) == INVALID
    tape_cfg = _copy(call.good["cfg"], rng_mode=_lib.RNG_TAPE)
    assert call.run(cfg=tape_cfg, tapes=_lib.Tapes(eps_uniform=P), chains=0) == INVALID
    assert call.run(cfg=tape_cfg, tapes=_lib.Tapes(rand_action=P), chains=0) == INVALID
    assert call.run(cfg=tape_cfg, tapes=_lib.Tapes(eps_uniform=P, rand_action=P), chains=0) == OK
    assert call.run(out=_lib.QlOut(score=P, trace_cap=4, trace_action=P), chains=0) == INVALID
    assert call.run(out=_lib.QlOut(score=P, trace_cap=4, trace_action=P, trace_state=P, trace_reward_done=P), chains=0) == OK
    assert call.run(cfg=_copy(call.good["cfg"], rng_mode=2)) == UNSUPPORTED


@pytest.mark.parametrize("name", AGENT_INIT)
def test_agent_init_entries(name):
    call = CALLS[name]
    assert call.run(rng_keys=None) == INVALID
    assert call.run(agent_init=None) == INVALID
    assert call.run(hp=_lib.ChainHp(q_hidden=P)) == INVALID
    assert call.run(hp=_lib.ChainHp(q_layers=P)) == INVALID
    assert call.run(hp=_lib.ChainHp(q_hidden=P, q_layers=P), chains=0) == OK      # lr / batch_size are not read here


# ---- layout queries: bytes and counts for a dozen cfgs, literals from the library before the fold ----

def _vary_max(cfgd, section):
    bd = vary.hp_bounds(cfgd["agents"][section])
    return dict(batch_size=bd["batch_size"][1], hidden=bd["hidden_size"][1], layers=max(1, bd["hidden_layer"][1]))


def _layout_cfgs():
    L = _lib.lib()
    ddqn, td3 = config.ddqn_cfg_from_config, config.td3_cfg_from_config
    out = {}

    def dueling_family(key, cfg):
        out[key] = [L.lenv_dueling_se_workspace_bytes(C.byref(cfg), 1), L.lenv_dueling_se_workspace_bytes(C.byref(cfg), 48),
                    L.lenv_dueling_num_params(C.byref(cfg)), L.lenv_icm_num_params(C.byref(cfg))]

    def td3_family(key, cfg):
        pa, pc = C.c_int64(), C.c_int64()
        out[key] = [L.lenv_td3_rn_workspace_bytes(C.byref(cfg), 1), L.lenv_td3_rn_workspace_bytes(C.byref(cfg), 48),
                    L.lenv_td3_num_params(C.byref(cfg), C.byref(pa), C.byref(pc)), pa.value, pc.value, L.lenv_td3_icm_num_params(C.byref(cfg))]

    cfg = ddqn(configs.cartpole_syn_env_ddqn())
    out["ddqn_cartpole"] = [L.lenv_ddqn_se_workspace_bytes(C.byref(cfg), 1), L.lenv_ddqn_se_workspace_bytes(C.byref(cfg), 48), L.lenv_ddqn_se_lds_bytes(C.byref(cfg))]
    cfg = ddqn(configs.cartpole_reward_env_ddqn())
    out["ddqn_cartpole_reward_env"] = [L.lenv_ddqn_se_workspace_bytes(C.byref(cfg), 1), L.lenv_ddqn_se_workspace_bytes(C.byref(cfg), 48), L.lenv_ddqn_se_lds_bytes(C.byref(cfg))]
    dueling_family("dueling_acrobot_wavechain", ddqn(configs.acrobot_syn_env_duelingddqn()))
    dueling_family("ddqn_acrobot_wavechain", ddqn(configs.acrobot_syn_env_ddqn()))
    dueling_family("ddqn_mountaincar_wide", ddqn(configs.mountaincar_syn_env_ddqn()))
    dueling_family("dueling_acrobot_icm", ddqn(configs.with_icm(configs.acrobot_syn_env_duelingddqn())))
    cfgd = configs.acrobot_syn_env_duelingddqn()
    cfgd["agents"]["duelingddqn"]["use_layer_norm"] = True
    cfgd["envs"]["Acrobot-v1"].update(hidden_layer=2)
    dueling_family("dueling_acrobot_layer_norm_deep_se", ddqn(cfgd))
    cfgd = configs.acrobot_syn_env_duelingddqn()
    bd = vary.hp_bounds(cfgd["agents"]["duelingddqn"])
    dueling_family("dueling_acrobot_vary_max", ddqn(cfgd, batch_size=bd["batch_size"][1], q_hidden=bd["hidden_size"][1], q_layers=bd["hidden_layer"][1]))
    dueling_family("ddqn_cartpole_reward_env_generic", ddqn(configs.cartpole_reward_env_ddqn(), grad_chunk=0, q_layers=2))
    td3_family("td3_halfcheetah_reward_env_wavechain", td3(configs.halfcheetah_reward_env_td3()))
    td3_family("td3_pendulum_virtual_env_wavechain", td3(configs.pendulum_syn_env_td3()))
    td3_family("td3_pendulum_reward_env_deep_rn", td3(configs.pendulum_reward_env_td3()))
    cfgd = configs.halfcheetah_reward_env_td3()
    cfgd["agents"]["td3"]["use_layer_norm"] = True
    td3_family("td3_halfcheetah_layer_norm", td3(cfgd))
    td3_family("td3_cmc_icm", td3(configs.with_icm(configs.cmc_reward_env_td3())))
    cfgd = configs.pendulum_syn_env_td3()
    td3_family("td3_pendulum_vary_max", td3(cfgd, **_vary_max(cfgd, "td3")))
    cfg = config.td3d_cfg_from_config(configs.cartpole_syn_env_td3_discrete())
    pa, pc = C.c_int64(), C.c_int64()
    out["td3d_cartpole"] = [L.lenv_td3d_workspace_bytes(C.byref(cfg), 1), L.lenv_td3d_workspace_bytes(C.byref(cfg), 48),
                            L.lenv_td3d_num_params(C.byref(cfg), C.byref(pa), C.byref(pc)), pa.value, pc.value, L.lenv_td3d_se_num_params(C.byref(cfg))]
    rn = _td3d_rn()
    out["td3d_cartpole_reward_env"] = [L.lenv_td3d_rn_workspace_bytes(C.byref(cfg), C.byref(rn), 1), L.lenv_td3d_rn_workspace_bytes(C.byref(cfg), C.byref(rn), 48),
                                       L.lenv_td3d_rn_num_params(C.byref(cfg), C.byref(rn))]
    cfg = config.ppo_cfg_from_config(configs.pendulum_reward_env_ppo())
    out["ppo_pendulum"] = [L.lenv_ppo_rn_workspace_bytes(C.byref(cfg), 1), L.lenv_ppo_rn_workspace_bytes(C.byref(cfg), 48), L.lenv_ppo_num_params(C.byref(cfg), C.byref(pa), C.byref(pc)),
                           pa.value, pc.value, L.lenv_ppo_rn_num_params(C.byref(cfg)), L.lenv_ppo_rn_lds_bytes(C.byref(cfg)), L.lenv_ppo_rows(C.byref(cfg))]
    cfg = _ql_se_cfg(rn_hidden=128, rn_layers=2)
    out["ql_se_cliff_128x2"] = [L.lenv_ql_se_workspace_bytes(C.byref(cfg), 1), L.lenv_ql_se_workspace_bytes(C.byref(cfg), 48), L.lenv_ql_se_num_params(C.byref(cfg)),
                                L.lenv_ql_se_lds_bytes(C.byref(cfg))]
    cfg = _ql_se_cfg()
    out["ql_se_cliff"] = [L.lenv_ql_se_workspace_bytes(C.byref(cfg), 1), L.lenv_ql_se_workspace_bytes(C.byref(cfg), 48), L.lenv_ql_se_num_params(C.byref(cfg)),
                          L.lenv_ql_se_lds_bytes(C.byref(cfg))]
    return out


# [workspace bytes for 1 chain, for 48 chains, then the family's counts in the order _layout_cfgs asks for them]
LAYOUTS = {
    "ddqn_cartpole": [6485760, 236083200, 156768],
    "ddqn_cartpole_reward_env": [1208064, 50432256, 158208],
    "dueling_acrobot_wavechain": [8746752, 419832064, 67460, -1],
    "ddqn_acrobot_wavechain": [8517376, 408822016, 17795, -1],
    "ddqn_mountaincar_wide": [6134528, 294445312, 67331, -1],
    "dueling_acrobot_icm": [11746048, 563798272, 67460, 89571],
    "dueling_acrobot_layer_norm_deep_se": [9017088, 432808192, 67716, -1],
    "dueling_acrobot_vary_max": [22897920, 1099088128, 381188, -1],
    "ddqn_cartpole_reward_env_generic": [1654016, 79380736, 4610, -1],
    "td3_halfcheetah_reward_env_wavechain": [20482560, 983150848, 59016, 19590, 19713, -1],
    "td3_pendulum_virtual_env_wavechain": [4049408, 194359552, 51715, 17153, 17281, -1],
    "td3_pendulum_reward_env_deep_rn": [3622912, 173887744, 51715, 17153, 17281, -1],
    "td3_halfcheetah_layer_norm": [20559360, 986837248, 59784, 19846, 19969, -1],
    "td3_cmc_icm": [9344256, 448512256, 51331, 17025, 17153, 88033],
    "td3_pendulum_vary_max": [35148288, 1687105792, 893571, 297601, 297985, -1],
    "td3d_cartpole": [28992000, 1391603968, 793564, 264182, 264691, 2247],
    "td3d_cartpole_reward_env": [28985088, 1391272192, 499],
    "ppo_pendulum": [1803008, 86532352, 8963, 4481, 4481, 17153, 108328, 1001],
    "ql_se_cliff_128x2": [305408, 14659584, 76338, 5824],
    "ql_se_cliff": [0, 0, 6738, 30472],
}


def test_layout_queries_answer_what_they_answered_before_the_fold():
    got = _layout_cfgs()
    assert sorted(got) == sorted(LAYOUTS)
    for key in sorted(LAYOUTS):
        assert got[key] == LAYOUTS[key], key
    # every family refused nothing here, and the wave-chain shapes are the ones the names say
    assert all(v[0] > 0 or key == "ql_se_cliff" for key, v in got.items())
    L = _lib.lib()
    assert L.lenv_dueling_se_workspace_bytes(None, 1) == 0 and L.lenv_td3_rn_workspace_bytes(None, 1) == 0 and L.lenv_ppo_rn_workspace_bytes(None, 1) == INVALID
