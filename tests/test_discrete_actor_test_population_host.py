"""lenv_td3d_test_population and lenv_ql_test_population without a device: the four symbols, the unchanged ABI housekeeping, every refusal of
the two entries (the checks run before any launch, so agents = 0 and host pointers do), the rows_cap values, and the host-side pieces above
them: engine.td3d_test_num_params, the refusals of rollout.test_discrete_actor_agents / test_tabular_agents by agent name,
ReplayRows.make_one_hot_buffer, and the settings block and skip rule of experiments/gridworld_heatmap."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

CARTPOLE, ACROBOT, MOUNTAINCAR = 0, 1, 3
OK, INVALID, UNSUPPORTED = 0, -1, -2
PRELU = 4


@pytest.fixture(scope="module")
def L():
    from learning_environments_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def p():
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    p._keep = buf
    return p


def _cfg(**over):
    """A cfg inside the envelope; only the fields the entry reads are set (training fields stay 0: they are ignored)."""
    from learning_environments_amd import _lib
    kw = dict(env_id=_lib.ENV["CartPole-v0"], state_dim=4, action_dim=2, max_steps=40, test_episodes=3, hidden=24, layers=2, act=1, use_layer_norm=0,
              gumbel_hard=0, gumbel_temp=1.0, action_std=0.1, max_action=1.0)
    kw.update(over)
    return _lib.Td3dCfg(**kw)


def _qcfg(**over):
    from learning_environments_amd import _lib
    kw = dict(n_states=48, n_actions=4, start_state=36, max_steps=40, test_episodes=2, same_action_num=1)
    kw.update(over)
    return _lib.QlCfg(**kw)


def _call(L, p, cfg="auto", agents=0, rows="none", **ptrs):
    """The TD3-discrete entry with dummy non-NULL host pointers; only calls that are refused or launch nothing (agents = 0) are made."""
    if isinstance(cfg, str):
        cfg = _cfg()
    a = dict(params=p, rng_keys=p, episode_offset=None, learn_calls=None, reset_states=None, gumbel=None, noise=None, returns=p, env_steps=p, agent_steps=p)
    a.update(ptrs)
    r = {"none": [None] * 5, "all": [p] * 5}[rows] if isinstance(rows, str) else rows
    return L.lenv_td3d_test_population(C.byref(cfg) if cfg is not None else None, a["params"], a["rng_keys"], a["episode_offset"], a["learn_calls"],
                                       a["reset_states"], a["gumbel"], a["noise"], agents, a["returns"], a["env_steps"], a["agent_steps"], *r, None)


def _qcall(L, p, cfg="auto", agents=0, rows="none", **ptrs):
    if isinstance(cfg, str):
        cfg = _qcfg()
    a = dict(q_table=p, next_state=p, reward=p, done=p, returns=p, env_steps=p, agent_steps=p)
    a.update(ptrs)
    r = {"none": [None] * 5, "all": [p] * 5}[rows] if isinstance(rows, str) else rows
    return L.lenv_ql_test_population(C.byref(cfg) if cfg is not None else None, a["q_table"], a["next_state"], a["reward"], a["done"], agents,
                                     a["returns"], a["env_steps"], a["agent_steps"], *r, None)


def test_symbols_and_unchanged_abi(L):
    import os
    from learning_environments_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lenv_hip.h")).read()
    for name in ("lenv_td3d_test_population", "lenv_td3d_test_rows_cap", "lenv_ql_test_population", "lenv_ql_test_rows_cap"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert name + "(" in header, name
    assert L.lenv_abi_version() == 7
    assert len(_lib.ABI_STRUCTS) == 17                  # functions only: no new struct
    assert L.lenv_struct_size(17) == -1
    assert len(_lib.SIGNATURES["lenv_td3d_test_population"][1]) == 18
    assert len(_lib.SIGNATURES["lenv_ql_test_population"][1]) == 15
    assert len(_lib.SIGNATURES["lenv_td3d_test_rows_cap"][1]) == len(_lib.SIGNATURES["lenv_ql_test_rows_cap"][1]) == 1


# ---- lenv_td3d_test_population ----

def test_td3d_no_agents_is_ok_after_the_checks(L, p):
    assert _call(L, p) == OK
    assert _call(L, p, rows="all") == OK
    assert _call(L, p, episode_offset=p, learn_calls=p, reset_states=p, gumbel=p, noise=p) == OK
    assert _call(L, p, gumbel=p) == OK and _call(L, p, noise=p) == OK          # each tape on its own
    far = _cfg(env_id=ACROBOT, state_dim=6, action_dim=3, hidden=512, layers=3, use_layer_norm=1, gumbel_hard=1, test_episodes=64)
    assert _call(L, p, cfg=far) == OK
    assert _call(L, p, cfg=_cfg(env_id=MOUNTAINCAR, state_dim=2, action_dim=3, hidden=1, layers=1, test_episodes=1, max_steps=1, gumbel_temp=1e-9)) == OK


def test_env_ids_are_the_librarys():
    from learning_environments_amd import _lib
    assert (_lib.ENV["CartPole-v0"], _lib.ENV["Acrobot-v1"], _lib.ENV["MountainCar-v0"]) == (CARTPOLE, ACROBOT, MOUNTAINCAR)


@pytest.mark.parametrize("name", ["params", "rng_keys", "returns", "env_steps", "agent_steps"])
def test_td3d_null_required_pointer_is_invalid(L, p, name):
    assert _call(L, p, **{name: None}) == INVALID


def test_td3d_null_cfg_negative_agents_and_max_steps_are_invalid(L, p):
    assert _call(L, p, cfg=None) == INVALID
    assert _call(L, p, agents=-1) == INVALID
    assert L.lenv_td3d_test_rows_cap(None) == INVALID
    for ms in (0, -3):
        assert _call(L, p, cfg=_cfg(max_steps=ms)) == INVALID
        assert L.lenv_td3d_test_rows_cap(C.byref(_cfg(max_steps=ms))) == INVALID


PARTIAL = [(1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (1, 1, 1, 1, 0), (0, 1, 1, 1, 1), (1, 1, 0, 1, 1)]


@pytest.mark.parametrize("given", PARTIAL)
def test_td3d_row_arrays_given_in_part_are_invalid(L, p, given):
    assert _call(L, p, rows=[p if g else None for g in given]) == INVALID


@pytest.mark.parametrize("over", [dict(env_id=2), dict(env_id=4), dict(env_id=-1), dict(env_id=ACROBOT), dict(env_id=MOUNTAINCAR), dict(state_dim=6),
                                  dict(action_dim=3), dict(env_id=MOUNTAINCAR, state_dim=2, action_dim=2), dict(hidden=0), dict(hidden=513), dict(layers=0),
                                  dict(layers=4), dict(test_episodes=0), dict(test_episodes=65), dict(act=PRELU), dict(act=5), dict(act=-1),
                                  dict(gumbel_temp=0.0), dict(gumbel_temp=-1.0), dict(gumbel_temp=float("nan"))])
def test_td3d_outside_the_envelope_is_unsupported(L, p, over):
    cfg = _cfg(**over)
    assert _call(L, p, cfg=cfg) == UNSUPPORTED
    assert L.lenv_td3d_test_rows_cap(C.byref(cfg)) == UNSUPPORTED


def test_td3d_training_fields_are_not_read(L, p):
    """batch_size, the SE nets, train_episodes, policy_delay ... are whatever they are; the fused entry itself refuses this cfg."""
    cfg = _cfg(batch_size=100000, se_hidden=-7, se_layers=99, train_episodes=-1, policy_delay=0, rb_size=-5, test_mode=5, init_episodes=-2, rng_mode=9,
               lr=float("nan"), tau=-1.0, step_budget=-9, se_layer_norm=3)
    assert _call(L, p, cfg=cfg) == OK and L.lenv_td3d_test_rows_cap(C.byref(cfg)) == 40
    assert L.lenv_td3d_num_params(C.byref(cfg), None, None) == UNSUPPORTED


def test_td3d_rows_cap_is_max_steps(L):
    for ms in (1, 7, 200, 999):
        assert L.lenv_td3d_test_rows_cap(C.byref(_cfg(max_steps=ms))) == ms


def test_td3d_num_params_matches_the_fused_entry(L):
    from learning_environments_amd import configs, engine
    from learning_environments_amd.config import td3d_cfg_from_config
    for make, over in ((configs.cartpole_syn_env_td3_discrete, {}), (configs.cartpole_syn_env_td3_discrete, dict(use_layer_norm=True, hidden_layer=3, hidden_size=33)),
                       (configs.acrobot_syn_env_td3_discrete, dict(use_layer_norm=True, hidden_layer=1, hidden_size=5))):
        cfg = td3d_cfg_from_config(make(2, **over))
        assert engine.td3d_test_num_params(cfg) == L.lenv_td3d_num_params(C.byref(cfg), None, None) > 0


# ---- lenv_ql_test_population ----

def test_ql_no_agents_is_ok_after_the_checks(L, p):
    assert _qcall(L, p) == OK and _qcall(L, p, rows="all") == OK
    assert _qcall(L, p, cfg=_qcfg(n_actions=8, test_episodes=128, same_action_num=64)) == OK
    assert _qcall(L, p, cfg=_qcfg(n_states=1, n_actions=1, start_state=0, test_episodes=1, same_action_num=0, max_steps=1)) == OK


@pytest.mark.parametrize("name", ["q_table", "next_state", "reward", "done", "returns", "env_steps", "agent_steps"])
def test_ql_null_required_pointer_is_invalid(L, p, name):
    assert _qcall(L, p, **{name: None}) == INVALID


def test_ql_null_cfg_negative_agents_and_max_steps_are_invalid(L, p):
    assert _qcall(L, p, cfg=None) == INVALID
    assert _qcall(L, p, agents=-1) == INVALID
    assert L.lenv_ql_test_rows_cap(None) == INVALID
    assert _qcall(L, p, cfg=_qcfg(max_steps=0)) == INVALID
    assert L.lenv_ql_test_rows_cap(C.byref(_qcfg(max_steps=0))) == INVALID


@pytest.mark.parametrize("given", PARTIAL)
def test_ql_row_arrays_given_in_part_are_invalid(L, p, given):
    assert _qcall(L, p, rows=[p if g else None for g in given]) == INVALID


@pytest.mark.parametrize("over", [dict(n_actions=0), dict(n_actions=9), dict(test_episodes=0), dict(test_episodes=129), dict(same_action_num=-1),
                                  dict(same_action_num=65), dict(start_state=48), dict(start_state=-1), dict(n_states=0)])
def test_ql_outside_the_envelope_is_unsupported(L, p, over):
    cfg = _qcfg(**over)
    assert _qcall(L, p, cfg=cfg) == UNSUPPORTED
    assert L.lenv_ql_test_rows_cap(C.byref(cfg)) == UNSUPPORTED


def test_ql_training_fields_are_not_read(L, p):
    cfg = _qcfg(rn_hidden=-7, rn_layers=99, rn_act=77, reward_env_type=55, train_episodes=-1, init_episodes=-4, batch_size=-1, rng_mode=9, agent_kind=5,
                count_based=3, alpha=float("nan"), gamma=-2.0, step_budget=-9, test_mode=7)
    assert _qcall(L, p, cfg=cfg) == OK and L.lenv_ql_test_rows_cap(C.byref(cfg)) == 40


def test_ql_rows_cap(L):
    cap = lambda **kw: L.lenv_ql_test_rows_cap(C.byref(_qcfg(**kw)))
    assert cap(max_steps=7, same_action_num=3) == 3
    assert cap(max_steps=200, same_action_num=1) == 200
    assert cap(max_steps=200, same_action_num=0) == 200
    assert cap(max_steps=40, same_action_num=64) == 1
    assert cap(max_steps=999, same_action_num=2) == 500


# ---- Python ----

@pytest.mark.parametrize("agent_name", ["TD3", "td3_vary", "DDQN", "QL", "ppo", "DuelingDDQN_vary"])
def test_test_discrete_actor_agents_refuses_other_agents_by_name(agent_name):
    from learning_environments_amd import configs
    from learning_environments_amd.agents.rollout import test_discrete_actor_agents
    c = configs.cartpole_syn_env_td3_discrete(2)
    c["agents"]["gtn"]["agent_name"] = agent_name
    with pytest.raises(NotImplementedError, match=agent_name):
        test_discrete_actor_agents(c, np.zeros((1, 8), np.float32), np.ones(1, np.uint64))


def test_test_discrete_actor_agents_refuses_vary_hp_on():
    from learning_environments_amd import configs
    from learning_environments_amd.agents.rollout import test_discrete_actor_agents
    c = configs.cartpole_syn_env_td3_discrete(2, vary_hp=True)
    with pytest.raises(NotImplementedError, match="(?i)td3_discrete_vary.*vary_hp"):
        test_discrete_actor_agents(c, np.zeros((1, 8), np.float32), np.ones(1, np.uint64))


@pytest.mark.parametrize("agent_name", ["TD3_discrete_vary", "DDQN", "td3", "ppo"])
def test_test_tabular_agents_refuses_other_agents_by_name(agent_name):
    from learning_environments_amd import configs
    from learning_environments_amd.agents.rollout import test_tabular_agents
    c = configs.cliff_reward_env_ql(2)
    c["agents"]["gtn"]["agent_name"] = agent_name
    with pytest.raises(NotImplementedError, match=agent_name):
        test_tabular_agents(c, np.zeros((1, 48 * 4)))


def test_histogram_admits_td3_discrete_vary():
    from learning_environments_amd.experiments import histogram
    assert histogram.AGENTS == ("ddqn", "duelingddqn", "td3_discrete_vary")


def test_make_one_hot_buffer_takes_the_argmax():
    """ReplayBuffer.make_one_hot_buffer (utils.py:71-72): actions -> their argmax, a column; ties go to the first maximum; the other four
    fields stay; an empty buffer stays empty; merging an index buffer into a vector buffer is refused before, accepted after."""
    from learning_environments_amd.agents.rollout import ReplayRows
    rng = np.random.RandomState(3)
    S, A, n = 6, 3, 7
    st, ns = rng.standard_normal((n, S)).astype(np.float32), rng.standard_normal((n, S)).astype(np.float32)
    ac = rng.standard_normal((n, A)).astype(np.float32)
    ac[2] = (0.5, 0.5, 0.5)
    ac[4] = (-1.0, 2.0, 2.0)
    rw, dn = rng.standard_normal(n).astype(np.float32), (rng.uniform(size=n) < 0.3).astype(np.float32)
    rows = ReplayRows(S, st, ac, ns, rw, dn, action_dim=A)
    other = ReplayRows(S, st[:2], ac[:2], ns[:2], rw[:2], dn[:2], action_dim=A)
    rows.merge_buffer(other)
    index_rows = ReplayRows(S)
    with pytest.raises(ValueError):
        index_rows.merge_buffer(rows)
    rows.make_one_hot_buffer()
    s, a, s2, r, d = rows.get_all()
    want = np.concatenate([ac, ac[:2]]).argmax(axis=1).astype(np.float32)[:, None]
    assert rows.action_dim == 1 and a.dtype == torch.float32 and tuple(a.shape) == (n + 2, 1) and np.array_equal(a.numpy(), want)
    assert a[2, 0] == 0.0 and a[4, 0] == 1.0
    assert np.array_equal(s.numpy(), np.concatenate([st, st[:2]])) and np.array_equal(s2.numpy(), np.concatenate([ns, ns[:2]]))
    assert np.array_equal(r.numpy()[:, 0], np.concatenate([rw, rw[:2]])) and np.array_equal(d.numpy()[:, 0], np.concatenate([dn, dn[:2]]))
    index_rows.merge_buffer(rows)
    assert index_rows.get_size() == n + 2
    empty = ReplayRows(S, action_dim=A)
    empty.make_one_hot_buffer()
    assert empty.action_dim == 1 and [tuple(t.shape) for t in empty.get_all()] == [(0, S), (0, 1), (0, S), (0, 1), (0, 1)]


def test_rows_of_episodes_with_state_indices():
    """the gridworld rows: [T,cap] int32 indices become ReplayRows(state_dim=1)"""
    from learning_environments_amd.agents.rollout import rows_of_episodes
    st = np.array([[36, 24, 25, -7], [36, 37, -7, -7]], np.int32)
    ns = np.array([[24, 25, 26, -7], [37, 47, -7, -7]], np.int32)
    ac = np.array([[0, 1, 1, -7], [1, 2, -7, -7]], np.int32)
    rw, dn = np.full((2, 4), -1.0, np.float32), np.zeros((2, 4), np.float32)
    rows = rows_of_episodes(st, ac, ns, rw, dn, [3, 2])
    s, a, s2, r, d = rows.get_all()
    assert rows.state_dim == 1 and rows.action_dim == 1 and rows.get_size() == 5
    assert s[:, 0].tolist() == [36, 24, 25, 36, 37] and s2[:, 0].tolist() == [24, 25, 26, 37, 47] and a[:, 0].tolist() == [0, 1, 1, 1, 2]


def test_heatmap_settings_block_is_the_scripts():
    """GTNC_evaluate_gridworld_heatmap.py:71-86, key for key: three constants, eleven values copied from the QL section."""
    from learning_environments_amd import configs
    from learning_environments_amd.experiments import gridworld_heatmap as gh
    config = configs.cliff_reward_env_ql(2)
    ql = config["agents"]["ql"]
    ql.setdefault("early_out_virtual_diff", 0.02)
    want = {"test_episodes": 1, "train_episodes": 200, "print_rate": 100, "init_episodes": ql["init_episodes"], "batch_size": ql["batch_size"],
            "alpha": ql["alpha"], "gamma": ql["gamma"], "eps_init": ql["eps_init"], "eps_min": ql["eps_min"], "eps_decay": ql["eps_decay"],
            "rb_size": ql["rb_size"], "same_action_num": ql["same_action_num"], "early_out_num": ql["early_out_num"],
            "early_out_virtual_diff": ql["early_out_virtual_diff"]}
    got = gh.sarsa_settings(config)
    assert got == want and list(got) == list(want)             # the script's keys in the script's order
    assert gh.SOLVED_REWARD == {"solved": -20, "end": 100000} and (gh.MODEL_NUM, gh.MODEL_AGENTS) == (10, 10)
    with pytest.raises(ValueError):
        gh.load_envs_and_config("unused.pt", break_="never")


def test_heatmap_skip_rule():
    """`if len(reward) == train_episodes and BREAK == 'solved': continue`"""
    from learning_environments_amd.experiments import gridworld_heatmap as gh
    assert not gh.keep_agent([0.0] * 200, 200, "solved")
    assert gh.keep_agent([0.0] * 199, 200, "solved")
    assert gh.keep_agent([0.0] * 200, 200, "end") and gh.keep_agent([0.0] * 13, 200, "end")
    from learning_environments_amd.agents.rollout import ReplayRows
    rows = ReplayRows(1, [36, 24, 25], [0, 1, 1], [24, 25, 26], [-1, -1, -1], [0, 0, 0])
    assert gh.states_of(rows) == [36, 24, 25, 26]


def test_heatmap_save_list_writes_the_scripts_dict(tmp_path):
    from learning_environments_amd.experiments import gridworld_heatmap as gh
    f = str(tmp_path / "heatmap_solved_6.pt")
    gh.save_list({"env_name": "Cliff"}, [[36, 24], [36, 37, 47]], f, mode=6)
    d = torch.load(f)
    assert d == {"config": {"env_name": "Cliff"}, "model_num": 10, "model_agents": 10, "mode": "6", "break": "solved", "state_list": [[36, 24], [36, 37, 47]]}
