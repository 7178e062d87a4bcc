"""lenv_agent_test_population without a device: the two symbols, the unchanged ABI housekeeping, every refusal of the entry (the checks run
before any launch, so agents = 0 and host pointers do), lenv_agent_test_rows_cap, and the host-side pieces above it: ReplayRows and
histogram.compare_env_output on a stub env."""
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
    kw = dict(env_id=CARTPOLE, state_dim=4, num_actions=2, max_steps=40, q_hidden=24, q_layers=1, q_act=3, q_prelu=0.25, agent_kind=0,
              feature_dim=0, q_layer_norm=0, test_episodes=3, same_action_num=1)
    kw.update(over)
    return _lib.DdqnCfg(**kw)


def _call(L, p, cfg="auto", agents=0, rows="none", **ptrs):
    """The entry with dummy non-NULL host pointers; only calls that are refused or launch nothing (agents = 0) are made."""
    if isinstance(cfg, str):
        cfg = _cfg()
    a = dict(params=p, rng_keys=p, episode_offset=None, reset_states=None, returns=p, env_steps=p, agent_steps=p)
    a.update(ptrs)
    r = {"none": [None] * 5, "all": [p] * 5}[rows] if isinstance(rows, str) else rows
    return L.lenv_agent_test_population(C.byref(cfg) if cfg is not None else None, a["params"], a["rng_keys"], a["episode_offset"], a["reset_states"],
                                        agents, a["returns"], a["env_steps"], a["agent_steps"], *r, None)


def test_symbols_and_unchanged_abi(L):
    from learning_environments_amd import _lib
    for name in ("lenv_agent_test_population", "lenv_agent_test_rows_cap"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.lenv_abi_version() == 7
    assert len(_lib.ABI_STRUCTS) == 17
    assert L.lenv_struct_size(17) == -1
    assert len(_lib.SIGNATURES["lenv_agent_test_population"][1]) == 15


def test_no_agents_is_ok_after_the_checks(L, p):
    assert _call(L, p) == OK
    assert _call(L, p, rows="all") == OK
    assert _call(L, p, episode_offset=p, reset_states=p) == OK
    assert _call(L, p, cfg=_cfg(env_id=ACROBOT, state_dim=6, num_actions=3, agent_kind=1, feature_dim=128, q_hidden=512, q_layers=3, q_layer_norm=1,
                                test_episodes=128, same_action_num=64)) == OK


@pytest.mark.parametrize("name", ["params", "rng_keys", "returns", "env_steps", "agent_steps"])
def test_null_required_pointer_is_invalid(L, p, name):
    assert _call(L, p, **{name: None}) == INVALID


def test_null_cfg_and_negative_agents_are_invalid(L, p):
    assert _call(L, p, cfg=None) == INVALID
    assert _call(L, p, agents=-1) == INVALID
    assert L.lenv_agent_test_rows_cap(None) == INVALID


@pytest.mark.parametrize("given", [(1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (1, 1, 1, 1, 0), (0, 1, 1, 1, 1), (1, 1, 0, 1, 1)])
def test_row_arrays_given_in_part_are_invalid(L, p, given):
    assert _call(L, p, rows=[p if g else None for g in given]) == INVALID


@pytest.mark.parametrize("over", [dict(env_id=2), dict(env_id=4), dict(env_id=-1), dict(env_id=ACROBOT), dict(state_dim=5), dict(num_actions=3),
                                  dict(q_hidden=513), dict(q_hidden=0), dict(q_layers=4), dict(q_layers=0), dict(test_episodes=0),
                                  dict(test_episodes=129), dict(q_act=PRELU), dict(same_action_num=65), dict(same_action_num=-1),
                                  dict(agent_kind=1, feature_dim=0), dict(agent_kind=1, feature_dim=129)])
def test_outside_the_envelope_is_unsupported(L, p, over):
    cfg = _cfg(**over)
    assert _call(L, p, cfg=cfg) == UNSUPPORTED
    assert L.lenv_agent_test_rows_cap(C.byref(cfg)) == UNSUPPORTED


def test_training_fields_are_not_read(L, p):
    """batch_size, se_hidden, train_episodes, the ICM fields and test_mode are whatever they are."""
    cfg = _cfg(batch_size=100000, se_hidden=-7, se_layers=99, train_episodes=-1, icm_enabled=1, icm_feature_dim=9999, test_mode=5, grad_chunk=3)
    assert _call(L, p, cfg=cfg) == OK and L.lenv_agent_test_rows_cap(C.byref(cfg)) == 40


def test_rows_cap(L):
    assert L.lenv_agent_test_rows_cap(C.byref(_cfg(max_steps=40, same_action_num=3))) == 14
    assert L.lenv_agent_test_rows_cap(C.byref(_cfg(max_steps=40, same_action_num=0))) == 40
    assert L.lenv_agent_test_rows_cap(C.byref(_cfg(max_steps=40, same_action_num=1))) == 40
    assert L.lenv_agent_test_rows_cap(C.byref(_cfg(max_steps=40, same_action_num=64))) == 1
    assert L.lenv_agent_test_rows_cap(C.byref(_cfg(max_steps=200, same_action_num=2))) == 100


def test_num_params_matches_the_generic_kernels():
    """engine.agent_test_num_params (network fields only) = lenv_dueling_num_params on complete cfgs: the row width of final_online."""
    from learning_environments_amd import _lib, configs, engine
    from learning_environments_amd.config import ddqn_cfg_from_config
    for cfgd, ln in ((configs.acrobot_syn_env_duelingddqn(4), False), (configs.mountaincar_syn_env_ddqn(4), False), (configs.mountaincar_syn_env_ddqn(4), True),
                     (configs.acrobot_syn_env_duelingddqn(4), True)):
        cfg = ddqn_cfg_from_config(cfgd)
        cfg.q_layer_norm = 1 if ln else 0
        assert engine.agent_test_num_params(cfg) == _lib.lib().lenv_dueling_num_params(C.byref(cfg)) > 0


def test_replay_rows_order_shapes_and_merge():
    from learning_environments_amd.agents.rollout import ReplayRows, rows_of_episodes
    S, T, cap = 3, 2, 4
    state = np.arange(T * cap * S, dtype=np.float32).reshape(T, cap, S)
    nxt = state + 100.0
    action = np.arange(T * cap, dtype=np.int32).reshape(T, cap) % 3
    reward = -np.arange(T * cap, dtype=np.float32).reshape(T, cap)
    done = np.zeros((T, cap), np.float32)
    done[0, 2] = done[1, 0] = 1.0
    rows = rows_of_episodes(state, action, nxt, reward, done, [3, 1])          # episode 0 filled three slots, episode 1 one
    s, a, s2, r, d = rows.get_all()
    assert [tuple(t.shape) for t in (s, a, s2, r, d)] == [(4, S), (4, 1), (4, S), (4, 1), (4, 1)]
    assert all(t.dtype == torch.float32 and t.device.type == "cpu" for t in (s, a, s2, r, d))
    assert np.array_equal(s.numpy(), np.concatenate([state[0, :3], state[1, :1]]))           # episode after episode, step after step
    assert np.array_equal(s2.numpy(), s.numpy() + 100.0)
    assert a.reshape(-1).tolist() == [0.0, 1.0, 2.0, 1.0] and r.reshape(-1).tolist() == [0.0, -1.0, -2.0, -4.0] and d.reshape(-1).tolist() == [0.0, 0.0, 1.0, 1.0]
    assert rows.get_size() == len(rows) == 4

    both = ReplayRows(S)
    assert both.get_size() == 0 and [tuple(t.shape) for t in both.get_all()] == [(0, S), (0, 1), (0, S), (0, 1), (0, 1)]
    both.merge_buffer(rows)
    both.merge_buffer(ReplayRows(S))                                            # an empty buffer adds nothing
    other = ReplayRows(S, np.full((2, S), 7.0), [1, 0], np.full((2, S), 8.0), [0.5, 0.25], [0, 1])
    both.merge_buffer(other)
    s, a, s2, r, d = both.get_all()
    assert both.get_size() == 6 and tuple(s.shape) == (6, S) and tuple(r.shape) == (6, 1)
    assert np.array_equal(s[:4].numpy(), rows.get_all()[0].numpy()) and np.array_equal(s[4:].numpy(), np.full((2, S), 7.0, np.float32))
    assert r.reshape(-1).tolist() == [0.0, -1.0, -2.0, -4.0, 0.5, 0.25] and d.reshape(-1).tolist()[4:] == [0.0, 1.0]
    assert rows.get_size() == 4                                                 # the merged-in buffer is unchanged
    with pytest.raises(ValueError):
        both.merge_buffer(ReplayRows(S + 1, np.zeros((1, S + 1)), [0], np.zeros((1, S + 1)), [0], [0]))
    with pytest.raises(ValueError):
        ReplayRows(S, states=np.zeros((1, S)))


class _StubEnv(object):
    """What compare_env_output uses of an EnvWrapper over a VirtualEnv: next state = state + action, reward = 10 * action + state[0], never done."""

    def __init__(self, n_actions, same_action_num=1):
        self.n_actions, self.same_action_num, self.calls = n_actions, same_action_num, []

    def get_action_dim(self):
        return self.n_actions

    def step_population(self, actions, states, eps=None, worker=None, sign=None, repeat=1):
        assert actions.dtype == torch.int32 and tuple(actions.shape) == (states.shape[0],) and states.dtype == torch.float32
        assert eps is None and worker is None and sign is None
        self.calls.append((actions.clone(), repeat))
        a = actions.to(torch.float32)
        return states + a[:, None], 10.0 * a + states[:, 0], torch.zeros(states.shape[0])


def test_compare_env_output_on_a_stub_env():
    from learning_environments_amd.agents.rollout import ReplayRows
    from learning_environments_amd.experiments import histogram
    S = 2
    train = ReplayRows(S, np.zeros((5, S)), np.zeros(5), np.ones((5, S)), np.ones(5), np.zeros(5))
    states = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], np.float32)

    env2 = _StubEnv(2, same_action_num=3)
    test2 = ReplayRows(S, states, [0, 1, 1], states + 1, [1, 1, 1], [0, 0, 1])
    out = histogram.compare_env_output(env2, train, test2, "ddqn", rewards=[3.0])
    assert sorted(out) == sorted(["train", "test", "virt_next_states", "virt_rewards", "virt_dones", "virt_rewards_incorrect", "rewards", "agentname"])
    assert [tuple(t.shape) for t in out["train"]] == [(5, S), (5, 1), (5, S), (5, 1), (5, 1)]
    assert np.array_equal(out["test"][0].numpy(), states)
    assert np.array_equal(out["virt_next_states"].numpy(), states + np.array([[0.0], [1.0], [1.0]], np.float32))
    assert tuple(out["virt_rewards"].shape) == (3, 1) and out["virt_rewards"].reshape(-1).tolist() == [1.0, 13.0, 15.0]
    assert out["virt_rewards_incorrect"].reshape(-1).tolist() == [11.0, 3.0, 5.0]         # 1 - action
    assert tuple(out["virt_dones"].shape) == (3, 1) and out["rewards"] == [3.0]
    assert [c[0].tolist() for c in env2.calls] == [[0, 1, 1], [1, 0, 0]] and [c[1] for c in env2.calls] == [3, 3]

    env3 = _StubEnv(3)
    test3 = ReplayRows(S, states, [2, 0, 1], states + 1, [1, 1, 1], [0, 0, 1])
    out = histogram.compare_env_output(env3, train, test3, "duelingddqn")
    assert out["virt_rewards_incorrect"] is None and len(env3.calls) == 1                  # 1 - action is no action of a three-action env
    assert out["virt_rewards"].reshape(-1).tolist() == [21.0, 3.0, 15.0]
