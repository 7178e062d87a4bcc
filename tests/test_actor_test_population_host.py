"""lenv_actor_test_population without a device: the two symbols, the unchanged ABI housekeeping, every refusal of the entry (the checks run
before any launch, so agents = 0 and host pointers do), lenv_actor_test_rows_cap, and the host-side pieces above it: engine.actor_test_num_params,
the refusals of rollout.test_actor_agents by agent name, and ReplayRows with action vectors."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

CHEETAH, PENDULUM, CMC = 2, 4, 5
TD3, PPO = 0, 1
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


def _cfg(kind, **over):
    """A cfg inside the envelope; only the fields the entry reads are set (training fields stay 0: they are ignored)."""
    from learning_environments_amd import _lib
    kw = dict(env_id=PENDULUM, state_dim=3, action_dim=1, max_steps=40, hidden=24, layers=2, act=1, test_episodes=3, same_action_num=1, action_std=0.5)
    if kind == TD3:
        kw.update(max_action=2.0, use_layer_norm=0)
    kw.update(over)
    return (_lib.Td3Cfg if kind == TD3 else _lib.PpoCfg)(**kw)


def _call(L, p, kind=TD3, cfg="auto", agents=0, rows="none", **ptrs):
    """The entry with dummy non-NULL host pointers; only calls that are refused or launch nothing (agents = 0) are made."""
    if isinstance(cfg, str):
        cfg = _cfg(kind)
    a = dict(params=p, rng_keys=p, episode_offset=None, reset_states=None, noise=None, returns=p, env_steps=p, agent_steps=p)
    a.update(ptrs)
    r = {"none": [None] * 5, "all": [p] * 5}[rows] if isinstance(rows, str) else rows
    return L.lenv_actor_test_population(kind, C.byref(cfg) if cfg is not None else None, a["params"], a["rng_keys"], a["episode_offset"], a["reset_states"],
                                        a["noise"], agents, a["returns"], a["env_steps"], a["agent_steps"], *r, None)


KINDS = pytest.mark.parametrize("kind", [TD3, PPO], ids=["td3", "ppo"])


def test_symbols_and_unchanged_abi(L):
    from learning_environments_amd import _lib
    for name in ("lenv_actor_test_population", "lenv_actor_test_rows_cap"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert (_lib.ACTOR_TD3, _lib.ACTOR_PPO) == (TD3, PPO)
    assert L.lenv_abi_version() == 7
    assert len(_lib.ABI_STRUCTS) == 17                  # functions only: no new struct
    assert L.lenv_struct_size(17) == -1
    assert len(_lib.SIGNATURES["lenv_actor_test_population"][1]) == 17
    assert len(_lib.SIGNATURES["lenv_actor_test_rows_cap"][1]) == 2


@KINDS
def test_no_agents_is_ok_after_the_checks(L, p, kind):
    assert _call(L, p, kind) == OK
    assert _call(L, p, kind, rows="all") == OK
    assert _call(L, p, kind, episode_offset=p, reset_states=p, noise=p) == OK
    # the far corner of each kind's envelope
    if kind == TD3:
        far = _cfg(TD3, env_id=CHEETAH, state_dim=17, action_dim=6, hidden=512, layers=3, use_layer_norm=1, test_episodes=30, same_action_num=64)
    else:
        far = _cfg(PPO, env_id=CHEETAH, state_dim=17, action_dim=6, hidden=128, layers=2, test_episodes=64, same_action_num=64)
    assert _call(L, p, kind, cfg=far) == OK
    assert _call(L, p, kind, cfg=_cfg(kind, env_id=CMC, state_dim=2, action_dim=1, layers=1, hidden=1, test_episodes=1, same_action_num=0)) == OK


@KINDS
@pytest.mark.parametrize("name", ["params", "rng_keys", "returns", "env_steps", "agent_steps"])
def test_null_required_pointer_is_invalid(L, p, kind, name):
    assert _call(L, p, kind, **{name: None}) == INVALID


@KINDS
def test_null_cfg_negative_agents_and_max_steps_are_invalid(L, p, kind):
    assert _call(L, p, kind, cfg=None) == INVALID
    assert _call(L, p, kind, agents=-1) == INVALID
    assert L.lenv_actor_test_rows_cap(kind, None) == INVALID
    assert _call(L, p, kind, cfg=_cfg(kind, max_steps=0)) == INVALID
    assert L.lenv_actor_test_rows_cap(kind, C.byref(_cfg(kind, max_steps=0))) == INVALID


@KINDS
@pytest.mark.parametrize("given", [(1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (1, 1, 1, 1, 0), (0, 1, 1, 1, 1), (1, 1, 0, 1, 1)])
def test_row_arrays_given_in_part_are_invalid(L, p, kind, given):
    assert _call(L, p, kind, rows=[p if g else None for g in given]) == INVALID


COMMON_OUTSIDE = [dict(env_id=0), dict(env_id=3), dict(env_id=-1), dict(env_id=CHEETAH), dict(env_id=CMC), dict(state_dim=2), dict(action_dim=6),
                  dict(hidden=0), dict(layers=0), dict(test_episodes=0), dict(act=PRELU), dict(act=5), dict(act=-1), dict(same_action_num=65),
                  dict(same_action_num=-1)]


@pytest.mark.parametrize("over", COMMON_OUTSIDE + [dict(hidden=513), dict(layers=4), dict(test_episodes=171),
                                                   dict(env_id=CHEETAH, state_dim=17, action_dim=6, test_episodes=31)])
def test_td3_outside_the_envelope_is_unsupported(L, p, over):
    cfg = _cfg(TD3, **over)
    assert _call(L, p, TD3, cfg=cfg) == UNSUPPORTED
    assert L.lenv_actor_test_rows_cap(TD3, C.byref(cfg)) == UNSUPPORTED


@pytest.mark.parametrize("over", COMMON_OUTSIDE + [dict(hidden=129), dict(layers=3), dict(test_episodes=65)])
def test_ppo_outside_the_envelope_is_unsupported(L, p, over):
    cfg = _cfg(PPO, **over)
    assert _call(L, p, PPO, cfg=cfg) == UNSUPPORTED
    assert L.lenv_actor_test_rows_cap(PPO, C.byref(cfg)) == UNSUPPORTED


@pytest.mark.parametrize("kind", [2, -1, 7])
def test_other_kinds_are_unsupported(L, p, kind):
    """TD3_discrete_vary and the gridworld agents have no kind."""
    cfg = _cfg(TD3)
    assert _call(L, p, kind, cfg=cfg) == UNSUPPORTED
    assert L.lenv_actor_test_rows_cap(kind, C.byref(cfg)) == UNSUPPORTED


def test_training_fields_are_not_read(L, p):
    """batch_size, the reward net, train_episodes, the ICM fields, PPO's update rule are whatever they are."""
    cfg = _cfg(TD3, batch_size=100000, rn_hidden=-7, rn_layers=99, train_episodes=-1, icm_enabled=1, icm_feature_dim=9999, test_mode=5, policy_delay=0,
               reward_env_type=55, virtual_env=3)
    assert _call(L, p, TD3, cfg=cfg) == OK and L.lenv_actor_test_rows_cap(TD3, C.byref(cfg)) == 40
    cfg = _cfg(PPO, rn_hidden=-7, rn_layers=99, train_episodes=-1, ppo_epochs=-3, update_episodes=float("nan"), reward_env_type=55, reserved=9)
    assert _call(L, p, PPO, cfg=cfg) == OK and L.lenv_actor_test_rows_cap(PPO, C.byref(cfg)) == 40


@KINDS
def test_rows_cap(L, kind):
    cap = lambda **kw: L.lenv_actor_test_rows_cap(kind, C.byref(_cfg(kind, **kw)))
    assert cap(max_steps=7, same_action_num=3) == 3
    assert cap(max_steps=200, same_action_num=1) == 200
    assert cap(max_steps=200, same_action_num=0) == 200
    assert cap(max_steps=40, same_action_num=64) == 1
    assert cap(max_steps=999, same_action_num=2) == 500


def test_num_params_matches_the_fused_entries(L):
    """engine.actor_test_num_params (network fields only) = lenv_td3_num_params / lenv_ppo_num_params on complete cfgs: the row width of
    final_params."""
    from learning_environments_amd import configs, engine
    from learning_environments_amd.config import ppo_cfg_from_config, td3_cfg_from_config
    for make, over in ((configs.halfcheetah_reward_env_td3, {}), (configs.pendulum_syn_env_td3, dict(hidden_layer=3, hidden_size=33, use_layer_norm=True)),
                       (configs.cmc_reward_env_td3, dict(hidden_layer=1, hidden_size=5, use_layer_norm=True))):
        c = make(2)
        c["agents"]["td3"].update(over)
        cfg = td3_cfg_from_config(c)
        assert engine.actor_test_num_params("td3", cfg) == L.lenv_td3_num_params(C.byref(cfg), None, None) > 0
    for over in ({}, dict(hidden_layer=1, hidden_size=5), dict(hidden_size=128)):
        cfg = ppo_cfg_from_config(configs.pendulum_reward_env_ppo(2, **over))
        assert engine.actor_test_num_params("ppo", cfg) == L.lenv_ppo_num_params(C.byref(cfg), None, None) > 0
    with pytest.raises(NotImplementedError):
        engine.actor_test_num_params("td3_discrete_vary", cfg)


@pytest.mark.parametrize("agent_name", ["TD3_discrete_vary", "DDQN", "QL", "td3_icm", "ppo_icm", "DuelingDDQN_vary"])
def test_test_actor_agents_refuses_other_agents_by_name(agent_name):
    from learning_environments_amd import configs
    from learning_environments_amd.agents.rollout import test_actor_agents
    c = configs.pendulum_reward_env_td3(2)
    c["agents"]["gtn"]["agent_name"] = agent_name
    with pytest.raises(NotImplementedError, match=agent_name):
        test_actor_agents(c, np.zeros((1, 8), np.float32), np.ones(1, np.uint64))


def test_test_actor_agents_refuses_td3_vary_with_vary_hp_on():
    from learning_environments_amd import configs
    from learning_environments_amd.agents.rollout import test_actor_agents
    c = configs.with_vary(configs.pendulum_reward_env_td3(2), vary_hp=True)
    with pytest.raises(NotImplementedError, match="td3_vary.*vary_hp"):
        test_actor_agents(c, np.zeros((1, 8), np.float32), np.ones(1, np.uint64))


def test_replay_rows_with_action_vectors():
    from learning_environments_amd.agents.rollout import ReplayRows, rows_of_episodes
    rng = np.random.RandomState(0)
    S, A = 17, 6
    parts = []
    for n in (3, 0, 5):
        parts.append(tuple(rng.standard_normal((n, w)).astype(np.float32) for w in (S, A, S, 1, 1)))
    merged = ReplayRows(S, action_dim=A)
    assert [tuple(t.shape) for t in merged.get_all()] == [(0, S), (0, A), (0, S), (0, 1), (0, 1)]
    for part in parts:
        rows = ReplayRows(S, *part, action_dim=A)
        assert rows.get_size() == part[0].shape[0]
        for got, want in zip(rows.get_all(), part):
            assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
        merged.merge_buffer(rows)
    assert len(merged) == 8
    for k, got in enumerate(merged.get_all()):
        assert np.array_equal(got.numpy(), np.concatenate([part[k] for part in parts]))
    # action_dim is checked like state_dim, and the default stays a column
    with pytest.raises(ValueError):
        merged.merge_buffer(ReplayRows(S))
    with pytest.raises(ValueError):
        ReplayRows(S).merge_buffer(merged)
    assert ReplayRows(S).action_dim == 1
    # padded per-episode arrays [T,cap,...] with action vectors
    T, cap = 2, 4
    st, ac, ns = rng.standard_normal((T, cap, S)).astype(np.float32), rng.standard_normal((T, cap, A)).astype(np.float32), rng.standard_normal((T, cap, S)).astype(np.float32)
    rw, dn = rng.standard_normal((T, cap)).astype(np.float32), np.zeros((T, cap), np.float32)
    rows = rows_of_episodes(st, ac, ns, rw, dn, [3, 1])
    s, a, s2, r, d = rows.get_all()
    assert rows.action_dim == A and tuple(a.shape) == (4, A) and np.array_equal(a.numpy(), np.concatenate([ac[0, :3], ac[1, :1]]))
    assert np.array_equal(s.numpy(), np.concatenate([st[0, :3], st[1, :1]])) and np.array_equal(r.numpy()[:, 0], np.concatenate([rw[0, :3], rw[1, :1]]))
