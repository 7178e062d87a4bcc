"""BaseAgent.test as a call of its own (reference agents/base_agent.py:155-227) for DDQN / DuelingDDQN agents (`test_agents`), TD3 / PPO
agents (`test_actor_agents`, lenv_actor_test_population, csrc/actor_test_population.hip), TD3_discrete_vary agents
(`test_discrete_actor_agents`, lenv_td3d_test_population, csrc/discrete_actor_test_population.hip) that exist as parameter rows, and the
tabular agents (`test_tabular_agents`, lenv_ql_test_population, csrc/ql_test_population.hip) that exist as Q-tables.

The reference's agent.test(env) returns (reward_list, episode_length_list, replay_buffer); in the fused launches a test is only the closing part
of training and yields final_returns alone.  `test_agents` runs the test of a whole population in one launch of lenv_agent_test_population
(csrc/agent_test_population.hip) and hands every agent's triple back, the visited transitions as `ReplayRows` -- what the histogram / heatmap
scripts merge and read with get_all()."""
import numpy as np
import torch

from .. import engine
from ..config import TABULAR_AGENTS, ddqn_cfg_from_config, ppo_cfg_from_config, ql_cfg_from_config, td3_cfg_from_config, td3d_cfg_from_config


class ReplayRows(object):
    """The transitions of a rollout in visiting order: what the scripts use of the reference's ReplayBuffer (get_all, merge_buffer, get_size),
    append-only and without a capacity.  All five fields are CPU float32 tensors; rewards / dones are columns [N,1], actions [N,action_dim]
    (1, a discrete index, unless stated: the continuous envs' action vectors are up to six wide)."""
    FIELDS = ("states", "actions", "next_states", "rewards", "dones")

    def __init__(self, state_dim, states=None, actions=None, next_states=None, rewards=None, dones=None, action_dim=1):
        self.state_dim, self.action_dim = int(state_dim), int(action_dim)
        given = (states, actions, next_states, rewards, dones)
        if any(g is None for g in given) and not all(g is None for g in given):
            raise ValueError("ReplayRows takes all five fields or none")
        widths = self._widths()
        self._parts = []
        if states is not None:
            part = tuple(torch.as_tensor(np.asarray(g.cpu() if torch.is_tensor(g) else g), dtype=torch.float32).reshape(-1, w) for g, w in zip(given, widths))
            if len(set(p.shape[0] for p in part)) != 1:
                raise ValueError("ReplayRows: the five fields must have one row count")
            self._parts.append(part)

    def _widths(self):
        return (self.state_dim, self.action_dim, self.state_dim, 1, 1)

    def get_all(self):
        """(states [N,S], actions [N,action_dim], next_states [N,S], rewards [N,1], dones [N,1]), episode after episode and step after step."""
        if not self._parts:
            return tuple(torch.zeros((0, w), dtype=torch.float32) for w in self._widths())
        if len(self._parts) > 1:
            self._parts = [tuple(torch.cat([p[k] for p in self._parts]) for k in range(5))]
        return self._parts[0]

    def merge_buffer(self, other):
        """Append another buffer's rows behind this one's (ReplayBuffer.merge_buffer)."""
        rows = other.get_all()
        if rows[0].shape[1] != self.state_dim:
            raise ValueError("merge_buffer: state_dim %d next to %d" % (rows[0].shape[1], self.state_dim))
        if rows[1].shape[1] != self.action_dim:
            raise ValueError("merge_buffer: action_dim %d next to %d" % (rows[1].shape[1], self.action_dim))
        if rows[0].shape[0]:
            self._parts.append(tuple(torch.as_tensor(r, dtype=torch.float32).cpu().reshape(-1, w) for r, w in zip(rows, self._widths())))

    def get_size(self):
        return int(sum(p[0].shape[0] for p in self._parts))

    def make_one_hot_buffer(self):
        """ReplayBuffer.make_one_hot_buffer (utils.py:71-72): despite its name, the action VECTORS become their argmax (first maximum), an
        index column; action_dim is 1 afterwards."""
        s, a, s2, r, d = self.get_all()
        self._parts = [(s, torch.argmax(a, dim=1, keepdim=True).to(torch.float32), s2, r, d)] if self._parts else []
        self.action_dim = 1

    __len__ = get_size


def rows_of_episodes(state, action, next_state, reward, done, counts):
    """ReplayRows of one agent from padded per-episode arrays [T,cap(,S)] (host) and the rows each episode filled, counts [T]."""
    if state.ndim == 2:                                                               # [T,cap]: the state indices of a gridworld
        state, next_state = state[..., None], next_state[..., None]
    S = state.shape[-1]
    keep = np.arange(state.shape[1])[None, :] < np.asarray(counts)[:, None]          # [T,cap], row-major = episode after episode
    A = action.shape[-1] if action.ndim == 3 else 1                                   # [T,cap,A]: action vectors of a continuous env
    return ReplayRows(S, state[keep].astype(np.float32), action[keep].astype(np.float32), next_state[keep].astype(np.float32), reward[keep], done[keep],
                      action_dim=A)


def _device_i64(v, n, dev, name):
    if v is None:
        return None
    if torch.is_tensor(v):
        t = v.to(device=dev, dtype=torch.int64)
    else:
        a = np.asarray(v)
        a = a.view(np.int64) if a.dtype == np.uint64 else a.astype(np.int64)
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if t.dim() == 0:
        t = t.repeat(n)
    if tuple(t.shape) != (n,):
        raise ValueError("%s must have one entry per agent" % name)
    return t.contiguous()


def _test_overrides(test_episodes, max_steps):
    """the cfg_from_config overrides of the test_* functions: what is None keeps the config's value"""
    return {k: int(v) for k, v in (("test_episodes", test_episodes), ("max_steps", max_steps)) if v is not None}


def _triples(out):
    """the reference's (reward_list, episode_length_list, replay_buffer) per agent from a *_test_population result"""
    host = {k: v.cpu().numpy() for k, v in out.items()}
    return [(host["returns"][i].tolist(), host["agent_steps"][i].tolist(),
             rows_of_episodes(host["row_state"][i], host["row_action"][i], host["row_next_state"][i], host["row_reward"][i], host["row_done"][i],
                              host["agent_steps"][i]))
            for i in range(host["returns"].shape[0])]


def test_agents(config, params, rng_keys, episode_offset=None, test_episodes=None, max_steps=None):
    """agent.test(env=real_env) for every row of `params` (fp32 [agents,P], the layout of the fused loops' final_online for the agent
    `config` selects: config['agents']['gtn']['agent_name'], default ddqn) on config's real env, in one launch.  rng_keys [agents] (uint64
    array or int64 tensor): episode e of agent i resets from the draw (rng_keys[i], test-reset stream, episode_offset[i] + e);
    episode_offset: one integer or one per agent.  test_episodes / max_steps override the config's.
    Returns, per agent, the reference's triple (reward_list, episode_length_list, replay_buffer): the T episode returns, the T episode
    lengths counted in agent steps (BaseAgent.test adds 1 per action, base_agent.py:213), and the visited transitions as ReplayRows."""
    dev = engine.require_device()
    over = _test_overrides(test_episodes, max_steps)
    cfg = ddqn_cfg_from_config(config, **over)
    params = torch.as_tensor(params, dtype=torch.float32).to(dev).contiguous()
    n = params.shape[0]
    out = engine.agent_test_population(cfg, params, _device_i64(rng_keys, n, dev, "rng_keys"), _device_i64(episode_offset, n, dev, "episode_offset"))
    return _triples(out)


test_agents.__test__ = False      # a library function, not a pytest case


def test_actor_agents(config, params, rng_keys, episode_offset=None, test_episodes=None, max_steps=None):
    """test_agents for the continuous-control agents: agent.test(env=real_env) for every row of `params` (fp32 [agents,P], the layout of the
    fused loops' final_params) on config's real env (the HalfCheetah stand-in, Pendulum-v0, MountainCarContinuous-v0), in one launch of
    lenv_actor_test_population.  The agent is config['agents']['gtn']['agent_name']: td3, td3_vary with vary_hp off (the agent IS TD3 then),
    or ppo; anything else -- td3_discrete_vary (a Gumbel-softmax actor: test_discrete_actor_agents), td3_vary with vary_hp on (per-agent shapes: group the agents by
    drawn shape and call engine.actor_test_population per group), the Q-net agents (test_agents) and the gridworld agents
    (test_tabular_agents) -- raises
    NotImplementedError naming it.  The test actions carry the noise of the fused loops' closing test, drawn from the counter RNG:
    (rng_keys[i], the agent's test-noise stream, episode_offset[i] + e, agent step); the resets as in test_agents.
    Returns, per agent, the reference's triple (reward_list, episode_length_list, replay_buffer); the ReplayRows carry action vectors
    (action_dim = the env's)."""
    name = config["agents"]["gtn"]["agent_name"].lower() if "gtn" in config["agents"] else "td3"
    if name == "td3_vary" and not config["agents"]["td3_vary"]["vary_hp"]:
        name = "td3"
    if name == "td3_vary":
        raise NotImplementedError("test_actor_agents: agent '%s' with vary_hp on draws a shape per agent; group the agents by shape and call "
                                  "engine.actor_test_population per group" % config["agents"]["gtn"]["agent_name"])
    if name not in ("td3", "ppo"):
        raise NotImplementedError("test_actor_agents: agent '%s' (TD3 and PPO actors of one shape only)" % config["agents"].get("gtn", {}).get("agent_name", name))
    dev = engine.require_device()
    over = _test_overrides(test_episodes, max_steps)
    cfg = (td3_cfg_from_config if name == "td3" else ppo_cfg_from_config)(config, **over)
    params = torch.as_tensor(params, dtype=torch.float32).to(dev).contiguous()
    n = params.shape[0]
    out = engine.actor_test_population(name, cfg, params, _device_i64(rng_keys, n, dev, "rng_keys"), _device_i64(episode_offset, n, dev, "episode_offset"))
    return _triples(out)


test_actor_agents.__test__ = False


def test_discrete_actor_agents(config, params, rng_keys, learn_calls=None, episode_offset=None, test_episodes=None, max_steps=None):
    """test_actor_agents for TD3_discrete_vary with vary_hp off: agent.test(env=real_env) for every row of `params` (fp32 [agents,P], the
    layout of the fused loops' final_params) on config's real env (CartPole-v0, Acrobot-v1, MountainCar-v0), in one launch of
    lenv_td3d_test_population.  learn_calls (one integer or one per agent, None = 0): the learn calls the agent has made -- column 2 of a
    fused launch's stats -- which set the annealed Gumbel-softmax temperature.  The test actions carry the Gumbel and Gaussian draws of the
    fused loops' closing test: (rng_keys[i], the stream, episode_offset[i] + e, step); the resets as in test_agents.  With vary_hp on every
    agent has its own shape: NotImplementedError naming it (group the agents by shape and call engine.td3d_test_population per group).
    Returns, per agent, the reference's triple (reward_list, episode_length_list, replay_buffer); the ReplayRows carry the action VECTORS
    (action_dim = the env's action count; make_one_hot_buffer turns them into indices)."""
    name = config["agents"]["gtn"]["agent_name"].lower() if "gtn" in config["agents"] else "td3_discrete_vary"
    if name != "td3_discrete_vary":
        raise NotImplementedError("test_discrete_actor_agents: agent '%s' (TD3_discrete_vary only)" % config["agents"]["gtn"]["agent_name"])
    if config["agents"]["td3_discrete_vary"]["vary_hp"]:
        raise NotImplementedError("test_discrete_actor_agents: agent '%s' with vary_hp on draws a shape per agent; group the agents by shape and "
                                  "call engine.td3d_test_population per group" % config["agents"].get("gtn", {}).get("agent_name", name))
    dev = engine.require_device()
    over = _test_overrides(test_episodes, max_steps)
    cfg = td3d_cfg_from_config(config, **over)
    params = torch.as_tensor(params, dtype=torch.float32).to(dev).contiguous()
    n = params.shape[0]
    out = engine.td3d_test_population(cfg, params, _device_i64(rng_keys, n, dev, "rng_keys"), _device_i64(episode_offset, n, dev, "episode_offset"),
                                      _device_i64(learn_calls, n, dev, "learn_calls"))
    return _triples(out)


test_discrete_actor_agents.__test__ = False


def test_tabular_agents(config, q_tables, tables=None, test_episodes=None, max_steps=None):
    """agent.test(env=real_env) for the tabular agents (config['agents']['gtn']['agent_name']: QL / QL_cb / SARSA / SARSA_cb -- they share
    select_test_action), every row of q_tables (fp64 [agents, n_states * n_actions], the q_table of the fused tabular launches) on the
    gridworld `tables` (GridEnv.tables: n_states, n_actions, start_state, next_state / reward / done; None: the gridworld config names), in
    one launch of lenv_ql_test_population.  Returns, per agent, the reference's triple (reward_list, episode_length_list, replay_buffer) with
    ReplayRows(state_dim=1): states, actions and next states are indices."""
    name = config["agents"]["gtn"]["agent_name"].lower() if "gtn" in config["agents"] else "ql"
    if name not in TABULAR_AGENTS:
        raise NotImplementedError("test_tabular_agents: agent '%s' (the tabular agents: %s)" % (config["agents"]["gtn"]["agent_name"], ", ".join(TABULAR_AGENTS)))
    if tables is None:
        from ..envs.env_factory import EnvFactory
        tables = EnvFactory(config=config).generate_real_env().env.tables
    over = _test_overrides(test_episodes, max_steps)
    cfg = ql_cfg_from_config(config, tables, **over)
    dev = engine.require_device()
    q = torch.as_tensor(q_tables, dtype=torch.float64).to(dev).contiguous()
    out = engine.ql_test_population(cfg, q.reshape(q.shape[0], -1), tables)
    return _triples(out)


test_tabular_agents.__test__ = False
