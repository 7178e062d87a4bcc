"""The state / reward histogram experiment (reference experiments/GTNC_visualize_cartpole_histogram.py and
GTNC_visualize_acrobot_histogram.py), without the plotting: which states and rewards do agents see while they train on the synthetic env,
which on the real env when they are tested, and what does the synthetic env answer on the real env's (state, action) pairs.

    load_envs_and_config(dir, file_name) -> (virtual_env, real_env, config)
    collect(virtual_env, real_env, config, agent_name, agents_num=10, seed=0) -> compare_env_output(...)'s dict
    compare_env_output(virtual_env, replay_buffer_train_all, replay_buffer_test_all, agentname) -> dict

The scripts' loop -- agent.train(env=virtual_env), agent.test(env=real_env), merge both replay buffers -- runs here as two launches for all
agents: the fused inner loop with test_mode 1 (train without a test env) and a step trace, then agents/rollout.test_agents on the trained
parameter rows -- for the scripts' third agent, td3_discrete_vary, rollout.test_discrete_actor_agents, whose buffers hold action vectors and
go through make_one_hot_buffer before they are merged, as in the scripts.  The first user of BaseAgent.test's third return value."""
import copy

import numpy as np
import torch

from ..agents import tasks
from ..agents.nes_common import chain_keys, fresh_agent_init
from ..agents.rollout import ReplayRows, test_agents, test_discrete_actor_agents
from ..engine import HipNesEngine
from . import syn_env_evaluate

AGENTS = ("ddqn", "duelingddqn", "td3_discrete_vary")


def load_envs_and_config(dir, file_name):
    return syn_env_evaluate.load_envs_and_config(file_name, dir, "cuda")


def _on_device(t):
    return t.cuda() if torch.cuda.is_available() else t


def compare_env_output(virtual_env, replay_buffer_train_all, replay_buffer_test_all, agentname, rewards=None):
    """The synthetic env on the real env's data: one step_population call on every (state, action) the tested agents visited and, for
    two-action envs, one on (state, 1 - action) -- the scripts' "incorrect" reward.  With three actions 1 - action is no action (the
    Acrobot script computes it all the same); virt_rewards_incorrect is None there.  Returns what the scripts plot: dict(train, test = the
    buffers' get_all() tuples, virt_next_states [N,S], virt_rewards / virt_dones / virt_rewards_incorrect [N,1], rewards)."""
    train = replay_buffer_train_all.get_all()
    test = replay_buffer_test_all.get_all()
    states, actions = test[0], test[1]
    repeat = max(1, int(getattr(virtual_env, "same_action_num", 1)))
    s_dev = _on_device(states.contiguous())
    a_dev = _on_device(actions.reshape(-1).to(torch.int32).contiguous())

    def step(act):
        ns, r, d = virtual_env.step_population(act, s_dev, repeat=repeat)
        return ns.cpu().reshape(states.shape), r.cpu().reshape(-1, 1), d.cpu().reshape(-1, 1)

    virt_next_states, virt_rewards, virt_dones = step(a_dev)
    virt_rewards_incorrect = step(1 - a_dev)[1] if virtual_env.get_action_dim() == 2 else None
    return dict(train=train, test=test, virt_next_states=virt_next_states, virt_rewards=virt_rewards, virt_dones=virt_dones,
                virt_rewards_incorrect=virt_rewards_incorrect, rewards=rewards, agentname=agentname)


def collect(virtual_env, real_env, config, agent_name, agents_num=10, seed=0):
    """The scripts' main block for agent_name in AGENTS: `agents_num` fresh agents (config['agents'][agent_name]) train on the synthetic env
    as the chains of one fused launch, are tested on the real env by test_agents, and the merged buffers go through compare_env_output.
    `seed` keys the agents' counter-RNG streams (the scripts seed the global generators from the clock).  collect.last holds the inner loop,
    the keys and the per-agent triples of the test."""
    key = agent_name.lower()
    if key not in AGENTS:
        raise NotImplementedError("histogram.collect: agent '%s' (built: %s)" % (agent_name, ", ".join(AGENTS)))
    if not virtual_env.is_virtual_env() or real_env.is_virtual_env():
        raise ValueError("collect(virtual_env, real_env, ...): a synthetic env to train on and the real env to test on")
    cfg_dict = copy.deepcopy(config)
    cfg_dict["agents"]["gtn"] = dict(cfg_dict["agents"].get("gtn", {}), agent_name=key, synthetic_env_type=0)
    engine = HipNesEngine()
    dev = engine.device
    n = int(agents_num)
    task = tasks.select_task(cfg_dict, engine, virtual_env, test_mode=1)
    cfg = task.cfg
    discrete_actor = key == "td3_discrete_vary"
    if discrete_actor and task.vary:
        raise NotImplementedError("histogram.collect: agent '%s' with vary_hp on draws a shape per agent" % agent_name)
    k_rep = 1 if discrete_actor else max(1, cfg.same_action_num)
    trace_cap = max(1, cfg.train_episodes * ((cfg.max_steps + k_rep - 1) // k_rep))         # every agent step of the longest possible run
    if discrete_actor:
        inner = engine.make_inner_td3d(cfg, n, want_episode_stats=True, want_final_params=True, trace_cap=trace_cap)
    else:
        inner = engine.make_inner(cfg, n, want_episode_stats=True, want_final_online=True, trace_cap=trace_cap)
    keys = chain_keys(int(seed), 0, np.arange(n), np.zeros(n, np.int64))
    keys_t = torch.from_numpy(keys.view(np.int64)).to(dev)
    theta = virtual_env.env.flat_params()
    g = torch.Generator(device=dev)
    g.manual_seed(int(seed))
    agent_init = None if discrete_actor else fresh_agent_init(task.agent_bounds, n, g, dev)     # TD3_discrete_vary: drawn from the keys in scores()
    task.scores(inner, theta, torch.zeros((1, theta.numel()), dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                torch.zeros(n, dtype=torch.float32, device=dev), keys_t, agent_init)
    engine.check_status(inner)

    # agent.train's replay buffer: the step trace, agent after agent
    train_steps = inner.stats[:, 1].cpu().numpy()
    tr = {k: v.cpu().numpy() for k, v in inner.trace.items()}
    S = cfg.state_dim
    train_all, test_all = ReplayRows(S), ReplayRows(S)
    episode_len = inner.episode_len.cpu().numpy() if discrete_actor else None
    episodes_run = inner.stats[:, 0].cpu().numpy()
    for i in range(n):
        m = int(train_steps[i])
        if discrete_actor:
            # the trace holds the action vector, the state pair and the reward; an episode's last step is the done one unless the episode
            # ran into max_steps on the VirtualEnv, which knows no TimeLimit (base_agent.py:104-131)
            lens = episode_len[i, :int(episodes_run[i])]
            ends = np.cumsum(lens) - 1
            done = np.zeros(m, np.float32)
            done[ends[lens < cfg.max_steps]] = 1.0
            rows = ReplayRows(S, tr["state"][i, :m], tr["action"][i, :m], tr["next_state"][i, :m], tr["reward"][i, :m], done, action_dim=cfg.action_dim)
            rows.make_one_hot_buffer()
            train_all.merge_buffer(rows)
        else:
            train_all.merge_buffer(ReplayRows(S, tr["state"][i, :m], (tr["action"][i, :m] & 0xffff).astype(np.float32), tr["next_state"][i, :m],
                                              tr["reward_done"][i, :m, 0], tr["reward_done"][i, :m, 1]))

    # agent.test(env=real_env): test_mode 1 ran no test before the launch's closing one, so these are its episodes
    if discrete_actor:
        triples = test_discrete_actor_agents(cfg_dict, inner.final_params, keys_t, learn_calls=inner.stats[:, 2])
    else:
        triples = test_agents(cfg_dict, inner.final_online, keys_t)
    finals = inner.final_returns.cpu().numpy()
    rewards = []
    for i, (reward_list, _, rows) in enumerate(triples):
        assert reward_list == finals[i].tolist(), "agent %d: test returns %s next to the launch's final_returns %s" % (i, reward_list, finals[i].tolist())
        rewards.append(float(np.mean(reward_list)))
        if discrete_actor:
            rows.make_one_hot_buffer()
        test_all.merge_buffer(rows)
    virtual_env.set_agent_params(same_action_num=k_rep, gamma=float(cfg.gamma))
    collect.last = dict(inner=inner, keys=keys_t, triples=triples, cfg=cfg, config=cfg_dict)
    return compare_env_output(virtual_env, train_all, test_all, key, rewards=rewards)


collect.last = None
