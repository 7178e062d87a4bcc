"""The gridworld heatmap experiment (reference experiments/GTNC_evaluate_gridworld_heatmap.py) without the hpbandster log reading and
without plotting: SARSA agents are trained on a learned Cliff reward net, then tested on the real env; the states a tested agent visits are
the heatmap.  Same names, arguments in the same order plus what a library needs:

    load_envs_and_config(model_file, break_="solved") -> (reward_env, real_env, config)
        reads a reference-format reward-net checkpoint; solved_reward becomes -20 for "solved" (the early out may trigger) and 100000 for
        "end" (it never does), the script's BREAK switch
    train_test_agents(env, real_env, config, agents_num=10, seed=0, break_="solved") -> states
        writes the script's "settings for comparability" block (SARSA_FIXED plus the SARSA_FROM_QL keys copied from config['agents']['ql'])
        into a fresh config['agents']['sarsa'] IN PLACE like the reference, then for each fresh agent:
            reward, _, _ = agent.train(env=env, test_env=real_env); _, _, replay_buffer = agent.test(env=real_env)
        states[i] = the states of agent i's test buffer plus its last next state; with break_ "solved" the agents whose reward list has
        train_episodes entries (the env was not solved) are skipped
    eval_models(model_files, break_="solved", agents_num=10, seed=0) -> (config, state_list)
    save_list(config, state_list, file_name, mode, break_="solved", model_num=10, model_agents=10)

All agents of a call -- and, through eval_models, all models of a mode -- train as the chains of ONE launch of lenv_ql_rn_inner_loop_hp, the
way experiments/transfer_gridworld.py runs them, and are tested by agents/rollout.test_tabular_agents (lenv_ql_test_population) on the
launch's q_table rows."""
import torch

from . import transfer_common, transfer_gridworld
from ..agents import tasks
from ..agents.rollout import test_tabular_agents
from ..engine import HipNesEngine

MODEL_NUM = 10             # models per mode
MODEL_AGENTS = 10          # agents per model
BREAKS = ("solved", "end")
SOLVED_REWARD = {"solved": -20, "end": 100000}

# the "settings for comparability" block, GTNC_evaluate_gridworld_heatmap.py:71-86: three constants, the rest read from the QL section
SARSA_FIXED = dict(test_episodes=1, train_episodes=200, print_rate=100)
SARSA_FROM_QL = ("init_episodes", "batch_size", "alpha", "gamma", "eps_init", "eps_min", "eps_decay", "rb_size", "same_action_num", "early_out_num",
                 "early_out_virtual_diff")


def _check_break(break_):
    if break_ not in BREAKS:
        raise ValueError("break_ is 'solved' or 'end', not %r" % (break_,))


def load_envs_and_config(model_file, break_="solved"):
    _check_break(break_)
    return transfer_common.load_envs_and_config(model_file, SOLVED_REWARD[break_])


def sarsa_settings(config):
    """The script's settings block for this config, as a fresh dict"""
    return dict(SARSA_FIXED, **{k: config['agents']['ql'][k] for k in SARSA_FROM_QL})


def keep_agent(reward_list, train_episodes, break_):
    """The script's skip rule: with break_ "solved" an agent that used every training episode did not solve the env and is left out"""
    return not (len(reward_list) == train_episodes and break_ == "solved")


def states_of(rows):
    """The script's list for one tested agent: the visited states of its buffer plus the last next state"""
    state, _, next_state, _, _ = rows.get_all()
    states = [int(elem[0]) for elem in state.tolist()]
    states.append(int(next_state.tolist()[-1][0]))
    return states


def train_test_agents(env, real_env, config, agents_num=MODEL_AGENTS, seed=0, break_="solved", model_index=0, settings=None):
    """`settings` overrides entries of the block (a reduced episode budget); `seed` / `model_index` key the agents' counter-RNG streams.
    train_test_agents.last holds the launch (inner, keys, the test triples, the per-agent reward lists)."""
    return _run([env], real_env, config, agents_num, seed, break_, [model_index], settings)


def _run(envs, real_env, config, agents_num, seed, break_, model_indices, settings):
    _check_break(break_)
    if real_env.is_virtual_env() or any(e.is_virtual_env() for e in envs):
        raise ValueError("the heatmap script trains on a reward env and tests on the real env, not on a VirtualEnv")
    if not hasattr(real_env.env, "tables"):
        raise NotImplementedError("gridworld_heatmap: the real env must be a gridworld")
    config['agents']['sarsa'] = dict(sarsa_settings(config), **(settings or {}))                     # in place, like the script
    n_ag = int(agents_num)
    chains = len(envs) * n_ag
    mode = str(int(envs[0].env.reward_env_type))
    cfg, theta = transfer_gridworld._task_config(mode, envs[0], config, "algo")                    # select_agent(config, 'sarsa')
    engine = HipNesEngine()
    dev = engine.device
    tables = real_env.env.tables
    task = tasks.QlRnTask(cfg, engine, tables, test_mode=0)                                         # agent.train(env=env, test_env=real_env)
    inner = task.make_inner(chains, want_episode_stats=True)
    keys, keys_t = transfer_common.model_chain_keys(seed, model_indices, n_ag, dev)
    others = lambda: [transfer_gridworld._task_config(mode, e, config, "algo")[1] for e in envs[1:]]
    theta, eps, worker, sign = transfer_common.models_as_population(theta, others, chains, n_ag, max(inner.p_theta, 1), dev)
    inner.run(theta, eps, worker, sign, rng_keys=keys_t)
    engine.check_status(inner)
    rewards = [r for per_model in transfer_common.inner_results(inner, n_ag) for r in per_model[0]]
    triples = test_tabular_agents(cfg, inner.q_table, tables)                                      # agent.test(env=real_env)
    train_episodes = int(config['agents']['sarsa']['train_episodes'])
    states = [states_of(rows) for reward, (_, _, rows) in zip(rewards, triples) if keep_agent(reward, train_episodes, break_)]
    train_test_agents.last = dict(inner=inner, keys=keys, triples=triples, rewards=rewards, config=cfg)
    return states


train_test_agents.last = None


def eval_models(model_files, break_="solved", agents_num=MODEL_AGENTS, seed=0, settings=None):
    """All models of a mode (the caller passes the model files; the script reads them from an hpbandster log) in one launch.  Returns
    (config of the last model, state_list): what the script hands to save_list."""
    loaded = [load_envs_and_config(f, break_) for f in model_files]
    if not loaded:
        raise ValueError("eval_models: no model files")
    real_env, config = loaded[-1][1], loaded[-1][2]
    state_list = _run([l[0] for l in loaded], real_env, config, agents_num, seed, break_, list(range(len(loaded))), settings)
    return config, state_list


def save_list(config, state_list, file_name, mode, break_="solved", model_num=MODEL_NUM, model_agents=MODEL_AGENTS):
    """The script's dict, written to file_name"""
    torch.save(dict(config=config, model_num=model_num, model_agents=model_agents, mode=str(mode), **{"break": break_, "state_list": state_list}), file_name)
