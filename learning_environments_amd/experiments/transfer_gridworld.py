"""Reward-net transfer on the gridworld: reward networks learned with QL are judged by how fast fresh tabular agents learn on them.

Mirrors the functions of experiments/GTNC_evaluate_gridworld_transfer_vary_hp.py:77-163 (script="vary_hp": QL agents, every one with its own
alpha and gamma drawn uniformly from [0.1, 1]) and experiments/GTNC_evaluate_gridworld_transfer_algo.py:74-126 (script="algo": SARSA, the
agent the nets were not trained with, at the script's fixed settings) -- same names, arguments in the same order plus what a library needs:

    load_envs_and_config(model_file) -> (reward_env, real_env, config)
        reads a reference-format reward-net checkpoint {'model': state_dict, 'config': dict}; solved_reward is raised so that the early out
        never triggers, as the scripts do
    vary_hp(config, units) -> the deep copy of config with the drawn alpha / gamma in config['agents']['ql'] (agents/vary.py: vary_tabular)
    train_test_agents(mode, env, real_env, config, script) -> (rewards, episode_lengths)
        writes the script's "settings for comparability" block (QL_SETTINGS / SARSA_SETTINGS, restated as data) into config['agents']['ql'] --
        or into a fresh config['agents']['sarsa'] -- IN PLACE like the reference, then for each of MODEL_AGENTS fresh agents:
        reward, episode_length, _ = agent.train(env=env, test_env=real_env)

Here all agents of a call -- and, through train_test_agents_models, all models of a mode -- are the chains of ONE launch of
lenv_ql_rn_inner_loop_hp, every chain with its own alpha / gamma (and, for reward types 1 / 2, its own shaped-reward table: the agent hands
gamma to the env).  Modes: '-1' = the count-based agent (ql_cb / sarsa_cb, beta 0.1) on the real env, '0' = QL / SARSA on the real env (a
RewardEnv of type 0: the real reward passes through), '1' / '2' / '5' / '6' = reward envs of that reward_env_type.  The variation lives in
the script, not in an agent name (the reference has no `ql_vary`), so select_task and the GTN master know nothing of it.  Reading hpbandster
logs is out of scope: the caller passes model files."""
import copy

import numpy as np
import torch

from . import transfer_common
from .. import _lib
from ..agents import tasks, vary
from ..engine import HipNesEngine
from ..envs.reward_env import RewardEnv

MODEL_NUM = 10             # models per mode (both scripts)
MODEL_AGENTS = 10          # agents per model (both scripts)
MODES = ("-1", "0", "1", "2", "5", "6")
SCRIPTS = ("vary_hp", "algo")

# the "settings for comparability" blocks: GTNC_evaluate_gridworld_transfer_vary_hp.py:130-149, GTNC_evaluate_gridworld_transfer_algo.py:93-113
QL_SETTINGS = dict(test_episodes=1, train_episodes=500, print_rate=100, alpha=1.0, eps_decay=0.0, eps_init=0.1, eps_min=0.1, gamma=0.8,
                   same_action_num=1, rb_size=1, init_episodes=0, batch_size=1, early_out_num=10, early_out_virtual_diff=0.02, beta=0.1)
SARSA_SETTINGS = dict(QL_SETTINGS, eps_init=0.01, eps_min=0.01)
SOLVED_REWARD = 100000     # "something big enough to prevent early out triggering"


def load_envs_and_config(model_file):
    return transfer_common.load_envs_and_config(model_file, SOLVED_REWARD)


def vary_hp(config, units):
    """The script's vary_hp with the two uniforms given (alpha's, then gamma's)."""
    sample = vary.vary_tabular(config['agents']['ql'], units)
    config_mod = copy.deepcopy(config)
    config_mod['agents']['ql']['alpha'] = sample['alpha']
    config_mod['agents']['ql']['gamma'] = sample['gamma']
    return config_mod


def agent_name_of(mode, script):
    """select_agent's name for a mode of a script: 'ql' / 'ql_cb', 'sarsa' / 'sarsa_cb'"""
    return ("ql" if script == "vary_hp" else "sarsa") + ("_cb" if str(mode) == "-1" else "")


def _task_config(mode, env, config, script):
    """(config of the launch, theta): the caller's config with the script's agent on a RewardEnv; modes '-1' / '0' = the real env itself = a
    RewardEnv of type 0 whose network is never evaluated."""
    cfg = copy.deepcopy(config)
    cfg["agents"]["gtn"] = dict(cfg["agents"].get("gtn", {}), agent_name=agent_name_of(mode, script), synthetic_env_type=1)
    e = cfg["envs"][cfg["env_name"]]
    if mode in ("-1", "0"):
        e["reward_env_type"] = 0
        return cfg, None
    if not isinstance(env.env, RewardEnv):
        raise ValueError("mode %s needs a reward env, got %s" % (mode, type(env.env).__name__))
    if int(env.env.reward_env_type) != int(mode) or int(e["reward_env_type"]) != int(mode):
        raise ValueError("mode %s needs a reward env of reward_env_type %s, the model has %s" % (mode, mode, env.env.reward_env_type))
    return cfg, env.env.flat_params()


def train_test_agents(mode, env, real_env, config, script="vary_hp", agents_num=MODEL_AGENTS, seed=0, model_index=0, settings=None, replay=None,
                      details=False):
    """Returns (rewards, episode_lengths): rewards[i] = the i-th agent's per-episode real-env test means (BaseAgent.train's first return value),
    episode_lengths[i] = its training episode lengths.  `settings` overrides entries of the script's block (a reduced episode budget); `seed` /
    `model_index` key the agents' counter-RNG streams and, for script="vary_hp", their alpha / gamma draws.  replay=dict(hp=[{alpha, gamma}] per
    agent or None, tapes=dict(eps_uniform=[...], rand_action=[...]) per agent): recorded draws replayed in tape mode.  details=True:
    ((rewards, episode_lengths), launch) with launch = the dict of what ran (inner, task, keys, hp, theta, eps, worker, sign)."""
    results, launch = _launch(mode, [env], real_env, config, script, agents_num, seed, [model_index], settings, replay)
    return (results[0], launch) if details else results[0]


def train_test_agents_models(mode, envs, real_env, config, script="vary_hp", agents_num=MODEL_AGENTS, seed=0, model_indices=None, settings=None,
                             replay=None, details=False):
    """All models of a mode as ONE launch: len(envs) * agents_num chains, chain (m, i) reading model m's reward net.  Returns
    [train_test_agents(mode, envs[m], ..., model_index=model_indices[m]) for m], bit for bit (details=True: that list and the launch).  A replay
    lists its chains model-major."""
    if model_indices is None:
        model_indices = list(range(len(envs)))
    results, launch = _launch(mode, list(envs), real_env, config, script, agents_num, seed, list(model_indices), settings, replay)
    return (results, launch) if details else results


def _tape_tensor(rows, dtype, dev):
    """ragged per-chain tapes -> one [chains, stride] device tensor (the kernel reports a chain that reads past its stride)"""
    stride = max([len(r) for r in rows] + [1])
    out = np.zeros((len(rows), stride), dtype)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return torch.from_numpy(out).to(dev)


def _launch(mode, envs, real_env, config, script, agents_num, seed, model_indices, settings, replay):
    mode = str(mode)
    if mode not in MODES:
        raise NotImplementedError("transfer_gridworld: mode '%s' (there are: %s)" % (mode, ", ".join(MODES)))
    if script not in SCRIPTS:
        raise NotImplementedError("transfer_gridworld: script '%s' (there are: %s)" % (script, ", ".join(SCRIPTS)))
    if real_env.is_virtual_env() or any(e.is_virtual_env() for e in envs):
        raise ValueError("the transfer scripts train on a reward env or the real env and test on the real env, not on a VirtualEnv")
    if not hasattr(real_env.env, "tables"):
        raise NotImplementedError("transfer_gridworld: the real env must be a gridworld")
    if script == "vary_hp":                                                      # in place, like the scripts
        config['agents']['ql'].update(dict(QL_SETTINGS, **(settings or {})))
    else:
        config['agents']['sarsa'] = dict(SARSA_SETTINGS, **(settings or {}))
    M, n_ag = len(envs), int(agents_num)
    chains = M * n_ag
    cfg, theta = _task_config(mode, envs[0], config, script)
    engine = HipNesEngine()
    dev = engine.device
    task = tasks.QlRnTask(cfg, engine, real_env.env.tables, test_mode=0)         # agent.train(env=env, test_env=real_env)
    tapes = None
    if replay is not None:
        task.cfg.rng_mode = _lib.RNG_TAPE
        if len(replay["tapes"]["eps_uniform"]) != chains or len(replay["tapes"]["rand_action"]) != chains:
            raise ValueError("replay: need the tapes of %d chains" % chains)
        tapes = dict(eps_uniform=_tape_tensor(replay["tapes"]["eps_uniform"], np.float64, dev),
                     rand_action=_tape_tensor(replay["tapes"]["rand_action"], np.int32, dev))
    inner = task.make_inner(chains, want_episode_stats=True)
    keys, keys_t = transfer_common.model_chain_keys(seed, model_indices, n_ag, dev)
    # every agent's own alpha / gamma: a recorded draw, or (the vary_hp script) vary_hp's on the chain key's STREAM_VARY_HP draws 0 and 1
    hp = None
    if replay is not None and replay.get("hp") is not None:
        hp = [dict(alpha=float(h["alpha"]), gamma=float(h["gamma"])) for h in replay["hp"]]
        if len(hp) != chains:
            raise ValueError("replay: need the alpha / gamma of %d chains" % chains)
    elif script == "vary_hp":
        hp = [vary_hp(config, vary.chain_units(k, 2))['agents']['ql'] for k in keys]
        hp = [dict(alpha=h["alpha"], gamma=h["gamma"]) for h in hp]
    if hp is not None:
        inner.set_hp([h["alpha"] for h in hp], [h["gamma"] for h in hp])
    p_theta = max(inner.p_theta, 1)
    others = lambda: [_task_config(mode, e, config, script)[1] for e in envs[1:]]
    theta, eps, worker, sign = transfer_common.models_as_population(theta, others, chains, n_ag, p_theta, dev)
    inner.run(theta, eps, worker, sign, rng_keys=keys_t, tapes=tapes)
    engine.check_status(inner)
    launch = dict(inner=inner, task=task, keys=keys, hp=hp, theta=theta, eps=eps, worker=worker, sign=sign)
    return transfer_common.inner_results(inner, n_ag), launch
