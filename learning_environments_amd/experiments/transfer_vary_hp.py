"""Reward-net transfer across hyper-parameters: reward networks learned with TD3 are judged by TD3 agents that each draw their own
lr / batch_size / hidden_size / hidden_layer.

Mirrors three functions of experiments/GTNC_evaluate_cmc_transfer_vary_hp.py:62-175 and its HalfCheetah sibling (same names, the scripts'
arguments first, same return shapes):

    load_envs_and_config(model_file) -> (reward_env, real_env, config)
        reads a reference-format reward-net checkpoint {'model': state_dict, 'config': dict}; solved_reward is raised so that the early out
        never triggers, as the scripts do
    vary_hp(config, rng) -> config_mod
        a deep copy of config whose td3 section carries one draw of the scripts' four distributions (agents/vary.py: the ranges TD3_vary uses)
    train_test_agents(mode, env, real_env, config) -> (rewards, episode_lengths)
        writes the script's "settings for comparability" blocks (TD3_SETTINGS / ICM_SETTINGS, restated as data) into config['agents']['td3']
        / ['icm'] IN PLACE like the reference, then for each of MODEL_AGENTS fresh agents, each with its own draw:
        reward, episode_length, _ = agent.train(env=env, test_env=real_env)

Here all agents of a call -- and, through train_test_agents_models, all models of a mode -- are the chains of one series of segment launches
of lenv_td3_rn_inner_loop_segment (episodes_per_launch episodes each; None: one launch of lenv_td3_rn_inner_loop_icm).  The scripts disable the
early out and train 3 000 x up to 500 (MountainCarContinuous) or 1 000 x 1 000 (HalfCheetah) agent steps per agent: one launch of that length
could neither be bounded nor report progress.  Modes: '-1' = td3_icm on the real env, '0' = the real env (a RewardEnv of type 0: the real reward
passes through), otherwise the reward_env_type of the loaded model.  Reading hpbandster logs is out of scope: the caller passes model files."""
import copy

import numpy as np
import torch

from . import transfer_common
from .. import configs
from ..agents import tasks, vary
from ..engine import HipNesEngine
from ..envs.reward_env import RewardEnv

MODEL_NUM = 10             # models per mode (both scripts)
MODEL_AGENTS = 10          # agents per model (both scripts)

# the "settings for comparability" blocks: GTNC_evaluate_cmc_transfer_vary_hp.py:128-146, GTNC_evaluate_halfcheetah_transfer_vary_hp.py:146-164
TD3_SETTINGS = {
    "MountainCarContinuous-v0": dict(test_episodes=1, train_episodes=3000, print_rate=100, lr=3e-4, tau=0.005, activation_fn="relu", same_action_num=2,
                                     policy_delay=2, policy_std_clip=0.5, policy_std=0.2, action_std=0.1, batch_size=256, gamma=0.99, rb_size=1000000,
                                     init_episodes=50, early_out_num=10, early_out_virtual_diff=1e-2),
    "HalfCheetah-v3": dict(test_episodes=1, train_episodes=1000, print_rate=100, lr=3e-4, tau=0.005, activation_fn="relu", same_action_num=1,
                           policy_delay=2, policy_std_clip=0.5, policy_std=0.2, action_std=0.1, batch_size=256, gamma=0.99, rb_size=1000000,
                           init_episodes=20, early_out_num=50, early_out_virtual_diff=0.02),
}
# the "optimized ICM HPs" the scripts leave switched on (:149-154 / :175-180)
ICM_SETTINGS = {
    "MountainCarContinuous-v0": dict(beta=0.1, eta=0.01, feature_dim=32, hidden_size=128, lr=5e-4),
    "HalfCheetah-v3": dict(beta=0.001, eta=0.1, feature_dim=32, hidden_size=128, lr=1e-5),
}
SOLVED_REWARD = 100000     # "something big enough to prevent early out triggering"
SCRIPT_DEFAULT = transfer_common.SCRIPT_DEFAULT  # episodes_per_launch: DEFAULT_EPISODES_PER_LAUNCH of the env
# Episodes per segment launch.  Measured on an MI355X (tools/bench_configs.py td3_episode_time, profiles/td3_episode_time.log; one workgroup per chain, so
# the time of a segment is the time of its slowest chain): a full-length learning episode of the slowest drawable chain (384 x 3, batch 768) takes 13.0 s
# on MountainCarContinuous (500 agent steps) and 26.3 s on the HalfCheetah stand-in (1 000 steps); the nominal chain (128 x 2, batch 256) 0.42 s / 0.91 s.
# A segment on the order of ten seconds is therefore ONE episode on both envs.  A caller whose agents are all near the nominal shape (hps=) can pass
# 20 / 10 for the same ten seconds; splitting itself costs nothing measurable (6 segments: 0.9997 of the single launch's time).
DEFAULT_EPISODES_PER_LAUNCH = {"MountainCarContinuous-v0": 1, "HalfCheetah-v3": 1}


def base_config(env_name):
    """The RewardEnv configuration of a continuous real env (the published reward-env YAML's values); train_test_agents writes the scripts'
    blocks into its td3 / icm sections."""
    make = {"MountainCarContinuous-v0": configs.cmc_reward_env_td3, "HalfCheetah-v3": configs.halfcheetah_reward_env_td3}
    if env_name not in make:
        raise NotImplementedError("transfer_vary_hp: real env '%s'" % env_name)
    return make[env_name]()


def load_envs_and_config(model_file):
    return transfer_common.load_envs_and_config(model_file, SOLVED_REWARD)


def vary_hp(config, rng):
    """One draw of the scripts' ConfigurationSpace around config's td3 section (lr log-uniform in [lr / 3, 3 lr], batch_size and hidden_size
    log-uniform integers in [int(x / 3), int(3 x)], hidden_layer uniform in [l - 1, l + 1]); rng: a numpy RandomState (four uniforms, in
    ConfigSpace's alphabetical order of the names)."""
    sample = vary.vary_hyperparameters(config['agents']['td3'], [float(rng.random_sample()) for _ in vary.HP_ORDER])
    config_mod = copy.deepcopy(config)
    config_mod['agents']['td3'].update(sample)
    return config_mod


def apply_settings(config, env_name, settings=None):
    """The scripts' in-place writes: the td3 block (then `settings`, a caller's reduced budget) and the ICM block."""
    config['agents']['td3'].update(TD3_SETTINGS[env_name])
    config['agents']['td3'].update(settings or {})
    config['agents']['icm'] = dict(ICM_SETTINGS[env_name])
    return config


def _replay_tapes(replay, cfg, n_ag, M, dev):
    """Device tapes [chains, rows, ...] from the per-agent recordings of a fixture (zero rows behind each: the closing test, which the scripts do
    not run, draws from them)."""
    from .._lib import TD3_TAPE_KEYS
    nag = -(-cfg.max_steps // max(1, cfg.same_action_num))
    extra = {"test_reset": cfg.test_episodes, "test_noise": cfg.test_episodes * nag}
    out = {}
    for k in TD3_TAPE_KEYS:
        rows = [np.asarray(t[k]) for t in replay["tapes"]]
        rows = [r.reshape(-1) if k == "replay_idx" else r.reshape(r.shape[0], -1) for r in rows]
        n = max(r.shape[0] for r in rows) + extra.get(k, 0)
        full = np.zeros((n_ag, n) + rows[0].shape[1:], rows[0].dtype)
        for i, r in enumerate(rows):
            full[i, :r.shape[0]] = r
        out[k] = torch.from_numpy(np.tile(full, (M,) + (1,) * (full.ndim - 1))).to(dev)
    return out


def _task_config(mode, env, config):
    """(config of the launch, theta)"""
    cfg = copy.deepcopy(config)
    cfg["agents"]["gtn"] = dict(cfg["agents"].get("gtn", {}), agent_name="td3_icm_vary" if mode == "-1" else "td3_vary", synthetic_env_type=1)
    e = cfg["envs"][cfg["env_name"]]
    if mode in ("-1", "0") or not isinstance(env.env, RewardEnv):
        e["reward_env_type"] = 0
        return cfg, None
    if int(e["reward_env_type"]) != int(mode):
        raise ValueError("mode %s needs a reward env of reward_env_type %s, the model has %s" % (mode, mode, e["reward_env_type"]))
    return cfg, env.env.flat_params()


def train_test_agents(mode, env, real_env, config, env_name=None, agents_num=MODEL_AGENTS, seed=0, model_index=0, settings=None, hps=None,
                      episodes_per_launch=SCRIPT_DEFAULT, details=False, on_segment=None, replay=None):
    """Returns (rewards, episode_lengths): rewards[i] = the i-th agent's per-episode real-env test means (TD3.train's first return value),
    episode_lengths[i] = its training episode lengths.  `settings` overrides entries of the script's td3 block (a reduced episode budget);
    `seed` / `model_index` key the agents' counter-RNG streams, from which every agent also draws its hyper-parameters unless `hps` (a list of
    {lr, batch_size, hidden_size, hidden_layer} per agent) gives them.  details=True: ((rewards, episode_lengths), launch).  replay (with hps): a recorded run of the reference -- dict(agent_init=[...],
    tapes=[{tape: rows} per agent], optional theta, icm_init=[...], icm={...} entries of the ICM block to override) -- replayed in tape mode."""
    results, launch = _launch(mode, [env], real_env, config, env_name, agents_num, seed, [model_index], settings, hps, episodes_per_launch, on_segment,
                              replay)
    return (results[0], launch) if details else results[0]


def train_test_agents_models(mode, envs, real_env, config, env_name=None, agents_num=MODEL_AGENTS, seed=0, model_indices=None, settings=None,
                             hps=None, episodes_per_launch=SCRIPT_DEFAULT, details=False, on_segment=None):
    """All models of a mode as the chains of ONE series of launches: chain (m, i) reads model m's reward net through its eps row.  Returns
    [train_test_agents(mode, envs[m], ..., model_index=model_indices[m]) for m], bit for bit (hps: per agent, the same for every model)."""
    if model_indices is None:
        model_indices = list(range(len(envs)))
    results, launch = _launch(mode, list(envs), real_env, config, env_name, agents_num, seed, list(model_indices), settings, hps,
                              episodes_per_launch, on_segment)
    return (results, launch) if details else results


def _launch(mode, envs, real_env, config, env_name, agents_num, seed, model_indices, settings, hps, episodes_per_launch, on_segment, replay=None):
    mode = str(mode)
    env_name = env_name or config["env_name"]
    if env_name != config["env_name"]:
        raise ValueError("env_name '%s' does not match the config's '%s'" % (env_name, config["env_name"]))
    if env_name not in TD3_SETTINGS:
        raise NotImplementedError("transfer_vary_hp: no transfer script for '%s' (there are: %s)" % (env_name, ", ".join(sorted(TD3_SETTINGS))))
    if real_env.is_virtual_env():
        raise ValueError("real_env must be the real environment")
    apply_settings(config, env_name, settings)                                     # in place, like the scripts
    if replay is not None:
        if hps is None:
            raise ValueError("replay needs the recorded hps")
        config['agents']['icm'].update(replay.get("icm", {}))
    if episodes_per_launch is SCRIPT_DEFAULT:
        episodes_per_launch = DEFAULT_EPISODES_PER_LAUNCH[env_name]
    M, n_ag = len(envs), int(agents_num)
    cfg, theta = _task_config(mode, envs[0], config)
    engine = HipNesEngine()
    dev = engine.device
    task = tasks.Td3VaryTask(cfg, engine)
    if replay is not None:
        from .. import _lib
        task.cfg.rng_mode = _lib.RNG_TAPE
        if replay.get("theta") is not None and theta is not None:
            theta = torch.as_tensor(replay["theta"], dtype=torch.float32)
    chains = M * n_ag
    inner = task.make_inner(chains, want_episode_stats=True)
    keys, keys_t = transfer_common.model_chain_keys(seed, model_indices, n_ag, dev)
    if hps is not None:
        if len(hps) != n_ag:
            raise ValueError("hps: need %d entries, one per agent" % n_ag)
        task.fixed_hp = [dict(h) for h in hps] * M
    p_theta = max(inner.p_theta, 1)
    others = lambda: [_task_config(mode, e, config)[1] for e in envs[1:]]
    theta, eps, worker, sign = transfer_common.models_as_population(theta, others, chains, n_ag, p_theta, dev)
    task._fresh_agents(inner, keys_t)               # the draws (or hps), fresh agents at every chain's own shapes, fresh ICMs
    tapes = None
    if replay is not None:                          # the recorded agents (and ICMs) instead of fresh ones, the recorded draws instead of the chains' own
        transfer_common.replay_agents(inner, replay, n_ag, M, dev)
        tapes = _replay_tapes(replay, task.cfg, n_ag, M, dev)
    inner.run(theta, eps, worker, sign, None, rng_keys=keys_t, tapes=tapes, episodes_per_launch=episodes_per_launch, on_segment=on_segment)
    engine.check_status(inner)
    launch = dict(inner=inner, task=task, keys=keys, hps=task.last_hp, theta=theta, eps=eps, worker=worker, sign=sign)
    return transfer_common.inner_results(inner, n_ag), launch
