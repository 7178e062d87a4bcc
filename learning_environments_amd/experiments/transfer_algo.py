"""Reward-net transfer to an unseen agent: reward networks learned with TD3 are judged by how fast a PPO agent learns on them.

Mirrors the two functions of experiments/GTNC_evaluate_cmc_transfer_algo.py:60-128 and its HalfCheetah sibling (same names, arguments in the
same order plus the env name, same return shapes):

    load_envs_and_config(model_file) -> (reward_env, real_env, config)
        reads a reference-format reward-net checkpoint {'model': state_dict, 'config': dict}; solved_reward is raised so that the early
        out never triggers, as the scripts do
    train_test_agents(mode, env, real_env, config, env_name) -> (rewards, episode_lengths)
        writes the script's "settings for comparability" block (PPO_SETTINGS, restated as data) into config['agents']['ppo'] IN PLACE like the
        reference, then for each of MODEL_AGENTS fresh PPO agents:  reward, episode_length, _ = agent.train(env=env, test_env=real_env)

    train_test_agents_icm(real_env, config, env_name) -> (rewards, episode_lengths)
        the same call with the scripts' mode '-1': `ppo_icm` agents (PPO with an Intrinsic Curiosity Module, engine.PpoIcmInnerLoop) on the real
        env; writes the scripts' ICM block (ICM_SETTINGS) into config['agents']['icm'] as well

and the scripts' drivers (:131-172), which take model files where the scripts read hpbandster logs:

    eval_models(mode, model_files) -> (reward_list, episode_length_list)      every model's MODEL_AGENTS agents, concatenated model by model
    eval_base(mode, model_file)    -> (reward_list, episode_length_list)      MODEL_NUM x MODEL_AGENTS agents on the real env of one model's config
    eval_icm(model_file)           -> (reward_list, episode_length_list)      mode '-1': MODEL_NUM x MODEL_AGENTS ppo_icm agents on that real env
    save_list(mode, config, reward_list, episode_length_list, save_dir)       best_transfer_algo<mode>.pt with the scripts' five keys

Here all agents of a call -- and, through train_test_agents_models / eval_models / eval_base, all models of a mode -- are the chains of ONE
launch of lenv_ppo_rn_inner_loop (episodes_per_launch None) or of one series of segment launches of lenv_ppo_rn_inner_loop_segment
(episodes_per_launch episodes each, same bits: docs/notebook_ppo_transfer.md).  The scripts disable the early out and train 3 000 x up to 200
(MountainCarContinuous) or 5 000 x 1 000 (HalfCheetah) agent steps per agent: one launch of that length could neither be bounded nor report
progress, so the drivers default to segments.  Modes: '0' = the real env (a RewardEnv of type 0: the real reward passes through), '1' / '2' /
'5' / '6' = reward envs of that reward_env_type.  Mode '-1' (ppo_icm, the curiosity baseline) has entry points of its own,
train_test_agents_icm and eval_icm (lenv_ppo_icm_inner_loop / _segment); train_test_agents, eval_models and eval_base keep refusing '-1';
eval_icm's segments have a measured length of their own, ICM_EPISODES_PER_LAUNCH.  Reading hpbandster logs is out of scope: the caller passes model
files."""
import copy
import os

import numpy as np
import torch

from . import transfer_common
from .. import _lib, configs
from ..agents import tasks
from ..agents.nes_common import fresh_agent_init, linear_init_bounds
from ..config import icm_layer_dims, ppo_icm_settings
from ..engine import HipNesEngine, PpoIcmInnerLoop
from ..envs.reward_env import RewardEnv

MODEL_NUM = 10             # models per mode (both scripts)
MODEL_AGENTS = 10          # agents per model (both scripts)
MODES = ("0", "1", "2", "5", "6")

# the "settings for comparability" blocks: GTNC_evaluate_cmc_transfer_algo.py:83-105, GTNC_evaluate_halfcheetah_transfer_algo.py:91-113
PPO_SETTINGS = {
    "MountainCarContinuous-v0": dict(test_episodes=1, train_episodes=3000, print_rate=100, init_episodes=0, update_episodes=10, ppo_epochs=80, gamma=0.99,
                                     lr=3e-4, vf_coef=1, ent_coef=0.01, eps_clip=0.2, rb_size=1000000, same_action_num=5, activation_fn="relu",
                                     hidden_size=64, hidden_layer=2, action_std=0.5, early_out_num=10, early_out_virtual_diff=0.02),
    "HalfCheetah-v3": dict(test_episodes=1, train_episodes=5000, print_rate=100, init_episodes=0, update_episodes=1, ppo_epochs=10, gamma=0.99, lr=1e-5,
                           vf_coef=1, ent_coef=0.001, eps_clip=0.2, rb_size=1000000, same_action_num=1, activation_fn="tanh", hidden_size=128,
                           hidden_layer=2, action_std=0.1, early_out_num=50, early_out_virtual_diff=0.02),
}
# the ICM blocks behind them (mode -1): GTNC_evaluate_cmc_transfer_algo.py:104-109, GTNC_evaluate_halfcheetah_transfer_algo.py:116-121
ICM_SETTINGS = {
    "MountainCarContinuous-v0": dict(beta=0.1, eta=0.01, feature_dim=32, hidden_size=128, lr=5e-4),
    "HalfCheetah-v3": dict(beta=0.05, eta=0.03, feature_dim=32, hidden_size=128, lr=1e-4),
}
# what the scripts set solved_reward to ("something big enough to prevent early out triggering")
SOLVED_REWARD = {"MountainCarContinuous-v0": 100000, "HalfCheetah-v3": 100000}
SCRIPT_DEFAULT = transfer_common.SCRIPT_DEFAULT  # episodes_per_launch: DEFAULT_EPISODES_PER_LAUNCH of the env
# Episodes per segment launch of the drivers: the largest of {1, 2, 5, 10, 20, 50, 100, 200} whose segment stays under about 2 s.  Measured on an MI355X
# (tools/bench_configs.py ppo_episode_time, profiles/ppo_episode_time.log; 10 models x 10 agents at PPO_SETTINGS, full-length episodes, one workgroup per
# chain, so a segment lasts as long as its slowest chain).  MountainCarContinuous: 0.0124 s per episode without a learn call, 0.10 to 0.13 s with one, a
# learn call every tenth episode of a chain: 50 episodes = 50 x 0.0124 + 5 x 0.103 = 1.1 s (100 would be 2.3 s).  HalfCheetah stand-in: 0.047 s per episode,
# a learn call in each: 20 episodes = 0.94 s (50 would be 2.4 s).  Splitting itself costs 0.1 to 0.7 ms per boundary (docs/notebook_ppo_transfer.md).
DEFAULT_EPISODES_PER_LAUNCH = {"MountainCarContinuous-v0": 50, "HalfCheetah-v3": 20}
# The same rule for eval_icm's chains, 10 x 10 ppo_icm agents on the real env (tools/bench_configs.py ppo_icm, profiles/ppo_icm_cost.log).
# MountainCarContinuous: 0.0060 s per episode without a learn call (no reward net to evaluate), 0.124 s with one, a call every tenth episode:
# 100 episodes = 100 x 0.0060 + 10 x 0.124 = 1.8 s (200 would be 3.7 s).  HalfCheetah stand-in: 0.048 s per episode, a call in each:
# 20 episodes = 0.96 s (50 would be 2.4 s).
ICM_EPISODES_PER_LAUNCH = {"MountainCarContinuous-v0": 100, "HalfCheetah-v3": 20}


def base_config(env_name):
    """The RewardEnv configuration of a continuous real env (the published reward-env YAML's values) with PPO as the inner agent; the `ppo`
    section is the caller's to fill (train_test_agents writes PPO_SETTINGS there)."""
    make = {"MountainCarContinuous-v0": configs.cmc_reward_env_td3, "HalfCheetah-v3": configs.halfcheetah_reward_env_td3,
            "Pendulum-v0": configs.pendulum_reward_env_td3}
    if env_name not in make:
        raise NotImplementedError("transfer_algo: real env '%s'" % env_name)
    cfg = make[env_name]()
    cfg["agents"]["gtn"]["agent_name"] = "ppo"
    return cfg


def load_envs_and_config(model_file):
    return transfer_common.load_envs_and_config(model_file, lambda env_name: SOLVED_REWARD.get(env_name, 100000))


def _task_config(mode, env, config):
    """(config of the launch, theta): the caller's config with PPO as the inner agent on a RewardEnv; mode '0' / the real env itself = a
    RewardEnv of type 0 whose network is never evaluated."""
    cfg = copy.deepcopy(config)
    cfg["agents"]["gtn"] = dict(cfg["agents"].get("gtn", {}), agent_name="ppo", synthetic_env_type=1)
    e = cfg["envs"][cfg["env_name"]]
    if str(mode) == "0" or not isinstance(env.env, RewardEnv):
        e["reward_env_type"] = 0
        return cfg, None
    if int(e["reward_env_type"]) != int(mode):
        raise ValueError("mode %s needs a reward env of reward_env_type %s, the model has %s" % (mode, mode, e["reward_env_type"]))
    return cfg, env.env.flat_params()


def train_test_agents(mode, env, real_env, config, env_name=None, agents_num=MODEL_AGENTS, seed=0, model_index=0, settings=None, details=False,
                      episodes_per_launch=None, on_segment=None):
    """Returns (rewards, episode_lengths): rewards[i] = the i-th agent's per-episode real-env test means (PPO.train's first return value),
    episode_lengths[i] = its training episode lengths.  `settings` overrides entries of the script's block (a reduced episode budget);
    `seed` / `model_index` key the agents' counter-RNG streams.  details=True: ((rewards, episode_lengths), launch) with launch = the dict of
    what ran (inner, task, keys, agent_init, theta, eps, worker, sign) for tests and benchmarks.  episodes_per_launch None: one launch; an
    integer (or SCRIPT_DEFAULT: the env's DEFAULT_EPISODES_PER_LAUNCH): a series of segment launches of that many episodes, after each of
    which on_segment(episodes_done, finished_count) is called (engine.PpoInnerLoop.run) -- the same results bit for bit."""
    results, launch = _launch(mode, [env], real_env, config, env_name, agents_num, seed, [model_index], settings, episodes_per_launch, on_segment)
    return (results[0], launch) if details else results[0]


def train_test_agents_models(mode, envs, real_env, config, env_name=None, agents_num=MODEL_AGENTS, seed=0, model_indices=None, settings=None,
                             details=False, episodes_per_launch=None, on_segment=None):
    """All models of a mode as ONE launch (or one series of segment launches: episodes_per_launch / on_segment as in train_test_agents):
    len(envs) * agents_num chains, chain (m, i) reading model m's reward net.  Returns
    [train_test_agents(mode, envs[m], ..., model_index=model_indices[m]) for m], bit for bit (details=True: that list and the launch)."""
    if model_indices is None:
        model_indices = list(range(len(envs)))
    results, launch = _launch(mode, list(envs), real_env, config, env_name, agents_num, seed, list(model_indices), settings, episodes_per_launch,
                              on_segment)
    return (results, launch) if details else results


def save_list(mode, config, reward_list, episode_length_list, save_dir, model_num=MODEL_NUM, model_agents=MODEL_AGENTS):
    """The scripts' result file save_dir/best_transfer_algo<mode>.pt: {'config', 'model_num', 'model_agents', 'reward_list',
    'episode_length_list'}.  Returns its path."""
    os.makedirs(save_dir, exist_ok=True)
    file_name = os.path.join(save_dir, 'best_transfer_algo' + str(mode) + '.pt')
    save_dict = {}
    save_dict['config'] = config
    save_dict['model_num'] = model_num
    save_dict['model_agents'] = model_agents
    save_dict['reward_list'] = reward_list
    save_dict['episode_length_list'] = episode_length_list
    torch.save(save_dict, file_name)
    return file_name


def eval_models(mode, model_files, save_dir=None, agents_num=MODEL_AGENTS, seed=0, settings=None, episodes_per_launch=SCRIPT_DEFAULT,
                on_segment=None):
    """The scripts' eval_models over the given model files (the scripts take the MODEL_NUM best of an hpbandster log): agents_num fresh PPO
    agents per model on that model's reward env, all models' agents as the chains of one series of segment launches.  Returns
    (reward_list, episode_length_list), concatenated model by model; with save_dir also writes save_list's file, with the config of the last
    model like the scripts.  The models of one call must have the same reward-net shapes and env settings (they come from one search)."""
    _check_mode(mode)
    loaded = [load_envs_and_config(f) for f in model_files]
    if not loaded:
        raise ValueError("eval_models: no model files")
    real_env, config = loaded[-1][1], loaded[-1][2]
    results = train_test_agents_models(mode, [l[0] for l in loaded], real_env, config, agents_num=agents_num, seed=seed, settings=settings,
                                       episodes_per_launch=episodes_per_launch, on_segment=on_segment)
    return _collect(mode, config, results, save_dir, len(loaded), agents_num)


def eval_base(mode, model_file, save_dir=None, model_num=MODEL_NUM, agents_num=MODEL_AGENTS, seed=0, settings=None,
              episodes_per_launch=SCRIPT_DEFAULT, on_segment=None):
    """The scripts' eval_base: model_num times agents_num fresh PPO agents on the REAL env of model_file's config (the scripts load the best
    model model_num times and train on its real env), as the chains of one series of segment launches; repetition m keys its agents as model
    index m.  Returns (reward_list, episode_length_list); with save_dir also writes save_list's file."""
    _check_mode(mode)
    _, real_env, config = load_envs_and_config(model_file)
    results = train_test_agents_models(mode, [real_env] * int(model_num), real_env, config, agents_num=agents_num, seed=seed, settings=settings,
                                       episodes_per_launch=episodes_per_launch, on_segment=on_segment)
    return _collect(mode, config, results, save_dir, int(model_num), agents_num)


def _collect(mode, config, results, save_dir, model_num, agents_num):
    reward_list, episode_length_list = [], []
    for rewards, episode_lengths in results:
        reward_list += rewards
        episode_length_list += episode_lengths
    if save_dir is not None:
        save_list(mode, config, reward_list, episode_length_list, save_dir, model_num=model_num, model_agents=int(agents_num))
    return reward_list, episode_length_list


def train_test_agents_icm(real_env, config, env_name=None, agents_num=MODEL_AGENTS, seed=0, model_index=0, settings=None, icm=None, replay=None,
                          details=False, episodes_per_launch=None, on_segment=None):
    """The scripts' train_test_agents with mode '-1': agents_num fresh `ppo_icm` agents (PPO(icm=True)) on the real env, as the chains of one
    lenv_ppo_icm_inner_loop launch (or a series of segment launches).  Writes PPO_SETTINGS (then `settings`) into config['agents']['ppo'] and
    ICM_SETTINGS (then `icm`, entries to override) into config['agents']['icm'], in place like the scripts.  Every agent draws its module from
    stream 12 of its chain key.  replay: a recorded run of the reference -- dict(agent_init=[...], icm_init=[...], tapes=[{act_noise,
    test_noise, train_reset, test_reset} per agent]) -- replayed in tape mode.  Returns train_test_agents' shapes."""
    results, launch = _launch_icm(real_env, config, env_name, agents_num, seed, [model_index], settings, icm, episodes_per_launch, on_segment, replay)
    return (results[0], launch) if details else results[0]


def eval_icm(model_file, model_num=MODEL_NUM, agents_num=MODEL_AGENTS, seed=0, settings=None, icm=None, episodes_per_launch=SCRIPT_DEFAULT,
             on_segment=None, save_dir=None):
    """The scripts' eval_icm (mode '-1', the curiosity baseline the reward nets are compared against): model_num times agents_num fresh
    ppo_icm agents on the REAL env of model_file's config (a RewardEnv of type 0, as mode 0), all of them the chains of one series of segment
    launches; repetition m keys its agents as model index m.  Returns (reward_list, episode_length_list); with save_dir also writes
    save_list's file, best_transfer_algo-1.pt."""
    _, real_env, config = load_envs_and_config(model_file)
    results, _ = _launch_icm(real_env, config, None, agents_num, seed, list(range(int(model_num))), settings, icm, episodes_per_launch, on_segment)
    return _collect("-1", config, results, save_dir, int(model_num), agents_num)


def _check_mode(mode):
    mode = str(mode)
    if mode == "-1":
        raise NotImplementedError("mode -1 (ppo_icm: PPO with an Intrinsic Curiosity Module) runs through train_test_agents_icm / eval_icm")
    if mode not in MODES:
        raise NotImplementedError("transfer_algo: mode '%s' (built: %s)" % (mode, ", ".join(MODES)))
    return mode


def _apply_settings(real_env, config, env_name, settings, episodes_per_launch, defaults=DEFAULT_EPISODES_PER_LAUNCH):
    """The checks and in-place writes every launch starts with; returns (env_name, episodes_per_launch)."""
    env_name = env_name or config["env_name"]
    if env_name != config["env_name"]:
        raise ValueError("env_name '%s' does not match the config's '%s'" % (env_name, config["env_name"]))
    if env_name not in PPO_SETTINGS:
        raise NotImplementedError("transfer_algo: no transfer script for '%s' (there are: %s)" % (env_name, ", ".join(sorted(PPO_SETTINGS))))
    if real_env.is_virtual_env():
        raise ValueError("real_env must be the real environment")
    config['agents']['ppo'] = dict(PPO_SETTINGS[env_name], **(settings or {}))       # in place, like the scripts
    if episodes_per_launch is SCRIPT_DEFAULT:
        episodes_per_launch = defaults[env_name]
    return env_name, episodes_per_launch


def _fresh_agents(task, seed, model_indices, n_ag, dev):
    rows = []
    for mi in model_indices:
        g = torch.Generator(device=dev)
        g.manual_seed(int(seed) + 1000003 * int(mi))
        rows.append(fresh_agent_init(task.agent_bounds, n_ag, g, dev))
    return torch.cat(rows)


def _replay_rows(rows, M, dev):
    """[M * agents, ...] device tensor of per-agent recordings (padded with zeros to the longest), the same for every model"""
    rows = [np.asarray(r) for r in rows]
    full = np.zeros((len(rows), max(r.shape[0] for r in rows)) + rows[0].shape[1:], rows[0].dtype)
    for i, r in enumerate(rows):
        full[i, :r.shape[0]] = r
    return torch.from_numpy(np.tile(full, (M,) + (1,) * (full.ndim - 1))).to(dev)


def _launch_icm(real_env, config, env_name, agents_num, seed, model_indices, settings, icm, episodes_per_launch=None, on_segment=None, replay=None):
    env_name, episodes_per_launch = _apply_settings(real_env, config, env_name, settings, episodes_per_launch, ICM_EPISODES_PER_LAUNCH)
    unknown = set(icm or {}) - set(ICM_SETTINGS[env_name])
    if unknown:
        raise ValueError("icm: unknown entries %s (there are: %s)" % (sorted(unknown), ", ".join(sorted(ICM_SETTINGS[env_name]))))
    config['agents']['icm'] = dict(ICM_SETTINGS[env_name], **(icm or {}))            # in place, like the scripts
    M, n_ag = len(model_indices), int(agents_num)
    if replay is not None and not (len(replay["agent_init"]) == len(replay["icm_init"]) == len(replay["tapes"]) == n_ag):
        raise ValueError("replay: need %d recorded agents, modules and tape sets" % n_ag)
    cfg, _ = _task_config("0", real_env, config)
    engine = HipNesEngine()
    dev = engine.device
    task = tasks.PpoRnTask(cfg, engine)
    if replay is not None:
        task.cfg.rng_mode = _lib.RNG_TAPE
    chains = M * n_ag
    ic = ppo_icm_settings(cfg)
    inner = PpoIcmInnerLoop(task.cfg, chains, ic, want_episode_stats=True)
    keys, keys_t = transfer_common.model_chain_keys(seed, model_indices, n_ag, dev)
    theta, eps, worker, sign = transfer_common.models_as_population(None, [], chains, n_ag, 1, dev)
    tapes = None
    if replay is None:
        agent_init = _fresh_agents(task, seed, model_indices, n_ag, dev)
        agent_init[:, :task.cfg.action_dim] = float(task.cfg.action_std)
        bounds = torch.from_numpy(linear_init_bounds(icm_layer_dims(task.cfg, ic["feature_dim"], ic["hidden_size"]))).to(dev)
        inner.draw_icm_init(keys_t, bounds)
    else:
        agent_init = _replay_rows(replay["agent_init"], M, dev).to(torch.float32)
        inner.icm_init.copy_(_replay_rows(replay["icm_init"], M, dev))
        tapes = {k: _replay_rows([t[k] for t in replay["tapes"]], M, dev) for k in _lib.PpoTapes.keys}
    inner.run(theta, eps, worker, sign, agent_init, rng_keys=keys_t, tapes=tapes, episodes_per_launch=episodes_per_launch, on_segment=on_segment)
    engine.check_status(inner)
    launch = dict(inner=inner, task=task, keys=keys, agent_init=agent_init, theta=theta, eps=eps, worker=worker, sign=sign)
    return transfer_common.inner_results(inner, n_ag), launch


def _launch(mode, envs, real_env, config, env_name, agents_num, seed, model_indices, settings, episodes_per_launch=None, on_segment=None):
    mode = _check_mode(mode)
    env_name, episodes_per_launch = _apply_settings(real_env, config, env_name, settings, episodes_per_launch)
    M, n_ag = len(envs), int(agents_num)
    cfg, theta = _task_config(mode, envs[0], config)
    engine = HipNesEngine()
    dev = engine.device
    task = tasks.select_task(cfg, engine, envs[0])
    chains = M * n_ag
    inner = task.make_inner(chains, want_episode_stats=True)
    keys, keys_t = transfer_common.model_chain_keys(seed, model_indices, n_ag, dev)
    p_theta = max(inner.p_theta, 1)
    others = lambda: [_task_config(mode, e, config)[1] for e in envs[1:]]
    theta, eps, worker, sign = transfer_common.models_as_population(theta, others, chains, n_ag, p_theta, dev)
    agent_init = _fresh_agents(task, seed, model_indices, n_ag, dev)
    if episodes_per_launch is None:
        task.scores(inner, theta, eps, worker, sign, keys_t, agent_init)
    else:
        agent_init[:, :task.cfg.action_dim] = float(task.cfg.action_std)            # what task.scores writes in front of its launch
        inner.run(theta, eps, worker, sign, agent_init, rng_keys=keys_t, episodes_per_launch=episodes_per_launch, on_segment=on_segment)
    engine.check_status(inner)
    launch = dict(inner=inner, task=task, keys=keys, agent_init=agent_init, theta=theta, eps=eps, worker=worker, sign=sign)
    return transfer_common.inner_results(inner, n_ag), launch
