"""Reward-net transfer on CartPole: reward networks learned with DDQN are judged by DDQN agents that each draw their own
lr / batch_size / hidden_size / hidden_layer (script "vary_hp") and by DuelingDDQN agents at fixed settings (script "algo").

Mirrors three functions of experiments/GTNC_evaluate_cartpole_transfer_vary_hp.py:71-190 and of
experiments/GTNC_evaluate_cartpole_transfer_algo.py (same names, the scripts' arguments first, same return shapes):

    load_envs_and_config(model_file) -> (reward_env, real_env, config)
        reads a reference-format reward-net checkpoint {'model': state_dict, 'config': dict}; solved_reward is raised so that the early out
        never triggers, as the scripts do
    vary_hp(config, rng) -> config_mod                                                                      ("vary_hp" script only)
        a deep copy of config whose ddqn section carries one draw of the script's four distributions (agents/vary.py: the ranges DDQN_vary uses)
    train_test_agents(mode, env, real_env, config, script=...) -> (rewards, episode_lengths)
        writes the script's "settings for comparability" block (DDQN_SETTINGS / DUELING_SETTINGS) and its "optimized ICM HPs" (ICM_SETTINGS),
        restated as data, into config['agents'] IN PLACE like the reference, then for each of MODEL_AGENTS fresh agents:
        reward, episode_length, _ = agent.train(env=env, test_env=real_env)

Here all agents of a call -- and, through train_test_agents_models, all models of a mode -- are the chains of one series of segment launches
of lenv_dueling_se_inner_loop_segment (episodes_per_launch episodes each; None: one launch of lenv_dueling_se_inner_loop_icm).  The scripts
disable the early out and train 1 000 episodes of up to 200 steps per agent: one launch of that length could neither be bounded nor report
progress.  Modes: '-1' = the `_icm` agent on the real env, '0' = the real env (a RewardEnv of type 0: the real reward passes through),
otherwise the reward_env_type of the loaded model ('1', '2', '5', '6').  Reading hpbandster logs is out of scope: the caller passes model
files."""
import copy

import numpy as np
import torch

from . import transfer_common
from .. import _lib, configs
from ..agents import vary
from ..agents.nes_common import linear_init_bounds
from ..config import ddqn_cfg_from_config, icm_layer_dims
from ..engine import HipNesEngine, mlp_desc, mlp_num_params
from ..envs.reward_env import RewardEnv

ENV_NAME = "CartPole-v0"
MODEL_NUM = 10             # models per mode (both scripts)
MODEL_AGENTS = 10          # agents per model (both scripts)
SCRIPTS = ("vary_hp", "algo")
SECTION = {"vary_hp": "ddqn", "algo": "duelingddqn"}

# the "settings for comparability" blocks: GTNC_evaluate_cartpole_transfer_vary_hp.py:142-162, GTNC_evaluate_cartpole_transfer_algo.py (the same
# values in a duelingddqn section that the script creates EMPTY first, plus feature_dim)
DDQN_SETTINGS = dict(test_episodes=1, train_episodes=1000, print_rate=100, lr=0.00025, eps_init=1.0, eps_min=0.1, eps_decay=0.9, gamma=0.99,
                     batch_size=32, same_action_num=1, activation_fn="relu", tau=0.01, hidden_size=64, hidden_layer=1, rb_size=1000000,
                     init_episodes=1, early_out_num=10, early_out_virtual_diff=0.02)
DUELING_SETTINGS = dict(test_episodes=1, train_episodes=1000, print_rate=100, lr=0.00025, eps_init=1.0, eps_min=0.1, eps_decay=0.9, gamma=0.99,
                        batch_size=32, same_action_num=1, activation_fn="relu", tau=0.01, hidden_size=64, hidden_layer=1, rb_size=1000000,
                        init_episodes=1, feature_dim=128, early_out_num=10, early_out_virtual_diff=0.02)
# the "optimized ICM HPs" both scripts leave switched on
ICM_SETTINGS = dict(beta=0.05, eta=0.03, feature_dim=32, hidden_size=128, lr=1e-5)
SOLVED_REWARD = 100000     # "something big enough to prevent early out triggering"
SCRIPT_DEFAULT = transfer_common.SCRIPT_DEFAULT  # episodes_per_launch: DEFAULT_EPISODES_PER_LAUNCH of the script
# Episodes per segment launch.  Measured on an MI355X (tools/bench_configs.py dueling_episode_time, profiles/dueling_episode_time.log; one workgroup per
# chain, so a segment takes what its slowest chain takes): a full-length learning episode (200 agent steps, each with a learn step, and the 200-step
# test episode behind it) takes 0.0163 s at the vary_hp script's nominal chain (DDQN 64 x 1, batch 32) and 0.0671 s at the slowest chain its draw can
# give (192 x 2, batch 96); the algo script's DuelingDDQN chain (64 x 1, batch 32, feature_dim 128) takes 0.0575 s (0.1321 s at 192 x 2, batch 96,
# which that script never builds).  A segment on the order of ten seconds is therefore 10 / 0.0671 = 149 -> 150 episodes for vary_hp (2.4 s when
# every chain is nominal) and 10 / 0.0575 = 174 -> 175 for algo: 7 / 6 launches for the scripts' 1 000 episodes.  Splitting itself costs 0.34 ms per
# boundary, but the chains of a launch wait for the slowest one at every boundary (profiles/dueling_segments.log), so fewer, longer segments
# are the better default; mode -1's ICM (not timed) makes a segment longer, not wrong.
DEFAULT_EPISODES_PER_LAUNCH = {"vary_hp": 150, "algo": 175}


def base_config():
    """The RewardEnv configuration of CartPole (the published reward-env YAML's values); train_test_agents writes the scripts' blocks into its
    ddqn / duelingddqn / icm sections."""
    return configs.cartpole_reward_env_ddqn()


def load_envs_and_config(model_file):
    return transfer_common.load_envs_and_config(model_file, SOLVED_REWARD)


def vary_hp(config, rng):
    """One draw of the script's ConfigurationSpace around config's ddqn section (lr log-uniform in [lr / 3, 3 lr], batch_size and hidden_size
    log-uniform integers in [int(x / 3), int(3 x)], hidden_layer uniform in [l - 1, l + 1]: with the script's block 10..96 rows, 21..192 units,
    0..2 layers); rng: a numpy RandomState (four uniforms, in ConfigSpace's alphabetical order of the names)."""
    sample = vary.vary_hyperparameters(config['agents']['ddqn'], [float(rng.random_sample()) for _ in vary.HP_ORDER])
    config_mod = copy.deepcopy(config)
    config_mod['agents']['ddqn'].update(sample)
    return config_mod


def apply_settings(config, script, settings=None):
    """The scripts' in-place writes: the agent block (then `settings`, a caller's reduced budget) and the ICM block.  The algo script replaces
    the duelingddqn section by an empty one before it fills it; the vary_hp script writes into the ddqn section it finds."""
    if script == "algo":
        config['agents']['duelingddqn'] = {}
        config['agents']['duelingddqn'].update(DUELING_SETTINGS)
    else:
        config['agents']['ddqn'].update(DDQN_SETTINGS)
    config['agents'][SECTION[script]].update(settings or {})
    config['agents']['icm'] = dict(ICM_SETTINGS)
    return config


def _replay_tapes(replay, cfg, n_ag, M, dev):
    """Device tapes [chains, rows, ...] from the per-agent recordings of a fixture (zero rows behind each: the closing test, which the scripts do
    not run, draws its resets from them)."""
    extra = {"test_reset": cfg.test_episodes}
    out = {}
    for k in _lib.TAPE_KEYS:
        rows = [np.asarray(t[k]) for t in replay["tapes"]]
        rows = [r.reshape(-1, 4) if k.endswith("_reset") else r.reshape(-1) for r in rows]
        n = max(max(r.shape[0] for r in rows) + extra.get(k, 0), 1)
        full = np.zeros((n_ag, n) + rows[0].shape[1:], rows[0].dtype)
        for i, r in enumerate(rows):
            full[i, :r.shape[0]] = r
        out[k] = torch.from_numpy(np.tile(full, (M,) + (1,) * (full.ndim - 1))).to(dev)
    return out


def _task_config(mode, env, config, script):
    """(config of the launch, theta)"""
    cfg = copy.deepcopy(config)
    name = SECTION[script] + ("_icm" if mode == "-1" else "") + "_vary"       # per-chain hyper-parameter arrays for both scripts (algo: all equal)
    cfg["agents"]["gtn"] = dict(cfg["agents"].get("gtn", {}), agent_name=name, synthetic_env_type=1)
    e = cfg["envs"][cfg["env_name"]]
    if mode in ("-1", "0") or not isinstance(env.env, RewardEnv):
        e["reward_env_type"] = 0
        return cfg, None
    if int(e["reward_env_type"]) != int(mode):
        raise ValueError("mode %s needs a reward env of reward_env_type %s, the model has %s" % (mode, mode, e["reward_env_type"]))
    return cfg, env.env.flat_params()


def train_test_agents(mode, env, real_env, config, script="vary_hp", agents_num=MODEL_AGENTS, seed=0, model_index=0, settings=None, hps=None,
                      episodes_per_launch=SCRIPT_DEFAULT, details=False, on_segment=None, replay=None):
    """Returns (rewards, episode_lengths): rewards[i] = the i-th agent's per-episode real-env test means (the agent's train()'s first return
    value), episode_lengths[i] = its training episode lengths.  `settings` overrides entries of the script's agent block (a reduced episode
    budget); `seed` / `model_index` key the agents' counter-RNG streams, from which every agent of the vary_hp script also draws its
    hyper-parameters unless `hps` (a list of {lr, batch_size, hidden_size, hidden_layer} per agent) gives them; the algo script's agents all
    carry the block's own four values.  details=True: ((rewards, episode_lengths), launch).  replay (with hps): a recorded run of the
    reference -- dict(agent_init=[...], tapes=[{tape: rows} per agent], optional theta, icm_init=[...], icm={...} entries of the ICM block to
    override) -- replayed in tape mode."""
    results, launch = _launch(mode, [env], real_env, config, script, agents_num, seed, [model_index], settings, hps, episodes_per_launch, on_segment,
                              replay)
    return (results[0], launch) if details else results[0]


def train_test_agents_models(mode, envs, real_env, config, script="vary_hp", agents_num=MODEL_AGENTS, seed=0, model_indices=None, settings=None,
                             hps=None, episodes_per_launch=SCRIPT_DEFAULT, details=False, on_segment=None):
    """All models of a mode as the chains of ONE series of launches: chain (m, i) reads model m's reward net through its eps row.  Returns
    [train_test_agents(mode, envs[m], ..., model_index=model_indices[m]) for m], bit for bit (hps: per agent, the same for every model)."""
    if model_indices is None:
        model_indices = list(range(len(envs)))
    results, launch = _launch(mode, list(envs), real_env, config, script, agents_num, seed, list(model_indices), settings, hps,
                              episodes_per_launch, on_segment)
    return (results, launch) if details else results


def _launch(mode, envs, real_env, config, script, agents_num, seed, model_indices, settings, hps, episodes_per_launch, on_segment, replay=None):
    mode = str(mode)
    if script not in SCRIPTS:
        raise ValueError("script must be one of %s" % (SCRIPTS,))
    if config["env_name"] != ENV_NAME:
        raise NotImplementedError("transfer_cartpole: the scripts are CartPole-v0's (the config names '%s')" % config["env_name"])
    if real_env.is_virtual_env():
        raise ValueError("real_env must be the real environment")
    apply_settings(config, script, settings)                                       # in place, like the scripts
    if replay is not None:
        if hps is None:
            raise ValueError("replay needs the recorded hps")
        config['agents']['icm'].update(replay.get("icm", {}))
    if episodes_per_launch is SCRIPT_DEFAULT:
        episodes_per_launch = DEFAULT_EPISODES_PER_LAUNCH[script]
    M, n_ag = len(envs), int(agents_num)
    chains = M * n_ag
    cfgd, theta = _task_config(mode, envs[0], config, script)
    section = cfgd["agents"][SECTION[script]]
    engine = HipNesEngine()
    dev = engine.device
    keys, keys_t = transfer_common.model_chain_keys(seed, model_indices, n_ag, dev)
    own = {k: section[k] for k in ("lr", "batch_size", "hidden_size", "hidden_layer")}
    if hps is not None:
        if len(hps) != n_ag:
            raise ValueError("hps: need %d entries, one per agent" % n_ag)
        chain_hp = [dict(h) for h in hps] * M
    elif script == "algo":
        chain_hp = [dict(own) for _ in range(chains)]
    else:
        chain_hp = [vary.vary_hyperparameters(section, vary.chain_units(int(k))) for k in keys]
    # the launch is sized for the largest shapes among its chains' (workspace / LDS / row strides)
    big = copy.deepcopy(cfgd)
    big["agents"][SECTION[script]].update(batch_size=max(h["batch_size"] for h in chain_hp), hidden_size=max(h["hidden_size"] for h in chain_hp),
                                          hidden_layer=max(h["hidden_layer"] for h in chain_hp))
    cfg = ddqn_cfg_from_config(big, rng_mode=_lib.RNG_TAPE if replay is not None else _lib.RNG_COUNTER)
    cfg.grad_chunk = 0                                    # one sequential batch gradient (GEMM-tiled kernel)
    if replay is not None and replay.get("theta") is not None and theta is not None:
        theta = torch.as_tensor(replay["theta"], dtype=torch.float32)
    inner = engine.make_inner(cfg, chains, want_episode_stats=True, vary=True, segments=True)
    inner.set_hp([h["lr"] for h in chain_hp], [h["batch_size"] for h in chain_hp], [h["hidden_size"] for h in chain_hp],
                 [h["hidden_layer"] for h in chain_hp])
    # the kernel stages the reward net it is given: state_dim -> hidden -> 1, for type 0 RewardEnv.build_reward_net's 1-input dummy (never evaluated)
    p_theta = mlp_num_params(mlp_desc(1 if cfg.reward_env_type == 0 else cfg.state_dim, cfg.se_hidden, cfg.se_layers, 1, cfg.se_act))
    others = lambda: [_task_config(mode, e, config, script)[1] for e in envs[1:]]
    theta, eps, worker, sign = transfer_common.models_as_population(theta, others, chains, n_ag, p_theta, dev)
    if theta.numel() != p_theta:
        raise ValueError("the reward net has %d parameters, the config describes one of %d" % (theta.numel(), p_theta))
    inner.draw_agent_init(keys_t)                         # fresh agents at every chain's own shapes, fresh ICMs
    if inner.icm:
        inner.draw_icm_init(keys_t, torch.from_numpy(linear_init_bounds(icm_layer_dims(cfg))).to(dev))
    tapes = None
    if replay is not None:                                # the recorded agents (and ICMs) instead of fresh ones, the recorded draws instead of the chains' own
        transfer_common.replay_agents(inner, replay, n_ag, M, dev)
        tapes = _replay_tapes(replay, cfg, n_ag, M, dev)
    inner.run(theta, eps, worker, sign, None, rng_keys=keys_t, tapes=tapes, episodes_per_launch=episodes_per_launch, on_segment=on_segment)
    engine.check_status(inner)
    launch = dict(inner=inner, cfg=cfg, keys=keys, hps=chain_hp, theta=theta, eps=eps, worker=worker, sign=sign)
    return transfer_common.inner_results(inner, n_ag), launch
