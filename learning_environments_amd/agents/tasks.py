"""Inner-loop tasks: which fused kernel evaluates a population member for a given (inner agent, synthetic env type).

The reference dispatches through select_agent (agents/agent_utils.py:15-66) + EnvFactory; here each supported
combination owns one fused kernel:
    DDQN on a VirtualEnv (synthetic_env_type 0)   -> lenv_ddqn_se_inner_loop   (BASELINE configs 1-2, Acrobot-DDQN)
    DuelingDDQN on a VirtualEnv                   -> lenv_dueling_se_inner_loop (BASELINE config 3)
    DDQN_vary / DuelingDDQN_vary on a VirtualEnv  -> lenv_dueling_se_inner_loop_hp (per-chain lr / batch / width / depth)
    TD3_vary on a RewardEnv over the stand-in     -> lenv_td3_rn_inner_loop_hp
    QL / QL_cb / SARSA / SARSA_cb on a RewardEnv over a gridworld (type 1) -> lenv_ql_rn_inner_loop (BASELINE config 4)
    the same agents with their own alpha / gamma per chain (the gridworld transfer scripts; experiments/transfer_gridworld.py builds QlRnTask itself: the
        variation lives in the script, no agent name selects it) -> lenv_ql_rn_inner_loop_hp
    QL / QL_cb / SARSA / SARSA_cb on a VirtualEnv over a gridworld (type 0) -> lenv_ql_se_inner_loop
    TD3  on a RewardEnv over the HalfCheetah stand-in -> lenv_td3_rn_inner_loop (BASELINE config 5)
    TD3_discrete_vary on a VirtualEnv (CartPole / Acrobot / MountainCar) -> lenv_td3d_inner_loop
    TD3_discrete_vary on a RewardEnv over CartPole / Acrobot / MountainCar, or the real env itself (type 1) -> lenv_td3d_rn_inner_loop
    PPO on a RewardEnv over the HalfCheetah stand-in / Pendulum / MountainCarContinuous (synthetic_env_type 1; reward_env_type 0 = the real env itself) -> lenv_ppo_rn_inner_loop
Anything else raises NotImplementedError, like the reference does for unknown agents."""
import copy

import numpy as np
import torch

from ..config import (TABULAR_AGENTS, TD3_DISCRETE_ENVS, agent_layer_dims, agent_layer_norm_slice, ddqn_cfg_from_config, icm_layer_dims, ppo_cfg_from_config,
                      ppo_layer_dims, ql_cfg_from_config, ql_se_cfg_from_config, td3_cfg_from_config, td3_layer_dims, td3_layer_norm_slices, td3d_cfg_from_config, td3d_rn_cfg_from_config)
from . import vary
from .nes_common import linear_init_bounds, set_layer_norm_init, with_layer_norm_block


def _device_bounds(engine, layer_dims, ln_slice=None):
    """nn.Linear default-init bounds of a flat parameter vector (LayerNorm blocks at ln_slice: bound 0) on the engine's device."""
    return torch.from_numpy(with_layer_norm_block(linear_init_bounds(layer_dims), ln_slice)).to(engine.device)


def _max_config(config, section):
    """A copy of config whose agent section carries the largest batch_size / hidden_size / hidden_layer agents/vary.py can draw:
    the launch is sized for it (workspace / LDS / row strides)."""
    bd = vary.hp_bounds(config["agents"][section])
    big = copy.deepcopy(config)
    big["agents"][section].update(batch_size=bd["batch_size"][1], hidden_size=bd["hidden_size"][1], hidden_layer=bd["hidden_layer"][1])
    return big


def _icm_bounds(engine, cfg):
    """ICM agents ("ddqn_icm", "td3_icm", ...: the agent carries an Intrinsic Curiosity Module, agents/DDQN.py:40-58): the bounds of the
    fresh ICM (nn.Linear default init) every chain draws from its own counter-RNG stream on the GPU; None without one."""
    return _device_bounds(engine, icm_layer_dims(cfg)) if engine.name == "hip" and cfg.icm_enabled else None


class _FixedShapeAgents(object):
    """Every chain at cfg's shapes: a fresh agent from the generation's draw with agent_bounds (use_layer_norm: the LayerNorm blocks at
    ln_slice get weight 1 / bias 0)."""

    def _init_bounds(self, layer_dims, ln_slice):
        self.ln_slice = ln_slice
        self.agent_bounds = _device_bounds(self.engine, layer_dims, ln_slice)
        self.icm_bounds = _icm_bounds(self.engine, self.cfg)

    def _fresh_agents(self, inner, keys_t, agent_init):
        if self.icm_bounds is not None:
            inner.draw_icm_init(keys_t, self.icm_bounds)
        set_layer_norm_init(agent_init, self.ln_slice)


class _VaryAgents(object):
    """The *_vary tasks: every chain draws its own lr / batch_size / hidden_size / hidden_layer (agents/vary.py) from its key and gets a
    fresh agent at those shapes inside scores() (draw_hp is host work between the kernels: such a task is not captured into a graph,
    GTN_master.py)."""
    icm_bounds = None

    def _init_vary(self, base):
        self.base = base                  # the config's agent section the draws start from
        self.agent_bounds = None
        self.last_hp = None
        self.fixed_hp = None

    def draw_hp(self, keys):
        if self.fixed_hp is not None:     # a recorded draw replayed (parity tests against the reference's runs)
            return list(self.fixed_hp)
        return [vary.vary_hyperparameters(self.base, vary.chain_units(k)) for k in keys]

    def _fresh_agents(self, inner, keys_t, draw_hp=True):
        # the draws are a host function of the chain keys (ConfigSpace's role in the reference); reading the keys back waits only
        # for the generation's draw kernel
        if draw_hp:
            hp = self.last_hp = self.draw_hp(keys_t.cpu().numpy().view(np.uint64))
            inner.set_hp([h["lr"] for h in hp], [h["batch_size"] for h in hp], [h["hidden_size"] for h in hp],
                         [h["hidden_layer"] for h in hp])
        inner.draw_agent_init(keys_t)
        if self.icm_bounds is not None:
            inner.draw_icm_init(keys_t, self.icm_bounds)


class DdqnSeTask(_FixedShapeAgents):
    name = "ddqn_se"

    def __init__(self, config, engine, test_mode=0):
        self.engine = engine
        self.cfg = ddqn_cfg_from_config(config, test_mode=test_mode) if engine.name == "hip" else engine.cfg_from_config(config)
        self._init_bounds(agent_layer_dims(self.cfg), agent_layer_norm_slice(self.cfg))

    def make_inner(self, chains, want_episode_stats=True):
        return self.engine.make_inner(self.cfg, chains, want_episode_stats=want_episode_stats)

    def scores(self, inner, theta, eps, chain_worker, chain_sign, keys_t, agent_init):
        self._fresh_agents(inner, keys_t, agent_init)
        return self.engine.inner_scores(inner, theta, eps, chain_worker, chain_sign, agent_init, keys_t)

    def needs_agent_init(self):
        return True


class DdqnVaryTask(_VaryAgents):
    """DDQN_vary / DuelingDDQN_vary on a VirtualEnv (agents/DDQN_vary.py, agents/DuelingDDQN_vary.py): every chain draws its
    own lr / batch_size / hidden_size / hidden_layer (agents/vary.py) and the whole heterogeneous population still runs as ONE
    launch of the GEMM-tiled kernel (per-chain hyper-parameter arrays, workspace sized for the largest draw)."""
    name = "ddqn_vary_se"

    def __init__(self, config, engine, test_mode=0):
        self.engine = engine              # HipNesEngine, or the test suite's oracle-backed stand-in (CPU tensors)
        self.agent_key = config["agents"]["gtn"]["agent_name"].lower()[:-5]
        if self.agent_key.endswith("_icm"):               # "ddqn_icm_vary": DDQN_vary(icm=True), agents/agent_utils.py:43-44
            self.agent_key = self.agent_key[:-4]
        self.cfg = ddqn_cfg_from_config(_max_config(config, self.agent_key), test_mode=test_mode)
        self.cfg.grad_chunk = 0                           # one sequential batch gradient (GEMM-tiled kernel)
        self._init_vary(config["agents"][self.agent_key])
        self.icm_bounds = _icm_bounds(engine, self.cfg)

    def make_inner(self, chains, want_episode_stats=True, **kw):
        """kw: InnerLoop's own keywords (segments=True: the launch will run as episode segments -- the same GEMM-tiled kernel, same bits)"""
        return self.engine.make_inner(self.cfg, chains, want_episode_stats=want_episode_stats, vary=True, **kw)

    def scores(self, inner, theta, eps, chain_worker, chain_sign, keys_t, agent_init, **run_kw):
        """run_kw: run()'s own keywords (episodes_per_launch, on_segment)"""
        self._fresh_agents(inner, keys_t)
        return self.engine.inner_scores(inner, theta, eps, chain_worker, chain_sign, None, keys_t, **run_kw)

    def needs_agent_init(self):
        return False          # drawn inside scores(), once the chains' shapes are known


class QlRnTask(object):
    name = "ql_rn"

    def __init__(self, config, engine, tables, test_mode=0):
        self.engine = engine
        self.tables = tables
        self.cfg = ql_cfg_from_config(config, tables, test_mode=test_mode)
        self.agent_bounds = None

    def make_inner(self, chains, want_episode_stats=False):
        return self.engine.make_inner_ql(self.cfg, chains, self.tables, want_episode_stats=want_episode_stats)

    def scores(self, inner, theta, eps, chain_worker, chain_sign, keys_t, agent_init):
        return self.engine.inner_scores_ql(inner, theta, eps, chain_worker, chain_sign, keys_t)

    def needs_agent_init(self):
        return False          # a fresh QL agent is an all-zero table (QL.py:25)


class QlSeTask(object):
    """QL / QL_cb / SARSA / SARSA_cb on a gridworld VirtualEnv (synthetic_env_type 0): one launch of lenv_ql_se_inner_loop per generation,
    theta = state_net | reward_net | done_net.  `tables` are the REAL grid's (the per-episode tests and the final test walk them).  No
    host-side draws: the task can be captured into a graph."""
    name = "ql_se"

    def __init__(self, config, engine, tables, test_mode=0):
        if engine.name != "hip":
            raise NotImplementedError("the tabular agents on a gridworld VirtualEnv need the HIP engine")
        self.engine = engine
        self.tables = tables
        self.cfg = ql_se_cfg_from_config(config, tables, test_mode=test_mode)
        self.agent_bounds = None

    def make_inner(self, chains, want_episode_stats=False, **kw):
        return self.engine.make_inner_ql_se(self.cfg, chains, self.tables, want_episode_stats=want_episode_stats, **kw)

    def scores(self, inner, theta, eps, chain_worker, chain_sign, keys_t, agent_init):
        return self.engine.inner_scores_ql_se(inner, theta, eps, chain_worker, chain_sign, keys_t)

    def needs_agent_init(self):
        return False          # a fresh tabular agent is an all-zero table (QL.py:25)


class Td3RnTask(_FixedShapeAgents):
    name = "td3_rn"

    def __init__(self, config, engine, test_mode=0):
        self.engine = engine
        self.cfg = td3_cfg_from_config(config, test_mode=test_mode)
        # use_layer_norm: the three nets' LayerNorm blocks in the flat parameter vector; "td3_icm": TD3(icm=True), a fresh ICM per chain
        self._init_bounds(td3_layer_dims(self.cfg), td3_layer_norm_slices(self.cfg))

    def make_inner(self, chains, want_episode_stats=False):
        return self.engine.make_inner_td3(self.cfg, chains, want_episode_stats=want_episode_stats)

    def scores(self, inner, theta, eps, chain_worker, chain_sign, keys_t, agent_init):
        self._fresh_agents(inner, keys_t, agent_init)
        return self.engine.inner_scores_td3(inner, theta, eps, chain_worker, chain_sign, agent_init, keys_t)

    def needs_agent_init(self):
        return True


class Td3VaryTask(_VaryAgents):
    """TD3_vary on the stand-in RewardEnv (agents/TD3_vary.py:24-58): per-chain lr / batch_size / hidden_size / hidden_layer in
    one launch of the TD3 kernel (lenv_td3_rn_inner_loop_hp), like DdqnVaryTask."""
    name = "td3_vary_rn"

    def __init__(self, config, engine, test_mode=0):
        if engine.name != "hip":
            raise NotImplementedError("the *_vary agents need the HIP engine")
        self.engine = engine
        self.cfg = td3_cfg_from_config(_max_config(config, "td3"), test_mode=test_mode)
        self._init_vary(config["agents"]["td3"])
        self.icm_bounds = _icm_bounds(engine, self.cfg)

    def make_inner(self, chains, want_episode_stats=False):
        return self.engine.make_inner_td3(self.cfg, chains, want_episode_stats=want_episode_stats, vary=True)

    def scores(self, inner, theta, eps, chain_worker, chain_sign, keys_t, agent_init):
        self._fresh_agents(inner, keys_t)
        return self.engine.inner_scores_td3(inner, theta, eps, chain_worker, chain_sign, None, keys_t)

    def needs_agent_init(self):
        return False


class Td3DiscreteTask(_VaryAgents):
    """TD3_discrete_vary on a VirtualEnv (agents/TD3_discrete_vary.py): one launch of lenv_td3d_inner_loop per generation.  With
    vary_hp (:21-26,119-157) every chain draws its own lr / batch_size / hidden_size / hidden_layer (agents/vary.py) and the launch is
    sized for the largest possible draw, like Td3VaryTask.  The fresh agents (nn.Linear default init, LayerNorm 1 / 0) are drawn on
    the device from the chain keys.  With synthetic_env_type 1 the chains train on a RewardEnv over the real env (or the real env
    itself, reward_env_type 0) through lenv_td3d_rn_inner_loop; theta is then the reward net."""
    name = "td3_discrete_se"

    def __init__(self, config, engine, test_mode=0):
        if engine.name != "hip":
            raise NotImplementedError("TD3_discrete_vary needs the HIP engine")
        self.engine = engine
        base = config["agents"]["td3_discrete_vary"]
        self.vary = bool(base["vary_hp"])
        self.cfg = td3d_cfg_from_config(_max_config(config, "td3_discrete_vary") if self.vary else config, test_mode=test_mode)
        self.rn = td3d_rn_cfg_from_config(config)
        if self.rn is not None:
            self.name = "td3_discrete_rn"
        self._init_vary(base)

    def make_inner(self, chains, want_episode_stats=False, **kw):
        return self.engine.make_inner_td3d(self.cfg, chains, want_episode_stats=want_episode_stats, vary=self.vary, rn=self.rn, **kw)

    def scores(self, inner, theta, eps, chain_worker, chain_sign, keys_t, agent_init, **run_kw):
        """run_kw: run()'s own keywords (episodes_per_launch, on_segment)"""
        self._fresh_agents(inner, keys_t, draw_hp=self.vary)
        return self.engine.inner_scores_td3(inner, theta, eps, chain_worker, chain_sign, None, keys_t, **run_kw)

    def needs_agent_init(self):
        return False          # drawn inside scores() (the LayerNorm parameters are not uniform draws)


class PpoRnTask(object):
    """PPO (agents/PPO.py) on a RewardEnv over a continuous real env, or on the real env itself (reward_env_type 0): one launch of
    lenv_ppo_rn_inner_loop per generation, theta = the reward net exactly as for TD3.  A fresh agent = action_std [A] at its configured
    constant (bound 0 in the generation's draw, then written the way set_layer_norm_init writes LayerNorm blocks) | actor.net | critic.net
    with nn.Linear's default init from the chain keys."""
    name = "ppo_rn"

    def __init__(self, config, engine, test_mode=0):
        if engine.name != "hip":
            raise NotImplementedError("the PPO inner agent needs the HIP engine")
        if int(test_mode) != 0:
            raise NotImplementedError("PPO with test_mode 1 (PPO.train without a test env) is not built")
        self.engine = engine
        self.cfg = ppo_cfg_from_config(config)
        A = self.cfg.action_dim
        self.agent_bounds = torch.from_numpy(np.concatenate([np.zeros(A, np.float32), linear_init_bounds(ppo_layer_dims(self.cfg))])).to(engine.device)

    def make_inner(self, chains, want_episode_stats=False, **kw):
        return self.engine.make_inner_ppo(self.cfg, chains, want_episode_stats=want_episode_stats, **kw)

    def scores(self, inner, theta, eps, chain_worker, chain_sign, keys_t, agent_init):
        agent_init[:, :self.cfg.action_dim] = float(self.cfg.action_std)
        return self.engine.inner_scores_ppo(inner, theta, eps, chain_worker, chain_sign, agent_init, keys_t)

    def needs_agent_init(self):
        return True


TD3_ENVS = ("HalfCheetah-v3", "Pendulum-v0", "MountainCarContinuous-v0")       # continuous real envs of the TD3 kernel


def select_task(config, engine, synthetic_env, test_mode=0):
    """test_mode: lenv_ddqn_cfg::test_mode -- 0 = GTN_Worker.calc_score's train(env, test_env=real_env); 1 = train(env) without a test env
    (the evaluation harness, experiments/syn_env_evaluate.py)."""
    agent_name = config["agents"]["gtn"]["agent_name"].lower()
    env_type = config["agents"]["gtn"]["synthetic_env_type"]
    tm = dict(test_mode=int(test_mode))
    if agent_name in ("ddqn", "duelingddqn", "ddqn_icm", "duelingddqn_icm") and env_type == 0:
        return DdqnSeTask(config, engine, **tm)
    if agent_name in ("ddqn_vary", "duelingddqn_vary", "ddqn_icm_vary", "duelingddqn_icm_vary") and env_type == 0:
        # vary_hp False: the agent IS its base agent (DDQN_vary.py:16-21); the *_icm_vary names read the same `<agent>_vary`
        # section (DDQN_vary.py:16) and switch the ICM on
        section = agent_name.replace("_icm", "")
        return DdqnVaryTask(config, engine, **tm) if config["agents"][section]["vary_hp"] else DdqnSeTask(config, engine, **tm)
    if agent_name in ("ddqn", "duelingddqn", "ddqn_icm", "duelingddqn_icm") and env_type == 1 and config["env_name"] in ("CartPole-v0", "Acrobot-v1", "MountainCar-v0"):
        return DdqnSeTask(config, engine, **tm)         # RewardEnv over the real env (default_config_cartpole_reward_env.yaml): same kernel
    if agent_name in ("ddqn_vary", "duelingddqn_vary", "ddqn_icm_vary", "duelingddqn_icm_vary") and env_type == 1 and config["env_name"] in ("CartPole-v0", "Acrobot-v1", "MountainCar-v0"):
        # the *_vary agents on a RewardEnv / on the real env itself (experiments/syn_env_run_vary_hp.py:47-54, mode 0): same kernel, per-chain shapes
        section = agent_name.replace("_icm", "")
        return DdqnVaryTask(config, engine, **tm) if config["agents"][section]["vary_hp"] else DdqnSeTask(config, engine, **tm)
    if agent_name in TABULAR_AGENTS and env_type == 1:
        real = synthetic_env.env.real_env
        if not hasattr(real, "tables"):
            raise NotImplementedError("QL needs a discrete (gridworld) real env")
        return QlRnTask(config, engine, real.tables, **tm)
    if agent_name in TABULAR_AGENTS and env_type == 0:
        grid = getattr(getattr(getattr(synthetic_env, "env", None), "reset_env", None), "env", None)     # VirtualEnv.reset_env = EnvWrapper(GridEnv)
        if not hasattr(grid, "tables"):
            raise NotImplementedError("inner agent '%s' on a VirtualEnv needs a discrete (gridworld) env" % agent_name)
        return QlSeTask(config, engine, grid.tables, **tm)
    # TD3 on the HalfCheetah stand-in / Pendulum-v0 / MountainCarContinuous-v0: RewardEnv (type 1, BASELINE config 5) or VirtualEnv (type 0, default_config_halfcheetah.yaml)
    if agent_name in ("td3", "td3_icm") and env_type in (0, 1) and config["env_name"] in TD3_ENVS:
        return Td3RnTask(config, engine, **tm)
    if agent_name in ("td3_vary", "td3_icm_vary") and env_type in (0, 1) and config["env_name"] in TD3_ENVS:
        return Td3VaryTask(config, engine, **tm) if config["agents"]["td3_vary"]["vary_hp"] else Td3RnTask(config, engine, **tm)
    if agent_name == "td3_discrete_vary" and env_type in (0, 1) and config["env_name"] in TD3_DISCRETE_ENVS:
        return Td3DiscreteTask(config, engine, **tm)           # type 1: RewardEnv over the real env / the real env itself (mode 0)
    if agent_name == "ppo":
        # the reference runs PPO as the unseen agent of the reward-net transfer experiments (experiments/GTNC_evaluate_*_transfer_algo.py)
        if env_type != 1:
            raise NotImplementedError("PPO on a VirtualEnv (synthetic_env_type %s) is not built: PPO trains on a RewardEnv (type 1)" % env_type)
        if config["env_name"] not in TD3_ENVS:
            raise NotImplementedError("PPO on '%s' is not built: the PPO kernel takes the continuous real envs %s" % (config["env_name"], ", ".join(TD3_ENVS)))
        return PpoRnTask(config, engine, **tm)
    if agent_name == "ppo_icm":
        raise NotImplementedError("ppo_icm (PPO with an Intrinsic Curiosity Module) is not built")
    raise NotImplementedError("inner agent '%s' on synthetic_env_type %s has no fused kernel yet" % (agent_name, env_type))
