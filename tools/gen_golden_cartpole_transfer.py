#!/usr/bin/env python3
"""Fixtures that pin experiments/transfer_cartpole.py to the reference's own CartPole transfer scripts
(experiments/GTNC_evaluate_cartpole_transfer_vary_hp.py: DDQN agents that each draw their hyper-parameters;
experiments/GTNC_evaluate_cartpole_transfer_algo.py: DuelingDDQN agents at fixed settings).

TEST INFRASTRUCTURE, run on the CPU in the build container: imports the read-only reference and the gym / ConfigSpace shims at run time (through
oracle/gen_golden.py's helpers), puts an empty stand-in for `hpbandster` (which the scripts import for reading logs and which is not installed)
into sys.modules, and runs the scripts' OWN load_envs_and_config / train_test_agents (and through it the vary_hp script's vary_hp) with
MODEL_AGENTS patched down to 2.  The budget is cut where the scripts hand every agent its config: the config an agent is built from gets CUT's
train_episodes (the algo script's agents also CUT_DUELING's feature_dim, the ICM is CUT_ICM's size), max_steps is cut in the checkpoint's env
section; everything else is the scripts' block.  Reward nets are narrow (16 units) reference-built nets with the weight matrices scaled by 1.5;
they reach the script as a checkpoint {'model', 'config'} that its load_envs_and_config reads back.

Writes only recorded arrays to tests/golden/g18*_cartpole_transfer_*.npz: the config before and after the script's in-place writes, theta, and
per agent (prefix a0_ / a1_) the hyper-parameters (the vary_hp script: as drawn), the fresh agent (and ICM), every draw (epsilon uniforms,
random actions, replay indices, train / test resets), every training row, and both returned lists.

    python tools/gen_golden_cartpole_transfer.py
"""
import copy
import importlib
import json
import os
import random
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402  (puts the reference and the shims on sys.path)

import torch  # noqa: E402

AGENTS = 2
ENV_NAME, ENV_CLS, YAML = "CartPole-v0", "CartPoleEnv", "default_config_cartpole_reward_env.yaml"
SCRIPTS = {"vary_hp": ("experiments.GTNC_evaluate_cartpole_transfer_vary_hp", "ddqn"),
           "algo": ("experiments.GTNC_evaluate_cartpole_transfer_algo", "duelingddqn")}
CUT_ICM = dict(feature_dim=8, hidden_size=16)       # the block's ICM (32 / 128) has tens of thousands of parameters per agent: too large to record
CUT_DUELING = dict(feature_dim=32)                  # the algo block's feature_dim 128: two 128 x 128 heads per agent, too large to record
HP_KEYS = ("lr", "batch_size", "hidden_size", "hidden_layer")


def load_script(key):
    for name in ("hpbandster", "hpbandster.core", "hpbandster.core.result"):       # the scripts only read logs with it: never called here
        sys.modules.setdefault(name, types.ModuleType(name))
    mod = importlib.import_module(SCRIPTS[key][0])
    mod.MODEL_AGENTS = AGENTS
    return mod


def write_checkpoint(path, seed, rtype, max_steps):
    from envs.env_factory import EnvFactory
    cfg = gg.load_cfg(YAML)
    cfg["device"] = "cpu"
    cfg["envs"][ENV_NAME].update(max_steps=max_steps, hidden_size=16, hidden_layer=1, reward_env_type=rtype)
    gg.seed_all(seed)
    with gg.quiet():
        env = EnvFactory(cfg).generate_reward_env()
    with torch.no_grad():
        for p in env.env.reward_net.parameters():
            if p.dim() == 2:
                p.mul_(1.5)
    torch.save({'model': env.state_dict(), 'config': cfg}, path)
    return copy.deepcopy(cfg)


def gen(name, key, mode, seed, rtype, max_steps, train_episodes):
    import ConfigSpace
    import gym.envs as genvs
    import gym.spaces as gspaces
    script = load_script(key)
    section = SCRIPTS[key][1]
    cut = dict(train_episodes=train_episodes)
    if key == "algo":
        cut.update(CUT_DUELING)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "model.pt")
        cfg_before = write_checkpoint(path, seed, rtype, max_steps)
        with gg.quiet():
            reward_env, real_env, config = script.load_envs_and_config(path)
    cfg_before["envs"][ENV_NAME]["solved_reward"] = config["envs"][ENV_NAME]["solved_reward"]
    env = real_env if mode in ("0", "-1") else reward_env          # eval_base / eval_icm hand the real env over, eval_models the reward env
    theta = gg.pack_linear_only(reward_env.state_dict(), "env.reward_net.")
    agents = []                                                     # one record per agent, in the order the script builds them
    state = dict(active=False, phase="train", cur=None, obs=None, hp=None)
    orig_random, orig_randint = random.random, np.random.randint
    env_class = getattr(genvs, ENV_CLS)
    orig_sample, orig_reset = gspaces.Discrete.sample, env_class.reset
    orig_vary, orig_select = getattr(script, "vary_hp", None), script.select_agent
    orig_step, orig_env_reset = env.step, env.reset

    def rec():
        return state["cur"]

    def rec_random():
        v = orig_random()
        if state["active"] and state["phase"] != "test":
            rec()["eps_uniform"].append(v)
        return v

    def rec_randint(*a, **k):
        v = orig_randint(*a, **k)
        if state["active"]:
            rec()["replay"].append(np.asarray(v).copy())
        return v

    def rec_sample(self):
        v = orig_sample(self)
        if state["active"]:
            rec()["rand"].append(int(v))
        return v

    def rec_reset(self):
        obs = orig_reset(self)
        if state["active"]:
            rec()["test_reset" if state["phase"] == "test" else "train_reset"].append(np.array(self.state, np.float64).copy())
        return obs

    def rec_env_reset():
        s = orig_env_reset()
        if state["phase"] != "test":
            state["obs"] = s.detach().numpy().astype(np.float32).copy()
        return s

    def rec_step(action, state_=None):
        ns, r, d = orig_step(action=action)
        if state["active"] and state["phase"] != "test":
            rec()["steps"].append(dict(state=state["obs"], action=int(action.item()), next_state=ns.detach().numpy().copy(), reward=float(r.item()),
                                       done=float(d.item()), n_rand=len(rec()["rand"])))
            state["obs"] = ns.detach().numpy().astype(np.float32).copy()
        return ns, r, d

    def cut_vary(config_):
        # the agent trains for CUT's episodes; the draw itself is the script's, around the block's values
        config_mod = orig_vary(config_)
        state["hp"] = {k: config_mod["agents"][section][k] for k in HP_KEYS}
        return config_mod

    def wrapped_select(config, agent_name):
        config = copy.deepcopy(config)                              # the script's own config stays as the script wrote it
        config["agents"][section].update(cut)
        config["agents"]["icm"].update(CUT_ICM)
        agent = orig_select(config=config, agent_name=agent_name)
        hp = state["hp"] if key == "vary_hp" else {k: config["agents"][section][k] for k in HP_KEYS}
        sd = agent.model.state_dict()
        r = dict(eps_uniform=[], rand=[], replay=[], train_reset=[], test_reset=[], steps=[], hp=hp, agent=agent, agent_name=agent_name,
                 init=gg.pack_linear_params(sd, "net.") if hasattr(agent.model, "net") else gg._pack_dueling(sd))
        if getattr(agent, "icm", None):
            r["icm_init"] = np.concatenate([v.detach().cpu().numpy().astype(np.float32).reshape(-1) for v in agent.icm.model.state_dict().values()])
        agents.append(r)
        state["cur"] = r
        orig_test = agent.test

        def test(*a, **k):
            prev, state["phase"] = state["phase"], "test"
            try:
                return orig_test(*a, **k)
            finally:
                state["phase"] = prev
        agent.test = test
        return agent

    gg.seed_all(seed)
    ConfigSpace.RANDOM.seed(seed)
    env.step, env.reset = rec_step, rec_env_reset
    random.random, np.random.randint = rec_random, rec_randint
    gspaces.Discrete.sample, env_class.reset = rec_sample, rec_reset
    script.select_agent = wrapped_select
    if orig_vary is not None:
        script.vary_hp = cut_vary
    try:
        state["active"] = True
        with gg.quiet():
            rewards, episode_lengths = script.train_test_agents(mode, env, real_env, config)
        state["active"] = False
    finally:
        random.random, np.random.randint = orig_random, orig_randint
        gspaces.Discrete.sample, env_class.reset = orig_sample, orig_reset
        script.select_agent = orig_select
        if orig_vary is not None:
            script.vary_hp = orig_vary
        env.step, env.reset = orig_step, orig_env_reset
    assert len(agents) == AGENTS == len(rewards) == len(episode_lengths)
    out = dict(config_before_json=np.array(json.dumps(cfg_before)), config_json=np.array(json.dumps(config)),
               cut_json=np.array(json.dumps(dict(agent=cut, icm=CUT_ICM))), mode=np.array(mode), script=np.array(key), env_name=np.array(ENV_NAME),
               theta=theta, agents=np.array(AGENTS))
    for i, r in enumerate(agents):
        p = "a%d_" % i
        steps = r["steps"]
        explored, prev = np.zeros(len(steps), np.int32), 0
        for k, st in enumerate(steps):
            explored[k], prev = int(st["n_rand"] > prev), st["n_rand"]
        B = int(r["hp"]["batch_size"])
        out.update({p + "hp_json": np.array(json.dumps(r["hp"])), p + "agent_name": np.array(r["agent_name"]), p + "agent_init": r["init"],
                    p + "tape_eps_uniform": np.array(r["eps_uniform"], np.float64), p + "tape_rand_action": np.array(r["rand"], np.int32),
                    p + "tape_replay_idx": (np.stack(r["replay"]).astype(np.int32) if r["replay"] else np.zeros((0, B), np.int32)),
                    p + "tape_train_reset": np.array(r["train_reset"], np.float64).reshape(-1, 4),
                    p + "tape_test_reset": np.array(r["test_reset"], np.float64).reshape(-1, 4),
                    p + "tr_state": np.stack([s["state"] for s in steps]).astype(np.float32), p + "tr_action": np.array([s["action"] for s in steps], np.int32),
                    p + "tr_explored": explored, p + "tr_next_state": np.stack([s["next_state"] for s in steps]).astype(np.float32),
                    p + "tr_reward": np.array([s["reward"] for s in steps], np.float32), p + "tr_done": np.array([s["done"] for s in steps], np.float32),
                    p + "rewards": np.array(rewards[i], np.float64), p + "episode_lengths": np.array(episode_lengths[i], np.int32)})
        if "icm_init" in r:
            out[p + "icm_init"] = r["icm_init"]
            out[p + "icm_final"] = np.concatenate([v.detach().cpu().numpy().astype(np.float32).reshape(-1) for v in r["agent"].icm.model.state_dict().values()])
        print(name, "agent", i, r["hp"], "rows", len(steps), "learn steps", len(r["replay"]), "rewards", np.round(rewards[i], 3).tolist(),
              "lengths", list(episode_lengths[i]))
    gg.save(name, **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["a", "b", "c", "d"]
    if "a" in which:      # the vary_hp script on a loaded reward net of type 2 (potential shaping on top of the real reward)
        gen("g18a_cartpole_transfer_vary_hp_mode2", "vary_hp", "2", seed=1801, rtype=2, max_steps=30, train_episodes=6)
    if "b" in which:      # the vary_hp script's mode -1: ddqn_icm on the real env
        gen("g18b_cartpole_transfer_vary_hp_mode_minus1", "vary_hp", "-1", seed=1802, rtype=2, max_steps=30, train_episodes=6)
    if "c" in which:      # the algo script on a loaded reward net of type 5 (the net's output alone)
        gen("g18c_cartpole_transfer_algo_mode5", "algo", "5", seed=1803, rtype=5, max_steps=30, train_episodes=6)
    if "d" in which:      # the algo script's mode -1: duelingddqn_icm on the real env
        gen("g18d_cartpole_transfer_algo_mode_minus1", "algo", "-1", seed=1804, rtype=2, max_steps=30, train_episodes=6)
