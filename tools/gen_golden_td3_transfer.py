#!/usr/bin/env python3
"""Fixtures that pin experiments/transfer_vary_hp.py to the reference's own TD3 transfer scripts (experiments/GTNC_evaluate_cmc_transfer_vary_hp.py,
experiments/GTNC_evaluate_halfcheetah_transfer_vary_hp.py).

TEST INFRASTRUCTURE, run on the CPU in the build container: imports the read-only reference and the gym / ConfigSpace shims at run time (through
oracle/gen_golden.py's helpers), puts an empty stand-in for `hpbandster` (which the scripts import for reading logs and which is not installed)
into sys.modules, and runs the scripts' OWN load_envs_and_config / train_test_agents (and through it their vary_hp) with MODEL_AGENTS patched down
to 2.  The budget is cut where the scripts hand every agent its config: the config that vary_hp returns gets CUT's train_episodes / init_episodes
(the draw runs around BATCH rows instead of the block's 256, the ICM is CUT_ICM's size), max_steps is cut in the checkpoint's env section; everything else is
the scripts' block.  Reward nets are narrow (16 units) reference-built nets with the weight matrices scaled by 1.5; they reach the script as a
checkpoint {'model', 'config'} that its load_envs_and_config reads back.

Writes only recorded arrays to tests/golden/g17*_td3_transfer_*.npz: the config before and after the script's in-place writes, theta, and per
agent (prefix a0_ / a1_) the sampled hyper-parameters, the fresh agent (and ICM), every draw (random actions, action / test / policy noise, replay
indices, train / test resets), every training row, the final parameters, and both returned lists.

    python tools/gen_golden_td3_transfer.py
"""
import copy
import importlib
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402  (puts the reference and the shims on sys.path)

import torch  # noqa: E402

AGENTS = 2
SCRIPTS = {"cmc": ("experiments.GTNC_evaluate_cmc_transfer_vary_hp", "default_config_cmc_reward_env.yaml", "MountainCarContinuous-v0", "Continuous_MountainCarEnv"),
           "cheetah": ("experiments.GTNC_evaluate_halfcheetah_transfer_vary_hp", "default_config_halfcheetah_reward_env.yaml", "HalfCheetah-v3", "CheetahStandinEnv")}
CUT = dict(train_episodes=4, init_episodes=2)      # of the config every agent is built from (the scripts: 3000 / 50 and 1000 / 20)
BATCH = 24                                          # the block's batch_size 256 would draw up to 768 rows per learn step: the draw runs around 24 instead
CUT_ICM = dict(feature_dim=8, hidden_size=16)       # the block's ICM (32 / 128) has 88 033 parameters per agent: too large to record
AGENT_SHAPE = dict(hidden_size=24, hidden_layer=2)  # the checkpoint's td3 section (the scripts leave it alone): draws of 8..72 units, 1..3 layers


def load_script(key):
    for name in ("hpbandster", "hpbandster.core", "hpbandster.core.result"):       # the scripts only read logs with it: never called here
        sys.modules.setdefault(name, types.ModuleType(name))
    mod = importlib.import_module(SCRIPTS[key][0])
    mod.MODEL_AGENTS = AGENTS
    return mod


def write_checkpoint(path, key, seed, rtype, max_steps):
    from envs.env_factory import EnvFactory
    _, yaml_name, env_name, _ = SCRIPTS[key]
    cfg = gg.load_cfg(yaml_name)
    cfg["device"] = "cpu"
    cfg["agents"]["td3"].update(AGENT_SHAPE)
    cfg["envs"][env_name].update(max_steps=max_steps, hidden_size=16, hidden_layer=1, reward_env_type=rtype)
    gg.seed_all(seed)
    with gg.quiet():
        env = EnvFactory(cfg).generate_reward_env()
    with torch.no_grad():
        for p in env.env.reward_net.parameters():
            if p.dim() == 2:
                p.mul_(1.5)
    torch.save({'model': env.state_dict(), 'config': cfg}, path)
    return copy.deepcopy(cfg)


def gen(name, key, mode, seed, rtype, max_steps):
    import ConfigSpace
    import gym.envs as genvs
    import gym.spaces as gspaces
    script = load_script(key)
    _, _, env_name, env_cls = SCRIPTS[key]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "model.pt")
        cfg_before = write_checkpoint(path, key, seed, rtype, max_steps)
        with gg.quiet():
            reward_env, real_env, config = script.load_envs_and_config(path)
    cfg_before["envs"][env_name]["solved_reward"] = config["envs"][env_name]["solved_reward"]
    env = real_env if mode in ("0", "-1") else reward_env          # eval_base / eval_icm hand the real env over, eval_models the reward env
    theta = gg.pack_linear_only(reward_env.state_dict(), "env.reward_net.")
    agents = []                                                     # one record per agent, in the order the script builds them
    state = dict(active=False, purpose=None, phase="train", cur=None, obs=None)
    orig_randn, orig_randn_like, orig_randint = torch.randn, torch.randn_like, np.random.randint
    env_class = getattr(genvs, env_cls)
    orig_box_sample, orig_reset = gspaces.Box.sample, env_class.reset
    orig_vary, orig_select = script.vary_hp, script.select_agent
    orig_step, orig_env_reset = env.step, env.reset

    def rec():
        return state["cur"]

    def rec_randn(*a, **k):
        v = orig_randn(*a, **k)
        if state["active"] and state["purpose"] in ("act_noise", "test_noise"):
            rec()[state["purpose"]].append(v.numpy().copy())
        return v

    def rec_randn_like(t, *a, **k):
        v = orig_randn_like(t, *a, **k)
        if state["active"] and state["purpose"] == "learn":
            rec()["policy_noise"].append(v.numpy().copy())
        return v

    def rec_randint(*a, **k):
        v = orig_randint(*a, **k)
        if state["active"]:
            rec()["replay"].append(np.asarray(v).copy())
        return v

    def rec_box_sample(self):
        v = orig_box_sample(self)
        if state["active"]:
            rec()["rand"].append(np.asarray(v).copy())
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
        ns, r, d = orig_step(action=action, state=state_) if state_ is not None else orig_step(action=action)
        if state["active"] and state["phase"] != "test":
            rec()["steps"].append(dict(state=state["obs"], action=action.detach().numpy().astype(np.float32).copy(), next_state=ns.detach().numpy().copy(),
                                       reward=float(r.item()), done=float(d.item())))
            state["obs"] = ns.detach().numpy().astype(np.float32).copy()
        return ns, r, d

    def cut_vary(config_):
        # the draw runs around BATCH rows, and the agent trains for CUT's episodes; the script's config itself stays as the script wrote it
        c = copy.deepcopy(config_)
        c["agents"]["td3"]["batch_size"] = BATCH
        config_mod = orig_vary(c)
        config_mod["agents"]["td3"].update(CUT)
        config_mod["agents"]["icm"].update(CUT_ICM)
        state["hp"] = {k: config_mod["agents"]["td3"][k] for k in ("lr", "batch_size", "hidden_size", "hidden_layer")}
        return config_mod

    def wrapped_select(config, agent_name):
        agent = orig_select(config=config, agent_name=agent_name)
        r = dict(rand=[], act_noise=[], test_noise=[], policy_noise=[], replay=[], train_reset=[], test_reset=[], steps=[], hp=state["hp"], agent=agent,
                 init=gg._pack_td3(agent), agent_name=agent_name)
        if getattr(agent, "icm", None):
            r["icm_init"] = np.concatenate([v.detach().cpu().numpy().astype(np.float32).reshape(-1) for v in agent.icm.model.state_dict().values()])
        agents.append(r)
        state["cur"] = r

        def wrap(fn, purpose=None, phase=None):
            def inner(*a, **k):
                prev = (state["purpose"], state["phase"])
                if purpose:
                    state["purpose"] = purpose
                if phase:
                    state["phase"] = phase
                try:
                    return fn(*a, **k)
                finally:
                    state["purpose"], state["phase"] = prev
            return inner
        agent.select_train_action = wrap(agent.select_train_action, "act_noise")
        agent.select_test_action = wrap(agent.select_test_action, "test_noise")
        agent.learn = wrap(agent.learn, "learn")
        agent.test = wrap(agent.test, phase="test")
        return agent

    gg.seed_all(seed)
    ConfigSpace.RANDOM.seed(seed)
    env.step, env.reset = rec_step, rec_env_reset
    torch.randn, torch.randn_like, np.random.randint = rec_randn, rec_randn_like, rec_randint
    gspaces.Box.sample, env_class.reset = rec_box_sample, rec_reset
    script.vary_hp, script.select_agent = cut_vary, wrapped_select
    try:
        state["active"] = True
        with gg.quiet():
            rewards, episode_lengths = script.train_test_agents(mode, env, real_env, config)
        state["active"] = False
    finally:
        torch.randn, torch.randn_like, np.random.randint = orig_randn, orig_randn_like, orig_randint
        gspaces.Box.sample, env_class.reset = orig_box_sample, orig_reset
        script.vary_hp, script.select_agent = orig_vary, orig_select
        env.step, env.reset = orig_step, orig_env_reset
    assert len(agents) == AGENTS == len(rewards) == len(episode_lengths)
    out = dict(config_before_json=np.array(json.dumps(cfg_before)), config_json=np.array(json.dumps(config)), cut_json=np.array(json.dumps(dict(td3=CUT, icm=CUT_ICM, batch_size_base=BATCH))),
               mode=np.array(mode), env_name=np.array(env_name), theta=theta, agents=np.array(AGENTS))
    for i, r in enumerate(agents):
        A = np.stack(r["rand"]).shape[-1]
        p = "a%d_" % i
        out.update({p + "hp_json": np.array(json.dumps(r["hp"])), p + "agent_name": np.array(r["agent_name"]), p + "agent_init": r["init"],
                    p + "tape_rand_action": np.stack(r["rand"][1::2]).astype(np.float32),          # get_random_action samples twice, returns the 2nd
                    p + "tape_act_noise": np.stack(r["act_noise"]).astype(np.float32), p + "tape_test_noise": np.stack(r["test_noise"]).astype(np.float32),
                    p + "tape_policy_noise": np.stack(r["policy_noise"]).astype(np.float32).reshape(-1, A),
                    p + "tape_replay_idx": np.concatenate([np.asarray(x).reshape(-1) for x in r["replay"]]).astype(np.int32),
                    p + "tape_train_reset": np.array(r["train_reset"]), p + "tape_test_reset": np.array(r["test_reset"]),
                    p + "tr_state": np.stack([s["state"] for s in r["steps"]]), p + "tr_action": np.stack([s["action"] for s in r["steps"]]),
                    p + "tr_next_state": np.stack([s["next_state"] for s in r["steps"]]).astype(np.float32),
                    p + "tr_reward": np.array([s["reward"] for s in r["steps"]], np.float32),
                    p + "rewards": np.array(rewards[i], np.float64), p + "episode_lengths": np.array(episode_lengths[i], np.int32),
                    p + "final_params": gg._pack_td3(r["agent"])})
        if "icm_init" in r:
            out[p + "icm_init"] = r["icm_init"]
            out[p + "icm_final"] = np.concatenate([v.detach().cpu().numpy().astype(np.float32).reshape(-1) for v in r["agent"].icm.model.state_dict().values()])
        print(name, "agent", i, r["hp"], "rows", len(r["steps"]), "learn steps", len(r["policy_noise"]), "rewards", np.round(rewards[i], 3).tolist(),
              "lengths", list(episode_lengths[i]))
    gg.save(name, **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["a", "b", "c", "d"]
    if "a" in which:      # MountainCarContinuous mode 2: the block's same_action_num 2, the shaped rewards of the repeats summed
        gen("g17a_td3_transfer_cmc_mode2", "cmc", "2", seed=1701, rtype=2, max_steps=16)
    if "b" in which:      # MountainCarContinuous mode -1: td3_icm on the real env
        gen("g17b_td3_transfer_cmc_mode_minus1", "cmc", "-1", seed=1702, rtype=2, max_steps=16)
    if "c" in which:      # HalfCheetah stand-in mode 0: the real env
        gen("g17c_td3_transfer_cheetah_mode0", "cheetah", "0", seed=1703, rtype=2, max_steps=8)
    if "d" in which:      # HalfCheetah stand-in, an info-vector type
        gen("g17d_td3_transfer_cheetah_mode3", "cheetah", "3", seed=1704, rtype=3, max_steps=8)
