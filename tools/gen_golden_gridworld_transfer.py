#!/usr/bin/env python3
"""Fixtures that pin experiments/transfer_gridworld.py and the per-chain alpha / gamma of lenv_ql_rn_inner_loop_hp to the reference's own
gridworld transfer scripts (experiments/GTNC_evaluate_gridworld_transfer_vary_hp.py, experiments/GTNC_evaluate_gridworld_transfer_algo.py).

TEST INFRASTRUCTURE, run on the CPU in the build container: imports the read-only reference and the gym / ConfigSpace shims at run time (through
oracle/gen_golden.py's helpers), puts an empty stand-in for `hpbandster` (which the scripts import for reading logs and which is not
installed) into sys.modules, and runs the scripts' OWN load_envs_and_config / train_test_agents (and through it their vary_hp) with
MODEL_AGENTS patched down to 3 and the scripts' 500 episodes.  It writes only recorded arrays to tests/golden/g16*_gridworld_transfer_*.npz:
per agent the drawn alpha / gamma, every random.random and Discrete.sample draw, every training step (state, action, explored, next state,
reward, done), the final Q-table, both returned lists and the reference's shaped-reward table for that agent's gamma; per fixture theta and the
config as the script left it.  Ragged per-agent arrays are stored concatenated, with offsets.

The reward nets are reference-built Cliff nets with the weight matrices scaled by 1.5 (a trained-looking net, as tools/gen_golden_ppo.py does);
they reach the scripts the way models do: as a checkpoint {'model', 'config'} that the script's load_envs_and_config reads back.  The checkpoint
of the vary_hp mode-2 fixture is kept as tests/golden/ckpt_cliff_reward_env_reference.pt.

A fixture is written only when the replay through the oracle's OWN shaped-reward table (bit-equal to the kernel's) returns the reference's two
lists: the reference's table differs from it by an ulp in places (torch's gemv order), and an ulp can flip an argmax between two near-tied Q
entries.  Otherwise the next seed is tried.  tests/test_transfer_gridworld_reference.py replays with the reference's table as input.

    python tools/gen_golden_gridworld_transfer.py
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
from oracle import oracle as orc  # noqa: E402

import torch  # noqa: E402

AGENTS = 3
SCRIPT_MODULES = {"vary_hp": "experiments.GTNC_evaluate_gridworld_transfer_vary_hp", "algo": "experiments.GTNC_evaluate_gridworld_transfer_algo"}


def load_script(script):
    for name in ("hpbandster", "hpbandster.core", "hpbandster.core.result"):       # the scripts only read logs with it: never called here
        sys.modules.setdefault(name, types.ModuleType(name))
    mod = importlib.import_module(SCRIPT_MODULES[script])
    mod.MODEL_AGENTS = AGENTS
    return mod


def write_checkpoint(path, seed, mode, env_over):
    """A reference-built Cliff reward env of the mode's type as GTN_Master.save_model's payload."""
    from envs.env_factory import EnvFactory
    cfg = gg.load_cfg("default_config_gridworld_reward_env.yaml")
    cfg["device"] = "cpu"
    e = cfg["envs"][cfg["env_name"]]
    e.update(env_over or {})
    e["reward_env_type"] = int(mode) if int(mode) > 0 else 2         # modes 0 / -1 pass the real env; the scripts load the type-2 models for them
    gg.seed_all(seed)
    with gg.quiet():
        env = EnvFactory(cfg).generate_reward_env()
    with torch.no_grad():
        for p in env.env.reward_net.parameters():
            if p.dim() == 2:
                p.mul_(1.5)
    torch.save({'model': env.state_dict(), 'config': cfg}, path)


def shaped_table(env, real, gamma):
    """What env.step pays for every (s, a) once the agent has handed it gamma (base_agent.py:86)."""
    out = np.zeros((48, 4), np.float32)
    env.set_agent_params(same_action_num=1, gamma=gamma)
    with torch.no_grad():
        for s in range(48):
            for a in range(4):
                if real:
                    env.env.reset()
                    env.env.env.state = env.env.env._obs_to_state(s)
                    out[s, a] = env.env.step(a)[1]
                else:
                    env.env.real_env.reset()
                    env.env.real_env.env.state = env.env.real_env.env._obs_to_state(s)
                    env.env.state = s
                    out[s, a] = env.env.step(a)[1]
    return out


def record(script, mode, seed, vary_seed, env_over):
    import ConfigSpace
    import gym.spaces as gspaces
    mod = load_script(script)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "model.pt")
        write_checkpoint(path, seed, mode, env_over)
        with gg.quiet():
            reward_env, real_env, config = mod.load_envs_and_config(path)
        ckpt = open(path, "rb").read()
    real = mode in ("0", "-1")
    env = real_env if real else reward_env                                        # eval_base / eval_models
    theta = gg.pack_linear_only(reward_env.state_dict(), "env.reward_net.")
    agents, state = [], dict(active=False, testing=False, cur=None, last_explored=0)
    orig_random, orig_sample, orig_select = random.random, gspaces.Discrete.sample, mod.select_agent

    def rec_random():
        v = orig_random()
        if state["active"]:
            agents[-1]["eps"].append(v)
        return v

    def rec_sample(self):
        v = orig_sample(self)
        if state["active"]:
            agents[-1]["act"].append(v)
        return v

    def rec_select(config, agent_name):
        state["active"] = False                   # (building an agent draws nothing; were it to, the draw would not be the agent's)
        agent = orig_select(config=config, agent_name=agent_name)
        state["active"] = True
        agents.append(dict(agent=agent, name=agent_name, alpha=float(agent.alpha), gamma=float(agent.gamma), eps=[], act=[], steps=[]))
        orig_test, orig_action = agent.test, agent.select_train_action

        def rec_test(*a, **k):
            state["testing"] = True
            try:
                return orig_test(*a, **k)
            finally:
                state["testing"] = False

        def rec_action(*a, **k):                  # SARSA also selects inside learn: a step's own selection is the last one before env.step
            before = len(agents[-1]["act"])
            out = orig_action(*a, **k)
            state["last_explored"] = 1 if len(agents[-1]["act"]) > before else 0
            return out

        agent.test, agent.select_train_action = rec_test, rec_action
        return agent

    orig_step, orig_reset = env.step, env.reset

    def rec_step(action, state_=None):
        ns, r, d = orig_step(action=action) if state_ is None else orig_step(action=action, state=state_)
        if not state["testing"]:
            agents[-1]["steps"].append(dict(state=state["cur"], action=int(action.item()), explored=state["last_explored"], next_state=int(ns.item()),
                                            reward=float(r.item()), done=float(d.item())))
        state["cur"] = int(ns.item())
        return ns, r, d

    def rec_reset():
        s = orig_reset()
        state["cur"] = int(s.item())
        return s

    env.step, env.reset = rec_step, rec_reset
    random.random, gspaces.Discrete.sample, mod.select_agent = rec_random, rec_sample, rec_select
    try:
        gg.seed_all(seed + 1)
        ConfigSpace.RANDOM.seed(vary_seed)
        state["active"] = True
        with gg.quiet():
            rewards, episode_lengths = mod.train_test_agents(mode=mode, env=env, real_env=real_env, config=config)
        state["active"] = False
    finally:
        random.random, gspaces.Discrete.sample, mod.select_agent = orig_random, orig_sample, orig_select
        env.step, env.reset = orig_step, orig_reset
    assert len(agents) == AGENTS == len(rewards) == len(episode_lengths)
    shaped = np.stack([shaped_table(env, real, a["gamma"]) for a in agents])

    def cat(rows, dtype):
        return np.concatenate([np.asarray(r, dtype).reshape(-1) for r in rows]), np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)

    fx = dict(script=np.array(script), mode=np.array(mode), agent_name=np.array(agents[0]["name"]), seed=np.array(seed), vary_seed=np.array(vary_seed),
              config_json=np.array(json.dumps(config)), theta=theta, hp_alpha=np.array([a["alpha"] for a in agents], np.float64),
              hp_gamma=np.array([a["gamma"] for a in agents], np.float64), shaped_ref=shaped,
              q_table=np.array([a["agent"].q_table for a in agents], np.float64))
    fx["tape_eps_uniform"], fx["tape_eps_offsets"] = cat([a["eps"] for a in agents], np.float64)
    fx["tape_rand_action"], fx["tape_act_offsets"] = cat([a["act"] for a in agents], np.int32)
    for k, dt in (("state", np.int32), ("action", np.int32), ("explored", np.int32), ("next_state", np.int32), ("reward", np.float32), ("done", np.float32)):
        fx["tr_" + k], fx["tr_offsets"] = cat([[s[k] for s in a["steps"]] for a in agents], dt)
    fx["reward_list"], fx["episode_offsets"] = cat([[float(v) for v in r] for r in rewards], np.float64)
    fx["episode_length"], off = cat(episode_lengths, np.int32)
    assert np.array_equal(off, fx["episode_offsets"])
    return fx, ckpt


def agent_slices(fx, i):
    """agent i's arrays of a fixture (tests/test_transfer_gridworld_reference.py carries the same few lines)"""
    def cut(key, off):
        return fx[key][int(fx[off][i]):int(fx[off][i + 1])]
    out = dict(alpha=float(fx["hp_alpha"][i]), gamma=float(fx["hp_gamma"][i]), shaped_ref=fx["shaped_ref"][i], q_table=fx["q_table"][i],
               eps=cut("tape_eps_uniform", "tape_eps_offsets"), act=cut("tape_rand_action", "tape_act_offsets"),
               reward_list=cut("reward_list", "episode_offsets"), episode_length=cut("episode_length", "episode_offsets"))
    for k in ("state", "action", "explored", "next_state", "reward", "done"):
        out["tr_" + k] = cut("tr_" + k, "tr_offsets")
    return out


def oracle_cfg(fx, alpha, gamma):
    from learning_environments_amd.envs.gridworld import transition_tables
    cfgd = json.loads(str(fx["config_json"]))
    cfgd["agents"]["gtn"]["agent_name"] = str(fx["agent_name"])
    tables = transition_tables(cfgd["env_name"])
    over = dict(alpha=alpha, gamma=gamma)
    if str(fx["mode"]) in ("0", "-1"):
        over["reward_env_type"] = 0
    return orc.ql_cfg_from_config(cfgd, tables, rng_mode=1, **over), tables


def own_table_replay_matches(fx):
    """the condition a fixture is written under (module docstring); also prints how far the two tables are apart"""
    ok = True
    for i in range(AGENTS):
        a = agent_slices(fx, i)
        cfg, tables = oracle_cfg(fx, a["alpha"], a["gamma"])
        tapes = orc.make_tapes(a["eps"], a["act"], np.zeros(0, np.int32), np.zeros((0, 4)), np.zeros((0, 4)))
        _, shaped = orc.rn_shaped_rewards(cfg, fx["theta"], tables)
        out = orc.ql_rn_chain(cfg, fx["theta"], tables, tapes=tapes)
        ne = a["reward_list"].size
        same = out["rc"] == 0 and np.array_equal(out["episode_test_mean"][:ne], a["reward_list"]) and np.array_equal(out["episode_len"][:ne], a["episode_length"])
        print("   agent %d: alpha %.4f gamma %.4f, %d steps, %d draws, tables differ in %d of 192 entries (max %.3g), own-table replay %s" %
              (i, a["alpha"], a["gamma"], a["tr_action"].size, a["eps"].size, int((shaped != a["shaped_ref"]).sum()),
               float(np.abs(shaped - a["shaped_ref"]).max()), "equal" if same else "DIFFERS"))
        ok = ok and same
    return ok


def covers(fx):
    a, g = fx["hp_alpha"], fx["hp_gamma"]
    if str(fx["script"]) == "vary_hp" and not (len(set(a)) == AGENTS and len(set(g)) == AGENTS and a.min() < 0.5):
        return False
    # on a reward net: episodes that are walks, not one step into the cliff, and tapes that keep the file small
    if str(fx["mode"]) not in ("0", "-1") and not all(1500 <= agent_slices(fx, i)["tr_action"].size <= 12000 for i in range(AGENTS)):
        return False
    return all(agent_slices(fx, i)["tr_explored"].any() for i in range(AGENTS))


def gen(name, script, mode, seeds, env_over=None, keep_ckpt=None):
    for seed in seeds:
        fx, ckpt = record(script, mode, seed, 7000 + seed, env_over)
        print("%s seed %d:" % (name, seed))
        if not covers(fx) or not own_table_replay_matches(fx):
            print("   not a fixture, next seed")
            continue
        gg.save(name, **fx)
        size = os.path.getsize(os.path.join(gg.OUT, name + ".npz"))
        print("   %d bytes" % size)
        assert size <= 1024 * 1024
        if keep_ckpt:
            with open(os.path.join(gg.OUT, keep_ckpt), "wb") as f:
                f.write(ckpt)
        return
    raise SystemExit("%s: no seed of %s gave a fixture" % (name, list(seeds)))


def main():
    seeds = range(1601, 1641)
    gen("g16a_gridworld_transfer_vary_hp_mode2", "vary_hp", "2", seeds, keep_ckpt="ckpt_cliff_reward_env_reference.pt")
    gen("g16b_gridworld_transfer_vary_hp_mode0", "vary_hp", "0", seeds)
    gen("g16c_gridworld_transfer_vary_hp_mode_minus1", "vary_hp", "-1", seeds)
    # the algo script on a two-hidden-layer tanh net of type 5
    gen("g16d_gridworld_transfer_algo_mode5", "algo", "5", seeds, env_over=dict(hidden_layer=2, activation_fn="tanh"))
    gen("g16e_gridworld_transfer_algo_mode_minus1", "algo", "-1", seeds)


if __name__ == "__main__":
    main()
