#!/usr/bin/env python3
"""Fixtures that pin the restatement of the tabular agents on a gridworld VirtualEnv (tests/ql_se_ref.c) to the reference's own
QL.train / SARSA.train on a VirtualEnv and BaseAgent.test on the real grid.

TEST INFRASTRUCTURE, run on the CPU in the build container: imports the read-only reference and the gym shims at run time (through
oracle/gen_golden.py's helpers) and writes only recorded arrays to tests/golden/g15*_ql_se_*.npz -- random.random and
action_space.sample taped, per SE step the raw outputs of the three nets, per agent step the agent-visible states, the action and whether it
was explored, per run reward_list / episode_length of train, the final test returns, the final Q-table, theta and the config.

A randomly initialised SE never ends an episode (its done output stays below 0.5), so each fixture's SE is first FITTED here, with a few
hundred Adam steps, to the real grid's transition tables (inputs [one_hot(a) | one_hot(s)], targets one-hot next state | reward | done).

The generator runs reference and restatement side by side and writes a fixture only when the conditions that keep the comparison honest
hold (check_conditions below, asserted again by tests/test_ql_se_reference.py); otherwise it tries the next seed.  It prints the measured
deviations the test's tolerances are derived from.

    python tools/gen_golden_ql_se.py
"""
import json
import os
import random
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import gen_golden as gg  # noqa: E402  (puts the reference and the shims on sys.path)

import torch  # noqa: E402

from learning_environments_amd import _lib  # noqa: E402
from learning_environments_amd.config import ql_se_cfg_from_config  # noqa: E402
from learning_environments_amd.envs.gridworld import transition_tables  # noqa: E402

from ql_se_ref import Unfit, check_conditions, measure  # noqa: E402  (the conditions live next to the restatement: the test asserts them too)


def fit_se(venv, tables, steps, lr=1e-2, reward_weight=1e-2):
    """Adam on the three nets against the real grid's tables: every (s, a) pair, full batch, MSE."""
    N, A = tables["n_states"], tables["n_actions"]
    x = torch.zeros((N * A, A + N))
    ty, tr, td = torch.zeros((N * A, N)), torch.zeros((N * A, 1)), torch.zeros((N * A, 1))
    for s in range(N):
        for a in range(A):
            i = s * A + a
            x[i, a] = 1.0
            x[i, A + s] = 1.0
            ty[i, int(tables["next_state"][s, a])] = 1.0
            tr[i, 0] = float(tables["reward"][s, a])
            td[i, 0] = float(tables["done"][s, a])
    env = venv.env
    opt = torch.optim.Adam(list(env.state_net.parameters()) + list(env.reward_net.parameters()) + list(env.done_net.parameters()), lr=lr)
    for _ in range(steps):
        opt.zero_grad()
        loss = ((env.state_net(x) - ty) ** 2).mean() + ((env.reward_net(x) - tr) ** 2).mean() * reward_weight + ((env.done_net(x) - td) ** 2).mean()
        loss.backward()
        opt.step()
    for p in env.parameters():
        p.requires_grad_(False)


def se_theta(venv):
    sd = venv.state_dict()
    return np.concatenate([gg.pack_linear_only(sd, "env.%s." % n) for n in ("state_net", "reward_net", "done_net")])


def record(seed, env_name, agent_name, fit_steps, agent_over, env_over=None, test_mode=0, fit_kw=None):
    import agents.GTN_worker as gw
    import gym.spaces as gspaces
    from envs.env_factory import EnvFactory
    cfg = gg.load_cfg("default_config_gridworld.yaml")
    cfg["env_name"], cfg["device"] = env_name, "cpu"
    cfg["agents"]["gtn"].update(synthetic_env_type=0, agent_name=agent_name)
    sec = "sarsa" if agent_name.lower().startswith("sarsa") else "ql"
    cfg["agents"][sec]["print_rate"] = int(1e9)
    cfg["agents"][sec].update(agent_over)
    cfg["envs"][env_name].update(env_over or {})
    tables = transition_tables(env_name)
    N = tables["n_states"]
    rec = dict(active=False, eps=[], act=[], se=[], steps=[], reset=True)
    orig_random, orig_sample = random.random, gspaces.Discrete.sample

    def rec_random():
        v = orig_random()
        if rec["active"]:
            rec["eps"].append(v)
        return v

    def rec_sample(self):
        v = orig_sample(self)
        if rec["active"]:
            rec["act"].append(v)
        return v

    with gg.quiet():
        gg.seed_all(seed)
        fac = EnvFactory(cfg)
        venv, real_env = fac.generate_virtual_env(), fac.generate_real_env()
        fit_se(venv, tables, fit_steps, **(fit_kw or {}))
        theta = se_theta(venv)
        agent = gw.select_agent(config=cfg, agent_name=agent_name)
        orig_wstep, orig_vstep, orig_reset = venv.step, venv.env.step, venv.reset

        def rec_vstep(action, state=None):
            ns, r, d = orig_vstep(action=action, state=state)
            rec["se"].append(dict(action=int(torch.argmax(action)), ns=ns.detach().numpy().astype(np.float32).copy(), r=float(r.item()), d=float(d.item()),
                                  reset=rec["reset"]))
            rec["reset"] = False
            return ns, r, d

        def rec_wstep(action, state=None):
            s_before = int(torch.argmax(venv.env.state))
            ns, r, d = orig_wstep(action=action, state=state)
            rec["steps"].append(dict(state=s_before, action=int(action.item()), next_state=int(ns.item()), reward=float(r.item()), done=float(d.item()),
                                     n_rand=len(rec["act"]), se_index=len(rec["se"]) - 1))
            return ns, r, d

        def rec_reset():
            rec["reset"] = True
            return orig_reset()

        venv.step, venv.env.step, venv.reset = rec_wstep, rec_vstep, rec_reset
        random.random, gspaces.Discrete.sample = rec_random, rec_sample
        try:
            rec["active"] = True
            if test_mode == 1:
                reward_list_train, episode_length_train, _ = agent.train(env=venv)
            else:
                reward_list_train, episode_length_train, _ = agent.train(env=venv, test_env=real_env)
            reward_list_test, _, _ = agent.test(env=real_env)
            rec["active"] = False
        finally:
            random.random, gspaces.Discrete.sample = orig_random, orig_sample
    explored, prev = np.zeros(len(rec["steps"]), np.int32), 0
    for k, st in enumerate(rec["steps"]):
        # a sample drawn since the previous step (QL / QL_cb; SARSA also draws inside learn: sarsa_explored below replaces the flags)
        explored[k] = 1 if st["n_rand"] > prev else 0
        prev = st["n_rand"]
    fx = dict(config_json=np.array(json.dumps(cfg)), theta=theta, test_mode=np.array(test_mode, np.int32),
              tape_eps_uniform=np.array(rec["eps"], np.float64), tape_rand_action=np.array(rec["act"], np.int32),
              se_action=np.array([s["action"] for s in rec["se"]], np.int32), se_reset=np.array([s["reset"] for s in rec["se"]], np.uint8),
              se_next_state=np.stack([s["ns"] for s in rec["se"]]).reshape(-1, N), se_reward=np.array([s["r"] for s in rec["se"]], np.float32),
              se_done=np.array([s["d"] for s in rec["se"]], np.float32),
              tr_state=np.array([s["state"] for s in rec["steps"]], np.int32), tr_action=np.array([s["action"] for s in rec["steps"]], np.int32),
              tr_explored=explored, tr_next_state=np.array([s["next_state"] for s in rec["steps"]], np.int32),
              tr_reward=np.array([s["reward"] for s in rec["steps"]], np.float32), tr_done=np.array([s["done"] for s in rec["steps"]], np.float32),
              tr_se_index=np.array([s["se_index"] for s in rec["steps"]], np.int64),
              q_table=np.array(agent.q_table, np.float64), reward_list_train=np.array([float(v) for v in reward_list_train], np.float64),
              episode_length_train=np.array(episode_length_train, np.int32), reward_list_test=np.array(reward_list_test, np.float64),
              score=np.array(statistics.mean(reward_list_test)))
    return cfg, tables, fx


def sarsa_explored(fx, cfg):
    """SARSA draws inside learn too (one select_train_action per batch element), so 'a sample was drawn since the last step' does not tell whether the
    step's own action was explored.  Replay the tape positions: the step's own select comes first, then batch_size selects in learn."""
    eps, act = fx["tape_eps_uniform"], fx["tape_rand_action"]
    out = np.zeros(len(fx["tr_action"]), np.int32)
    ie = ia = 0
    eps_g, ep, lens = None, 0, fx["episode_length_train"]
    k_rep = max(1, cfg.same_action_num)
    left = 0
    for k in range(len(out)):
        if left == 0:
            eps_g = cfg.eps_init if ep == 0 else max(eps_g * cfg.eps_decay, cfg.eps_min)
            left = int(lens[ep]) // k_rep
            cur_ep, ep = ep, ep + 1
        if eps[ie] < eps_g:
            out[k] = 1
            ia += 1
        ie += 1
        if cur_ep >= cfg.init_episodes:
            for _ in range(cfg.batch_size):
                if eps[ie] < eps_g:
                    ia += 1
                ie += 1
        left -= 1
    assert ie == len(eps) and ia == len(act), (ie, len(eps), ia, len(act))
    return out


def gen(name, seeds, env_name, agent_name, fit_steps, agent_over, env_over=None, test_mode=0, expect=None):
    """Try the seeds in order until the conditions hold, then write the fixture; returns its measurement."""
    for seed in seeds:
        cfg_dict, tables, fx = record(seed, env_name, agent_name, fit_steps, agent_over, env_over, test_mode)
        cfg = ql_se_cfg_from_config(cfg_dict, tables, rng_mode=_lib.RNG_TAPE, test_mode=test_mode)
        if cfg.agent_kind == 1:
            fx["tr_explored"] = sarsa_explored(fx, cfg)
        try:
            m = measure(fx, cfg, tables)
            check_conditions(m)
            if expect is not None:
                expect(fx, cfg, m)
        except Unfit as e:
            print("%s seed %d: not a fixture: %s" % (name, seed, e))
            continue
        lens_, k_ = fx["episode_length_train"], max(1, cfg.same_action_num)
        last_done = fx["tr_done"][np.cumsum(lens_ // k_) - 1]                     # the done output of every episode's last step
        m["coverage"] = dict(ends_on_done=bool(((lens_ < cfg.max_steps) & (last_done > 0.5)).any()), runs_to_max_steps=bool((lens_ >= cfg.max_steps).any()),
                             explored=bool(fx["tr_explored"].any()), greedy=bool((fx["tr_explored"] == 0).any()))
        fx["seed"] = np.array(seed)
        gg.save(name, **fx)
        lens, done_hi = fx["episode_length_train"], float((fx["tr_done"] > 0.5).mean())
        print("%s seed %d: %d agent steps, %d episodes (lengths %d..%d), done > 0.5 on %.0f %% of the steps, explored %d" %
              (name, seed, len(fx["tr_action"]), len(lens), lens.min(), lens.max(), 100 * done_hi, int(fx["tr_explored"].sum())))
        for kind in ("tf", "fr"):
            print("   %s: " % ("teacher-forced" if kind == "tf" else "free-running ") + ", ".join(
                "%s %.3g (%.2f spacings at %.3g)" % (q, v, v / np.spacing(np.float32(m["mags"][q])), m["mags"][q]) for q, v in m[kind].items()))
        print("   gaps: " + ", ".join("%s %.3g" % kv for kv in m["gaps"].items()))
        return m
    raise SystemExit("%s: no seed of %s gave a fixture" % (name, list(seeds)))


def main():
    def ends_early(fx, cfg, m):
        if len(fx["episode_length_train"]) >= cfg.train_episodes:
            raise Unfit("the run did not leave by the early-out")

    seeds = range(1501, 1541)
    # (a) Cliff + QL at the YAML shape (32 x 1 leakyrelu)
    ms = {}
    ms["a"] = gen("g15a_ql_se_cliff_ql", seeds, "Cliff", "QL", 1500, dict(train_episodes=20, eps_init=0.2, eps_min=0.05, eps_decay=0.9))
    # (b) HoleRoomLarge + SARSA, two hidden layers, batch_size 2.  The fitted two-layer SE amplifies a deviation of its fed-back state about
    # threefold per step (measured: 2e-7 after one step, 1e-4 after eight, 1e-2 after fifteen), so the episodes are kept at eight steps
    ms["b"] = gen("g15b_ql_se_holeroom_sarsa", seeds, "HoleRoomLarge", "SARSA", 1500,
        dict(train_episodes=25, batch_size=2, eps_init=0.3, eps_min=0.05, eps_decay=0.9, init_episodes=2), dict(hidden_layer=2, max_steps=8))
    # (c) EmptyRoom33 + QL_cb leaving by the real early-out
    ms["c"] = gen("g15c_ql_se_emptyroom33_qlcb", seeds, "EmptyRoom33", "QL_cb", 150, dict(train_episodes=40, eps_init=0.2, eps_min=0.05, eps_decay=0.9, early_out_num=3),
        expect=ends_early)
    # (d) Cliff + QL, same_action_num 2, tanh
    ms["d"] = gen("g15d_ql_se_cliff_ql_k2_tanh", seeds, "Cliff", "QL", 1500, dict(train_episodes=15, same_action_num=2, eps_init=0.2, eps_min=0.05, eps_decay=0.9),
        dict(activation_fn="tanh"))
    # (e) train(env) without a test env (test_mode 1): EmptyRoom33 + QL leaving by the VIRTUAL early-out rule
    ms["e"] = gen("g15e_ql_se_emptyroom33_virtual_early_out", seeds, "EmptyRoom33", "QL", 200,
        dict(train_episodes=80, eps_init=0.1, eps_min=0.1, early_out_num=5, early_out_virtual_diff=0.02), test_mode=1, expect=ends_early)

    # over the set: an episode that ends on done > 0.5 before max_steps, one that runs to max_steps, explored and greedy actions
    short = any(m["coverage"]["ends_on_done"] for m in ms.values())
    full = any(m["coverage"]["runs_to_max_steps"] for m in ms.values())
    assert short and full and any(m["coverage"]["explored"] for m in ms.values()) and any(m["coverage"]["greedy"] for m in ms.values()), \
        {k: m["coverage"] for k, m in ms.items()}
    # what tests/test_ql_se_reference.py derives its tolerances from: the worst deviation over the fixtures in spacings of the quantity's magnitude
    for kind in ("tf", "fr"):
        worst = {}
        for m in ms.values():
            for q, v in m[kind].items():
                worst[q] = max(worst.get(q, 0.0), v / float(np.spacing(np.float32(m["mags"][q]))))
        print("worst %s deviation over the fixtures, in spacings: " % ("teacher-forced" if kind == "tf" else "free-running") +
              ", ".join("%s %.2f" % kv for kv in worst.items()))


if __name__ == "__main__":
    main()
