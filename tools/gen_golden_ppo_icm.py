#!/usr/bin/env python3
"""Fixtures that pin the PPO + ICM restatement (tests/ppo_icm_ref.c) to the reference's own PPO(icm=True).train / BaseAgent.test.

TEST INFRASTRUCTURE, run on the CPU in the build container like tools/gen_golden_ppo.py, whose taping it repeats: imports the read-only
reference and the gym shims at run time and writes only recorded arrays to tests/golden/g19*_ppo_icm_*.npz -- what the g14 fixtures hold, and
in addition the fresh ICMModel's parameters (icm_init, state-dict order), the module's parameters after every PPO.learn call (learn_icm) and
each call's compute_intrinsic_rewards output (learn_intr, one row per call).  The parameters after the run are those after the last call (only
PPO.learn changes them), so no final rows are stored: every file stays within the size of the largest g14 fixture.

    python tools/gen_golden_ppo_icm.py
"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402  (puts the reference and the shims on sys.path)
from tools.gen_golden_ppo import pack_ppo  # noqa: E402

import torch  # noqa: E402


def pack_icm(agent):
    """ICMModel parameters in state-dict order (features, inverse, forward_pre, residual blocks 1-4, forward_post)"""
    return np.concatenate([v.detach().cpu().numpy().astype(np.float32).reshape(-1) for v in agent.icm.model.state_dict().values()])


def gen(name, seed, cfg_yaml, env_name, env_cls, ppo, env_over, icm, write=True):
    import gym.envs as genvs
    import torch.distributions.normal as tdn
    from agents.PPO import PPO
    from envs.env_factory import EnvFactory
    cfg = gg.load_cfg(cfg_yaml)
    cfg["device"] = "cpu"
    cfg["agents"]["ppo"] = dict(print_rate=int(1e9), rb_size=100000, init_episodes=0, gamma=0.99, vf_coef=1.0, ent_coef=0.01, eps_clip=0.2,
                                early_out_num=3, early_out_virtual_diff=0.02)
    cfg["agents"]["ppo"].update(ppo)
    cfg["agents"]["icm"] = dict(icm)
    cfg["envs"][env_name].update(env_over)
    cfg["envs"][env_name]["solved_reward"] = 1e9
    rec = dict(learn_icm=[], learn_intr=[], std_seen=[], act_noise=[], test_noise=[], resets=[], steps=[], learn_step=[], learn_params=[], testing=False, active=False)
    env_class = getattr(genvs, env_cls)
    orig_normal, orig_reset = tdn._standard_normal, env_class.reset

    def rec_normal(shape, dtype, device):
        v = orig_normal(shape, dtype=dtype, device=device)
        if rec["active"]:
            rec["test_noise" if rec["testing"] else "act_noise"].append(v.numpy().copy().reshape(-1))
        return v

    def rec_reset(self):
        obs = orig_reset(self)
        if rec["active"]:
            rec["resets"].append((id(self), np.array(self.state, np.float64).copy()))
        return obs

    with gg.quiet():
        gg.seed_all(seed)
        fac = EnvFactory(cfg)
        env = fac.generate_reward_env()
        real_env = fac.generate_real_env()
        with torch.no_grad():              # a trained-looking reward net: the default init gives potentials of a few 1e-2
            for p in env.env.reward_net.parameters():
                if p.dim() == 2:
                    p.mul_(1.5)
        theta = gg.pack_linear_only(env.state_dict(), "env.reward_net.") if cfg["envs"][env_name]["reward_env_type"] != 0 else np.zeros(1, np.float32)
        agent = PPO(env=env, config=cfg, icm=True)
        agent_init = pack_ppo(agent)
        icm_init = pack_icm(agent)
        orig_intr = agent.icm.compute_intrinsic_rewards

        def rec_intr(states, next_states, actions):
            r = orig_intr(states, next_states, actions)
            rec["learn_intr"].append(r.detach().numpy().astype(np.float32).reshape(-1).copy())
            return r
        agent.icm.compute_intrinsic_rewards = rec_intr
        orig_step, orig_learn, orig_test, orig_evaluate = env.step, agent.learn, agent.test, agent.actor.evaluate

        def rec_evaluate(states, actions):        # action_std as each epoch's log-probabilities see it (before evaluate's clamp)
            rec["std_seen"].append(agent.actor.action_std.detach().numpy().astype(np.float32).copy())
            return orig_evaluate(states, actions)
        agent.actor.evaluate = rec_evaluate

        def rec_step(action, state=None):
            s_before = np.asarray(env.env.state, np.float64).astype(np.float32)
            ns, r, d = orig_step(action=action, state=state)
            rec["steps"].append(dict(state=s_before, action=action.detach().numpy().astype(np.float32).reshape(-1).copy(),
                                     next_state=ns.detach().numpy().astype(np.float32).copy(), reward=float(r.item()), done=float(d.item())))
            return ns, r, d

        def rec_learn(rb):
            orig_learn(rb)
            rec["learn_step"].append(len(rec["steps"]))
            rec["learn_params"].append(pack_ppo(agent))
            rec["learn_icm"].append(pack_icm(agent))

        def rec_test(*a, **k):
            rec["testing"] = True
            try:
                return orig_test(*a, **k)
            finally:
                rec["testing"] = False

        env.step, agent.learn, agent.test = rec_step, rec_learn, rec_test
        tdn._standard_normal, env_class.reset = rec_normal, rec_reset
        train_reset_id = id(env.env.real_env.unwrapped)
        try:
            rec["active"] = True
            reward_list_train, episode_length_train, _ = agent.train(env=env, test_env=real_env)
            reward_list_test, _, _ = agent.test(env=real_env)
            rec["active"] = False
        finally:
            tdn._standard_normal, env_class.reset = orig_normal, orig_reset
    A = rec["act_noise"][0].size
    if not write:
        return rec
    rows = max(r.size for r in rec["learn_intr"])
    gg.save(name, config_json=np.array(json.dumps(cfg)), theta=theta, agent_init=agent_init, icm_init=icm_init,
            learn_icm=np.stack(rec["learn_icm"]).astype(np.float32),
            learn_intr=np.stack([np.pad(r, (0, rows - r.size)) for r in rec["learn_intr"]]).astype(np.float32),
            tape_act_noise=np.stack(rec["act_noise"]).astype(np.float32).reshape(-1, A),
            tape_test_noise=np.stack(rec["test_noise"]).astype(np.float32).reshape(-1, A),
            tape_train_reset=np.array([s for (i, s) in rec["resets"] if i == train_reset_id]),
            tape_test_reset=np.array([s for (i, s) in rec["resets"] if i != train_reset_id]),
            tr_state=np.stack([s["state"] for s in rec["steps"]]), tr_action=np.stack([s["action"] for s in rec["steps"]]),
            tr_next_state=np.stack([s["next_state"] for s in rec["steps"]]), tr_reward=np.array([s["reward"] for s in rec["steps"]], np.float32),
            tr_done=np.array([s["done"] for s in rec["steps"]], np.float32),
            learn_step=np.array(rec["learn_step"], np.int32), learn_params=np.stack(rec["learn_params"]).astype(np.float32),
            std_seen=np.stack(rec["std_seen"]).astype(np.float32),
            reward_list_train=np.array(reward_list_train, np.float64), episode_length_train=np.array(episode_length_train, np.int32),
            reward_list_test=np.array(reward_list_test, np.float64), score=np.array(statistics.mean(reward_list_test)))


def main():
    small = dict(train_episodes=6, test_episodes=2, ppo_epochs=4, lr=3e-3, hidden_size=24, hidden_layer=2, activation_fn="relu", action_std=0.5)
    # the reference's default beta / eta: the intrinsic term is not negligible next to the shaped reward
    icm_a = dict(lr=1e-3, beta=0.2, eta=0.5, feature_dim=8, hidden_size=16)
    icm_b = dict(lr=1e-3, beta=0.2, eta=0.5, feature_dim=5, hidden_size=24)
    icm_c = dict(lr=1e-3, beta=0.2, eta=0.5, feature_dim=4, hidden_size=8)       # (the stand-in's 17 + 6 inputs: a small module and 20-wide agent nets keep the file small)
    icm_d = dict(lr=1e-3, beta=0.2, eta=0.5, feature_dim=5, hidden_size=12)
    # the g14p / g14c / g14h settings: 28 rows firing mid-episode; same_action_num 5; A = 6 on the real env itself
    gen("g19p_ppo_icm_pendulum_type2", 1901, "default_config_pendulum_reward_env.yaml", "Pendulum-v0", "PendulumEnv",
        dict(small, update_episodes=2.5, same_action_num=1), dict(max_steps=11, hidden_size=16, reward_env_type=2), icm_a)
    gen("g19c_ppo_icm_cmc_type5_k5", 1902, "default_config_cmc_reward_env.yaml", "MountainCarContinuous-v0", "Continuous_MountainCarEnv",
        dict(small, update_episodes=1.5, same_action_num=5, activation_fn="tanh", hidden_layer=1), dict(max_steps=40, hidden_size=16, reward_env_type=5),
        icm_b)
    gen("g19h_ppo_icm_cheetah_type0", 1903, "default_config_halfcheetah_reward_env.yaml", "HalfCheetah-v3", "CheetahStandinEnv",
        dict(small, update_episodes=2, same_action_num=1, action_std=0.3, activation_fn="leakyrelu", hidden_size=20),
        dict(max_steps=9, hidden_size=16, reward_env_type=0),
        icm_c)
    # learn calls of 131 rows: more than two 64-deep stages of the weight-gradient reductions, the stacked 262 feature rows more than one
    # 256-row block
    gen("g19r_ppo_icm_pendulum_131_rows", 1904, "default_config_pendulum_reward_env.yaml", "Pendulum-v0", "PendulumEnv",
        dict(small, test_episodes=1, ppo_epochs=3, update_episodes=2.6, same_action_num=1), dict(max_steps=50, hidden_size=16, reward_env_type=2), icm_d)


if __name__ == "__main__":
    main()
