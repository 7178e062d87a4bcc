#!/usr/bin/env python3
"""Fixtures that pin the PPO restatement (tests/ppo_ref.c) to the reference's own PPO.train / BaseAgent.test.

TEST INFRASTRUCTURE, run on the CPU in the build container: imports the read-only reference and the gym shims at run time (through
oracle/gen_golden.py's helpers) and writes only recorded arrays to tests/golden/g14*_ppo_*.npz -- every draw taped
(torch.distributions' _standard_normal, env resets, the fresh agent), every training row, the step at which each learn call fired and
the parameters after it, the per-episode test means and the final test returns.

    python tools/gen_golden_ppo.py
"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402  (puts the reference and the shims on sys.path)

import torch  # noqa: E402


def pack_ppo(agent):
    """action_std | actor.net | critic.net: state-dict order of Actor_PPO (its own parameter first), then Critic_V"""
    return np.concatenate([agent.actor.action_std.detach().numpy().astype(np.float32).reshape(-1),
                           gg.pack_linear_params(agent.actor.state_dict(), "net."), gg.pack_linear_params(agent.critic.state_dict(), "net.")])


def gen(name, seed, cfg_yaml, env_name, env_cls, ppo, env_over, write=True):
    import gym.envs as genvs
    import torch.distributions.normal as tdn
    from agents.PPO import PPO
    from envs.env_factory import EnvFactory
    cfg = gg.load_cfg(cfg_yaml)
    cfg["device"] = "cpu"
    cfg["agents"]["ppo"] = dict(print_rate=int(1e9), rb_size=100000, init_episodes=0, gamma=0.99, vf_coef=1.0, ent_coef=0.01, eps_clip=0.2,
                                early_out_num=3, early_out_virtual_diff=0.02)
    cfg["agents"]["ppo"].update(ppo)
    cfg["envs"][env_name].update(env_over)
    cfg["envs"][env_name]["solved_reward"] = 1e9
    rec = dict(std_seen=[], act_noise=[], test_noise=[], resets=[], steps=[], learn_step=[], learn_params=[], testing=False, active=False)
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
        agent = PPO(env=env, config=cfg)
        agent_init = pack_ppo(agent)
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
    gg.save(name, config_json=np.array(json.dumps(cfg)), theta=theta, agent_init=agent_init,
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
            reward_list_test=np.array(reward_list_test, np.float64), score=np.array(statistics.mean(reward_list_test)),
            final_params=pack_ppo(agent))


def gen_ckpt():
    """A reference-written reward-net checkpoint ({'model', 'config'}: GTN_Master.save_model's payload) of default_config_cmc_reward_env.yaml's
    RewardEnv at a small width, and what the reference's re-loaded env pays for a few transitions (RewardEnv._calc_reward)."""
    from envs.env_factory import EnvFactory
    env_name = "MountainCarContinuous-v0"
    cfg = gg.load_cfg("default_config_cmc_reward_env.yaml")
    cfg["device"] = "cpu"
    cfg["envs"][env_name].update(hidden_size=32)
    gg.seed_all(1450)
    with gg.quiet():
        env = EnvFactory(cfg).generate_reward_env()
    path = os.path.join(gg.OUT, "ckpt_cmc_reward_env_reference.pt")
    torch.save({'model': env.state_dict(), 'config': cfg}, path)
    sd = torch.load(path)
    with gg.quiet():
        e2 = EnvFactory(sd['config']).generate_reward_env()
    e2.load_state_dict(sd['model'])
    gg.save("ckpt_cmc_reward_env_reference_theta", theta=gg.pack_linear_only(e2.state_dict(), "env.reward_net."),
            reward_env_type=np.array(cfg["envs"][env_name]["reward_env_type"]))
    print("wrote", path, os.path.getsize(path))


def main():
    gen_ckpt()
    small = dict(train_episodes=6, test_episodes=2, ppo_epochs=4, lr=3e-3, hidden_size=24, hidden_layer=2, activation_fn="relu", action_std=0.5)
    # Pendulum-v0, reward_env_type 2: 11 steps per episode, learn every 2.5 episodes (28 rows: fires mid-episode)
    gen("g14p_ppo_pendulum_type2", 1401, "default_config_pendulum_reward_env.yaml", "Pendulum-v0", "PendulumEnv",
        dict(small, update_episodes=2.5, same_action_num=1), dict(max_steps=11, hidden_size=16, reward_env_type=2))
    # MountainCarContinuous-v0, same_action_num 5, reward_env_type 5
    gen("g14c_ppo_cmc_type5_k5", 1402, "default_config_cmc_reward_env.yaml", "MountainCarContinuous-v0", "Continuous_MountainCarEnv",
        dict(small, update_episodes=1.5, same_action_num=5, activation_fn="tanh", hidden_layer=1), dict(max_steps=40, hidden_size=16, reward_env_type=5))
    # the HalfCheetah stand-in (A = 6) on the real env itself (type 0)
    gen("g14h_ppo_cheetah_type0", 1403, "default_config_halfcheetah_reward_env.yaml", "HalfCheetah-v3", "CheetahStandinEnv",
        dict(small, update_episodes=2, same_action_num=1, action_std=0.3, activation_fn="leakyrelu"), dict(max_steps=9, hidden_size=16, reward_env_type=0))
    # action_std just above evaluate's floor of 0.01 and an lr with which Adam pushes it under the floor between epochs: the clamp behind the
    # log-probabilities and the gradient action_std gets in such an epoch (std_seen records what every epoch saw)
    gen("g14s_ppo_pendulum_std_floor", 1409, "default_config_pendulum_reward_env.yaml", "Pendulum-v0", "PendulumEnv",
        dict(small, update_episodes=2, same_action_num=1, action_std=0.0105, lr=4e-3, ppo_epochs=5, ent_coef=0.01), dict(max_steps=10, hidden_size=16, reward_env_type=2))
    # one epoch per learn call and an lr that takes action_std from 0.0102 to under 0.001: the rows after it are acted with forward's floor of
    # 0.001 on actor_old while the actor keeps the smaller value, which the next call's log-probabilities see before evaluate lifts it to 0.01
    gen("g14f_ppo_pendulum_std_forward_floor", 1410, "default_config_pendulum_reward_env.yaml", "Pendulum-v0", "PendulumEnv",
        dict(small, update_episodes=1, same_action_num=1, action_std=0.0102, lr=9.7e-3, ppo_epochs=1, ent_coef=0.01), dict(max_steps=10, hidden_size=16, reward_env_type=2))


if __name__ == "__main__":
    main()
