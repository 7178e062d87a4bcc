#!/usr/bin/env python3
"""Comparison line for the PPO transfer experiment: the reference's own PPO.train(env=reward_env, test_env=real_env) on one CPU thread, at the
MountainCarContinuous transfer script's PPO settings on a reduced episode budget.  TEST / MEASUREMENT INFRASTRUCTURE, runs only where the
reference is present (it is imported at run time through oracle/gen_golden.py's helpers); prints one JSON line.

    python tools/time_reference_ppo.py [train_episodes=40] [agents=3]        # the median over the agents is reported
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402

import torch  # noqa: E402


def main():
    episodes = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    agents = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    from agents.PPO import PPO
    from envs.env_factory import EnvFactory
    from learning_environments_amd.experiments.transfer_algo import PPO_SETTINGS
    env_name = "MountainCarContinuous-v0"
    cfg = gg.load_cfg("default_config_cmc_reward_env.yaml")
    cfg["device"] = "cpu"
    cfg["envs"][env_name]["solved_reward"] = 100000
    cfg["agents"]["ppo"] = dict(PPO_SETTINGS[env_name], train_episodes=episodes, print_rate=int(1e9))
    torch.set_num_threads(1)
    times = []
    with gg.quiet():
        gg.seed_all(1)
        fac = EnvFactory(cfg)
        env, real_env = fac.generate_reward_env(), fac.generate_real_env()
        for i in range(agents):
            agent = PPO(env=env, config=cfg)
            t0 = time.time()
            agent.train(env=env, test_env=real_env)
            times.append(time.time() - t0)
    print(json.dumps({"reference": "PPO.train on the CMC RewardEnv, transfer-script settings, 1 CPU thread", "train_episodes": episodes,
                      "agents_timed": agents, "seconds_per_agent_median": sorted(times)[len(times) // 2], "agents_per_s": 1.0 / sorted(times)[len(times) // 2], "all": times}))


if __name__ == "__main__":
    main()
