#!/usr/bin/env python3
"""Comparison line for the tabular agents on a gridworld VirtualEnv: the reference's own select_agent('QL').train(env=virtual_env,
test_env=real_env) + agent.test(real_env) -- what GTN_Worker.calc_score does for one chain -- on one CPU thread, on the workload of the `ql_se`
row of tools/bench_configs.py: default_config_gridworld.yaml (Cliff, synthetic_env_type 0), 100 training episodes, no early-out, the fitted SE
of the g15a fixture.  MEASUREMENT INFRASTRUCTURE, runs only where the reference is present (it is imported at run time through
oracle/gen_golden.py's helpers); prints one JSON line.

    python tools/time_reference_ql_se.py [train_episodes=100] [agents=3]        # the median over the agents is reported
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402

import torch  # noqa: E402


def main():
    episodes = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    agents = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    import agents.GTN_worker as gw
    from envs.env_factory import EnvFactory
    cfg = gg.load_cfg("default_config_gridworld.yaml")
    cfg["device"] = "cpu"
    cfg["agents"]["gtn"]["synthetic_env_type"] = 0
    cfg["agents"]["ql"].update(train_episodes=episodes, print_rate=int(1e9))
    cfg["envs"]["Cliff"]["solved_reward"] = 1e9
    theta = np.load(os.path.join(ROOT, "tests", "golden", "g15a_ql_se_cliff_ql.npz"))["theta"]
    torch.set_num_threads(1)
    times, steps = [], []
    with gg.quiet():
        gg.seed_all(1)
        fac = EnvFactory(cfg)
        venv, real_env = fac.generate_virtual_env(), fac.generate_real_env()
        off = 0
        with torch.no_grad():                       # theta = state_net | reward_net | done_net, the nn.Linear parameters in module order
            for net in (venv.env.state_net, venv.env.reward_net, venv.env.done_net):
                for m in net.modules():
                    if isinstance(m, torch.nn.Linear):
                        for p in (m.weight, m.bias):
                            p.copy_(torch.from_numpy(theta[off:off + p.numel()]).reshape(p.shape))
                            off += p.numel()
        assert off == theta.size
        for i in range(agents):
            agent = gw.select_agent(config=cfg, agent_name="QL")
            t0 = time.time()
            _, lens, _ = agent.train(env=venv, test_env=real_env)
            agent.test(env=real_env)
            times.append(time.time() - t0)
            steps.append(int(sum(lens)))
    med = sorted(times)[len(times) // 2]
    print(json.dumps({"reference": "QL.train on the fitted Cliff VirtualEnv + test, default_config_gridworld.yaml, 1 CPU thread", "train_episodes": episodes,
                      "agents_timed": agents, "seconds_per_agent_median": med, "agents_per_s": 1.0 / med, "train_steps": steps, "all": times}))


if __name__ == "__main__":
    main()
