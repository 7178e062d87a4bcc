#!/usr/bin/env python3
"""Comparison line for the gridworld reward-net transfer experiment: the reference's own train_test_agents of
experiments/GTNC_evaluate_gridworld_transfer_vary_hp.py (QL agents, each with its own alpha / gamma; 500 episodes) -- or, with `algo`, of
experiments/GTNC_evaluate_gridworld_transfer_algo.py (SARSA) -- for ONE model on one CPU thread; the scripts run it once per model, ten times
per mode.  The model is the reference-written Cliff checkpoint tests/golden/ckpt_cliff_reward_env_reference.pt (reward_env_type 2).
MEASUREMENT INFRASTRUCTURE, runs only where the reference is present (it is imported at run time through oracle/gen_golden.py's helpers, with
the empty `hpbandster` stand-in of tools/gen_golden_gridworld_transfer.py); prints one JSON line.

    python tools/time_reference_gridworld_transfer.py [script=vary_hp] [mode=2] [agents=10]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import gen_golden as gg  # noqa: E402
import gen_golden_gridworld_transfer as ggt  # noqa: E402

import torch  # noqa: E402


def main():
    script = sys.argv[1] if len(sys.argv) > 1 else "vary_hp"
    mode = sys.argv[2] if len(sys.argv) > 2 else "2"
    agents = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    import ConfigSpace
    mod = ggt.load_script(script)
    mod.MODEL_AGENTS = agents
    torch.set_num_threads(1)
    with gg.quiet():
        gg.seed_all(1)
        ConfigSpace.RANDOM.seed(1)
        reward_env, real_env, config = mod.load_envs_and_config(os.path.join(ROOT, "tests", "golden", "ckpt_cliff_reward_env_reference.pt"))
        env = real_env if mode in ("0", "-1") else reward_env
        t0 = time.time()
        rewards, lengths = mod.train_test_agents(mode=mode, env=env, real_env=real_env, config=config)
        dt = time.time() - t0
    print(json.dumps({"reference": "train_test_agents of the gridworld transfer script '%s', mode %s, one model, 1 CPU thread" % (script, mode),
                      "agents": agents, "train_episodes": len(rewards[0]), "train_steps": int(sum(sum(l) for l in lengths)), "seconds_per_model": dt,
                      "agents_per_s": agents / dt, "seconds_per_mode_of_10_models": 10 * dt * 10 / agents}))


if __name__ == "__main__":
    main()
