"""The evaluation harness as an experiment runs it (reference experiments/syn_env_evaluate_cartpole_vary_hp_2.py __main__: 40 models x 10
DDQN_vary agents per mode): run_vary_hp with all models in ONE fused launch against the model-by-model calls the reference's loop makes.
Models: CartPole SEs of default_config_cartpole.yaml's shape whose reward net says ~1 per step (a stand-in for trained SEs: 200-step episodes,
the virtual early-out after 20-30 episodes).  usage: python tools/bench_harness.py [model_num] [agents_num] [agent] [mode]
agent = ppo_transfer: the reward-net transfer experiment (experiments/GTNC_evaluate_cmc_transfer_algo.py: 10 models x 10 PPO agents per mode) at the
script's PPO settings on a reduced episode budget ([mode] = training episodes per agent, default 40), all models in one launch; models =
freshly initialised MountainCarContinuous reward nets of default_config_cmc_reward_env.yaml's shape (a stand-in for trained ones).
agent = gridworld_transfer: the gridworld reward-net transfer experiment (experiments/GTNC_evaluate_gridworld_transfer_vary_hp.py: 10 models x 10 QL
agents per mode, every agent with its own alpha / gamma) at the script's size (500 episodes), all models in ONE launch of
lenv_ql_rn_inner_loop_hp ([mode] = the script's mode, default 2), and in the same run the same agents as model_num x agents_num single-chain
launches of lenv_ql_rn_inner_loop, each with its own cfg -- the only way a heterogeneous population runs without the per-chain entry.  Medians
of 7.  Models = freshly initialised Cliff reward nets with the weight matrices scaled by 1.5 (a stand-in for trained ones)."""
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learning_environments_amd.experiments import syn_env_run_vary_hp as rv                      # noqa: E402
from learning_environments_amd.experiments.syn_env_evaluate import load_envs_and_config, train_test_agents   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def ppo_transfer(model_num, agents_num, episodes):
    import copy
    from learning_environments_amd.envs.env_factory import EnvFactory
    from learning_environments_amd.experiments import transfer_algo as ta
    env_name = "MountainCarContinuous-v0"
    base = ta.base_config(env_name)
    envs = []
    for m in range(model_num):
        torch.manual_seed(100 + m)
        envs.append(EnvFactory(copy.deepcopy(base)).generate_reward_env())
    real_env = EnvFactory(copy.deepcopy(base)).generate_real_env()
    settings = dict(train_episodes=episodes)
    ta.train_test_agents_models("2", envs[:1], real_env, copy.deepcopy(base), env_name, agents_num=1, settings=dict(train_episodes=11))       # warm-up
    torch.cuda.synchronize()
    times = []
    for rep in range(3):
        t0 = time.time()
        _, launch = ta.train_test_agents_models("2", envs, real_env, copy.deepcopy(base), env_name, agents_num=agents_num, seed=rep, settings=settings,
                                                details=True)
        torch.cuda.synchronize()
        times.append(time.time() - t0)
    st = launch["inner"].stats.cpu().numpy()
    dt = sorted(times)[1]
    cfg = launch["task"].cfg
    W = 2 * (cfg.state_dim * cfg.hidden + (cfg.layers - 1) * cfg.hidden * cfg.hidden) + cfg.action_dim * cfg.hidden + cfg.hidden
    rows = launch["inner"].rows
    epochs = float(st[:, 2].sum()) * cfg.ppo_epochs
    import bench
    busy = min(st.shape[0], 256)
    print(json.dumps({"experiment": "ppo transfer, mode 2", "models": model_num, "agents": int(st.shape[0]), "train_episodes": episodes,
                      "seconds_median_of_3": dt, "seconds_all": times, "agents_per_s": st.shape[0] / dt, "rows_per_learn": rows,
                      "learn_calls": int(st[:, 2].sum()), "us_per_learn_epoch_per_chain": 1e6 * dt / max(1.0, epochs / st.shape[0]),
                      "mfma_f32_frac_of_busy_cus": 6.0 * rows * W * epochs / dt / 1e12 / (bench.MFMA_F32_PEAK_TFLOPS * busy / 256.0)}))


def gridworld_transfer(model_num, agents_num, mode):
    import copy
    import numpy as np
    from learning_environments_amd import _lib, configs, engine
    from learning_environments_amd.envs.env_factory import EnvFactory
    from learning_environments_amd.experiments import transfer_gridworld as tg
    base = configs.cliff_reward_env_ql()
    base["envs"]["Cliff"].update(solved_reward=tg.SOLVED_REWARD, reward_env_type=int(mode) if int(mode) > 0 else 2)
    real_env = EnvFactory(copy.deepcopy(base)).generate_real_env()
    envs = []
    for m in range(model_num):
        torch.manual_seed(100 + m)
        env = EnvFactory(copy.deepcopy(base)).generate_reward_env()
        with torch.no_grad():
            for p in env.env.reward_net.parameters():
                if p.dim() == 2:
                    p.mul_(1.5)
        envs.append(env if int(mode) > 0 else real_env)
    tg.train_test_agents_models(mode, envs[:1], real_env, copy.deepcopy(base), agents_num=1, settings=dict(train_episodes=5))       # warm-up
    torch.cuda.synchronize()
    reps = 7

    def median(fn):
        times = []
        for rep in range(reps):
            torch.cuda.synchronize()
            t0 = time.time()
            fn(rep)
            torch.cuda.synchronize()
            times.append(time.time() - t0)
        return sorted(times)[reps // 2], times

    # (1) the whole call: settings, draws, set_hp, one launch, the lists
    res = {}

    def call(rep):
        res["out"], res["launch"] = tg.train_test_agents_models(mode, envs, real_env, copy.deepcopy(base), agents_num=agents_num, seed=0, details=True)
    t_call, all_call = median(call)
    launch = res["launch"]
    inner, chains = launch["inner"], launch["inner"].chains
    keys_t = torch.from_numpy(launch["keys"].view(np.int64)).to(inner.dev)
    # (2) its launch alone
    t_launch, all_launch = median(lambda rep: inner.run(launch["theta"], launch["eps"], launch["worker"], launch["sign"], rng_keys=keys_t))
    st = inner.stats.cpu().numpy()
    fused = (inner.episode_test_mean.cpu().numpy().copy(), inner.episode_len.cpu().numpy().copy(), inner.q_table.cpu().numpy().copy())
    # (3) the same agents as single-chain launches of the plain entry, each with its own cfg (buffers allocated before the clock starts)
    singles = []
    for c in range(chains):
        cfg = _lib.QlCfg.from_buffer_copy(inner.cfg)
        cfg.alpha, cfg.gamma = launch["hp"][c]["alpha"], launch["hp"][c]["gamma"]
        il = engine.QlInnerLoop(cfg, 1, real_env.env.tables)
        w = int(launch["worker"][c])
        theta = (launch["eps"][w] if float(launch["sign"][c]) != 0.0 else launch["theta"]).contiguous()
        singles.append((il, theta, keys_t[c:c + 1].contiguous()))

    def run_singles(rep):
        for il, theta, k in singles:
            il.run(theta, None, None, None, rng_keys=k)
    t_single, all_single = median(run_singles)
    for c, (il, _, _) in enumerate(singles):                  # the same agents: the same runs
        assert np.array_equal(il.episode_test_mean[0].cpu().numpy(), fused[0][c], equal_nan=True) and np.array_equal(il.episode_len[0].cpu().numpy(), fused[1][c])
        assert np.array_equal(il.q_table[0].cpu().numpy(), fused[2][c])
    print(json.dumps({"experiment": "gridworld transfer (vary_hp script), mode %s" % mode, "models": model_num, "agents": chains,
                      "train_episodes": int(inner.cfg.train_episodes), "train_steps": int(st[:, 1].sum()), "test_steps": int(st[:, 3].sum()),
                      "seconds_call_median_of_7": t_call, "seconds_launch_median_of_7": t_launch,
                      "seconds_single_chain_launches_median_of_7": t_single, "agents_per_s_call": chains / t_call,
                      "agents_per_s_launch": chains / t_launch, "agents_per_s_single_chain_launches": chains / t_single,
                      "single_over_fused_launch": t_single / t_launch, "all_call": all_call, "all_launch": all_launch, "all_single": all_single}))


def main():
    if len(sys.argv) > 3 and sys.argv[3] == "gridworld_transfer":
        return gridworld_transfer(int(sys.argv[1]), int(sys.argv[2]), sys.argv[4] if len(sys.argv) > 4 else "2")
    if len(sys.argv) > 3 and sys.argv[3] == "ppo_transfer":
        return ppo_transfer(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[4]) if len(sys.argv) > 4 else 40)
    model_num = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    agents_num = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    agent = sys.argv[3] if len(sys.argv) > 3 else None      # a sibling script's agent (DuelingDDQN_vary, td3_discrete_vary): fused launch only
    agent_mode = int(sys.argv[4]) if len(sys.argv) > 4 else 2   # its run_vary_hp mode (0: the agents train on the real env)
    base = torch.load(os.path.join(HERE, "..", "tests", "golden", "ckpt_cartpole_se_reference_b.pt"), map_location="cpu", weights_only=False)
    d = tempfile.mkdtemp(prefix="lenv_harness_")
    gen = torch.Generator().manual_seed(1)
    for m in range(model_num):
        sd = {k: (v + 0.01 * torch.randn(v.shape, generator=gen)) if v.dtype.is_floating_point else v for k, v in base["model"].items()}
        cfg = json.loads(json.dumps(base["config"]))
        cfg["envs"]["CartPole-v0"].update(max_steps=200, solved_reward=195.0)
        cfg["agents"]["ddqn_vary"]["vary_hp"] = True
        torch.save({"model": sd, "config": cfg}, os.path.join(d, "CartPole-v0_%d_%06d.pt" % (m, m)))
    from learning_environments_amd.experiments import syn_env_evaluate as se
    if agent is not None:
        from functools import partial
        if agent == "generalization_gap":                     # the *_eval_generalization_gap script: fixed optimised DDQN = the headline kernel's shape
            fn = se.train_test_agents_generalization_gap
        else:
            fn = partial(train_test_agents, agent_name=agent)
            fn.fused = partial(se.train_test_agents_models, agent_name=agent)
        if agent.lower() == "td3_discrete_vary":            # the script takes this section from default_config_cartpole.yaml (`td3_discrete_vary_layer_norm_2`)
            sect = {"train_episodes": 1000, "test_episodes": 10, "init_episodes": 10, "batch_size": 128, "gamma": 0.99, "lr": 5e-4, "tau": 0.01,
                    "policy_delay": 2, "rb_size": 1000000, "same_action_num": 1, "activation_fn": "tanh", "hidden_size": 128, "hidden_layer": 2,
                    "action_std": 0.1, "policy_std": 0.2, "policy_std_clip": 0.5, "print_rate": 1, "early_out_num": 10, "early_out_virtual_diff": 1e-2,
                    "gumbel_softmax_temp": 1.0, "gumbel_softmax_hard": False, "vary_hp": False, "use_layer_norm": True}

            def load(file_name, model_dir, device):
                v, r, c = load_envs_and_config(file_name, model_dir, device)
                c["agents"]["td3_discrete_vary"] = dict(sect)
                return v, r, c
        else:
            load = load_envs_and_config
        rv.run_vary_hp(agent_mode, "warm", 1, agents_num, d, load, fn, "CartPole", out_dir=d)
        torch.cuda.synchronize()
        t0 = time.time()
        rewards, steps, episodes = rv.run_vary_hp(agent_mode, "b", model_num, agents_num, d, load, fn, "CartPole", out_dir=d)
        torch.cuda.synchronize()
        dt = time.time() - t0
        print(json.dumps({"mode": agent_mode, "agent": agent, "path": "one fused launch", "models": model_num, "agents": model_num * agents_num,
                          "seconds": round(dt, 3), "agents_per_s": round(model_num * agents_num / dt, 2), "train_steps": sum(s_[0] for s_ in steps),
                          "mean_episodes": round(sum(e[0] for e in episodes) / len(episodes), 1)}), flush=True)
        return
    for mode in (2, 2, 0):
        lpt = se.LPT_MIN_CHAINS
        for label, fn in (("one fused launch", train_test_agents), ("one fused launch, launch order = (model, agent) order", train_test_agents),
                          ("model by model", lambda **k: train_test_agents(**k))):
            se.LPT_MIN_CHAINS = 10 ** 9 if "launch order" in label else lpt
            n = model_num
            if label == "model by model":
                n = min(n, 8)                               # (a sample: the loop is model_num times this)
            rv.run_vary_hp(mode, "warm", 1, agents_num, d, load_envs_and_config, fn, "CartPole", out_dir=d)
            torch.cuda.synchronize()
            t0 = time.time()
            rewards, steps, episodes = rv.run_vary_hp(mode, "b", n, agents_num, d, load_envs_and_config, fn, "CartPole", out_dir=d)
            torch.cuda.synchronize()
            dt = time.time() - t0
            tot_steps = sum(s[0] for s in steps)
            print(json.dumps({"mode": mode, "path": label, "models": n, "agents": n * agents_num, "seconds": round(dt, 3),
                              "agents_per_s": round(n * agents_num / dt, 2), "train_steps": tot_steps,
                              "mean_episodes": round(sum(e[0] for e in episodes) / len(episodes), 1),
                              "mean_test_return": round(sum(sum(r) / len(r) for r in rewards) / len(rewards), 1)}), flush=True)


if __name__ == "__main__":
    main()
