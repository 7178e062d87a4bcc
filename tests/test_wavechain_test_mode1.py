"""`test_mode` 1 (BaseAgent.train(env) without a test env, base_agent.py:49-62,134-148: the evaluation harness's training call) in the
wave-chain kernels `dueling_wavechain.hip` and `td3_wavechain.hip`: no per-episode tests, the reward meter holds each episode's TRAINING
return and `env_solved` runs on the training env (the virtual rule on a VirtualEnv, the real rule on a RewardEnv's shaped returns).

Bar: bit for bit against the GEMM-queue kernels (the same inputs through a launch that asks for a step trace, or with kernel_variant
NO_WAVECHAIN) and against the CPU oracle.  Every case asserts the team-size query FIRST: a launch that fell back to the GEMM-queue
kernel would pass the comparisons and prove nothing.  The early-out thresholds were picked with the oracle so that the chains of a launch
stop at different episodes (the members of a team must agree on every break decision, or the launch ends with status -10)."""
import ctypes as C
import copy

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

P_SE_ACROBOT = 3 * (9 * 128 + 128) + (6 + 1 + 1) * 128 + 8       # the three SE nets 9-128-{6,1,1}
P_Q = {"duelingddqn": 67460, "ddqn": 6 * 128 + 128 + 128 * 128 + 128 + 3 * 128 + 3}


@pytest.fixture(scope="module")
def eng():
    from learning_environments_amd import engine
    engine.require_device()
    return engine


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------
# inputs (shared by the tests; the thresholds below were chosen on the CPU with the oracle)
# ---------------------------------------------------------------------------------------------------------------
# (agent, SE done bias) -> (train_episodes E, early_out_virtual_diff): per the oracle the six chains stop at >= 2 distinct episodes, at
# least one before E, and the longest chain takes >= 80 learn steps (the rule can fire from episode init_episodes + early_out_num = 3 on).
# Stops of the six chains per the oracle: dueling/-10: 4 8 4 4 8 6; dueling/0: 8 4 8 7 8 6; ddqn/-10: 4 8 4 4 5 6; ddqn/0: 8 4 6 4 8 6
DDQN_CASES = {("duelingddqn", -10.0): (8, 0.025), ("duelingddqn", 0.0): (8, 0.025), ("ddqn", -10.0): (8, 0.025), ("ddqn", 0.0): (8, 0.025)}
# the two chains the oracle runs in the test: different stops, and with done bias 0 both have episodes the SE ended
DDQN_ORACLE_CHAINS = {("duelingddqn", -10.0): (0, 5), ("duelingddqn", 0.0): (0, 3), ("ddqn", -10.0): (0, 5), ("ddqn", 0.0): (0, 2)}
# env steps: full-length episodes take 40, so training stops in front of episode 5 (200 > 170) -- chains 1, 4, 5 time out there, chains 0, 2, 3
# have left on the virtual rule after 4 episodes
STEP_BUDGET = 170


def ddqn_case(orc, agent, done_bias, E=None, diff=None, step_budget=0):
    """(HIP cfg, oracle cfg, inputs) of a six-chain launch of the published 128-wide Acrobot shape with test_mode 1."""
    from learning_environments_amd import configs
    from learning_environments_amd.agents.nes_common import chain_keys
    from learning_environments_amd.config import ddqn_cfg_from_config
    E0, diff0 = DDQN_CASES[(agent, done_bias)]
    E, diff = E0 if E is None else E, diff0 if diff is None else diff
    make = configs.acrobot_syn_env_duelingddqn if agent == "duelingddqn" else configs.acrobot_syn_env_ddqn
    cfgd = configs.fixed_work(make(2), E)
    cfgd["agents"][agent].update(init_episodes=1, early_out_num=2, early_out_virtual_diff=diff, step_budget=step_budget)
    cfgd["envs"]["Acrobot-v1"]["max_steps"] = 40
    cfg = ddqn_cfg_from_config(cfgd, test_mode=1)
    ocfg = orc.ddqn_cfg_from_config(cfgd, grad_chunk=0, rng_mode=0, test_mode=1)
    assert (cfg.test_mode, cfg.early_out_virtual_diff, cfg.step_budget) == (1, diff, step_budget) == (ocfg.test_mode, ocfg.early_out_virtual_diff, ocfg.step_budget)
    chains = 6
    rng = np.random.RandomState(31)
    theta = (rng.randn(P_SE_ACROBOT) * 0.1).astype(np.float32)
    theta[-1] = done_bias                                         # done net's output bias: -10 = no episode ends early, 0 = the SE ends episodes
    eps = (rng.randn(2, P_SE_ACROBOT) * 0.05).astype(np.float32)
    worker = (np.arange(chains) // 3).astype(np.int32)
    sign = np.tile(np.array([0.0, 1.0, -1.0], np.float32), 2)
    keys = chain_keys(91, 3, worker, np.arange(chains) % 3)
    init = rng.uniform(-0.08, 0.08, (chains, P_Q[agent])).astype(np.float32)
    return cfg, ocfg, dict(theta=theta, eps=eps, worker=worker, sign=sign, keys=keys, init=init, chains=chains)


def ddqn_oracle_chain(orc, ocfg, d, c):
    w = (np.float32(d["sign"][c]) * d["eps"][d["worker"][c]] + d["theta"]).astype(np.float32)
    o = orc.ddqn_se_chain(ocfg, w, d["init"][c], rng_key=int(d["keys"][c]), want_final_online=True)
    assert o["rc"] == 0
    return o


def oracle_chains(fn, orc, ocfg, d, chains):
    """{chain: the oracle's result}, the chains side by side (the oracle is C behind ctypes: the threads run in parallel)."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(len(chains)) as ex:
        return dict(zip(chains, ex.map(lambda c: fn(orc, ocfg, d, c), chains)))


def ddqn_run(eng, cfg, d, trace_cap=0):
    il = eng.InnerLoop(cfg, d["chains"], trace_cap=trace_cap, want_final_online=True)
    il.run(dev(d["theta"]), dev(d["eps"]), dev(d["worker"]), dev(d["sign"]), dev(d["init"]), rng_keys=dev(d["keys"].view(np.int64)))
    torch.cuda.synchronize()
    assert il.status.cpu().tolist() == [0] * d["chains"], il.status.cpu().tolist()
    return [t.cpu().numpy() for t in (il.score, il.stats, il.episode_test_mean, il.episode_len, il.final_returns, il.final_online)]


def assert_ddqn_equals_oracle(out, o, c):
    assert float(out[0][c]) == o["score"], c
    assert out[1][c].tolist() == [o["episodes_run"], o["train_steps"], o["learn_steps"], o["test_steps"]], c
    assert np.array_equal(out[2][c], o["episode_test_mean"], equal_nan=True), c
    assert np.array_equal(out[3][c], o["episode_len"]), c
    assert np.array_equal(out[4][c], o["final_test_returns"]), c
    assert np.array_equal(out[5][c], o["final_online"]), c


# the TD3 cases (td3_case).  Pendulum RewardEnv: the real rule on the shaped training returns (two-episode means between -79 and -256 per the
# oracle) -- the five chains run 6 4 2 6 2 of 6 episodes.  CMC VirtualEnv: the virtual rule -- the chains run 4 5 8 5 8 of 8 episodes.
TD3_SOLVED_REWARD_PENDULUM = -160.0
TD3_CMC_DIFF = 0.02
TD3_ORACLE_CHAINS = {"pendulum_reward_env": (0, 1), "cmc": (0, 4)}         # (cmc chain 4: the learned done flag ends its episodes early)


def td3_case(orc, which, E=None, solved_reward=None, diff=None):
    from learning_environments_amd import _lib, configs
    from learning_environments_amd.agents.nes_common import chain_keys
    if which == "pendulum_reward_env":
        cfgd = configs.fixed_work(configs.pendulum_reward_env_td3(2), 6 if E is None else E)
        env_name = "Pendulum-v0"
        cfgd["agents"]["td3"].update(init_episodes=1, early_out_num=2)
        cfgd["envs"][env_name].update(max_steps=30, solved_reward=TD3_SOLVED_REWARD_PENDULUM if solved_reward is None else solved_reward)
        seed, kseed = 17, 81
    else:
        cfgd = configs.fixed_work(configs.cmc_syn_env_td3(2), 8 if E is None else E)
        env_name = "MountainCarContinuous-v0"
        cfgd["agents"]["td3"].update(init_episodes=1, early_out_num=2, early_out_virtual_diff=TD3_CMC_DIFF if diff is None else diff)
        cfgd["envs"][env_name]["max_steps"] = 41                 # odd: range(0, 41, 2) = 21 agent steps per full-length training episode
        seed, kseed = 28, 84
    o = orc.td3_cfg_from_config(cfgd, rng_mode=0, test_mode=1)
    cfg = _lib.Td3Cfg()
    for f, _ in _lib.Td3Cfg._fields_:
        setattr(cfg, f, getattr(o, f, 0))                         # (team_size / kernel_variant exist only in the HIP cfg)
    S, A = cfg.state_dim, cfg.action_dim
    e = cfgd["envs"][env_name]
    if which == "pendulum_reward_env":
        assert (S, A, cfg.hidden, cfg.layers, cfg.batch_size, cfg.test_episodes, cfg.rn_layers, cfg.policy_delay, cfg.virtual_env) == (3, 1, 128, 2, 192, 10, 2, 1, 0)
        P_env = orc.rn_num_params(2, 3, 0, 128, 2)
    else:
        assert (S, A, cfg.hidden, cfg.layers, cfg.batch_size, cfg.test_episodes, cfg.rn_hidden, cfg.rn_layers, cfg.policy_delay, cfg.same_action_num,
                cfg.virtual_env) == (2, 1, 128, 2, 256, 1, 96, 2, 2, 2, 1)
        P_env = orc.mlp_num_params(orc.mlp_desc(S + A, e["hidden_size"], e["hidden_layer"], S, e["activation_fn"])) + \
            2 * orc.mlp_num_params(orc.mlp_desc(S + A, e["hidden_size"], e["hidden_layer"], 1, e["activation_fn"]))
    assert cfg.test_mode == 1
    chains = 5
    Pa, Pc = orc.td3_param_counts(o)
    rng = np.random.RandomState(seed)
    theta = (rng.randn(P_env) * 0.1).astype(np.float32)
    eps = (rng.randn(2, P_env) * 0.05).astype(np.float32)
    if which == "cmc":
        theta[-1] = 0.4                                           # done net's output bias: the learned done flag ends some episodes early
    worker = (np.arange(chains) // 3).astype(np.int32)
    sign = np.tile(np.array([0.0, 1.0, -1.0], np.float32), 2)[:chains].copy()
    keys = chain_keys(kseed, 2, worker, np.arange(chains) % 3)
    init = rng.uniform(-0.08, 0.08, (chains, Pa + 2 * Pc)).astype(np.float32)
    return cfg, o, dict(theta=theta, eps=eps, worker=worker, sign=sign, keys=keys, init=init, chains=chains)


def td3_oracle_chain(orc, ocfg, d, c):
    w = (np.float32(d["sign"][c]) * d["eps"][d["worker"][c]] + d["theta"]).astype(np.float32)
    o = orc.td3_rn_chain(ocfg, w, d["init"][c], rng_key=int(d["keys"][c]), want_final_params=True)
    assert o["rc"] == 0
    return o


def td3_run(eng, cfg, d, trace_cap=0):
    il = eng.Td3InnerLoop(cfg, d["chains"], trace_cap=trace_cap, want_final_params=True, want_episode_stats=True)
    il.run(dev(d["theta"]), dev(d["eps"]), dev(d["worker"]), dev(d["sign"]), dev(d["init"]), rng_keys=dev(d["keys"].view(np.int64)))
    torch.cuda.synchronize()
    assert il.status.cpu().tolist() == [0] * d["chains"], il.status.cpu().tolist()
    return [t.cpu().numpy() for t in (il.score, il.stats, il.episode_test_mean, il.final_returns, il.final_params, il.episode_len)]


# ---------------------------------------------------------------------------------------------------------------
# 1. team-size queries
# ---------------------------------------------------------------------------------------------------------------
def test_team_size_queries_accept_test_mode_1(eng, orc):
    """The wave-chain kernels take test_mode 1 launches: the team-size queries answer what they answer for test_mode 0 (they said 1 while
    these launches fell back to the GEMM-queue kernels), and team_size 1 still forces one workgroup per chain."""
    from learning_environments_amd import _lib
    L = _lib.lib()
    for agent in ("duelingddqn", "ddqn"):
        cfg, _, _ = ddqn_case(orc, agent, -10.0)
        assert L.lenv_dueling_team_size(C.byref(cfg), 6) == 2, agent
        cfg.team_size = 1
        assert L.lenv_dueling_team_size(C.byref(cfg), 6) == 1, agent
    for which, chains in (("pendulum_reward_env", 5), ("cmc", 5)):
        cfg, _, _ = td3_case(orc, which)
        got = L.lenv_td3_rn_team_size(C.byref(cfg), chains)
        cfg.test_mode = 0
        want = L.lenv_td3_rn_team_size(C.byref(cfg), chains)
        cfg.test_mode = 1
        assert got == want and got > 1, (which, got, want)
        cfg.team_size = 1
        assert L.lenv_td3_rn_team_size(C.byref(cfg), chains) == 1, which


# ---------------------------------------------------------------------------------------------------------------
# 2. DuelingDDQN / plain DQN on the Acrobot SE
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agent,done_bias", sorted(DDQN_CASES))
def test_wavechain_dueling_kernel_test_mode_1(eng, orc, agent, done_bias):
    """Production launches (teams of two workgroups per chain, and one workgroup) of kWcShapes[1] / [2] with test_mode 1 against the
    GEMM-queue kernel (a launch with a step trace; kernel_variant NO_WAVECHAIN) and the oracle on two chains: score, counters (test_steps
    = the final test only), the per-episode training returns, episode lengths, final returns and the trained online net, bit for bit."""
    from learning_environments_amd import _lib
    cfg, ocfg, d = ddqn_case(orc, agent, done_bias)
    E = cfg.train_episodes
    oracle = oracle_chains(ddqn_oracle_chain, orc, ocfg, d, DDQN_ORACLE_CHAINS[(agent, done_bias)])
    stops = [o["episodes_run"] for o in oracle.values()]
    print("oracle stops", stops, "learn steps", [o["learn_steps"] for o in oracle.values()])
    assert len(set(stops)) >= 2 and min(stops) < E and max(o["learn_steps"] for o in oracle.values()) >= 80
    for o in oracle.values():
        assert o["test_steps"] == int(np.sum(np.abs(o["final_test_returns"])))        # only the final test touched the real Acrobot (|return| = length)
        if done_bias < -1.0:
            assert o["episode_len"][:o["episodes_run"]].tolist() == [40] * o["episodes_run"]
        else:
            assert o["episode_len"][:o["episodes_run"]].min() < 40
    assert _lib.lib().lenv_dueling_team_size(C.byref(cfg), d["chains"]) == 2
    team = ddqn_run(eng, cfg, d)
    print("stats", team[1].tolist())
    assert len(set(team[1][:, 0].tolist())) >= 2
    cfg.team_size = 1
    one = ddqn_run(eng, cfg, d)
    cfg.team_size = 0
    traced = ddqn_run(eng, cfg, d, trace_cap=2)                   # GEMM-queue kernel
    cfg.kernel_variant = _lib.VARIANT_NO_WAVECHAIN
    assert _lib.lib().lenv_dueling_team_size(C.byref(cfg), d["chains"]) == 1
    generic = ddqn_run(eng, cfg, d)
    cfg.kernel_variant = 0
    for other, name in ((one, "one workgroup"), (traced, "trace launch"), (generic, "NO_WAVECHAIN")):
        for x, y in zip(team, other):
            assert np.array_equal(x, y, equal_nan=True), name
    assert not np.array_equal(team[5], d["init"])
    for c, o in oracle.items():
        assert_ddqn_equals_oracle(team, o, c)


# ---------------------------------------------------------------------------------------------------------------
# 3. the deterministic time-out with training returns in the meter
# ---------------------------------------------------------------------------------------------------------------
def test_wavechain_dueling_test_mode_1_step_budget(eng, orc):
    """A step budget that stops the full-length dueling case in mid-training: the per-episode list is padded with the minimum of the
    TRAINING returns so far, the final test is cut against the remaining budget.  Team launch, one-workgroup launch and oracle agree."""
    from learning_environments_amd import _lib
    cfg, ocfg, d = ddqn_case(orc, "duelingddqn", -10.0, step_budget=STEP_BUDGET)
    assert _lib.lib().lenv_dueling_team_size(C.byref(cfg), d["chains"]) == 2
    team = ddqn_run(eng, cfg, d)
    cfg.team_size = 1
    one = ddqn_run(eng, cfg, d)
    for x, y in zip(team, one):
        assert np.array_equal(x, y, equal_nan=True)
    assert sorted(set(team[1][:, 0].tolist())) == [4, 5]
    for c, o in oracle_chains(ddqn_oracle_chain, orc, ocfg, d, (0, 5)).items():
        n = o["episodes_run"]
        assert o["train_steps"] == 40 * n and o["learn_steps"] == 40 * (n - 1)
        if c == 0:                                                # left on the virtual rule: nothing is padded
            assert n == 4 and np.all(np.isnan(o["episode_test_mean"][n:]))
        else:                                                     # timed out in mid-training: padded with the smallest training return so far
            assert n == 5 and np.all(o["episode_test_mean"][n:] == o["episode_test_mean"][:n].min()) and o["score"] == -1e9
        assert_ddqn_equals_oracle(team, o, c)


# ---------------------------------------------------------------------------------------------------------------
# 4. TD3
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,teams", [("pendulum_reward_env", (1, 2, 3, 6)), ("cmc", (1, 2, 4, 8))])
def test_wavechain_td3_kernel_test_mode_1(eng, orc, which, teams):
    """The Pendulum RewardEnv shape (real rule on the shaped training returns) and the CMC VirtualEnv shape (virtual rule; batch 256,
    policy_delay 2, same_action_num 2, odd max_steps) with test_mode 1 at every team size against the GEMM-queue kernel (a launch with a
    step trace) and the oracle on two chains: scores, counters, training returns, final returns, all parameters and the episode lengths."""
    from learning_environments_amd import _lib
    cfg, ocfg, d = td3_case(orc, which)
    E = cfg.train_episodes
    oracle = oracle_chains(td3_oracle_chain, orc, ocfg, d, TD3_ORACLE_CHAINS[which])
    stops = [o["episodes_run"] for o in oracle.values()]
    print("oracle stops", stops, "learn steps", [o["learn_steps"] for o in oracle.values()])
    assert len(set(stops)) >= 2 and min(stops) < E, stops
    for o in oracle.values():
        assert o["test_steps"] == cfg.test_episodes * cfg.max_steps or which == "cmc"      # the final test only (Pendulum never terminates)
    ref = td3_run(eng, cfg, d, trace_cap=2)                       # GEMM-queue kernel
    print("stats", ref[1].tolist())
    assert _lib.lib().lenv_td3_rn_team_size(C.byref(cfg), d["chains"]) == max(teams)
    for G in teams:
        cfg.team_size = G
        assert _lib.lib().lenv_td3_rn_team_size(C.byref(cfg), d["chains"]) == G
        out = td3_run(eng, cfg, d)
        for x, y in zip(out, ref):
            assert np.array_equal(x, y, equal_nan=True), G
    cfg.team_size = 0
    assert not np.array_equal(ref[4], d["init"])
    for c, o in oracle.items():
        assert float(ref[0][c]) == o["score"]
        assert ref[1][c].tolist() == [o["episodes_run"], o["train_steps"], o["learn_steps"], o["test_steps"]]
        assert np.array_equal(ref[2][c], o["episode_test_mean"], equal_nan=True)
        assert np.array_equal(ref[3][c], o["final_test_returns"])
        assert np.array_equal(ref[4][c], o["final_params"])
        assert np.array_equal(ref[5][c], o["episode_len"])


# ---------------------------------------------------------------------------------------------------------------
# 5. the evaluation harness
# ---------------------------------------------------------------------------------------------------------------
def test_harness_dueling_launch_runs_on_teams(eng):
    """train_test_agents_models with DuelingDDQN_vary, vary_hp off, on two Acrobot VirtualEnvs of the published shape: the launch takes the
    wave-chain kernel on teams, and returns what the GEMM-queue kernel (gtn.kernel_variant NO_WAVECHAIN) returns."""
    from learning_environments_amd import _lib, configs
    from learning_environments_amd.envs.env_factory import EnvFactory
    from learning_environments_amd.experiments.syn_env_evaluate import train_test_agents, train_test_agents_models
    config = configs.with_vary(configs.acrobot_syn_env_duelingddqn(num_workers=1))
    config["device"] = "cuda"
    config["envs"]["Acrobot-v1"]["max_steps"] = 8
    torch.manual_seed(5)
    fac = EnvFactory(config)
    venvs, real_env = [fac.generate_virtual_env(), fac.generate_virtual_env()], fac.generate_real_env()

    def run(variant):
        c = copy.deepcopy(config)
        c["agents"]["gtn"]["kernel_variant"] = variant
        out = train_test_agents_models(venvs, real_env, c, agents_num=3, agent_name="DuelingDDQN_vary", train_episodes=14, vary_hp=False, seed=4)
        last = train_test_agents.last
        assert last["inner"].cfg.test_mode == 1 and last["inner"].chains == 6
        return out, _lib.lib().lenv_dueling_team_size(C.byref(last["task"].cfg), 6), last["inner"].stats.cpu().numpy()

    got, team, stats = run(0)
    assert team > 1
    assert stats[:, 2].min() > 0                                   # every chain learned (ten init episodes, then learning ones)
    want, team_off, _ = run(_lib.VARIANT_NO_WAVECHAIN)
    assert team_off == 1
    assert got == want and len(got) == 2 and len(got[0][0]) == 3


# ---------------------------------------------------------------------------------------------------------------
# 6. the register-resident DDQN kernel's team instantiation with test_mode 1
# ---------------------------------------------------------------------------------------------------------------
def test_register_resident_ddqn_team_launch_test_mode_1(eng, orc):
    """CartPole SE + DDQN (the published 4-57-2 net) with test_mode 1 at 24 chains: the launch takes the kernel's TEAM instantiation; team
    launch, team_size 1 and the oracle on three chains agree bit for bit (the case no test held against the oracle before; it passed as the
    kernel stood)."""
    from learning_environments_amd import _lib, configs
    from learning_environments_amd.config import ddqn_cfg_from_config
    cfgd = configs.fixed_work(configs.cartpole_syn_env_ddqn(num_workers=8), 8)
    cfgd["envs"]["CartPole-v0"]["max_steps"] = 20
    cfgd["agents"]["ddqn"].update(early_out_num=2, early_out_virtual_diff=0.1)
    cfg = ddqn_cfg_from_config(cfgd, test_mode=1)
    ocfg = orc.ddqn_cfg_from_config(cfgd, grad_chunk=cfg.grad_chunk, rng_mode=0, test_mode=1)
    chains = 24
    assert _lib.lib().lenv_ddqn_se_team_size(C.byref(cfg), chains) > 1
    rng = np.random.RandomState(12)
    P_se = sum(orc.mlp_num_params(dsc) for dsc in orc.se_descs(4, 2, ocfg.se_hidden, 1, "leakyrelu"))
    theta = (rng.randn(P_se) * 0.1).astype(np.float32)
    eps = (rng.randn(8, P_se) * 0.0124).astype(np.float32)
    worker = np.repeat(np.arange(8), 3).astype(np.int32)
    sign = np.tile(np.array([0.0, 1.0, -1.0], np.float32), 8)
    keys = np.array([orc.chain_key(7, 0, int(worker[c]), c % 3) for c in range(chains)], np.uint64)
    d = dict(theta=theta, eps=eps, worker=worker, sign=sign, keys=keys, chains=chains)
    il = eng.InnerLoop(cfg, chains, want_final_online=True)
    d["init"] = rng.uniform(-0.4, 0.4, (chains, il.p_agent)).astype(np.float32)
    team = ddqn_run(eng, cfg, d)
    cfg.team_size = 1
    assert _lib.lib().lenv_ddqn_se_team_size(C.byref(cfg), chains) == 1
    one = ddqn_run(eng, cfg, d)
    for x, y in zip(team, one):
        assert np.array_equal(x, y, equal_nan=True)
    oracle = oracle_chains(ddqn_oracle_chain, orc, ocfg, d, (2, 10, 23))
    assert [o["episodes_run"] for o in oracle.values()] == [4, 8, 6]      # the virtual rule ends training at different episodes, or never
    for c, o in oracle.items():
        assert o["learn_steps"] == 20 * (o["episodes_run"] - 1)
        assert_ddqn_equals_oracle(team, o, c)
