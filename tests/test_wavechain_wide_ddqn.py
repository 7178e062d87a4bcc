"""The 256-wide DDQN wave-chain kernel (ddqn_wavechain_wide.hip): default_config_mountaincar.yaml's Critic_DQN 2-256-256-3 relu, B = 128, on
the MountainCar-v0 SE (hidden 128 leakyrelu, ten test episodes), on teams of 1, 2 or 4 workgroups per chain.

Bar: bit for bit against the GEMM-queue kernel (the same inputs through a launch that asks for a step trace, or with kernel_variant
NO_WAVECHAIN) and against the oracle's DDQN chain."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


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


def _published_cfg(pop=16):
    from learning_environments_amd import configs
    from learning_environments_amd.config import ddqn_cfg_from_config
    cfgd = configs.mountaincar_syn_env_ddqn(pop)
    cfg = ddqn_cfg_from_config(cfgd)
    assert (cfg.agent_kind, cfg.state_dim, cfg.num_actions, cfg.q_hidden, cfg.q_layers, cfg.batch_size, cfg.se_hidden, cfg.test_episodes) == \
        (0, 2, 3, 256, 2, 128, 128, 10)
    return cfgd, cfg


def test_team_size_of_the_published_shape(eng):
    """The published cfg takes the wave-chain kernel on teams: four workgroups per chain at 48 chains (pop 16), two at 96; one workgroup for
    every mode the kernel does not cover (they stay on the GEMM-queue kernel)."""
    from learning_environments_amd import _lib
    lib = _lib.lib()
    _, cfg = _published_cfg()
    assert lib.lenv_dueling_team_size(C.byref(cfg), 48) == 4
    assert lib.lenv_dueling_team_size(C.byref(cfg), 96) == 2
    for G in (1, 2):
        cfg.team_size = G
        assert lib.lenv_dueling_team_size(C.byref(cfg), 48) == G
    cfg.team_size = 0
    for field, value in (("kernel_variant", _lib.VARIANT_NO_WAVECHAIN), ("kernel_variant", _lib.VARIANT_GENERIC), ("test_mode", 1),
                         ("se_layers", 2), ("q_layer_norm", 1), ("icm_enabled", 1), ("same_action_num", 2)):
        _, c = _published_cfg()
        setattr(c, field, value)
        if field == "icm_enabled":
            c.icm_feature_dim, c.icm_hidden = 32, 64
        assert lib.lenv_dueling_team_size(C.byref(c), 48) == 1, field


def _chain_inputs(orc, cfg, chains, seed, done_bias):
    S, A = cfg.state_dim, cfg.num_actions
    rng = np.random.RandomState(seed)
    P_se = sum(orc.mlp_num_params(d) for d in orc.se_descs(S, A, cfg.se_hidden, 1, "leakyrelu"))
    P_q = S * 256 + 256 + 256 * 256 + 256 + A * 256 + A
    theta = (rng.randn(P_se) * 0.1).astype(np.float32)
    theta[-1] = done_bias                               # the done net's output bias: -10 = the SE never ends an episode
    pop = chains // 3
    eps = (rng.randn(pop, P_se) * 0.05).astype(np.float32)
    agent_init = rng.uniform(-0.06, 0.06, (chains, P_q)).astype(np.float32)
    worker = np.repeat(np.arange(pop), 3).astype(np.int32)
    sign = np.tile(np.array([0.0, 1.0, -1.0], np.float32), pop)
    keys = np.array([orc.chain_key(seed, 5, int(worker[c]), c % 3) for c in range(chains)], np.uint64)
    return theta, eps, worker, sign, agent_init, keys


@pytest.mark.parametrize("case", ["ring_wraps", "early_out"])
def test_wavechain_wide_every_team_size_equals_gemm_queue_and_oracle(eng, orc, case):
    """Production launches with team_size 1, 2, 4 and automatic, the trace launch (GEMM-queue kernel) and the oracle chain agree bit for
    bit on scores, counters, per-episode test means and lengths, final returns and all 67 331 online parameters.  ring_wraps: the SE never
    ends an episode, a 60-row replay ring wraps, >= 80 learn steps per chain; early_out: the SE may end episodes and every chain stops after
    its first learning episode (solved_reward below any return)."""
    from learning_environments_amd import _lib, configs
    from learning_environments_amd.config import ddqn_cfg_from_config
    cfgd = configs.mountaincar_syn_env_ddqn(4)
    ag = cfgd["agents"]["ddqn"]
    if case == "ring_wraps":
        cfgd = configs.fixed_work(cfgd, 3)
        ag = cfgd["agents"]["ddqn"]
        ag.update(init_episodes=1, rb_size=60)
        cfgd["envs"]["MountainCar-v0"]["max_steps"] = 45
        done_bias = -10.0
    else:
        ag.update(train_episodes=4, init_episodes=1, early_out_num=1)
        cfgd["envs"]["MountainCar-v0"].update(max_steps=40, solved_reward=-1e9)
        done_bias = 0.0
    cfg = ddqn_cfg_from_config(cfgd)
    ocfg = orc.ddqn_cfg_from_config(cfgd, grad_chunk=0, rng_mode=0)
    chains = 12
    theta, eps, worker, sign, agent_init, keys = _chain_inputs(orc, cfg, chains, 31 if case == "ring_wraps" else 32, done_bias)

    def run(team_size, trace_cap=0):
        cfg.team_size = team_size
        if not trace_cap:
            assert _lib.lib().lenv_dueling_team_size(C.byref(cfg), chains) == (4 if team_size == 0 else team_size)
        il = eng.InnerLoop(cfg, chains, trace_cap=trace_cap, want_final_online=True)
        assert il.dueling and il.p_agent == agent_init.shape[1] == 67331
        il.run(dev(theta), dev(eps), dev(worker), dev(sign), dev(agent_init), rng_keys=dev(keys.view(np.int64)))
        torch.cuda.synchronize()
        assert il.status.cpu().tolist() == [0] * chains
        return [t.cpu().numpy().copy() for t in (il.score, il.stats, il.episode_test_mean, il.episode_len, il.final_returns, il.final_online)]

    ref = run(1, trace_cap=2)                           # GEMM-queue kernel
    for G in (1, 2, 4, 0):
        got = run(G)
        for name, a, b in zip(("score", "stats", "episode_test_mean", "episode_len", "final_returns", "final_online"), got, ref):
            assert np.array_equal(a, b, equal_nan=True), (G, name)
    st = ref[1]
    if case == "ring_wraps":
        assert (st[:, 2] >= 80).all() and (st[:, 1] > 60).all()
    else:
        assert (st[:, 0] == 2).all()                    # the random init episode, then one learning episode: early out
        assert (st[:, 2] > 0).all()
    assert not np.array_equal(ref[5], agent_init)
    for c in (1, 8):
        w = (np.float32(sign[c]) * eps[worker[c]] + theta).astype(np.float32)
        o = orc.ddqn_se_chain(ocfg, w, agent_init[c], rng_key=int(keys[c]), want_final_online=True)
        assert float(ref[0][c]) == o["score"]
        assert ref[1][c].tolist() == [o["episodes_run"], o["train_steps"], o["learn_steps"], o["test_steps"]]
        assert np.array_equal(ref[2][c], o["episode_test_mean"], equal_nan=True)
        assert np.array_equal(ref[3][c], o["episode_len"])
        assert np.array_equal(ref[4][c], o["final_test_returns"])
        assert np.array_equal(ref[5][c], o["final_online"])


def test_wavechain_wide_step_budget_equals_gemm_queue(eng, orc):
    """lenv_ddqn_cfg::step_budget on the wave-chain kernel (teams of four, and one workgroup per chain) against kernel_variant NO_WAVECHAIN
    (the GEMM-queue kernel, held to the oracle by test_gpu_parity.py's budget tests), every output bit for bit.  Two budgets, both derived from
    the step counts of an unbudgeted run of the same cfg: one that one training episode with its tests just fits (the check in front of an
    episode asks `steps so far > budget`, so the chains time out in front of the second or third of four episodes and the per-episode lists
    are padded), and one that lets training finish and leaves the final test the steps of about three of its ten episodes."""
    from learning_environments_amd import _lib, configs
    from learning_environments_amd.config import ddqn_cfg_from_config
    E, chains = 4, 3
    cfgd = configs.fixed_work(configs.mountaincar_syn_env_ddqn(4), E)
    cfgd["agents"]["ddqn"].update(init_episodes=1, rb_size=60)
    cfgd["envs"]["MountainCar-v0"]["max_steps"] = 30
    cfg = ddqn_cfg_from_config(cfgd)
    T = cfg.test_episodes
    theta, eps, worker, sign, agent_init, keys = _chain_inputs(orc, cfg, chains, 33, -10.0)
    names = ("score", "stats", "episode_test_mean", "episode_len", "final_returns", "final_online")

    def run(budget, variant, team_size):
        cfg.step_budget, cfg.kernel_variant, cfg.team_size = budget, variant, team_size
        il = eng.InnerLoop(cfg, chains, want_final_online=True)
        il.run(dev(theta), dev(eps), dev(worker), dev(sign), dev(agent_init), rng_keys=dev(keys.view(np.int64)))
        torch.cuda.synchronize()
        assert il.status.cpu().tolist() == [0] * chains
        return dict(zip(names, (t.cpu().numpy().copy() for t in (il.score, il.stats, il.episode_test_mean, il.episode_len, il.final_returns,
                                                                 il.final_online))))

    free = run(0, _lib.VARIANT_NO_WAVECHAIN, 0)
    assert (free["stats"][:, 0] == E).all()
    final_len = (-free["final_returns"]).sum(axis=1).astype(np.int64)        # MountainCar-v0 pays -1 per step: |return| = length
    before_final = free["stats"][:, 1] + free["stats"][:, 3] - final_len     # env steps in front of the final test
    budgets = {"training": int(before_final.min()) // E, "final_test": int(before_final.max()) + 3 * int(final_len.min()) // T}
    for which, budget in budgets.items():
        ref = run(budget, _lib.VARIANT_NO_WAVECHAIN, 0)
        if which == "training":
            ran = ref["stats"][:, 0]
            assert ((ran >= 1) & (ran <= 2) & (ran < E)).all(), ran.tolist()
            for c in range(chains):                                        # time_is_up's padding: minimum of the means, maximum of the lengths
                n = int(ran[c])
                assert (ref["episode_test_mean"][c, n:] == ref["episode_test_mean"][c, :n].min()).all()
                assert (ref["episode_len"][c, n:] == ref["episode_len"][c, :n].max()).all()
        else:
            assert (ref["stats"][:, 0] == E).all()
            used = ref["stats"][:, 1] + ref["stats"][:, 3] - before_final
            assert ((used > 0) & (used < final_len)).all(), used.tolist()   # the final test stopped between its episodes 1 and T - 1
        cfg.step_budget, cfg.kernel_variant, cfg.team_size = budget, 0, 0
        assert _lib.lib().lenv_dueling_team_size(C.byref(cfg), chains) == 4
        for team_size in (0, 1):
            got = run(budget, 0, team_size)
            for name in names:
                assert np.array_equal(got[name], ref[name], equal_nan=True), (which, team_size, name)


def test_gtn_generation_wavechain_equals_no_wavechain():
    """One GTN_Master generation of configs.mountaincar_syn_env_ddqn(16) in fixed-work form (48 chains, teams of four): the wave-chain
    kernel and kernel_variant NO_WAVECHAIN (the GEMM-queue kernel) leave the same updated theta and chain outputs, bit for bit."""
    import ctypes as C2
    from learning_environments_amd import _lib, configs
    from learning_environments_amd.agents.GTN import GTN_Master
    outs = []
    for variant in (0, _lib.VARIANT_NO_WAVECHAIN):
        c = configs.fixed_work(configs.mountaincar_syn_env_ddqn(16), 2)
        c["agents"]["ddqn"]["init_episodes"] = 1
        c["envs"]["MountainCar-v0"]["max_steps"] = 50
        c["agents"]["gtn"]["kernel_variant"] = variant
        torch.manual_seed(0)
        m = GTN_Master(c, bohb_id=0, seed=7)
        assert _lib.lib().lenv_dueling_team_size(C2.byref(m.cfg), 48) == (4 if variant == 0 else 1)
        m.step(0)
        torch.cuda.synchronize()
        assert m.inner.status.cpu().abs().max().item() == 0
        outs.append([t.cpu().numpy().copy() for t in (m.inner.score, m.inner.stats, m.inner.episode_test_mean, m.inner.final_returns, m.theta)])
    assert int(outs[0][1][:, 2].min()) == 50
    for a, b in zip(*outs):
        assert np.array_equal(a, b, equal_nan=True)
