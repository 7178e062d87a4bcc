"""lenv_agent_test_population (csrc/agent_test_population.hip): BaseAgent.test of a population of DDQN / DuelingDDQN agents on the real env in
one launch.  Everything is held bit for bit:

1. against the oracle's chain with train_episodes = 0 (a bare test): returns and the env-step total;
2. against the composition of entries that already exist -- lenv_real_env_reset, lenv_mlp_forward (oracle.dueling_forward for dueling agents)
   with an argmax on the host, lenv_real_env_step repeated same_action_num times: every row field, both step counts, the returns, and the
   sentinel in the slots no step filled;
3. against the closing test of the three fused loops, on their final_online rows;
4. through histogram.collect, the first user of the rows.

Parameter rows are 0.5 * standard_normal so that actions vary; every case has 5 agents, two of them with identical rows, keys and offsets
(their outputs must be identical), and non-zero episode offsets."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

AGENTS = 5
OFFSETS = np.array([3, 0, 17, 17, 1000000007], np.int64)         # agents 2 and 3 are the identical pair
SENTINEL = -12345.0
ROW_FIELDS = ("row_state", "row_action", "row_next_state", "row_reward", "row_done")


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


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _config(env, dueling, H, L, T, max_steps, san=1, F=0, act="tanh", ln=False):
    """A reference-format config dict for the agent under test (no test reads the SE section)."""
    from learning_environments_amd import configs
    c = configs.cartpole_syn_env_ddqn(4)
    e = c["envs"].pop("CartPole-v0")
    e["max_steps"] = max_steps
    c["env_name"], c["envs"] = env, {env: e}
    a = c["agents"].pop("ddqn")
    a.update(hidden_size=H, hidden_layer=L, test_episodes=T, same_action_num=san, activation_fn=act, use_layer_norm=ln, batch_size=8, train_episodes=0)
    if dueling:
        a["feature_dim"] = F
    c["agents"]["duelingddqn" if dueling else "ddqn"] = a
    c["agents"]["gtn"]["agent_name"] = "DuelingDDQN" if dueling else "DDQN"
    return c


def _population(eng, cfg, seed):
    """5 agents: parameter rows 0.5 * N(0,1) and keys; agents 2 and 3 identical."""
    rng = np.random.RandomState(seed)
    params = (0.5 * rng.standard_normal((AGENTS, eng.agent_test_num_params(cfg)))).astype(np.float32)
    keys = rng.randint(1, 2 ** 62, size=AGENTS).astype(np.uint64)
    params[3], keys[3] = params[2], keys[2]
    return params, keys


def _resets(cfg, keys, offsets):
    """(fp64 states [agents,T,4], fp32 observations [agents,T,S]) of the episodes offsets[i] + e, from lenv_real_env_reset (the test-reset
    stream of the counter RNG)."""
    from learning_environments_amd import _lib
    T, S, n = cfg.test_episodes, cfg.state_dim, len(keys) * cfg.test_episodes
    k = dev(np.repeat(keys, T).view(np.int64))
    ep = dev(np.repeat(offsets, T) + np.tile(np.arange(T, dtype=np.int64), len(keys)))
    st = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    obs = torch.zeros((n, S), dtype=torch.float32, device="cuda")
    el = torch.zeros(n, dtype=torch.int32, device="cuda")
    assert _lib.lib().lenv_real_env_reset(cfg.env_id, ptr(k), ptr(ep), n, ptr(st), ptr(obs), ptr(el), None) == 0
    torch.cuda.synchronize()
    return st.cpu().numpy().reshape(len(keys), T, 4), obs.cpu().numpy().reshape(len(keys), T, S)


def _run(cfg, params, keys, offsets=None, reset_states=None):
    """The entry through the C-ABI on buffers this test owns, every one pre-filled with a sentinel; host copies of everything."""
    from learning_environments_amd import _lib
    L = _lib.lib()
    n, T, S = params.shape[0], cfg.test_episodes, cfg.state_dim
    cap = int(L.lenv_agent_test_rows_cap(C.byref(cfg)))
    assert cap == -(-cfg.max_steps // max(cfg.same_action_num, 1))
    f32 = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device="cuda")
    out = dict(returns=torch.full((n, T), SENTINEL, dtype=torch.float64, device="cuda"), env_steps=i32(n, T), agent_steps=i32(n, T),
               row_state=f32(n, T, cap, S), row_action=i32(n, T, cap), row_next_state=f32(n, T, cap, S), row_reward=f32(n, T, cap), row_done=f32(n, T, cap))
    p, k = dev(params), dev(keys.view(np.int64))
    off = dev(offsets) if offsets is not None else None
    rs = dev(reset_states) if reset_states is not None else None
    rc = L.lenv_agent_test_population(C.byref(cfg), ptr(p), ptr(k), ptr(off), ptr(rs), n, ptr(out["returns"]), ptr(out["env_steps"]), ptr(out["agent_steps"]),
                                      *[ptr(out[f]) for f in ROW_FIELDS], None)
    assert rc == 0
    torch.cuda.synchronize()
    return {name: v.cpu().numpy() for name, v in out.items()}


def _check_identical_pair(got):
    for name, v in got.items():
        assert np.array_equal(v[2], v[3]), name


# ---- 1. the oracle's bare test ----

ORACLE_CASES = {
    "cartpole_plain_24": dict(env="CartPole-v0", dueling=False, H=24, L=1, T=3, max_steps=40),
    "acrobot_dueling_130_2_16": dict(env="Acrobot-v1", dueling=True, H=130, L=2, F=16, T=1, max_steps=40, act="relu"),
    "mountaincar_plain_24_3_ln_T70_repeat3": dict(env="MountainCar-v0", dueling=False, H=24, L=3, T=70, max_steps=40, san=3, ln=True),
}


@pytest.mark.parametrize("case", sorted(ORACLE_CASES))
def test_equals_the_oracles_bare_test(eng, orc, case):
    """oracle.ddqn_se_chain with train_episodes = 0 runs the closing test alone on the given parameter row; its test resets come from a
    tape holding the states of episodes offset + e, so the non-zero offsets are covered.  returns and the env-step total are equal."""
    from learning_environments_amd.config import ddqn_cfg_from_config
    cfgd = _config(**ORACLE_CASES[case])
    cfg = ddqn_cfg_from_config(cfgd)
    assert cfg.train_episodes == 0
    params, keys = _population(eng, cfg, 11)
    got = _run(cfg, params, keys, OFFSETS)
    _check_identical_pair(got)
    assert (got["env_steps"] >= 1).all() and (got["env_steps"] <= cfg.max_steps).all()
    assert np.array_equal(got["agent_steps"], -(-got["env_steps"] // max(cfg.same_action_num, 1)))
    resets, _ = _resets(cfg, keys, OFFSETS)
    ocfg = orc.ddqn_cfg_from_config(cfgd, grad_chunk=0, rng_mode=1)
    P_se = sum(orc.mlp_num_params(d) for d in orc.se_descs(cfg.state_dim, cfg.num_actions, cfg.se_hidden, cfg.se_layers, cfg.se_act))
    for i in range(AGENTS):
        tapes = orc.make_tapes(np.zeros(1), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros((1, 4)), resets[i])
        o = orc.ddqn_se_chain(ocfg, np.zeros(P_se, np.float32), params[i], rng_key=int(keys[i]), tapes=tapes)
        assert o["rc"] == 0
        assert np.array_equal(got["returns"][i], o["final_test_returns"]), (case, i)
        assert int(got["env_steps"][i].sum()) == o["test_steps"], (case, i)
    # no offsets = the counter draws a chain without tapes tests on
    got0 = _run(cfg, params[:2], keys[:2])
    ocfg0 = orc.ddqn_cfg_from_config(cfgd, grad_chunk=0, rng_mode=0)
    o = orc.ddqn_se_chain(ocfg0, np.zeros(P_se, np.float32), params[0], rng_key=int(keys[0]))
    assert np.array_equal(got0["returns"][0], o["final_test_returns"]) and int(got0["env_steps"][0].sum()) == o["test_steps"]
    assert np.array_equal(got0["returns"][1], got["returns"][1])              # agent 1 has offset 0 in OFFSETS


# ---- 2. composition of the existing one-step entries ----

COMPOSE_CASES = {
    "cartpole_plain": dict(env="CartPole-v0", dueling=False, H=24, L=1, T=3, max_steps=20),
    "mountaincar_dueling_repeat2": dict(env="MountainCar-v0", dueling=True, H=20, L=2, F=8, T=3, max_steps=20, san=2, act="relu"),
    "acrobot_plain_ln_repeat3": dict(env="Acrobot-v1", dueling=False, H=33, L=2, T=3, max_steps=20, san=3, ln=True),
    # 6-208-208-3 with LayerNorm: 45 971 floats, past the 40 704 that fit next to the activations, so the weights are read from global
    # memory; T 17 = a second workgroup per agent with one episode
    "acrobot_plain_unstaged_ln_T17_repeat2": dict(env="Acrobot-v1", dueling=False, H=208, L=2, T=17, max_steps=8, san=2, ln=True),
}


def _replay_by_steps(eng, orc, cfgd, cfg, params, states0, obs0):
    """The same test step by step, all agents' episodes together: Q from lenv_mlp_forward (plain) / oracle.dueling_forward, argmax on the host
    (numpy: the first maximum = the lower index), lenv_real_env_step once per repeat on the episodes that are still inside their agent step.
    The arrays start filled with what _run pre-fills, so an equal comparison also shows which slots were never written."""
    from learning_environments_amd import _lib
    L = _lib.lib()
    n, T, S, A = params.shape[0], cfg.test_episodes, cfg.state_dim, cfg.num_actions
    k_rep = max(cfg.same_action_num, 1)
    cap = -(-cfg.max_steps // k_rep)
    N = n * T
    st = dev(states0.reshape(N, 4).copy())
    el = torch.zeros(N, dtype=torch.int32, device="cuda")
    cur = obs0.reshape(N, S).copy()
    desc = eng.mlp_desc(S, cfg.q_hidden, cfg.q_layers, A, cfg.q_act, use_layer_norm=bool(cfg.q_layer_norm)) if cfg.agent_kind == 0 else None
    ocfg = orc.ddqn_cfg_from_config(cfgd, grad_chunk=0, rng_mode=0) if cfg.agent_kind == 1 else None
    exp = dict(row_state=np.full((n, T, cap, S), SENTINEL, np.float32), row_action=np.full((n, T, cap), -7, np.int32),
               row_next_state=np.full((n, T, cap, S), SENTINEL, np.float32), row_reward=np.full((n, T, cap), SENTINEL, np.float32),
               row_done=np.full((n, T, cap), SENTINEL, np.float32), agent_steps=np.zeros((n, T), np.int32))
    ret32 = np.zeros(N, np.float32)
    alive = np.ones(N, bool)
    for step in range(cap):
        q = np.zeros((N, A), np.float32)
        for i in range(n):
            x = cur[i * T:(i + 1) * T]
            q[i * T:(i + 1) * T] = eng.mlp_forward(desc, dev(params[i]), dev(x)).cpu().numpy() if desc is not None else orc.dueling_forward(ocfg, params[i], x)
        act = np.argmax(q, axis=1).astype(np.int32)
        running = alive.copy()
        rsum = np.zeros(N, np.float64)
        nxt, done = cur.copy(), np.zeros(N, np.float32)
        for _ in range(k_rep):
            idx = np.nonzero(running)[0]
            if idx.size == 0:
                break
            it = dev(idx.astype(np.int64))
            s_sub, e_sub, a_sub = st[it].contiguous(), el[it].contiguous(), dev(act[idx])
            o_sub = torch.zeros((idx.size, S), dtype=torch.float32, device="cuda")
            r_sub, d_sub = torch.zeros(idx.size, dtype=torch.float32, device="cuda"), torch.zeros(idx.size, dtype=torch.float32, device="cuda")
            assert L.lenv_real_env_step(cfg.env_id, cfg.max_steps, idx.size, ptr(a_sub), ptr(s_sub), ptr(e_sub), ptr(o_sub), ptr(r_sub), ptr(d_sub), None) == 0
            st[it], el[it] = s_sub, e_sub
            rsum[idx] += r_sub.cpu().numpy().astype(np.float64)               # python-float sum of the repeats' rewards
            nxt[idx], done[idx] = o_sub.cpu().numpy(), d_sub.cpu().numpy()
            running[idx] = done[idx] < 0.5
        for j in np.nonzero(alive)[0]:
            i, e = divmod(int(j), T)
            r32 = np.float32(rsum[j])
            exp["row_state"][i, e, step], exp["row_action"][i, e, step], exp["row_next_state"][i, e, step] = cur[j], act[j], nxt[j]
            exp["row_reward"][i, e, step], exp["row_done"][i, e, step] = r32, done[j]
            ret32[j] = np.float32(ret32[j] + r32)
            exp["agent_steps"][i, e] += 1
        cur = nxt
        alive &= done < 0.5
        if not alive.any():
            break
    exp["returns"] = ret32.astype(np.float64).reshape(n, T)
    exp["env_steps"] = el.cpu().numpy().reshape(n, T)
    return exp


@pytest.mark.parametrize("case", sorted(COMPOSE_CASES))
def test_rows_equal_the_composition_of_the_step_entries(eng, orc, case):
    from learning_environments_amd.config import ddqn_cfg_from_config
    cfgd = _config(**COMPOSE_CASES[case])
    cfg = ddqn_cfg_from_config(cfgd)
    params, keys = _population(eng, cfg, 23)
    T = cfg.test_episodes
    resets, obs0 = _resets(cfg, keys, OFFSETS)
    given = None
    if cfg.env_id == 3:
        # MountainCar: no policy reaches the flag in 20 steps from the valley; one episode starts next to it, moving right (reset_states)
        resets[1, 1] = (0.45, 0.07, 0.0, 0.0)
        obs0[1, 1] = np.array([0.45, 0.07]).astype(np.float32)
        given = resets
    got = _run(cfg, params, keys, OFFSETS, reset_states=given)
    _check_identical_pair(got)
    exp = _replay_by_steps(eng, orc, cfgd, cfg, params, resets, obs0)
    for name in ("agent_steps", "env_steps", "returns") + ROW_FIELDS:
        assert np.array_equal(got[name], exp[name]), (case, name)
    # slots no step filled still hold the sentinel (the comparison above covers it: exp started from the sentinel; spelled out)
    cap = got["row_action"].shape[2]
    beyond = np.arange(cap)[None, None, :] >= got["agent_steps"][:, :, None]
    if cfg.env_id == 0 or cfg.env_id == 3:
        assert beyond.any()
    assert (got["row_reward"][beyond] == SENTINEL).all() and (got["row_action"][beyond] == -7).all()
    assert (got["row_state"][beyond] == SENTINEL).all() and (got["row_next_state"][beyond] == SENTINEL).all() and (got["row_done"][beyond] == SENTINEL).all()
    # done = 1 in the last filled slot of every episode and nowhere before it
    ii, ee = np.meshgrid(np.arange(AGENTS), np.arange(T), indexing="ij")
    assert (got["row_done"][ii, ee, got["agent_steps"] - 1] == 1.0).all() and got["row_done"][~beyond].sum() == AGENTS * T
    if cfg.env_id == 0:
        assert (got["env_steps"] < cfg.max_steps).any(), "CartPole: some episode must end on the env's own done flag"
    if cfg.env_id == 3:
        assert got["env_steps"][1, 1] == 1 and got["agent_steps"][1, 1] == 1            # the flag, inside the first agent step
        others = np.ones((AGENTS, T), bool)
        others[1, 1] = False
        assert (got["env_steps"][others] == cfg.max_steps).all()                         # everyone else: TimeLimit


# ---- 3. the closing test of the fused loops ----

def _fused_case(name):
    from learning_environments_amd import configs
    if name == "register_resident_ddqn":
        c = configs.fixed_work(configs.cartpole_syn_env_ddqn(4), 3)
        c["agents"]["ddqn"].update(hidden_size=64, init_episodes=1, test_episodes=4)
        c["envs"]["CartPole-v0"]["max_steps"] = 60
    elif name == "generic_dueling":
        c = configs.fixed_work(configs.acrobot_syn_env_duelingddqn(4), 3)
        c["agents"]["duelingddqn"].update(hidden_size=64, feature_dim=32, init_episodes=1, batch_size=32, test_episodes=3)
        c["envs"]["Acrobot-v1"]["max_steps"] = 60
    else:
        c = configs.fixed_work(configs.mountaincar_syn_env_ddqn(4), 3)                  # the published 2-256-256-3 shape
        c["agents"]["ddqn"].update(init_episodes=1)
        c["envs"]["MountainCar-v0"]["max_steps"] = 60
    return c


@pytest.mark.parametrize("name", ["register_resident_ddqn", "generic_dueling", "ddqn_wavechain_wide"])
def test_returns_equal_the_fused_loops_final_returns(eng, name):
    """2 chains train 3 episodes (test_mode 0: T test episodes after each), then the launch's closing test.  The entry on final_online with the
    chains' keys and episode_offset = episodes_run * T gives final_returns bit for bit."""
    from learning_environments_amd.config import ddqn_cfg_from_config
    cfgd = _fused_case(name)
    cfg = ddqn_cfg_from_config(cfgd)
    chains = 2
    rng = np.random.RandomState(5)
    P_se = sum(eng.mlp_num_params(d) for d in eng.se_descs(cfg.state_dim, cfg.num_actions, cfg.se_hidden, cfg.se_layers, cfg.se_act))
    theta = (rng.randn(P_se) * 0.1).astype(np.float32)
    il = eng.InnerLoop(cfg, chains, want_final_online=True)
    assert il.dueling == (name != "register_resident_ddqn")
    assert il.p_agent == eng.agent_test_num_params(cfg)
    agent_init = rng.uniform(-0.3, 0.3, (chains, il.p_agent)).astype(np.float32)
    keys = rng.randint(1, 2 ** 62, size=chains).astype(np.uint64)
    il.run(dev(theta), dev(np.zeros((1, P_se), np.float32)), dev(np.zeros(chains, np.int32)), dev(np.zeros(chains, np.float32)), dev(agent_init),
           rng_keys=dev(keys.view(np.int64)))
    torch.cuda.synchronize()
    assert il.status.cpu().tolist() == [0] * chains
    stats = il.stats.cpu().numpy()
    assert (stats[:, 0] == 3).all() and (stats[:, 2] > 0).all()
    T = cfg.test_episodes
    offsets = (stats[:, 0] * T).astype(np.int64)
    got = eng.agent_test_population(cfg, il.final_online, dev(keys.view(np.int64)), episode_offset=dev(offsets), want_rows=False)
    assert sorted(got) == ["agent_steps", "env_steps", "returns"]
    assert np.array_equal(got["returns"].cpu().numpy(), il.final_returns.cpu().numpy()), name
    assert not np.array_equal(il.final_online.cpu().numpy(), agent_init)


# ---- 4. histogram.collect ----

def test_histogram_collect_on_a_fresh_cartpole_se(eng):
    from learning_environments_amd import configs
    from learning_environments_amd.agents.rollout import ReplayRows, test_agents
    from learning_environments_amd.envs.env_factory import EnvFactory
    from learning_environments_amd.experiments import histogram
    config = configs.cartpole_syn_env_ddqn(4)
    config["agents"]["ddqn"].update(train_episodes=4, init_episodes=1, test_episodes=3, hidden_size=24, batch_size=16, early_out_num=2)
    config["envs"]["CartPole-v0"].update(max_steps=30, hidden_size=16)
    torch.manual_seed(3)
    fac = EnvFactory(config)
    virtual_env, real_env = fac.generate_virtual_env(), fac.generate_real_env()
    out = histogram.collect(virtual_env, real_env, config, "ddqn", agents_num=3, seed=9)      # its own assertion: returns == final_returns
    last = histogram.collect.last
    inner = last["inner"]
    stats = inner.stats.cpu().numpy()
    assert [tuple(t.shape)[1:] for t in out["train"]] == [(4,), (1,), (4,), (1,), (1,)]
    assert out["train"][0].shape[0] == int(stats[:, 1].sum()) > 0
    assert set(out["train"][1].reshape(-1).tolist()) <= {0.0, 1.0}
    assert len(out["rewards"]) == 3 and out["agentname"] == "ddqn"
    # the test rows are test_agents's, agent after agent
    triples = test_agents(last["config"], inner.final_online, last["keys"])
    merged = ReplayRows(4)
    for reward_list, length_list, rows in triples:
        assert len(reward_list) == len(length_list) == 3 and rows.get_size() == sum(length_list)
        merged.merge_buffer(rows)
    for a, b in zip(out["test"], merged.get_all()):
        assert torch.equal(a, b)
    assert [np.mean(t[0]) for t in triples] == out["rewards"]
    # the episode returns are the sums of the rows' rewards (CartPole: 1 per step, exact in fp32)
    s, a, s2, r, d = triples[0][2].get_all()
    assert float(r.sum()) == sum(triples[0][0]) and int(d.sum()) == 3
    # virt_* = a direct step_population call on the real env's (state, action) pairs
    states, actions = out["test"][0].cuda().contiguous(), out["test"][1].reshape(-1).to(torch.int32).cuda().contiguous()
    ns, rr, dd = virtual_env.step_population(actions, states, repeat=1)
    assert torch.equal(out["virt_next_states"], ns.cpu()) and torch.equal(out["virt_rewards"], rr.cpu().reshape(-1, 1))
    assert torch.equal(out["virt_dones"], dd.cpu().reshape(-1, 1))
    _, ri, _ = virtual_env.step_population(1 - actions, states, repeat=1)
    assert torch.equal(out["virt_rewards_incorrect"], ri.cpu().reshape(-1, 1))
    assert not torch.equal(out["virt_rewards_incorrect"], out["virt_rewards"])
