"""lenv_actor_test_population (csrc/actor_test_population.hip): BaseAgent.test of a population of TD3 / PPO agents on the real env in one
launch.  Everything is held bit for bit:

(a) against the closing test of the fused loops in counter mode, on their final_params rows (TD3: the GEMM-queue kernel on the three envs and
    the wave-chain kernel on its Pendulum shape; PPO: the three envs), with training episodes and without;
(b) against the composition of entries that already exist -- lenv_mlp_forward on the actor, the action formula in numpy fp32 (the tanh is the
    oracle's orc_tanhf, the project's table tanh), lenv_cont_env_step once per repeat -- from given reset states and a given noise tape: every
    row field, both step counts, the returns, and the sentinel in the slots no step filled;
(c) at the edges of the indexing, against the same composition;
(d) through rollout.test_actor_agents.

The one thing the step entry cannot give bit for bit is the reward of an agent step with same_action_num > 1: lenv_cont_env_step returns each
repeat's reward rounded to fp32, while the kernel (like the fused loops and the reference's python-float sum) adds the repeats' fp64 rewards and
rounds once.  There the reward is held to the fp64 sum r of the fp32 step rewards within (sum |r_k| + |r|) * 2^-24, the two roundings' own
bound; the exact check of such sums is (a), MountainCarContinuous with same_action_num 2 against the fused kernels."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

TD3, PPO = 0, 1
SENTINEL = -12345.0
ROW_FIELDS = ("row_state", "row_action", "row_next_state", "row_reward", "row_done")
ENVS = {"pendulum": ("Pendulum-v0", 3, 1, 2, 2.0), "cmc": ("MountainCarContinuous-v0", 2, 1, 2, 1.0), "cheetah": ("HalfCheetah-v3", 17, 6, 17, 1.0)}
OFFSETS = np.array([3, 0, 1000000007], np.int64)


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


def _dims(cfg):
    from learning_environments_amd import engine
    S, SD, A = engine.REAL_ENV_DIMS[int(cfg.env_id)]
    return S, A, SD


def _cfg(kind, env, H, L, T, max_steps, san=1, act="relu", ln=False, action_std=0.1):
    """Only the fields the entry reads."""
    from learning_environments_amd import _lib
    name, S, A, _, ma = ENVS[env]
    kw = dict(env_id=_lib.ENV[name], state_dim=S, action_dim=A, max_steps=max_steps, hidden=H, layers=L, act=_lib.ACT[act], test_episodes=T,
              same_action_num=san, action_std=action_std)
    if kind == TD3:
        kw.update(max_action=ma, use_layer_norm=1 if ln else 0)
    return (_lib.Td3Cfg if kind == TD3 else _lib.PpoCfg)(**kw)


def _population(eng, kind, cfg, n, seed):
    """n agents: parameter rows uniform in +-2 / sqrt(H) (PPO: action_std 0.3, 0.0004 -- below the clamp -- and 0.7 in front) and keys."""
    rng = np.random.RandomState(seed)
    P = eng.actor_test_num_params(kind, cfg)
    b = 2.0 / np.sqrt(cfg.hidden)
    params = rng.uniform(-b, b, (n, P)).astype(np.float32)
    if kind == PPO:
        params[:, :cfg.action_dim] = np.array([0.3, 0.0004, 0.7], np.float32)[np.arange(n) % 3, None]
    keys = rng.randint(1, 2 ** 62, size=n).astype(np.uint64)
    return params, keys


def _resets(cfg, keys, offsets):
    """(fp64 states [agents,T,SD], fp32 observations [agents,T,S]) of the episodes offsets[i] + e, from lenv_cont_env_reset (the test-reset
    stream of the counter RNG)."""
    from learning_environments_amd import _lib
    S, A, SD = _dims(cfg)
    T, n = cfg.test_episodes, len(keys) * cfg.test_episodes
    k = dev(np.repeat(keys, T).view(np.int64))
    ep = dev(np.repeat(offsets, T) + np.tile(np.arange(T, dtype=np.int64), len(keys)))
    st = torch.zeros((n, SD), dtype=torch.float64, device="cuda")
    obs = torch.zeros((n, S), dtype=torch.float32, device="cuda")
    el = torch.zeros(n, dtype=torch.int32, device="cuda")
    assert _lib.lib().lenv_cont_env_reset(cfg.env_id, ptr(k), ptr(ep), n, ptr(st), ptr(obs), ptr(el), None) == 0
    torch.cuda.synchronize()
    return st.cpu().numpy().reshape(len(keys), T, SD), obs.cpu().numpy().reshape(len(keys), T, S)


def _run(kind, cfg, params, keys, offsets=None, reset_states=None, noise=None):
    """The entry through the C-ABI on buffers this test owns, every one pre-filled with a sentinel; host copies of everything."""
    from learning_environments_amd import _lib
    L = _lib.lib()
    S, A, SD = _dims(cfg)
    n, T = params.shape[0], cfg.test_episodes
    cap = int(L.lenv_actor_test_rows_cap(kind, C.byref(cfg)))
    assert cap == -(-cfg.max_steps // max(cfg.same_action_num, 1))
    f32 = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device="cuda")
    out = dict(returns=torch.full((n, T), SENTINEL, dtype=torch.float64, device="cuda"), env_steps=i32(n, T), agent_steps=i32(n, T),
               row_state=f32(n, T, cap, S), row_action=f32(n, T, cap, A), row_next_state=f32(n, T, cap, S), row_reward=f32(n, T, cap), row_done=f32(n, T, cap))
    p, k = dev(params), dev(keys.view(np.int64))
    off = dev(offsets) if offsets is not None else None
    rs = dev(reset_states) if reset_states is not None else None
    nz = dev(noise) if noise is not None else None
    assert nz is None or tuple(nz.shape) == (n, T, cap, A)
    rc = L.lenv_actor_test_population(kind, C.byref(cfg), ptr(p), ptr(k), ptr(off), ptr(rs), ptr(nz), n, ptr(out["returns"]), ptr(out["env_steps"]),
                                      ptr(out["agent_steps"]), *[ptr(out[f]) for f in ROW_FIELDS], None)
    assert rc == 0
    torch.cuda.synchronize()
    return {name: v.cpu().numpy() for name, v in out.items()}


def _compose(eng, orc, kind, cfg, params, states0, obs0, noise):
    """The same test step by step, all agents' episodes together: the actor's last Linear from lenv_mlp_forward, the action formula on the
    host in numpy fp32, lenv_cont_env_step once per repeat on the episodes that are still inside their agent step.  The arrays start filled
    with what _run pre-fills, so an equal comparison also shows which slots were never written.  Also returns, per slot, the bound of the
    reward's two roundings (0 where the agent step had one repeat)."""
    from learning_environments_amd import _lib
    L = _lib.lib()
    S, A, SD = _dims(cfg)
    n, T = params.shape[0], cfg.test_episodes
    k_rep = max(cfg.same_action_num, 1)
    cap = -(-cfg.max_steps // k_rep)
    N = n * T
    st = dev(states0.reshape(N, SD).copy())
    el = torch.zeros(N, dtype=torch.int32, device="cuda")
    cur = obs0.reshape(N, S).copy()
    desc = eng.mlp_desc(S, cfg.hidden, cfg.layers, A, cfg.act, use_layer_norm=bool(kind == TD3 and cfg.use_layer_norm))
    Pa, o = eng.mlp_num_params(desc), (0 if kind == TD3 else A)
    actors = [dev(params[i, o:o + Pa].copy()) for i in range(n)]
    exp = dict(row_state=np.full((n, T, cap, S), SENTINEL, np.float32), row_action=np.full((n, T, cap, A), SENTINEL, np.float32),
               row_next_state=np.full((n, T, cap, S), SENTINEL, np.float32), row_reward=np.full((n, T, cap), SENTINEL, np.float32),
               row_done=np.full((n, T, cap), SENTINEL, np.float32), agent_steps=np.zeros((n, T), np.int32))
    slack = np.zeros((n, T, cap), np.float64)
    ret32 = np.zeros(N, np.float32)
    alive = np.ones(N, bool)
    for step in range(cap):
        raw = np.zeros((N, A), np.float32)
        for i in range(n):
            raw[i * T:(i + 1) * T] = eng.mlp_forward(desc, actors[i], dev(cur[i * T:(i + 1) * T])).cpu().numpy()
        th = orc.tanhf(raw).reshape(N, A)
        z = noise[:, :, step, :].reshape(N, A).astype(np.float32)
        if kind == TD3:       # TD3.select_test_action: (actor(s) + randn * action_std * max_action).clamp(-max_action, max_action)
            ma, sd = np.float32(cfg.max_action), np.float32(cfg.action_std)
            v = th * ma + (z * sd) * ma
            act = np.where(v < -ma, -ma, np.where(v > ma, ma, v)).astype(np.float32)
        else:                 # Actor_PPO.forward of actor_old: action_std clamped to >= 0.001, tanh(net(s)) + std * z
            sd = np.repeat(np.maximum(params[:, :A], np.float32(0.001)), T, axis=0)
            act = (th + z * sd).astype(np.float32)
        running = alive.copy()
        rsum, rabs = np.zeros(N, np.float64), np.zeros(N, np.float64)
        nrep = np.zeros(N, np.int32)
        nxt, done = cur.copy(), np.zeros(N, np.float32)
        for _ in range(k_rep):
            idx = np.nonzero(running)[0]
            if idx.size == 0:
                break
            it = dev(idx.astype(np.int64))
            s_sub, e_sub, a_sub = st[it].contiguous(), el[it].contiguous(), dev(act[idx])
            o_sub = torch.zeros((idx.size, S), dtype=torch.float32, device="cuda")
            r_sub, d_sub = torch.zeros(idx.size, dtype=torch.float32, device="cuda"), torch.zeros(idx.size, dtype=torch.float32, device="cuda")
            assert L.lenv_cont_env_step(cfg.env_id, cfg.max_steps, idx.size, ptr(a_sub), ptr(s_sub), ptr(e_sub), ptr(o_sub), ptr(r_sub), ptr(d_sub), None) == 0
            st[it], el[it] = s_sub, e_sub
            r = r_sub.cpu().numpy().astype(np.float64)
            rsum[idx] += r
            rabs[idx] += np.abs(r)
            nrep[idx] += 1
            nxt[idx], done[idx] = o_sub.cpu().numpy(), d_sub.cpu().numpy()
            running[idx] = done[idx] < 0.5
        for j in np.nonzero(alive)[0]:
            i, e = divmod(int(j), T)
            exp["row_state"][i, e, step], exp["row_action"][i, e, step], exp["row_next_state"][i, e, step] = cur[j], act[j], nxt[j]
            exp["row_reward"][i, e, step], exp["row_done"][i, e, step] = np.float32(rsum[j]), done[j]
            slack[i, e, step] = (rabs[j] + abs(rsum[j])) * 2.0 ** -24 if nrep[j] > 1 else 0.0
            exp["agent_steps"][i, e] += 1
        cur = nxt
        alive &= done < 0.5
        if not alive.any():
            break
    exp["env_steps"] = el.cpu().numpy().reshape(n, T)
    return exp, slack


def _assert_equals_composition(got, exp, slack, cfg, label):
    for name in ("agent_steps", "env_steps", "row_state", "row_action", "row_next_state", "row_done"):
        assert np.array_equal(got[name], exp[name]), (label, name)
    if max(cfg.same_action_num, 1) == 1:
        assert slack.max() == 0.0
        assert np.array_equal(got["row_reward"], exp["row_reward"]), (label, "row_reward")
    else:
        err = np.abs(got["row_reward"].astype(np.float64) - exp["row_reward"].astype(np.float64))
        print(label, "row_reward: max |kernel - fp32(sum of the fp32 step rewards)| =", err.max(), "bound there", slack.reshape(-1)[err.argmax()])
        assert (err <= slack).all(), (label, "row_reward", err.max())
    # the episode return is the fp32 running sum of the kernel's own fp32 rewards; slots no step filled hold the sentinel
    n, T, cap = got["row_reward"].shape
    filled = np.arange(cap)[None, None, :] < got["agent_steps"][:, :, None]
    ret = np.zeros((n, T), np.float32)
    for s in range(cap):
        ret = np.where(filled[:, :, s], (ret + got["row_reward"][:, :, s]).astype(np.float32), ret)
    assert np.array_equal(got["returns"], ret.astype(np.float64)), (label, "returns")
    for name in ROW_FIELDS:
        assert (got[name][~filled] == SENTINEL).all(), (label, name)
    assert (got["agent_steps"] >= 1).all() and np.array_equal(got["agent_steps"], -(-got["env_steps"] // max(cfg.same_action_num, 1)))
    ii, ee = np.meshgrid(np.arange(n), np.arange(T), indexing="ij")
    assert (got["row_done"][ii, ee, got["agent_steps"] - 1] == 1.0).all() and got["row_done"][filled].sum() == n * T


def _case(eng, orc, kind, env, H, L, T, max_steps, san=1, act="relu", ln=False, given_resets=True, flag=None, seed=0, label=""):
    cfg = _cfg(kind, env, H, L, T, max_steps, san=san, act=act, ln=ln)
    S, A, SD = _dims(cfg)
    params, keys = _population(eng, kind, cfg, 3, seed)
    resets, obs0 = _resets(cfg, keys, OFFSETS)
    if flag is not None:                                  # MountainCarContinuous: an episode that starts next to the flag, moving right
        resets[flag] = (0.449, 0.05)
        obs0[flag] = np.array([0.449, 0.05]).astype(np.float32)
    cap = -(-max_steps // max(san, 1))
    noise = np.random.RandomState(seed + 1).standard_normal((3, T, cap, A)).astype(np.float32)
    got = _run(kind, cfg, params, keys, OFFSETS, reset_states=resets if given_resets else None, noise=noise)
    exp, slack = _compose(eng, orc, kind, cfg, params, resets, obs0, noise)
    _assert_equals_composition(got, exp, slack, cfg, label)
    return cfg, got


# ---- (a) the closing test of the fused loops ----

def _fused_config(kind, env, E, T=3, ln=False):
    """Small nets on the env's RewardEnv config: 24 x 2 agent nets, a 16-wide one-layer reward net, episodes of 9 steps."""
    from learning_environments_amd import configs
    c = {"pendulum": configs.pendulum_reward_env_td3, "cmc": configs.cmc_reward_env_td3, "cheetah": configs.halfcheetah_reward_env_td3}[env](2)
    name = c["env_name"]
    c["envs"][name].update(max_steps=9, hidden_size=16, hidden_layer=1, activation_fn="tanh", solved_reward=1e9)
    san = c["agents"]["td3"]["same_action_num"]           # MountainCarContinuous ships 2: the last repeat of an episode is cut by TimeLimit
    if kind == TD3:
        c["agents"]["td3"].update(train_episodes=E, test_episodes=T, init_episodes=1, hidden_size=24, hidden_layer=2, batch_size=16, use_layer_norm=ln)
    else:
        c["agents"]["gtn"]["agent_name"] = "ppo"
        c["agents"]["ppo"] = dict(train_episodes=E, test_episodes=T, init_episodes=0, update_episodes=1, ppo_epochs=2, gamma=0.99, lr=3e-4, vf_coef=1, ent_coef=0.01,
                                  eps_clip=0.2, rb_size=1000000, same_action_num=san, activation_fn="tanh", hidden_size=24, hidden_layer=2, action_std=0.5,
                                  print_rate=100, early_out_num=10, early_out_virtual_diff=0.02)
    return c


def _fused_run(eng, kind, cfg, p_theta, chains, seed, std=None):
    rng = np.random.RandomState(seed)
    il = (eng.Td3InnerLoop if kind == TD3 else eng.PpoInnerLoop)(cfg, chains, want_final_params=True)
    assert il.p_agent == eng.actor_test_num_params(kind, cfg)
    theta = (rng.randn(p_theta) * 0.1).astype(np.float32)
    init = rng.uniform(-0.3, 0.3, (chains, il.p_agent)).astype(np.float32)
    if std is not None:
        init[:, :cfg.action_dim] = np.asarray(std, np.float32)[:, None]
    keys = rng.randint(1, 2 ** 62, size=chains).astype(np.uint64)
    il.run(dev(theta), dev(np.zeros((1, p_theta), np.float32)), dev(np.zeros(chains, np.int32)), dev(np.zeros(chains, np.float32)), dev(init),
           rng_keys=dev(keys.view(np.int64)))
    torch.cuda.synchronize()
    assert il.status.cpu().tolist() == [0] * chains
    return il, init, keys


def _assert_entry_equals_closing_test(eng, kind, cfg, il, keys, E, label):
    stats = il.stats.cpu().numpy()
    assert (stats[:, 0] == E).all(), (label, stats)
    T = cfg.test_episodes
    offsets = (stats[:, 0] * T).astype(np.int64)          # test_mode 0: T test episodes after every training episode, then the closing test
    got = eng.actor_test_population(kind, cfg, il.final_params, dev(keys.view(np.int64)), episode_offset=dev(offsets), want_rows=False)
    assert sorted(got) == ["agent_steps", "env_steps", "returns"]
    ret, fin = got["returns"].cpu().numpy(), il.final_returns.cpu().numpy()
    assert np.array_equal(ret, fin), (label, ret, fin)
    if E == 0:
        assert np.array_equal(got["env_steps"].cpu().numpy().sum(axis=1), stats[:, 3]), label       # test_steps of a launch that only tested
    assert len(set(ret.reshape(-1).tolist())) > 1, label                                           # (the returns do tell episodes apart)


@pytest.mark.parametrize("E", [3, 0])
@pytest.mark.parametrize("env", sorted(ENVS))
@pytest.mark.parametrize("kind", [TD3, PPO], ids=["td3", "ppo"])
def test_returns_equal_the_fused_loops_final_returns(eng, kind, env, E):
    """2 (PPO: 3) chains train E episodes (T test episodes after each), then the launch's closing test.  The entry on final_params with the
    chains' keys and episode_offset = episodes_run * T gives final_returns bit for bit.  TD3 on MountainCarContinuous carries the shared
    LayerNorm; without training PPO's chain 1 has action_std 0.0005: its final_params row keeps it, below actor_old's clamp."""
    from learning_environments_amd.config import ppo_cfg_from_config, td3_cfg_from_config
    cfgd = _fused_config(kind, env, E, ln=(env == "cmc"))
    cfg = (td3_cfg_from_config if kind == TD3 else ppo_cfg_from_config)(cfgd)
    p_theta = eng.rn_num_params(cfg.reward_env_type, cfg.state_dim, cfg.info_dim, cfg.rn_hidden, cfg.rn_layers)
    chains = 2 if kind == TD3 else 3
    il, init, keys = _fused_run(eng, kind, cfg, p_theta, chains, seed=5 + E, std=None if kind == TD3 else [0.5, 0.0005 if E == 0 else 0.3, 0.2])
    label = ("td3" if kind == TD3 else "ppo", env, E)
    _assert_entry_equals_closing_test(eng, kind, cfg, il, keys, E, label)
    fp = il.final_params.cpu().numpy()
    if E == 0:
        assert np.array_equal(fp, init)
        if kind == PPO:
            assert (fp[1, :cfg.action_dim] < 0.001).all()
    else:
        assert not np.array_equal(fp, init)               # training moved the agents (PPO: two learn calls)
        if kind == PPO:
            assert (il.stats.cpu().numpy()[:, 2] >= 1).all()


@pytest.mark.parametrize("variant", ["wavechain", "gemm_queue"])
def test_returns_equal_the_wavechain_td3_closing_test(eng, variant):
    """default_config_pendulum.yaml's td3 shape (128 x 2, batch 256, ten test episodes, a VirtualEnv of three 4-32-32-x nets) takes the
    wave-chain kernel; with kernel_variant GENERIC | NO_WAVECHAIN the same launch runs on the GEMM-queue kernel.  Both closing tests are the
    entry's returns."""
    from learning_environments_amd import _lib, configs
    from learning_environments_amd.config import td3_cfg_from_config
    E = 2
    cfgd = configs.fixed_work(configs.pendulum_syn_env_td3(2), E)
    cfgd["agents"]["td3"].update(init_episodes=1)
    cfgd["envs"]["Pendulum-v0"]["max_steps"] = 20
    cfg = td3_cfg_from_config(cfgd)
    assert (cfg.hidden, cfg.layers, cfg.batch_size, cfg.test_episodes, cfg.virtual_env, cfg.policy_delay) == (128, 2, 256, 10, 1, 2)
    if variant == "gemm_queue":
        cfg.kernel_variant = _lib.VARIANT_GENERIC | _lib.VARIANT_NO_WAVECHAIN
    e = cfgd["envs"]["Pendulum-v0"]
    p_theta = sum(eng.mlp_num_params(d) for d in eng.se_descs(cfg.state_dim, cfg.action_dim, e["hidden_size"], e["hidden_layer"], e["activation_fn"]))
    il, init, keys = _fused_run(eng, TD3, cfg, p_theta, 2, seed=31)
    _assert_entry_equals_closing_test(eng, TD3, cfg, il, keys, E, ("td3", variant))


# ---- (b) composition of the existing one-step entries ----

COMPOSE_CASES = {
    "td3_cheetah": dict(kind=TD3, env="cheetah", H=24, L=2, T=3, max_steps=6),
    "ppo_cheetah": dict(kind=PPO, env="cheetah", H=24, L=2, T=3, max_steps=6, act="tanh"),
    "td3_pendulum": dict(kind=TD3, env="pendulum", H=16, L=1, T=3, max_steps=8, act="leakyrelu"),
    "ppo_pendulum": dict(kind=PPO, env="pendulum", H=16, L=2, T=3, max_steps=8),
    "td3_cmc": dict(kind=TD3, env="cmc", H=16, L=2, T=3, max_steps=8, act="tanh"),
    "ppo_cmc": dict(kind=PPO, env="cmc", H=16, L=1, T=3, max_steps=8),
}


@pytest.mark.parametrize("case", sorted(COMPOSE_CASES))
def test_rows_equal_the_composition_of_the_step_entries(eng, orc, case):
    """3 agents, given reset states and a given noise tape."""
    cfg, got = _case(eng, orc, seed=23, label=case, **COMPOSE_CASES[case])
    assert (got["env_steps"] == cfg.max_steps).all()      # nobody reaches the flag from the valley in 8 steps


# ---- (c) edges ----

EDGE_CASES = {
    "T1_width5_one_layer": dict(kind=PPO, env="pendulum", H=5, L=1, T=1, max_steps=5),
    "T16_width33_three_layers_ln": dict(kind=TD3, env="pendulum", H=33, L=3, T=16, max_steps=5, ln=True, act="tanh"),
    "T17_second_block_ln_repeat3_drawn_resets": dict(kind=TD3, env="cmc", H=33, L=3, T=17, max_steps=7, san=3, ln=True, given_resets=False),
    "T17_second_block_ppo_cheetah_width5": dict(kind=PPO, env="cheetah", H=5, L=2, T=17, max_steps=4, act="leakyrelu", given_resets=False),
    "repeat3_cut_by_timelimit_ppo": dict(kind=PPO, env="pendulum", H=33, L=2, T=3, max_steps=7, san=3),
    "td3_three_layers_no_ln_width5": dict(kind=TD3, env="cheetah", H=5, L=3, T=2, max_steps=4),
    "streamed_actor_17_384_384_384_6": dict(kind=TD3, env="cheetah", H=384, L=3, T=2, max_steps=3),
    "streamed_actor_ln": dict(kind=TD3, env="cheetah", H=384, L=3, T=2, max_steps=3, ln=True, act="tanh"),
    "streamed_actor_ppo_17_128_128_6": dict(kind=PPO, env="cheetah", H=128, L=2, T=2, max_steps=3, act="tanh"),
    "staged_actor_ppo_17_120_120_6": dict(kind=PPO, env="cheetah", H=120, L=2, T=2, max_steps=3, act="tanh"),
}


@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_edges_equal_the_composition(eng, orc, case):
    spec = EDGE_CASES[case]
    cfg, got = _case(eng, orc, seed=41, label=case, **spec)
    if spec.get("san", 1) == 3:
        assert (got["env_steps"] == 7).all() and (got["agent_steps"] == 3).all()                    # 3 + 3 + 1: TimeLimit cuts the last repeat
    # the entry stages the actor where it fits next to the two activation buffers [T][H] in half a CU's LDS less 8 KiB; 120 wide still does
    lds = 4 * (eng.mlp_num_params(eng.mlp_desc(17, spec["H"], spec["L"], 6, "relu", use_layer_norm=spec.get("ln", False))) + 2 * spec["T"] * spec["H"])
    if case.startswith("streamed"):
        assert lds > 80 * 1024 - 8192
    if case.startswith("staged"):
        assert lds <= 80 * 1024 - 8192


@pytest.mark.parametrize("kind", [TD3, PPO], ids=["td3", "ppo"])
def test_flag_in_the_first_step_beside_a_full_length_episode(eng, orc, kind):
    """MountainCarContinuous from (0.449, 0.05): the car passes 0.45 moving right whatever the force, the episode ends in its first env step
    (inside the first agent step of same_action_num 2) with the bonus of 100 and idles while its neighbours in the block run to max_steps."""
    cfg, got = _case(eng, orc, kind, "cmc", H=8, L=1, T=2, max_steps=6, san=2, flag=(1, 0), seed=57, label="flag")
    assert got["env_steps"][1, 0] == 1 and got["agent_steps"][1, 0] == 1 and got["row_done"][1, 0, 0] == 1.0
    assert got["row_reward"][1, 0, 0] > 99.0 and got["returns"][1, 0] == np.float64(got["row_reward"][1, 0, 0])
    assert (got["row_reward"][1, 0, 1:] == SENTINEL).all() and (got["row_action"][1, 0, 1:] == SENTINEL).all()
    others = np.ones((3, 2), bool)
    others[1, 0] = False
    assert (got["env_steps"][others] == 6).all() and (got["agent_steps"][others] == 3).all()


# ---- (d) test_actor_agents ----

@pytest.mark.parametrize("kind", [TD3, PPO], ids=["td3", "ppo"])
def test_test_actor_agents_returns_the_entrys_rows(eng, kind):
    """The triples of rollout.test_actor_agents: returns, lengths in agent steps, and ReplayRows that concatenate to the rows of the entry
    (C-ABI call on the cfg the config builders give, same keys and offsets), episode after episode."""
    from learning_environments_amd.agents.rollout import ReplayRows, test_actor_agents
    from learning_environments_amd.config import ppo_cfg_from_config, td3_cfg_from_config
    from learning_environments_amd import configs
    cfgd = _fused_config(kind, "cheetah" if kind == TD3 else "cmc", 0)
    if kind == TD3:
        cfgd = configs.with_vary(cfgd, vary_hp=False)      # td3_vary with vary_hp off IS td3
    cfg = (td3_cfg_from_config if kind == TD3 else ppo_cfg_from_config)(cfgd, test_episodes=4, max_steps=5)
    S, A, SD = _dims(cfg)
    params, keys = _population(eng, kind, cfg, 3, seed=77)
    triples = test_actor_agents(cfgd, params, keys, episode_offset=OFFSETS, test_episodes=4, max_steps=5)
    got = _run(kind, cfg, params, keys, OFFSETS)
    merged = ReplayRows(S, action_dim=A)
    for i, (reward_list, length_list, rows) in enumerate(triples):
        assert reward_list == got["returns"][i].tolist() and length_list == got["agent_steps"][i].tolist()
        assert rows.action_dim == A and rows.get_size() == sum(length_list)
        merged.merge_buffer(rows)
    filled = np.arange(got["row_reward"].shape[2])[None, None, :] < got["agent_steps"][:, :, None]
    want = (got["row_state"][filled], got["row_action"][filled], got["row_next_state"][filled], got["row_reward"][filled][:, None], got["row_done"][filled][:, None])
    for a, b in zip(merged.get_all(), want):
        assert a.dtype == torch.float32 and np.array_equal(a.numpy(), b)
    assert merged.get_size() == int(got["agent_steps"].sum()) > 0
    # the same episodes again under a scalar offset: agent 1 has offset 0 in OFFSETS
    again = test_actor_agents(cfgd, params[1:2], keys[1:2], test_episodes=4, max_steps=5)
    assert again[0][0] == triples[1][0]
    for a, b in zip(again[0][2].get_all(), triples[1][2].get_all()):
        assert torch.equal(a, b)
