"""lenv_td3d_test_population (csrc/discrete_actor_test_population.hip) and lenv_ql_test_population (csrc/ql_test_population.hip): BaseAgent.test
of a population of TD3_discrete_vary agents / tabular agents in one launch.  Everything is held bit for bit unless stated:

1. against the closing test of the fused TD3-discrete loops in counter mode (VirtualEnv and RewardEnv launches, the three envs, LayerNorm and
   the hard head on and off, with training -- the temperature has moved -- and without, test_mode 0 and 1), on their final_params rows;
2. against a composition on the host from given reset states and gumbel / noise tapes: the oracle's td3d_actor_forward at the oracle's
   temperature, the noise added in numpy fp32, the first-maximum argmax, lenv_real_env_step: every row field, both step counts, the returns
   and the sentinel in the slots no step filled;
3. the temperature's edges and 4. the kernel's edges against the same composition; 5. ties;
6. a run of the reference (a CartPole chain fixture of test_td3_discrete.py), re-laid from its tapes: the fixture's final returns;
7. through rollout.test_discrete_actor_agents and histogram.collect;
8. the tabular entry: the closing test of the fused tabular loops, a numpy walk, a reference Q-table, gridworld_heatmap."""
import ctypes as C
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
ROW_FIELDS = ("row_state", "row_action", "row_next_state", "row_reward", "row_done")
ENVS = {"cartpole": (0, 4, 2), "acrobot": (1, 6, 3), "mountaincar": (3, 2, 3)}
OFFSETS = np.array([3, 0, 1000000007], np.int64)
STREAM_TD3_TEST_NOISE, STREAM_TD3D_GUMBEL_TEST = 7, 14


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


def _kw(env, H, L, T, max_steps, ln=False, hard=False, act=3, temp=1.5, astd=0.1, **over):
    """A complete cfg (the fused entries read all of it); act 3 = tanh."""
    env_id, S, A = ENVS[env]
    kw = dict(env_id=env_id, state_dim=S, action_dim=A, max_steps=max_steps, se_hidden=12, se_layers=1, se_act=2, se_prelu=0.25, hidden=H, layers=L,
              act=act, prelu=0.25, use_layer_norm=1 if ln else 0, gumbel_hard=1 if hard else 0, batch_size=8, rb_size=1000, train_episodes=0,
              test_episodes=T, init_episodes=1, early_out_num=2, policy_delay=2, rng_mode=0, solved_reward=1e9, gamma=0.99, lr=1e-3, tau=0.01,
              action_std=astd, policy_std=0.2, policy_std_clip=0.5, max_action=1.0, gumbel_temp=temp, adam_beta1=0.9, adam_beta2=0.999,
              adam_eps=1e-8, step_budget=0, se_layer_norm=0, test_mode=0, early_out_virtual_diff=0.01)
    kw.update(over)
    return kw


def _cfgs(orc, **kw):
    from learning_environments_amd import _lib
    return orc.Td3dCfg(**kw), _lib.Td3dCfg(**kw)


def _population(eng, cfg, n, seed, scale=2.0):
    """n agents: parameter rows uniform in +-scale / sqrt(H) and keys."""
    rng = np.random.RandomState(seed)
    b = scale / np.sqrt(cfg.hidden)
    params = rng.uniform(-b, b, (n, eng.td3d_test_num_params(cfg))).astype(np.float32)
    keys = rng.randint(1, 2 ** 62, size=n).astype(np.uint64)
    return params, keys


def _resets(cfg, keys, offsets):
    """(fp64 states [agents,T,4], fp32 observations [agents,T,S]) of the episodes offsets[i] + e, from lenv_real_env_reset."""
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


def _obs_of(cfg, states):
    """the fp32 observation of given fp64 env states (CartPole / MountainCar: the state words themselves)"""
    assert cfg.env_id in (0, 3)
    return states[..., :cfg.state_dim].astype(np.float32)


def _run(cfg, params, keys, offsets=None, learn_calls=None, reset_states=None, gumbel=None, noise=None):
    """The entry through the C-ABI on buffers this test owns, every one pre-filled with a sentinel; host copies of everything."""
    from learning_environments_amd import _lib
    L = _lib.lib()
    n, T, S, A = params.shape[0], cfg.test_episodes, cfg.state_dim, cfg.action_dim
    cap = int(L.lenv_td3d_test_rows_cap(C.byref(cfg)))
    assert cap == cfg.max_steps
    f32 = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device="cuda")
    out = dict(returns=torch.full((n, T), SENTINEL, dtype=torch.float64, device="cuda"), env_steps=i32(n, T), agent_steps=i32(n, T),
               row_state=f32(n, T, cap, S), row_action=f32(n, T, cap, A), row_next_state=f32(n, T, cap, S), row_reward=f32(n, T, cap), row_done=f32(n, T, cap))
    opt = lambda a, dt=None: None if a is None else dev(np.asarray(a, dt) if dt else a)
    p, k = dev(params), dev(keys.view(np.int64))
    off, lc, rs, gm, nz = opt(offsets, np.int64), opt(learn_calls, np.int64), opt(reset_states), opt(gumbel), opt(noise)
    for t in (gm, nz):
        assert t is None or tuple(t.shape) == (n, T, cap, A)
    rc = L.lenv_td3d_test_population(C.byref(cfg), ptr(p), ptr(k), ptr(off), ptr(lc), ptr(rs), ptr(gm), ptr(nz), n, ptr(out["returns"]),
                                     ptr(out["env_steps"]), ptr(out["agent_steps"]), *[ptr(out[f]) for f in ROW_FIELDS], None)
    assert rc == 0
    torch.cuda.synchronize()
    return {name: v.cpu().numpy() for name, v in out.items()}


def _counter_tapes(orc, cfg, keys, offsets, which):
    """the draws of the keys' own streams, laid out as a tape [agents,T,cap,A]: index ((offset + e) * max_steps + step) * A + k"""
    lib = orc.lib()
    lib.orc_normal.restype = C.c_double
    n, T, cap, A = len(keys), cfg.test_episodes, cfg.max_steps, cfg.action_dim
    out = np.zeros((n, T, cap, A), np.float32)
    for i in range(n):
        for e in range(T):
            for s in range(cap):
                for k in range(A):
                    idx = ((int(offsets[i]) + e) * cap + s) * A + k
                    if which == "gumbel":
                        out[i, e, s, k] = orc.gumbel(int(keys[i]), STREAM_TD3D_GUMBEL_TEST, idx)
                    else:
                        out[i, e, s, k] = np.float32(lib.orc_normal(C.c_uint64(int(keys[i])), C.c_uint32(STREAM_TD3_TEST_NOISE), C.c_uint64(idx)))
    return out


def _compose(orc, ocfg, cfg, params, states0, obs0, gumbel, noise, learn_calls):
    """The same test step by step, all agents' episodes together: the oracle's actor with its Gumbel-softmax head at the oracle's temperature
    of index max(L - 1, 0), the noise added in numpy fp32, numpy's argmax (the first maximum), lenv_real_env_step (its done has TimeLimit in).
    The arrays start filled with what _run pre-fills, so an equal comparison also shows which slots were never written."""
    from learning_environments_amd import _lib
    L = _lib.lib()
    n, T, S, A, cap = params.shape[0], cfg.test_episodes, cfg.state_dim, cfg.action_dim, cfg.max_steps
    N = n * T
    Pa = orc.td3d_num_params(ocfg)[1]
    st = dev(states0.reshape(N, 4).copy())
    el = torch.zeros(N, dtype=torch.int32, device="cuda")
    cur = obs0.reshape(N, S).copy()
    taus = [orc.td3d_temperature(ocfg, max(int(lc) - 1, 0)) for lc in learn_calls]
    sd = np.float32(cfg.action_std)
    exp = dict(row_state=np.full((n, T, cap, S), SENTINEL, np.float32), row_action=np.full((n, T, cap, A), SENTINEL, np.float32),
               row_next_state=np.full((n, T, cap, S), SENTINEL, np.float32), row_reward=np.full((n, T, cap), SENTINEL, np.float32),
               row_done=np.full((n, T, cap), SENTINEL, np.float32), agent_steps=np.zeros((n, T), np.int32))
    ret32 = np.zeros(N, np.float32)
    alive = np.ones(N, bool)
    for step in range(cap):
        y = np.zeros((N, A), np.float32)
        for i in range(n):
            y[i * T:(i + 1) * T] = orc.td3d_actor_forward(ocfg, params[i, :Pa], cur[i * T:(i + 1) * T], gumbel[i, :, step, :], taus[i])
        act = (y + (noise[:, :, step, :].reshape(N, A).astype(np.float32) * sd).astype(np.float32)).astype(np.float32)
        idx = np.nonzero(alive)[0]
        it = dev(idx.astype(np.int64))
        s_sub, e_sub, a_sub = st[it].contiguous(), el[it].contiguous(), dev(np.argmax(act[idx], axis=1).astype(np.int32))
        o_sub = torch.zeros((idx.size, S), dtype=torch.float32, device="cuda")
        r_sub, d_sub = torch.zeros(idx.size, dtype=torch.float32, device="cuda"), torch.zeros(idx.size, dtype=torch.float32, device="cuda")
        assert L.lenv_real_env_step(cfg.env_id, cfg.max_steps, idx.size, ptr(a_sub), ptr(s_sub), ptr(e_sub), ptr(o_sub), ptr(r_sub), ptr(d_sub), None) == 0
        st[it], el[it] = s_sub, e_sub
        nxt, done, rew = cur.copy(), np.zeros(N, np.float32), np.zeros(N, np.float32)
        nxt[idx], done[idx], rew[idx] = o_sub.cpu().numpy(), d_sub.cpu().numpy(), r_sub.cpu().numpy()
        for j in idx:
            i, e = divmod(int(j), T)
            exp["row_state"][i, e, step], exp["row_action"][i, e, step], exp["row_next_state"][i, e, step] = cur[j], act[j], nxt[j]
            exp["row_reward"][i, e, step], exp["row_done"][i, e, step] = rew[j], done[j]
            ret32[j] = np.float32(ret32[j] + rew[j])
            exp["agent_steps"][i, e] += 1
        cur = nxt
        alive &= done < 0.5
        if not alive.any():
            break
    exp["returns"] = ret32.astype(np.float64).reshape(n, T)
    exp["env_steps"] = el.cpu().numpy().reshape(n, T)
    return exp


def _assert_equal(got, exp, label):
    for name in ("agent_steps", "env_steps", "row_state", "row_action", "row_next_state", "row_reward", "row_done", "returns"):
        assert np.array_equal(got[name], exp[name]), (label, name)
    n, T, cap = got["row_reward"].shape
    filled = np.arange(cap)[None, None, :] < got["agent_steps"][:, :, None]
    for name in ROW_FIELDS:
        assert (got[name][~filled] == SENTINEL).all(), (label, name)
    assert (got["agent_steps"] >= 1).all() and np.array_equal(got["agent_steps"], got["env_steps"])
    ii, ee = np.meshgrid(np.arange(n), np.arange(T), indexing="ij")
    assert (got["row_done"][ii, ee, got["agent_steps"] - 1] == 1.0).all() and got["row_done"][filled].sum() == n * T


def _case(eng, orc, env, H, L, T, max_steps, ln=False, hard=False, act=3, learn_calls=(0, 7, 2500), given="both", given_resets=True, first_step_done=None,
          seed=0, label="", **over):
    ocfg, cfg = _cfgs(orc, **_kw(env, H, L, T, max_steps, ln=ln, hard=hard, act=act, **over))
    n = len(learn_calls)
    offsets = np.resize(OFFSETS, n)
    params, keys = _population(eng, cfg, n, seed)
    resets, obs0 = _resets(cfg, keys, offsets)
    if first_step_done is not None:                       # CartPole: the pole just inside its 12 degrees with a large angular velocity
        resets[first_step_done] = (0.0, 0.0, 12 * 2 * np.pi / 360 - 0.001, 3.0)
        obs0[first_step_done] = _obs_of(cfg, resets[first_step_done])
    A = cfg.action_dim
    rng = np.random.RandomState(seed + 1)
    gumbel = -np.log(-np.log(rng.uniform(1e-6, 1 - 1e-6, (n, T, max_steps, A)))).astype(np.float32)
    noise = rng.standard_normal((n, T, max_steps, A)).astype(np.float32)
    if given == "gumbel":
        noise = _counter_tapes(orc, cfg, keys, offsets, "noise")
    if given == "noise":
        gumbel = _counter_tapes(orc, cfg, keys, offsets, "gumbel")
    got = _run(cfg, params, keys, offsets, learn_calls=learn_calls, reset_states=resets if given_resets else None,
               gumbel=gumbel if given in ("both", "gumbel") else None, noise=noise if given in ("both", "noise") else None)
    exp = _compose(orc, ocfg, cfg, params, resets, obs0, gumbel, noise, learn_calls)
    _assert_equal(got, exp, label)
    return cfg, got


# ---- 1. the closing test of the fused loops, counter mode ----

FUSED_CASES = [   # env, RewardEnv launch, LayerNorm, hard head, train_episodes, test_mode
    ("cartpole", False, False, True, 3, 0), ("cartpole", True, True, False, 3, 0), ("cartpole", False, True, True, 0, 0), ("cartpole", True, False, False, 3, 1),
    ("acrobot", False, True, False, 3, 0), ("acrobot", True, False, True, 0, 0), ("acrobot", True, True, True, 3, 0),
    ("mountaincar", False, False, False, 3, 0), ("mountaincar", True, True, True, 3, 0), ("mountaincar", False, True, False, 0, 0),
]


@pytest.mark.parametrize("env,renv,ln,hard,E,test_mode", FUSED_CASES)
def test_returns_equal_the_fused_loops_final_returns(eng, orc, env, renv, ln, hard, E, test_mode):
    """3 chains (hidden 16 x 2, batch 8, episodes of 20 steps, three test episodes) train E episodes, the first one at random, then the
    launch's closing test.  The entry on final_params with the chains' keys, episode_offset = episodes_run * T (0 under test_mode 1) and
    learn_calls = stats[:, 2] gives final_returns bit for bit."""
    from learning_environments_amd import _lib
    _, cfg = _cfgs(orc, **_kw(env, 16, 2, 3, 20, ln=ln, hard=hard, train_episodes=E, test_mode=test_mode))
    rn = _lib.Td3dRnCfg(synthetic_env_type=1, reward_env_type=2, rn_hidden=16, rn_layers=1, rn_act=3, rn_prelu=0.25, rn_layer_norm=0) if renv else None
    chains = 3
    il = eng.Td3DiscreteInnerLoop(cfg, chains, want_final_params=True, rn=rn)
    assert il.p_agent == eng.td3d_test_num_params(cfg)
    rng = np.random.RandomState(5 + E)
    keys = rng.randint(1, 2 ** 62, size=chains).astype(np.uint64)
    kt = dev(keys.view(np.int64))
    init = il.draw_agent_init(kt).cpu().numpy().copy()
    theta = (rng.randn(il.p_theta) * 0.3).astype(np.float32)
    il.run(dev(theta), dev(np.zeros((1, il.p_theta), np.float32)), dev(np.zeros(chains, np.int32)), dev(np.zeros(chains, np.float32)), None, rng_keys=kt)
    torch.cuda.synchronize()
    assert il.status.cpu().tolist() == [0] * chains
    stats = il.stats.cpu().numpy()
    label = (env, renv, ln, hard, E, test_mode)
    assert (stats[:, 0] == E).all(), (label, stats)
    T = cfg.test_episodes
    offsets = (stats[:, 0] * T * (0 if test_mode == 1 else 1)).astype(np.int64)
    got = eng.td3d_test_population(cfg, il.final_params, kt, episode_offset=dev(offsets), learn_calls=il.stats[:, 2].contiguous(), want_rows=False)
    assert sorted(got) == ["agent_steps", "env_steps", "returns"]
    ret, fin = got["returns"].cpu().numpy(), il.final_returns.cpu().numpy()
    assert np.array_equal(ret, fin), (label, ret, fin)
    fp = il.final_params.cpu().numpy()
    if E == 0:
        assert np.array_equal(fp, init) and (stats[:, 2] == 0).all()
        assert np.array_equal(got["env_steps"].cpu().numpy().sum(axis=1), stats[:, 3]), label       # test_steps of a launch that only tested
    else:
        assert not np.array_equal(fp, init) and (stats[:, 2] > 1).all(), (label, stats)             # learn calls happened: the temperature has moved


# ---- 2. composition on the host ----

COMPOSE_CASES = {
    "cartpole_soft": dict(env="cartpole", H=24, L=2, T=3, max_steps=12),
    "cartpole_hard_ln": dict(env="cartpole", H=24, L=2, T=3, max_steps=12, ln=True, hard=True, act=1),
    "acrobot_soft_ln": dict(env="acrobot", H=20, L=3, T=3, max_steps=8, ln=True, act=2),
    "acrobot_hard": dict(env="acrobot", H=20, L=1, T=3, max_steps=8, hard=True),
    "mountaincar_soft": dict(env="mountaincar", H=16, L=2, T=3, max_steps=10, astd=0.5),
    "mountaincar_hard_ln": dict(env="mountaincar", H=16, L=2, T=3, max_steps=10, ln=True, hard=True),
}


@pytest.mark.parametrize("case", sorted(COMPOSE_CASES))
def test_rows_equal_the_composition_on_the_host(eng, orc, case):
    """3 agents (0, 7 and 2500 learn calls), given reset states and given gumbel / noise tapes."""
    cfg, got = _case(eng, orc, seed=23, label=case, **COMPOSE_CASES[case])
    if not case.startswith("cartpole"):
        assert (got["env_steps"] == cfg.max_steps).all()  # neither Acrobot nor MountainCar ends within a dozen steps
    a = got["row_action"][got["row_action"] != SENTINEL].reshape(-1, cfg.action_dim)
    assert len(set(a.argmax(axis=1).tolist())) > 1, case  # (the actions do vary)


# ---- 3. the temperature's edges ----

def test_temperature_edges(eng, orc):
    """learn_calls 0 and 1 share the schedule's first entry, 2000 and above its last; a soft head shows the temperature in every action."""
    lcs = (0, 1, 2, 1999, 2000, 2001, 5000)
    ocfg, cfg = _cfgs(orc, **_kw("cartpole", 16, 2, 2, 6, temp=2.3076235))
    assert [orc.td3d_temperature(ocfg, max(l - 1, 0)) for l in lcs] == [orc.td3d_temperature(ocfg, i) for i in (0, 0, 1, 1998, 1999, 1999, 1999)]
    _, got = _case(eng, orc, "cartpole", 16, 2, 2, 6, temp=2.3076235, learn_calls=lcs, seed=31, label="temperature")
    # the same agent under every count: equal where the temperature is equal, different where it differs
    params, keys = _population(eng, cfg, 1, 77)
    rep = lambda a: np.repeat(a, len(lcs), axis=0)
    resets, _ = _resets(cfg, keys, OFFSETS[:1])
    rng = np.random.RandomState(1)
    gm, nz = rng.standard_normal((1, 2, 6, 2)).astype(np.float32), rng.standard_normal((1, 2, 6, 2)).astype(np.float32)
    same = _run(cfg, rep(params), rep(keys), learn_calls=lcs, reset_states=rep(resets), gumbel=rep(gm), noise=rep(nz))
    acts = same["row_action"]
    assert np.array_equal(acts[0], acts[1]) and np.array_equal(acts[4], acts[5]) and np.array_equal(acts[4], acts[6])
    assert not np.array_equal(acts[1], acts[2]) and not np.array_equal(acts[3], acts[4])


# ---- 4. the kernel's edges ----

EDGE_CASES = {
    "T1_width5_one_layer": dict(env="cartpole", H=5, L=1, T=1, max_steps=7),
    "T16_width33_three_layers_ln": dict(env="mountaincar", H=33, L=3, T=16, max_steps=7, ln=True),
    "T17_second_block_drawn_resets": dict(env="acrobot", H=33, L=2, T=17, max_steps=7, ln=True, hard=True, given_resets=False),
    "T17_width5_three_layers_no_ln": dict(env="cartpole", H=5, L=3, T=17, max_steps=7, given_resets=False),
    "streamed_actor_6_512_512_512_3_ln": dict(env="acrobot", H=512, L=3, T=2, max_steps=8, ln=True),
    "widest_staged_actor": dict(env="acrobot", H=108, L=2, T=16, max_steps=4, ln=True),
    "first_unstaged_actor": dict(env="acrobot", H=109, L=2, T=16, max_steps=4, ln=True),
    "only_gumbel_given": dict(env="mountaincar", H=16, L=2, T=2, max_steps=5, given="gumbel", astd=0.5),
    "only_noise_given": dict(env="cartpole", H=16, L=2, T=2, max_steps=5, given="noise", astd=0.5),
}


def _lds_bytes(S, A, H, L, T, ln):
    rows = min(T, 16)
    pa = S * H + H + (L - 1) * (H * H + H) + (2 * H if ln and L >= 2 else 0) + A * H + A
    return 4 * (2 * rows * ((H + 3) & ~3) + (rows * (H | 1) if ln and L >= 2 else 0) + pa)


@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_edges_equal_the_composition(eng, orc, case):
    spec = EDGE_CASES[case]
    cfg, got = _case(eng, orc, seed=41, label=case, **spec)
    # the entry stages the actor where it fits next to the activation buffers in half a CU's LDS less 8 KiB
    lds = _lds_bytes(cfg.state_dim, cfg.action_dim, spec["H"], spec["L"], spec["T"], spec.get("ln", False))
    if case.startswith("streamed") or case.startswith("first_unstaged"):
        assert lds > 80 * 1024 - 8192
    if case.startswith("widest_staged"):
        assert lds <= 80 * 1024 - 8192


def test_done_in_the_first_step_beside_full_length_episodes(eng, orc):
    """CartPole from the angle threshold with a large angular velocity: the episode ends in its first step whatever the action and idles while
    its neighbours in the block run on; max_steps 7 ends the others by TimeLimit at the latest."""
    _, got = _case(eng, orc, "cartpole", 16, 2, 3, 7, first_step_done=(1, 0), seed=57, label="first_step_done")
    assert got["env_steps"][1, 0] == 1 and got["row_done"][1, 0, 0] == 1.0 and got["returns"][1, 0] == 1.0
    assert (got["row_reward"][1, 0, 1:] == SENTINEL).all() and (got["row_action"][1, 0, 1:] == SENTINEL).all()
    others = np.ones((3, 3), bool)
    others[1, 0] = False
    assert got["env_steps"][others].max() == 7 and got["env_steps"][others].min() > 1


# ---- 5. ties ----

@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
def test_ties_go_to_action_0(eng, orc, hard):
    """All-zero weights and biases, equal Gumbel values in a row, no noise: with the soft head every action vector has equal components and the
    env gets action 0; with the hard head y_soft ties, so the straight-through one-hot sits at index 0 too.  The episodes are the ones
    lenv_real_env_step gives under action 0."""
    ocfg, cfg = _cfgs(orc, **_kw("mountaincar", 8, 2, 2, 6, hard=hard))
    params, keys = _population(eng, cfg, 2, 3)
    params[:] = 0.0
    resets, obs0 = _resets(cfg, keys, OFFSETS[:2])
    gumbel = np.repeat(np.random.RandomState(2).standard_normal((2, 2, 6, 1)).astype(np.float32), 3, axis=3)
    noise = np.zeros((2, 2, 6, 3), np.float32)
    got = _run(cfg, params, keys, OFFSETS[:2], reset_states=resets, gumbel=gumbel, noise=noise)
    a = got["row_action"]
    assert (a != SENTINEL).all() and (a[..., 1] == a[..., 2]).all()
    assert (a[..., 0] > a[..., 1]).all() if hard else (a[..., 0] == a[..., 1]).all()
    exp = _compose(orc, ocfg, cfg, params, resets, obs0, gumbel, noise, (0, 0))
    _assert_equal(got, exp, "ties")
    # MountainCar under action 0 (push left) from the valley: the velocity falls in the first step
    assert (got["row_next_state"][:, :, 0, 1] < got["row_state"][:, :, 0, 1]).all()


# ---- 6. a run of the reference ----

def test_reference_run_re_laid_from_its_tapes(eng, orc, golden):
    """The CartPole chain fixture of test_td3_discrete.py: the oracle's tape-mode replay gives final_params, the learn calls and the tape
    positions; the closing test's reset rows and -- consumed episode after episode, CartPole paying 1 per step -- its Gumbel / noise rows are
    re-laid into [1, T, cap, A].  The entry's returns are the fixture's final returns at test_calc_score_vs_reference's tolerance for them
    (1e-9; test_hip_tape_mode_vs_reference_and_oracle holds the kernel to the oracle exactly)."""
    from learning_environments_amd import _lib
    g = golden("g8td_calc_score_cartpole_td3_discrete")
    cfgd, hp = json.loads(str(g["config_json"])), json.loads(str(g["hp_json"]))
    ocfg = orc.td3d_cfg_from_config(cfgd, rng_mode=1, hp=hp)
    tapes = {k: g["tape_" + k] for k in orc.TD3D_TAPE_KEYS}
    o = orc.td3d_chain(ocfg, g["theta"], g["agent_init"], tapes=orc.make_td3d_tapes(ocfg.action_dim, **tapes))
    assert o["rc"] == 0 and ocfg.test_mode == 0
    cfg = _lib.Td3dCfg()
    for f, _ in _lib.Td3dCfg._fields_:
        setattr(cfg, f, getattr(ocfg, f))
    T, cap, A = cfg.test_episodes, cfg.max_steps, cfg.action_dim
    want = np.asarray(g["reward_list_test"], np.float64)
    lengths = want.astype(np.int64)
    assert np.array_equal(lengths.astype(np.float64), want) and len(lengths) == T
    resets = np.asarray(tapes["test_reset"], np.float64).reshape(-1, 4)[o["episodes_run"] * T:o["episodes_run"] * T + T].reshape(1, T, 4)
    first = o["test_steps"] - int(lengths.sum())
    gum, nz = np.asarray(tapes["gumbel_test"], np.float32).reshape(-1, A), np.asarray(tapes["test_noise"], np.float32).reshape(-1, A)
    gumbel, noise = np.zeros((1, T, cap, A), np.float32), np.zeros((1, T, cap, A), np.float32)
    at = first
    for e in range(T):
        gumbel[0, e, :lengths[e]], noise[0, e, :lengths[e]] = gum[at:at + lengths[e]], nz[at:at + lengths[e]]
        at += int(lengths[e])
    assert at == o["test_steps"]
    params = np.asarray(o["final_params"], np.float32).reshape(1, -1)
    got = _run(cfg, params, np.array([1], np.uint64), learn_calls=[o["learn_steps"]], reset_states=resets, gumbel=gumbel, noise=noise)
    print("entry", got["returns"][0].tolist(), "fixture", want.tolist(), "oracle", np.asarray(o["final_test_returns"]).tolist())
    np.testing.assert_allclose(got["returns"][0], want, rtol=0, atol=1e-9)
    assert np.array_equal(got["returns"][0], np.asarray(o["final_test_returns"]))
    assert np.array_equal(got["env_steps"][0], lengths)


# ---- 7. test_discrete_actor_agents, histogram.collect ----

def _td3d_config(**agent_over):
    from learning_environments_amd import configs
    c = configs.cartpole_syn_env_td3_discrete(2, **agent_over)
    c["envs"]["CartPole-v0"].update(max_steps=12)
    return c


def test_test_discrete_actor_agents_returns_the_entrys_rows(eng, orc):
    """The triples of rollout.test_discrete_actor_agents: returns, lengths, and ReplayRows that concatenate to the rows of the entry (C-ABI call
    on the cfg the config builder gives, same keys, offsets and learn calls), episode after episode."""
    from learning_environments_amd.agents.rollout import ReplayRows, test_discrete_actor_agents
    from learning_environments_amd.config import td3d_cfg_from_config
    cfgd = _td3d_config(hidden_size=24, use_layer_norm=True, gumbel_softmax_hard=False, action_std=0.3)
    cfg = td3d_cfg_from_config(cfgd, test_episodes=4, max_steps=9)
    params, keys = _population(eng, cfg, 3, seed=77)
    lcs = [0, 40, 3000]
    triples = test_discrete_actor_agents(cfgd, params, keys, learn_calls=lcs, episode_offset=OFFSETS, test_episodes=4, max_steps=9)
    got = _run(cfg, params, keys, OFFSETS, learn_calls=lcs)
    S, A = cfg.state_dim, cfg.action_dim
    merged = ReplayRows(S, action_dim=A)
    for i, (reward_list, length_list, rows) in enumerate(triples):
        assert reward_list == got["returns"][i].tolist() and length_list == got["agent_steps"][i].tolist()
        assert rows.action_dim == A and rows.get_size() == sum(length_list)
        merged.merge_buffer(rows)
    filled = np.arange(got["row_reward"].shape[2])[None, None, :] < got["agent_steps"][:, :, None]
    want = (got["row_state"][filled], got["row_action"][filled], got["row_next_state"][filled], got["row_reward"][filled][:, None], got["row_done"][filled][:, None])
    for a, b in zip(merged.get_all(), want):
        assert a.dtype == torch.float32 and np.array_equal(a.numpy(), b)
    merged.make_one_hot_buffer()
    assert np.array_equal(merged.get_all()[1].numpy()[:, 0], want[1].argmax(axis=1).astype(np.float32))
    again = test_discrete_actor_agents(cfgd, params[1:2], keys[1:2], learn_calls=40, test_episodes=4, max_steps=9)      # agent 1 has offset 0
    assert again[0][0] == triples[1][0]


def test_histogram_collect_with_td3_discrete_vary(eng):
    """A fresh CartPole SE, three agents at the td3_discrete_vary_layer_norm_2 shape (4-128-128-2, tanh, LayerNorm, soft head, temperature 1,
    batch 128, policy_delay 2) with a few training episodes: collect's own assertion (test returns == the launch's final_returns) holds,
    and both merged buffers carry action indices."""
    from learning_environments_amd.envs.env_factory import EnvFactory
    from learning_environments_amd.experiments import histogram
    config = _td3d_config(train_episodes=4, test_episodes=3, init_episodes=1, batch_size=128, gamma=0.99, lr=5e-4, tau=0.01, policy_delay=2,
                          hidden_size=128, hidden_layer=2, action_std=0.1, policy_std=0.2, early_out_num=10, gumbel_softmax_temp=1.0,
                          gumbel_softmax_hard=False, use_layer_norm=True)
    config["envs"]["CartPole-v0"].update(max_steps=30, hidden_size=16)
    torch.manual_seed(3)
    fac = EnvFactory(config)
    virtual_env, real_env = fac.generate_virtual_env(), fac.generate_real_env()
    out = histogram.collect(virtual_env, real_env, config, "td3_discrete_vary", agents_num=3, seed=9)
    inner = histogram.collect.last["inner"]
    stats = inner.stats.cpu().numpy()
    assert (inner.cfg.hidden, inner.cfg.layers, inner.cfg.use_layer_norm, inner.cfg.test_mode) == (128, 2, 1, 1)
    assert (stats[:, 2] > 0).all()                        # the agents did learn before they were tested
    assert [tuple(t.shape)[1:] for t in out["train"]] == [(4,), (1,), (4,), (1,), (1,)]
    assert [tuple(t.shape)[1:] for t in out["test"]] == [(4,), (1,), (4,), (1,), (1,)]
    assert out["train"][0].shape[0] == int(stats[:, 1].sum()) > 0
    for part in ("train", "test"):
        assert set(out[part][1].reshape(-1).tolist()) <= {0.0, 1.0}, part
    n_test = sum(sum(t[1]) for t in histogram.collect.last["triples"])
    assert out["test"][0].shape[0] == n_test == out["virt_rewards"].shape[0] and out["virt_rewards_incorrect"] is not None
    assert len(out["rewards"]) == 3 and out["agentname"] == "td3_discrete_vary"


# ---- 8. the tabular entry ----

def _ql_run(cfg, q, tables):
    """lenv_ql_test_population through the C-ABI on sentinel-filled buffers"""
    from learning_environments_amd import _lib
    L = _lib.lib()
    n, T = q.shape[0], cfg.test_episodes
    cap = int(L.lenv_ql_test_rows_cap(C.byref(cfg)))
    assert cap == -(-cfg.max_steps // max(cfg.same_action_num, 1))
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device="cuda")
    f32 = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")
    out = dict(returns=torch.full((n, T), SENTINEL, dtype=torch.float64, device="cuda"), env_steps=i32(n, T), agent_steps=i32(n, T),
               row_state=i32(n, T, cap), row_action=i32(n, T, cap), row_next_state=i32(n, T, cap), row_reward=f32(n, T, cap), row_done=f32(n, T, cap))
    qd = dev(np.ascontiguousarray(q, np.float64).reshape(n, -1))
    ns, rw, dn = dev(tables["next_state"].astype(np.int32)), dev(tables["reward"].astype(np.float64)), dev(tables["done"].astype(np.uint8))
    rc = L.lenv_ql_test_population(C.byref(cfg), ptr(qd), ptr(ns), ptr(rw), ptr(dn), n, ptr(out["returns"]), ptr(out["env_steps"]), ptr(out["agent_steps"]),
                                   *[ptr(out[f]) for f in ROW_FIELDS], None)
    assert rc == 0
    torch.cuda.synchronize()
    return {name: v.cpu().numpy() for name, v in out.items()}


def _ql_walk(cfg, q, tables):
    """BaseAgent.test with select_test_action in numpy: fp32-cast argmax (the first maximum), the action same_action_num times or until done,
    the python-float reward sum rounded once, TimeLimit at max_steps env steps."""
    n, T = q.shape[0], cfg.test_episodes
    k_rep = max(cfg.same_action_num, 1)
    cap = -(-cfg.max_steps // k_rep)
    exp = dict(returns=np.zeros((n, T)), env_steps=np.zeros((n, T), np.int32), agent_steps=np.zeros((n, T), np.int32),
               row_state=np.full((n, T, cap), -7, np.int32), row_action=np.full((n, T, cap), -7, np.int32), row_next_state=np.full((n, T, cap), -7, np.int32),
               row_reward=np.full((n, T, cap), SENTINEL, np.float32), row_done=np.full((n, T, cap), SENTINEL, np.float32))
    for i in range(n):
        q32 = q[i].reshape(cfg.n_states, cfg.n_actions).astype(np.float32)
        for e in range(T):
            s, done, el, k, ret = cfg.start_state, False, 0, 0, np.float32(0.0)
            while el < cfg.max_steps and not done:
                a = int(np.argmax(q32[s]))
                s0, rsum = s, 0.0
                for _ in range(k_rep):
                    done = bool(tables["done"][s, a])
                    rsum += float(tables["reward"][s, a])
                    s = int(tables["next_state"][s, a])
                    el += 1
                    done = done or el >= cfg.max_steps
                    if done:
                        break
                r32 = np.float32(rsum)
                ret = np.float32(ret + r32)
                exp["row_state"][i, e, k], exp["row_action"][i, e, k], exp["row_next_state"][i, e, k] = s0, a, s
                exp["row_reward"][i, e, k], exp["row_done"][i, e, k] = r32, 1.0 if done else 0.0
                k += 1
            exp["returns"][i, e], exp["env_steps"][i, e], exp["agent_steps"][i, e] = float(ret), el, k
    return exp


def _cliff(orc, golden, agent, rtype, **agent_over):
    """(HIP cfg, tables) of a Cliff RewardEnv with the named tabular agent, 30 training episodes"""
    import gridworld_transfer_ref as gt
    from learning_environments_amd.config import ql_cfg_from_config
    cfgd, tables = gt.recorded_config(golden(gt.FIXTURES[0]))
    cfgd["agents"]["gtn"]["agent_name"] = agent
    sec = "sarsa" if agent.startswith("sarsa") else "ql"
    cfgd["agents"][sec] = dict(cfgd["agents"]["ql"], eps_init=0.3, eps_min=0.05, eps_decay=0.9, train_episodes=30, beta=0.1, **agent_over)
    cfgd["envs"]["Cliff"].update(reward_env_type=rtype, hidden_layer=1, solved_reward=-20)
    return ql_cfg_from_config(cfgd, tables), tables


@pytest.mark.parametrize("agent,rtype,over", [("ql", 2, dict()), ("sarsa", 1, dict(same_action_num=3, test_episodes=3)), ("ql_cb", 0, dict()),
                                              ("sarsa_cb", 6, dict(same_action_num=3))])
def test_tabular_returns_equal_the_rn_loops_final_returns(eng, orc, golden, agent, rtype, over):
    """5 chains of lenv_ql_rn_inner_loop on Cliff (four actions: the fused test's fast path with same_action_num 1, its repeat form with 3): the
    entry on the launch's q_table rows gives final_returns, and the env steps of a launch that only tests."""
    cfg, tables = _cliff(orc, golden, agent, rtype, **over)
    assert cfg.n_actions == 4 and max(cfg.same_action_num, 1) == over.get("same_action_num", 1)
    chains = 5
    il = eng.QlInnerLoop(cfg, chains, tables)
    P = il.p_theta
    rng = np.random.RandomState(21 + rtype)
    theta, eps = (rng.randn(P) * 0.3).astype(np.float32), (rng.randn(2, P) * 0.1).astype(np.float32)
    worker, sign = np.array([0, 0, 1, 1, 0], np.int32), np.array([0, 1, -1, 1, -1], np.float32)
    keys = dev(rng.randint(1, 2 ** 62, size=chains).astype(np.uint64).view(np.int64))
    il.run(dev(theta), dev(eps), dev(worker), dev(sign), rng_keys=keys)
    torch.cuda.synchronize()
    assert il.status.cpu().tolist() == [0] * chains
    got = eng.ql_test_population(cfg, il.q_table, tables, want_rows=False)
    assert sorted(got) == ["agent_steps", "env_steps", "returns"]
    ret, fin = got["returns"].cpu().numpy(), il.final_returns.cpu().numpy()
    assert np.array_equal(ret, fin), (agent, ret, fin)
    assert np.abs(il.q_table.cpu().numpy()).max() > 0
    # and all of it against the numpy walk
    q = il.q_table.cpu().numpy()
    full, exp = _ql_run(cfg, q, tables), _ql_walk(cfg, q, tables)
    for name in exp:
        assert np.array_equal(full[name], exp[name]), (agent, name)
    assert np.array_equal(full["returns"], fin)


def test_tabular_returns_equal_the_se_loops_final_returns(eng, golden):
    """12 chains of one lenv_ql_se_inner_loop launch (SARSA on a HoleRoom VirtualEnv; its tests walk the real grid)."""
    import ql_se_ref
    from learning_environments_amd import _lib
    g = golden("g15b_ql_se_holeroom_sarsa")
    cfg, tables, _ = ql_se_ref.fixture_inputs(g, rng_mode=_lib.RNG_COUNTER, agent_kind=1, count_based=0)
    eps, worker, sign, _ = ql_se_ref.population(g["theta"], 4, 0.01, 7)
    keys = np.arange(1000, 1012, dtype=np.uint64) * np.uint64(0x9e3779b97f4a7c15)
    inner = eng.QlSeInnerLoop(cfg, 12, tables, want_episode_stats=True)
    inner.run(dev(np.asarray(g["theta"], np.float32)), dev(eps), dev(worker), dev(sign), rng_keys=dev(keys.view(np.int64)))
    torch.cuda.synchronize()
    assert inner.status.cpu().tolist() == [0] * 12
    got = eng.ql_test_population(cfg, inner.q_table, tables)
    assert np.array_equal(got["returns"].cpu().numpy(), inner.final_returns.cpu().numpy())
    assert got["row_state"].dtype == torch.int32 and tuple(got["row_state"].shape) == (12, cfg.test_episodes, -(-cfg.max_steps // max(cfg.same_action_num, 1)))


@pytest.mark.parametrize("grid,san,T", [("HoleRoom", 1, 2), ("HoleRoom", 3, 1), ("EmptyRoom33", 1, 3), ("EmptyRoom33", 2, 1)])
def test_tabular_rows_equal_a_numpy_walk_on_random_tables(eng, grid, san, T):
    """6 Q-tables drawn at random.  Table 0 never terminates (it keeps walking into the wall behind the start cell: rows reach cap, row_done
    is 1 only at the max_steps-th env step); table 1 walks from HoleRoom's start cell straight into the hole two cells on (inside one agent
    step when the action is repeated), and, started next to the hole, steps into it at once; table 2 is all ties, table 3 has a tie that
    only the fp32 cast makes."""
    from learning_environments_amd import _lib
    from learning_environments_amd.envs.gridworld import transition_tables
    tables = transition_tables(grid)
    N, A, start = tables["n_states"], tables["n_actions"], tables["start_state"]
    cfg = _lib.QlCfg(n_states=N, n_actions=A, start_state=start, max_steps=11, test_episodes=T, same_action_num=san)
    rng = np.random.RandomState(N + san)
    q = rng.standard_normal((6, N, A))
    q[2, :, :] = np.float32(0.3)                          # ties everywhere: action 0
    q[3, start] = [1.0 + 1e-12, 1.0] + [0.0] * (A - 2)    # equal after the fp32 cast: the first maximum
    stay = [a for a in range(A) if tables["next_state"][start, a] == start and not tables["done"][start, a]]
    assert stay                                           # both grids start in a corner
    q[0, start] = -1.0
    q[0, start, stay[0]] = 1.0
    hole = grid == "HoleRoom"
    if hole:                                              # 0 -right-> 1 -right-> the hole at 2
        assert tables["next_state"][0, 0] == 1 and tables["done"][1, 0] and tables["reward"][1, 0] == -1.0 and start == 0
        q[1, 0], q[1, 1] = [1.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]
    got, exp = _ql_run(cfg, q, tables), _ql_walk(cfg, q, tables)
    for name in exp:
        assert np.array_equal(got[name], exp[name]), (grid, name)
    cap = got["row_done"].shape[2]
    assert (got["env_steps"][0] == 11).all() and (got["agent_steps"][0] == cap).all()
    assert (got["row_done"][0, :, :cap - 1] == 0.0).all() and (got["row_done"][0, :, cap - 1] == 1.0).all()
    assert (got["row_state"][0] == start).all() and (got["row_next_state"][0] == start).all()
    assert got["row_action"][3, 0, 0] == 0
    assert (got["row_action"][2][got["row_action"][2] != -7] == 0).all()
    if hole:
        assert (got["env_steps"][1] == 2).all() and (got["agent_steps"][1] == (1 if san == 3 else 2)).all()
        assert (got["returns"][1] == float(np.float32(-1.01) if san == 3 else np.float32(np.float32(-0.01) + np.float32(-1.0)))).all()
        cfg.start_state = 1                               # next to the hole: done in the first env step
        got, exp = _ql_run(cfg, q, tables), _ql_walk(cfg, q, tables)
        for name in exp:
            assert np.array_equal(got[name], exp[name]), (grid, "start 1", name)
        assert (got["env_steps"][1] == 1).all() and (got["row_done"][1, :, 0] == 1.0).all() and (got["row_reward"][1, :, 0] == -1.0).all()
        assert (got["row_reward"][1, :, 1:] == SENTINEL).all() and (got["row_state"][1, :, 1:] == -7).all()


def test_tabular_return_on_a_reference_q_table(eng, golden):
    """The g16b fixture (QL on the real Cliff, 500 episodes, test_episodes 1): the reference's last per-episode test ran on its final fp64
    Q-table, so the entry's return on that table is the last entry of its reward_list."""
    import gridworld_transfer_ref as gt
    from learning_environments_amd.config import ql_cfg_from_config
    g = golden("g16b_gridworld_transfer_vary_hp_mode0")
    cfgd, tables = gt.recorded_config(g)
    cfg = ql_cfg_from_config(cfgd, tables)
    assert cfg.test_episodes == 1
    q = np.stack([gt.agent_slices(g, i)["q_table"] for i in range(gt.AGENTS)]).astype(np.float64)
    got = _ql_run(cfg, q, tables)
    for i in range(gt.AGENTS):
        a = gt.agent_slices(g, i)
        assert len(a["reward_list"]) == 500
        assert got["returns"][i, 0] == float(a["reward_list"][-1]), (i, got["returns"][i, 0], a["reward_list"][-1])


def test_gridworld_heatmap_states_are_the_rows_of_test_tabular_agents(eng, golden):
    """gridworld_heatmap.train_test_agents on a fresh Cliff reward net, 3 agents, 20 training episodes: the states lists equal those rebuilt
    from test_tabular_agents' rows on the launch's Q-tables, under both BREAK settings."""
    import gridworld_transfer_ref as gt
    from learning_environments_amd.agents.rollout import test_tabular_agents
    from learning_environments_amd.envs.env_factory import EnvFactory
    from learning_environments_amd.experiments import gridworld_heatmap as gh
    config = json.loads(str(golden(gt.FIXTURES[0])["config_json"]))
    config["agents"].pop("sarsa", None)
    config["agents"]["ql"].update(eps_init=0.1, eps_min=0.1, eps_decay=0.0, alpha=1.0, gamma=0.8)
    for break_ in ("end", "solved"):
        config["envs"]["Cliff"]["solved_reward"] = gh.SOLVED_REWARD[break_]
        torch.manual_seed(5)
        fac = EnvFactory(config)
        env, real_env = fac.generate_reward_env(), fac.generate_real_env()
        states = gh.train_test_agents(env, real_env, config, agents_num=3, seed=4, break_=break_, settings=dict(train_episodes=20))
        assert config["agents"]["sarsa"] == dict(gh.sarsa_settings(config), train_episodes=20)       # written in place
        last = gh.train_test_agents.last
        inner = last["inner"]
        assert inner.chains == 3 and (inner.cfg.agent_kind, inner.cfg.count_based, inner.cfg.test_episodes) == (1, 0, 1)
        triples = test_tabular_agents(last["config"], inner.q_table, real_env.env.tables)
        want = []
        for reward, (rets, lens, rows) in zip(last["rewards"], triples):
            s, a, s2, r, d = rows.get_all()
            assert rows.state_dim == 1 and s.shape[0] == lens[0] and d[-1, 0] == 1.0 and s[0, 0] == 36
            if break_ == "end" or len(reward) != 20:
                want.append([int(v) for v in s[:, 0].tolist()] + [int(s2[-1, 0])])
        assert states == want
        if break_ == "end":
            assert len(states) == 3 and all(len(r) == 20 for r in last["rewards"])
