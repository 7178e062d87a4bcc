"""lenv_se_step_population_vec: the population-batched VirtualEnv step for action VECTORS (the continuous-action SEs) with the
`same_action_num` repeat inside the launch -- host checks without a device; on the GPU the reference's own SE rows, a perturbed population
against the oracle bit for bit on both kernels (weights resident in LDS / streamed through it) and across the switch between them, the
index entry on one-hot rows, and EnvWrapper.step_population over continuous and discrete action spaces."""
import ctypes as C
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ACTS = ["identity", "relu", "leakyrelu", "tanh", "prelu"]
FIXTURES = ["g8p_calc_score_pendulum_td3_virtual_env", "g8pf_calc_score_pendulum_td3_virtual_env_fullshape",
            "g8c_calc_score_cmc_td3_virtual_env", "g8cf_calc_score_cmc_td3_virtual_env_fullshape",
            "g8ts_calc_score_cheetah_td3_virtual_env", "g8hf_calc_score_cheetah_td3_virtual_env_fullshape"]


def _descs(mod, S, A, H, L, act, ln=False):
    """The three SE nets as `mod`'s lenv_mlp_desc (mod = the engine or the oracle)."""
    return tuple(mod.mlp_desc(S + A, H, L, o, act, use_layer_norm=ln) for o in (S, 1, 1))


def _path(S, A, H, L, n=1, ln=False):
    from learning_environments_amd import _lib, engine
    d = _descs(engine, S, A, H, L, "relu", ln)
    return _lib.lib().lenv_se_step_vec_path(C.byref(d[0]), C.byref(d[1]), C.byref(d[2]), n)


def test_exports_path_query_and_argument_checks_without_a_device():
    from learning_environments_amd import _lib, engine
    L = _lib.lib()
    for name in ("lenv_se_step_population_vec", "lenv_se_step_vec_path"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.lenv_abi_version() == 7
    d = _descs(engine, 3, 1, 20, 2, "relu")
    by = [C.byref(x) for x in d]
    # argument validation happens before any device work
    assert L.lenv_se_step_population_vec(*by, None, None, None, None, 1, 1, 1, None, None, None, None, None, None) == -1
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert L.lenv_se_step_population_vec(*by, p, None, None, None, 1, 1, 0, p, p, p, p, p, None) == -1           # repeat < 1
    assert L.lenv_se_step_population_vec(*by, p, p, None, None, 1, 1, 1, p, p, p, p, p, None) == -1              # eps without worker / sign
    assert L.lenv_se_step_population_vec(*by, p, None, None, None, 0, 1, 1, p, p, p, p, p, None) == 0            # no chains: nothing to launch
    assert _path(3, 1, 20, 2) == 0                       # Pendulum 4-20-20-x: 1 665 floats stay in LDS
    assert _path(17, 6, 128, 3) == 1                     # the published HalfCheetah SE: 110 739 floats = 443 KB are streamed
    assert _path(17, 6, 128, 3, n=256) == 1
    assert L.lenv_se_step_vec_path(by[0], by[1], by[2], 0) == -1 and L.lenv_se_step_vec_path(None, by[1], by[2], 1) == -1
    # every shape inside hidden <= 256, layers 1..3, S + A <= 256 has a kernel; beyond them the entry refuses
    for S, A, H, Ln in ((255, 1, 256, 3), (1, 255, 256, 3), (254, 2, 1, 1), (1, 1, 1, 1), (200, 56, 60, 1), (128, 128, 256, 1)):
        for n in (1, 9):
            assert _path(S, A, H, Ln, n) in (0, 1) and _path(S, A, H, Ln, n, ln=True) in (0, 1), (S, A, H, Ln, n)
    assert _path(17, 6, 257, 2) == -2 and _path(17, 6, 128, 4) == -2 and _path(200, 57, 64, 2) == -2
    bad = _descs(engine, 3, 1, 20, 2, "relu")
    bad[1].hidden = 21
    assert L.lenv_se_step_vec_path(C.byref(bad[0]), C.byref(bad[1]), C.byref(bad[2]), 1) == -1
    bb = [C.byref(x) for x in bad]
    assert L.lenv_se_step_population_vec(*bb, p, None, None, None, 1, 1, 1, p, p, p, p, p, None) == -1
    # like lenv_se_step_population, a launch without chains is done before the descriptors are looked at
    assert L.lenv_se_step_population_vec(*bb, p, None, None, None, 0, 1, 1, p, p, p, p, p, None) == 0
    assert L.lenv_se_step_population(*bb, p, None, None, None, 0, 1, p, p, p, p, p, None) == 0
    assert L.lenv_se_step_population_vec(*by, p, None, None, None, 2 ** 31, 1, 1, p, p, p, p, p, None) == -2      # more chains than a grid has


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------

@pytest.fixture(scope="module")
def eng():
    from learning_environments_amd import engine
    engine.require_device()
    return engine


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _oracle_step(orc, odescs, w, state, action, repeat):
    """EnvWrapper.step's virtual branch on one weight vector: `repeat` times three oracle.mlp_forward calls on cat(action, state), the
    next state fed back, the rewards summed left to right in fp32."""
    sizes = [orc.mlp_num_params(d) for d in odescs]
    assert w.size == sum(sizes)
    parts = np.split(w, np.cumsum(sizes)[:-1])
    s, rsum = state, None
    for _ in range(repeat):
        x = np.ascontiguousarray(np.concatenate([action, s], axis=1), dtype=np.float32)
        s, r, d = [orc.mlp_forward(dsc, p, x) for dsc, p in zip(odescs, parts)]
        rsum = r[:, 0] if rsum is None else (rsum + r[:, 0]).astype(np.float32)
    return s, rsum, d[:, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_rows_of_the_reference_on_continuous_action_ses(eng, orc, golden, name):
    """SE steps the reference itself took with continuous actions (TD3 on the Pendulum / MountainCarContinuous / HalfCheetah VirtualEnvs;
    same_action_num 2 on MountainCarContinuous), one chain, all rows in one launch: within the trace tolerance 1e-5 of the reference,
    and the oracle composition's bits.  The HalfCheetah full shape 23-128-128-128-x is the streaming kernel."""
    g = golden(name)
    cfg = json.loads(str(g["config_json"]))
    env = cfg["envs"][cfg["env_name"]]
    S, A = g["tr_state"].shape[1], g["tr_action"].shape[1]
    H, L, act = int(env["hidden_size"]), int(env["hidden_layer"]), env["activation_fn"]
    k = int(cfg["agents"]["td3"]["same_action_num"])
    assert _path(S, A, H, L, g["tr_state"].shape[0]) == (1 if "cheetah" in name and "fullshape" in name else 0)
    ns, r, d = eng.se_step_population_vec(_descs(eng, S, A, H, L, act), dev(g["theta"]), None, None, None,
                                          dev(g["tr_state"][None]), dev(g["tr_action"][None]), repeat=k)
    ns, r, d = ns[0].cpu().numpy(), r[0].cpu().numpy(), d[0].cpu().numpy()
    ons, orr, od = _oracle_step(orc, _descs(orc, S, A, H, L, act), g["theta"], g["tr_state"], g["tr_action"], k)
    print(name, "k", k, "max |next_state - ref|", np.abs(ns - g["tr_next_state"]).max(), "max |reward - ref|", np.abs(r - g["tr_reward"]).max())
    np.testing.assert_allclose(ns, g["tr_next_state"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(r, g["tr_reward"], rtol=0, atol=1e-5)
    assert np.array_equal(ns, ons) and np.array_equal(r, orr) and np.array_equal(d, od)


def _largest_resident_hidden(S, A, L, ln):
    H = max(h for h in range(1, 257) if _path(S, A, h, L, 1, ln) == 0)
    assert _path(S, A, H + 1, L, 1, ln) == 1
    return H


def _population_case(eng, orc, S, A, H, L, act, ln, seed, rows=(1, 5, 70)):
    """7 chains over 3 noise rows, sign in {-1, 0, +1} (theta +- eps in numpy fp32 is then exactly the kernel's fma)."""
    rng = np.random.RandomState(seed)
    hd, od = _descs(eng, S, A, H, L, act, ln), _descs(orc, S, A, H, L, act, ln)
    P = sum(orc.mlp_num_params(d) for d in od)
    theta = (rng.randn(P) * 0.08).astype(np.float32)
    eps = (rng.randn(3, P) * 0.02).astype(np.float32)
    worker = np.array([0, 0, 0, 1, 1, 2, 2], np.int32)
    sign = np.array([0, 1, -1, 1, -1, -1, 1], np.float32)
    w = [(theta + sign[c] * eps[worker[c]]).astype(np.float32) for c in range(7)]
    t_theta, t_eps, t_worker, t_sign = dev(theta), dev(eps), dev(worker), dev(sign)
    for n in rows:
        st = rng.randn(7, n, S).astype(np.float32)
        ac = rng.uniform(-2, 2, (7, n, A)).astype(np.float32)
        for repeat in (1, 3):
            ns, r, d = eng.se_step_population_vec(hd, t_theta, t_eps, t_worker, t_sign, dev(st), dev(ac), repeat=repeat)
            ns, r, d = ns.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy()
            for c in range(7):
                ons, orr, odn = _oracle_step(orc, od, w[c], st[c], ac[c], repeat)
                assert np.isfinite(ons).all()
                tag = (S, A, H, L, act, ln, n, repeat, c)
                assert np.array_equal(ns[c], ons), tag
                assert np.array_equal(r[c], orr) and np.array_equal(d[c], odn), tag


SHAPES = {"pendulum": (3, 1, 20, 2), "cmc_full": (2, 1, 96, 2), "cheetah_full": (17, 6, 128, 3), "last_resident": (17, 6, 0, 2),
          "first_streaming": (17, 6, 1, 2)}


@pytest.mark.gpu
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_perturbed_population_equals_the_oracle_bit_for_bit(eng, orc, shape, ln):
    """Both kernels and the pair of widths on either side of the switch between them (the largest H whose 17+6 -> H x 2 SE still stays
    in LDS, and H + 1), n_per_chain 1 / 5 / 70 (a partial register tile; streaming: 70 rows = two row blocks of 32 and one of 6, resident: nine
    blocks of 8), repeat 1 / 3, with and without the nets' LayerNorm."""
    S, A, H, L = SHAPES[shape]
    if shape in ("last_resident", "first_streaming"):
        H += _largest_resident_hidden(S, A, L, ln)
    assert _path(S, A, H, L, 70, ln) == (1 if shape in ("cheetah_full", "first_streaming") else 0)
    _population_case(eng, orc, S, A, H, L, "leakyrelu", ln, seed=len(shape) + 7 * ln)


@pytest.mark.gpu
@pytest.mark.parametrize("S,A,H,L", [(17, 6, 128, 3), (5, 2, 256, 2)])
def test_streaming_kernel_other_row_blocks_and_panels(eng, orc, S, A, H, L):
    """What the issue's rows do not reach in the streaming kernel: 12 rows = one row block of two register tiles, and the widest nets,
    whose panels are 24 columns wide (256 inputs = ten panels and one of 16 columns)."""
    assert _path(S, A, H, L, 12) == 1
    _population_case(eng, orc, S, A, H, L, "relu", True, seed=H, rows=(12,))


@pytest.mark.gpu
@pytest.mark.parametrize("act", ACTS)
def test_every_activation_at_the_smallest_shape(eng, orc, act):
    _population_case(eng, orc, 3, 1, 20, 2, act, False, seed=ACTS.index(act))


@pytest.mark.gpu
@pytest.mark.parametrize("S,A,H,L,ln", [(4, 2, 64, 1, False), (6, 3, 33, 3, True)])
def test_one_hot_rows_equal_the_index_entry(eng, S, A, H, L, ln):
    """Where lenv_se_step_population takes the shape, one-hot float rows through the new entry give its bits -- with a general sign,
    so that the perturbation is an fma that numpy cannot restate."""
    rng = np.random.RandomState(11)
    hd = _descs(eng, S, A, H, L, "tanh", ln)
    P = sum(eng.mlp_num_params(d) for d in hd)
    theta, eps = dev((rng.randn(P) * 0.1).astype(np.float32)), dev((rng.randn(2, P) * 0.05).astype(np.float32))
    worker, sign = dev(np.array([0, 1, 1, 0, 1], np.int32)), dev(np.array([0.37, -1.61, 0.37, 2.5e-3, 1.0], np.float32))
    st = dev(rng.randn(5, 9, S).astype(np.float32))
    idx = rng.randint(0, A, (5, 9)).astype(np.int32)
    want = eng.se_step_population(hd, theta, eps, worker, sign, st, dev(idx))
    got = eng.se_step_population_vec(hd, theta, eps, worker, sign, st, dev(np.eye(A, dtype=np.float32)[idx]))
    for g_, w_ in zip(got, want):
        assert g_.shape == w_.shape and torch.equal(g_, w_)


def _small_venv(cfg, env_name, **env_over):
    from learning_environments_amd.envs.env_factory import EnvFactory
    cfg["device"] = "cuda"
    cfg["envs"][env_name].update(env_over)
    return EnvFactory(cfg).generate_virtual_env()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["pendulum", "cmc"])
def test_step_population_on_continuous_action_virtual_envs(eng, which):
    from learning_environments_amd import configs
    torch.manual_seed(5)
    if which == "pendulum":
        venv = _small_venv(configs.pendulum_syn_env_td3(), "Pendulum-v0", hidden_size=24)
    else:
        venv = _small_venv(configs.cmc_syn_env_td3(), "MountainCarContinuous-v0", hidden_size=20)
    assert venv.is_virtual_env() and not venv.has_discrete_action_space()
    S, A = venv.get_state_dim(), venv.get_action_dim()
    theta = venv.env.flat_params()
    d_ = theta.device
    states, actions = (torch.randn(6, S) * 0.5).to(d_), (torch.rand(6, A) * 2 - 1).to(d_)
    # eps None: VirtualEnv.step on the same rows
    ns, r, d = venv.step_population(actions, states)
    wns, wr, wd = venv.env.step(actions, state=states)
    assert tuple(ns.shape) == (6, S) and tuple(r.shape) == (6,) and ns.is_cuda
    assert torch.equal(ns, wns) and torch.equal(r, wr[:, 0]) and torch.equal(d, wd[:, 0])
    # repeat 2: EnvWrapper.step with same_action_num 2, row by row
    ns2, r2, d2 = venv.step_population(actions, states, repeat=2)
    venv.set_agent_params(same_action_num=2, gamma=0.99)
    for i in range(6):
        sns, sr, sd = venv.step(actions[i], state=states[i])
        assert torch.equal(ns2[i].cpu(), sns) and torch.equal(r2[i].cpu().reshape(1), sr) and torch.equal(d2[i].cpu().reshape(1), sd)
    # a perturbed population is the engine call on the env's own descriptors and parameters
    eps = (0.05 * torch.randn(2, theta.numel())).to(d_)
    worker = torch.tensor([0, 1, 1, 0, 0, 1], dtype=torch.int32, device=d_)
    sign = torch.tensor([1.0, -1.0, 0.0, 0.37, -1.0, 1.0], device=d_)
    got = venv.step_population(actions, states, eps, worker, sign, repeat=2)
    want = eng.se_step_population_vec(venv.env.descs(), theta, eps, worker, sign, states, actions, repeat=2)
    assert all(torch.equal(g_, w_) for g_, w_ in zip(got, want))
    assert not torch.equal(got[0], ns2)


@pytest.mark.gpu
def test_step_population_repeats_on_a_discrete_action_virtual_env(eng):
    from learning_environments_amd import configs
    torch.manual_seed(6)
    venv = _small_venv(configs.cartpole_syn_env_ddqn(), "CartPole-v0", hidden_size=32)
    theta = venv.env.flat_params()
    d_ = theta.device
    states = (torch.randn(5, 4) * 0.1).to(d_)
    actions = torch.tensor([0, 1, 1, 0, 1], dtype=torch.int32, device=d_)
    eps = (0.05 * torch.randn(2, theta.numel())).to(d_)
    worker = torch.tensor([0, 1, 1, 0, 0], dtype=torch.int32, device=d_)
    sign = torch.tensor([1.0, -1.0, 0.0, 0.37, -1.0], device=d_)
    ns, r, d = venv.step_population(actions, states, eps, worker, sign, repeat=3)
    s, rsum = states, None
    for _ in range(3):
        s, r1, d1 = eng.se_step_population(venv.env.descs(), theta, eps, worker, sign, s.contiguous(), actions)
        rsum = r1 if rsum is None else rsum + r1
    assert torch.equal(ns, s) and torch.equal(r, rsum) and torch.equal(d, d1)
    # repeat 1 stays the index entry
    one = venv.step_population(actions, states, eps, worker, sign)
    want = eng.se_step_population(venv.env.descs(), theta, eps, worker, sign, states, actions)
    assert all(torch.equal(g_, w_) for g_, w_ in zip(one, want))
