"""PPO inner agent, CPU side: the restatement (tests/ppo_ref.c) against fixtures recorded from the reference's own
PPO.train(env=reward_env, test_env=real_env) + agent.test(real_env) with every draw taped (tools/gen_golden_ppo.py), and the host logic
that needs no device: the cfg of the two transfer scripts, the rows of a learn call, parameter counts, workspace queries, refusals, struct sizes."""
import copy
import ctypes as C
import json

import numpy as np
import pytest

import ppo_ref
from learning_environments_amd import _lib
from learning_environments_amd.config import ppo_cfg_from_config, ppo_layer_dims, ppo_rows

FIXTURES = ["g14p_ppo_pendulum_type2", "g14c_ppo_cmc_type5_k5", "g14h_ppo_cheetah_type0", "g14s_ppo_pendulum_std_floor",
            "g14f_ppo_pendulum_std_forward_floor"]
# |restatement - reference| over the parameters after every learn call: the worst value measured over the five fixtures is 1.67e-6
# (g14f, the fifth call: full-batch sums over the rows in torch's order against the row-ascending chains); twice that is allowed
PARAM_ATOL = 3.4e-6


def _run(golden, name, **over):
    g = golden(name)
    cfg = ppo_cfg_from_config(json.loads(str(g["config_json"])), rng_mode=_lib.RNG_TAPE, **over)
    tapes = dict(act_noise=g["tape_act_noise"], test_noise=g["tape_test_noise"], train_reset=g["tape_train_reset"], test_reset=g["tape_test_reset"])
    out = ppo_ref.chain(cfg, g["theta"], g["agent_init"], tapes=tapes, trace_cap=g["tr_reward"].size + 4, learn_cap=g["learn_step"].size + 2)
    return g, cfg, out


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_against_the_reference(golden, name):
    g, cfg, out = _run(golden, name)
    assert out["rc"] == 0
    tr, n = out["trace"], g["tr_reward"].size
    assert tr["reward"].size == n
    # every recorded return below 128 in magnitude (fp32 spacing <= 7.7e-6), so that 1e-4 on the test means is a meaningful bound
    assert max(np.abs(g["reward_list_train"]).max(), np.abs(g["reward_list_test"]).max()) < 128.0
    print(name, "action %.3g next_state %.3g reward %.3g" % (np.abs(tr["action"] - g["tr_action"]).max(), np.abs(tr["next_state"] - g["tr_next_state"]).max(),
                                                           np.abs(tr["reward"] - g["tr_reward"]).max()))
    np.testing.assert_allclose(tr["state"], g["tr_state"], rtol=0, atol=5e-5)
    np.testing.assert_allclose(tr["action"], g["tr_action"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(tr["next_state"], g["tr_next_state"], rtol=0, atol=5e-5)
    np.testing.assert_allclose(tr["reward"], g["tr_reward"], rtol=0, atol=5e-5)
    assert np.array_equal(tr["done"], g["tr_done"])
    assert np.array_equal(out["episode_len"], g["episode_length_train"])
    # the step at which each learn call fired: exact; at least two calls, one of them in the middle of an episode, rows after the last
    assert np.array_equal(out["learn_step"], g["learn_step"]) and out["learn_calls"] == g["learn_step"].size >= 2
    agent_steps = -(-cfg.max_steps // max(1, cfg.same_action_num))
    assert any(int(s) % agent_steps != 0 for s in g["learn_step"])
    assert g["learn_step"][-1] < n
    dev = np.abs(out["learn_params"] - g["learn_params"]).max(axis=1)
    print(name, "parameters after each learn call: max |restatement - reference| =", dev)
    np.testing.assert_allclose(out["learn_params"], g["learn_params"], rtol=0, atol=PARAM_ATOL)
    np.testing.assert_allclose(out["final_params"], g["final_params"], rtol=0, atol=PARAM_ATOL)
    np.testing.assert_allclose(out["episode_test_mean"], g["reward_list_train"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(out["final_returns"], g["reward_list_test"], rtol=0, atol=1e-4)
    assert abs(out["score"] - float(g["score"])) <= 1e-4


def test_fixtures_cover_what_they_are_for(golden):
    g = golden("g14p_ppo_pendulum_type2")
    c = json.loads(str(g["config_json"]))
    assert c["envs"]["Pendulum-v0"]["reward_env_type"] == 2 and c["agents"]["ppo"]["ppo_epochs"] >= 3
    g = golden("g14c_ppo_cmc_type5_k5")
    c = json.loads(str(g["config_json"]))
    assert c["agents"]["ppo"]["same_action_num"] == 5 and c["envs"]["MountainCarContinuous-v0"]["reward_env_type"] in (1, 5, 6)
    g = golden("g14h_ppo_cheetah_type0")
    c = json.loads(str(g["config_json"]))
    assert c["envs"]["HalfCheetah-v3"]["reward_env_type"] == 0 and g["tr_action"].shape[1] == 6
    # the std-floor fixtures: action_std as the epochs' log-probabilities saw it.  g14s: under evaluate's floor of 0.01 between epochs of one
    # call; g14f: under forward's floor of 0.001 after a call, seen like that by the next call's first epoch
    # Both keep a non-zero ent_coef, so the entropy's share of the action_std gradient in an epoch whose clamp fires is the reference's too.
    gs = golden("g14s_ppo_pendulum_std_floor")
    s = gs["std_seen"].reshape(-1)
    assert s[0] > 0.01 and (s[1:5] < 0.01).all() and json.loads(str(gs["config_json"]))["agents"]["ppo"]["ent_coef"] > 0
    f = golden("g14f_ppo_pendulum_std_forward_floor")
    assert f["std_seen"].reshape(-1)[1] < 0.001 and f["learn_params"][0, 0] < 0.001 and json.loads(str(f["config_json"]))["agents"]["ppo"]["ent_coef"] > 0


def test_expf_error_over_the_ratio_arguments(golden):
    """The project's deterministic expf was only used for arguments <= 0; the ratio exp(logp - old_logp) takes both signs.  Over [-20, 20]
    (clipping makes anything beyond +-0.2 irrelevant to the gradient) its relative error against libm's exp in fp64 stays within 2 ulp."""
    from oracle import oracle as orc
    L = orc.lib()
    L.orc_expf.restype, L.orc_expf.argtypes = C.c_float, [C.c_float]
    xs = np.concatenate([np.linspace(-20, 20, 4001), np.linspace(-0.5, 0.5, 4001)]).astype(np.float32)
    got = np.array([L.orc_expf(float(x)) for x in xs], np.float64)
    rel = np.abs(got - np.exp(xs.astype(np.float64))) / np.exp(xs.astype(np.float64))
    print("expf: max relative error %.3g" % rel.max())
    assert rel.max() <= 2 * 2.0 ** -23


def _script_config(env_name, ppo, max_steps):
    """A RewardEnv config with the `ppo` section of a transfer script's "settings for comparability" block."""
    from learning_environments_amd.experiments.transfer_algo import base_config
    cfg = base_config(env_name)
    cfg["agents"]["ppo"] = dict(ppo)
    cfg["envs"][env_name]["max_steps"] = max_steps
    return cfg


def test_cfg_rows_and_queries_of_the_two_scripts():
    from learning_environments_amd.experiments.transfer_algo import PPO_SETTINGS
    L = _lib.lib()
    for env_name, max_steps, rows, dims in (("MountainCarContinuous-v0", 999, 1999, (2, 1)), ("HalfCheetah-v3", 1000, 1001, (17, 6))):
        cfg = ppo_cfg_from_config(_script_config(env_name, PPO_SETTINGS[env_name], max_steps))
        S, A = dims
        assert (cfg.state_dim, cfg.action_dim) == dims and cfg.max_steps == max_steps
        assert ppo_rows(cfg) == rows == ppo_ref.rows(cfg) == L.lenv_ppo_rows(C.byref(cfg))
        H = cfg.hidden
        net = lambda out: S * H + H + (cfg.layers - 1) * (H * H + H) + out * H + out      # noqa: E731
        pa, pc = C.c_int64(), C.c_int64()
        P = L.lenv_ppo_num_params(C.byref(cfg), C.byref(pa), C.byref(pc))
        assert (P, pa.value, pc.value) == (A + net(A) + net(1), net(A), net(1)) and P == ppo_ref.num_params(cfg)
        assert sum(i * o + o for i, o in ppo_layer_dims(cfg)) == P - A
        one, many = L.lenv_ppo_rn_workspace_bytes(C.byref(cfg), 1), L.lenv_ppo_rn_workspace_bytes(C.byref(cfg), 48)
        assert one > 0 and many - 256 == 48 * (one - 256)
        # at least: four parameter-sized arrays, the rows, four activation matrices and two gradient matrices of rows x hidden
        assert one >= 4 * (4 * P + rows * (S + A + 2) + 6 * rows * H)
    cmc = ppo_cfg_from_config(_script_config("MountainCarContinuous-v0", PPO_SETTINGS["MountainCarContinuous-v0"], 999))
    assert (cmc.ppo_epochs, cmc.same_action_num, cmc.hidden, cmc.layers, cmc.act, cmc.test_episodes) == (80, 5, 64, 2, _lib.ACT["relu"], 1)
    assert (cmc.lr, cmc.vf_coef, cmc.ent_coef, cmc.eps_clip, cmc.update_episodes, cmc.action_std) == (3e-4, 1.0, 0.01, 0.2, 10.0, 0.5)
    # a fractional update_episodes: the float comparison of PPO.py:100
    cmc.update_episodes, cmc.same_action_num, cmc.max_steps = 2.5, 1, 11
    assert ppo_rows(cmc) == 28 == L.lenv_ppo_rows(C.byref(cmc))


def test_refusals_before_a_launch():
    from learning_environments_amd.experiments.transfer_algo import PPO_SETTINGS
    L = _lib.lib()
    base = ppo_cfg_from_config(_script_config("Pendulum-v0", PPO_SETTINGS["HalfCheetah-v3"], 200))
    assert L.lenv_ppo_rn_workspace_bytes(C.byref(base), 4) > 0

    def probe(**kw):
        c = _lib.PpoCfg.from_buffer_copy(base)
        for k, v in kw.items():
            setattr(c, k, v)
        return [L.lenv_ppo_rn_workspace_bytes(C.byref(c), 4), L.lenv_ppo_num_params(C.byref(c), None, None), L.lenv_ppo_rows(C.byref(c))]
    UNS = -2
    assert probe(hidden=129) == [UNS] * 3                       # hidden_size <= 128
    assert probe(layers=3) == [UNS] * 3                         # hidden_layer 1-2
    assert probe(act=_lib.ACT["prelu"]) == [UNS] * 3            # a PReLU agent activation
    assert probe(update_episodes=20.0) == [UNS] * 3             # 4001 rows: over the compile-time cap of 2048
    assert probe(update_episodes=0.0, max_steps=1000) == [UNS] * 3      # one row: the unbiased std of the returns is NaN
    assert probe(test_episodes=65) == [UNS] * 3
    assert probe(reward_env_type=9) == [UNS] * 3                # reward_env.py: NotImplementedError
    assert probe(state_dim=4) == [UNS] * 3                      # not one of the three continuous real envs
    assert probe(reward_env_type=3) == [-1] * 3                 # Pendulum's step has no info vector: the reference's ValueError
    assert probe(update_episodes=float("nan")) == [UNS] * 3
    with pytest.raises(ValueError):
        nan = _lib.PpoCfg.from_buffer_copy(base)
        nan.update_episodes = float("nan")
        ppo_rows(nan)
    # a launch itself: invalid without outputs / workspace, never reaches the device
    assert L.lenv_ppo_rn_inner_loop(C.byref(base), None, None, None, None, None, None, None, 1, None, 0, None, None) == -1


def test_select_task_and_config_refusals():
    from learning_environments_amd.agents.tasks import select_task
    from learning_environments_amd.experiments.transfer_algo import PPO_SETTINGS

    class Hip(object):
        name = "hip"
        device = "cpu"

    class Other(object):
        name = "oracle"
        device = "cpu"
    cfg = _script_config("Pendulum-v0", PPO_SETTINGS["HalfCheetah-v3"], 200)
    cfg["agents"]["gtn"]["agent_name"] = "ppo"
    task = select_task(cfg, Hip(), None)
    assert task.name == "ppo_rn" and task.needs_agent_init()
    A = task.cfg.action_dim
    assert task.agent_bounds.numel() == _lib.lib().lenv_ppo_num_params(C.byref(task.cfg), None, None)
    assert (task.agent_bounds[:A] == 0).all() and abs(float(task.agent_bounds[A]) - 3 ** -0.5) < 1e-7
    with pytest.raises(NotImplementedError, match="HIP engine"):
        select_task(cfg, Other(), None)
    with pytest.raises(NotImplementedError, match="test_mode 1"):
        select_task(cfg, Hip(), None, test_mode=1)
    for mutate, what in ((lambda c: c["agents"]["gtn"].update(synthetic_env_type=0), "VirtualEnv"),
                         (lambda c: c["agents"]["gtn"].update(agent_name="ppo_icm"), "ppo_icm"),
                         (lambda c: c.update(env_name="CartPole-v0"), "CartPole-v0"),
                         (lambda c: c["agents"]["ppo"].update(use_layer_norm=True), "use_layer_norm")):
        bad = copy.deepcopy(cfg)
        mutate(bad)
        with pytest.raises(NotImplementedError, match=what):
            select_task(bad, Hip(), None)
    bad = copy.deepcopy(cfg)
    bad["agents"]["ppo"]["activation_fn"] = "prelu"
    with pytest.raises(NotImplementedError):
        from learning_environments_amd import engine
        engine._count("lenv_ppo_num_params", C.byref(ppo_cfg_from_config(bad)), None, None)


def test_struct_sizes_through_the_abi_table():
    L = _lib.lib()
    assert [L.lenv_struct_size(i) for i in (14, 15, 16)] == [C.sizeof(_lib.PpoCfg), C.sizeof(_lib.PpoTapes), C.sizeof(_lib.PpoOut)] == [176, 64, 128]
    assert _lib.ABI_STRUCTS[14:] == [_lib.PpoCfg, _lib.PpoTapes, _lib.PpoOut] and L.lenv_struct_size(17) == -1
    assert L.lenv_abi_version() == 7
    for name in ("lenv_ppo_rows", "lenv_ppo_num_params", "lenv_ppo_rn_num_params", "lenv_ppo_rn_workspace_bytes", "lenv_ppo_rn_inner_loop"):
        assert name in _lib.EXPORTS and hasattr(L, name)

