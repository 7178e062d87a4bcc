"""PPO with an Intrinsic Curiosity Module, CPU side: the restatement (tests/ppo_icm_ref.c) against fixtures recorded from the reference's own
PPO(icm=True).train(env=reward_env, test_env=real_env) + agent.test(real_env) with every draw taped (tools/gen_golden_ppo_icm.py), and the
host logic that needs no device: the ABI housekeeping, the four entry points' refusals, the drivers' argument checks and ICM block.

Bounds of the replay.  Rows, per-episode test means, final returns and score: those of tests/test_ppo_reference.py (5e-5 / 2e-5 / 1e-4).
The three below are twice the worst |restatement - reference| measured over the four G19 runs:
    agent parameters after a learn call   1.94e-7  (g19h, both calls; 6e-8 on the other three)   -> 3.9e-7
    ICM parameters after a learn call     2.98e-8  (g19c, g19h, g19r)                             -> 6.0e-8
    intrinsic rewards of a call           2.24e-8  (g19r, first call; rewards up to 0.157)        -> 4.5e-8
(the module takes one Adam step of lr 1e-3 per call, so the re-association of the stacked-rows feature gradient stays at the last bit of
that step and, unlike over the hundreds of steps of a DDQN / TD3 run, the module's distance does not exceed the agent's).  The fixtures hold
no parameters "after the run": only PPO.learn changes them, so they are those after the last call."""
import copy
import ctypes as C
import json

import numpy as np
import pytest

import ppo_icm_ref
from learning_environments_amd import _lib
from learning_environments_amd.config import icm_layer_dims, ppo_cfg_from_config, ppo_icm_settings

FIXTURES = ["g19p_ppo_icm_pendulum_type2", "g19c_ppo_icm_cmc_type5_k5", "g19h_ppo_icm_cheetah_type0", "g19r_ppo_icm_pendulum_131_rows"]
PARAM_ATOL = 3.9e-7
ICM_ATOL = 6.0e-8
INTR_ATOL = 4.5e-8
ENTRIES = ("lenv_ppo_icm_num_params", "lenv_ppo_icm_workspace_bytes", "lenv_ppo_icm_inner_loop", "lenv_ppo_icm_inner_loop_segment")


def replay(golden, name):
    """(fixture, cfg, icm settings, tapes, the restatement's run of it)"""
    g = golden(name)
    config = json.loads(str(g["config_json"]))
    cfg = ppo_cfg_from_config(config, rng_mode=_lib.RNG_TAPE)
    icm = ppo_icm_settings(config)
    tapes = dict(act_noise=g["tape_act_noise"], test_noise=g["tape_test_noise"], train_reset=g["tape_train_reset"], test_reset=g["tape_test_reset"])
    out = ppo_icm_ref.chain(cfg, icm, g["icm_init"], g["theta"], g["agent_init"], tapes=tapes, trace_cap=g["tr_reward"].size + 4,
                            learn_cap=g["learn_step"].size + 2)
    return g, cfg, icm, tapes, out


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_against_the_reference(golden, name):
    g, cfg, icm, _, out = replay(golden, name)
    assert out["rc"] == 0
    tr, n = out["trace"], g["tr_reward"].size
    assert tr["reward"].size == n
    np.testing.assert_allclose(tr["state"], g["tr_state"], rtol=0, atol=5e-5)
    np.testing.assert_allclose(tr["action"], g["tr_action"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(tr["next_state"], g["tr_next_state"], rtol=0, atol=5e-5)
    np.testing.assert_allclose(tr["reward"], g["tr_reward"], rtol=0, atol=5e-5)
    assert np.array_equal(tr["done"], g["tr_done"])
    assert np.array_equal(out["episode_len"], g["episode_length_train"])
    assert np.array_equal(out["learn_step"], g["learn_step"]) and out["learn_calls"] == g["learn_step"].size >= 2
    assert g["learn_step"][-1] < n                         # rows acted by the policy the ICM-augmented returns trained
    rows = g["learn_intr"].shape[1]
    assert rows == ppo_icm_ref.ppo_ref.rows(cfg)
    dev_p = np.abs(out["learn_params"] - g["learn_params"]).max(axis=1)
    dev_i = np.abs(out["learn_icm"] - g["learn_icm"]).max(axis=1)
    dev_r = np.abs(out["learn_intr"][:, :rows] - g["learn_intr"]).max(axis=1)
    print(name, "max |restatement - reference| per learn call: agent", dev_p, "icm", dev_i, "intrinsic rewards", dev_r)
    np.testing.assert_allclose(out["learn_params"], g["learn_params"], rtol=0, atol=PARAM_ATOL)
    assert np.array_equal(out["final_params"], out["learn_params"][-1]) and np.array_equal(out["icm_final"], out["learn_icm"][-1])
    np.testing.assert_allclose(out["learn_icm"], g["learn_icm"], rtol=0, atol=ICM_ATOL)
    np.testing.assert_allclose(out["learn_intr"][:, :rows], g["learn_intr"], rtol=0, atol=INTR_ATOL)
    np.testing.assert_allclose(out["episode_test_mean"], g["reward_list_train"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(out["final_returns"], g["reward_list_test"], rtol=0, atol=1e-4)
    assert abs(out["score"] - float(g["score"])) <= 1e-4
    # the module did train, and the intrinsic term is not negligible next to the shaped reward
    assert np.abs(g["learn_icm"][0] - g["icm_init"]).max() > 1e-4 and np.abs(g["learn_icm"][-1] - g["learn_icm"][0]).max() > 1e-4
    assert g["learn_intr"].max() > 1e-3 * np.abs(g["tr_reward"]).max()


def test_fixtures_cover_what_they_are_for(golden):
    want = {"g19p_ppo_icm_pendulum_type2": ("Pendulum-v0", 2, 1, 28, (8, 16)), "g19c_ppo_icm_cmc_type5_k5": ("MountainCarContinuous-v0", 5, 5, 13, (5, 24)),
            "g19h_ppo_icm_cheetah_type0": ("HalfCheetah-v3", 0, 1, 19, (4, 8)), "g19r_ppo_icm_pendulum_131_rows": ("Pendulum-v0", 2, 1, 131, (5, 12))}
    for name, (env, rtype, k, rows, dims) in want.items():
        g = golden(name)
        c = json.loads(str(g["config_json"]))
        ic = c["agents"]["icm"]
        assert c["env_name"] == env and c["envs"][env]["reward_env_type"] == rtype and c["agents"]["ppo"]["same_action_num"] == k
        assert g["learn_intr"].shape[1] == rows and (ic["feature_dim"], ic["hidden_size"]) == dims and (ic["beta"], ic["eta"]) == (0.2, 0.5)
        cfg = ppo_cfg_from_config(c)
        assert g["icm_init"].size == sum(i * o + o for i, o in icm_layer_dims(cfg, *dims)) == ppo_icm_ref.icm_num_params(cfg, *dims)
    g = golden("g19p_ppo_icm_pendulum_type2")
    assert any(int(s) % 11 != 0 for s in g["learn_step"])                 # a learn call in the middle of an episode
    g = golden("g19c_ppo_icm_cmc_type5_k5")
    assert not np.array_equal(g["tr_next_state"][:-1], g["tr_state"][1:])   # s' is not the next row's s at an episode end
    assert golden("g19h_ppo_icm_cheetah_type0")["tr_action"].shape[1] == 6


def test_abi_housekeeping_is_unchanged_and_the_entries_are_there():
    L = _lib.lib()
    assert L.lenv_abi_version() == 7 and len(_lib.ABI_STRUCTS) == 17 and L.lenv_struct_size(17) == -1
    assert L.lenv_struct_size(14) == C.sizeof(_lib.PpoCfg) == 176 and L.lenv_struct_size(12) == C.sizeof(_lib.IcmIo) == 16
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(L, name)


def _base_cfg():
    from learning_environments_amd.experiments.transfer_algo import PPO_SETTINGS, base_config
    config = base_config("Pendulum-v0")
    config["agents"]["ppo"] = dict(PPO_SETTINGS["HalfCheetah-v3"])
    config["envs"]["Pendulum-v0"]["max_steps"] = 200
    return ppo_cfg_from_config(config)


def test_queries_and_layout():
    L = _lib.lib()
    base = _base_cfg()
    for F, H in ((32, 128), (1, 1), (128, 128), (5, 24)):
        P = L.lenv_ppo_icm_num_params(C.byref(base), F, H)
        assert P == sum(i * o + o for i, o in icm_layer_dims(base, F, H)) == ppo_icm_ref.icm_num_params(base, F, H)
        one, many = L.lenv_ppo_icm_workspace_bytes(C.byref(base), F, H, 1), L.lenv_ppo_icm_workspace_bytes(C.byref(base), F, H, 48)
        assert one > 0 and many - 256 == 48 * (one - 256)
        rows = L.lenv_ppo_rows(C.byref(base))
        # the ICM-less arena, the next-observation rows, four parameter-sized arrays, the stacked feature activations and their gradients
        assert one - 256 >= L.lenv_ppo_rn_workspace_bytes(C.byref(base), 1) - 256 + 4 * (rows * base.state_dim + 4 * P + 2 * rows * (4 * H + 2 * F))


def test_refusals_before_a_launch():
    """Every refusal with chains = 0 and host pointers: nothing reaches the device."""
    L = _lib.lib()
    base = _base_cfg()
    INV, UNS = -1, -2
    buf = (C.c_float * 16)()
    ptr = C.cast(buf, C.c_void_p)
    io = _lib.IcmIo(ptr, None)
    out = _lib.PpoOut()
    out.score = ptr
    keys = ptr

    def launch(cfg=base, F=32, H=128, icm=io, segment=None, out=out, workspace=ptr, agent_init=ptr, rng_keys=keys, resume=ptr, theta=ptr):
        icm_arg = C.byref(icm) if icm is not None else None
        head = (C.byref(cfg), F, H, 5e-4, 0.1, 0.01, icm_arg, theta, None, None, None, agent_init, rng_keys, None, 0, workspace, 0,
                C.byref(out) if out is not None else None)
        if segment is None:
            return L.lenv_ppo_icm_inner_loop(*head, None)
        return L.lenv_ppo_icm_inner_loop_segment(*head, segment[0], segment[1], resume, None)
    E = base.train_episodes
    assert launch() == 0 and launch(segment=(0, E)) == 0 and launch(segment=(3, 7)) == 0       # admitted; zero chains: nothing to do
    for seg in (None, (0, E)):
        assert launch(icm=None, segment=seg) == INV
        assert launch(icm=_lib.IcmIo(None, ptr), segment=seg) == INV
        for F, H in ((0, 128), (129, 128), (32, 0), (32, 129), (-1, -1)):
            assert launch(F=F, H=H, segment=seg) == UNS
        # everything the ICM-less entries refuse, with their codes
        assert launch(out=None, segment=seg) == INV and launch(workspace=None, segment=seg) == INV and launch(agent_init=None, segment=seg) == INV
        assert launch(rng_keys=None, segment=seg) == INV            # counter mode without keys
        for field, value, code in (("hidden", 129, UNS), ("layers", 3, UNS), ("act", _lib.ACT["prelu"], UNS), ("update_episodes", 20.0, UNS),
                                   ("test_episodes", 65, UNS), ("reward_env_type", 9, UNS), ("state_dim", 4, UNS), ("reward_env_type", 3, INV),
                                   ("rng_mode", 7, INV)):
            bad = _lib.PpoCfg.from_buffer_copy(base)
            setattr(bad, field, value)
            assert launch(cfg=bad, segment=seg) == code, (field, seg)
        tape = _lib.PpoCfg.from_buffer_copy(base)
        tape.rng_mode = _lib.RNG_TAPE
        assert launch(cfg=tape, segment=seg) == INV                 # tape mode without tapes
        typed = _lib.PpoCfg.from_buffer_copy(base)
        typed.reward_env_type = 2
        assert launch(cfg=typed, theta=None, segment=seg) == INV    # a reward net without theta
    for seg in ((-1, 2), (2, 2), (3, 1), (0, E + 1)):
        assert launch(segment=seg) == INV
    assert launch(segment=(0, E), resume=None) == INV
    for F, H in ((0, 128), (32, 129)):
        assert L.lenv_ppo_icm_num_params(C.byref(base), F, H) == UNS and L.lenv_ppo_icm_workspace_bytes(C.byref(base), F, H, 4) == UNS
    bad = _lib.PpoCfg.from_buffer_copy(base)
    bad.hidden = 129
    assert L.lenv_ppo_icm_num_params(C.byref(bad), 32, 128) == UNS and L.lenv_ppo_icm_workspace_bytes(C.byref(bad), 32, 128, 4) == UNS
    assert L.lenv_ppo_icm_num_params(None, 32, 128) == INV and L.lenv_ppo_icm_workspace_bytes(C.byref(base), 32, 128, -1) == INV


def test_icm_settings_of_the_two_scripts():
    from learning_environments_amd.experiments import transfer_algo as ta
    assert ta.ICM_SETTINGS["MountainCarContinuous-v0"] == dict(beta=0.1, eta=0.01, feature_dim=32, hidden_size=128, lr=5e-4)
    assert ta.ICM_SETTINGS["HalfCheetah-v3"] == dict(beta=0.05, eta=0.03, feature_dim=32, hidden_size=128, lr=1e-4)
    assert sorted(ta.ICM_SETTINGS) == sorted(ta.PPO_SETTINGS)
    config = ta.base_config("HalfCheetah-v3")
    config["agents"]["icm"] = dict(ta.ICM_SETTINGS["HalfCheetah-v3"])
    assert ppo_icm_settings(config) == dict(feature_dim=32, hidden_size=128, lr=1e-4, beta=0.05, eta=0.03)
    assert "-1" not in ta.MODES
    with pytest.raises(NotImplementedError, match="ppo_icm"):
        ta._check_mode("-1")


class _Env(object):
    def __init__(self, virtual):
        self.virtual = virtual

    def is_virtual_env(self):
        return self.virtual


def test_driver_argument_checks():
    """What train_test_agents_icm refuses before it touches a device -- and the blocks it has written into the config by then."""
    from learning_environments_amd.experiments import transfer_algo as ta
    env_name = "MountainCarContinuous-v0"
    config = ta.base_config(env_name)
    with pytest.raises(ValueError, match="does not match"):
        ta.train_test_agents_icm(_Env(False), copy.deepcopy(config), "HalfCheetah-v3")
    with pytest.raises(ValueError, match="real environment"):
        ta.train_test_agents_icm(_Env(True), copy.deepcopy(config), env_name)
    pend = ta.base_config("Pendulum-v0")
    with pytest.raises(NotImplementedError, match="no transfer script"):
        ta.train_test_agents_icm(_Env(False), pend)
    with pytest.raises(ValueError, match="unknown entries"):
        ta.train_test_agents_icm(_Env(False), copy.deepcopy(config), env_name, icm=dict(feature_size=8))
    cfg = copy.deepcopy(config)
    with pytest.raises(ValueError, match="replay"):
        ta.train_test_agents_icm(_Env(False), cfg, env_name, agents_num=2, settings=dict(train_episodes=3), icm=dict(eta=0.5),
                                 replay=dict(agent_init=[[0.0]], icm_init=[[0.0]], tapes=[{}]))
    assert cfg["agents"]["ppo"] == dict(ta.PPO_SETTINGS[env_name], train_episodes=3)
    assert cfg["agents"]["icm"] == dict(ta.ICM_SETTINGS[env_name], eta=0.5)
