"""The gridworld reward-net transfer experiments (experiments/transfer_gridworld.py, lenv_ql_rn_inner_loop_hp), CPU side: every agent the
reference's two scripts trained for the g16* fixtures is replayed through the oracle chain with its own alpha / gamma, and the restated
settings, the draw and the new export are checked without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gridworld_transfer_ref as gt
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("agent", range(gt.AGENTS))
@pytest.mark.parametrize("name", gt.FIXTURES)
def test_replay_of_every_agent_is_the_reference_run(golden, name, agent):
    """Trajectory, explored flags, fp64 Q-table (bit-equal) and both returned lists of agent.train(env=env, test_env=real_env) with the agent's
    own alpha / gamma.  As in test_g9_calc_score_cliff the integer path is pinned with the reference's own shaped-reward table as input (an
    ulp of torch's gemv order can flip an argmax); the oracle's table for that gamma is held to G9's bound."""
    g = golden(name)
    a = gt.agent_slices(g, agent)
    cfg, tables = gt.oracle_cfg(orc, g, a["alpha"], a["gamma"])
    assert (cfg.alpha, cfg.gamma, cfg.test_mode) == (a["alpha"], a["gamma"], 0)
    tapes = orc.make_tapes(a["eps"], a["act"], np.zeros(0, np.int32), np.zeros((0, 4)), np.zeros((0, 4)))
    _, shaped = orc.rn_shaped_rewards(cfg, g["theta"], tables)
    np.testing.assert_allclose(shaped, a["shaped_ref"], rtol=2e-6, atol=2e-6)
    n = a["tr_action"].size
    out = orc.ql_rn_chain(cfg, g["theta"], tables, tapes=tapes, trace_cap=n + 4, shaped_override=a["shaped_ref"])
    assert out["rc"] == 0
    tr = out["trace"]
    assert tr["action"].size == n
    assert np.array_equal(tr["action"] & 0xFFFF, a["tr_action"])
    assert np.array_equal(tr["action"] >> 16, a["tr_explored"])
    assert np.array_equal(tr["state"], a["tr_state"])
    assert np.array_equal(tr["next_state"], a["tr_next_state"])
    assert np.array_equal(tr["done"], a["tr_done"])
    assert np.array_equal(tr["reward"], a["tr_reward"])
    assert np.array_equal(out["q_table"], a["q_table"])          # fp64 Q-table: bit-exact
    ne = a["reward_list"].size
    assert ne == cfg.train_episodes == 500                       # solved_reward 100000: no early out
    assert np.array_equal(out["episode_test_mean"], a["reward_list"])
    assert np.array_equal(out["episode_len"], a["episode_length"])


def test_fixtures_cover_what_they_are_for(golden):
    for name in gt.FIXTURES:
        g = golden(name)
        ag = [gt.agent_slices(g, i) for i in range(gt.AGENTS)]
        if str(g["script"]) == "vary_hp":
            assert len({a["alpha"] for a in ag}) == gt.AGENTS and len({a["gamma"] for a in ag}) == gt.AGENTS, name
            assert min(a["alpha"] for a in ag) < 0.5, name
            assert all(0.1 <= a["alpha"] <= 1.0 and 0.1 <= a["gamma"] <= 1.0 for a in ag), name
        else:
            assert all((a["alpha"], a["gamma"]) == (1.0, 0.8) for a in ag), name
        for a in ag:
            assert a["tr_explored"].any() and not a["tr_explored"].all(), name
        if str(g["agent_name"]).endswith("_cb"):
            for a in ag:
                sa = a["tr_state"].astype(np.int64) * 4 + a["tr_action"]
                assert np.bincount(sa).max() > 1, name          # a revisited (s, a): the bonus beta / sqrt(n) with n > 1
    assert {(str(golden(n)["script"]), str(golden(n)["mode"])) for n in gt.FIXTURES} == {("vary_hp", "2"), ("vary_hp", "0"), ("vary_hp", "-1"),
                                                                                      ("algo", "5"), ("algo", "-1")}
    # reward nets with one and with two hidden layers
    assert {gt.recorded_config(golden(n))[0]["envs"]["Cliff"]["hidden_layer"] for n in gt.FIXTURES} == {1, 2}


def test_restated_settings_are_what_the_scripts_left_in_the_config(golden):
    from learning_environments_amd.experiments import transfer_gridworld as tg
    for name in gt.FIXTURES:
        g = golden(name)
        cfgd, _ = gt.recorded_config(g)
        if str(g["script"]) == "vary_hp":
            assert cfgd["agents"]["ql"] == tg.QL_SETTINGS, name
        else:
            assert cfgd["agents"]["sarsa"] == tg.SARSA_SETTINGS, name
        assert cfgd["envs"]["Cliff"]["solved_reward"] == tg.SOLVED_REWARD
        assert str(g["agent_name"]) == tg.agent_name_of(str(g["mode"]), str(g["script"]))
    assert tg.MODEL_AGENTS == tg.MODEL_NUM == 10 and tg.MODES == ("-1", "0", "1", "2", "5", "6")


def test_settings_are_written_in_place_and_vary_hp_returns_a_copy():
    from learning_environments_amd.experiments import transfer_gridworld as tg
    config = {"agents": {"ql": dict(tg.QL_SETTINGS, alpha=0.3)}}
    mod = tg.vary_hp(config, [0.5, 0.25])
    assert mod is not config and mod["agents"]["ql"] is not config["agents"]["ql"]
    assert config["agents"]["ql"]["alpha"] == 0.3 and config["agents"]["ql"]["gamma"] == 0.8
    assert mod["agents"]["ql"]["alpha"] == 0.5 * (1 - 0.1) + 0.1 and mod["agents"]["ql"]["gamma"] == 0.25 * (1 - 0.1) + 0.1
    assert {k: v for k, v in mod["agents"]["ql"].items() if k not in ("alpha", "gamma")} == \
        {k: v for k, v in tg.QL_SETTINGS.items() if k not in ("alpha", "gamma")}


def test_vary_tabular_bounds_order_and_clipping():
    from learning_environments_amd.agents import vary
    assert vary.TABULAR_HP_ORDER == ("alpha", "gamma") == tuple(sorted(vary.TABULAR_HP_BOUNDS))
    assert vary.TABULAR_HP_BOUNDS == {"alpha": (0.1, 1.0), "gamma": (0.1, 1.0)}
    sec = {"alpha": 1.0, "gamma": 0.8}
    assert vary.vary_tabular(sec, [0.0, 0.0]) == {"alpha": 0.1, "gamma": 0.1}
    hi = vary.vary_tabular(sec, [1.0 - 2 ** -53, 1.0 - 2 ** -53])
    assert hi["alpha"] <= 1.0 and hi["gamma"] <= 1.0 and hi["alpha"] > 0.999999
    # the first unit is alpha's, the second gamma's; the section's own values do not enter
    d = vary.vary_tabular(sec, [0.25, 0.75])
    assert d == vary.vary_tabular({"alpha": 0.2, "gamma": 0.3}, [0.25, 0.75]) == {"alpha": 0.25 * (1.0 - 0.1) + 0.1, "gamma": 0.75 * (1.0 - 0.1) + 0.1}
    assert list(d) == ["alpha", "gamma"]
    # clipped to the bounds (a unit outside [0, 1) cannot leave them)
    assert vary.vary_tabular(sec, [-0.5, 1.5]) == {"alpha": 0.1, "gamma": 1.0}
    # uniform: mean and spread of a large sample
    u = np.random.RandomState(5).uniform(size=(20000, 2))
    s = np.array([[v["alpha"], v["gamma"]] for v in (vary.vary_tabular(sec, r) for r in u)])
    assert s.min() >= 0.1 and s.max() <= 1.0
    assert np.all(np.abs(s.mean(axis=0) - 0.55) < 0.01) and np.all(np.abs(s.std(axis=0) - 0.9 / np.sqrt(12)) < 0.01)
    # the chain's units are draws 0 and 1 of its key on STREAM_VARY_HP
    from learning_environments_amd import _lib
    L = _lib.lib()
    assert vary.chain_units(12345, 2) == [L.lenv_rng_unit(12345, vary.STREAM_VARY_HP, 0), L.lenv_rng_unit(12345, vary.STREAM_VARY_HP, 1)]
    assert vary.chain_units(12345)[:2] == vary.chain_units(12345, 2) and len(vary.chain_units(12345)) == 4


def test_hp_entry_is_exported_declared_and_refuses_null_arguments():
    from learning_environments_amd import _lib
    L = _lib.lib()
    name = "lenv_ql_rn_inner_loop_hp"
    header = open(os.path.join(ROOT, "include", "lenv_hip.h")).read()
    assert name in _lib.EXPORTS and hasattr(L, name)
    assert re.search(r"\b%s\s*\(" % name, header)
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # lenv_ql_cfg as it is, two arrays in front of the plain entry's arguments
    plain, hp = _lib.SIGNATURES["lenv_ql_rn_inner_loop"][1], _lib.SIGNATURES[name][1]
    assert hp == [plain[0], C.c_void_p, C.c_void_p] + plain[1:]
    assert L.lenv_abi_version() == 7 and len(_lib.ABI_STRUCTS) == 17 and L.lenv_struct_size(17) == -1
    # argument validation happens before any device work: the plain entry's codes
    cfg = _lib.QlCfg(n_states=48, n_actions=4, max_steps=50, rn_hidden=32, rn_layers=1, reward_env_type=2, train_episodes=1, test_episodes=1,
                     batch_size=1, rng_mode=_lib.RNG_COUNTER)
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
    out = _lib.QlOut(score=p)
    tail = (p, None, None, None, None, p, p, p, p, None, 1)
    for hp_args in ((None, None), (p, p)):
        assert L.lenv_ql_rn_inner_loop_hp(None, *hp_args, *tail, C.byref(out), None) == -1                 # NULL cfg
        assert L.lenv_ql_rn_inner_loop_hp(C.byref(cfg), *hp_args, *tail, None, None) == -1                 # NULL out
        assert L.lenv_ql_rn_inner_loop_hp(C.byref(cfg), *hp_args, *tail, C.byref(_lib.QlOut()), None) == -1   # NULL out->score
        assert L.lenv_ql_rn_inner_loop_hp(C.byref(cfg), *hp_args, p, None, None, None, None, None, p, p, p, None, 1, C.byref(out), None) == -1   # NULL table
        assert L.lenv_ql_rn_inner_loop_hp(C.byref(cfg), *hp_args, p, None, None, None, None, p, p, p, None, None, 1, C.byref(out), None) == -1   # counter mode, no keys
        assert L.lenv_ql_rn_inner_loop_hp(C.byref(cfg), *hp_args, p, p, None, None, None, p, p, p, p, None, 1, C.byref(out), None) == -1        # eps without worker / sign
    assert L.lenv_ql_rn_inner_loop(None, *tail, C.byref(out), None) == L.lenv_ql_rn_inner_loop(C.byref(cfg), *tail, None, None) == -1
