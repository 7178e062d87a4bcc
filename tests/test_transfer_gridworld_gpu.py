"""The gridworld reward-net transfer experiments on the GPU: lenv_ql_rn_inner_loop_hp (per-chain alpha / gamma) against the plain entry and the
oracle, bit for bit, and experiments/transfer_gridworld.py against the runs of the reference's two scripts (the g16* fixtures).  Cliff: 48
states x 4 actions."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import gridworld_transfer_ref as gt
from learning_environments_amd import _lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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
    return (t.to(dtype) if dtype is not None else t).cuda()


def _cfgs(orc, golden, agent, rtype, layers, rng_mode=0, **agent_over):
    """(oracle cfg, HIP cfg, tables, P) of a Cliff RewardEnv of the type with `layers` hidden layers and the named tabular agent"""
    from learning_environments_amd.config import ql_cfg_from_config
    cfgd, tables = gt.recorded_config(golden(gt.FIXTURES[0]))
    cfgd["agents"]["gtn"]["agent_name"] = agent
    sec = "sarsa" if agent.startswith("sarsa") else "ql"
    cfgd["agents"][sec] = dict(cfgd["agents"]["ql"], eps_init=0.3, eps_min=0.05, eps_decay=0.9, train_episodes=30, **agent_over)
    cfgd["envs"]["Cliff"].update(reward_env_type=rtype, hidden_layer=layers, activation_fn="tanh" if layers == 2 else "prelu", solved_reward=-20)
    ocfg = orc.ql_cfg_from_config(cfgd, tables, rng_mode=rng_mode)
    cfg = ql_cfg_from_config(cfgd, tables, rng_mode=rng_mode)
    for f, _ in _lib.QlCfg._fields_:
        assert f == "early_out_virtual_diff" or getattr(cfg, f) == getattr(ocfg, f), f     # (a grid RewardEnv never reads the virtual early-out rule)
    H = cfg.rn_hidden
    return ocfg, cfg, tables, 48 * H + H + (layers - 1) * (H * H + H) + H + 1


def _population(orc, P, pop, seed):
    rng = np.random.RandomState(seed)
    theta = (rng.randn(P) * 0.3).astype(np.float32)
    eps = (rng.randn(pop, P) * 0.1).astype(np.float32)
    return theta, eps


def _outputs(il):
    torch.cuda.synchronize()
    out = {k: getattr(il, k).cpu().numpy().copy() for k in ("score", "stats", "status", "episode_test_mean", "episode_len", "final_returns", "q_table", "shaped")}
    out.update({"trace_" + k: v.cpu().numpy().copy() for k, v in il.trace.items()})
    return out


def _run_hp_entry(eng, il, alpha, gamma, theta, eps, worker, sign, keys):
    """the C entry itself (engine.QlInnerLoop.run goes to the plain entry when no hp is set): alpha / gamma device tensors or None"""
    p = eng._ptr
    rc = _lib.lib().lenv_ql_rn_inner_loop_hp(C.byref(il.cfg), p(alpha), p(gamma), p(theta), p(eps), p(worker), p(sign), None, p(il.next_state),
                                             p(il.reward), p(il.done), p(keys), None, il.chains, C.byref(il.out), eng._stream())
    assert rc == 0


@pytest.mark.parametrize("agent,rtype,layers", [("ql", 2, 1), ("sarsa_cb", 1, 2)])
def test_hp_entry_with_cfg_values_is_the_plain_entry_bit_for_bit(eng, orc, golden, agent, rtype, layers):
    """(a) NULL / NULL, arrays filled with cfg's alpha / gamma, one array only, and QlInnerLoop.set_hp with cfg's values: score, stats, episode
    arrays, Q-table, shaped and the step trace of lenv_ql_rn_inner_loop, bit for bit; 5 chains."""
    _, cfg, tables, P = _cfgs(orc, golden, agent, rtype, layers, alpha=0.7, gamma=0.9, beta=0.1)
    chains = 5
    theta, eps = _population(orc, P, 2, 21)
    worker = np.array([0, 0, 1, 1, 0], np.int32)
    sign = np.array([0, 1, -1, 1, -1], np.float32)
    keys = np.array([orc.chain_key(7, 3, int(worker[c]), c) for c in range(chains)], np.uint64)
    args = (dev(theta), dev(eps), dev(worker), dev(sign), dev(keys.view(np.int64)))
    cap = cfg.train_episodes * cfg.max_steps
    plain = eng.QlInnerLoop(cfg, chains, tables, trace_cap=cap)
    plain.run(*args[:4], rng_keys=args[4])
    want = _outputs(plain)
    assert want["status"].tolist() == [0] * chains and want["stats"][:, 1].min() > 30
    al, ga = dev(np.full(chains, cfg.alpha)), dev(np.full(chains, cfg.gamma))
    for what, a, g in (("NULL / NULL", None, None), ("arrays", al, ga), ("alpha only", al, None), ("gamma only", None, ga)):
        il = eng.QlInnerLoop(cfg, chains, tables, trace_cap=cap)
        _run_hp_entry(eng, il, a, g, *args)
        got = _outputs(il)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))
    il = eng.QlInnerLoop(cfg, chains, tables, trace_cap=cap)
    il.set_hp([cfg.alpha] * chains, [cfg.gamma] * chains)
    il.run(*args[:4], rng_keys=args[4])
    got = _outputs(il)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg="set_hp: " + k)
    with pytest.raises(ValueError):
        il.set_hp([0.5] * (chains - 1), [0.5] * chains)


HETERO = [("ql", 2, 1), ("sarsa", 1, 2), ("ql_cb", 5, 2), ("sarsa_cb", 6, 1), ("ql", 0, 1), ("sarsa", 2, 2), ("ql_cb", 1, 1), ("sarsa_cb", 5, 1)]
ALPHAS = [0.1, 1.0, 0.37, 0.5, 0.9, 0.25, 0.73]
GAMMAS = [1.0, 0.1, 0.8, 0.95, 0.33, 0.6, 0.99]


def test_hetero_cases_cover_the_agents_types_and_depths():
    assert {c[0] for c in HETERO} == {"ql", "sarsa", "ql_cb", "sarsa_cb"} and {c[1] for c in HETERO} == {0, 1, 2, 5, 6} and {c[2] for c in HETERO} == {1, 2}
    assert 0.1 in ALPHAS and 1.0 in GAMMAS and len(set(ALPHAS)) == len(set(GAMMAS)) == 7


@pytest.mark.parametrize("agent,rtype,layers", HETERO)
def test_heterogeneous_population_vs_oracle_chain_by_chain(eng, orc, golden, agent, rtype, layers):
    """(b) 7 chains with their own (alpha, gamma) in one counter-mode launch of 30 training episodes; every chain against the oracle run with
    its own cfg copy: Q-table, shaped table (the chain's gamma in the potential term), score and the episode arrays, bit for bit."""
    ocfg, cfg, tables, P = _cfgs(orc, golden, agent, rtype, layers, beta=0.1)
    chains = 7
    theta, eps = _population(orc, P, 3, 40 + rtype)
    worker = np.array([0, 0, 0, 1, 1, 2, 2], np.int32)
    sign = np.array([0, 1, -1, 1, -1, 1, 0], np.float32)
    keys = np.array([orc.chain_key(11, 2, int(worker[c]), c) for c in range(chains)], np.uint64)
    il = eng.QlInnerLoop(cfg, chains, tables)
    il.set_hp(ALPHAS, GAMMAS)
    assert il.hp_alpha.dtype == il.hp_gamma.dtype == torch.float64 and il.hp_alpha.shape == (chains,) and il.hp_alpha.is_cuda
    il.run(dev(theta), dev(eps), dev(worker), dev(sign), rng_keys=dev(keys.view(np.int64)))
    torch.cuda.synchronize()
    assert il.status.cpu().tolist() == [0] * chains
    tables_seen = set()
    for c in range(chains):
        oc = copy.copy(ocfg)
        oc.alpha, oc.gamma = ALPHAS[c], GAMMAS[c]
        w = (np.float32(sign[c]) * eps[worker[c]] + theta).astype(np.float32)
        _, oshaped = orc.rn_shaped_rewards(oc, w, tables)
        o = orc.ql_rn_chain(oc, w, tables, rng_key=int(keys[c]))
        what = "%s type %d chain %d" % (agent, rtype, c)
        np.testing.assert_array_equal(il.shaped[c].cpu().numpy().reshape(48, 4), oshaped, err_msg=what)
        np.testing.assert_array_equal(il.q_table[c].cpu().numpy().reshape(48, 4), o["q_table"], err_msg=what)
        np.testing.assert_array_equal(il.episode_test_mean[c].cpu().numpy(), o["episode_test_mean"], err_msg=what)
        np.testing.assert_array_equal(il.episode_len[c].cpu().numpy(), o["episode_len"], err_msg=what)
        np.testing.assert_array_equal(il.final_returns[c].cpu().numpy(), o["final_test_returns"], err_msg=what)
        assert float(il.score[c]) == o["score"], what
        assert il.stats[c].cpu().tolist() == [o["episodes_run"], o["train_steps"], o["learn_steps"], o["test_steps"]], what
        tables_seen.add(oshaped.tobytes())
    if rtype in (1, 2):
        assert len(tables_seen) == chains          # gamma enters the potential term: no two chains share a table (chains 0 and 6 share the weights)


def _envs_of(g):
    """(env, real_env, config) of a fixture as the scripts' eval_models / eval_base pass them: built from the recorded config, the recorded theta in
    the reward net"""
    from learning_environments_amd.envs.env_factory import EnvFactory
    config = json.loads(str(g["config_json"]))
    fac = EnvFactory(config)
    real_env = fac.generate_real_env()
    if str(g["mode"]) in ("0", "-1"):
        return real_env, real_env, config
    env = fac.generate_reward_env()
    with torch.no_grad():
        env.env.flat_params().copy_(dev(g["theta"]))
    env.env.params_changed()
    return env, real_env, config


@pytest.mark.parametrize("name", gt.FIXTURES)
def test_fixture_agents_replayed_as_one_launch(golden, name):
    """(c) the three agents the reference's script trained = three chains of ONE tape-mode launch with per-chain alpha / gamma, through
    train_test_agents(..., replay=...): both returned lists are the reference's."""
    from learning_environments_amd.experiments import transfer_gridworld as tg
    g = golden(name)
    env, real_env, config = _envs_of(g)
    script, mode = str(g["script"]), str(g["mode"])
    section = "ql" if script == "vary_hp" else "sarsa"
    if script == "algo":                   # what the scripts find before they write their settings: no sarsa section / another ql section
        config["agents"].pop("sarsa", None)
    else:
        config["agents"]["ql"].update(train_episodes=7, alpha=0.123)
    (rewards, lengths), launch = tg.train_test_agents(mode, env, real_env, config, script=script, agents_num=gt.AGENTS, replay=gt.replay_of(g), details=True)
    assert config["agents"][section] == (tg.QL_SETTINGS if script == "vary_hp" else tg.SARSA_SETTINGS)          # written in place
    inner = launch["inner"]
    assert inner.cfg.rng_mode == _lib.RNG_TAPE and inner.cfg.test_mode == 0 and inner.chains == gt.AGENTS
    assert (inner.cfg.agent_kind, inner.cfg.count_based) == (int(script == "algo"), int(mode == "-1"))
    for i in range(gt.AGENTS):
        a = gt.agent_slices(g, i)
        assert launch["hp"][i] == dict(alpha=a["alpha"], gamma=a["gamma"])
        assert rewards[i] == a["reward_list"].tolist(), (name, i)
        assert lengths[i] == a["episode_length"].tolist(), (name, i)
        shaped = inner.shaped[i].cpu().numpy().reshape(48, 4)
        np.testing.assert_allclose(shaped, a["shaped_ref"], rtol=2e-6, atol=2e-6)
        assert inner.stats[i].cpu().tolist()[:3] == [500, a["tr_action"].size, a["tr_action"].size]
        if mode in ("0", "-1"):            # the real reward itself: nothing the reference's gemv order could move
            assert np.array_equal(shaped, a["shaped_ref"])
            assert np.array_equal(inner.q_table[i].cpu().numpy().reshape(48, 4), a["q_table"])


@pytest.fixture(scope="module")
def models(golden):
    """three Cliff reward envs of type 2 with their own weights, the real env and a config"""
    from learning_environments_amd.envs.env_factory import EnvFactory
    config = json.loads(str(golden(gt.FIXTURES[0])["config_json"]))
    fac = EnvFactory(config)
    torch.manual_seed(5)
    envs = [fac.generate_reward_env() for _ in range(3)]
    return envs, fac.generate_real_env(), config, fac


SMALL = dict(train_episodes=40)


@pytest.mark.parametrize("script,mode", [("vary_hp", "2"), ("algo", "2"), ("vary_hp", "-1")])
def test_model_loop_is_the_single_model_calls_bit_for_bit(models, script, mode):
    """(d) train_test_agents_models = [train_test_agents(model m, model_index=m)], the same seed the same result, another seed another draw"""
    from learning_environments_amd.agents import vary
    from learning_environments_amd.experiments import transfer_gridworld as tg
    envs, real_env, config, _ = models
    envs = envs if mode == "2" else [real_env] * 3
    config = copy.deepcopy(config)
    kw = dict(script=script, agents_num=4, seed=3, settings=SMALL)
    allm, launch = tg.train_test_agents_models(mode, envs, real_env, config, details=True, **kw)
    assert launch["inner"].chains == 12 and len(allm) == 3
    singles = [tg.train_test_agents(mode, envs[m], real_env, config, model_index=m, **kw) for m in range(3)]
    assert allm == singles
    assert tg.train_test_agents_models(mode, envs, real_env, config, **kw) == allm
    assert all(len(r) == 40 and len(l) == 40 for res in allm for r, l in zip(*res))
    if script == "vary_hp":
        hp = launch["hp"]
        assert hp == [vary.vary_tabular(None, vary.chain_units(k, 2)) for k in launch["keys"]]
        assert len({h["alpha"] for h in hp}) == 12 and len({h["gamma"] for h in hp}) == 12
        other = tg.train_test_agents_models(mode, envs, real_env, config, **dict(kw, seed=4))
        assert other != allm
    else:
        assert launch["hp"] is None and launch["inner"].hp_alpha is None          # the script's fixed alpha / gamma: the plain entry
    if mode == "2":
        assert allm[0] != allm[1]          # the models' own weights reach their chains


def test_refusals(models):
    from learning_environments_amd.experiments import transfer_gridworld as tg
    envs, real_env, config, fac = models
    config = copy.deepcopy(config)
    with pytest.raises(ValueError, match="reward_env_type"):
        tg.train_test_agents("1", envs[0], real_env, config, settings=SMALL)                # a type-2 model under mode 1
    with pytest.raises(ValueError, match="reward env"):
        tg.train_test_agents("2", real_env, real_env, config, settings=SMALL)               # eval_models needs the reward env
    venv = fac.generate_virtual_env()
    with pytest.raises(ValueError, match="VirtualEnv"):
        tg.train_test_agents("2", envs[0], venv, config, settings=SMALL)
    with pytest.raises(ValueError, match="VirtualEnv"):
        tg.train_test_agents("0", venv, real_env, config, settings=SMALL)
    with pytest.raises(NotImplementedError):
        tg.train_test_agents("3", envs[0], real_env, config, settings=SMALL)
    with pytest.raises(NotImplementedError):
        tg.train_test_agents("2", envs[0], real_env, config, script="vary", settings=SMALL)
    with pytest.raises(ValueError, match="replay"):
        tg.train_test_agents("0", real_env, real_env, config, agents_num=2, settings=SMALL,
                             replay=dict(hp=None, tapes=dict(eps_uniform=[np.zeros(4)], rand_action=[np.zeros(4, np.int32)])))


def test_reference_written_checkpoint(golden):
    """(e) load_envs_and_config on the checkpoint the reference wrote: the env, the raised solved_reward, and the kernel's shaped table of every
    recorded gamma within 2e-6 of what the reference's env paid."""
    from learning_environments_amd.experiments import transfer_gridworld as tg
    g = golden(gt.FIXTURES[0])
    reward_env, real_env, config = tg.load_envs_and_config(os.path.join(GOLDEN, gt.CKPT))
    e = config["envs"]["Cliff"]
    assert config["env_name"] == "Cliff" and e["solved_reward"] == 100000 and e["reward_env_type"] == 2
    assert reward_env.env.reward_env_type == 2 and not real_env.is_virtual_env() and real_env.env.tables["n_states"] == 48
    assert np.array_equal(reward_env.env.flat_params().cpu().numpy(), g["theta"])
    (rewards, lengths), launch = tg.train_test_agents("2", reward_env, real_env, config, agents_num=gt.AGENTS, replay=gt.replay_of(g), details=True)
    for i in range(gt.AGENTS):
        a = gt.agent_slices(g, i)
        np.testing.assert_allclose(launch["inner"].shaped[i].cpu().numpy().reshape(48, 4), a["shaped_ref"], rtol=2e-6, atol=2e-6)
        assert rewards[i] == a["reward_list"].tolist() and lengths[i] == a["episode_length"].tolist()
