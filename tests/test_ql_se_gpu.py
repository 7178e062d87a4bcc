"""Tabular agents on a gridworld VirtualEnv, GPU side: lenv_ql_se_inner_loop against its CPU restatement (tests/ql_se_ref.c) bit for bit, its SE
steps against lenv_se_step_population bit for bit, and GTN_Master / GTN_Worker end to end on configs.cliff_syn_env_ql."""
import threading

import numpy as np
import pytest
import torch

import ql_se_ref
from learning_environments_amd import _lib

pytestmark = pytest.mark.gpu

FIXTURES = ql_se_ref.FIXTURES


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda().contiguous()


def _same(a, b, what):
    """bit for bit (a NaN pad equals a NaN pad)"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(a, b, err_msg=what)


def _compare_chain(inner, c, ref, cfg, what):
    n = int(ref["train_steps"])
    st = inner.stats[c].cpu().numpy()
    assert int(inner.status[c]) == ref["status"] == 0, what
    assert st.tolist() == [ref["episodes_run"], ref["train_steps"], ref["learn_steps"], ref["test_steps"]], (what, st, ref["episodes_run"])
    assert n <= inner.trace_cap, "trace_cap too small for the comparison"
    tr = ref["trace"]
    _same(inner.trace["action"][c, :n].cpu().numpy(), tr["action"], what + " action")
    _same(inner.trace["state"][c, :n].cpu().numpy(), tr["state"], what + " state")
    _same(inner.trace["reward_done"][c, :n].cpu().numpy(), tr["reward_done"], what + " reward / done")
    _same(inner.trace_se[c, :n].cpu().numpy(), tr["se"], what + " raw SE outputs")
    _same(inner.q_table[c].cpu().numpy(), ref["q_table"], what + " Q-table")
    _same(inner.episode_test_mean[c, :cfg.train_episodes].cpu().numpy(), ref["episode_test_mean"], what + " meter")
    _same(inner.episode_len[c, :cfg.train_episodes].cpu().numpy(), ref["episode_len"], what + " episode lengths")
    _same(inner.final_returns[c].cpu().numpy(), ref["final_returns"], what + " final returns")
    assert float(inner.score[c]) == ref["score"], what


@pytest.mark.parametrize("name", FIXTURES)
def test_kernel_equals_restatement_in_tape_mode(golden, name):
    from learning_environments_amd.engine import QlSeInnerLoop
    g = golden(name)
    cfg, tables, tapes = ql_se_ref.fixture_inputs(g)
    cap = int(g["tr_action"].size) + 8
    ref = ql_se_ref.chain(cfg, g["theta"], tables, tapes=tapes, trace_cap=cap)
    inner = QlSeInnerLoop(cfg, 1, tables, want_episode_stats=True, trace_cap=cap)
    dt = dict(eps_uniform=_dev(tapes["eps_uniform"].reshape(1, -1), torch.float64), rand_action=_dev(tapes["rand_action"].reshape(1, -1), torch.int32))
    inner.run(_dev(g["theta"]), None, None, None, tapes=dt)
    torch.cuda.synchronize()
    _compare_chain(inner, 0, ref, cfg, name)
    # and the run is the reference's: the decisions of the fixture
    n = g["tr_action"].size
    assert np.array_equal(inner.trace["action"][0, :n].cpu().numpy() & 0xffff, g["tr_action"])
    assert np.array_equal(inner.trace["state"][0, :n, 1].cpu().numpy(), g["tr_next_state"])
    # a short tape: status -2 / -3 (the last underrun met: with the recorded actions replaced by 0 the run leaves the recorded trajectory and
    # may then outrun the other tape too), the chain finishes, and it is still the restatement's chain
    for key in ("eps_uniform", "rand_action"):
        short, short_host = dict(dt), dict(tapes)
        short[key], short_host[key] = dt[key][:, :1].contiguous(), tapes[key][:1]
        ref = ql_se_ref.chain(cfg, g["theta"], tables, tapes=short_host, trace_cap=cap)
        inner.run(_dev(g["theta"]), None, None, None, tapes=short)
        torch.cuda.synchronize()
        assert int(inner.status[0]) == ref["status"]
        if key == "eps_uniform" or name in ("g15a_ql_se_cliff_ql", "g15c_ql_se_emptyroom33_qlcb"):      # (g15d explores once: one entry is its whole tape)
            assert ref["status"] == (-2 if key == "eps_uniform" else -3)
        assert float(inner.score[0]) == ref["score"] and np.isfinite(ref["score"])
        assert inner.stats[0].cpu().numpy().tolist() == [ref["episodes_run"], ref["train_steps"], ref["learn_steps"], ref["test_steps"]]


# the four agent kinds on perturbed fixture thetas; same_action_num 2, test_mode 1 and a step_budget that cuts training short among them
COUNTER_CASES = [("g15a_ql_se_cliff_ql", dict(agent_kind=0, count_based=0)),
                 ("g15b_ql_se_holeroom_sarsa", dict(agent_kind=1, count_based=0)),
                 ("g15c_ql_se_emptyroom33_qlcb", dict(agent_kind=0, count_based=1, same_action_num=2)),
                 ("g15e_ql_se_emptyroom33_virtual_early_out", dict(agent_kind=1, count_based=1, test_mode=1)),
                 ("g15d_ql_se_cliff_ql_k2_tanh", dict(agent_kind=0, count_based=0, step_budget=400, solved_reward=1e9))]


def _counter_population(golden, name, over, cap=4096):
    from learning_environments_amd.engine import QlSeInnerLoop
    g = golden(name)
    cfg, tables, _ = ql_se_ref.fixture_inputs(g, rng_mode=_lib.RNG_COUNTER, **over)
    eps, worker, sign, per_chain = ql_se_ref.population(g["theta"], 4, 0.01, 7)
    keys = np.arange(1000, 1012, dtype=np.uint64) * np.uint64(0x9e3779b97f4a7c15)
    inner = QlSeInnerLoop(cfg, 12, tables, want_episode_stats=True, trace_cap=cap)
    inner.run(_dev(g["theta"]), _dev(eps), _dev(worker), _dev(sign), rng_keys=_dev(keys.view(np.int64)))
    torch.cuda.synchronize()
    return g, cfg, tables, (eps, worker, sign, per_chain, keys), inner


@pytest.mark.parametrize("name,over", COUNTER_CASES)
def test_kernel_equals_restatement_in_counter_mode(golden, name, over):
    g, cfg, tables, (eps, worker, sign, per_chain, keys), inner = _counter_population(golden, name, over)
    runs = []
    for c in range(12):
        ref = ql_se_ref.chain(cfg, per_chain[c], tables, rng_key=int(keys[c]), trace_cap=inner.trace_cap)
        assert np.isfinite(ref["trace"]["se"]).all()
        _compare_chain(inner, c, ref, cfg, "%s chain %d" % (name, c))
        runs.append(ref["episodes_run"])
    if over.get("step_budget"):
        assert 0 < min(runs) and max(runs) < cfg.train_episodes            # the budget really cut training short


@pytest.mark.parametrize("name", ["g15a_ql_se_cliff_ql", "g15b_ql_se_holeroom_sarsa"])
def test_one_se_step_is_one_se_step(golden, name):
    """The rows of trace_se equal lenv_se_step_population on the same perturbed theta, previous raw state vector and action."""
    from learning_environments_amd import engine
    g, cfg, tables, (eps, worker, sign, per_chain, keys), inner = _counter_population(golden, name, dict(solved_reward=1e9))
    assert cfg.same_action_num <= 1
    N, A = cfg.n_states, cfg.n_actions
    steps = inner.stats[:, 1].cpu().numpy()
    n = int(steps.max())
    assert 0 < n <= inner.trace_cap
    se = inner.trace_se[:, :n].cpu().numpy()
    act = (inner.trace["action"][:, :n].cpu().numpy() & 0xffff).astype(np.int32)
    lens = inner.episode_len.cpu().numpy()
    prev = np.zeros((12, n, N), np.float32)
    for c in range(12):
        prev[c, 1:] = se[c, :-1, :N]
        starts = np.concatenate([[0], np.cumsum(lens[c, :int(inner.stats[c, 0])])[:-1]])
        for s0 in starts:                                      # VirtualEnv.reset: the one-hot of the S cell
            prev[c, s0] = 0.0
            prev[c, s0, cfg.start_state] = 1.0
    descs = engine.se_descs(N, A, cfg.rn_hidden, cfg.rn_layers, cfg.rn_act, cfg.rn_prelu)
    ns, r, d = engine.se_step_population(descs, _dev(g["theta"]), _dev(eps), _dev(worker), _dev(sign), _dev(prev), _dev(act))
    ns, r, d = ns.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy()
    for c in range(12):
        k = int(steps[c])
        _same(se[c, :k, :N], ns[c, :k], "chain %d next-state vector" % c)
        _same(se[c, :k, N], r[c, :k], "chain %d reward" % c)
        _same(se[c, :k, N + 1], d[c, :k], "chain %d done" % c)


def test_parameter_count_equals_the_virtual_envs_flat_theta():
    import ctypes as C
    from learning_environments_amd import configs
    from learning_environments_amd.config import ql_se_cfg_from_config
    from learning_environments_amd.envs.env_factory import EnvFactory
    config = configs.cliff_syn_env_ql()
    venv = EnvFactory(config).generate_virtual_env()
    cfg = ql_se_cfg_from_config(config, venv.env.reset_env.env.tables)
    assert _lib.lib().lenv_ql_se_num_params(C.byref(cfg)) == 6738 == venv.env.flat_params().numel()


def test_workspace_path_equals_restatement():
    """128 x 2 on Cliff: the staged theta does not fit LDS and lives in the workspace."""
    import ctypes as C
    from learning_environments_amd import configs
    from learning_environments_amd.config import ql_se_cfg_from_config
    from learning_environments_amd.engine import QlSeInnerLoop
    from learning_environments_amd.envs.gridworld import transition_tables
    config = configs.cliff_syn_env_ql()
    config["envs"]["Cliff"].update(hidden_size=128, hidden_layer=2, max_steps=12)
    config["agents"]["ql"].update(train_episodes=3, eps_init=0.3, eps_min=0.3)
    tables = transition_tables("Cliff")
    cfg = ql_se_cfg_from_config(config, tables)
    P = ql_se_ref.num_params(cfg)
    assert _lib.lib().lenv_ql_se_workspace_bytes(C.byref(cfg), 2) >= 2 * 4 * P
    rng = np.random.RandomState(3)
    theta = (rng.standard_normal(P) * 0.05).astype(np.float32)
    keys = np.array([11, 12], np.uint64)
    inner = QlSeInnerLoop(cfg, 2, tables, want_episode_stats=True, trace_cap=64)
    inner.run(_dev(theta), None, None, None, rng_keys=_dev(keys.view(np.int64)))
    torch.cuda.synchronize()
    for c in range(2):
        _compare_chain(inner, c, ql_se_ref.chain(cfg, theta, tables, rng_key=int(keys[c]), trace_cap=64), cfg, "workspace chain %d" % c)


def test_a_nan_in_the_state_vector_resolves_as_in_torch_argmax(golden):
    """A NaN is the maximum for torch.argmax (the first one wins); kernel and restatement agree on it wherever the NaN sits among the lanes."""
    from learning_environments_amd.engine import QlSeInnerLoop
    g = golden("g15a_ql_se_cliff_ql")
    cfg, tables, _ = ql_se_ref.fixture_inputs(g, rng_mode=_lib.RNG_COUNTER, max_steps=6, train_episodes=6, solved_reward=1e9, eps_init=0.5, eps_min=0.5)
    theta = g["theta"].copy()
    theta[3280 - 48 + 41] = np.nan                 # the state net's output bias of state 41: the vector carries one NaN after a reset's first step
    keys = np.array([77, 78], np.uint64)
    inner = QlSeInnerLoop(cfg, 2, tables, want_episode_stats=True, trace_cap=64)
    inner.run(_dev(theta), None, None, None, rng_keys=_dev(keys.view(np.int64)))
    torch.cuda.synchronize()
    for c in range(2):
        ref = ql_se_ref.chain(cfg, theta, tables, rng_key=int(keys[c]), trace_cap=64)
        assert (ref["trace"]["state"][:, 1] == 41).any() and np.isnan(ref["trace"]["se"]).any()
        _compare_chain(inner, c, ref, cfg, "NaN chain %d" % c)


def _master_config(num_workers=8, max_iterations=2):
    from learning_environments_amd import configs
    cfg = configs.cliff_syn_env_ql(num_workers=num_workers, max_iterations=max_iterations)
    cfg["agents"]["ql"]["train_episodes"] = 12
    cfg["agents"]["gtn"]["quit_when_solved"] = False
    return cfg


@pytest.mark.timeout(600)
def test_gtn_master_eager_equals_graph_and_the_restatement(tmp_path, monkeypatch):
    from learning_environments_amd.agents.GTN import GTN_Master
    from learning_environments_amd.agents.nes_common import chain_keys
    from oracle import oracle as orc
    monkeypatch.chdir(tmp_path)
    cfg = _master_config()
    torch.manual_seed(0)
    a = GTN_Master(cfg, bohb_id=0, seed=9, graph=True)
    torch.manual_seed(0)
    b = GTN_Master(cfg, bohb_id=1, seed=9, graph=False)
    assert a.task.name == "ql_se" and a.use_graph and not b.use_graph and torch.equal(a.theta, b.theta) and a.p_theta == 6738
    for it in range(2):
        theta_before = b.theta.cpu().numpy().copy()
        ra, rb = a.step(it), b.step(it)
        assert ra == rb
        assert a.score_list == b.score_list and a.score_orig_list == b.score_orig_list
        assert torch.equal(a.theta, b.theta), it
        # the per-worker scores are the restatement's for the same noise and keys
        eps = b.eps.cpu().numpy()
        W = 8
        keys = chain_keys(b.seed, it, np.repeat(np.arange(W), 3), np.tile(np.arange(3), W))
        scores = np.zeros(3 * W)
        for c in range(3 * W):
            sg = (0.0, 1.0, -1.0)[c % 3]
            th = (np.float64(sg) * np.float64(eps[c // 3]) + np.float64(theta_before)).astype(np.float32)
            scores[c] = ql_se_ref.chain(b.cfg, th, b.task.tables, rng_key=int(keys[c]))["score"]
        best, _ = orc.worker_best(scores[1::3], scores[2::3], True)
        assert np.array_equal(np.array(b.score_orig_list), scores[0::3]) and np.array_equal(np.array(b.score_list), best)
    assert a.graph_replays == 2


FILE_SEED = 9          # the workers' seed = the fused master's: generation 0's score_orig chains then carry the same keys on both transports


def _worker_thread(id, errors, records):
    """A GTN_Worker that also records what each of its launches was given and returned."""
    try:
        from learning_environments_amd.agents.GTN import GTN_Worker
        w = GTN_Worker(id, bohb_id=-1, seed=FILE_SEED)
        run_chains = w._run_chains

        def recording(thetas):
            gen, counter = w.generation, w.test_counter
            scores = run_chains(thetas)
            records.append(dict(id=id, generation=gen, counter=counter, thetas=[t.cpu().numpy().copy() for t in thetas], scores=list(scores),
                                stats=w._inner[len(thetas)].stats.cpu().numpy().copy()))
            return scores
        w._run_chains = recording
        w.run()
    except Exception as e:  # noqa
        errors.append(e)


@pytest.mark.timeout(600)
def test_file_transport_with_two_workers(golden, tmp_path, monkeypatch):
    """This package's master <-> two GTN_Workers through the sync directory on the new task, on the fitted SE of fixture g15a.  Every chain a
    worker launched scores what the restatement scores for the parameters and the key the worker gave it; what the master read back is the
    worker's pick of those; and generation 0's score_orig equals the fused transport's for the same seed and theta."""
    from learning_environments_amd.agents.GTN import GTN_Master
    from learning_environments_amd.agents.nes_common import chain_keys, host_worker_best
    from learning_environments_amd.models.model_utils import linear_params
    monkeypatch.chdir(tmp_path)
    theta0 = _dev(golden("g15a_ql_se_cliff_ql")["theta"])
    cfg = _master_config(num_workers=2, max_iterations=2)
    cfg["agents"]["gtn"].update(mode="single", time_sleep_master=0.05, time_sleep_worker=0.1)
    fused = GTN_Master(cfg, bohb_id=1, seed=FILE_SEED, graph=False)
    fused.theta.copy_(theta0)
    fused.step(0)
    fused_orig = list(fused.score_orig_list)
    master = GTN_Master(cfg, bohb_id=-1, transport="file")
    master.theta.copy_(theta0)
    master.clean_working_dir()
    errors, records = [], []
    threads = [threading.Thread(target=_worker_thread, args=(i, errors, records), daemon=True) for i in range(2)]
    for t in threads:
        t.start()
    mean_score, mean_list, _ = master.run()
    for t in threads:
        t.join(timeout=120)
        assert not t.is_alive()
    assert errors == []
    assert len(mean_list) == 2 and np.isfinite(mean_score)
    assert sorted((r["id"], r["generation"]) for r in records) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    tables = fused.task.tables
    seen = set()
    for r in records:
        assert r["counter"] == r["generation"] and len(r["thetas"]) == 3
        keys = chain_keys(FILE_SEED, r["generation"] * 1000 + r["counter"], np.full(3, r["id"]), np.arange(3))
        refs = [ql_se_ref.chain(fused.cfg, r["thetas"][c], tables, rng_key=int(keys[c])) for c in range(3)]
        want = [o["score"] for o in refs]
        assert r["scores"] == want, (r["id"], r["generation"], r["scores"], want)
        # the Cliff's returns are coarse (-50, -100, ...): the chains' step counts tell the runs apart
        want_stats = [[o["episodes_run"], o["train_steps"], o["learn_steps"], o["test_steps"]] for o in refs]
        assert r["stats"].tolist() == want_stats, (r["id"], r["generation"], r["stats"].tolist(), want_stats)
        seen.update(o["train_steps"] for o in refs)
        if r["generation"] == 0:          # theta0 unperturbed under key (seed, 0, id, 0): the fused transport's score_orig chain
            assert np.array_equal(r["thetas"][0], theta0.cpu().numpy()) and r["scores"][0] == fused_orig[r["id"]]
        if r["generation"] == 1:          # what the master holds after run() is the last generation's
            best, _ = host_worker_best([r["scores"][1]], [r["scores"][2]], True, "mean")
            assert master.score_list[r["id"]] == best and master.score_orig_list[r["id"]] == r["scores"][0]
    assert len(seen) > 4                  # (the comparison is not one constant against itself)
    flat = torch.cat([p.detach().reshape(-1) for p in linear_params(master.synthetic_env_orig)])
    assert torch.equal(flat, master.theta) and master.p_theta == 6738
