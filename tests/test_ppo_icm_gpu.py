"""PPO with an Intrinsic Curiosity Module on the GPU: lenv_ppo_icm_inner_loop / _segment (ppo_icm_segment_kernel) against the CPU
restatement (tests/ppo_icm_ref.c) bit for bit -- on the G19 replays of the reference and on synthetic shapes --, every split of the episodes
into segments against the single launch, icm_eta = 0 against the ICM-less entry, the counter-RNG properties of a launch, and the transfer
experiment's mode -1 entry points.  Helpers and shapes are those of tests/test_ppo_gpu.py and tests/test_ppo_segments_gpu.py."""
import copy
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest
import torch

import ppo_icm_ref
import segments_common
from learning_environments_amd import _lib
from learning_environments_amd.agents.nes_common import linear_init_bounds
from learning_environments_amd.config import icm_layer_dims, ppo_cfg_from_config
from test_ppo_gpu import SMALL, bits, launch as launch_without_icm, make_cfg, make_inputs
from test_ppo_icm_reference import FIXTURES, replay

pytestmark = pytest.mark.gpu

OUT_NAMES = ("score", "stats", "status", "episode_test_mean", "episode_len", "final_returns", "final_params", "learn_step", "learn_params")
ICM_A = dict(feature_dim=8, hidden_size=16, lr=1e-3, beta=0.2, eta=0.5)
ICM_B = dict(feature_dim=5, hidden_size=24, lr=2e-3, beta=0.3, eta=0.5)
REC_N_ROWS = 7                                            # word of the resume record: rows waiting in the on-policy buffer


def icm_inputs(cfg, icm, chains, seed):
    """fresh modules per chain: nn.Linear's default init from a numpy generator"""
    bounds = linear_init_bounds(icm_layer_dims(cfg, icm["feature_dim"], icm["hidden_size"]))
    assert bounds.size == _lib.lib().lenv_ppo_icm_num_params(C.byref(cfg), icm["feature_dim"], icm["hidden_size"])
    rng = np.random.RandomState(seed)
    return ((rng.rand(chains, bounds.size) * 2 - 1) * bounds).astype(np.float32)


class Run(object):
    """One workload on the device: the inner loop's owner and the arguments every launch of a series gets."""

    def __init__(self, cfg, icm, chains, theta, eps, sign, init, icm_init, tapes=None, keys=None, trace_cap=0, learn_cap=0):
        from learning_environments_amd.engine import PpoIcmInnerLoop
        dev = torch.device("cuda")
        self.il = PpoIcmInnerLoop(cfg, chains, icm, want_episode_stats=True, want_final_params=True, trace_cap=trace_cap, learn_cap=learn_cap)
        self.il.icm_init.copy_(torch.from_numpy(np.ascontiguousarray(icm_init, np.float32).reshape(chains, -1)))
        self.names = OUT_NAMES if learn_cap else OUT_NAMES[:-2]
        self.pos = (torch.from_numpy(theta).to(dev), torch.from_numpy(eps).to(dev), torch.arange(chains, dtype=torch.int32, device=dev),
                    torch.from_numpy(sign).to(dev), torch.from_numpy(np.ascontiguousarray(init, np.float32).reshape(chains, -1)).to(dev))
        self.kw = dict(tapes={k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in tapes.items()} if tapes is not None else None,
                       rng_keys=torch.from_numpy(np.asarray(keys, np.uint64).view(np.int64)).to(dev) if keys is not None else None)

    def single(self):
        self.il.run(*self.pos, **self.kw)
        return self.snapshot()

    def split(self, ranges, between=None):
        segments_common.split(self.il, self.pos, self.kw, ranges, (), between=between)
        return self.snapshot()

    def snapshot(self):
        """every output, the trace arrays (trace_<name>) and icm_final"""
        if self.il.trace is None:                         # (built without a trace: segments_common.snapshot walks the dict)
            self.il.trace = {}
        return segments_common.snapshot(self.il, self.names)


def assert_chain_equals_restatement(cfg, icm, c, got, theta, eps, sign, init, icm_init, tapes=None, key=0, trace_cap=0, learn_cap=0):
    w = (np.float32(sign[c]) * eps[c] + theta).astype(np.float32) if sign[c] != 0 else theta      # fma(sign, eps, theta) with sign in {0, 1, -1}: exact
    tp = {k: v[c] for k, v in tapes.items()} if tapes is not None else None
    ref = ppo_icm_ref.chain(cfg, icm, icm_init[c], w, init[c], rng_key=key, tapes=tp, trace_cap=trace_cap, learn_cap=learn_cap)
    assert ref["rc"] == 0 and got["status"][c] == 0
    assert list(got["stats"][c]) == [ref["episodes_run"], ref["train_steps"], ref["learn_calls"], ref["test_steps"]]
    n = ref["trace"]["reward"].size
    if trace_cap:
        assert n == ref["train_steps"]                    # the capture covers the run
        for k in ("state", "action", "next_state", "reward", "done"):
            assert np.array_equal(bits(got["trace_" + k][c][:n]), bits(ref["trace"][k])), (k, c)
    if learn_cap:
        nl = ref["learn_step"].size
        assert nl == ref["learn_calls"] <= learn_cap and np.array_equal(got["learn_step"][c][:nl], ref["learn_step"])
        for i in range(nl):
            assert np.array_equal(bits(got["learn_params"][c][i]), bits(ref["learn_params"][i])), "parameters after learn call %d of chain %d" % (i, c)
    assert np.array_equal(got["episode_len"][c], ref["episode_len"])
    assert np.array_equal(bits(got["episode_test_mean"][c]), bits(ref["episode_test_mean"]))
    assert np.array_equal(bits(got["final_returns"][c]), bits(ref["final_returns"]))
    assert np.array_equal(bits(got["final_params"][c]), bits(ref["final_params"]))
    assert np.array_equal(bits(got["icm_final"][c]), bits(ref["icm_final"])), "the module after the run, chain %d" % c
    assert bits(np.array([got["score"][c]]))[0] == bits(np.array([ref["score"]]))[0]
    return ref


# ---- 1. kernel == restatement, bit for bit, in tape mode ----

@pytest.mark.parametrize("name", FIXTURES)
def test_kernel_equals_restatement_on_the_reference_replays(golden, name):
    g, cfg, icm, tapes, ref = replay(golden, name)
    assert cfg.train_episodes <= 6 and cfg.max_steps <= 50 and cfg.ppo_epochs <= 4
    tc, lc = g["tr_reward"].size + 4, g["learn_step"].size + 2
    theta = np.ascontiguousarray(g["theta"], np.float32)
    one = lambda a: np.ascontiguousarray(a)[None]         # noqa: E731
    got = Run(cfg, icm, 1, theta, np.zeros((1, theta.size), np.float32), np.zeros(1, np.float32), one(g["agent_init"]), one(g["icm_init"]),
              tapes={k: one(v) for k, v in tapes.items()}, trace_cap=tc, learn_cap=lc).single()
    out = assert_chain_equals_restatement(cfg, icm, 0, got, theta, np.zeros((1, theta.size), np.float32), np.zeros(1, np.float32),
                                          one(g["agent_init"]), one(g["icm_init"]), tapes={k: one(v) for k, v in tapes.items()}, trace_cap=tc,
                                          learn_cap=lc)
    assert np.array_equal(bits(out["icm_final"]), bits(ref["icm_final"])) and out["learn_calls"] == g["learn_step"].size


CASES = {
    # env, cfg, module, rows of a learn call
    "pendulum_28_rows_mid_episode": ("Pendulum-v0", dict(rtype=2, max_steps=11, ue=2.5, L=2, H=64), ICM_A, 28),
    "cmc_k5_13_rows_one_layer": ("MountainCarContinuous-v0", dict(rtype=1, k=5, max_steps=40, ue=1.5, L=1, H=64, act="tanh"), ICM_B, 13),
    "standin_a6_19_rows_type3": ("HalfCheetah-v3", dict(rtype=3, max_steps=9, ue=2.0, L=2, H=64, act="leakyrelu"), ICM_A, 19),
    "pendulum_151_rows": ("Pendulum-v0", dict(rtype=2, max_steps=50, ue=3.0, L=2, H=32, epochs=2, T=1), ICM_B, 151),
    # F + A = 134 inputs of the forward model: two column blocks in its weight gradients
    "standin_f128_h128_33_rows": ("HalfCheetah-v3", dict(rtype=2, max_steps=16, ue=2.0, L=1, H=64, epochs=2, T=1),
                                  dict(feature_dim=128, hidden_size=128, lr=1e-3, beta=0.2, eta=0.5), 33),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_restatement_in_tape_mode(name):
    """Three chains with different eps rows and signs (0, +1, -1) in one launch."""
    env, over, icm, rows = CASES[name]
    cfg = make_cfg(env, train_episodes=6, **over)
    assert _lib.lib().lenv_ppo_rows(C.byref(cfg)) == rows
    chains = 3
    theta, eps, sign, init, tapes = make_inputs(cfg, env, chains, seed=1900 + rows)
    icm_init = icm_inputs(cfg, icm, chains, seed=2900 + rows)
    assert sign.tolist() == [0.0, 1.0, -1.0]
    tc = 6 * -(-cfg.max_steps // max(1, cfg.same_action_num))
    got = Run(cfg, icm, chains, theta, eps, sign, init, icm_init, tapes=tapes, trace_cap=tc, learn_cap=6).single()
    assert got["status"].tolist() == [0] * chains
    for c in range(chains):
        ref = assert_chain_equals_restatement(cfg, icm, c, got, theta, eps, sign, init, icm_init, tapes=tapes, trace_cap=tc, learn_cap=6)
        assert ref["learn_calls"] >= (1 if rows == 151 else 2) and ref["train_steps"] > ref["learn_step"][0]
        assert not np.array_equal(ref["icm_final"], icm_init[c])
    assert not np.array_equal(got["icm_final"][0], got["icm_final"][1])


# ---- 2. segments ----

E = 6
SEG_CFG = dict(rtype=2, max_steps=10, ue=1.9, L=2, H=64)  # 20 rows per call = two whole episodes: learn calls behind episodes 1, 3 and 5


def compositions(n, parts):
    """every way to cut n episodes into `parts` consecutive launches, as [(begin, end), ...]"""
    for cuts in itertools.combinations(range(1, n), parts - 1):
        edges = (0,) + cuts + (n,)
        yield list(zip(edges[:-1], edges[1:]))


def test_every_split_equals_the_single_launch():
    """All 1 + 5 + 10 + 1 splits of 6 episodes into 1, 2, 3 and 6 launches.  Boundaries behind episodes 2 and 4 come directly after a learn
    call (no row waits), those behind episodes 1, 3 and 5 fall between two calls with 10 rows waiting (the record's n_rows word)."""
    cfg = make_cfg("Pendulum-v0", train_episodes=E, **SEG_CFG)
    chains = 3
    theta, eps, sign, init, tapes = make_inputs(cfg, "Pendulum-v0", chains, seed=2600)
    icm_init = icm_inputs(cfg, ICM_A, chains, seed=2601)
    mk = lambda: Run(cfg, ICM_A, chains, theta, eps, sign, init, icm_init, tapes=tapes, trace_cap=60, learn_cap=4)       # noqa: E731
    ref = mk().single()
    assert ref["status"].tolist() == [0] * chains and ref["learn_step"][:, :3].tolist() == [[20, 40, 60]] * chains
    assert_chain_equals_restatement(cfg, ICM_A, 1, ref, theta, eps, sign, init, icm_init, tapes=tapes, trace_cap=60, learn_cap=4)
    assert "icm_final" in ref and not np.array_equal(ref["icm_final"], icm_init)
    splits = [s for parts in (1, 2, 3, 6) for s in compositions(E, parts)]
    assert len(splits) == 17
    for ranges in splits:
        run, pending = mk(), []
        got = run.split(ranges, between=lambda il, b, e: pending.append(il.resume[:, REC_N_ROWS].cpu().tolist()))
        segments_common.same_bits(ref, got, ranges)
        finished, status = run.il.segment_state()
        assert finished.tolist() == [1] * chains and status.tolist() == [0] * chains, ranges
        assert [p[0] for p in pending[:-1]] == [10 if e % 2 else 0 for _, e in ranges[:-1]], ranges
        # the module's Adam powers travel in words 22..23 of the record: three steps by the end (the agent's: 3 calls x 3 epochs)
        rec = run.il.resume.cpu().numpy()
        assert np.ascontiguousarray(rec[:, 22:24]).view(np.float64).tolist() == [[1.0 * 0.9 * 0.9 * 0.9, 1.0 * 0.999 * 0.999 * 0.999]] * chains
        assert (rec[:, 24:] == 0).all()


def test_splits_on_the_standin_with_a_mid_episode_call():
    """19 rows per call on 9-step episodes: a partly filled row buffer at every boundary, next observations carried across it."""
    env, over, icm, rows = CASES["standin_a6_19_rows_type3"]
    cfg = make_cfg(env, train_episodes=E, **over)
    theta, eps, sign, init, tapes = make_inputs(cfg, env, 2, seed=2610)
    icm_init = icm_inputs(cfg, icm, 2, seed=2611)
    mk = lambda: Run(cfg, icm, 2, theta, eps, sign, init, icm_init, tapes=tapes, trace_cap=54, learn_cap=4)       # noqa: E731
    ref = mk().single()
    assert ref["status"].tolist() == [0, 0] and ref["learn_step"][:, :2].tolist() == [[19, 38]] * 2
    for ranges in ([(0, 2), (2, 6)], [(0, 3), (3, 4), (4, 6)], [(i, i + 1) for i in range(E)]):
        segments_common.same_bits(ref, mk().split(ranges), ranges)


def test_early_out_in_a_middle_segment():
    """solved_reward -1e9 with one init episode: every chain leaves behind its second episode.  With one episode per launch the closing
    outputs, icm_final among them, appear in the second segment; a further segment leaves everything as it is."""
    cfg = make_cfg("Pendulum-v0", train_episodes=E, solved_reward=-1e9, init_episodes=1, early_out_num=2, **SEG_CFG)
    chains = 3
    theta, eps, sign, init, tapes = make_inputs(cfg, "Pendulum-v0", chains, seed=2620)
    icm_init = icm_inputs(cfg, ICM_A, chains, seed=2621)
    mk = lambda: Run(cfg, ICM_A, chains, theta, eps, sign, init, icm_init, tapes=tapes, trace_cap=60, learn_cap=4)       # noqa: E731
    ref = mk().single()
    assert ref["stats"][:, 0].tolist() == [2] * chains and np.isnan(ref["episode_test_mean"][:, 2:]).all() and ref["stats"][:, 2].tolist() == [1] * chains
    run, calls, seen = mk(), [], []
    run.il.score.fill_(-7.0)
    run.il.icm_final.fill_(-7.0)

    def on_segment(done, fin):
        calls.append((done, fin))
        seen.append(run.snapshot())
    run.il.run(*run.pos, episodes_per_launch=1, on_segment=on_segment, **run.kw)
    assert calls == [(1, 0), (2, chains)]
    # the unfinished segment: a checkpoint of the module (still the fresh one: no learn call yet), nothing of the closing part
    assert (seen[0]["score"] == -7.0).all() and np.array_equal(bits(seen[0]["icm_final"]), bits(icm_init))
    segments_common.same_bits(ref, seen[-1], "the segment of the early out")
    before, rec = run.snapshot(), run.il.resume.cpu().numpy().copy()
    run.il.run_segment(*run.pos, 2, 3, **run.kw)
    segments_common.same_bits(before, run.snapshot(), "a segment behind the end")
    assert np.array_equal(run.il.resume.cpu().numpy(), rec)


# ---- 3. icm_eta = 0: the agent of the ICM-less entry ----

@pytest.mark.parametrize("name", ["pendulum_28_rows_mid_episode", "cmc_k5_13_rows_one_layer", "standin_a6_19_rows_type3"])
def test_eta_zero_leaves_the_agent_of_the_entry_without_icm(name):
    env, over, icm, rows = CASES[name]
    cfg = make_cfg(env, train_episodes=6, **over)
    chains = 3
    theta, eps, sign, init, tapes = make_inputs(cfg, env, chains, seed=3000 + rows)
    icm_init = icm_inputs(cfg, icm, chains, seed=3100 + rows)
    tc = 6 * -(-cfg.max_steps // max(1, cfg.same_action_num))
    plain = launch_without_icm(cfg, chains, theta, eps, sign, init, tapes=tapes, trace_cap=tc, learn_cap=6)
    got = Run(cfg, dict(icm, eta=0.0), chains, theta, eps, sign, init, icm_init, tapes=tapes, trace_cap=tc, learn_cap=6).single()
    assert got["status"].tolist() == [0] * chains and (got["stats"][:, 2] >= 2).all()
    for k in OUT_NAMES:
        assert got[k].tobytes() == plain[k].tobytes(), k
    for k, v in plain["trace"].items():
        assert got["trace_" + k].tobytes() == v.tobytes(), k
    assert not np.array_equal(got["icm_final"], icm_init)         # ... while the module trained
    with_eta = Run(cfg, icm, chains, theta, eps, sign, init, icm_init, tapes=tapes, trace_cap=tc, learn_cap=6).single()
    assert with_eta["learn_params"].tobytes() != plain["learn_params"].tobytes()


# ---- 4. counter-RNG mode ----

def test_counter_rng_mode():
    env = "MountainCarContinuous-v0"
    cfg = make_cfg(env, rtype=2, rng_mode=_lib.RNG_COUNTER, k=5, max_steps=20, ue=1.5, H=64)
    chains = 6
    theta, eps, sign, init, _ = make_inputs(cfg, env, chains, seed=5)
    init[:] = init[0]
    eps[:] = 0
    icm_init = icm_inputs(cfg, ICM_A, chains, seed=6)
    icm_init[:] = icm_init[0]                              # the same fresh agent and module everywhere: only the keys tell the chains apart
    keys = np.array([_lib.lib().lenv_chain_key(19, 0, c, 0) for c in range(chains)], np.uint64)
    mk = lambda k: Run(cfg, ICM_A, chains, theta, eps, sign, init, icm_init, keys=k, learn_cap=4)       # noqa: E731
    a, b = mk(keys).single(), mk(keys).single()
    assert a["status"].tolist() == [0] * chains
    segments_common.same_bits(a, b, "two identical launches")
    assert len(set(a["score"].tolist())) == chains and len(set(a["icm_final"][i].tobytes() for i in range(chains))) == chains
    other = mk(keys[::-1].copy()).single()
    assert np.array_equal(bits(other["score"][::-1]), bits(a["score"])) and not np.array_equal(other["score"], a["score"])
    assert np.array_equal(bits(other["icm_final"][::-1]), bits(a["icm_final"]))
    for c in (0, 5):
        assert_chain_equals_restatement(cfg, ICM_A, c, a, theta, eps, sign, init, icm_init, key=int(keys[c]), learn_cap=4)


def _real_env(cfg, seed):
    from learning_environments_amd.envs.env_factory import EnvFactory
    torch.manual_seed(seed)
    return EnvFactory(copy.deepcopy(cfg)).generate_real_env()


def test_train_test_agents_icm_equals_single_chain_launches():
    from learning_environments_amd.experiments import transfer_algo as ta
    env_name = "MountainCarContinuous-v0"
    base = ta.base_config(env_name)
    base["envs"][env_name].update(max_steps=60, hidden_size=32)
    real_env = _real_env(base, 1)
    cfg = copy.deepcopy(base)
    small_icm = dict(feature_dim=8, hidden_size=16)
    (rewards, lengths), last = ta.train_test_agents_icm(real_env, cfg, env_name, agents_num=3, seed=9, settings=SMALL, icm=small_icm, details=True)
    assert cfg["agents"]["icm"] == dict(ta.ICM_SETTINGS[env_name], **small_icm) and cfg["agents"]["ppo"]["same_action_num"] == 5
    assert len(rewards) == len(lengths) == 3 and all(len(r) == 3 and np.isfinite(r).all() for r in rewards) and all(sum(l) > 0 for l in lengths)
    inner = last["inner"]
    pcfg, icm = last["task"].cfg, inner.icm_settings
    assert pcfg.reward_env_type == 0 and icm == dict(feature_dim=8, hidden_size=16, lr=5e-4, beta=0.1, eta=0.01)
    init, icm_init = last["agent_init"].cpu().numpy(), inner.icm_init.cpu().numpy()
    assert len(set(icm_init[i].tobytes() for i in range(3))) == 3 and np.abs(icm_init).max() > 0       # every agent drew a module of its own
    z1 = np.zeros((1, 1), np.float32)
    for i in range(3):
        one = Run(pcfg, icm, 1, np.zeros(1, np.float32), z1, np.zeros(1, np.float32), init[i:i + 1], icm_init[i:i + 1], keys=last["keys"][i:i + 1]).single()
        n = int(one["stats"][0, 0])
        assert one["episode_test_mean"][0][:n].tolist() == rewards[i] and one["episode_len"][0][:n].tolist() == lengths[i]
        assert np.array_equal(bits(one["icm_final"][0]), bits(inner.icm_final[i].cpu().numpy()))
    # segments give the same results; another model index other agents
    again = ta.train_test_agents_icm(real_env, copy.deepcopy(base), env_name, agents_num=3, seed=9, settings=SMALL, icm=small_icm, episodes_per_launch=2)
    assert again == (rewards, lengths)
    other = ta.train_test_agents_icm(real_env, copy.deepcopy(base), env_name, agents_num=3, seed=9, model_index=1, settings=SMALL, icm=small_icm)
    assert other != (rewards, lengths)


def test_train_test_agents_icm_replays_a_recorded_run(golden):
    """replay=: the recorded agent, module and draws of g19c in tape mode give the restatement's run of that fixture."""
    from learning_environments_amd.experiments import transfer_algo as ta
    g, _, icm, tapes, _ = replay(golden, "g19c_ppo_icm_cmc_type5_k5")
    config = json.loads(str(g["config_json"]))
    env_name = config["env_name"]
    config["envs"][env_name]["reward_env_type"] = 0         # the driver trains on the real env: only the settings and draws are replayed
    plain = copy.deepcopy(config)
    rec = dict(agent_init=[g["agent_init"]], icm_init=[g["icm_init"]], tapes=[tapes])
    rewards, lengths = ta.train_test_agents_icm(_real_env(plain, 1), config, env_name, agents_num=1, settings=dict(config["agents"]["ppo"]),
                                                icm=dict(config["agents"]["icm"]), replay=rec)
    want = ppo_icm_ref.chain(ppo_cfg_from_config(config, rng_mode=_lib.RNG_TAPE), icm, g["icm_init"], None, g["agent_init"], tapes=tapes)
    assert rewards[0] == want["episode_test_mean"].tolist() and lengths[0] == want["episode_len"].tolist()


def test_eval_icm_on_a_reference_written_checkpoint(tmp_path):
    from learning_environments_amd.experiments import transfer_algo as ta
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ckpt_cmc_reward_env_reference.pt")
    settings = dict(train_episodes=2, update_episodes=1, ppo_epochs=2)
    calls = []
    reward_list, length_list = ta.eval_icm(path, model_num=2, agents_num=2, settings=settings, icm=dict(feature_dim=8, hidden_size=16),
                                           episodes_per_launch=1, on_segment=lambda done, fin: calls.append((done, fin)), save_dir=str(tmp_path))
    assert calls == [(1, 0), (2, 4)] and len(reward_list) == len(length_list) == 4
    assert all(len(r) == 2 and np.isfinite(r).all() for r in reward_list) and all(sum(l) > 0 for l in length_list)
    saved = torch.load(os.path.join(str(tmp_path), "best_transfer_algo-1.pt"))
    assert saved["reward_list"] == reward_list and saved["model_num"] == 2 and saved["model_agents"] == 2
    assert saved["config"]["agents"]["icm"] == dict(ta.ICM_SETTINGS["MountainCarContinuous-v0"], feature_dim=8, hidden_size=16)
    # without overrides the block the driver leaves is the script's own
    _, real_env, config = ta.load_envs_and_config(path)
    per_model = [ta.train_test_agents_icm(real_env, copy.deepcopy(config), agents_num=2, model_index=m, settings=settings,
                                          icm=dict(feature_dim=8, hidden_size=16)) for m in range(2)]
    assert reward_list == per_model[0][0] + per_model[1][0] and length_list == per_model[0][1] + per_model[1][1]
    ta.train_test_agents_icm(real_env, config, agents_num=1, settings=dict(settings, train_episodes=1))
    assert config["agents"]["icm"] == ta.ICM_SETTINGS["MountainCarContinuous-v0"]
    with pytest.raises(NotImplementedError, match="ppo_icm"):
        ta.eval_base("-1", path)
