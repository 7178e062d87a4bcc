"""lenv_dueling_se_inner_loop_segment: the DDQN / DuelingDDQN inner loop in episode segments.

Bar: for every split of the episodes the launches leave every output array, the step trace, final_online and icm_final BIT-EQUAL to the
single launch of lenv_dueling_se_inner_loop_hp / _icm on the generic GEMM-queue kernel, which in turn is bit-equal to the CPU oracle.

The workload: the real CartPole (S 4, A 2) behind a RewardEnv of type 2 with a 4-16-1 tanh reward net; six chains with their own
hyper-parameters (hidden 8 / 24 / 40 and one chain at 136 -- a layer wider than 128 runs as two column blocks --, 1 / 2 hidden layers, batch
8 / 20, two learning rates); max_steps 12, so episodes end on the pole's own `done` and are uneven; 7 training episodes of which 2 are init
episodes; rb_size 40 (the ring wraps before the later boundaries); eps_decay 0.9 (epsilon crosses every boundary); 2 test episodes.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from segments_common import SENTINEL, _poison_finished, same_bits as _same_bits, single, snapshot, split  # noqa: E402
from test_gpu_parity import _inner_cfg, _lib_cfg_copy, dev, eng, orc  # noqa: E402,F401  (cfg helpers and fixtures)

pytestmark = pytest.mark.gpu

HPS = [dict(lr=1e-3, batch_size=8, hidden_size=8, hidden_layer=1), dict(lr=2e-3, batch_size=20, hidden_size=24, hidden_layer=2),
       dict(lr=1e-3, batch_size=20, hidden_size=40, hidden_layer=1), dict(lr=2e-3, batch_size=8, hidden_size=136, hidden_layer=2),
       dict(lr=1e-3, batch_size=8, hidden_size=24, hidden_layer=2), dict(lr=2e-3, batch_size=20, hidden_size=8, hidden_layer=1)]
CHAINS = len(HPS)
EPISODES, INIT, MAX_STEPS, T, RB = 7, 2, 12, 2, 40
CAP = EPISODES * MAX_STEPS + 4                             # trace rows: the whole run
SPLITS = ([(0, 7)], [(0, 3), (3, 4), (4, 7)], [(0, 1), (1, 7)])
SE_HIDDEN = 16
OUT_NAMES = ("score", "stats", "status", "episode_test_mean", "episode_len", "final_returns", "final_online")


def _snapshot(il):
    return snapshot(il, OUT_NAMES)


def _config(family, icm, virtual, agent_over, solved):
    from learning_environments_amd import configs
    cfgd = configs.cartpole_reward_env_ddqn()
    agent = dict(cfgd["agents"]["ddqn"], train_episodes=EPISODES, init_episodes=INIT, test_episodes=T, rb_size=RB, eps_init=1.0, eps_min=0.05,
                 eps_decay=0.9, early_out_num=50, batch_size=20, hidden_size=136, hidden_layer=2, activation_fn="relu", feature_dim=16)
    agent.update(agent_over)
    cfgd["agents"] = {"gtn": dict(cfgd["agents"]["gtn"], agent_name=family + ("_icm" if icm else "") + "_vary", synthetic_env_type=0 if virtual else 1),
                      family: agent, "icm": {"lr": 1e-3, "beta": 0.2, "eta": 0.5, "feature_dim": 8, "hidden_size": 16}}
    cfgd["envs"]["CartPole-v0"].update(max_steps=MAX_STEPS, hidden_size=SE_HIDDEN, hidden_layer=1, activation_fn="tanh", reward_env_type=2,
                                       solved_reward=solved)
    return cfgd


class Case(object):
    """One workload: the cfgs (the launch's, with the maxima, and every chain's own for the oracle), inputs, tapes."""

    def __init__(self, orc, tape=False, family="ddqn", icm=False, virtual=False, test_mode=0, solved=1e9, key_seed=59, **agent_over):
        from learning_environments_amd.config import agent_layer_dims
        self.tape, self.icm, self.virtual = tape, icm, virtual
        cfgd = _config(family, icm, virtual, agent_over, solved)
        common = dict(grad_chunk=0, rng_mode=1 if tape else 0, test_mode=test_mode)
        _, self.cfg = _inner_cfg(orc, cfgd, **common)
        assert self.cfg.icm_enabled == int(icm) and self.cfg.synthetic_env_type == int(not virtual) and self.cfg.test_mode == test_mode
        assert self.cfg.agent_kind == int(family == "duelingddqn") and self.cfg.q_hidden == 136 and self.cfg.q_layers == 2
        if virtual:
            P_se = sum(orc.mlp_num_params(d) for d in orc.se_descs(4, 2, SE_HIDDEN, 1, "tanh"))
        else:
            P_se = orc.mlp_num_params(orc.mlp_desc(4, SE_HIDDEN, 1, 1, "tanh"))
        rng = np.random.RandomState(211 + 2 * int(virtual) + int(icm))
        self.theta = (rng.randn(P_se) * 0.3).astype(np.float32)
        self.eps = (rng.randn(2, P_se) * 0.05).astype(np.float32)
        self.worker = (np.arange(CHAINS) % 2).astype(np.int32)
        self.sign = np.array([0.0, 1.0, -1.0, 1.0, -1.0, 0.0], np.float32)
        self.keys = np.array([orc.chain_key(key_seed, 4, int(self.worker[c]), c) for c in range(CHAINS)], np.uint64)
        self.ocfgs, self.inits, self.icm_inits = [], [], []
        for c, h in enumerate(HPS):
            oc = orc.ddqn_cfg_from_config(cfgd, **common, **orc.hp_overrides(h))
            self.ocfgs.append(oc)
            self.inits.append(orc.agent_init_from_key(int(self.keys[c]), agent_layer_dims(_lib_cfg_copy(oc))))
            self.icm_inits.append(orc.agent_init_from_key(int(self.keys[c]), orc.icm_layer_dims(oc), stream=orc.STREAM_ICM_INIT) if icm else None)
        self.tapes = None
        if tape:
            steps, learn = EPISODES * MAX_STEPS, (EPISODES - INIT) * MAX_STEPS
            idx = np.zeros((CHAINS, learn * 20), np.int32)
            for c, h in enumerate(HPS):
                B = h["batch_size"]
                for j in range(learn):
                    size = min(INIT + j + 1, RB)        # rows in the buffer at learn step j: at least one per init episode, one per learn step
                    idx[c, j * B:(j + 1) * B] = rng.randint(0, size, B)
            self.tapes = dict(eps_uniform=rng.uniform(0, 1, (CHAINS, steps)), rand_action=rng.randint(0, 2, (CHAINS, steps)).astype(np.int32),
                              replay_idx=idx, train_reset=rng.uniform(-0.1, 0.1, (CHAINS, EPISODES, 4)),
                              test_reset=rng.uniform(-0.1, 0.1, (CHAINS, (EPISODES + 1) * T, 4)))

    def oracle(self, orc, c):
        w = (np.float32(self.sign[c]) * self.eps[self.worker[c]] + self.theta).astype(np.float32)
        tapes = None
        if self.tape:
            t = self.tapes
            tapes = orc.make_tapes(t["eps_uniform"][c], t["rand_action"][c], t["replay_idx"][c], t["train_reset"][c], t["test_reset"][c])
        if self.icm:
            return orc.ddqn_se_chain(self.ocfgs[c], w, self.inits[c], rng_key=int(self.keys[c]), tapes=tapes, trace_cap=CAP, icm_init=self.icm_inits[c])
        return orc.ddqn_se_chain(self.ocfgs[c], w, self.inits[c], rng_key=int(self.keys[c]), tapes=tapes, trace_cap=CAP, want_final_online=True)

    def inner(self, eng, segments=True):
        il = eng.InnerLoop(self.cfg, CHAINS, trace_cap=CAP, want_episode_stats=True, want_final_online=True, vary=True, segments=segments)
        il.set_hp([h["lr"] for h in HPS], [h["batch_size"] for h in HPS], [h["hidden_size"] for h in HPS], [h["hidden_layer"] for h in HPS])
        init = np.full((CHAINS, il.p_agent), np.nan, np.float32)        # (behind a chain's own parameters: never read)
        for c, w in enumerate(self.inits):
            init[c, :w.size] = w
        il.agent_init.copy_(dev(init))
        if self.icm:
            il.icm_init.copy_(dev(np.stack(self.icm_inits)))
        return il

    def args(self):
        """(positional arguments of run / run_segment up to agent_init, keyword arguments)"""
        kw = dict(tapes={k: dev(v) for k, v in self.tapes.items()}) if self.tape else dict(rng_keys=dev(self.keys.view(np.int64)))
        return (dev(self.theta), dev(self.eps), dev(self.worker), dev(self.sign), None), kw

    def single(self, eng):
        il = self.inner(eng, segments=False)             # lenv_dueling_se_inner_loop_icm (hp given: the generic kernel)
        return il, single(il, *self.args(), OUT_NAMES)

    def split(self, eng, segments, between=None):
        il = self.inner(eng)
        return il, split(il, *self.args(), segments, OUT_NAMES, between=between)


def _check_vs_oracle(case, orc, snap, oracles=None):
    for c in range(CHAINS):
        o = oracles[c] if oracles else case.oracle(orc, c)
        assert o["rc"] == 0 and o["learn_steps"] > 0, c
        n = o["trace"]["action"].size
        act = snap["trace_action"][c, :n]
        assert np.array_equal(act & 0xFFFF, o["trace"]["action"]) and np.array_equal(act >> 16, o["trace"]["explored"]), c
        assert np.array_equal(snap["trace_state"][c, :n], o["trace"]["state"]), c
        assert np.array_equal(snap["trace_next_state"][c, :n], o["trace"]["next_state"]), c
        assert np.array_equal(snap["trace_reward_done"][c, :n, 0], o["trace"]["reward"]), c
        assert np.array_equal(snap["trace_reward_done"][c, :n, 1], o["trace"]["done"]), c
        assert np.array_equal(snap["episode_test_mean"][c], o["episode_test_mean"], equal_nan=True), c
        assert np.array_equal(snap["episode_len"][c], o["episode_len"]), c
        assert np.array_equal(snap["final_returns"][c], o["final_test_returns"]), c
        assert float(snap["score"][c]) == o["score"], c
        assert snap["stats"][c].tolist() == [o["episodes_run"], o["train_steps"], o["learn_steps"], o["test_steps"]], c
        if case.icm:
            assert np.array_equal(snap["icm_final"][c], o["icm_final"]), c
        else:
            assert np.array_equal(snap["final_online"][c, :o["final_online"].size], o["final_online"]), c


CASES = {"plain_counter": dict(), "tape": dict(tape=True), "dueling": dict(family="duelingddqn"), "icm": dict(icm=True),
         "dueling_icm_tape": dict(family="duelingddqn", icm=True, tape=True), "virtual_env": dict(virtual=True), "test_mode_1": dict(test_mode=1),
         "virtual_env_test_mode_1": dict(virtual=True, test_mode=1)}


@pytest.mark.parametrize("name", list(CASES))
def test_every_split_equals_the_single_launch_and_the_oracle(eng, orc, name):
    case = Case(orc, **CASES[name])
    il, ref = case.single(eng)
    assert ref["status"].tolist() == [0] * CHAINS
    _check_vs_oracle(case, orc, ref)
    if not case.virtual:
        lens = ref["episode_len"]
        assert lens.min() < MAX_STEPS and len(set(lens.reshape(-1).tolist())) > 1          # the pole's own done: uneven episodes
        assert (ref["stats"][:, 1] > RB).all()                                             # the ring of 40 rows wrapped
    for segments in SPLITS:
        il2, got = case.split(eng, segments)
        _same_bits(ref, got, segments)
        finished, status = il2.segment_state()
        assert finished.tolist() == [1] * CHAINS and status.tolist() == [0] * CHAINS, segments
        rec = il2.resume.cpu().numpy()
        assert np.array_equal(rec[:, 7], ref["stats"][:, 1]) and np.array_equal(rec[:, 10], rec[:, 7]) and not rec[:, 16:].any()


# chain keys of the early-out case: with this seed the oracle's means (computed in the test, on the CPU) leave a solved_reward for which chains
# leave in episode 2, in episode 3 (the middle segment), in episode 5, and never
EARLY_KEY_SEED = 66


def test_early_out_chains_finish_in_the_middle_segment_and_stay_untouched(eng, orc):
    """early_out_num 1: a chain leaves at the first learning episode whose test mean reaches solved_reward.  solved_reward is chosen here, on
    the CPU, between the oracle's per-episode means of a run without early out: chains whose episode-3 mean reaches it while their
    episode-2 mean does not leave inside the middle segment [3, 4); chains that never reach it run all seven episodes."""
    free = Case(orc, icm=True, early_out_num=1, key_seed=EARLY_KEY_SEED)
    means = np.stack([free.oracle(orc, c)["episode_test_mean"] for c in range(CHAINS)])           # [chains, 7], no early out (solved 1e9)
    assert not np.isnan(means).any()
    learn = means[:, INIT:]
    # candidates: midpoints between the distinct values of the learning episodes' means; keep one for which some chain first reaches it in
    # episode 3 and another never does
    vals = np.unique(learn)
    pick = None
    for s in (vals[:-1] + vals[1:]) / 2:
        first = np.array([np.argmax(row >= s) + INIT if (row >= s).any() else -1 for row in learn])
        if (first == 3).any() and (first == -1).any():
            pick = (float(s), first)
            break
    assert pick is not None, means.tolist()
    solved, first = pick
    case = Case(orc, icm=True, early_out_num=1, solved=solved, key_seed=EARLY_KEY_SEED)
    il, ref = case.single(eng)
    assert ref["status"].tolist() == [0] * CHAINS
    episodes_run = ref["stats"][:, 0]
    middle, never = np.flatnonzero(first == 3), np.flatnonzero(first == -1)
    assert episodes_run.tolist() == [f + 1 if f >= 0 else EPISODES for f in first.tolist()], (episodes_run.tolist(), first.tolist())
    _check_vs_oracle(case, orc, ref)
    names = OUT_NAMES + ("icm_final",)
    segments = SPLITS[1]
    hook, seen = _poison_finished(names)
    il2, got = case.split(eng, segments, between=hook)
    assert sorted(seen) == list(range(CHAINS))                               # every chain finished at some boundary
    for c in range(CHAINS):
        for k in names:
            assert np.all(got[k][c] == SENTINEL), (c, k)                     # ... and nothing wrote its outputs afterwards
            assert seen[c][k].tobytes() == ref[k][c].tobytes(), (c, k)
    for k in got:
        if k.startswith("trace_"):
            assert got[k].tobytes() == ref[k].tobytes(), k
    states = []
    case.split(eng, segments[:2], between=lambda il_, b, e: states.append(il_.segment_state()[0].numpy().copy()))
    assert not states[0][middle].any() and states[1][middle].all() and not states[1][never].any()
    _same_bits(ref, case.split(eng, SPLITS[2])[1], SPLITS[2])


def test_step_budget_that_expires_in_a_later_segment(eng, orc):
    """The check in front of an episode compares the env steps so far (training + tests) with step_budget.  An episode takes at most
    12 + 2 * 12 = 36 env steps, so two episodes stay within a budget of 80 and every chain runs episode 2; CartPole cannot fall in fewer than
    8 steps, so an episode takes at least 24 and four exceed 80: every chain times out in front of episode 3 or 4 -- behind the first
    boundary of both splits, in the segment [3, 4) or [4, 7) of the first and in the second segment of the other."""
    case = Case(orc, step_budget=80)
    il, ref = case.single(eng)
    assert ref["status"].tolist() == [0] * CHAINS
    run = ref["stats"][:, 0]
    assert (run >= 3).all() and (run <= 4).all(), run.tolist()
    assert not np.isnan(ref["episode_test_mean"]).any()                      # time_is_up's padding
    _check_vs_oracle(case, orc, ref)
    for segments in SPLITS[1:]:
        hook, seen = _poison_finished(OUT_NAMES)
        il2, got = case.split(eng, segments, between=hook)
        for c in range(CHAINS):
            for k in OUT_NAMES:
                assert np.all(got[k][c] == SENTINEL), (segments, c, k)
                assert seen[c][k].tobytes() == ref[k][c].tobytes(), (segments, c, k)
        first = []
        case.split(eng, segments[:1], between=lambda il_, b, e: first.append(il_.segment_state()[0].tolist()))
        assert first == [[0] * CHAINS], segments                             # no chain is finished behind the first segment


def test_refusals_and_a_record_that_names_another_episode(eng, orc):
    import ctypes as C
    from learning_environments_amd import _lib
    case = Case(orc)
    il = case.inner(eng)
    pos, kw = case.args()
    il.resume = torch.full((CHAINS, _lib.DUELING_RESUME_WORDS), 5, dtype=torch.int64, device=il.dev)
    before = _snapshot(il)
    args = il._run_args(*pos[:4], il.agent_init, kw["rng_keys"], None)

    def launch(b, e, resume):
        return _lib.lib().lenv_dueling_se_inner_loop_segment(C.byref(il.cfg), il._hp_arg(), None, *args[:-1], b, e, resume, args[-1])
    res = C.c_void_p(il.resume.data_ptr())
    for b, e, r in ((3, 3, res), (4, 3, res), (-1, 2, res), (0, EPISODES + 1, res), (EPISODES, EPISODES + 1, res), (0, EPISODES, None)):
        assert launch(b, e, r) == -1, (b, e)                                 # LENV_ERR_INVALID
    with pytest.raises(ValueError):
        il.run_segment(*pos, 2, 2, **kw)
    with pytest.raises(ValueError):
        il.run(*pos, episodes_per_launch=0, **kw)
    with pytest.raises(ValueError):                                          # an inner loop that was not built for segments
        case.inner(eng, segments=False).run_segment(*pos, 0, 3, **kw)
    _same_bits(before, _snapshot(il), "refused launches")                    # none reached the device
    assert il.resume.cpu().unique().tolist() == [5]

    # a continuation from the wrong episode: status -10 per chain, nothing else
    il, _ = case.split(eng, [(0, 3)])
    before, rec = _snapshot(il), il.resume.cpu().numpy().copy()
    assert rec[:, 0].tolist() == [3] * CHAINS and rec[:, 1].tolist() == [0] * CHAINS
    il.run_segment(*pos, 4, EPISODES, **kw)
    after = _snapshot(il)
    assert after.pop("status").tolist() == [-10] * CHAINS and before.pop("status").tolist() == [0] * CHAINS
    _same_bits(before, after, "wrong episode_begin")
    assert np.array_equal(il.resume.cpu().numpy(), rec)
    assert il.segment_state()[1].tolist() == [-10] * CHAINS


def test_run_with_episodes_per_launch(eng, orc):
    """InnerLoop.run(episodes_per_launch=n): the same outputs as the single launch; on_segment sees the progress; the series stops when
    every chain is finished."""
    case = Case(orc, family="duelingddqn")
    _, ref = case.single(eng)
    pos, kw = case.args()
    for n, want in ((1, [(e, 0) for e in range(1, EPISODES)] + [(EPISODES, CHAINS)]), (3, [(3, 0), (6, 0), (7, CHAINS)]), (50, [(7, CHAINS)])):
        il, calls = case.inner(eng), []
        il.run(*pos, episodes_per_launch=n, on_segment=lambda done, fin: calls.append((done, fin)), **kw)
        assert calls == want, n
        _same_bits(ref, _snapshot(il), n)
    # every chain leaves at the first learning episode: three launches of one episode, then the series is over
    case = Case(orc, solved=-1e9, early_out_num=1)
    _, ref = case.single(eng)
    assert ref["stats"][:, 0].tolist() == [3] * CHAINS
    il, calls = case.inner(eng), []
    il.run(*case.args()[0], episodes_per_launch=1, on_segment=lambda done, fin: calls.append((done, fin)), **case.args()[1])
    assert calls == [(1, 0), (2, 0), (3, CHAINS)]
    _same_bits(ref, _snapshot(il), "early out")
    # a bad chain status ends the series like check_status: a replay-index tape that runs out in the first learning episode
    case = Case(orc, tape=True)
    case.tapes["replay_idx"] = case.tapes["replay_idx"][:, :30]
    il, calls = case.inner(eng), []
    from learning_environments_amd import _lib
    with pytest.raises(_lib.LenvError):
        il.run(*case.args()[0], episodes_per_launch=3, on_segment=lambda done, fin: calls.append((done, fin)), **case.args()[1])
    assert calls == [(3, 0)] and il.status.cpu().tolist() == [-4] * CHAINS
