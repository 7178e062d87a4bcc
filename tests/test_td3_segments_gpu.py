"""lenv_td3_rn_inner_loop_segment: the TD3 inner loop in episode segments.

Bar: for every split of the episodes the launches leave every output array, the step trace, final_params and icm_final BIT-EQUAL to the
single launch of lenv_td3_rn_inner_loop_hp / _icm on the generic GEMM-queue kernel, which in turn is bit-equal to the CPU oracle (the
comparison helper of tests/test_gpu_parity.py).

The workload: Pendulum-v0 (S 3, A 1), six chains with their own hyper-parameters (hidden 8 / 24 / 40, 1 / 2 / 3 hidden layers, batch 8 / 20,
two learning rates), max_steps 12 at same_action_num 2 (six agent steps per episode), 7 training episodes of which 2 are init episodes,
rb_size 40 (a ring of min(7 * 12, 40) rows: the 42 agent steps of a full run wrap it), policy_delay 2 (30 learn steps: the parity of learn_it
crosses the boundaries), 2 test episodes.  The splits put one boundary inside the init episodes and the others behind them.  One test adds a
ring of 16 rows, which has wrapped before the boundaries at episodes 3 and 4.
"""
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from segments_common import SENTINEL, _poison_finished, same_bits as _same_bits, single, snapshot, split  # noqa: E402
from test_gpu_parity import _td3_cfgs, _td3_compare, dev, eng, orc  # noqa: E402,F401  (the oracle comparison helper and its fixtures)

pytestmark = pytest.mark.gpu

ENV = "Pendulum-v0"
HPS = [dict(lr=1e-3, batch_size=8, hidden_size=8, hidden_layer=1), dict(lr=2e-3, batch_size=20, hidden_size=24, hidden_layer=2),
       dict(lr=1e-3, batch_size=20, hidden_size=40, hidden_layer=3), dict(lr=2e-3, batch_size=8, hidden_size=40, hidden_layer=1),
       dict(lr=1e-3, batch_size=8, hidden_size=24, hidden_layer=3), dict(lr=2e-3, batch_size=20, hidden_size=8, hidden_layer=2)]
CHAINS = len(HPS)
EPISODES, INIT, MAX_STEPS, K, T, RB = 7, 2, 12, 2, 2, 40
STEPS = MAX_STEPS // K                                     # agent steps of an episode (Pendulum never terminates)
CAP = EPISODES * STEPS + 4                                 # trace rows: the whole run
SPLITS = ([(0, 7)], [(0, 3), (3, 4), (4, 7)], [(0, 1), (1, 7)])
RN_HIDDEN = 16
OUT_NAMES = ("score", "stats", "status", "episode_test_mean", "episode_len", "final_returns", "final_params")
# the early-out case: with early_out_num 1 a chain leaves at the first learning episode whose test mean reaches solved_reward.  The value lies
# between the oracle's per-episode test means of the six chains (computed on the CPU when the case was written): chains whose episode-2 mean
# is above it stop after three episodes, the others never reach it.  The test asserts both kinds on the single launch before it uses them.
EARLY_SOLVED = -58.0        # episode-2 means: -76.4 -93.8 -78.1 -55.4 -92.9 -91.2; chain 1 stays below -61 in every learning episode


def _snapshot(il):
    return snapshot(il, OUT_NAMES)


class Case(object):
    """One workload: the cfgs (the launch's, with the maxima, and every chain's own for the oracle), inputs, tapes."""

    def __init__(self, orc, golden, tape, virtual, test_mode, icm, hps=HPS, **td3_over):
        self.hps = hps
        from learning_environments_amd.config import td3_layer_dims
        cfgd = json.loads(str(golden("g8pr_calc_score_pendulum_td3_reward_env")["config_json"]))
        cfgd["agents"]["gtn"]["synthetic_env_type"] = 0 if virtual else 1
        cfgd["agents"]["gtn"]["agent_name"] = "td3_icm" if icm else "td3"
        cfgd["agents"]["icm"] = {"lr": 1e-3, "beta": 0.2, "eta": 0.5, "feature_dim": 8, "hidden_size": 16}
        td3 = dict(train_episodes=EPISODES, init_episodes=INIT, test_episodes=T, rb_size=RB, policy_delay=2, same_action_num=K, early_out_num=50,
                   batch_size=20, hidden_size=40, hidden_layer=3)
        td3.update(td3_over)
        solved = td3.pop("solved_reward", 1e9)
        cfgd["agents"]["td3"].update(td3)
        cfgd["envs"][ENV].update(max_steps=MAX_STEPS, hidden_size=RN_HIDDEN, hidden_layer=1, activation_fn="tanh", reward_env_type=0 if virtual else 2,
                                 solved_reward=solved)
        self.tape, self.virtual, self.icm = tape, virtual, icm
        mode = 1 if tape else 0
        _, self.cfg = _td3_cfgs(orc, cfgd, mode, test_mode=test_mode)
        assert self.cfg.icm_enabled == int(icm) and self.cfg.virtual_env == int(virtual) and self.cfg.test_mode == test_mode
        if virtual:
            P_rn = orc.mlp_num_params(orc.mlp_desc(4, RN_HIDDEN, 1, 3, "tanh")) + 2 * orc.mlp_num_params(orc.mlp_desc(4, RN_HIDDEN, 1, 1, "tanh"))
        else:
            P_rn = orc.rn_num_params(2, 3, 0, RN_HIDDEN, 1)
        rng = np.random.RandomState(101 + 2 * int(virtual) + int(icm))
        self.theta = (rng.randn(P_rn) * 0.2).astype(np.float32)
        self.eps = (rng.randn(2, P_rn) * 0.05).astype(np.float32)
        self.worker = (np.arange(CHAINS) % 2).astype(np.int32)
        self.sign = np.array([0.0, 1.0, -1.0, 1.0, -1.0, 0.0], np.float32)
        self.keys = np.array([orc.chain_key(57, 3, int(self.worker[c]), c) for c in range(CHAINS)], np.uint64)
        self.ocfgs, self.inits, self.icm_inits = [], [], []
        for c, h in enumerate(hps):
            oc, pc = _td3_cfgs(orc, cfgd, mode, test_mode=test_mode, lr=float(h["lr"]), batch_size=int(h["batch_size"]),
                               hidden=int(h["hidden_size"]), layers=int(h["hidden_layer"]))
            self.ocfgs.append(oc)
            self.inits.append(orc.agent_init_from_key(int(self.keys[c]), td3_layer_dims(pc)))
            self.icm_inits.append(orc.agent_init_from_key(int(self.keys[c]), orc.icm_layer_dims(oc), stream=orc.STREAM_ICM_INIT) if icm else None)
        self.tapes = None
        if tape:
            learn = (EPISODES - INIT) * STEPS
            idx = np.zeros((CHAINS, learn * 20), np.int32)
            for c, h in enumerate(hps):
                B = h["batch_size"]
                for j in range(learn):
                    # rows in the buffer at learn step j: every step so far on the RewardEnv (episodes of full length); on a VirtualEnv, whose
                    # learned done flag may cut an episode short, at least one row per episode so far plus one per learn step
                    size = min((INIT * STEPS if not virtual else INIT) + j + 1, RB)
                    idx[c, j * B:(j + 1) * B] = rng.randint(0, size, B)
            self.tapes = dict(rand_action=rng.uniform(-2, 2, (CHAINS, INIT * STEPS, 1)).astype(np.float32),
                              act_noise=rng.randn(CHAINS, learn, 1).astype(np.float32),
                              test_noise=rng.randn(CHAINS, (EPISODES + 1) * T * STEPS, 1).astype(np.float32),
                              policy_noise=rng.randn(CHAINS, learn * 20, 1).astype(np.float32), replay_idx=idx,
                              train_reset=np.stack([rng.uniform(-np.pi, np.pi, (CHAINS, EPISODES)), rng.uniform(-1, 1, (CHAINS, EPISODES))], -1),
                              test_reset=np.stack([rng.uniform(-np.pi, np.pi, (CHAINS, (EPISODES + 1) * T)),
                                                   rng.uniform(-1, 1, (CHAINS, (EPISODES + 1) * T))], -1))

    def oracle(self, orc, c, want_final_params=False):
        w = (np.float32(self.sign[c]) * self.eps[self.worker[c]] + self.theta).astype(np.float32)
        tapes = None
        if self.tape:
            t = self.tapes
            tapes = orc.make_td3_tapes(t["rand_action"][c], t["act_noise"][c], t["test_noise"][c], t["policy_noise"][c], t["replay_idx"][c],
                                       t["train_reset"][c], t["test_reset"][c], A=1, S=2)
        return orc.td3_rn_chain(self.ocfgs[c], w, self.inits[c], rng_key=int(self.keys[c]), tapes=tapes, trace_cap=CAP, icm_init=self.icm_inits[c],
                                want_final_params=want_final_params)

    def inner(self, eng):
        il = eng.Td3InnerLoop(self.cfg, CHAINS, trace_cap=CAP, want_episode_stats=True, want_final_params=True, vary=True)
        hps = self.hps
        il.set_hp([h["lr"] for h in hps], [h["batch_size"] for h in hps], [h["hidden_size"] for h in hps], [h["hidden_layer"] for h in hps])
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
        il = self.inner(eng)
        return il, single(il, *self.args(), OUT_NAMES)

    def split(self, eng, segments, between=None):
        il = self.inner(eng)
        return il, split(il, *self.args(), segments, OUT_NAMES, between=between)


def _check_vs_oracle(case, orc, il, snap):
    for c in range(CHAINS):
        o = case.oracle(orc, c, want_final_params=not case.icm)
        assert o["rc"] == 0 and o["learn_steps"] > 0, c
        _td3_compare(il, o, c, o["trace"]["reward"].size)
        if case.icm:
            assert np.array_equal(snap["icm_final"][c], o["icm_final"]), c
        else:
            assert np.array_equal(snap["final_params"][c, :o["final_params"].size], o["final_params"]), c


@pytest.mark.parametrize("icm", [False, True], ids=["plain", "icm"])
@pytest.mark.parametrize("test_mode", [0, 1])
@pytest.mark.parametrize("virtual", [False, True], ids=["reward_env_2", "virtual_env"])
@pytest.mark.parametrize("tape", [True, False], ids=["tape", "counter"])
def test_every_split_equals_the_single_launch_and_the_oracle(eng, orc, golden, tape, virtual, test_mode, icm):
    case = Case(orc, golden, tape, virtual, test_mode, icm)
    il, ref = case.single(eng)
    assert ref["status"].tolist() == [0] * CHAINS
    _check_vs_oracle(case, orc, il, ref)
    if not virtual:
        assert ref["stats"][:, 1].tolist() == [EPISODES * STEPS] * CHAINS          # 42 agent steps: the ring of 40 rows wrapped
        assert ref["stats"][:, 2].tolist() == [(EPISODES - INIT) * STEPS] * CHAINS
    for segments in SPLITS:
        il2, got = case.split(eng, segments)
        _same_bits(ref, got, segments)
        finished, status = il2.segment_state()
        assert finished.tolist() == [1] * CHAINS and status.tolist() == [0] * CHAINS, segments


def test_a_ring_that_wrapped_before_the_boundaries(eng, orc, golden):
    """rb_size 16: the ring wraps in episode 2 and again in episode 5, the boundaries at 3 and 4 cut through a wrapped buffer."""
    case = Case(orc, golden, False, False, 0, False, rb_size=16)
    il, ref = case.single(eng)
    assert ref["status"].tolist() == [0] * CHAINS
    _check_vs_oracle(case, orc, il, ref)
    for segments in SPLITS:
        _same_bits(ref, case.split(eng, segments)[1], segments)


def test_one_hidden_layer_maxima_where_the_old_entry_skips_the_product_queue(eng, orc, golden):
    """A launch whose maxima are one hidden layer of 40 units and batch 20 takes the DIRECT instantiation through the old entry (no product
    queue); the segments always run the queued kernel.  Same bits all the same, and kernel_variant NO_DIRECT on the old entry too."""
    from learning_environments_amd import _lib
    hps = [dict(h, hidden_layer=1) for h in HPS]
    case = Case(orc, golden, False, False, 0, False, hps=hps, hidden_layer=1)
    assert case.cfg.layers == 1 and case.cfg.kernel_variant == 0
    il, ref = case.single(eng)
    assert ref["status"].tolist() == [0] * CHAINS
    _check_vs_oracle(case, orc, il, ref)
    for segments in SPLITS:
        _same_bits(ref, case.split(eng, segments)[1], segments)
    case.cfg.kernel_variant = _lib.VARIANT_NO_DIRECT
    _same_bits(ref, case.single(eng)[1], "the old entry on the queued kernel")


def test_early_out_chains_finish_in_their_segment_and_stay_untouched(eng, orc, golden):
    case = Case(orc, golden, False, False, 0, True, solved_reward=EARLY_SOLVED, early_out_num=1)
    il, ref = case.single(eng)
    assert ref["status"].tolist() == [0] * CHAINS
    episodes_run = ref["stats"][:, 0]
    early, full = np.flatnonzero(episodes_run <= 3), np.flatnonzero(episodes_run == EPISODES)
    assert early.size >= 1 and full.size >= 1, episodes_run.tolist()        # (else the case is vacuous)
    _check_vs_oracle(case, orc, il, ref)
    names = OUT_NAMES + ("icm_final",)
    for segments in SPLITS[1:]:
        hook, seen = _poison_finished(names)
        il2, got = case.split(eng, segments, between=hook)
        assert sorted(seen) == list(range(CHAINS))                           # every chain finished at some boundary
        for c in range(CHAINS):
            for k in names:
                assert np.all(got[k][c] == SENTINEL), (segments, c, k)       # ... and nothing wrote its outputs afterwards
                assert seen[c][k].tobytes() == ref[k][c].tobytes(), (segments, c, k)
        for k in got:
            if k.startswith("trace_"):
                assert got[k].tobytes() == ref[k].tobytes(), (segments, k)
        if segments[0] == (0, 3):                                            # the early chains were finished at the first boundary
            first = []
            case.split(eng, segments[:1], between=lambda il_, b, e: first.append(il_.segment_state()[0].numpy().copy()))
            assert np.flatnonzero(first[0] == 1).tolist() == early.tolist()


def test_step_budget_that_expires_in_the_second_segment(eng, orc, golden):
    """30 env steps per episode (6 agent steps + 2 test episodes of 12): the check in front of episode 3 sees 90 > 80."""
    case = Case(orc, golden, False, False, 0, False, step_budget=80)
    il, ref = case.single(eng)
    assert ref["status"].tolist() == [0] * CHAINS
    assert ref["stats"][:, 0].tolist() == [3] * CHAINS
    assert np.all(ref["episode_len"][:, 3:] == MAX_STEPS) and not np.isnan(ref["episode_test_mean"]).any()      # time_is_up's padding
    _check_vs_oracle(case, orc, il, ref)
    for segments in SPLITS[1:]:
        hook, seen = _poison_finished(OUT_NAMES)
        il2, got = case.split(eng, segments, between=hook)
        for c in range(CHAINS):
            for k in OUT_NAMES:
                assert np.all(got[k][c] == SENTINEL), (segments, c, k)
                assert seen[c][k].tobytes() == ref[k][c].tobytes(), (segments, c, k)
        # finished behind the second segment, not the first
        first = []
        case.split(eng, segments[:2], between=lambda il_, b, e: first.append(il_.segment_state()[0].tolist()))
        assert first == [[0] * CHAINS, [1] * CHAINS], segments


def test_refusals(eng, orc, golden):
    import ctypes as C
    from learning_environments_amd import _lib
    case = Case(orc, golden, False, False, 0, False)
    il = case.inner(eng)
    pos, kw = case.args()
    il.resume = torch.full((CHAINS, _lib.TD3_RESUME_WORDS), 5, dtype=torch.int64, device=il.dev)
    before = _snapshot(il)
    args = il._run_args(*pos[:4], il.agent_init, kw["rng_keys"], None)

    def launch(b, e, resume):
        return _lib.lib().lenv_td3_rn_inner_loop_segment(C.byref(il.cfg), il._hp_arg(), None, *args[:-1], b, e, resume, args[-1])
    res = C.c_void_p(il.resume.data_ptr())
    for b, e, r in ((3, 3, res), (4, 3, res), (-1, 2, res), (0, EPISODES + 1, res), (EPISODES, EPISODES + 1, res), (0, EPISODES, None)):
        assert launch(b, e, r) == -1, (b, e)                                 # LENV_ERR_INVALID
    with pytest.raises(ValueError):
        il.run_segment(*pos, 2, 2, **kw)
    with pytest.raises(ValueError):
        il.run(*pos, episodes_per_launch=0, **kw)
    _same_bits(before, _snapshot(il), "refused launches")                    # none reached the device
    assert il.resume.cpu().unique().tolist() == [5]

    # a continuation from the wrong episode: status -10 per chain, nothing else
    il, _ = case.split(eng, [(0, 3)])
    before, rec = _snapshot(il), il.resume.cpu().numpy().copy()
    il.run_segment(*pos, 4, EPISODES, **kw)
    after = _snapshot(il)
    assert after.pop("status").tolist() == [-10] * CHAINS and before.pop("status").tolist() == [0] * CHAINS
    _same_bits(before, after, "wrong episode_begin")
    assert np.array_equal(il.resume.cpu().numpy(), rec)
    assert il.segment_state()[1].tolist() == [-10] * CHAINS


def test_run_with_episodes_per_launch(eng, orc, golden):
    """Td3InnerLoop.run(episodes_per_launch=n): the same outputs as the single launch; on_segment sees the progress; the series stops when
    every chain is finished."""
    case = Case(orc, golden, False, False, 0, False)
    _, ref = case.single(eng)
    pos, kw = case.args()
    for n, want in ((1, [(e, 0) for e in range(1, EPISODES)] + [(EPISODES, CHAINS)]), (3, [(3, 0), (6, 0), (7, CHAINS)]), (50, [(7, CHAINS)])):
        il, calls = case.inner(eng), []
        il.run(*pos, episodes_per_launch=n, on_segment=lambda done, fin: calls.append((done, fin)), **kw)
        assert calls == want, n
        _same_bits(ref, _snapshot(il), n)
    # every chain leaves at the first learning episode: three launches of one episode, then the series is over
    case = Case(orc, golden, False, False, 0, False, solved_reward=-1e9, early_out_num=1)
    _, ref = case.single(eng)
    assert ref["stats"][:, 0].tolist() == [3] * CHAINS
    il, calls = case.inner(eng), []
    il.run(*case.args()[0], episodes_per_launch=1, on_segment=lambda done, fin: calls.append((done, fin)), **case.args()[1])
    assert calls == [(1, 0), (2, 0), (3, CHAINS)]
    _same_bits(ref, _snapshot(il), "early out")
    # a bad chain status ends the series like check_status: an action-noise tape of three rows runs out in the first learning episode
    case = Case(orc, golden, True, False, 0, False)
    case.tapes["act_noise"] = case.tapes["act_noise"][:, :3]
    il, calls = case.inner(eng), []
    from learning_environments_amd import _lib
    with pytest.raises(_lib.LenvError):
        il.run(*case.args()[0], episodes_per_launch=3, on_segment=lambda done, fin: calls.append((done, fin)), **case.args()[1])
    assert calls == [(3, 0)] and il.status.cpu().tolist() == [-7] * CHAINS
