"""lenv_td3d_inner_loop_segment / lenv_td3d_rn_inner_loop_segment: the TD3_discrete_vary inner loop in episode segments.

Bar: for every split of the episodes the launches leave every output array, the step trace and final_params BIT-EQUAL to the single launch
of lenv_td3d_inner_loop / lenv_td3d_rn_inner_loop, which in turn is bit-equal to its CPU reference: oracle.td3d_chain on the VirtualEnv (tape
and counter mode), the composer of tests/td3d_composer.py on a RewardEnv / the real env (tape mode; there is no CPU chain for the counter-mode
launches on a real env, which are held to the single launch alone).

The workload: CartPole-v0 (S 4, A 2; one case on Acrobot-v1, S 6, A 3), six chains with their own hyper-parameters (hidden 8 / 24 / 40,
1 / 2 / 3 hidden layers, batch 8 / 20, two learning rates) in a launch sized for the maxima, 7 training episodes of which 2 are init episodes,
max_steps 12, 2 test episodes, rb_size 40 (a ring of min(7 * 12, 40) rows), policy_delay 2, gumbel_temp 1.0 (annealed with every learn call),
SE nets / reward nets 12 / 16 wide.  The splits put one boundary inside the init episodes and the others behind them.  The seeds were chosen on
the CPU such that the conditions each test asserts on its single launch hold.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import td3d_composer as comp  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from segments_common import SENTINEL, _poison_finished, same_bits as _same_bits, single, snapshot, split  # noqa: E402

pytestmark = pytest.mark.gpu

ENVS = {0: (4, 2), 1: (6, 3)}
HPS = [dict(lr=1e-3, batch_size=8, hidden_size=8, hidden_layer=1), dict(lr=2e-3, batch_size=20, hidden_size=24, hidden_layer=2),
       dict(lr=1e-3, batch_size=20, hidden_size=40, hidden_layer=3), dict(lr=2e-3, batch_size=8, hidden_size=40, hidden_layer=1),
       dict(lr=1e-3, batch_size=8, hidden_size=24, hidden_layer=3), dict(lr=2e-3, batch_size=20, hidden_size=8, hidden_layer=2)]
CHAINS = len(HPS)
EPISODES, INIT, MAX_STEPS, T, RB = 7, 2, 12, 2, 40
CAP = EPISODES * MAX_STEPS + 4                             # trace rows: the whole run
SPLITS = ([(0, 7)], [(0, 3), (3, 4), (4, 7)], [(0, 1), (1, 7)])
BOUNDARIES = (3, 4)                                        # the boundaries behind the init episodes
SE_HIDDEN, RN_HIDDEN = 12, 16
OUT_NAMES = ("score", "stats", "status", "episode_test_mean", "episode_len", "final_returns", "final_params")
SEED = 9        # of the cases that name no seed.  CartPole VirtualEnv, counter mode, test_mode 0: episode lengths of the six chains on the CPU
#                 12 12 8 12 6 12 5 | 12 x 7 | 12 x 7 | 12 x 7 | 12 x 7 | 9 8 7 8 7 8 9  (chains 0 and 5 meet the learned done flag)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _hip(ocfg):
    from learning_environments_amd import _lib
    c = _lib.Td3dCfg()
    for f, _ in _lib.Td3dCfg._fields_:
        setattr(c, f, getattr(ocfg, f))
    return c


def _pad(rows):
    n = max(1, max(r.shape[0] for r in rows))
    out = np.zeros((len(rows), n) + rows[0].shape[1:], rows[0].dtype)
    for i, r in enumerate(rows):
        out[i, :r.shape[0]] = r
    return out


class Case(object):
    """One workload: the cfgs (the launch's, with the maxima, and every chain's own for the CPU reference), inputs, tapes.
    env: "virtual" (the three SE nets), "reward2" (RewardEnv of type 2 over the real env) or "real" (the real env itself, type 0)."""

    def __init__(self, env_id=0, tape=False, env="virtual", test_mode=0, ln=0, hard=1, seed=SEED, scale=0.5, **over):
        S, A = ENVS[env_id]
        self.env_id, self.tape, self.env, self.S, self.A = env_id, tape, env, S, A
        kw = dict(env_id=env_id, state_dim=S, action_dim=A, max_steps=MAX_STEPS, se_hidden=SE_HIDDEN, se_layers=1, se_act=2, se_prelu=0.25,
                  hidden=40, layers=3, act=3, prelu=0.25, use_layer_norm=ln, gumbel_hard=hard, batch_size=20, rb_size=RB,
                  train_episodes=EPISODES, test_episodes=T, init_episodes=INIT, early_out_num=50, policy_delay=2, rng_mode=1 if tape else 0,
                  solved_reward=1e9, gamma=0.99, lr=1e-3, tau=0.01, action_std=0.1, policy_std=0.2, policy_std_clip=0.5, max_action=1.0,
                  gumbel_temp=1.0, adam_beta1=0.9, adam_beta2=0.999, adam_eps=1e-8, step_budget=0, se_layer_norm=0, test_mode=test_mode,
                  early_out_virtual_diff=0.01)
        kw.update(over)
        self.base = orc.Td3dCfg(**kw)
        self.cfg = _hip(self.base)
        self.rtype = {"virtual": None, "reward2": 2, "real": 0}[env]
        rng = np.random.RandomState(1000 * env_id + 100 * (self.rtype or 0) + 10 * int(tape) + seed)
        if env == "virtual":
            P_th = sum(orc.mlp_num_params(d) for d in orc.se_descs(S, A, SE_HIDDEN, 1, 2))
        else:
            P_th = (1 if self.rtype == 0 else S) * RN_HIDDEN + RN_HIDDEN + RN_HIDDEN + 1
        self.theta = (rng.randn(P_th) * scale).astype(np.float32)
        self.eps = (rng.randn(2, P_th) * 0.1).astype(np.float32)
        self.worker = (np.arange(CHAINS) % 2).astype(np.int32)
        self.sign = np.array([0.0, 1.0, -1.0, 1.0, -1.0, 0.0], np.float32)       # 0 / +-1: the kernel's fma is exact
        self.keys = np.array([orc.chain_key(57 + seed, 3, int(self.worker[c]), c) for c in range(CHAINS)], np.uint64)
        self.ccfgs, self.inits, self.chain_tapes = [], [], []
        for h in HPS:
            cc = orc.Td3dCfg.from_buffer_copy(self.base)
            cc.lr, cc.batch_size, cc.hidden, cc.layers = h["lr"], h["batch_size"], h["hidden_size"], h["hidden_layer"]
            self.ccfgs.append(cc)
            self.inits.append(rng.uniform(-0.4, 0.4, orc.td3d_num_params(cc)[0]).astype(np.float32))
            self.chain_tapes.append(comp.make_tapes(rng, cc) if tape else None)
        self._refs = {}

    def weights(self, c):
        return (np.float32(self.sign[c]) * self.eps[self.worker[c]] + self.theta).astype(np.float32)

    @property
    def has_reference(self):
        return self.env == "virtual" or (self.tape and self.base.step_budget == 0)

    def reference(self, c):
        """The chain on the CPU (computed once)."""
        if c not in self._refs:
            cc, t = self.ccfgs[c], self.chain_tapes[c]
            if self.env == "virtual":
                o = orc.td3d_chain(cc, self.weights(c), self.inits[c], rng_key=int(self.keys[c]),
                                   tapes=orc.make_td3d_tapes(self.A, **t) if self.tape else None, trace_cap=CAP)
                assert o["rc"] == 0, c
            else:
                o = comp.td3d_chain(cc, comp.RewardEnvStep(cc, self.rtype, self.weights(c), RN_HIDDEN, 1, 3), self.inits[c], t)
            self._refs[c] = o
        return self._refs[c]

    def inner(self):
        from learning_environments_amd import _lib, engine
        rn = None
        if self.env != "virtual":
            rn = _lib.Td3dRnCfg(synthetic_env_type=1, reward_env_type=self.rtype, rn_hidden=RN_HIDDEN, rn_layers=1, rn_act=3, rn_prelu=0.25,
                                rn_layer_norm=0)
        il = engine.Td3DiscreteInnerLoop(self.cfg, CHAINS, trace_cap=CAP, want_episode_stats=True, want_final_params=True, vary=True, rn=rn)
        il.set_hp(*[[h[k] for h in HPS] for k in ("lr", "batch_size", "hidden_size", "hidden_layer")])
        init = np.full((CHAINS, il.p_agent), np.nan, np.float32)        # (behind a chain's own parameters: never read)
        for c, w in enumerate(self.inits):
            init[c, :w.size] = w
        il.agent_init.copy_(dev(init))
        return il

    def args(self):
        """(positional arguments of run / run_segment up to agent_init, keyword arguments)"""
        if self.tape:
            kw = dict(tapes={k: dev(_pad([t[k] for t in self.chain_tapes])) for k in comp.TAPE_KEYS})
        else:
            kw = dict(rng_keys=dev(self.keys.view(np.int64)))
        return (dev(self.theta), dev(self.eps), dev(self.worker), dev(self.sign), None), kw

    def single(self):
        il = self.inner()
        return il, single(il, *self.args(), OUT_NAMES)

    def split(self, segments, between=None):
        il = self.inner()
        return il, split(il, *self.args(), segments, OUT_NAMES, between=between)


def _check_vs_reference(case, snap):
    """the single launch's snapshot against the CPU chains, bit for bit"""
    for c in range(CHAINS):
        o = case.reference(c)
        assert o["learn_steps"] > 0, c
        assert snap["stats"][c].tolist() == [o["episodes_run"], o["train_steps"], o["learn_steps"], o["test_steps"]], c
        assert np.array_equal(snap["episode_test_mean"][c], np.asarray(o["episode_test_mean"]), equal_nan=True), c
        assert np.array_equal(snap["episode_len"][c], np.asarray(o["episode_len"])), c
        assert np.array_equal(snap["final_returns"][c], np.asarray(o["final_test_returns"])), c
        assert float(snap["score"][c]) == o["score"], c
        P = case.inits[c].size
        assert np.array_equal(snap["final_params"][c, :P], np.asarray(o["final_params"])[:P]), c
        if "trace" in o:
            n = o["trace"]["reward"].size
            assert n == o["train_steps"]
            for k in ("action", "state", "next_state", "reward"):
                assert np.array_equal(snap["trace_" + k][c, :n], o["trace"][k][:n]), (c, k)


def _learn_steps_before(episode_len, boundary):
    return int(episode_len[INIT:boundary].sum())


def _check_conditions(case, ref):
    """What makes the case worth running: every chain learns, policy_delay 2 is cut mid-pair at a boundary, and the learned done flag ends
    an episode of the VirtualEnv early."""
    assert ref["status"].tolist() == [0] * CHAINS
    assert ref["stats"][:, 2].min() > 0
    if case.has_reference:
        odd = [(c, b) for c in range(CHAINS) for b in BOUNDARIES if _learn_steps_before(ref["episode_len"][c], b) % 2 == 1]
        assert odd, ref["episode_len"].tolist()
    if case.env == "virtual":
        assert (ref["episode_len"] < MAX_STEPS).any()


# tape / counter mode, the training env, test_mode, use_layer_norm, gumbel_hard: a covering subset of the product
CASES = [
    pytest.param(dict(env_id=0, tape=True, env="virtual", test_mode=0, ln=0, hard=1, seed=4), id="cartpole-tape-virtual-test0-hard"),
    pytest.param(dict(env_id=0, tape=False, env="virtual", test_mode=1, ln=1, hard=0, seed=9), id="cartpole-counter-virtual-test1-ln-soft"),
    pytest.param(dict(env_id=0, tape=True, env="reward2", test_mode=0, ln=1, hard=1, seed=0), id="cartpole-tape-reward2-test0-ln-hard"),
    pytest.param(dict(env_id=0, tape=False, env="reward2", test_mode=1, ln=0, hard=0, seed=0), id="cartpole-counter-reward2-test1-soft"),
    pytest.param(dict(env_id=0, tape=True, env="real", test_mode=1, ln=0, hard=0, seed=0), id="cartpole-tape-real-test1-soft"),
    pytest.param(dict(env_id=0, tape=False, env="real", test_mode=0, ln=0, hard=1, seed=0), id="cartpole-counter-real-test0-hard"),
    pytest.param(dict(env_id=1, tape=True, env="virtual", test_mode=0, ln=1, hard=0, seed=5), id="acrobot-tape-virtual-test0-ln-soft"),
]


@pytest.mark.parametrize("kw", CASES)
def test_every_split_equals_the_single_launch_and_the_reference(kw):
    case = Case(**kw)
    il, ref = case.single()
    _check_conditions(case, ref)
    if case.has_reference:
        _check_vs_reference(case, ref)
    for segments in SPLITS:
        il2, got = case.split(segments)
        _same_bits(ref, got, segments)
        finished, status = il2.segment_state()
        assert finished.tolist() == [1] * CHAINS and status.tolist() == [0] * CHAINS, segments
        rec = il2.resume.cpu().numpy()
        assert rec[:, 0].tolist() == [EPISODES] * CHAINS and np.array_equal(rec[:, 9], ref["stats"][:, 1]) and np.array_equal(rec[:, 12], rec[:, 9])


def test_a_ring_that_wrapped_before_the_boundaries():
    """rb_size 16: the ring wraps in the init episodes and again behind them, the boundaries at 3 and 4 cut through a wrapped buffer."""
    case = Case(env_id=0, tape=False, env="virtual", test_mode=0, rb_size=16)
    il, ref = case.single()
    _check_conditions(case, ref)
    assert ref["episode_len"][:, :3].sum(axis=1).min() > 16                  # every chain's ring has wrapped before the first boundary
    _check_vs_reference(case, ref)
    for segments in SPLITS:
        _same_bits(ref, case.split(segments)[1], segments)


# The early-out cases: with early_out_num 1 a chain leaves at the first learning episode whose meter value satisfies the rule.  The thresholds
# lie between the chains' per-episode values of the CPU reference (computed when the cases were written, quoted below); the tests assert on
# the single launch that some chains finish early and others never.
# test_mode 0, the real rule on the per-episode test means (multiples of 0.5 up to 12); episodes 2..6 of the chains:
#   9.5 10.5 12 11.5 12 | 12 11 10.5 12 12 | 12 10 11 9 9.5 | 10.5 12 12 10.5 9 | 11.5 8.5 11 10.5 9.5 | 12 12 9.5 12 12
# -> the chains run 5, 3, 3, 4, 7, 3 episodes: chain 3 finishes in the middle segment [3, 4), chain 4 never leaves early
EARLY_REAL = dict(solved_reward=11.75)
# test_mode 1, the virtual rule |mean_e - mean_(e-1)| / |mean_(e-1)| < diff from episode 3 on; episodes 3..6 of the chains:
#   .745 .486 .597 .477 | .165 .118 .006 .001 | .431 .612 .330 .345 | .238 .087 .116 .139 | 1.01 .391 .411 1.55 | .342 .216 .002 .171
# -> the chains run 7, 4, 7, 5, 7, 6 episodes: chain 1 finishes in the middle segment [3, 4), chains 0, 2 and 4 never leave early
EARLY_VIRTUAL = dict(early_out_virtual_diff=0.2)


def _early_out(case):
    il, ref = case.single()
    assert ref["status"].tolist() == [0] * CHAINS
    episodes_run = ref["stats"][:, 0]
    middle, full = np.flatnonzero(episodes_run == 4), np.flatnonzero(episodes_run == EPISODES)     # 4 episodes: finished in the segment [3, 4)
    assert middle.size >= 1 and full.size >= 1, episodes_run.tolist()       # (else the case is vacuous)
    _check_vs_reference(case, ref)
    for segments in SPLITS[1:]:
        hook, seen = _poison_finished(OUT_NAMES)
        il2, got = case.split(segments, between=hook)
        assert sorted(seen) == list(range(CHAINS))                           # every chain finished at some boundary
        for c in range(CHAINS):
            for k in OUT_NAMES:
                assert np.all(got[k][c] == SENTINEL), (segments, c, k)       # ... and nothing wrote its outputs afterwards
                assert seen[c][k].tobytes() == ref[k][c].tobytes(), (segments, c, k)
        for k in got:
            if k.startswith("trace_"):
                assert got[k].tobytes() == ref[k].tobytes(), (segments, k)
        if segments[0] == (0, 3):                                            # who was finished at the first boundary: the chains of 3 episodes
            first = []
            case.split(segments[:1], between=lambda il_, b, e: first.append(il_.segment_state()[0].numpy().copy()))
            assert np.flatnonzero(first[0] == 1).tolist() == np.flatnonzero(episodes_run <= 3).tolist()


def test_early_out_chains_finish_in_their_segment_and_stay_untouched():
    _early_out(Case(env_id=0, tape=False, env="virtual", test_mode=0, early_out_num=1, **EARLY_REAL))


def test_early_out_through_the_virtual_rule():
    case = Case(env_id=0, tape=False, env="virtual", test_mode=1, early_out_num=1, **EARLY_VIRTUAL)
    _early_out(case)


# env steps (training + per-episode tests) of the six chains on the CPU: 69 66 72 71 69 63 after two episodes, 96 102 108 104 104 94 after three
# -> the check in front of episode 3 is the first that sees more than 80
STEP_BUDGET = 80


def test_step_budget_that_expires_in_the_second_segment():
    case = Case(env_id=0, tape=False, env="virtual", test_mode=0, step_budget=STEP_BUDGET)
    il, ref = case.single()
    assert ref["status"].tolist() == [0] * CHAINS
    assert ref["stats"][:, 0].tolist() == [3] * CHAINS                       # the check in front of episode 3 fires for every chain
    assert not np.isnan(ref["episode_test_mean"]).any()                      # time_is_up's padding
    _check_vs_reference(case, ref)
    for segments in SPLITS[1:]:
        hook, seen = _poison_finished(OUT_NAMES)
        il2, got = case.split(segments, between=hook)
        for c in range(CHAINS):
            for k in OUT_NAMES:
                assert np.all(got[k][c] == SENTINEL), (segments, c, k)
                assert seen[c][k].tobytes() == ref[k][c].tobytes(), (segments, c, k)
        first = []                                                           # finished behind the second segment, not the first
        case.split(segments[:2], between=lambda il_, b, e: first.append(il_.segment_state()[0].tolist()))
        assert first == [[0] * CHAINS, [1] * CHAINS], segments


def _snapshot(il):
    return snapshot(il, OUT_NAMES)


@pytest.mark.parametrize("env", ["virtual", "reward2"])
def test_refusals(env):
    import ctypes as C
    from learning_environments_amd import _lib
    case = Case(env_id=0, tape=False, env=env)
    il = case.inner()
    pos, kw = case.args()
    il.resume = torch.full((CHAINS, _lib.TD3D_RESUME_WORDS), 5, dtype=torch.int64, device=il.dev)
    before = _snapshot(il)
    for b, e in ((3, 3), (4, 3), (-1, 2), (0, EPISODES + 1), (EPISODES, EPISODES + 1)):
        with pytest.raises(ValueError):
            il.run_segment(*pos, b, e, **kw)
    args = il._launch_args(*pos, kw["rng_keys"], None, segment=True)
    fn = getattr(_lib.lib(), il.segment_entry)
    assert fn(C.byref(il.cfg), *il._prefix_args(), *args[:-1], 0, EPISODES, None, args[-1]) == -1      # resume == NULL
    with pytest.raises(ValueError):
        il.run(*pos, episodes_per_launch=0, **kw)
    _same_bits(before, _snapshot(il), "refused launches")                    # none reached the device
    assert il.resume.cpu().unique().tolist() == [5]

    # a record filled with 5s: neither "finished" nor "next episode 3" -- status -10 per chain and no other write
    il.run_segment(*pos, 3, 4, **kw)
    after = _snapshot(il)
    assert after.pop("status").tolist() == [-10] * CHAINS and before.pop("status").tolist() == [0] * CHAINS
    _same_bits(before, after, "a record of 5s")
    assert il.resume.cpu().unique().tolist() == [5]

    # a continuation from the wrong episode: status -10 per chain, nothing else
    il, _ = case.split([(0, 3)])
    before, rec = _snapshot(il), il.resume.cpu().numpy().copy()
    il.run_segment(*pos, 4, EPISODES, **kw)
    after = _snapshot(il)
    assert after.pop("status").tolist() == [-10] * CHAINS and before.pop("status").tolist() == [0] * CHAINS
    _same_bits(before, after, "wrong episode_begin")
    assert np.array_equal(il.resume.cpu().numpy(), rec)
    assert il.segment_state()[1].tolist() == [-10] * CHAINS

    # a loop built with another train_episodes: its segment [5, 7) lies outside the 5 episodes its workspace and outputs were sized for
    short = Case(env_id=0, tape=False, env=env, train_episodes=5)
    il5 = short.inner()
    before = _snapshot(il5)
    with pytest.raises(ValueError):
        il5.run_segment(*pos, 5, EPISODES, **kw)
    _same_bits(before, _snapshot(il5), "a segment beyond the loop's train_episodes")


def test_run_with_episodes_per_launch():
    """Td3DiscreteInnerLoop.run(episodes_per_launch=n): the same outputs as the single launch; on_segment sees the progress; the series stops
    when every chain is finished."""
    case = Case(env_id=0, tape=False, env="virtual")
    _, ref = case.single()
    pos, kw = case.args()
    for n, want in ((2, [(2, 0), (4, 0), (6, 0), (7, CHAINS)]), (50, [(7, CHAINS)])):
        il, calls = case.inner(), []
        il.run(*pos, episodes_per_launch=n, on_segment=lambda done, fin: calls.append((done, fin)), **kw)
        assert calls == want, n
        _same_bits(ref, _snapshot(il), n)
    # every chain leaves at the first learning episode (episode 2): the series is over after the second launch of two episodes
    case = Case(env_id=0, tape=False, env="virtual", solved_reward=-1e9, early_out_num=1)
    _, ref = case.single()
    assert ref["stats"][:, 0].tolist() == [3] * CHAINS
    il, calls = case.inner(), []
    il.run(*case.args()[0], episodes_per_launch=2, on_segment=lambda done, fin: calls.append((done, fin)), **case.args()[1])
    assert calls == [(2, 0), (4, CHAINS)]
    _same_bits(ref, _snapshot(il), "early out")
    # the reward-env pair through run() as well
    case = Case(env_id=0, tape=False, env="reward2", test_mode=1)
    _, ref = case.single()
    il, calls = case.inner(), []
    il.run(*case.args()[0], episodes_per_launch=2, on_segment=lambda done, fin: calls.append((done, fin)), **case.args()[1])
    assert [c[0] for c in calls] == [2, 4, 6, 7] and calls[-1] == (7, CHAINS)
    _same_bits(ref, _snapshot(il), "reward env")
