"""lenv_ppo_rn_inner_loop_segment: the PPO inner loop in episode segments.

Bar: for every split of the episodes the launches leave every lenv_ppo_out array -- score, stats, status, the per-episode arrays, final_returns,
final_params, the five trace arrays, learn_step and learn_params -- BIT-EQUAL to the single launch of lenv_ppo_rn_inner_loop, which in turn
equals the CPU restatement (tests/ppo_ref.c) bit for bit.  Shapes and helpers are those of tests/test_ppo_gpu.py: 3 chains (signs 0, +1, -1),
6 training episodes, 2 test episodes, trace and learn captures that cover the whole run."""
import copy
import os

import numpy as np
import pytest
import torch

import ppo_ref
import segments_common
from learning_environments_amd import _lib
from test_ppo_gpu import SMALL, _reward_env_and_real_env, assert_chain_equals_restatement, bits, make_cfg, make_inputs

pytestmark = pytest.mark.gpu

CHAINS, E = 3, 6
TRACE_CAP, LEARN_CAP = 80, 6
SPLITS = ([6], [1] * 6, [2, 4], [3, 1, 2])
OUT_NAMES = ("score", "stats", "status", "episode_test_mean", "episode_len", "final_returns", "final_params", "learn_step", "learn_params")
REC_N_ROWS = 7                                            # word of the resume record: rows waiting in the on-policy buffer


def ranges(split):
    edges = np.concatenate([[0], np.cumsum(split)])
    return [(int(b), int(e)) for b, e in zip(edges[:-1], edges[1:])]


class Run(object):
    """One workload on the device: the inner loop's owner and the arguments every launch of a series gets."""

    def __init__(self, cfg, chains, theta, eps, sign, init, tapes=None, keys=None, trace_cap=TRACE_CAP, learn_cap=LEARN_CAP):
        from learning_environments_amd.engine import PpoInnerLoop
        dev = torch.device("cuda")
        self.il = PpoInnerLoop(cfg, chains, want_episode_stats=True, want_final_params=True, trace_cap=trace_cap, learn_cap=learn_cap)
        self.pos = (torch.from_numpy(theta).to(dev), torch.from_numpy(eps).to(dev), torch.arange(chains, dtype=torch.int32, device=dev),
                    torch.from_numpy(sign).to(dev), torch.from_numpy(init).to(dev))
        self.kw = dict(tapes={k: torch.from_numpy(v).to(dev) for k, v in tapes.items()} if tapes is not None else None,
                       rng_keys=torch.from_numpy(np.asarray(keys, np.uint64).view(np.int64)).to(dev) if keys is not None else None)

    def single(self):
        self.il.run(*self.pos, **self.kw)
        return self.snapshot()

    def split(self, split, between=None):
        segments_common.split(self.il, self.pos, self.kw, ranges(split), (), between=between)
        return self.snapshot()

    def snapshot(self):
        """the outputs in the form tests/test_ppo_gpu.py's launch() returns them: the trace arrays in a dict of their own"""
        out = segments_common.snapshot(self.il, OUT_NAMES)
        out["trace"] = {k[len("trace_"):]: out.pop(k) for k in sorted(out) if k.startswith("trace_")}
        return out


def flat(snap):
    out = {k: v for k, v in snap.items() if k != "trace"}
    out.update({"trace_" + k: v for k, v in snap["trace"].items()})
    return out


def same_bits(a, b, what):
    segments_common.same_bits(flat(a), flat(b), what)


CASES = {
    # learn fires at rows 31 and 62 (12 rows per episode): 12, 24 and 5 rows wait at the boundaries behind episodes 1, 2, 3; the first is before any learn call
    "pendulum_t0": ("Pendulum-v0", dict(rtype=0)),
    "cmc_t2_k5_128tanh": ("MountainCarContinuous-v0", dict(rtype=2, k=5, L=2, H=128, act="tanh", max_steps=45, ue=1.3)),
    # info inputs: phi([s | info]) is evaluated at every step, nothing of it is carried
    "cheetah_t3_64leaky": ("HalfCheetah-v3", dict(rtype=3, L=2, H=64, act="leakyrelu")),
    # a reward net of two hidden layers: every segment stages it into the arena again
    "cmc_t6_rn2": ("MountainCarContinuous-v0", dict(rtype=6, k=5, L=1, H=128, act="relu", max_steps=40, ue=2.0, rn_layers=2)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_split_equals_the_single_launch_and_the_restatement_in_tape_mode(name):
    env, over = CASES[name]
    cfg = make_cfg(env, train_episodes=E, **over)
    theta, eps, sign, init, tapes = make_inputs(cfg, env, CHAINS, seed=2000 + len(name))
    assert sign.tolist() == [0.0, 1.0, -1.0]
    ref = Run(cfg, CHAINS, theta, eps, sign, init, tapes=tapes).single()
    assert ref["status"].tolist() == [0] * CHAINS
    assert (ref["stats"][:, 1] <= TRACE_CAP).all() and (ref["stats"][:, 2] <= LEARN_CAP).all() and (ref["stats"][:, 2] >= 2).all()   # the captures cover the run
    assert_chain_equals_restatement(cfg, 0, ref, theta, eps, sign, init, tapes=tapes, trace_cap=TRACE_CAP, learn_cap=LEARN_CAP)
    pending = []
    for split in SPLITS:
        run = Run(cfg, CHAINS, theta, eps, sign, init, tapes=tapes)
        hook = (lambda il, b, e: pending.append(il.resume[:, REC_N_ROWS].cpu().tolist())) if split == [1] * 6 else None
        got = run.split(split, between=hook)
        same_bits(ref, got, (name, split))
        finished, status = run.il.segment_state()
        assert finished.tolist() == [1] * CHAINS and status.tolist() == [0] * CHAINS, split
    if name == "pendulum_t0":
        assert ref["learn_step"][:, :2].tolist() == [[31, 62]] * CHAINS and ref["stats"][:, 2].tolist() == [2] * CHAINS
        # ... so the boundary behind episode 1 (12 agent steps) lies before the first learn call and the row buffer is partly filled at every boundary
        assert [p[0] for p in pending] == [12, 24, 5, 17, 29, 10] and all(len(set(p)) == 1 for p in pending)


def test_every_split_equals_the_single_launch_and_the_restatement_in_counter_mode():
    env, over = CASES["cmc_t2_k5_128tanh"]
    cfg = make_cfg(env, train_episodes=E, rng_mode=_lib.RNG_COUNTER, **over)
    theta, eps, sign, init, _ = make_inputs(cfg, env, CHAINS, seed=2100)
    keys = np.array([_lib.lib().lenv_chain_key(23, 1, c, 0) for c in range(CHAINS)], np.uint64)
    ref = Run(cfg, CHAINS, theta, eps, sign, init, keys=keys).single()
    assert ref["status"].tolist() == [0] * CHAINS
    assert_chain_equals_restatement(cfg, 0, ref, theta, eps, sign, init, key=int(keys[0]), trace_cap=TRACE_CAP, learn_cap=LEARN_CAP)
    for split in ([1] * 6, [6]):
        same_bits(ref, Run(cfg, CHAINS, theta, eps, sign, init, keys=keys).split(split), split)


def test_action_std_below_the_clamp_of_actor_old():
    """action_std 0.0005: act() clamps actor_old's std to 0.001 in place, actor's own parameter stays 0.0005 until the first learn call (row 31).
    The boundary behind episode 0 lies before it: the actions of episode 1 must be drawn with 0.001, as in the single launch."""
    cfg = make_cfg("Pendulum-v0", rtype=2, train_episodes=E, action_std=0.0005)
    theta, eps, sign, init, tapes = make_inputs(cfg, "Pendulum-v0", CHAINS, seed=2200)
    assert (init[:, 0] == np.float32(0.0005)).all()
    ref = Run(cfg, CHAINS, theta, eps, sign, init, tapes=tapes).single()
    assert ref["learn_step"][:, 0].tolist() == [31] * CHAINS
    # the restatement clamps actor_old's std alone: rows 12..23 (episode 1) are mean + noise * 0.001 there
    assert_chain_equals_restatement(cfg, 0, ref, theta, eps, sign, init, tapes=tapes, trace_cap=TRACE_CAP, learn_cap=LEARN_CAP)
    for split in ([1, 5], [6]):
        got = Run(cfg, CHAINS, theta, eps, sign, init, tapes=tapes).split(split)
        assert np.array_equal(bits(got["trace"]["action"][:, 12:24]), bits(ref["trace"]["action"][:, 12:24])), split
        same_bits(ref, got, split)


def _restatement_episodes_run(cfg, theta, eps, sign, init, tapes):
    out = []
    for c in range(init.shape[0]):
        w = (np.float32(sign[c]) * eps[c] + theta).astype(np.float32) if sign[c] != 0 else theta
        r = ppo_ref.chain(cfg, w, init[c], tapes={k: v[c] for k, v in tapes.items()})
        assert r["rc"] == 0
        out.append(int(r["episodes_run"]))
    return out


CLOSING = ("score", "final_returns", "episode_test_mean", "episode_len", "stats", "final_params")


def test_early_out_in_a_middle_segment():
    """solved_reward -1e9 with one init episode: every chain leaves behind its second episode.  With one episode per launch the closing
    outputs appear in the second segment, the series stops there, and a further segment leaves everything as it is."""
    cfg = make_cfg("Pendulum-v0", rtype=2, train_episodes=E, solved_reward=-1e9, init_episodes=1, early_out_num=2)
    theta, eps, sign, init, tapes = make_inputs(cfg, "Pendulum-v0", CHAINS, seed=2300)
    ran = _restatement_episodes_run(cfg, theta, eps, sign, init, tapes)
    assert all(2 <= n <= 4 for n in ran) and len(set(ran)) == 1, ran
    n = ran[0]
    ref = Run(cfg, CHAINS, theta, eps, sign, init, tapes=tapes).single()
    assert ref["stats"][:, 0].tolist() == ran and np.isnan(ref["episode_test_mean"][:, n:]).all()
    run, calls, seen = Run(cfg, CHAINS, theta, eps, sign, init, tapes=tapes), [], []
    run.il.score.fill_(-7.0)                               # (the caller owns the outputs: the closing part has to write the score)
    run.il.final_returns.fill_(-7.0)

    def on_segment(done, fin):
        calls.append((done, fin))
        seen.append(run.snapshot())
    run.il.run(*run.pos, episodes_per_launch=1, on_segment=on_segment, **run.kw)
    assert calls == [(e, 0) for e in range(1, n)] + [(n, CHAINS)]                      # ... and no launch behind the one that finished them
    for s in seen[:-1]:                                    # an unfinished segment: the checkpoint, nothing of the closing part
        assert (s["score"] == -7.0).all() and (s["final_returns"] == -7.0).all()
    assert (seen[0]["stats"][:, 0] == 1).all() and not np.array_equal(seen[0]["final_params"], np.zeros_like(seen[0]["final_params"]))
    same_bits(ref, seen[-1], "the segment of the early out")
    before, rec = run.snapshot(), run.il.resume.cpu().numpy().copy()
    assert rec[:, 1].tolist() == [1] * CHAINS
    run.il.run_segment(*run.pos, n, n + 1, **run.kw)       # the range a caller unaware of the early out would run next
    same_bits(before, run.snapshot(), "a segment behind the end")
    assert np.array_equal(run.il.resume.cpu().numpy(), rec)


# chains that leave in different segments: early_out_num 1, one init episode, and a threshold between the chains' per-episode test means of the
# restatement (computed on the CPU when the case was written; the test asserts the spread before it uses it)
# seed 2301: the test means of episodes 1.. are  -95.5 -66.3 ..  /  -87.5 -75.0 -85.6 -56.0 ..  /  -15.0 ..: the chains leave behind 3, 5 and 2 episodes
UNEVEN = dict(seed=2301, solved_reward=-70.0)


def test_chains_that_finish_in_different_segments():
    cfg = make_cfg("Pendulum-v0", rtype=2, train_episodes=E, solved_reward=UNEVEN["solved_reward"], init_episodes=1, early_out_num=1)
    theta, eps, sign, init, tapes = make_inputs(cfg, "Pendulum-v0", CHAINS, seed=UNEVEN["seed"])
    ran = _restatement_episodes_run(cfg, theta, eps, sign, init, tapes)
    assert ran == [3, 5, 2], ran
    ref = Run(cfg, CHAINS, theta, eps, sign, init, tapes=tapes).single()
    assert ref["stats"][:, 0].tolist() == ran and ref["status"].tolist() == [0] * CHAINS
    run, calls = Run(cfg, CHAINS, theta, eps, sign, init, tapes=tapes), []
    run.il.run(*run.pos, episodes_per_launch=1, on_segment=lambda done, fin: calls.append((done, fin)), **run.kw)
    same_bits(ref, run.snapshot(), "uneven chains")
    assert calls == [(e, sum(1 for n in ran if n <= e)) for e in range(1, max(ran) + 1)]
    same_bits(ref, Run(cfg, CHAINS, theta, eps, sign, init, tapes=tapes).split([2, 4]), "uneven chains, [2, 4]")


def test_wrong_continuation():
    cfg = make_cfg("Pendulum-v0", rtype=2, train_episodes=E)
    theta, eps, sign, init, tapes = make_inputs(cfg, "Pendulum-v0", CHAINS, seed=2400)
    run = Run(cfg, CHAINS, theta, eps, sign, init, tapes=tapes)
    run.il.run_segment(*run.pos, 0, 2, **run.kw)
    before, rec = run.snapshot(), run.il.resume.cpu().numpy().copy()
    assert before["status"].tolist() == [0] * CHAINS and rec[:, 0].tolist() == [2] * CHAINS and rec[:, 1].tolist() == [0] * CHAINS
    assert before["stats"][:, 0].tolist() == [2] * CHAINS                               # the checkpoint of [0, 2)
    run.il.run_segment(*run.pos, 3, 4, **run.kw)
    after = run.snapshot()
    assert after.pop("status").tolist() == [-10] * CHAINS
    before.pop("status")
    same_bits(before, after, "wrong episode_begin")
    assert np.array_equal(run.il.resume.cpu().numpy(), rec)
    assert run.il.segment_state()[1].tolist() == [-10] * CHAINS


def test_tape_underrun_in_a_later_segment():
    """An action-noise tape one row short of what episode 4 needs (12 rows per episode: 59 instead of 60)."""
    cfg = make_cfg("Pendulum-v0", rtype=2, train_episodes=E)
    theta, eps, sign, init, tapes = make_inputs(cfg, "Pendulum-v0", CHAINS, seed=2500)
    tapes = dict(tapes, act_noise=np.ascontiguousarray(tapes["act_noise"][:, :59]))
    ref = Run(cfg, CHAINS, theta, eps, sign, init, tapes=tapes).single()
    assert ref["status"].tolist() == [-7] * CHAINS
    run = Run(cfg, CHAINS, theta, eps, sign, init, tapes=tapes)
    first = []
    got = run.split([3, 3], between=lambda il, b, e: first.append(il.segment_state()[1].tolist()))
    assert first[0] == [0] * CHAINS                        # ... the first segment had all its rows
    assert got["status"].tolist() == ref["status"].tolist() and run.il.segment_state()[1].tolist() == [-7] * CHAINS
    same_bits(ref, got, "underrun in the second segment")
    run, calls = Run(cfg, CHAINS, theta, eps, sign, init, tapes=tapes), []
    with pytest.raises(_lib.LenvError):
        run.il.run(*run.pos, episodes_per_launch=3, on_segment=lambda done, fin: calls.append((done, fin)), **run.kw)
    assert calls == [(3, 0), (6, CHAINS)]                  # the callback sees the segment in which the chains failed; then the status raises


def test_run_argument_checks():
    cfg = make_cfg("Pendulum-v0", rtype=2, train_episodes=E)
    theta, eps, sign, init, tapes = make_inputs(cfg, "Pendulum-v0", CHAINS, seed=2600)
    run = Run(cfg, CHAINS, theta, eps, sign, init, tapes=tapes)
    before = run.snapshot()
    for n in (0, -3):
        with pytest.raises(ValueError):
            run.il.run(*run.pos, episodes_per_launch=n, **run.kw)
    for b, e in ((2, 2), (4, 3), (-1, 2), (0, E + 1), (E, E + 1)):
        with pytest.raises(ValueError):
            run.il.run_segment(*run.pos, b, e, **run.kw)
    same_bits(before, run.snapshot(), "refused launches")   # none reached the device
    none = make_cfg("Pendulum-v0", rtype=2, train_episodes=0)
    run0 = Run(none, CHAINS, theta, eps, sign, init, tapes=tapes)
    with pytest.raises(ValueError):
        run0.il.run(*run0.pos, episodes_per_launch=1, **run0.kw)
    calls = []
    got = None
    for n, want in ((1, [(e, 0) for e in range(1, E)] + [(E, CHAINS)]), (4, [(4, 0), (6, CHAINS)]), (50, [(6, CHAINS)])):
        run, calls = Run(cfg, CHAINS, theta, eps, sign, init, tapes=tapes), []
        run.il.run(*run.pos, episodes_per_launch=n, on_segment=lambda done, fin: calls.append((done, fin)), **run.kw)
        assert calls == want, n
        if got is None:
            got = run.snapshot()
        else:
            same_bits(got, run.snapshot(), n)


GOLDEN_CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ckpt_cmc_reward_env_reference.pt")


def test_transfer_algo_entry_points_in_segments(tmp_path):
    from learning_environments_amd.experiments import transfer_algo as ta
    env_name = "MountainCarContinuous-v0"
    base = ta.base_config(env_name)
    base["envs"][env_name].update(max_steps=60, hidden_size=32)
    envs = [_reward_env_and_real_env(base, s) for s in (1, 2)]
    real_env = envs[0][1]
    calls = []
    one = ta.train_test_agents("2", envs[0][0], real_env, copy.deepcopy(base), env_name, agents_num=3, seed=9, settings=SMALL)
    seg = ta.train_test_agents("2", envs[0][0], real_env, copy.deepcopy(base), env_name, agents_num=3, seed=9, settings=SMALL, episodes_per_launch=1,
                               on_segment=lambda done, fin: calls.append((done, fin)))
    assert seg == one and calls == [(1, 0), (2, 0), (3, 3)]
    both = ta.train_test_agents_models("2", [e[0] for e in envs], real_env, copy.deepcopy(base), env_name, agents_num=2, seed=9, settings=SMALL)
    both_seg = ta.train_test_agents_models("2", [e[0] for e in envs], real_env, copy.deepcopy(base), env_name, agents_num=2, seed=9, settings=SMALL,
                                           episodes_per_launch=1)
    assert both_seg == both and both[0] != both[1]
    assert ta.DEFAULT_EPISODES_PER_LAUNCH.keys() == ta.PPO_SETTINGS.keys()

    small = dict(train_episodes=3, update_episodes=1, ppo_epochs=2)
    calls = []
    rewards, lengths = ta.eval_models("2", [GOLDEN_CKPT, GOLDEN_CKPT], save_dir=str(tmp_path), agents_num=2, settings=small, episodes_per_launch=1,
                                      on_segment=lambda done, fin: calls.append((done, fin)))
    assert [c[0] for c in calls] == [1, 2, 3] and calls[-1][1] == 4                  # on_segment once per training episode; 2 models x 2 agents
    assert len(rewards) == len(lengths) == 4 and all(len(r) == 3 and np.isfinite(r).all() for r in rewards) and all(len(l) == 3 for l in lengths)
    # the concatenation, model by model, of what train_test_agents returns for each model (model index m keys its agents)
    for m in range(2):
        reward_env, real, config = ta.load_envs_and_config(GOLDEN_CKPT)
        r, l = ta.train_test_agents("2", reward_env, real, config, agents_num=2, model_index=m, settings=small)
        assert rewards[2 * m:2 * m + 2] == r and lengths[2 * m:2 * m + 2] == l
    saved = torch.load(os.path.join(str(tmp_path), "best_transfer_algo2.pt"))
    assert sorted(saved) == ["config", "episode_length_list", "model_agents", "model_num", "reward_list"]
    assert saved["reward_list"] == rewards and saved["episode_length_list"] == lengths and saved["model_num"] == 2 and saved["model_agents"] == 2
    assert saved["config"]["agents"]["ppo"]["train_episodes"] == 3 and saved["config"]["agents"]["ppo"]["same_action_num"] == 5
    path = ta.save_list("7", config, rewards, lengths, str(tmp_path / "again"))
    again = torch.load(path)
    assert os.path.basename(path) == "best_transfer_algo7.pt" and again["model_num"] == 10 and again["model_agents"] == 10

    calls = []
    rewards, lengths = ta.eval_base("0", GOLDEN_CKPT, model_num=2, agents_num=2, settings=small, episodes_per_launch=1,
                                    on_segment=lambda done, fin: calls.append((done, fin)))
    assert len(calls) == 3 and len(rewards) == len(lengths) == 4 and all(len(r) == 3 for r in rewards)
    assert rewards[:2] != rewards[2:]                      # repetition m keys its agents as model index m
    _, real, config = ta.load_envs_and_config(GOLDEN_CKPT)
    r, l = ta.train_test_agents("0", real, real, config, agents_num=2, model_index=1, settings=small)
    assert rewards[2:] == r and lengths[2:] == l
    for fn, arg in ((ta.eval_models, [GOLDEN_CKPT]), (ta.eval_base, GOLDEN_CKPT)):
        with pytest.raises(NotImplementedError, match="ppo_icm"):
            fn("-1", arg)
