"""The PPO kernel over the envelope its layout function admits: lenv_ppo_rn_inner_loop (and its segment form) against the CPU restatement
(tests/ppo_ref.c) bit for bit at the widths, row counts, episode / repeat counts and reward-net sizes where the code takes another path.

Every case: tape mode, 2 chains (signs 0 and +1), a trace that holds every row and a learn capture that holds every call; compared are the
trace, the parameters after every learn call, the final parameters, episode lengths, test means, final returns and the score
(assert_chain_equals_restatement of test_ppo_gpu.py).  Every case asserts lenv_ppo_rows(cfg) == N, at least two learn calls and rows acted
after the last one; the two degenerate cases (ppo_epochs 0, train_episodes 0) assert what they are there for instead.

What each group is for (docs/notebook_ppo_envelope.md has the table and the wall times):
  WIDTHS    hidden 1, 3, 15 (net_row1's scalar tail alone), 17, 33 (one unrolled step + tail), 100, 127; rows of the activation matrices that
            are not 16-byte aligned (the staging falls to its element-wise branches), one-column outputs; every state_dim meets an odd width
  ROWS      2 .. 2048 rows per learn call: 1 .. 32 stages of 64 in every weight-gradient reduction and wg_colsum, 1 .. 8 row blocks of 256 in
            gemm_run_queue's block-by-block branch with every count of 32-row tiles in the last block, the returns scan's LDS copy filled to
            its last float at 2048
  CMC       an episode that ends at the flag inside the row buffer: the returns scan restarts there
  COUNTS    64 / 63 test episodes (ret[PP_MAXT]), same_action_num 64 (one agent step per episode), 7 (a ragged last repeat), 0 (== 1)
  RN        reward-net widths 1, 5, 100 and the widest admitted with theta in LDS; 5, 100 and 512 with theta in the arena (2 and 3 hidden layers)
  SEGMENTS  the 2048-row case and the width-33, 257-row case cut where the row buffer is partly filled"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import ppo_ref
from learning_environments_amd import _lib
from test_ppo_gpu import assert_chain_equals_restatement, bits, launch, make_cfg, make_inputs

pytestmark = pytest.mark.gpu

CHAINS = 2
PEND, CMC, CHEETAH = "Pendulum-v0", "MountainCarContinuous-v0", "HalfCheetah-v3"


def rows_of(cfg):
    return int(_lib.lib().lenv_ppo_rows(C.byref(cfg)))


def agent_steps(cfg):
    return -(-cfg.max_steps // max(1, cfg.same_action_num))


def caps(cfg, N):
    """trace / learn capacities that hold the whole run: every episode at its full length, every learn call"""
    rows = max(cfg.train_episodes, 1) * agent_steps(cfg)
    return rows + 4, rows // N + 2


def run_case(env, N, seed, tapes_hook=None, **over):
    """One launch of 2 chains and the restatement of both: (cfg, inputs, got, [ref per chain]) after the common assertions."""
    cfg = make_cfg(env, **over)
    assert rows_of(cfg) == N == ppo_ref.rows(cfg)
    inputs = make_inputs(cfg, env, CHAINS, seed=seed)
    theta, eps, sign, init, tapes = inputs
    if tapes_hook is not None:
        tapes_hook(tapes)
    trace_cap, learn_cap = caps(cfg, N)
    got = launch(cfg, CHAINS, theta, eps, sign, init, tapes=tapes, trace_cap=trace_cap, learn_cap=learn_cap)
    assert (got["status"] == 0).all()
    def one_chain(c):
        ref = assert_chain_equals_restatement(cfg, c, got, theta, eps, sign, init, tapes=tapes, trace_cap=trace_cap, learn_cap=learn_cap)
        assert ref["train_steps"] <= trace_cap and ref["learn_calls"] <= learn_cap            # the captures held the whole run
        return ref
    with ThreadPoolExecutor(CHAINS) as pool:              # the restatement of a 2048-row chain takes seconds: both chains at once
        refs = list(pool.map(one_chain, range(CHAINS)))
    return cfg, inputs, got, refs


def assert_calls_and_rows_after(refs, N):
    for ref in refs:
        assert ref["learn_calls"] >= 2 and list(ref["learn_step"]) == [N * (i + 1) for i in range(ref["learn_calls"])]
        assert ref["train_steps"] > ref["learn_step"][-1]                    # rows acted by the policy the last call left


# the single cases: name -> (env, rows per learn call, make_cfg arguments); tests/test_ppo_envelope_reference.py checks every N on the CPU
NAMED = {
    "flag": (CMC, 513, dict(rtype=2, k=5, L=2, H=64, act="tanh", max_steps=100, ue=25.62, train_episodes=65, T=1, epochs=2)),
    "T64": (PEND, 21, dict(rtype=2, H=64, max_steps=8, ue=2.5, train_episodes=6, T=64)),
    "T63": (PEND, 21, dict(rtype=2, H=64, max_steps=8, ue=2.5, train_episodes=6, T=63)),
    "k64": (PEND, 7, dict(rtype=2, k=64, H=64, max_steps=40, ue=10.0, train_episodes=16)),
    "k7": (CHEETAH, 15, dict(rtype=4, k=7, H=64, L=1, act="tanh", max_steps=40, ue=2.5, train_episodes=6)),
    "k0": (PEND, 31, dict(rtype=2, k=0, H=64)),
    "k1": (PEND, 31, dict(rtype=2, k=1, H=64)),
    "epochs0": (PEND, 31, dict(rtype=2, H=64, epochs=0)),
    "episodes0": (PEND, 31, dict(rtype=2, H=64, train_episodes=0, T=3)),
}


def named_case(name, seed, **kw):
    env, N, over = NAMED[name]
    return run_case(env, N, seed, **kw, **over)


# ---- widths ---------------------------------------------------------------------------------------------------------------------------------
# env, reward type, same_action_num, hidden layers, width, activation, rows, extra.  31 rows: 12 agent steps per episode, update_episodes 2.5
WIDTHS = [
    (PEND, 2, 1, 1, 1, "leakyrelu", 31, {}),
    (CMC, 1, 1, 2, 1, "tanh", 31, {}),
    (CHEETAH, 0, 1, 1, 3, "leakyrelu", 31, {}),
    (PEND, 5, 1, 2, 3, "relu", 31, {}),
    (CMC, 6, 5, 1, 15, "tanh", 13, dict(max_steps=40, ue=1.5)),
    (CHEETAH, 2, 1, 2, 15, "relu", 31, {}),
    (PEND, 0, 1, 1, 17, "leakyrelu", 31, {}),
    (CHEETAH, 5, 1, 2, 17, "tanh", 31, {}),
    (CMC, 2, 1, 1, 33, "relu", 31, {}),
    (CHEETAH, 6, 1, 2, 33, "leakyrelu", 31, {}),
    (PEND, 1, 5, 1, 100, "tanh", 10, dict(max_steps=30, ue=1.5)),
    (CMC, 5, 1, 2, 100, "leakyrelu", 31, {}),
    (CHEETAH, 1, 1, 1, 127, "relu", 31, {}),
    (PEND, 6, 1, 2, 127, "tanh", 31, {}),
]


@pytest.mark.parametrize("env,rtype,k,L,H,act,N,extra", WIDTHS, ids=["%s-H%d-L%d-%s" % (c[0][:4], c[4], c[3], c[5]) for c in WIDTHS])
def test_odd_widths(env, rtype, k, L, H, act, N, extra):
    _, _, _, refs = run_case(env, N, seed=3000 + 10 * H + L, rtype=rtype, k=k, L=L, H=H, act=act, **extra)
    assert_calls_and_rows_after(refs, N)


WIDE_ROWS = dict(rtype=2, L=2, max_steps=64, ue=4.0, train_episodes=9, T=1)        # 257 rows: a block of 256 and a block of one row


_shared = {}                                              # cases the segment tests run again: one launch and one restatement each


def wide_case(H, act):
    if ("wide", H) not in _shared:
        _shared[("wide", H)] = run_case(PEND, 257, seed=3100 + H, H=H, act=act, **WIDE_ROWS)
    return _shared[("wide", H)]


@pytest.mark.parametrize("H,act", [(33, "tanh"), (1, "leakyrelu")], ids=["H33", "H1"])
def test_odd_widths_in_the_blocked_products(H, act):
    """257 rows: the block-by-block branch re-offsets aux / out by 256 rows of 33 floats (not 16-byte aligned) and of one float."""
    _, _, _, refs = wide_case(H, act)
    assert_calls_and_rows_after(refs, 257)


# ---- rows -----------------------------------------------------------------------------------------------------------------------------------
# N: (max_steps, update_episodes, train_episodes): the first n with n / max_steps > update_episodes is N; two calls and a few rows.
# (2 rows at 13 steps per episode, not 12: with an even episode length every episode would end on a learn call and no row would follow the last)
ROWS = {
    2: (13, 0.1, 1), 64: (16, 3.99, 9), 65: (16, 4.0, 9), 255: (64, 3.98, 9), 256: (64, 3.99, 9), 257: (64, 4.0, 9), 512: (64, 7.99, 17),
    513: (64, 8.0, 17), 1999: (200, 9.9925, 21), 2047: (200, 10.2325, 21), 2048: (200, 10.2375, 21),
}


def rows_cfg_args(N, H=128):
    max_steps, ue, E = ROWS[N]
    return dict(rtype=2, L=2, H=H, act="relu", max_steps=max_steps, ue=ue, train_episodes=E, T=1, epochs=2 if N > 513 else 3)


def rows_case(N, H=128):
    if (N, H) not in _shared:
        _shared[(N, H)] = run_case(PEND, N, seed=3200 + N + H, **rows_cfg_args(N, H))
    return _shared[(N, H)]


@pytest.mark.parametrize("N,H", [(n, 128) for n in sorted(ROWS)] + [(2048, 64)], ids=lambda v: str(v))
def test_rows_per_learn_call(N, H):
    cfg, _, _, refs = rows_case(N, H)
    assert_calls_and_rows_after(refs, N)
    assert cfg.hidden == H and cfg.layers == 2


def flag_resets(tapes):
    """every fifth training episode starts one env step from the flag, moving right: it ends there in its first agent step"""
    tapes["train_reset"][:, ::5, 0] = 0.44
    tapes["train_reset"][:, ::5, 1] = 0.03


def test_an_episode_that_ends_at_the_flag_inside_the_row_buffer():
    """MountainCarContinuous, 513 rows, same_action_num 5: the backward returns scan restarts at a done row in the middle of a block."""
    N, nag = 513, 20
    cfg, _, got, refs = named_case("flag", 3300, tapes_hook=flag_resets)
    assert agent_steps(cfg) == nag
    assert_calls_and_rows_after(refs, N)
    for c in range(CHAINS):
        done = got["trace"]["done"][c][:N]
        ends = np.flatnonzero(done > 0.5)
        lengths = np.diff(np.concatenate([[-1], ends]))
        assert (lengths < nag).any() and (lengths == nag).any()              # episodes cut short by the flag among full ones
        short = ends[lengths < nag]
        assert ((short > 0) & (short < N - 1) & (short % 256 != 255)).any()   # ... one of them inside the buffer, not at a block's edge


# ---- counts ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [64, 63])
def test_many_test_episodes(T):
    cfg, _, got, refs = named_case("T%d" % T, 3400 + T)
    assert_calls_and_rows_after(refs, 21)
    assert got["final_returns"].shape == (CHAINS, T) and (got["stats"][:, 3] == 7 * T * 8).all()
    assert len(set(got["final_returns"][0].tolist())) == T                   # every slot of the returns buffer its own episode


def test_same_action_num_above_max_steps():
    """same_action_num 64 over 40 steps: one agent step per episode, 40 env steps behind it; 10 / (64 / 40) -> 7 rows per learn call"""
    cfg, _, got, refs = named_case("k64", 3500)
    assert agent_steps(cfg) == 1 and (got["episode_len"] == 64).all() and (got["stats"][:, 1] == 16).all()
    assert_calls_and_rows_after(refs, 7)


def test_ragged_last_repeat():
    """same_action_num 7 over 40 steps: six agent steps per episode, the last one of five env steps"""
    cfg, _, got, refs = named_case("k7", 3600)
    assert agent_steps(cfg) == 6 and (got["episode_len"] == 42).all() and (got["stats"][:, 3] == 7 * 2 * 40).all()
    assert_calls_and_rows_after(refs, 15)


def test_same_action_num_zero_is_one():
    """k_rep = same_action_num > 1 ? same_action_num : 1 in the kernel, the restatement and the row count: 0 repeats nothing, like 1"""
    outs = []
    for k in (0, 1):
        _, _, got, refs = named_case("k%d" % k, 3700)
        assert_calls_and_rows_after(refs, 31)
        outs.append(got)
    for name in ("score", "final_params", "final_returns", "episode_test_mean", "learn_params"):
        assert np.array_equal(bits(outs[0][name]), bits(outs[1][name])), name
    for name in ("stats", "episode_len", "learn_step", "status"):
        assert np.array_equal(outs[0][name], outs[1][name]), name
    for name in outs[0]["trace"]:
        assert np.array_equal(bits(outs[0]["trace"][name]), bits(outs[1]["trace"][name])), name


# ---- reward net -----------------------------------------------------------------------------------------------------------------------------
def rn_cfg(rn_hidden, rn_layers):
    return make_cfg(CHEETAH, rtype=3, H=64, rn_hidden=rn_hidden, rn_layers=rn_layers)


def widest_reward_net_in_lds():
    L = _lib.lib()
    ok = [h for h in range(1, 600) if L.lenv_ppo_rn_lds_bytes(C.byref(rn_cfg(h, 1))) > 0]
    assert ok == list(range(1, len(ok) + 1))               # admitted up to a limit, refused from there on
    return ok[-1]


def test_widest_reward_net_query():
    L = _lib.lib()
    widest = widest_reward_net_in_lds()
    assert 100 < widest <= 512
    assert 0 < L.lenv_ppo_rn_lds_bytes(C.byref(rn_cfg(widest, 1))) <= 160 * 1024
    for q in (L.lenv_ppo_rn_lds_bytes, L.lenv_ppo_rows, L.lenv_ppo_rn_num_params):
        assert q(C.byref(rn_cfg(widest + 1, 1))) == -2                        # LENV_ERR_UNSUPPORTED
    assert L.lenv_ppo_rn_workspace_bytes(C.byref(rn_cfg(widest + 1, 1)), CHAINS) == -2


@pytest.mark.parametrize("rn_layers,rn_hidden", [(1, 1), (1, 5), (1, 100), (1, "widest"), (2, 5), (2, 100), (3, 5), (3, 100), (3, 512)],
                         ids=lambda v: str(v))
def test_reward_net_sizes(rn_layers, rn_hidden):
    """HalfCheetah type 3: the net's input is state | info, 21 wide, and phi([s | info]) is evaluated twice a step"""
    if rn_hidden == "widest":
        rn_hidden = widest_reward_net_in_lds()
    cfg, inputs, _, refs = run_case(CHEETAH, 31, seed=3800 + 7 * rn_layers + rn_hidden, rtype=3, H=64, rn_hidden=rn_hidden, rn_layers=rn_layers)
    assert inputs[0].size == 21 * rn_hidden + rn_hidden + (rn_layers - 1) * (rn_hidden * rn_hidden + rn_hidden) + rn_hidden + 1
    assert_calls_and_rows_after(refs, 31)
    assert np.abs(refs[0]["trace"]["reward"]).max() > 0                        # the shaped reward is the net's alone (type 3)


# ---- degenerate but admitted ----------------------------------------------------------------------------------------------------------------
def test_zero_epochs():
    """ppo_epochs 0: learn computes the returns and runs no epoch; the parameters after every call are the fresh agent's"""
    cfg, inputs, got, refs = named_case("epochs0", 3900)
    init = inputs[3]
    for c in range(CHAINS):
        assert refs[c]["learn_calls"] == 2 and list(refs[c]["learn_step"]) == [31, 62]
        for i in range(2):
            assert np.array_equal(bits(got["learn_params"][c][i]), bits(init[c]))
        assert np.array_equal(bits(got["final_params"][c]), bits(init[c]))


def test_zero_train_episodes():
    """train_episodes 0: the launch is the final test alone (BaseAgent.test of the fresh agent)"""
    env, N, over = NAMED["episodes0"]
    cfg = make_cfg(env, **over)
    assert rows_of(cfg) == N
    one = make_cfg(env, **dict(over, train_episodes=1))              # (tapes of one episode: the launch refuses a tape without rows)
    theta, eps, sign, init, tapes = make_inputs(one, PEND, CHAINS, seed=3950)
    got = launch(cfg, CHAINS, theta, eps, sign, init, tapes=tapes, trace_cap=4, learn_cap=2)
    assert got["status"].tolist() == [0] * CHAINS
    for c in range(CHAINS):
        w = (np.float32(sign[c]) * eps[c] + theta).astype(np.float32) if sign[c] != 0 else theta
        ref = ppo_ref.chain(cfg, w, init[c], tapes={k: v[c] for k, v in tapes.items()}, trace_cap=4, learn_cap=2)
        assert ref["rc"] == 0 and (ref["episodes_run"], ref["train_steps"], ref["learn_calls"], ref["test_steps"]) == (0, 0, 0, 3 * 12)
        assert got["stats"][c].tolist() == [0, 0, 0, 3 * 12]
        assert np.array_equal(bits(got["final_returns"][c]), bits(ref["final_returns"]))
        assert bits(np.array([got["score"][c]]))[0] == bits(np.array([ref["score"]]))[0]
        assert np.array_equal(bits(got["final_params"][c]), bits(init[c])) and np.array_equal(bits(ref["final_params"]), bits(init[c]))
        assert (got["learn_step"][c] == 0).all() and (got["trace"]["reward"][c] == 0).all()      # nothing captured
    assert got["score"][0] != got["score"][1]


# ---- segments -------------------------------------------------------------------------------------------------------------------------------
def segments_equal_single(case, split, min_pending):
    from test_ppo_segments_gpu import REC_N_ROWS, Run, same_bits
    cfg, (theta, eps, sign, init, tapes), got, refs = case
    N = rows_of(cfg)
    trace_cap, learn_cap = caps(cfg, N)
    single = Run(cfg, CHAINS, theta, eps, sign, init, tapes=tapes, trace_cap=trace_cap, learn_cap=learn_cap).single()
    for k in ("score", "final_params", "learn_params"):                       # the launch the restatement was compared with
        assert np.array_equal(bits(single[k]), bits(got[k])), k
    pending = []
    run = Run(cfg, CHAINS, theta, eps, sign, init, tapes=tapes, trace_cap=trace_cap, learn_cap=learn_cap)
    seg = run.split(split, between=lambda il, b, e: pending.append(il.resume[:, REC_N_ROWS].cpu().tolist()))
    same_bits(single, seg, split)
    finished, status = run.il.segment_state()
    assert finished.tolist() == [1] * CHAINS and status.tolist() == [0] * CHAINS
    assert min(pending[0]) > min_pending, pending
    return pending


def test_segments_at_2048_rows():
    """boundaries behind episodes 6 and 11 of 21 (200 rows each): 1200 rows wait at the first, 152 at the second (one learn call lies between)"""
    pending = segments_equal_single(rows_case(2048), [6, 5, 10], 1000)
    assert pending == [[1200] * CHAINS, [152] * CHAINS, [104] * CHAINS]


def test_segments_at_width_33():
    """257 rows of width 33; boundaries behind episodes 2 and 5 of 9 (64 rows each): 128 and 63 rows wait"""
    pending = segments_equal_single(wide_case(33, "tanh"), [2, 3, 4], 100)
    assert pending == [[128] * CHAINS, [63] * CHAINS, [62] * CHAINS]
