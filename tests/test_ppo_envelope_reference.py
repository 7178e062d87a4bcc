"""The PPO restatement (tests/ppo_ref.c) against an fp64 PPO.learn written here with torch autograd, at the widths and row counts where only
"kernel equals restatement" stood before, and the row counts of tests/test_ppo_envelope_gpu.py checked on the CPU.

The fp64 learn follows the algorithm as DESIGN.md section 4 and the kernel's header describe it: the discounted returns scan that restarts at a
done row, (R - mean) / (std + 1e-5) with the unbiased std; a tanh-mean Gaussian actor with the action_std parameter, a value critic; the loss
-min(ratio * A, clip(ratio) * A) + vf_coef * (V - R)^2 - ent_coef * entropy averaged over the rows, A = R - V detached; one Adam step per
epoch; actor_old's action_std floored at 0.001 where it acts, the actor's floored at 0.01 in place behind the log-probabilities of an epoch.
It is fed the rows [0, N) of the restatement's trace (state, action, reward, done) and the chain's fresh parameters, and the parameters
after the first learn call are compared.

Yardstick (the issue's rule: the bound is not chosen, it is 4 x what the same comparison gives where the restatement is pinned already): the five
g14 fixtures pin the restatement to the reference's own PPO.train within 1.67e-6; they are 24 wide, so the yardstick runs each fixture's config,
reward net and tapes (11, 13, 19, 21 and 28 rows per learn call) with a fresh agent of hidden 64.  Two figures per comparison: the maximum of
|restatement - fp64| over the parameters, and its 99.9th percentile.  The maximum is set by single parameters whose gradient is of the order
of Adam's eps (1e-8), where g / (sqrt(v) + eps) turns an fp32 rounding of g into a visible part of a step of lr; the percentile is what
all the others do.  Measured when the test was written:

                                              maximum     99.9th percentile    wrong fp64 learn (maximum)
    yardstick, hidden 64    g14p (28 rows)    1.001e-05   4.37e-08             1.86e-02
                            g14c (13 rows)    3.81e-08    3.75e-08             1.20e-02
                            g14h (19 rows)    1.206e-06   1.323e-07            1.98e-02
                            g14s (21 rows)    6.85e-08    4.88e-08             2.38e-02
                            g14f (11 rows)    1.60e-08    1.51e-08             1.94e-02
    (the fixtures as they are, hidden 24:     2.22e-07 at the most, 8.24e-08)
    YARDSTICK = 1.01e-05, YARDSTICK_999 = 1.33e-07;  BOUND = 4 x = 4.04e-05, BOUND_999 = 4 x = 5.32e-07
    new shapes      H1-L1       2.19e-08    8.47e-09    9.01e-03        H33-L1        5.06e-08    3.76e-08    1.77e-02
                    H1-L2       5.96e-08    3.44e-08    9.01e-03        H33-L2        3.66e-08    3.44e-08    1.44e-02
                    H15-L1      2.05e-08    1.76e-08    9.00e-03        H100-L1       4.63e-08    3.50e-08    1.78e-02
                    H15-L2      3.52e-08    3.43e-08    1.76e-02        H100-L2       1.96e-07    6.72e-08    1.73e-02
                    H33-L2-N257 4.91e-08    3.58e-08    1.70e-02        H128-L2-N2048 1.160e-05   4.02e-08    1.74e-02
The 4 x covers the longer row sums (sqrt(2048 / 40) is about 7 in the worst case); 2048 rows stay inside it and need no yardstick of their own.

The test has to bite.  Two deliberately wrong fp64 learns: in one the last hidden unit does not reach the output layer of either net, in the
other the last row is left out of the sums over the rows.  The first must miss BOUND by 10 x or more at every shape, the yardstick's included
(measured: 200 x and more, last column above).  The second moves every gradient by a part in N, which Adam's normalised steps shrink further:
it misses BOUND_999 by 10 x or more at every shape (measured: 40 x at H15-L1, 54 x at H1-L1, 600 x and more elsewhere), while against BOUND,
which one parameter with a tiny gradient sets, it would pass at H15-L1 (2.2e-05) -- the reason the percentile is asserted too."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import ppo_ref
from learning_environments_amd import _lib
from learning_environments_amd.config import ppo_cfg_from_config
from test_ppo_gpu import make_cfg, make_inputs

FIXTURES = ["g14p_ppo_pendulum_type2", "g14c_ppo_cmc_type5_k5", "g14h_ppo_cheetah_type0", "g14s_ppo_pendulum_std_floor",
            "g14f_ppo_pendulum_std_forward_floor"]
ACT_NAME = {v: k for k, v in _lib.ACT.items()}


def fp64_learn(cfg, init, state, action, reward, done, wrong=None):
    """PPO.learn in float64 with autograd on the rows given; returns the flat parameters (action_std | actor.net | critic.net) after it.
    wrong = "unit": the last hidden unit does not reach the output layer (both nets); wrong = "row": the last row is left out of the sums."""
    dt = torch.float64
    S, A, H, L = cfg.state_dim, cfg.action_dim, cfg.hidden, cfg.layers
    flat = torch.tensor(np.asarray(init, np.float64), dtype=dt)
    pos = [A]

    def take(*shape):
        n = int(np.prod(shape))
        t = flat[pos[0]:pos[0] + n].reshape(shape).clone().requires_grad_(True)
        pos[0] += n
        return t

    def net(out):
        layers, n_in = [], S
        for _ in range(L):
            layers.append((take(H, n_in), take(H)))
            n_in = H
        layers.append((take(out, H), take(out)))
        return layers
    std = flat[:A].clone().requires_grad_(True)
    actor, critic = net(A), net(1)
    assert pos[0] == flat.numel()
    leaves = [std] + [t for wb in actor for t in wb] + [t for wb in critic for t in wb]
    fn = {"relu": torch.relu, "tanh": torch.tanh, "leakyrelu": lambda z: torch.nn.functional.leaky_relu(z, 0.01)}[ACT_NAME[cfg.act]]

    def forward(layers, x):
        for W, b in layers[:-1]:
            x = fn(x @ W.t() + b)
        W, b = layers[-1]
        if wrong == "unit":
            return x[:, :-1] @ W[:, :-1].t() + b
        return x @ W.t() + b

    x = torch.tensor(np.asarray(state, np.float64), dtype=dt)
    a = torch.tensor(np.asarray(action, np.float64), dtype=dt)
    n = x.shape[0]
    ret, disc = torch.zeros(n, dtype=dt), 0.0
    for i in range(n - 1, -1, -1):
        if done[i] > 0.5:
            disc = 0.0
        disc = float(reward[i]) + cfg.gamma * disc
        ret[i] = disc
    ret = (ret - ret.mean()) / (ret.std() + 1e-5)
    keep = slice(0, n - 1) if wrong == "row" else slice(0, n)
    with torch.no_grad():                                   # actor_old: the same net before the first call, its own std floored where it acted
        std_old = std.clamp(min=0.001)
        old_lp = torch.distributions.Normal(torch.tanh(forward(actor, x)), std_old).log_prob(a).sum(-1)
    opt = torch.optim.Adam(leaves, lr=cfg.lr, betas=(cfg.adam_beta1, cfg.adam_beta2), eps=cfg.adam_eps)
    for _ in range(cfg.ppo_epochs):
        dist = torch.distributions.Normal(torch.tanh(forward(actor, x)), std)
        lp = dist.log_prob(a).sum(-1)
        std.data.clamp_(min=0.01)                           # in place behind the log-probabilities: the entropy and the backward pass see it
        entropy = dist.entropy().sum(-1)
        v = forward(critic, x)[:, 0]
        ratio = torch.exp(lp - old_lp)
        adv = ret - v.detach()
        surr = torch.min(ratio * adv, torch.clamp(ratio, 1.0 - cfg.eps_clip, 1.0 + cfg.eps_clip) * adv)
        loss = (-surr + cfg.vf_coef * (v - ret) ** 2 - cfg.ent_coef * entropy)[keep].sum() / n
        opt.zero_grad()
        loss.backward()
        opt.step()
    return torch.cat([t.detach().reshape(-1) for t in leaves]).numpy()


def first_call(cfg, rn, init, tapes):
    """The restatement up to and including its first learn call: the rows it learned from and the parameters behind it."""
    N = ppo_ref.rows(cfg)
    out = ppo_ref.chain(cfg, rn, init, tapes=tapes, trace_cap=N, learn_cap=1)
    assert out["rc"] == 0 and out["learn_calls"] >= 1 and out["learn_step"][0] == N and out["trace"]["reward"].size == N
    return N, out["trace"], out["learn_params"][0].astype(np.float64)


def p999(d):
    return np.percentile(d, 99.9, method="lower")


def distances(cfg, rn, init, tapes):
    """(N, d, d999, unit, row999): |restatement - fp64| over the parameters after the first learn call, its maximum and its 99.9th percentile
    (every parameter but one in a thousand, and but the farthest one of a small net, lies within it); the maximum against the fp64 learn
    that is wrong by a hidden unit; the 99.9th percentile against the one that is wrong by a row"""
    N, tr, got = first_call(cfg, rn, init, tapes)
    rows = (tr["state"], tr["action"], tr["reward"], tr["done"])
    moved = np.abs(got - np.asarray(init, np.float64)).max()
    assert moved > 0.5 * cfg.lr                               # the call moved the parameters: Adam's first steps are about lr each
    d = np.abs(got - fp64_learn(cfg, init, *rows))
    return (N, d.max(), p999(d), np.abs(got - fp64_learn(cfg, init, *rows, wrong="unit")).max(),
            p999(np.abs(got - fp64_learn(cfg, init, *rows, wrong="row"))))


# ---- the yardstick: hidden 64 at the fixtures' row counts, where the restatement is pinned to the reference's own runs --------------------------
YARDSTICK, YARDSTICK_999 = 1.01e-5, 1.33e-7               # the worst of the five measured values of the header, rounded up in the third digit
BOUND, BOUND_999 = 4 * YARDSTICK, 4 * YARDSTICK_999
MISS = 10                                                 # the wrong fp64 learn has to miss BOUND by this factor


def fixture_distance(golden, name, hidden=None):
    """hidden None: the fixture as it is (its own fresh agent, hidden 24); hidden 64: the fixture's config, reward net and tapes with a fresh
    agent of that width drawn here (uniform in +-0.3, action_std at its configured value)"""
    g = golden(name)
    over = {} if hidden is None else dict(hidden=hidden)
    cfg = ppo_cfg_from_config(json.loads(str(g["config_json"])), rng_mode=_lib.RNG_TAPE, **over)
    tapes = dict(act_noise=g["tape_act_noise"], test_noise=g["tape_test_noise"], train_reset=g["tape_train_reset"], test_reset=g["tape_test_reset"])
    init = g["agent_init"]
    if hidden is not None:
        init = ((np.random.RandomState(len(name)).rand(ppo_ref.num_params(cfg)) * 2 - 1) * 0.3).astype(np.float32)
        init[:cfg.action_dim] = np.float32(cfg.action_std)
    return distances(cfg, g["theta"], init, tapes)


# ---- the new shapes ---------------------------------------------------------------------------------------------------------------------------
# name: (env, reward type, hidden layers, width, activation, extra make_cfg arguments, rows)
PEND, CMC, CHEETAH = "Pendulum-v0", "MountainCarContinuous-v0", "HalfCheetah-v3"
SMALL = dict(max_steps=16, ue=2.5, train_episodes=3, T=1)            # 41 rows
SHAPES = {
    "H1-L1": (PEND, 2, 1, 1, "tanh", SMALL, 41),
    "H1-L2": (CHEETAH, 0, 2, 1, "leakyrelu", SMALL, 41),
    "H15-L1": (CMC, 2, 1, 15, "relu", SMALL, 41),
    "H15-L2": (PEND, 2, 2, 15, "tanh", SMALL, 41),
    "H33-L1": (CHEETAH, 2, 1, 33, "leakyrelu", SMALL, 41),
    "H33-L2": (CMC, 2, 2, 33, "tanh", SMALL, 41),
    "H100-L1": (PEND, 2, 1, 100, "relu", SMALL, 41),
    "H100-L2": (CHEETAH, 2, 2, 100, "relu", SMALL, 41),
    "H33-L2-N257": (PEND, 2, 2, 33, "tanh", dict(max_steps=64, ue=4.0, train_episodes=5, T=1), 257),
    "H128-L2-N2048": (PEND, 2, 2, 128, "relu", dict(max_steps=200, ue=10.2375, train_episodes=11, T=1), 2048),
}


def shape_distance(name):
    env, rtype, L, H, act, extra, N = SHAPES[name]
    cfg = make_cfg(env, rtype=rtype, L=L, H=H, act=act, epochs=3, **extra)
    assert ppo_ref.rows(cfg) == N == _lib.lib().lenv_ppo_rows(C.byref(cfg))
    theta, eps, sign, init, tapes = make_inputs(cfg, env, 1, seed=4000 + 10 * H + L)
    n, d, d999, unit, row999 = distances(cfg, theta, init[0], {k: v[0] for k, v in tapes.items()})
    assert n == N
    return d, d999, unit, row999


def report(what, n, d, d999, unit, row999):
    print("%s, %d rows: max %.3e  99.9%% %.3e | wrong by a unit: max %.3e  wrong by a row: 99.9%% %.3e" % (what, n, d, d999, unit, row999))


def assert_bites(unit, row999):
    assert unit >= MISS * BOUND and row999 >= MISS * BOUND_999


@pytest.mark.parametrize("name", FIXTURES)
def test_yardstick_at_hidden_64(golden, name):
    n, d, d999, unit, row999 = fixture_distance(golden, name, hidden=64)
    report(name + " at hidden 64", n, d, d999, unit, row999)
    assert d <= YARDSTICK and d999 <= YARDSTICK_999       # the recorded figures still hold: the bounds below rest on them
    assert_bites(unit, row999)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_as_they_are(golden, name):
    """hidden 24, the fresh agent the reference itself trained: where restatement, reference run and fp64 learn all meet"""
    n, d, d999, unit, row999 = fixture_distance(golden, name)
    report(name + " as it is (hidden 24)", n, d, d999, unit, row999)
    assert d <= YARDSTICK and d999 <= YARDSTICK_999
    assert_bites(unit, row999)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_restatement_against_fp64_learn(name):
    d, d999, unit, row999 = shape_distance(name)
    report(name, SHAPES[name][6], d, d999, unit, row999)
    assert d <= BOUND and d999 <= BOUND_999
    assert_bites(unit, row999)


def test_shapes_cover_what_they_are_for():
    assert {(v[3], v[2]) for v in SHAPES.values() if v[6] == 41} == {(h, l) for h in (1, 15, 33, 100) for l in (1, 2)}
    assert ("H33-L2-N257" in SHAPES) and SHAPES["H128-L2-N2048"][2:4] == (2, 128) and SHAPES["H128-L2-N2048"][6] == 2048
    assert {v[0] for v in SHAPES.values()} == {PEND, CMC, CHEETAH} and {v[4] for v in SHAPES.values()} == {"relu", "leakyrelu", "tanh"}


def test_rows_of_the_gpu_envelope_cases():
    """lenv_ppo_rows needs no device: every case of tests/test_ppo_envelope_gpu.py gives exactly the N it names (the reference's own float
    comparison, time_step / max_steps > update_episodes), and the groups cover the widths, layers, activations and envs they are there for."""
    import test_ppo_envelope_gpu as G
    L = _lib.lib()

    def rows(cfg):
        assert L.lenv_ppo_rows(C.byref(cfg)) == ppo_ref.rows(cfg)
        return ppo_ref.rows(cfg)
    for env, rtype, k, layers, H, act, N, extra in G.WIDTHS:
        assert rows(make_cfg(env, rtype=rtype, k=k, L=layers, H=H, act=act, **extra)) == N
    assert {(c[4], c[3]) for c in G.WIDTHS} == {(h, l) for h in (1, 3, 15, 17, 33, 100, 127) for l in (1, 2)}
    assert {c[5] for c in G.WIDTHS} == {"relu", "leakyrelu", "tanh"}
    for env in (PEND, CMC, CHEETAH):                      # state_dim 3, 2 and 17 each meet odd widths
        assert len({c[4] for c in G.WIDTHS if c[0] == env and c[4] % 2}) >= 3
    assert rows(make_cfg(PEND, H=33, **G.WIDE_ROWS)) == 257 == rows(make_cfg(PEND, H=1, **G.WIDE_ROWS))
    assert sorted(G.ROWS) == [2, 64, 65, 255, 256, 257, 512, 513, 1999, 2047, 2048]
    for N in G.ROWS:
        for H in (128, 64):
            cfg = make_cfg(PEND, **G.rows_cfg_args(N, H))
            assert rows(cfg) == N and (cfg.hidden, cfg.layers) == (H, 2)
            assert 2 * N < cfg.train_episodes * cfg.max_steps < 3 * N or N == 2      # two learn calls and rows behind them
    for name, (env, N, over) in G.NAMED.items():
        assert rows(make_cfg(env, **over)) == N, name
    assert rows(G.rn_cfg(100, 3)) == 31
