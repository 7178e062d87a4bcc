"""Test-side composer of one TD3_discrete_vary chain in tape mode (not collected by pytest).

A Python restatement of `orc_td3d_chain` (oracle/lenv_oracle_td3d.inc), step for step, built only from pinned primitives of the oracle
library: `orc_td3d_actor_forward`, `orc_td3d_learn` and `orc_td3d_temperature` for the agent, and an env object for the training env.
Every value the C code keeps in a `float` is a numpy float32 scalar or array here, every `double` a Python float.

Two training envs:
  VirtualEnvStep  -- the three SE nets through `orc_se_step_population` (what `orc_td3d_chain` does: the composer is checked against it)
  RewardEnvStep   -- RewardEnv over the real env (reference envs/reward_env.py:61-133, the DDQN oracle chain's `reward_env` branch): the real
                     env's fp64 physics (`orc_cartpole_step` / `orc_acrobot_step` / `orc_mountaincar_step`, TimeLimit done at max_steps) and
                     the reward through `orc_rn_shape_rows`; reward type 0 = the real env itself
"""
import ctypes as C

import numpy as np

from oracle import oracle as orc

f32 = np.float32
CARTPOLE, ACROBOT, MOUNTAINCAR = 0, 1, 3
TAPE_KEYS = ("rand_action", "act_noise", "test_noise", "policy_noise", "gumbel_act", "gumbel_test", "gumbel_target", "gumbel_actor",
             "replay_idx", "train_reset", "test_reset")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def real_obs(env_id, st):
    """real_env_obs: the fp32 observation of the fp64 env state"""
    if env_id == CARTPOLE:
        return st[:4].astype(f32)
    if env_id == MOUNTAINCAR:
        return st[:2].astype(f32)
    o = np.zeros(6, np.float64)
    orc.lib().orc_acrobot_obs(_dp(st), _dp(o))
    return o.astype(f32)


def real_step(env_id, st, action):
    """one step of the real env on st (float64[4], updated in place) -> (reward as a double, done)"""
    fn = {CARTPOLE: "orc_cartpole_step", ACROBOT: "orc_acrobot_step", MOUNTAINCAR: "orc_mountaincar_step"}[env_id]
    rew, dn = C.c_double(), C.c_int()
    getattr(orc.lib(), fn)(_dp(st), C.c_int(int(action)), C.byref(rew), C.byref(dn))
    return rew.value, int(dn.value)


def argmax_first(v):
    best = 0
    for k in range(1, len(v)):
        if v[k] > v[best]:
            best = k
    return best


def seq_sum(v):
    s = 0.0
    for x in v:
        s += x
    return s


def mean_seq(v):
    return seq_sum(v) / len(v)


def meter_env_solved(meter, num, virtual_rule, solved_reward, virtual_diff, episode, init_episodes):
    n = len(meter)
    lo = max(n - num, 0)
    avg = seq_sum(meter[lo:n]) / ((n - lo) + 1e-9)
    if not virtual_rule:
        return avg >= solved_reward
    hi2, lo2 = max(n - num, 0), max(n - 2 * num, 0)
    last = seq_sum(meter[lo2:hi2]) / ((hi2 - lo2) + 1e-9)
    return abs(avg - last) / (abs(last) + 1e-9) < virtual_diff and episode >= init_episodes + num


class VirtualEnvStep(object):
    """VirtualEnv.step on cat(one_hot(action), state) (envs/virtual_env.py:43-54); reward / done see the pre-transition state"""
    virtual = True

    def __init__(self, cfg, se_params):
        self.descs = orc.se_descs(cfg.state_dim, cfg.action_dim, cfg.se_hidden, cfg.se_layers, cfg.se_act, cfg.se_prelu)
        self.theta = np.ascontiguousarray(se_params, f32)
        self.env_id = cfg.env_id

    def reset(self, st4):
        self.state = real_obs(self.env_id, np.array(st4, np.float64))
        return self.state

    def step(self, a_idx):
        ns, r, d = orc.se_step_population(self.descs, self.theta, None, None, None, self.state[None], np.array([a_idx], np.int32))
        self.state = ns[0]
        return ns[0], f32(r[0]), f32(d[0])


class RewardEnvStep(object):
    """RewardEnv(real env).step (reward_env.py:61-66): the real transition, TimeLimit done at max_steps, _calc_reward (:68-133)"""
    virtual = False

    def __init__(self, cfg, rtype, rn_params, rn_hidden, rn_layers, rn_act, rn_prelu=0.25):
        self.cfg, self.rtype = cfg, int(rtype)
        self.rn = (rn_hidden, rn_layers, rn_act, rn_prelu)
        self.theta = np.ascontiguousarray(rn_params, f32)

    def reset(self, st4):
        self.st = np.array(st4, np.float64)
        self.steps = 0
        self.state = real_obs(self.cfg.env_id, self.st)
        return self.state

    def step(self, a_idx):
        cfg = self.cfg
        rew, dn = real_step(cfg.env_id, self.st, a_idx)
        self.steps += 1
        if self.steps >= cfg.max_steps:
            dn = 1
        ns = real_obs(cfg.env_id, self.st)
        r32 = f32(rew)
        if self.rtype == 0:
            shaped = r32
        else:
            H, L, act, pr = self.rn
            shaped = f32(orc.rn_shape_rows(self.rtype, cfg.state_dim, 0, H, L, act, pr, cfg.gamma, self.theta, self.state[None], ns[None],
                                           None, np.array([r32], f32))[0])
        self.state = ns
        return ns, shaped, f32(1.0 if dn else 0.0)


def td3d_chain(cfg, env, agent_init, tapes):
    """orc_td3d_chain in tape mode (step_budget 0) with `env` as the training env.  Returns the dict orc.td3d_chain returns (no trace)."""
    assert cfg.rng_mode == 1 and cfg.step_budget == 0
    S, A, B, T, E = cfg.state_dim, cfg.action_dim, cfg.batch_size, cfg.test_episodes, cfg.train_episodes
    P, Pa, _ = orc.td3d_num_params(cfg)
    t = {k: np.asarray(tapes[k]) for k in TAPE_KEYS}
    cap = max(min(E * cfg.max_steps, cfg.rb_size), 1)
    RS = 2 * S + A + 2
    params = np.array(agent_init, f32).reshape(-1)[:P].copy()
    targets = params.copy()
    am, av = np.zeros(P, f32), np.zeros(P, f32)
    pows = [1.0] * 4
    rb = np.zeros((cap, RS), f32)
    st = dict(n_rand=0, n_actn=0, n_testn=0, n_test_ep=0, learn_it=0, policy_it=0, train_steps=0, test_steps=0, rb_ptr=0, rb_size=0)
    astd = f32(cfg.action_std)
    temp = [f32(orc.td3d_temperature(cfg, 0))]

    def row(name, i, n=1):
        if i + n > t[name].shape[0]:
            raise IndexError("tape %s underrun" % name)
        return t[name][i:i + n]

    def policy_action(obs, gum, noise):
        pa = orc.td3d_actor_forward(cfg, params[:Pa], obs[None], gum[None], float(temp[0]))[0]
        return (pa + noise.astype(f32) * astd).astype(f32)

    def test_phase():
        rets = []
        for _ in range(T):
            xs = np.array(row("test_reset", st["n_test_ep"])[0], np.float64)
            st["n_test_ep"] += 1
            ep_reward = f32(0.0)
            for _tt in range(cfg.max_steps):
                o = real_obs(cfg.env_id, xs)
                n = st["n_testn"]
                act = policy_action(o, row("gumbel_test", n)[0], row("test_noise", n)[0])
                st["n_testn"] += 1
                rew, dn = real_step(cfg.env_id, xs, argmax_first(act))
                ep_reward = f32(ep_reward + f32(rew))
                st["test_steps"] += 1
                if dn:
                    break
            rets.append(float(ep_reward))
        return rets

    ep_mean = np.full(max(E, 1), np.nan)
    ep_len_out = np.zeros(max(E, 1), np.int32)
    meter = []
    episodes_run = 0
    for episode in range(E):
        state = env.reset(row("train_reset", episode)[0])
        ep_len, tr_reward = 0, f32(0.0)
        for _step in range(cfg.max_steps):
            if episode < cfg.init_episodes:
                idx = int(row("rand_action", st["n_rand"])[0])
                st["n_rand"] += 1
                if not 0 <= idx < A:
                    raise ValueError("random action out of range")
                action = np.array([1.0 if k == idx else 0.0 for k in range(A)], f32)
            else:
                n = st["n_actn"]
                action = policy_action(state, row("gumbel_act", n)[0], row("act_noise", n)[0])
                st["n_actn"] += 1
            ns, shaped, done_f = env.step(argmax_first(action))
            dn = done_f > f32(0.5)
            rb[st["rb_ptr"]] = np.concatenate([state, action, ns, np.array([shaped, done_f], f32)])
            st["rb_ptr"] = (st["rb_ptr"] + 1) % cap
            st["rb_size"] = min(st["rb_size"] + 1, cap)
            state = ns
            tr_reward = f32(tr_reward + shaped)
            ep_len += 1
            st["train_steps"] += 1
            if episode >= cfg.init_episodes:
                li, pi = st["learn_it"], st["policy_it"]
                policy_step = (li + 1) % cfg.policy_delay == 0
                idx = row("replay_idx", li * B, B).astype(np.int64)
                if idx.min() < 0 or idx.max() >= st["rb_size"]:
                    raise ValueError("replay index out of range")
                batch = rb[idx]
                pn, gt = row("policy_noise", li * B, B), row("gumbel_target", li * B, B)
                ga = row("gumbel_actor", pi * B, B) if policy_step else np.zeros((B, A), f32)
                temp[0] = f32(orc.td3d_temperature(cfg, li))
                st["learn_it"] += 1
                params, targets, am, av, pows = orc.td3d_learn(cfg, params, targets, am, av, pows, st["learn_it"], batch, pn, gt, ga)
                if policy_step:
                    st["policy_it"] += 1
            if dn:
                break
        episodes_run += 1
        ep_len_out[episode] = ep_len
        tm = float(tr_reward) if cfg.test_mode == 1 else mean_seq(test_phase())
        meter.append(tm)
        ep_mean[episode] = tm
        if episode >= cfg.init_episodes and meter_env_solved(meter, cfg.early_out_num, cfg.test_mode == 1 and env.virtual, cfg.solved_reward,
                                                             cfg.early_out_virtual_diff, episode, cfg.init_episodes):
            break
    rets = test_phase()
    return dict(rc=0, score=mean_seq(rets), episodes_run=episodes_run, train_steps=st["train_steps"], learn_steps=st["learn_it"],
                test_steps=st["test_steps"], episode_test_mean=ep_mean[:E], episode_len=ep_len_out[:E], final_test_returns=np.array(rets),
                final_params=params)


def make_tapes(rng, cfg, n_learn_rows=None):
    """Random tapes long enough for any run of cfg: every replay index valid whatever the episodes' lengths (index < min(k + 1, capacity) at
    learn call k), resets drawn from the env's own reset ranges."""
    S, A, B, T, E, M = cfg.state_dim, cfg.action_dim, cfg.batch_size, cfg.test_episodes, cfg.train_episodes, cfg.max_steps
    cap = max(min(E * M, cfg.rb_size), 1)
    n_act, n_test, n_learn = E * M, (E + 1) * T * M, (E * M if n_learn_rows is None else n_learn_rows)

    def gumbel(n):
        u = rng.uniform(1e-6, 1 - 1e-6, (n, A))
        return (-np.log(-np.log(u))).astype(f32)

    def normal(n):
        return rng.randn(n, A).astype(f32)

    def resets(n):
        if cfg.env_id == MOUNTAINCAR:
            r = np.zeros((n, 4))
            r[:, 0] = rng.uniform(-0.6, -0.4, n)
            return r
        lim = 0.05 if cfg.env_id == CARTPOLE else 0.1
        return rng.uniform(-lim, lim, (n, 4))
    k = np.repeat(np.arange(n_learn), B)
    replay = np.floor(rng.uniform(0, 1, n_learn * B) * np.minimum(k + 1, cap)).astype(np.int32)
    return dict(rand_action=rng.randint(0, A, max(cfg.init_episodes * M, 1)).astype(np.int32), act_noise=normal(n_act), gumbel_act=gumbel(n_act),
                test_noise=normal(n_test), gumbel_test=gumbel(n_test), policy_noise=normal(n_learn * B), gumbel_target=gumbel(n_learn * B),
                gumbel_actor=gumbel(n_learn * B), replay_idx=replay, train_reset=resets(max(E, 1)), test_reset=resets((E + 1) * T))
