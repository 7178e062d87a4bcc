"""PPO inner agent on the GPU: lenv_ppo_rn_inner_loop against the CPU restatement (tests/ppo_ref.c) bit for bit, the counter-RNG
properties of a launch, GTN_Master with `agent_name: ppo`, and the transfer experiment's entry points."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import ppo_ref
from learning_environments_amd import _lib

pytestmark = pytest.mark.gpu

ENVS = {"Pendulum-v0": (4, 3, 1, 2), "MountainCarContinuous-v0": (5, 2, 1, 2), "HalfCheetah-v3": (2, 17, 6, 17)}     # env id, S, A, state words


def make_cfg(env, rtype=2, k=1, L=2, H=64, act="relu", max_steps=12, ue=2.5, epochs=3, train_episodes=6, T=2, rn_hidden=16, rn_layers=1,
             rn_act="tanh", rng_mode=_lib.RNG_TAPE, solved_reward=1e9, init_episodes=0, early_out_num=3, lr=3e-3, action_std=0.5):
    env_id, S, A, _ = ENVS[env]
    return _lib.PpoCfg(env_id=env_id, state_dim=S, action_dim=A, max_steps=max_steps, rn_hidden=rn_hidden, rn_layers=rn_layers, rn_act=_lib.ACT[rn_act],
                       rn_prelu=0.25, reward_env_type=rtype, info_dim=4 if env == "HalfCheetah-v3" else 0, hidden=H, layers=L, act=_lib.ACT[act],
                       prelu=0.25, train_episodes=train_episodes, test_episodes=T, init_episodes=init_episodes, early_out_num=early_out_num,
                       ppo_epochs=epochs, same_action_num=k, rng_mode=rng_mode, solved_reward=solved_reward, gamma=0.99, lr=lr,
                       action_std=action_std, vf_coef=1.0, ent_coef=0.01, eps_clip=0.2, update_episodes=ue, adam_beta1=0.9, adam_beta2=0.999,
                       adam_eps=1e-8)


def make_inputs(cfg, env, chains, seed):
    """Per-chain reward nets (theta + eps rows), fresh agents and tapes from a numpy generator."""
    rng = np.random.RandomState(seed)
    _, S, A, SD = ENVS[env]
    L = _lib.lib()
    P = int(L.lenv_ppo_num_params(C.byref(cfg), None, None))
    p_rn = int(L.lenv_ppo_rn_num_params(C.byref(cfg)))
    assert P > 0 and p_rn >= 0
    theta = (rng.randn(max(p_rn, 1)) * 0.3).astype(np.float32)
    eps = (rng.randn(chains, max(p_rn, 1)) * 0.05).astype(np.float32)
    sign = np.array([(0.0, 1.0, -1.0)[c % 3] for c in range(chains)], np.float32)
    init = ((rng.rand(chains, P) * 2 - 1) * 0.3).astype(np.float32)
    init[:, :A] = np.float32(cfg.action_std)
    nag = -(-cfg.max_steps // max(1, cfg.same_action_num))
    E, T = cfg.train_episodes, cfg.test_episodes

    def resets(n):
        if env == "Pendulum-v0":
            return np.stack([rng.uniform(-np.pi, np.pi, (chains, n)), rng.uniform(-1, 1, (chains, n))], -1)
        if env == "MountainCarContinuous-v0":
            return np.stack([rng.uniform(-0.6, -0.4, (chains, n)), np.zeros((chains, n))], -1)
        return rng.uniform(-0.1, 0.1, (chains, n, SD))
    tapes = dict(act_noise=rng.randn(chains, E * nag, A).astype(np.float32), test_noise=rng.randn(chains, (E + 1) * T * nag, A).astype(np.float32),
                 train_reset=np.ascontiguousarray(resets(E), np.float64), test_reset=np.ascontiguousarray(resets((E + 1) * T), np.float64))
    return theta, eps, sign, init, tapes


def launch(cfg, chains, theta, eps, sign, init, tapes=None, keys=None, trace_cap=0, learn_cap=0):
    from learning_environments_amd.engine import PpoInnerLoop
    dev = torch.device("cuda")
    inner = PpoInnerLoop(cfg, chains, want_episode_stats=True, want_final_params=True, trace_cap=trace_cap, learn_cap=learn_cap)
    t = {k: torch.from_numpy(v).to(dev) for k, v in tapes.items()} if tapes is not None else None
    kt = torch.from_numpy(np.asarray(keys, np.uint64).view(np.int64)).to(dev) if keys is not None else None
    inner.run(torch.from_numpy(theta).to(dev), torch.from_numpy(eps).to(dev), torch.arange(chains, dtype=torch.int32, device=dev),
              torch.from_numpy(sign).to(dev), torch.from_numpy(init).to(dev), rng_keys=kt, tapes=t)
    torch.cuda.synchronize()
    out = dict(score=inner.score.cpu().numpy(), stats=inner.stats.cpu().numpy(), status=inner.status.cpu().numpy(),
               episode_test_mean=inner.episode_test_mean.cpu().numpy(), episode_len=inner.episode_len.cpu().numpy(),
               final_returns=inner.final_returns.cpu().numpy(), final_params=inner.final_params.cpu().numpy())
    if trace_cap:
        out["trace"] = {k: v.cpu().numpy() for k, v in inner.trace.items()}
    if learn_cap:
        out["learn_step"], out["learn_params"] = inner.learn_step.cpu().numpy(), inner.learn_params.cpu().numpy()
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_chain_equals_restatement(cfg, c, got, theta, eps, sign, init, tapes=None, key=0, trace_cap=0, learn_cap=0):
    w = (np.float32(sign[c]) * eps[c] + theta).astype(np.float32) if sign[c] != 0 else theta      # fma(sign, eps, theta) with sign in {0, 1, -1}: exact
    tp = {k: v[c] for k, v in tapes.items()} if tapes is not None else None
    ref = ppo_ref.chain(cfg, w, init[c], rng_key=key, tapes=tp, trace_cap=trace_cap, learn_cap=learn_cap)
    assert ref["rc"] == 0 and got["status"][c] == 0
    assert list(got["stats"][c]) == [ref["episodes_run"], ref["train_steps"], ref["learn_calls"], ref["test_steps"]]
    n = ref["trace"]["reward"].size
    if trace_cap:
        for k in ("state", "action", "next_state", "reward", "done"):
            assert np.array_equal(bits(got["trace"][k][c][:n]), bits(ref["trace"][k])), (k, c)
    if learn_cap:
        nl = ref["learn_step"].size
        assert nl == min(ref["learn_calls"], learn_cap) and np.array_equal(got["learn_step"][c][:nl], ref["learn_step"])
        for i in range(nl):
            assert np.array_equal(bits(got["learn_params"][c][i]), bits(ref["learn_params"][i])), "parameters after learn call %d of chain %d" % (i, c)
    assert np.array_equal(got["episode_len"][c], ref["episode_len"])
    assert np.array_equal(bits(got["episode_test_mean"][c]), bits(ref["episode_test_mean"]))
    assert np.array_equal(bits(got["final_returns"][c]), bits(ref["final_returns"]))
    assert np.array_equal(bits(got["final_params"][c]), bits(ref["final_params"]))
    assert bits(np.array([got["score"][c]]))[0] == bits(np.array([ref["score"]]))[0]
    return ref


CASES = [
    # env, reward type, same_action_num, hidden layers, width, activation, extra
    ("Pendulum-v0", 0, 1, 2, 64, "relu", {}),
    ("Pendulum-v0", 1, 5, 1, 128, "tanh", dict(max_steps=30, ue=1.5)),
    ("Pendulum-v0", 2, 1, 2, 128, "leakyrelu", dict(rn_layers=2, rn_act="prelu")),
    ("Pendulum-v0", 5, 5, 2, 64, "relu", dict(max_steps=32, ue=1.2)),
    ("Pendulum-v0", 6, 1, 1, 64, "tanh", {}),
    ("MountainCarContinuous-v0", 0, 5, 2, 64, "relu", dict(max_steps=40, ue=1.5)),
    ("MountainCarContinuous-v0", 1, 1, 1, 64, "leakyrelu", {}),
    ("MountainCarContinuous-v0", 2, 5, 2, 128, "tanh", dict(max_steps=45, ue=1.3)),
    ("MountainCarContinuous-v0", 5, 1, 2, 128, "relu", {}),
    ("MountainCarContinuous-v0", 6, 5, 1, 128, "relu", dict(max_steps=40, ue=2.0, rn_layers=2)),
    ("HalfCheetah-v3", 0, 1, 2, 128, "tanh", {}),
    ("HalfCheetah-v3", 1, 5, 2, 64, "relu", dict(max_steps=30, ue=1.4)),
    ("HalfCheetah-v3", 2, 1, 1, 64, "relu", dict(rn_act="prelu")),
    ("HalfCheetah-v3", 3, 1, 2, 64, "leakyrelu", {}),
    ("HalfCheetah-v3", 4, 5, 1, 128, "tanh", dict(max_steps=25, ue=1.6)),
    ("HalfCheetah-v3", 5, 1, 2, 64, "relu", {}),
    ("HalfCheetah-v3", 6, 1, 2, 64, "relu", {}),
    ("HalfCheetah-v3", 7, 1, 1, 64, "relu", dict(rn_layers=2)),
    ("HalfCheetah-v3", 8, 5, 2, 64, "tanh", dict(max_steps=25, ue=1.6)),
    ("HalfCheetah-v3", 101, 1, 2, 64, "relu", {}),
    ("HalfCheetah-v3", 102, 1, 1, 128, "leakyrelu", {}),
    # types 101 / 102 are Linear(info_dim, 1, bias=False) whatever the ENV section's hidden_layer says: theta stays in LDS
    ("HalfCheetah-v3", 101, 1, 2, 64, "relu", dict(rn_layers=2)),
    ("HalfCheetah-v3", 102, 5, 1, 64, "tanh", dict(rn_layers=3, max_steps=25, ue=1.6)),
]


@pytest.mark.parametrize("env,rtype,k,L,H,act,extra", CASES, ids=["%s-t%d-k%d-L%d-H%d-rn%d" % (c[0][:4], c[1], c[2], c[3], c[4], c[6].get("rn_layers", 1)) for c in CASES])
def test_kernel_equals_restatement_in_tape_mode(env, rtype, k, L, H, act, extra):
    cfg = make_cfg(env, rtype=rtype, k=k, L=L, H=H, act=act, **extra)
    chains = 3
    theta, eps, sign, init, tapes = make_inputs(cfg, env, chains, seed=1000 + 7 * rtype + k + L + H)
    got = launch(cfg, chains, theta, eps, sign, init, tapes=tapes, trace_cap=80, learn_cap=6)
    assert (got["status"] == 0).all()
    for c in range(chains):
        ref = assert_chain_equals_restatement(cfg, c, got, theta, eps, sign, init, tapes=tapes, trace_cap=80, learn_cap=6)
        assert ref["learn_calls"] >= 2 and ref["train_steps"] > ref["learn_step"][0]      # rows acted by the updated policy afterwards


def test_rows_not_a_multiple_of_the_row_block():
    """313 rows per learn call: one full 256-row block and a ragged one in every forward / input-gradient product, five 64-deep stages
    (the last one ragged) in every weight-gradient reduction."""
    cfg = make_cfg("Pendulum-v0", rtype=2, H=128, L=2, max_steps=60, ue=5.2, train_episodes=12, T=1, epochs=3)
    assert _lib.lib().lenv_ppo_rows(C.byref(cfg)) == 313
    theta, eps, sign, init, tapes = make_inputs(cfg, "Pendulum-v0", 2, seed=77)
    got = launch(cfg, 2, theta, eps, sign, init, tapes=tapes, trace_cap=720, learn_cap=3)
    for c in range(2):
        ref = assert_chain_equals_restatement(cfg, c, got, theta, eps, sign, init, tapes=tapes, trace_cap=720, learn_cap=3)
        assert list(ref["learn_step"]) == [313, 626]


def test_early_out():
    cfg = make_cfg("Pendulum-v0", rtype=2, train_episodes=6, solved_reward=-1e6, init_episodes=2, early_out_num=2)
    theta, eps, sign, init, tapes = make_inputs(cfg, "Pendulum-v0", 2, seed=78)
    got = launch(cfg, 2, theta, eps, sign, init, tapes=tapes, trace_cap=80, learn_cap=4)
    for c in range(2):
        ref = assert_chain_equals_restatement(cfg, c, got, theta, eps, sign, init, tapes=tapes, trace_cap=80, learn_cap=4)
        assert ref["episodes_run"] == 3 and np.isnan(got["episode_test_mean"][c][3:]).all() and (got["episode_len"][c][3:] == 0).all()


@pytest.mark.parametrize("env", sorted(ENVS))
def test_counter_rng_mode(env):
    """Two launches with the same keys are identical, different keys differ, chain c of a 48-chain launch equals the same key run alone --
    and equals the restatement fed that key."""
    cfg = make_cfg(env, rtype=2, rng_mode=_lib.RNG_COUNTER, k=5 if env != "Pendulum-v0" else 1, max_steps=20, ue=1.5, H=64)
    chains = 48
    theta, eps, sign, init, _ = make_inputs(cfg, env, chains, seed=5)
    init[:] = init[0]                                      # the same fresh agent everywhere: only the keys tell the chains apart
    eps[:] = 0
    keys = np.array([_lib.lib().lenv_chain_key(11, 0, c, 0) for c in range(chains)], np.uint64)
    a = launch(cfg, chains, theta, eps, sign, init, keys=keys, learn_cap=4)
    b = launch(cfg, chains, theta, eps, sign, init, keys=keys, learn_cap=4)
    assert (a["status"] == 0).all()
    for k in ("score", "final_params", "episode_test_mean", "learn_params", "learn_step", "final_returns", "stats"):
        assert np.array_equal(bits(a[k]) if a[k].dtype.kind == "f" else a[k], bits(b[k]) if b[k].dtype.kind == "f" else b[k]), k
    assert len(set(a["score"].tolist())) == chains
    other = launch(cfg, chains, theta, eps, sign, init, keys=keys[::-1].copy(), learn_cap=4)
    assert np.array_equal(bits(other["score"][::-1]), bits(a["score"])) and not np.array_equal(other["score"], a["score"])
    for c in (0, 17, 47):
        alone = launch(cfg, 1, theta, eps[c:c + 1], sign[c:c + 1], init[c:c + 1], keys=keys[c:c + 1], learn_cap=4)
        for k in ("score", "final_params", "episode_test_mean", "learn_params"):
            assert np.array_equal(bits(alone[k][0]), bits(a[k][c])), (k, c)
        assert_chain_equals_restatement(cfg, c, a, theta, eps, sign, init, key=int(keys[c]), learn_cap=4)


def _pendulum_ppo_config(num_workers=3, max_iterations=2):
    from learning_environments_amd.configs import pendulum_reward_env_td3
    cfg = pendulum_reward_env_td3(num_workers=num_workers, max_iterations=max_iterations)
    cfg["agents"]["gtn"].update(agent_name="ppo", quit_when_solved=False)
    cfg["agents"]["ppo"] = dict(train_episodes=4, test_episodes=2, init_episodes=0, update_episodes=1.5, ppo_epochs=3, gamma=0.99, lr=3e-3, vf_coef=1.0,
                                ent_coef=0.01, eps_clip=0.2, rb_size=100000, same_action_num=1, activation_fn="relu", hidden_size=64, hidden_layer=2,
                                action_std=0.5, print_rate=100, early_out_num=3, early_out_virtual_diff=0.02)
    cfg["envs"]["Pendulum-v0"].update(max_steps=16, hidden_size=32, hidden_layer=1)
    return cfg


def test_gtn_master_with_ppo_runs_two_generations(tmp_path, monkeypatch):
    from learning_environments_amd.agents.GTN import GTN_Master
    from learning_environments_amd.config import ppo_cfg_from_config
    from oracle import oracle as orc
    cfg = _pendulum_ppo_config()
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    m = GTN_Master(cfg, bohb_id=0, seed=5)
    assert m.task.name == "ppo_rn" and m.p_theta == 3 * 32 + 32 + 32 + 1 == m.inner.p_theta
    pcfg = ppo_cfg_from_config(cfg)
    theta0 = m.theta.cpu().numpy().copy()
    gathered = m.evaluate_population(0).cpu().numpy()
    eps = m.eps.cpu().numpy()
    oeps, init, okeys = orc.nes_draw(m.seed, 0, 3, m.p_theta, cfg["agents"]["gtn"]["noise_std"], 9, 3, 0, m.agent_bounds.cpu().numpy())
    assert np.array_equal(eps, oeps) and (init[:, 0] == 0).all()
    init[:, 0] = np.float32(0.5)                            # the action_std slot: its constant, not a draw
    best, orig = [], []
    for p in range(3):
        sc = []
        for kind, sg in enumerate((0.0, 1.0, -1.0)):
            w = (np.float32(sg) * eps[p] + theta0).astype(np.float32)
            sc.append(ppo_ref.chain(pcfg, w, init[3 * p + kind], rng_key=orc.chain_key(m.seed, 0, p, kind))["score"])
        assert gathered[p, 1] == sc[0] and gathered[p, 0] == max(sc[1], sc[2])
        best.append(max(sc[1], sc[2]))
        orig.append(sc[0])
    assert (gathered[:, 3] == 0).all() and np.array_equal(np.argsort(gathered[:, 0]), np.argsort(best))      # ranks agree with the restatement
    mean_score, mean_list, _ = m.run()
    assert len(mean_list) == 2 and np.isfinite(mean_score) and np.isfinite(mean_list).all()
    assert not np.array_equal(m.theta.cpu().numpy(), theta0)


def _reward_env_and_real_env(cfg, seed):
    from learning_environments_amd.envs.env_factory import EnvFactory
    torch.manual_seed(seed)
    fac = EnvFactory(copy.deepcopy(cfg))
    return fac.generate_reward_env(), fac.generate_real_env()


SMALL = dict(train_episodes=3, update_episodes=1, ppo_epochs=2)


def test_transfer_algo_equals_single_chain_launches():
    """train_test_agents for modes 0 and 2 equals, agent for agent, single-chain launches with the same keys; the many-models launch equals the
    per-model calls."""
    from learning_environments_amd.experiments import transfer_algo as ta
    env_name = "MountainCarContinuous-v0"
    base = ta.base_config(env_name)
    base["envs"][env_name].update(max_steps=60, hidden_size=32)
    envs = [_reward_env_and_real_env(base, s) for s in (1, 2)]
    real_env = envs[0][1]
    for mode in ("0", "2"):
        cfg = copy.deepcopy(base)
        (rewards, lengths), last = ta.train_test_agents(mode, envs[0][0], real_env, cfg, env_name, agents_num=3, seed=9, settings=SMALL, details=True)
        assert cfg["agents"]["ppo"]["ppo_epochs"] == 2 and cfg["agents"]["ppo"]["same_action_num"] == 5 and len(rewards) == len(lengths) == 3
        assert all(len(r) == 3 and np.isfinite(r).all() for r in rewards) and all(sum(l) > 0 for l in lengths)
        pcfg = last["task"].cfg
        assert pcfg.reward_env_type == int(mode)
        theta = last["theta"].cpu().numpy()
        init = last["agent_init"].cpu().numpy()
        for i in range(3):
            one = launch(pcfg, 1, theta, np.zeros((1, theta.size), np.float32), np.zeros(1, np.float32), init[i:i + 1], keys=last["keys"][i:i + 1])
            n = int(one["stats"][0, 0])
            assert one["episode_test_mean"][0][:n].tolist() == rewards[i] and one["episode_len"][0][:n].tolist() == lengths[i]
    cfg = copy.deepcopy(base)
    both = ta.train_test_agents_models("2", [e[0] for e in envs], real_env, cfg, env_name, agents_num=2, seed=9, settings=SMALL)
    for mi in range(2):
        single = ta.train_test_agents("2", envs[mi][0], real_env, copy.deepcopy(base), env_name, agents_num=2, seed=9, model_index=mi, settings=SMALL)
        assert both[mi] == single
    assert both[0] != both[1]
    with pytest.raises(NotImplementedError, match="ppo_icm"):
        ta.train_test_agents("-1", envs[0][0], real_env, copy.deepcopy(base), env_name)


def test_load_envs_and_config_reads_a_reference_written_checkpoint(golden):
    """(on the GPU machine: the real env of the pair allocates its state on the device)  transfer_algo.load_envs_and_config on a reward-net checkpoint the reference wrote ({'model', 'config'}): the weights arrive in the reward
    net, solved_reward is raised out of the early out's reach like the scripts do, and the pair is what train_test_agents takes."""
    import os
    import torch
    from learning_environments_amd.experiments import transfer_algo as ta
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ckpt_cmc_reward_env_reference.pt")
    reward_env, real_env, config = ta.load_envs_and_config(path)
    g = golden("ckpt_cmc_reward_env_reference_theta")
    assert config["env_name"] == "MountainCarContinuous-v0" and config["envs"]["MountainCarContinuous-v0"]["solved_reward"] == 100000
    assert not reward_env.is_virtual_env() and not real_env.is_virtual_env()
    flat = np.concatenate([np.concatenate([m.weight.detach().numpy().reshape(-1), m.bias.detach().numpy().reshape(-1)])
                           for m in reward_env.env.reward_net.modules() if isinstance(m, torch.nn.Linear)])
    assert np.array_equal(flat, g["theta"])
    cfg, _ = ta._task_config("0", reward_env, config)
    assert cfg["envs"]["MountainCarContinuous-v0"]["reward_env_type"] == 0 and cfg["agents"]["gtn"]["agent_name"] == "ppo"
    with pytest.raises(ValueError, match="mode 5"):
        ta._task_config("5", reward_env, config)        # the model is a type-2 reward net
    with pytest.raises(NotImplementedError, match="ppo_icm"):
        ta.train_test_agents("-1", reward_env, real_env, config)
    rewards, lengths = ta.train_test_agents("2", reward_env, real_env, config, agents_num=2, settings=dict(train_episodes=2, update_episodes=1, ppo_epochs=2))
    assert len(rewards) == 2 and all(len(r) == 2 and np.isfinite(r).all() for r in rewards) and all(sum(l) > 0 for l in lengths)
