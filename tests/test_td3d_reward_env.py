"""TD3_discrete_vary trained on RewardEnv(real env) or on the real env itself (lenv_td3d_rn_inner_loop).

The oracle has no TD3_discrete chain on a RewardEnv, so the anchor is the test-side composer of tests/td3d_composer.py, built from pinned
oracle primitives only.  CPU: the composer equals orc_td3d_chain bit for bit on the VirtualEnv (so it is faithful), and the host routes and
refuses as it should.  GPU: the RENV launch in tape mode equals the composer over real physics + orc_rn_shape_rows bit for bit; counter-mode
launches are consistent; the public interface (train_test_agents, run_vary_hp mode 0, GTN_Master) runs the new launch."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

import td3d_composer as comp
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = {0: (4, 2), 1: (6, 3), 3: (2, 3)}


def small_cfg(env_id, **over):
    S, A = ENVS[env_id]
    kw = dict(env_id=env_id, state_dim=S, action_dim=A, max_steps=25, se_hidden=12, se_layers=1, se_act=2, se_prelu=0.25, hidden=16, layers=2,
              act=3, prelu=0.25, use_layer_norm=0, gumbel_hard=1, batch_size=8, rb_size=1000, train_episodes=4, test_episodes=2,
              init_episodes=1, early_out_num=2, policy_delay=2, rng_mode=1, solved_reward=1e9, gamma=0.99, lr=1e-3, tau=0.01,
              action_std=0.1, policy_std=0.2, policy_std_clip=0.5, max_action=1.0, gumbel_temp=1.5, adam_beta1=0.9, adam_beta2=0.999,
              adam_eps=1e-8, step_budget=0, se_layer_norm=0, test_mode=0, early_out_virtual_diff=0.01)
    kw.update(over)
    return orc.Td3dCfg(**kw)


def _agent_init(rng, cfg):
    P = orc.td3d_num_params(cfg)[0]
    return rng.uniform(-0.4, 0.4, P).astype(np.float32)


def _assert_same_run(got, ref, P=None):
    assert got["episodes_run"] == ref["episodes_run"]
    assert [got[k] for k in ("train_steps", "learn_steps", "test_steps")] == [ref[k] for k in ("train_steps", "learn_steps", "test_steps")]
    assert np.array_equal(np.asarray(got["episode_test_mean"]), np.asarray(ref["episode_test_mean"]), equal_nan=True)
    assert np.array_equal(np.asarray(got["episode_len"]), np.asarray(ref["episode_len"]))
    assert np.array_equal(np.asarray(got["final_test_returns"]), np.asarray(ref["final_test_returns"]))
    assert got["score"] == ref["score"]
    P = P or len(ref["final_params"])
    assert np.array_equal(np.asarray(got["final_params"])[:P], np.asarray(ref["final_params"])[:P])


# ------------------------------------------------------------------------------------------------------------------
# CPU: the composer is orc_td3d_chain
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id,over", [
    (0, dict()),
    (0, dict(use_layer_norm=1, layers=3, test_mode=1, policy_delay=1)),
    (1, dict(test_mode=1, early_out_num=1)),
    (1, dict(use_layer_norm=1, gumbel_hard=0, se_layers=2, act=2)),
])
def test_composer_equals_oracle_chain_on_the_virtual_env(env_id, over):
    rng = np.random.RandomState(10 + env_id)
    cfg = small_cfg(env_id, **over)
    tapes = comp.make_tapes(rng, cfg)
    theta = (rng.randn(sum(orc.mlp_num_params(d) for d in orc.se_descs(cfg.state_dim, cfg.action_dim, cfg.se_hidden, cfg.se_layers,
                                                                          cfg.se_act))) * 0.3).astype(np.float32)
    init = _agent_init(rng, cfg)
    ref = orc.td3d_chain(cfg, theta, init, tapes=orc.make_td3d_tapes(cfg.action_dim, **tapes))
    assert ref["rc"] == 0 and ref["learn_steps"] > 0
    got = comp.td3d_chain(cfg, comp.VirtualEnvStep(cfg, theta), init, tapes)
    _assert_same_run(got, ref)
    assert not np.array_equal(ref["final_params"], init)


def test_composer_reward_env_type_0_is_the_real_env():
    """RewardEnvStep of type 0 passes the real reward through: CartPole's +1 per step, episodes end at done or the TimeLimit."""
    rng = np.random.RandomState(3)
    cfg = small_cfg(0, test_mode=1, early_out_num=10)
    r = comp.td3d_chain(cfg, comp.RewardEnvStep(cfg, 0, np.zeros(1, np.float32), 8, 1, 3), _agent_init(rng, cfg), comp.make_tapes(rng, cfg))
    assert np.array_equal(r["episode_test_mean"], r["episode_len"].astype(np.float64))
    assert r["episode_len"].max() <= cfg.max_steps


# ------------------------------------------------------------------------------------------------------------------
# CPU: host side
# ------------------------------------------------------------------------------------------------------------------
def _cartpole_reward_env_config(**env_over):
    from learning_environments_amd.configs import cartpole_syn_env_td3_discrete
    cfg = cartpole_syn_env_td3_discrete(num_workers=2, max_iterations=1)
    cfg["agents"]["gtn"]["synthetic_env_type"] = 1
    e = cfg["envs"]["CartPole-v0"]
    e.update(reward_env_type=2, info_dim=0, hidden_size=16, hidden_layer=1, activation_fn="tanh")
    e.update(env_over)
    return cfg


class _HostEngine(object):
    name = "hip"
    device = "cpu"

    def make_inner_td3d(self, cfg, chains, **kw):
        return ("td3d", cfg, chains, kw)


def test_select_task_routes_td3_discrete_on_a_reward_env_to_the_rn_launch():
    from learning_environments_amd import _lib
    from learning_environments_amd.agents import tasks
    for vary_hp in (False, True):
        cfg = _cartpole_reward_env_config()
        cfg["agents"]["td3_discrete_vary"]["vary_hp"] = vary_hp
        t = tasks.select_task(cfg, _HostEngine(), None, test_mode=1)
        assert isinstance(t, tasks.Td3DiscreteTask) and t.name == "td3_discrete_rn" and t.vary == vary_hp
        assert isinstance(t.rn, _lib.Td3dRnCfg)
        assert (t.rn.synthetic_env_type, t.rn.reward_env_type, t.rn.rn_hidden, t.rn.rn_layers, t.rn.rn_act) == (1, 2, 16, 1, _lib.ACT["tanh"])
        assert t.cfg.test_mode == 1
        kind, _, chains, kw = t.make_inner(5)
        assert kind == "td3d" and chains == 5 and kw["rn"] is t.rn and kw["vary"] == vary_hp
    cfg = _cartpole_reward_env_config()
    cfg["agents"]["gtn"]["synthetic_env_type"] = 0
    t = tasks.select_task(cfg, _HostEngine(), None)
    assert t.rn is None and t.make_inner(2)[3]["rn"] is None        # the VirtualEnv launch as before


@pytest.mark.parametrize("rtype", [3, 4, 7, 8, 101, 102])
def test_info_vector_reward_types_raise_value_error(rtype):
    from learning_environments_amd.agents import tasks
    with pytest.raises(ValueError):
        tasks.select_task(_cartpole_reward_env_config(reward_env_type=rtype), _HostEngine(), None)


def test_same_action_num_2_is_still_refused():
    from learning_environments_amd.agents import tasks
    cfg = _cartpole_reward_env_config()
    cfg["agents"]["td3_discrete_vary"]["same_action_num"] = 2
    with pytest.raises(NotImplementedError):
        tasks.select_task(cfg, _HostEngine(), None)


def test_rn_entry_points_validate_on_the_host():
    """Parameter count and workspace of the RENV launch, and the combinations it refuses (LENV_ERR_UNSUPPORTED) -- no device needed."""
    from learning_environments_amd import _lib
    from learning_environments_amd.config import td3d_cfg_from_config, td3d_rn_cfg_from_config
    L = _lib.lib()
    cfgd = _cartpole_reward_env_config(hidden_layer=2)
    cfg, rn = td3d_cfg_from_config(cfgd), td3d_rn_cfg_from_config(cfgd)
    assert L.lenv_td3d_rn_num_params(C.byref(cfg), C.byref(rn)) == 4 * 16 + 16 + 16 * 16 + 16 + 16 + 1
    assert L.lenv_td3d_rn_workspace_bytes(C.byref(cfg), C.byref(rn), 4) > 0
    rn0 = _lib.Td3dRnCfg.from_buffer_copy(rn)
    rn0.reward_env_type = 0
    assert L.lenv_td3d_rn_num_params(C.byref(cfg), C.byref(rn0)) == 1 * 16 + 16 + 16 * 16 + 16 + 16 + 1      # the 1-input dummy
    for field, value in (("reward_env_type", 3), ("reward_env_type", 101), ("synthetic_env_type", 0), ("rn_layers", 4), ("rn_hidden", 0),
                         ("rn_layer_norm", 1)):
        bad = _lib.Td3dRnCfg.from_buffer_copy(rn)
        setattr(bad, field, value)
        assert L.lenv_td3d_rn_num_params(C.byref(cfg), C.byref(bad)) == -2, field
        assert L.lenv_td3d_rn_workspace_bytes(C.byref(cfg), C.byref(bad), 4) == 0
    assert L.lenv_td3d_rn_inner_loop(C.byref(cfg), None, None, None, None, None, None, None, None, None, 1, None, 0, None, None) == -1


def test_td3d_rn_cfg_stub_in_integration_md_has_the_library_size():
    from learning_environments_amd import _lib
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"^class Td3dRnCfg\(C\.Structure\):[^\n]*\n((?:[ \t]+[^\n]*\n)+)", text, re.M)
    assert m, "INTEGRATION.md documents no Td3dRnCfg stub"
    ns = {"C": C}
    exec("class Td3dRnCfg(C.Structure):\n" + m.group(1), ns)
    L = _lib.lib()
    assert C.sizeof(ns["Td3dRnCfg"]) == L.lenv_struct_size(13) == C.sizeof(_lib.Td3dRnCfg) == 28
    assert _lib.ABI_STRUCTS[13] is _lib.Td3dRnCfg
    assert [f[0] for f in ns["Td3dRnCfg"]._fields_] == [f[0] for f in _lib.Td3dRnCfg._fields_]


# ------------------------------------------------------------------------------------------------------------------
# GPU: the RENV launch against the composer over real physics + orc_rn_shape_rows, bit for bit
# ------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _hip(ocfg):
    from learning_environments_amd import _lib
    c = _lib.Td3dCfg()
    for f, _ in _lib.Td3dCfg._fields_:
        setattr(c, f, getattr(ocfg, f))
    return c


def _pad(rows):
    """per-chain tapes of different lengths -> one [chains, max_len, ...] array"""
    n = max(1, max(r.shape[0] for r in rows))
    out = np.zeros((len(rows), n) + rows[0].shape[1:], rows[0].dtype)
    for i, r in enumerate(rows):
        out[i, :r.shape[0]] = r
    return out


def _chain_of(il, c, E, P):
    return dict(episodes_run=int(il.stats[c, 0]), train_steps=int(il.stats[c, 1]), learn_steps=int(il.stats[c, 2]), test_steps=int(il.stats[c, 3]),
                episode_test_mean=il.episode_test_mean[c, :E].cpu().numpy(), episode_len=il.episode_len[c, :E].cpu().numpy(),
                final_test_returns=il.final_returns[c].cpu().numpy(), score=float(il.score[c]), final_params=il.final_params[c, :P].cpu().numpy())


RN_CASES = [   # env, reward type, test_mode, vary_hp, reward-net layers / activation, cfg overrides
    (0, 0, 1, False, 1, 3, dict()),
    (0, 2, 0, True, 1, 4, dict()),
    (0, 1, 1, False, 2, 2, dict(use_layer_norm=1, layers=3)),
    (0, 6, 0, False, 1, 1, dict(gumbel_hard=0)),
    (1, 5, 0, False, 1, 3, dict(max_steps=30)),
    (1, 6, 1, True, 2, 3, dict(use_layer_norm=1)),
    (1, 0, 0, False, 1, 3, dict()),
    (3, 2, 1, False, 1, 3, dict()),
    (3, 0, 0, True, 1, 2, dict()),
    (0, 0, 1, False, 1, 3, dict(train_episodes=8, solved_reward=8.0)),       # the real rule's early out fires on the training reward
]


@pytest.mark.gpu
@pytest.mark.parametrize("env_id,rtype,test_mode,vary,rn_layers,rn_act,over", RN_CASES)
def test_rn_launch_tape_mode_equals_composer(env_id, rtype, test_mode, vary, rn_layers, rn_act, over):
    import torch
    from learning_environments_amd import _lib, engine
    engine.require_device()
    rng = np.random.RandomState(100 * env_id + 10 * rtype + test_mode)
    base = small_cfg(env_id, test_mode=test_mode, **over)
    rn = _lib.Td3dRnCfg(synthetic_env_type=1, reward_env_type=rtype, rn_hidden=24, rn_layers=rn_layers, rn_act=rn_act, rn_prelu=0.25, rn_layer_norm=0)
    chains = 2
    hps = [dict(lr=2e-3, batch_size=6, hidden_size=12, hidden_layer=1), dict(lr=5e-4, batch_size=10, hidden_size=20, hidden_layer=3)]
    cfg = _hip(base)
    if vary:
        cfg.hidden, cfg.layers, cfg.batch_size = 20, 3, 10
    il = engine.Td3DiscreteInnerLoop(cfg, chains, want_final_params=True, vary=vary, rn=rn)
    Drn = 1 if rtype == 0 else base.state_dim
    assert il.p_theta == Drn * 24 + 24 + (rn_layers - 1) * (24 * 24 + 24) + 24 + 1
    theta = (rng.randn(2, il.p_theta) * 0.5).astype(np.float32)           # chain c runs theta[0] + sign[c] * eps[worker[c]]
    eps = (rng.randn(2, il.p_theta) * 0.2).astype(np.float32)
    worker, sign = np.array([0, 1], np.int32), np.array([1.0, -1.0], np.float32)
    ccfgs = []
    for c in range(chains):
        cc = orc.Td3dCfg.from_buffer_copy(base)
        if vary:
            h = hps[c]
            cc.lr, cc.batch_size, cc.hidden, cc.layers = h["lr"], h["batch_size"], h["hidden_size"], max(1, h["hidden_layer"])
        ccfgs.append(cc)
    if vary:
        il.set_hp(*[[h[k] for h in hps] for k in ("lr", "batch_size", "hidden_size", "hidden_layer")])
        init = il.draw_agent_init(_dev(np.array([7, 8], np.int64))).cpu().numpy()
    else:
        init = rng.uniform(-0.4, 0.4, (chains, il.p_agent)).astype(np.float32)
    tapes = [comp.make_tapes(rng, cc) for cc in ccfgs]
    dt = {k: _dev(_pad([t[k] for t in tapes])) for k in comp.TAPE_KEYS}
    il.run(_dev(theta[0]), _dev(eps), _dev(worker), _dev(sign), _dev(init), tapes=dt)
    torch.cuda.synchronize()
    assert il.status.cpu().tolist() == [0] * chains
    for c in range(chains):
        cc = ccfgs[c]
        w = (np.float32(sign[c]) * eps[worker[c]] + theta[0]).astype(np.float32)      # sign +-1: the kernel's fma is exact
        env = comp.RewardEnvStep(cc, rtype, w, 24, rn_layers, rn_act)
        ref = comp.td3d_chain(cc, env, init[c], tapes[c])
        assert ref["learn_steps"] > 0
        P = orc.td3d_num_params(cc)[0]
        _assert_same_run(_chain_of(il, c, cc.train_episodes, P), ref, P)
        if over.get("solved_reward"):
            assert ref["episodes_run"] < cc.train_episodes                 # the early out fired


def _counter_launch(cfg, rn, hps, keys, theta):
    import torch
    from learning_environments_amd import engine
    n = len(keys)
    il = engine.Td3DiscreteInnerLoop(cfg, n, want_final_params=True, vary=True, rn=rn)
    il.set_hp(*[[h[k] for h in hps] for k in ("lr", "batch_size", "hidden_size", "hidden_layer")])
    kt = _dev(np.asarray(keys, np.uint64).view(np.int64))
    il.draw_agent_init(kt)
    il.run(_dev(theta), None, None, None, None, rng_keys=kt)
    torch.cuda.synchronize()
    assert il.status.cpu().tolist() == [0] * n
    return il


@pytest.mark.gpu
def test_rn_counter_mode_launch_equals_one_chain_launches_and_repeats():
    """Production RNG: one launch of three heterogeneous _vary chains == three one-chain launches, and two identical launches agree."""
    from learning_environments_amd import _lib, engine
    engine.require_device()
    base = small_cfg(1, rng_mode=0, test_mode=1, hidden=24, layers=3, batch_size=12, train_episodes=5, max_steps=40)
    cfg = _hip(base)
    rn = _lib.Td3dRnCfg(synthetic_env_type=1, reward_env_type=2, rn_hidden=32, rn_layers=1, rn_act=4, rn_prelu=0.25, rn_layer_norm=0)
    hps = [dict(lr=1e-3, batch_size=12, hidden_size=24, hidden_layer=2), dict(lr=3e-3, batch_size=5, hidden_size=9, hidden_layer=1),
           dict(lr=7e-4, batch_size=8, hidden_size=17, hidden_layer=3)]
    keys = [11, 2 ** 62 + 5, 123456789]
    theta = (np.random.RandomState(4).randn(6 * 32 + 32 + 32 + 1) * 0.3).astype(np.float32)
    a = _counter_launch(cfg, rn, hps, keys, theta)
    b = _counter_launch(cfg, rn, hps, keys, theta)
    for name in ("score", "stats", "episode_test_mean", "episode_len", "final_returns", "final_params"):
        assert np.array_equal(getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy(), equal_nan=True), name
    for c in range(3):
        one = _counter_launch(cfg, rn, hps[c:c + 1], keys[c:c + 1], theta)
        for name in ("score", "stats", "episode_test_mean", "episode_len", "final_returns", "final_params"):
            assert np.array_equal(getattr(a, name)[c].cpu().numpy(), getattr(one, name)[0].cpu().numpy(), equal_nan=True), (c, name)
    assert int(a.stats[:, 2].min()) > 0 and len({tuple(r) for r in a.episode_test_mean.cpu().numpy().tolist()}) == 3     # shaped rewards differ


# ------------------------------------------------------------------------------------------------------------------
# GPU: the public interface
# ------------------------------------------------------------------------------------------------------------------
def _load_ckpt_b(tmp_path):
    import shutil
    from learning_environments_amd.experiments.syn_env_evaluate import load_envs_and_config
    shutil.copy(os.path.join(ROOT, "tests", "golden", "ckpt_cartpole_se_reference_b.pt"), tmp_path / "model.pt")
    return load_envs_and_config("model.pt", str(tmp_path), "cuda")


def _shrink(config):
    config["agents"]["td3_discrete_vary"].update(hidden_size=20, batch_size=12, hidden_layer=1, use_layer_norm=False)
    return config


@pytest.mark.gpu
def test_train_test_agents_on_the_real_env_with_td3_discrete(tmp_path):
    """Mode 0 of the TD3_discrete sibling script: agents trained on the real CartPole (a RewardEnv of type 0) -- the reference's list shapes;
    several models in one launch == model-by-model calls."""
    from learning_environments_amd.experiments.syn_env_evaluate import train_test_agents, train_test_agents_models
    _, real_env, config = _load_ckpt_b(tmp_path)
    _shrink(config)
    rewards, steps, episodes = train_test_agents(real_env, real_env, copy.deepcopy(config), agents_num=3, agent_name="td3_discrete_vary",
                                                 train_episodes=14, seed=2)
    last = train_test_agents.last
    assert last["task"].rn is not None and last["task"].rn.reward_env_type == 0 and last["inner"].rn is not None
    assert len(rewards) == len(steps) == len(episodes) == 3
    for r, s, e in zip(rewards, steps, episodes):
        assert len(r) == 10 and all(isinstance(x, float) for x in r)
        assert len(s) == 1 and len(e) == 1 and 11 <= e[0] <= 14 and s[0] >= e[0]
    assert last["reward_train"][0] == [float(x) for x in last["episode_length"][0]]      # the real CartPole's reward: +1 per step
    both = train_test_agents_models([real_env, real_env], real_env, copy.deepcopy(config), agents_num=2, agent_name="td3_discrete_vary",
                                    train_episodes=14, seed=2, model_indices=[0, 3])
    for m, mi in enumerate((0, 3)):
        one = train_test_agents(real_env, real_env, copy.deepcopy(config), agents_num=2, agent_name="td3_discrete_vary", train_episodes=14, seed=2,
                                model_index=mi)
        assert both[m] == one
    assert both[0][0] == rewards[:2]                                              # model 0's agents are the agents of the first call


@pytest.mark.gpu
def test_run_vary_hp_mode_0_with_td3_discrete_writes_the_reference_layout(tmp_path):
    import shutil
    import torch
    from learning_environments_amd.experiments import syn_env_run_vary_hp as rv
    from learning_environments_amd.experiments.syn_env_evaluate import load_envs_and_config, train_test_agents, train_test_agents_models

    def harness(train_env, test_env, config, agents_num):
        return train_test_agents(train_env, test_env, _shrink(config), agents_num, agent_name="td3_discrete_vary", train_episodes=12)
    harness.fused = lambda envs, test_env, config, agents_num, model_indices=None: train_test_agents_models(
        envs, test_env, _shrink(config), agents_num, agent_name="td3_discrete_vary", train_episodes=12, model_indices=model_indices)
    model_dir = tmp_path / "models"
    model_dir.mkdir()
    shutil.copy(os.path.join(ROOT, "tests", "golden", "ckpt_cartpole_se_reference_b.pt"), model_dir / "CartPole-v0_1_AAAAAA.pt")
    out = rv.run_vary_hp(0, "td3d", 2, 2, str(model_dir), load_envs_and_config, harness, "CartPole", out_dir=str(tmp_path))
    assert len(out[0]) == 4 and all(len(r) == 10 for r in out[0]) and len(out[1]) == 4 and len(out[2]) == 4
    saved = torch.load(str(tmp_path / "0_td3d.pt"), weights_only=False)
    ref = torch.load(os.path.join(ROOT, "tests", "golden", "g13_ref_run_vary_hp_mode2.pt"), weights_only=False)     # the reference's mode-2 file
    assert list(saved) == list(ref)                                              # same keys, same order
    assert saved["env_reward_overview"].shape == (2, 2 * 10)                     # np.hstack of each model's agents' return lists
    for k in ("reward_list", "train_steps_needed", "episode_length_needed"):
        assert type(saved[k]) is type(ref[k]) and type(saved[k][0]) is type(ref[k][0]) and type(saved[k][0][0]) is type(ref[k][0][0]), k
    assert type(saved["env_reward_overview"]) is type(ref["env_reward_overview"])
    assert saved["config"]["agents"]["td3_discrete_vary"]["train_episodes"] == 12


def _gtn_reward_env_td3d_config():
    from learning_environments_amd.configs import _td3_discrete_section, cartpole_reward_env_ddqn, fixed_work
    cfg = cartpole_reward_env_ddqn(num_workers=2, max_iterations=2)
    cfg["agents"]["gtn"]["agent_name"] = "TD3_discrete_vary"
    cfg["agents"].pop("ddqn")
    cfg["agents"]["td3_discrete_vary"] = _td3_discrete_section(hidden_size=24, batch_size=16, test_episodes=2, policy_delay=2)
    cfg = fixed_work(cfg, 3)
    cfg["envs"]["CartPole-v0"]["max_steps"] = 20
    return cfg


@pytest.mark.gpu
def test_gtn_master_trains_a_reward_env_for_td3_discrete(tmp_path, monkeypatch):
    """default_config_cartpole_reward_env.yaml with agent_name TD3_discrete_vary: two NES generations over the PReLU reward net; theta moves
    and two seeded runs are bit-identical."""
    import torch
    from learning_environments_amd.agents import tasks
    from learning_environments_amd.agents.GTN import GTN_Master
    monkeypatch.chdir(tmp_path)
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        m = GTN_Master(_gtn_reward_env_td3d_config(), bohb_id=0, seed=9)
        assert isinstance(m.task, tasks.Td3DiscreteTask) and m.task.rn is not None and m.inner.rn is not None
        assert m.p_theta == 4 * 64 + 64 + 64 + 1 and m.task.rn.rn_act == 4
        theta0 = m.theta.cpu().numpy().copy()
        mean_score, mean_list, _ = m.run()
        assert len(mean_list) == 2 and np.isfinite(mean_score)
        theta1 = m.theta.cpu().numpy().copy()
        assert not np.array_equal(theta0, theta1)
        runs.append((theta0, theta1, mean_list, m.inner.score.cpu().numpy().copy()))
    assert all(np.array_equal(x, y) for x, y in zip(runs[0][:2], runs[1][:2]))
    assert runs[0][2] == runs[1][2] and np.array_equal(runs[0][3], runs[1][3])
