"""The early-gradient instantiation of the published CartPole DDQN shape (chunk-aligned forward deal, per-wave "forward done" tags
instead of the barrier between forward and gradient) against the same shape's instantiation without it (`VARIANT_NO_EARLY_GRAD`:
pass-major deal, barrier) and the generic instantiation (`VARIANT_GENERIC`): every output of every chain bit for bit, the trained
online parameters included, and one whole chain against the oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POP, CHAINS = 2, 6                      # 2 workers x (theta, theta + eps, theta - eps)
# theta / eps seed of the production-form cases, chosen with oracle.ddqn_se_chain on the CPU (theta ~ 0.15 N, eps ~ 0.08 N): the SE's
# done-net ends all learning episodes of chain 4 after 1 - 4 steps and two of chain 2's after one step, chain 2's other three and all
# of chains 0, 1, 3, 5 run the full 200 steps
SEED_EARLY_ENDING = 7


@pytest.fixture(scope="module")
def eng():
    from learning_environments_amd import engine
    engine.require_device()
    return engine


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _case(which):
    from learning_environments_amd import configs
    if which in ("fixed_work", "ring_wrap"):
        cfgd = configs.fixed_work(configs.cartpole_syn_env_ddqn(POP), 3)      # 1 init + 2 learning episodes = 400 learn steps per chain
        if which == "ring_wrap":
            cfgd["agents"]["ddqn"]["rb_size"] = 300                            # wraps inside the learning episodes: ~half the steps draw their own row
        return cfgd, 17, 0.02, 4
    cfgd = configs.cartpole_syn_env_ddqn(POP)                                   # production form: early-out on
    cfgd["agents"]["ddqn"].update(train_episodes=6)
    if which == "time_out":
        cfgd["agents"]["ddqn"]["step_budget"] = 700
    # oracle chain: 2 (short and full learning episodes); under the budget chain 0, which is timed out after two full learning episodes
    return cfgd, SEED_EARLY_ENDING, 0.08, 0 if which == "time_out" else 2


@pytest.mark.parametrize("which", ["fixed_work", "ring_wrap", "early_ending", "time_out"])
def test_early_gradient_vs_barrier_vs_generic_instantiation(eng, orc, which):
    from learning_environments_amd import _lib
    from learning_environments_amd.config import ddqn_cfg_from_config
    cfgd, seed, eps_scale, oracle_chain = _case(which)
    cfg = ddqn_cfg_from_config(cfgd)
    ocfg = orc.ddqn_cfg_from_config(cfgd, grad_chunk=cfg.grad_chunk, rng_mode=0)
    assert (cfg.q_hidden, cfg.se_hidden, cfg.batch_size, cfg.test_episodes, cfg.max_steps, cfg.grad_chunk) == (57, 83, 199, 10, 200, 17)
    S, A = cfg.state_dim, cfg.num_actions
    rng = np.random.RandomState(seed)
    P_se = sum(orc.mlp_num_params(d) for d in orc.se_descs(S, A, cfg.se_hidden, 1, "leakyrelu"))
    P_q = orc.mlp_num_params(orc.mlp_desc(S, cfg.q_hidden, 1, A, "tanh"))
    theta = (rng.randn(P_se) * 0.15).astype(np.float32)
    eps = (rng.randn(POP, P_se) * eps_scale).astype(np.float32)
    agent_init = rng.uniform(-0.4, 0.4, (CHAINS, P_q)).astype(np.float32)
    worker = np.repeat(np.arange(POP), 3).astype(np.int32)
    sign = np.tile(np.array([0.0, 1.0, -1.0], np.float32), POP)
    keys = np.array([orc.chain_key(77, 3, int(worker[c]), c % 3) for c in range(CHAINS)], np.uint64)
    item, mask = (C.c_int32 * 768)(), (C.c_int32 * 16)()
    outs = {}
    for variant in (0, _lib.VARIANT_NO_EARLY_GRAD, _lib.VARIANT_GENERIC):
        c = _lib.DdqnCfg.from_buffer_copy(cfg)
        c.kernel_variant = variant
        # the default launch is the one on the early-gradient instantiation
        assert _lib.lib().lenv_ddqn_se_forward_deal(C.byref(c), item, mask) == (12 if variant == 0 else 0)
        il = eng.InnerLoop(c, CHAINS, want_final_online=True)
        il.run(dev(theta), dev(eps), dev(worker), dev(sign), dev(agent_init), rng_keys=dev(keys.view(np.int64)))
        torch.cuda.synchronize()
        assert il.status.cpu().tolist() == [0] * CHAINS, (variant, il.status.cpu().tolist())
        outs[variant] = [t.cpu().numpy().copy() for t in (il.score, il.stats, il.episode_test_mean, il.episode_len, il.final_returns, il.final_online)]
    for variant in (_lib.VARIANT_NO_EARLY_GRAD, _lib.VARIANT_GENERIC):
        for a, b in zip(outs[0], outs[variant]):
            assert np.array_equal(a, b, equal_nan=True), variant
    score, stats, ep_mean, ep_len, final_returns, final_online = outs[0]
    if which in ("fixed_work", "ring_wrap"):
        assert (stats[:, 1] == 600).all() and (stats[:, 2] == 400).all()
    if which == "early_ending":
        learn_len = np.concatenate([ep_len[c, 1:int(stats[c, 0])] for c in range(CHAINS)])
        assert (learn_len < 200).any() and (learn_len == 200).any(), ep_len.tolist()
    if which == "time_out":
        assert (stats[:, 0] < 6).any(), stats.tolist()                     # the budget ended some chain's training early
    c = oracle_chain
    w = (np.float32(sign[c]) * eps[worker[c]] + theta).astype(np.float32)
    o = orc.ddqn_se_chain(ocfg, w, agent_init[c], rng_key=int(keys[c]), want_final_online=True)
    assert o["learn_steps"] > 0
    assert float(score[c]) == o["score"] and stats[c].tolist() == [o["episodes_run"], o["train_steps"], o["learn_steps"], o["test_steps"]]
    assert np.array_equal(ep_mean[c], o["episode_test_mean"], equal_nan=True) and np.array_equal(final_returns[c], o["final_test_returns"])
    assert np.array_equal(final_online[c], o["final_online"])
