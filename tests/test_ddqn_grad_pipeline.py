"""The pipelined gradient chunk of the published CartPole DDQN shape (`LENV_DDQN_GRAD_PIPE`: a chunk's samples in groups, the LDS reads of
group g + 1 requested before the arithmetic of group g, the first group's reads in the TD error's round trip).  The path exists only in
the two one-workgroup instantiations of that shape -- the default launch and `VARIANT_NO_EARLY_GRAD` -- so the shape is fixed and the
cases are short runs at it; `VARIANT_GENERIC` keeps the loop every other instantiation runs and is the independent reference.  Every
output of every chain bit for bit across the three (scores, counters, per-episode means and lengths, final test returns, the trained
online parameters -- the entry has no output for the target net, whose every Polyak step the online parameters of the following steps
depend on), and chain 0 against the oracle.

Every learn step of either case runs eleven full chunks (17 samples: all the groups, the short one at the end included), the
12-sample last chunk (which requests one group more than it uses), the bias lane 57 and the idle lanes 58-63."""
import ctypes as C

import numpy as np
import pytest

from test_ddqn_early_gradient import CHAINS, POP, dev, eng, orc  # noqa: F401  (fixtures and helpers)

pytestmark = pytest.mark.gpu

# replay capacity: (a) fewer rows than one chunk has samples -- rows repeat inside every chunk, and from the twelfth step on the ring
# wraps every twelve steps; (b) forty rows: the ring wraps, and a minibatch of 199 draws from forty rows misses the row appended in the
# same step (the LDS copy the forward patches in) with probability (39 / 40) ** 199 < 1 % per step
CASES = {"short_ring": 12, "wrapping_ring": 40}


@pytest.mark.parametrize("which", sorted(CASES))
def test_pipelined_chunk_vs_barrier_vs_generic_instantiation(eng, orc, which):
    import torch
    from learning_environments_amd import _lib, configs
    from learning_environments_amd.config import ddqn_cfg_from_config
    cfgd = configs.fixed_work(configs.cartpole_syn_env_ddqn(POP), 3)          # one init episode and two learning episodes
    cfgd["agents"]["ddqn"]["rb_size"] = CASES[which]
    cfg = ddqn_cfg_from_config(cfgd)
    ocfg = orc.ddqn_cfg_from_config(cfgd, grad_chunk=cfg.grad_chunk, rng_mode=0)
    assert (cfg.q_hidden, cfg.se_hidden, cfg.batch_size, cfg.test_episodes, cfg.max_steps, cfg.grad_chunk) == (57, 83, 199, 10, 200, 17)
    S, A = cfg.state_dim, cfg.num_actions
    rng = np.random.RandomState(17)
    P_se = sum(orc.mlp_num_params(d) for d in orc.se_descs(S, A, cfg.se_hidden, 1, "leakyrelu"))
    P_q = orc.mlp_num_params(orc.mlp_desc(S, cfg.q_hidden, 1, A, "tanh"))
    theta = (rng.randn(P_se) * 0.15).astype(np.float32)
    eps = (rng.randn(POP, P_se) * 0.02).astype(np.float32)
    agent_init = rng.uniform(-0.4, 0.4, (CHAINS, P_q)).astype(np.float32)
    worker = np.repeat(np.arange(POP), 3).astype(np.int32)
    sign = np.tile(np.array([0.0, 1.0, -1.0], np.float32), POP)
    keys = np.array([orc.chain_key(78, 5, int(worker[c]), c % 3) for c in range(CHAINS)], np.uint64)
    item, mask = (C.c_int32 * 768)(), (C.c_int32 * 16)()
    outs = {}
    for variant in (0, _lib.VARIANT_NO_EARLY_GRAD, _lib.VARIANT_GENERIC):
        c = _lib.DdqnCfg.from_buffer_copy(cfg)
        c.kernel_variant = variant
        # the default launch is the one on the early-gradient instantiation; the other two do not report a deal
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
    assert (stats[:, 2] > 0).all(), stats.tolist()                              # every chain learned
    assert (stats[:, 1] > 2 * CASES[which]).all(), stats.tolist()               # ... and its ring wrapped
    assert np.isfinite(final_online).all() and (final_online != agent_init).any(axis=1).all()
    w = (np.float32(sign[0]) * eps[worker[0]] + theta).astype(np.float32)
    o = orc.ddqn_se_chain(ocfg, w, agent_init[0], rng_key=int(keys[0]), want_final_online=True)
    assert o["learn_steps"] > 0
    assert float(score[0]) == o["score"] and stats[0].tolist() == [o["episodes_run"], o["train_steps"], o["learn_steps"], o["test_steps"]]
    assert np.array_equal(ep_mean[0], o["episode_test_mean"], equal_nan=True) and np.array_equal(final_returns[0], o["final_test_returns"])
    assert np.array_equal(final_online[0], o["final_online"])
