#!/usr/bin/env python3
"""Throughput of the fused kernels at the FULL shapes of BASELINE configs 2-5 on a reduced episode budget (extra
information for DESIGN.md; bench.py's contract line is config 2 only).  Prints one JSON object per config."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.makedirs("/tmp/lenv_bench", exist_ok=True)
os.chdir("/tmp/lenv_bench")

from learning_environments_amd.agents.GTN import GTN_Master  # noqa: E402
from learning_environments_amd import configs  # noqa: E402


def run(name, cfg, gens=2, extra=None, force_gemm=False, median=False, theta=None):
    torch.manual_seed(0)
    m = GTN_Master(cfg, bohb_id=0, seed=7, graph=False if theta is not None else None)
    if theta is not None:    # a given synthetic env, put back before every generation: each one is the same work up to its noise draw
        theta = torch.from_numpy(theta).to(m.theta.device)
        m.theta.copy_(theta)
    if force_gemm:       # A/B aid: one sequential batch gradient (grad_chunk 0) = the GEMM-queue kernel instead of the register-resident one
        m.cfg.grad_chunk = 0
        m.inner = m.task.make_inner(m.cpw * m.n_local)
        assert m.inner.dueling
    m.step(0)
    torch.cuda.synchronize()
    if median:           # every generation timed on its own (a synchronise behind each), the median reported
        times = []
        for it in range(1, 1 + gens):
            if theta is not None:
                m.theta.copy_(theta)
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.step(it)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        dt = sorted(times)[len(times) // 2]
    else:
        t0 = time.perf_counter()
        for it in range(1, 1 + gens):
            m.step(it)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / gens
    st = m.inner.stats.cpu().numpy()
    out = dict(config=name, pop=cfg["agents"]["gtn"]["num_workers"], chains=int(st.shape[0]), s_per_generation=dt,
               evals_per_s=cfg["agents"]["gtn"]["num_workers"] / dt, train_steps=int(st[:, 1].sum()), learn_steps=int(st[:, 2].sum()),
               test_steps=int(st[:, 3].sum()), us_per_learn_step_per_chain=1e6 * dt / max(1.0, st[:, 2].mean()))
    out.update(extra(cfg, st, dt) if extra else {})
    print(json.dumps(out))
    return out


def run_test_mode1_ab(name, cfg, gens=7):
    """One `test_mode` 1 launch (BaseAgent.train without a test env, the evaluation harness's training call) per generation, on the wave-chain
    kernel and -- the same launch, gtn.kernel_variant = NO_WAVECHAIN -- on the GEMM-queue kernel: two masters with the same seed in one
    process, a warm-up generation each, then `gens` generations each in alternation, every one timed on its own.  Reports the medians, the
    spread (max - min) of the samples and whether the wave-chain median lies below the other by more than the larger spread; the two
    masters' scores, counters and updated theta must agree bit for bit after every generation."""
    import copy
    import ctypes as C
    from learning_environments_amd import _lib
    masters = {}
    for label, variant in (("wavechain", 0), ("no_wavechain", _lib.VARIANT_NO_WAVECHAIN)):
        c = copy.deepcopy(cfg)
        c["agents"]["gtn"]["kernel_variant"] = variant
        torch.manual_seed(0)
        m = GTN_Master(c, bohb_id=0, seed=7, graph=False)
        m.cfg.test_mode = 1
        m.inner = m.task.make_inner(m.cpw * m.n_local)
        m.step(0)
        torch.cuda.synchronize()
        masters[label] = m
    chains = masters["wavechain"].cpw * masters["wavechain"].n_local
    query = _lib.lib().lenv_td3_rn_team_size if isinstance(masters["wavechain"].cfg, _lib.Td3Cfg) else _lib.lib().lenv_dueling_team_size
    teams = {label: int(query(C.byref(m.cfg), chains)) for label, m in masters.items()}
    times = {label: [] for label in masters}
    same = True
    for it in range(1, 1 + gens):
        for label, m in masters.items():
            t0 = time.perf_counter()
            m.step(it)
            torch.cuda.synchronize()
            times[label].append(time.perf_counter() - t0)
        a, b = masters["wavechain"], masters["no_wavechain"]
        same = same and torch.equal(a.inner.score, b.inner.score) and torch.equal(a.inner.stats, b.inner.stats) and torch.equal(a.theta, b.theta)
    med = {label: sorted(t)[len(t) // 2] for label, t in times.items()}
    spread = {label: max(t) - min(t) for label, t in times.items()}
    st = masters["wavechain"].inner.stats.cpu().numpy()
    out = dict(config=name, test_mode=1, chains=int(chains), team_size=teams, generations_each=gens,
               ms_median={k: 1e3 * v for k, v in med.items()}, ms_spread={k: 1e3 * v for k, v in spread.items()},
               ms_samples={k: [round(1e3 * x, 3) for x in v] for k, v in times.items()}, ratio=med["no_wavechain"] / med["wavechain"],
               wavechain_faster_by_more_than_the_spread=bool(med["no_wavechain"] - med["wavechain"] > max(spread.values())),
               bit_identical=bool(same), train_steps=int(st[:, 1].sum()), learn_steps=int(st[:, 2].sum()), test_steps=int(st[:, 3].sum()))
    print(json.dumps(out))
    return out


def _td3_loop(cfgd, chains, seed=0, **over):
    """A Td3InnerLoop at cfgd's TD3 shape on the generic GEMM-queue kernel with seeded inputs: (inner loop, run arguments, keyword arguments)."""
    import numpy as np
    from learning_environments_amd import _lib, engine
    from learning_environments_amd.agents.nes_common import linear_init_bounds
    from learning_environments_amd.config import td3_cfg_from_config, td3_layer_dims
    cfg = td3_cfg_from_config(cfgd, kernel_variant=_lib.VARIANT_GENERIC, **over)
    il = engine.Td3InnerLoop(cfg, chains, want_episode_stats=True, want_final_params=True)
    rng = np.random.RandomState(seed)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    S, Hrn, Lrn = cfg.state_dim, cfg.rn_hidden, cfg.rn_layers
    if cfg.virtual_env:
        SA = S + cfg.action_dim
        p_theta = sum(SA * Hrn + Hrn + (Lrn - 1) * (Hrn * Hrn + Hrn) + o * Hrn + o for o in (S, 1, 1))
    else:
        p_theta = max(1, engine.rn_num_params(cfg.reward_env_type, S, cfg.info_dim, Hrn, Lrn))
    theta = dev((rng.randn(p_theta) * 0.1).astype(np.float32))
    bounds = linear_init_bounds(td3_layer_dims(cfg))
    init = dev((rng.uniform(-1.0, 1.0, (chains, il.p_agent)) * bounds[None]).astype(np.float32))
    keys = dev(np.array([engine.chain_key(11, 0, c, 0) for c in range(chains)], np.uint64).view(np.int64))
    return il, (theta, None, None, None, init), dict(rng_keys=keys)


def _timed_segments(il, pos, kw, episodes, after=None):
    """Segment launches of ONE episode each, every one timed on its own: the seconds per launch.  after(): called behind each, outside its time."""
    times = []
    for e in range(episodes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        il.run_segment(*pos, e, e + 1, **kw)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        if after is not None:
            after()
    return times


def run_segments(name, loop, final, episodes, splits, runs=7, boundary_wait=False):
    """The cost of splitting: the workload of `loop` = (inner loop, run arguments, keyword arguments) as one launch of the family's old entry,
    as ONE segment launch and as `splits` segment launches (with the host's read of the finished words behind each), `runs` timed runs each in
    alternation after a warm-up of each; medians, the runs' ranges and spreads (max - min) and ratios to the old entry; the three must agree
    bit for bit in every output and in `final`, the final-parameter buffer.  boundary_wait: also where a split series can lose time."""
    il, pos, kw = loop
    per = -(-episodes // splits)
    last = "%d_segments" % splits
    forms = (("old_entry", None), ("one_segment", episodes), (last, per))
    times, snaps = {k: [] for k, _ in forms}, {}
    for it in range(runs + 1):
        for label, epl in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            il.run(*pos, episodes_per_launch=epl, **kw)
            torch.cuda.synchronize()
            if it:
                times[label].append(time.perf_counter() - t0)
            snaps[label] = [t.clone() for t in (il.score, il.stats, il.status, il.episode_test_mean, il.episode_len, il.final_returns, getattr(il, final))]
    same = all(all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(snaps["old_entry"], snaps[k])) for k in snaps)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    lo, hi = min(times["old_entry"]), max(times["old_entry"])
    st = il.stats.cpu().numpy()
    learn = float(st[:, 2].mean())
    out = dict(config=name, chains=il.chains, episodes=episodes, runs_each=runs, s_median=med, s_min={k: min(v) for k, v in times.items()},
               s_max={k: max(v) for k, v in times.items()}, s_spread={k: max(v) - min(v) for k, v in times.items()},
               s_samples={k: [round(x, 5) for x in v] for k, v in times.items()}, ratio_to_old_entry={k: med[k] / med["old_entry"] for k in med},
               ms_per_boundary=1e3 * (med[last] - med["old_entry"]) / max(1, splits - 1), split_median_inside_old_entry_range=bool(lo <= med[last] <= hi),
               bit_identical=bool(same), status_ok=bool(int(il.status.min()) == 0), train_steps_per_chain=float(st[:, 1].mean()),
               train_steps_max=int(st[:, 1].max()), learn_steps_per_chain=learn, learn_calls_per_chain=learn,
               test_steps_per_chain=float(st[:, 3].mean()), workspace_MiB=il.ws_bytes / 2.0 ** 20)
    if boundary_wait:
        assert same, "the three forms of the launch differ"
        # where a split series can lose time: a workgroup per chain and every chain resident, so a launch lasts as long as its slowest chain -- one launch
        # max_c sum_e steps(c, e), a series sum_seg max_c sum_(e in seg) steps(c, e): the chains wait for each other at every boundary.  steps = the
        # episode's agent steps plus `w` times its test steps (CartPole with one test episode: the test return IS its length), for w = 0 and 0.2
        ln = il.episode_len.cpu().numpy().astype(float)
        tl = il.episode_test_mean.cpu().numpy() if il.cfg.test_episodes == 1 and il.cfg.env_id == 0 else 0.0 * ln
        model = {}
        for w in (0.0, 0.2):
            S = ln + w * tl
            model["test_step_weight_%.1f" % w] = sum(S[:, b:b + per].sum(1).max() for b in range(0, episodes, per)) / S.sum(1).max()
        out["boundary_wait_model_ratio"] = model
        out["slowest_chain_per_segment"] = [int(ln[:, b:b + per].sum(1).argmax()) for b in range(0, episodes, per)]
    print(json.dumps(out))
    return out


def run_td3_episode_time(name, cfgd, shape, chains=8, timed=2):
    """Seconds per learning episode of a chain at `shape` = (hidden, layers, batch): segment launches of one episode each, one init episode and
    one learning episode as warm-up, then `timed` learning episodes timed one by one (the median).  A chain has its workgroup to itself, so the
    time does not depend on the number of chains while they fit the CUs."""
    H, L, B = shape
    il, pos, kw = _td3_loop(cfgd, chains, train_episodes=2 + timed, init_episodes=1, hidden=H, layers=L, batch_size=B)
    times = _timed_segments(il, pos, kw, 2 + timed)
    st = il.stats.cpu().numpy()
    fin, status = il.segment_state()
    out = dict(config=name, hidden=H, layers=L, batch=B, chains=chains, s_per_learning_episode=sorted(times[2:])[len(times[2:]) // 2],
               s_samples=[round(t, 4) for t in times], status_ok=bool(int(status.min()) == 0), train_steps_per_chain=float(st[:, 1].mean()),
               learn_steps_per_chain=float(st[:, 2].mean()), test_steps_per_chain=float(st[:, 3].mean()))
    print(json.dumps(out))
    return out


def _td3d_loop(chains, episodes, real_env=False, init_episodes=6, max_steps=None, seed=0):
    """A Td3DiscreteInnerLoop at the histogram scripts' shape (`td3_discrete_vary_layer_norm_2`: 4-128-128-2 tanh with LayerNorm, the agent section
    of fixture g12t) as the evaluation harness launches it -- test_mode 1, every chain its own key and freshly drawn agent -- on the reference-written
    CartPole SE checkpoint of the test suite (its config: episodes of 40 steps; max_steps: another length, CartPole-v0's own is 200), or on the
    real CartPole (a RewardEnv of type 0); no early out.  (inner loop, run arguments, keywords)"""
    import numpy as np
    from learning_environments_amd import engine
    from learning_environments_amd.config import td3d_cfg_from_config, td3d_rn_cfg_from_config
    golden = os.path.join(ROOT, "tests", "golden")
    save = torch.load(os.path.join(golden, "ckpt_cartpole_se_reference_b.pt"), map_location="cpu", weights_only=False)
    cfgd = save["config"]
    g = np.load(os.path.join(golden, "g12t_train_test_agents_cartpole_mode2_td3_discrete_vary.npz"), allow_pickle=True)
    cfgd["agents"]["td3_discrete_vary"] = dict(json.loads(str(g["config_json"]))["agents"]["td3_discrete_vary"], train_episodes=episodes,
                                               init_episodes=init_episodes, early_out_num=10, early_out_virtual_diff=0.0, vary_hp=False)
    cfgd["agents"]["gtn"] = dict(cfgd["agents"].get("gtn", {}), agent_name="td3_discrete_vary", synthetic_env_type=1 if real_env else 0)
    e = cfgd["envs"][cfgd["env_name"]]
    e["solved_reward"] = 1e9
    if max_steps is not None:
        e["max_steps"] = max_steps
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rn = None
    if real_env:
        e["reward_env_type"] = 0
        rn = td3d_rn_cfg_from_config(cfgd)
    cfg = td3d_cfg_from_config(cfgd, test_mode=1)
    il = engine.Td3DiscreteInnerLoop(cfg, chains, want_episode_stats=True, want_final_params=True, rn=rn)
    theta = torch.zeros(il.p_theta, dtype=torch.float32, device="cuda") if real_env else dev(g["theta"])
    keys = dev(np.array([engine.chain_key(17 + seed, 0, c, 0) for c in range(chains)], np.uint64).view(np.int64))
    il.draw_agent_init(keys)
    return il, (theta, None, None, None, None), dict(rng_keys=keys)


def run_td3d_entry_builds(name, loop, other_lib, runs=7):
    """The single-launch entry of `loop` on this build against the same entry of another build of the library (the parent commit's: its path is
    the caller's), a warm-up of each, then `runs` alternating launches; medians, the runs' ranges and whether the outputs agree bit for bit."""
    import ctypes as C
    from learning_environments_amd import _lib
    il, pos, kw = loop
    args = il._launch_args(*pos, kw["rng_keys"], None)
    fn_name = il.entry[0]
    other = C.CDLL(os.path.abspath(other_lib))
    fns = {"this_build": getattr(_lib.lib(), fn_name), "other_build": getattr(other, fn_name)}
    fns["other_build"].restype, fns["other_build"].argtypes = _lib.SIGNATURES[fn_name]
    times, snaps = {k: [] for k in fns}, {}
    for r in range(runs + 1):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _lib.check(fn(C.byref(il.cfg), *il._prefix_args(), *args), k)
            torch.cuda.synchronize()
            if r:
                times[k].append(time.perf_counter() - t0)
            snaps[k] = [getattr(il, n).cpu().numpy().tobytes() for n in ("score", "stats", "status", "episode_test_mean", "episode_len", "final_params")]
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    out = dict(config=name, entry=fn_name, runs_each=runs, s_median=med, s_min={k: min(v) for k, v in times.items()},
               s_max={k: max(v) for k, v in times.items()}, s_spread={k: max(v) - min(v) for k, v in times.items()},
               s_samples={k: [round(t, 5) for t in v] for k, v in times.items()}, ratio_this_to_other=med["this_build"] / med["other_build"],
               difference_inside_the_runs_spread=bool(abs(med["this_build"] - med["other_build"]) <= max(max(v) - min(v) for v in times.values())),
               bit_identical=snaps["this_build"] == snaps["other_build"], status_ok=bool(int(il.status.min()) == 0))
    print(json.dumps(out))
    return out


def run_td3d_episode_time(name, loop):
    """Seconds per FULL-LENGTH learning episode (max_steps agent steps, each with a learn step) of the harness's TD3_discrete chains: segment
    launches of one episode each, every one timed.  A workgroup per chain, so a segment takes what its longest chain takes; the figure is the
    median over the learning segments in which some chain ran max_steps steps, beside every learning segment's time scaled to max_steps by its
    longest chain's length."""
    il, pos, kw = loop
    E, full_len, init = il.cfg.train_episodes, il.cfg.max_steps, il.cfg.init_episodes
    times = _timed_segments(il, pos, kw, E)
    fin, status = il.segment_state()
    longest = il.episode_len.cpu().numpy().max(axis=0)
    full = sorted(t for t, n in zip(times[init:], longest[init:]) if n == full_len)
    scaled = sorted(t * full_len / n for t, n in zip(times[init:], longest[init:]))
    st = il.stats.cpu().numpy()
    out = dict(config=name, chains=il.chains, episodes=E, init_episodes=init, max_steps=full_len, full_length_segments=len(full),
               s_per_full_length_episode=full[len(full) // 2] if full else None, s_full_min=full[0] if full else None, s_full_max=full[-1] if full else None,
               s_scaled_to_full_length_median=scaled[len(scaled) // 2], s_scaled_to_full_length_min=scaled[0], s_scaled_to_full_length_max=scaled[-1],
               s_init_episode_median=sorted(times[1:init])[len(times[1:init]) // 2] if init > 1 else None,
               longest_chain_steps_per_learning_segment=[int(n) for n in longest[init:]], status_ok=bool(int(status.min()) == 0),
               finished=int(fin.sum()), train_steps_per_chain=float(st[:, 1].mean()), learn_steps_per_chain=float(st[:, 2].mean()))
    print(json.dumps(out))
    return out


def _dueling_loop(cfgd, chains, shape, seed=0, lr=None):
    """An InnerLoop built for segments (the generic GEMM-tiled kernel, per-chain hyper-parameter arrays with `shape` = (hidden, layers, batch) for
    every chain, as experiments/transfer_cartpole.py launches its agents) with seeded inputs: (inner loop, run arguments, keyword arguments)."""
    import numpy as np
    from learning_environments_amd import engine
    from learning_environments_amd.config import ddqn_cfg_from_config
    H, L, B = shape
    family = "duelingddqn" if "duelingddqn" in cfgd["agents"] else "ddqn"
    cfgd["agents"][family].update(hidden_size=H, hidden_layer=L, batch_size=B)
    cfgd["agents"]["gtn"]["agent_name"] = family + "_vary"
    cfg = ddqn_cfg_from_config(cfgd)
    cfg.grad_chunk = 0
    il = engine.InnerLoop(cfg, chains, want_episode_stats=True, want_final_online=True, vary=True, segments=True)
    a = cfgd["agents"][family]
    il.set_hp([a["lr"] if lr is None else lr] * chains, [B] * chains, [H] * chains, [L] * chains)
    rng = np.random.RandomState(seed)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    p_theta = engine.mlp_num_params(engine.mlp_desc(1 if cfg.reward_env_type == 0 else cfg.state_dim, cfg.se_hidden, cfg.se_layers, 1, cfg.se_act))
    theta = dev((rng.randn(p_theta) * 0.1).astype(np.float32))
    keys = dev(np.array([engine.chain_key(13, 0, c, 0) for c in range(chains)], np.uint64).view(np.int64))
    il.draw_agent_init(keys)
    return il, (theta, None, None, None, None), dict(rng_keys=keys)


def _cartpole_transfer_config(script, episodes):
    """The CartPole RewardEnv (published values: type 2, PReLU reward net 4-64-1, 200 steps) with the transfer script's settings block."""
    from learning_environments_amd.experiments import transfer_cartpole as tc
    c = tc.apply_settings(tc.base_config(), script, dict(train_episodes=episodes))
    c["envs"]["CartPole-v0"]["solved_reward"] = tc.SOLVED_REWARD
    if script == "algo":
        c["agents"].pop("ddqn")
    return c


def run_dueling_episode_time(name, cfgd, shape, chains=8, episodes=300, lr=1e-3):
    """Seconds per FULL-LENGTH learning episode (max_steps agent steps, each with a learn step) of a chain at `shape` = (hidden, layers, batch):
    segment launches of one episode each, every one timed.  CartPole episodes end when the pole falls, so a launch is full-length only once an
    agent balances: the chains train (lr 1e-3 instead of the block's: the time of a step does not depend on it) and the figure is the median
    over the segments in which some chain ran max_steps steps -- a workgroup per chain, so such a segment takes what its longest chain takes,
    including that chain's test episode.  Beside it: every learning segment's time scaled to max_steps by its longest chain's length."""
    il, pos, kw = _dueling_loop(cfgd, chains, shape, lr=lr)
    E, full_len = il.cfg.train_episodes, il.cfg.max_steps
    assert E == episodes
    times = _timed_segments(il, pos, kw, E)
    fin, status = il.segment_state()
    longest = il.episode_len.cpu().numpy().max(axis=0)
    full = sorted(t for t, n in zip(times[2:], longest[2:]) if n == full_len)
    scaled = sorted(t * full_len / n for t, n in zip(times[2:], longest[2:]))
    st = il.stats.cpu().numpy()
    out = dict(config=name, hidden=shape[0], layers=shape[1], batch=shape[2], chains=chains, episodes=E, full_length_segments=len(full),
               s_per_full_length_episode=full[len(full) // 2] if full else None, s_full_min=full[0] if full else None, s_full_max=full[-1] if full else None,
               s_scaled_to_full_length_median=scaled[len(scaled) // 2], s_scaled_to_full_length_max=scaled[-1],
               us_per_agent_step_of_full_segments=1e6 * full[len(full) // 2] / full_len if full else None, status_ok=bool(int(status.min()) == 0),
               finished=int(fin.sum()), train_steps_per_chain=float(st[:, 1].mean()), learn_steps_per_chain=float(st[:, 2].mean()),
               test_steps_per_chain=float(st[:, 3].mean()))
    print(json.dumps(out))
    return out


def _ppo_loop(cfgd, chains, models=1, seed=0, icm=None, **over):
    """A PpoInnerLoop at cfgd's PPO shape with seeded inputs: (inner loop, run arguments, keyword arguments).  models > 1: chain c reads reward net
    c // (chains / models) through its eps row (theta 0, sign 1), as experiments/transfer_algo.py launches the models of a mode.  icm (a dict of
    the config's `icm` section): a PpoIcmInnerLoop with seeded fresh modules instead."""
    import numpy as np
    from learning_environments_amd import engine
    from learning_environments_amd.agents.nes_common import linear_init_bounds
    from learning_environments_amd.config import icm_layer_dims, ppo_cfg_from_config, ppo_layer_dims
    cfg = ppo_cfg_from_config(cfgd, **over)
    rng = np.random.RandomState(seed)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if icm is None:
        il = engine.PpoInnerLoop(cfg, chains, want_episode_stats=True, want_final_params=True)
    else:
        il = engine.PpoIcmInnerLoop(cfg, chains, icm, want_episode_stats=True, want_final_params=True)
        ib = linear_init_bounds(icm_layer_dims(cfg, icm["feature_dim"], icm["hidden_size"]))
        il.icm_init.copy_(dev((np.random.RandomState(seed + 1).uniform(-1.0, 1.0, (chains, il.p_icm)) * ib[None]).astype(np.float32)))
    p_theta = max(1, il.p_theta)
    nets = (rng.randn(models, p_theta) * 0.1).astype(np.float32)
    bounds = np.concatenate([np.zeros(cfg.action_dim, np.float32), linear_init_bounds(ppo_layer_dims(cfg))])
    init = (rng.uniform(-1.0, 1.0, (chains, il.p_agent)) * bounds[None]).astype(np.float32)
    init[:, :cfg.action_dim] = np.float32(cfg.action_std)
    keys = dev(np.array([engine.chain_key(11, 0, c, 0) for c in range(chains)], np.uint64).view(np.int64))
    if models == 1:
        pos = (dev(nets[0]), None, None, None, dev(init))
    else:
        pos = (dev(np.zeros(p_theta, np.float32)), dev(nets), dev((np.arange(chains) // (chains // models)).astype(np.int32)),
               dev(np.ones(chains, np.float32)), dev(init))
    return il, pos, dict(rng_keys=keys)


def run_ppo_icm_cost(name, cfgd, chains, icm, runs=7):
    """The ICM's cost on one shape: the same seeded launch through lenv_ppo_rn_inner_loop and through lenv_ppo_icm_inner_loop, a warm-up of each, then
    `runs` alternating launches of each timed with the host clock around a synchronise; medians, and the difference per learn call of a chain."""
    loops = {"without_icm": _ppo_loop(cfgd, chains), "with_icm": _ppo_loop(cfgd, chains, icm=icm)}
    times = {k: [] for k in loops}
    for r in range(runs + 1):
        for k, (il, pos, kw) in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            il.run(*pos, **kw)
            torch.cuda.synchronize()
            if r:
                times[k].append(time.perf_counter() - t0)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    calls = {k: float(l[0].stats[:, 2].cpu().numpy().mean()) for k, l in loops.items()}
    il = loops["with_icm"][0]
    out = dict(config=name, chains=chains, runs_each=runs, rows_per_learn=il.rows, ppo_epochs=il.cfg.ppo_epochs, icm=icm, s_median=med,
               s_spread={k: max(v) - min(v) for k, v in times.items()}, s_samples={k: [round(t, 5) for t in v] for k, v in times.items()},
               learn_calls_per_chain=calls, ms_icm_per_learn_call=1e3 * (med["with_icm"] - med["without_icm"]) / max(1.0, calls["with_icm"]),
               ratio_with_to_without=med["with_icm"] / med["without_icm"], workspace_MiB={k: l[0].ws_bytes / 2.0 ** 20 for k, l in loops.items()},
               status_ok=all(int(l[0].status.min()) == 0 for l in loops.values()))
    print(json.dumps(out))
    return out


def run_ppo_entry_builds(name, cfgd, chains, other_lib, runs=7):
    """lenv_ppo_rn_inner_loop of this build against the same entry of another build of the library (the parent commit's: its path is the
    caller's), one seeded launch, a warm-up of each, then `runs` alternating launches; medians and whether the outputs agree bit for bit."""
    import ctypes as C
    from learning_environments_amd import _lib
    il, pos, kw = _ppo_loop(cfgd, chains)
    args = il._launch_args(*pos, kw["rng_keys"], None)
    other = C.CDLL(os.path.abspath(other_lib))
    fns = {"this_build": _lib.lib().lenv_ppo_rn_inner_loop, "other_build": other.lenv_ppo_rn_inner_loop}
    fns["other_build"].restype, fns["other_build"].argtypes = _lib.SIGNATURES["lenv_ppo_rn_inner_loop"]
    times, snaps = {k: [] for k in fns}, {}
    for r in range(runs + 1):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _lib.check(fn(C.byref(il.cfg), *args), k)
            torch.cuda.synchronize()
            if r:
                times[k].append(time.perf_counter() - t0)
            snaps[k] = [getattr(il, n).cpu().numpy().tobytes() for n in ("score", "stats", "status", "episode_test_mean", "episode_len", "final_params")]
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    out = dict(config=name, runs_each=runs, s_median=med, s_spread={k: max(v) - min(v) for k, v in times.items()},
               s_samples={k: [round(t, 5) for t in v] for k, v in times.items()}, ratio_this_to_other=med["this_build"] / med["other_build"],
               bit_identical=snaps["this_build"] == snaps["other_build"], status_ok=bool(int(il.status.min()) == 0))
    print(json.dumps(out))
    return out


def run_ppo_episode_time(name, env_name, episodes, models=10, agents=10, seed=0, icm=None):
    """Seconds per episode of the PPO transfer scripts' chains: models x agents chains at experiments/transfer_algo.py's PPO_SETTINGS of the env on a
    RewardEnv of the real env at full episode length, `episodes` segment launches of ONE episode each, every one timed on its own (the first is
    the warm-up and is left out); segments in which some chain ran PPO.learn and segments in which none did are reported apart (a segment lasts
    as long as its slowest chain).  icm: the chains of mode -1 (ppo_icm agents on the real env, the module of that dict) instead."""
    from learning_environments_amd.experiments import transfer_algo as ta
    cfgd = ta.base_config(env_name)
    cfgd["agents"]["ppo"] = dict(ta.PPO_SETTINGS[env_name])
    cfgd["envs"][env_name]["solved_reward"] = ta.SOLVED_REWARD[env_name]
    if icm is not None:
        cfgd["envs"][env_name]["reward_env_type"] = 0
    chains = models * agents
    il, pos, kw = _ppo_loop(cfgd, chains, models=models if icm is None else 1, seed=seed, icm=icm, train_episodes=episodes)
    calls = [0]
    times = _timed_segments(il, pos, kw, episodes, after=lambda: calls.append(int(il.stats[:, 2].sum())))
    learned = [b > a for a, b in zip(calls[:-1], calls[1:])]
    fin, status = il.segment_state()
    st = il.stats.cpu().numpy()
    med = lambda v: sorted(v)[len(v) // 2] if v else None
    with_learn = [t for t, l in list(zip(times, learned))[1:] if l]
    without = [t for t, l in list(zip(times, learned))[1:] if not l]
    out = dict(config=name, chains=chains, episodes=episodes, rows_per_learn=il.rows, ppo_epochs=il.cfg.ppo_epochs, max_steps=il.cfg.max_steps,
               same_action_num=il.cfg.same_action_num, s_per_episode_without_learn=med(without), s_per_episode_with_learn=med(with_learn),
               s_per_episode_mean=sum(times[1:]) / max(1, len(times) - 1), s_samples=[round(t, 4) for t in times], learn_in_segment=learned,
               status_ok=bool(int(status.min()) == 0), train_steps_per_chain=float(st[:, 1].mean()), learn_calls_per_chain=float(st[:, 2].mean()),
               test_steps_per_chain=float(st[:, 3].mean()), workspace_MiB=il.ws_bytes / 2.0 ** 20)
    print(json.dumps(out))
    return out


import bench  # noqa: E402  (the byte / FLOP models live next to the contract line)
HBM_PEAK_GBPS, MFMA_F32_PEAK_TFLOPS = bench.HBM_PEAK_GBPS, bench.MFMA_F32_PEAK_TFLOPS


def run_rn_step(name, chains=192, hidden=128, repeat=1, runs=7, iters=(40, 2000)):
    """One RewardEnv step of `chains` chains on the HalfCheetah stand-in (reward type 2, a `hidden`-wide one-hidden-layer PReLU reward net, 3 chains
    per NES worker with signs 0, +1, -1): lenv_rn_step_population against the composition of the older entries -- per repeat one lenv_cont_env_step
    launch and `chains` lenv_rn_shape_rows launches on the chain's perturbed theta (perturbed ahead of the clock) -- `runs` timed runs of `iters`
    = (composed, one launch) steps each, so that either window is a good part of a second, in alternation after a warm-up of each; medians and ranges per step; the two must agree bit for bit before anything is timed."""
    import numpy as np
    from learning_environments_amd import _lib, engine
    dev = engine.require_device()
    env_id, S, SD, A, max_steps, rtype, gamma = _lib.ENV["HalfCheetah-v3"], 17, 17, 6, 1000, 2, 0.99
    torch.manual_seed(0)
    desc = engine.mlp_desc(S, hidden, 1, 1, "prelu")
    P = engine.mlp_num_params(desc)
    pop = (chains + 2) // 3
    theta, eps = (0.3 * torch.randn(P)).to(dev), (0.1 * torch.randn(pop, P)).to(dev)
    worker = (torch.arange(chains, dtype=torch.int32) // 3).to(dev)
    sign = torch.tensor([(0.0, 1.0, -1.0)[c % 3] for c in range(chains)], device=dev)
    W = (sign[:, None] * eps[worker.long()] + theta).contiguous()            # signs 0, +1, -1: the product is exact, so this is the kernel's fmaf
    action = (torch.rand(chains, A) * 2 - 1).to(dev)
    L = _lib.lib()
    keys = torch.from_numpy(np.array([L.lenv_chain_key(0, 0, c, 3) for c in range(chains)], np.uint64).view(np.int64)).to(dev)
    state0, elapsed0 = torch.zeros((chains, SD), dtype=torch.float64, device=dev), torch.zeros(chains, dtype=torch.int32, device=dev)
    obs0 = torch.zeros((chains, S), dtype=torch.float32, device=dev)
    _lib.check(L.lenv_cont_env_reset(env_id, engine._ptr(keys), engine._ptr(torch.zeros(chains, dtype=torch.int64, device=dev)), chains, engine._ptr(state0),
                                     engine._ptr(obs0), engine._ptr(elapsed0), engine._stream()), "lenv_cont_env_reset")

    def composed():
        st, el, s, total = state0.clone(), elapsed0.clone(), obs0, None
        for _ in range(repeat):                      # (the stand-in ends through the TimeLimit only: no chain stops inside the repeat)
            ob, r, d = torch.empty_like(obs0), torch.empty(chains, device=dev), torch.empty(chains, device=dev)
            _lib.check(L.lenv_cont_env_step(env_id, max_steps, chains, engine._ptr(action), engine._ptr(st), engine._ptr(el), engine._ptr(ob), engine._ptr(r),
                                            engine._ptr(d), engine._stream()), "lenv_cont_env_step")
            shaped = torch.cat([engine.rn_shape_rows(rtype, desc, S, 0, gamma, W[c], s[c:c + 1], ob[c:c + 1], None, r[c:c + 1]) for c in range(chains)])
            total = shaped.double() if total is None else total + shaped.double()
            s = ob
        return ob, total.float(), d, st, el

    def fused():
        st, el = state0.clone(), elapsed0.clone()
        return engine.rn_step_population(env_id, max_steps, rtype, desc, 0, gamma, theta, eps, worker, sign, action, st, el, repeat=repeat) + (st, el)

    same = all(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)) for a, b in zip(composed(), fused()))
    assert same, "lenv_rn_step_population and the composition of the older entries differ"
    forms, times = (("composed", composed, iters[0]), ("one_launch", fused, iters[1])), {"composed": [], "one_launch": []}
    for it in range(runs + 1):
        for label, fn, n in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            if it:
                times[label].append((time.perf_counter() - t0) / n)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    out = dict(config=name, chains=chains, repeat=repeat, rn_hidden=hidden, runs_each=runs, steps_per_run=dict(composed=iters[0], one_launch=iters[1]), launches_per_step=dict(composed=repeat * (chains + 1), one_launch=1),
               us_median={k: 1e6 * v for k, v in med.items()}, us_min={k: 1e6 * min(v) for k, v in times.items()}, us_max={k: 1e6 * max(v) for k, v in times.items()},
               us_samples={k: [round(1e6 * x, 1) for x in v] for k, v in times.items()}, composed_over_one_launch=med["composed"] / med["one_launch"],
               bit_identical=bool(same))
    print(json.dumps(out))
    return out


def run_agent_test(name, cfgd, agents=400, test_episodes=10, runs=7, seed=0):
    """BaseAgent.test of `agents` freshly initialised agents of cfgd's shape, `test_episodes` episodes each (a fresh agent almost never ends a
    MountainCar / Acrobot episode, so nearly every episode runs to the time limit and both sides do the same steps): lenv_agent_test_population
    against the only route there was before it, the generic GEMM-queue kernel launched with train_episodes = 0 (its closing test alone; kernel_variant
    GENERIC | NO_WAVECHAIN keeps the launch on that kernel).  Host clock around a synchronise, a warm-up of each, then `runs` runs in alternation;
    medians and ranges; the returns must be equal before anything is timed."""
    from learning_environments_amd import _lib, engine
    from learning_environments_amd.agents import tasks
    from learning_environments_amd.agents.nes_common import chain_keys, fresh_agent_init
    import numpy as np
    eng = engine.HipNesEngine()
    dev = eng.device
    c = configs.fixed_work(cfgd, 0)
    key = c["agents"]["gtn"]["agent_name"].lower()
    c["agents"][key]["test_episodes"] = test_episodes
    c["agents"]["gtn"]["kernel_variant"] = _lib.VARIANT_GENERIC | _lib.VARIANT_NO_WAVECHAIN
    task = tasks.DdqnSeTask(c, eng)
    cfg = task.cfg
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    params = fresh_agent_init(task.agent_bounds, agents, g, dev)
    keys = torch.from_numpy(chain_keys(seed, 0, np.arange(agents), np.zeros(agents, np.int64)).view(np.int64)).to(dev)
    il = engine.InnerLoop(cfg, agents, want_episode_stats=True)
    assert il.dueling and il.p_agent == params.shape[1] == engine.agent_test_num_params(cfg)
    p_se = sum(engine.mlp_num_params(d) for d in engine.se_descs(cfg.state_dim, cfg.num_actions, cfg.se_hidden, cfg.se_layers, cfg.se_act))
    theta, eps = torch.zeros(p_se, device=dev), torch.zeros((1, p_se), device=dev)
    worker, sign = torch.zeros(agents, dtype=torch.int32, device=dev), torch.zeros(agents, device=dev)

    def generic():
        il.run(theta, eps, worker, sign, params, rng_keys=keys)
        return il.final_returns

    def entry():
        return engine.agent_test_population(cfg, params, keys, want_rows=False)["returns"]

    def entry_rows():
        return engine.agent_test_population(cfg, params, keys, want_rows=True)["returns"]

    ref = generic().clone()
    torch.cuda.synchronize()
    assert int(il.status.cpu().abs().max()) == 0
    same = bool(torch.equal(ref, entry())) and bool(torch.equal(ref, entry_rows()))
    assert same, "lenv_agent_test_population and the generic kernel's closing test differ"
    forms = (("generic_train_episodes_0", generic), ("agent_test_population", entry), ("agent_test_population_with_rows", entry_rows))
    times = {label: [] for label, _ in forms}
    for it in range(runs + 1):
        for label, fn in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it:
                times[label].append(time.perf_counter() - t0)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    out = dict(config=name, agents=agents, test_episodes=test_episodes, max_steps=cfg.max_steps, params_per_agent=int(params.shape[1]), runs_each=runs,
               test_steps=int(il.stats[:, 3].sum()), ms_median={k: 1e3 * v for k, v in med.items()}, ms_min={k: 1e3 * min(v) for k, v in times.items()},
               ms_max={k: 1e3 * max(v) for k, v in times.items()}, ms_samples={k: [round(1e3 * x, 3) for x in v] for k, v in times.items()},
               generic_over_entry=med["generic_train_episodes_0"] / med["agent_test_population"], same_returns=same)
    print(json.dumps(out))
    return out


def run_actor_test(name, cfgd, kind, agents=400, test_episodes=10, runs=7, seed=0):
    """BaseAgent.test of `agents` freshly initialised TD3 / PPO agents of cfgd's shape, `test_episodes` episodes each: lenv_actor_test_population
    against the only route there was before it, the fused entry launched with train_episodes = 0 (its closing test alone) -- as the launch
    picks its kernel and, for TD3, also with kernel_variant GENERIC | NO_WAVECHAIN (the GEMM-queue kernel).  Host clock around a synchronise, a
    warm-up of each, then `runs` runs in alternation; medians and ranges; the returns must be equal before anything is timed."""
    from learning_environments_amd import _lib, engine
    from learning_environments_amd.agents import tasks
    from learning_environments_amd.agents.nes_common import chain_keys, fresh_agent_init, set_layer_norm_init
    import numpy as np
    eng = engine.HipNesEngine()
    dev = eng.device
    c = configs.fixed_work(cfgd, 0)
    c["agents"][kind]["test_episodes"] = test_episodes
    task = (tasks.Td3RnTask if kind == "td3" else tasks.PpoRnTask)(c, eng)
    cfg = task.cfg
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    params = fresh_agent_init(task.agent_bounds, agents, g, dev)
    if kind == "td3":
        set_layer_norm_init(params, task.ln_slice)
    else:
        params[:, :cfg.action_dim] = float(cfg.action_std)
    keys = torch.from_numpy(chain_keys(seed, 0, np.arange(agents), np.zeros(agents, np.int64)).view(np.int64)).to(dev)
    loops = {}
    if kind == "td3":
        loops["fused_train_episodes_0"] = engine.Td3InnerLoop(cfg, agents, want_episode_stats=True)
        queue_cfg = _lib.Td3Cfg.from_buffer_copy(cfg)
        queue_cfg.kernel_variant = _lib.VARIANT_GENERIC | _lib.VARIANT_NO_WAVECHAIN
        loops["fused_gemm_queue_train_episodes_0"] = engine.Td3InnerLoop(queue_cfg, agents, want_episode_stats=True)
        if cfg.virtual_env:
            p_theta = sum(engine.mlp_num_params(d) for d in engine.se_descs(cfg.state_dim, cfg.action_dim, cfg.rn_hidden, cfg.rn_layers, cfg.rn_act))
        else:
            p_theta = engine.rn_num_params(cfg.reward_env_type, cfg.state_dim, cfg.info_dim, cfg.rn_hidden, cfg.rn_layers)
    else:
        loops["fused_train_episodes_0"] = engine.PpoInnerLoop(cfg, agents, want_episode_stats=True)
        p_theta = loops["fused_train_episodes_0"].p_theta
    first = loops["fused_train_episodes_0"]
    assert first.p_agent == params.shape[1] == engine.actor_test_num_params(kind, cfg)
    theta, eps = torch.zeros(max(p_theta, 1), device=dev)[:p_theta].contiguous(), torch.zeros((1, p_theta), device=dev)
    worker, sign = torch.zeros(agents, dtype=torch.int32, device=dev), torch.zeros(agents, device=dev)

    def fused(il):
        def f():
            il.run(theta, eps, worker, sign, params, rng_keys=keys)
            return il.final_returns
        return f

    def entry():
        return engine.actor_test_population(kind, cfg, params, keys, want_rows=False)["returns"]

    def entry_rows():
        return engine.actor_test_population(kind, cfg, params, keys, want_rows=True)["returns"]

    forms = tuple((label, fused(il)) for label, il in loops.items()) + (("actor_test_population", entry), ("actor_test_population_with_rows", entry_rows))
    ref = forms[0][1]().clone()
    torch.cuda.synchronize()
    assert int(first.status.cpu().abs().max()) == 0
    same = all(bool(torch.equal(ref, fn())) for _, fn in forms[1:])
    assert same, "lenv_actor_test_population and the fused kernels' closing test differ"
    times = {label: [] for label, _ in forms}
    for it in range(runs + 1):
        for label, fn in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it:
                times[label].append(time.perf_counter() - t0)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    out = dict(config=name, kind=kind, agents=agents, test_episodes=test_episodes, max_steps=cfg.max_steps, params_per_agent=int(params.shape[1]),
               runs_each=runs, test_steps=int(first.stats[:, 3].sum()), ms_median={k: 1e3 * v for k, v in med.items()},
               ms_min={k: 1e3 * min(v) for k, v in times.items()}, ms_max={k: 1e3 * max(v) for k, v in times.items()},
               ms_samples={k: [round(1e3 * x, 3) for x in v] for k, v in times.items()},
               fused_over_entry={k: med[k] / med["actor_test_population"] for k in loops}, same_returns=same)
    print(json.dumps(out))
    return out


def _time_forms(forms, runs):
    """a warm-up of each form, then `runs` runs in alternation, host clock around a synchronise: (medians, all samples) in seconds"""
    times = {label: [] for label, _ in forms}
    for it in range(runs + 1):
        for label, fn in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it:
                times[label].append(time.perf_counter() - t0)
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}, times


def run_discrete_actor_test(name, cfgd, agents=400, test_episodes=10, runs=7, seed=0):
    """BaseAgent.test of `agents` freshly initialised TD3_discrete_vary agents of cfgd's shape, `test_episodes` episodes each:
    lenv_td3d_test_population against the only route there was before it, lenv_td3d_inner_loop launched with train_episodes = 0 (its closing
    test alone, at the start temperature, behind a full training arena per chain).  Host clock around a synchronise, a warm-up of each, then
    `runs` runs in alternation; medians and ranges; the returns must be equal before anything is timed."""
    from learning_environments_amd import engine
    from learning_environments_amd.agents import tasks
    from learning_environments_amd.agents.nes_common import chain_keys
    import numpy as np
    eng = engine.HipNesEngine()
    dev = eng.device
    c = configs.fixed_work(cfgd, 0)
    c["agents"]["td3_discrete_vary"]["test_episodes"] = test_episodes
    task = tasks.Td3DiscreteTask(c, eng)
    cfg = task.cfg
    keys = torch.from_numpy(chain_keys(seed, 0, np.arange(agents), np.zeros(agents, np.int64)).view(np.int64)).to(dev)
    il = engine.Td3DiscreteInnerLoop(cfg, agents, want_episode_stats=True, want_final_params=True)
    params = il.draw_agent_init(keys).clone()
    assert il.p_agent == params.shape[1] == engine.td3d_test_num_params(cfg)
    theta, eps = torch.zeros(il.p_theta, device=dev), torch.zeros((1, il.p_theta), device=dev)
    worker, sign = torch.zeros(agents, dtype=torch.int32, device=dev), torch.zeros(agents, device=dev)

    def fused():
        il.run(theta, eps, worker, sign, params, rng_keys=keys)
        return il.final_returns

    def entry():
        return engine.td3d_test_population(cfg, params, keys, want_rows=False)["returns"]

    def entry_rows():
        return engine.td3d_test_population(cfg, params, keys, want_rows=True)["returns"]

    forms = (("fused_train_episodes_0", fused), ("td3d_test_population", entry), ("td3d_test_population_with_rows", entry_rows))
    ref = fused().clone()
    torch.cuda.synchronize()
    assert int(il.status.cpu().abs().max()) == 0
    same = all(bool(torch.equal(ref, fn())) for _, fn in forms[1:])
    assert same, "lenv_td3d_test_population and the fused kernel's closing test differ"
    med, times = _time_forms(forms, runs)
    out = dict(config=name, agents=agents, test_episodes=test_episodes, max_steps=cfg.max_steps, params_per_agent=int(params.shape[1]),
               workspace_mib_fused=il.ws_bytes / 2 ** 20, runs_each=runs, test_steps=int(il.stats[:, 3].sum()), ms_median={k: 1e3 * v for k, v in med.items()},
               ms_min={k: 1e3 * min(v) for k, v in times.items()}, ms_max={k: 1e3 * max(v) for k, v in times.items()},
               ms_samples={k: [round(1e3 * x, 3) for x in v] for k, v in times.items()},
               fused_over_entry=med["fused_train_episodes_0"] / med["td3d_test_population"], same_returns=same)
    print(json.dumps(out))
    return out


def run_ql_test(name, agents=400, test_episodes=10, runs=7, seed=0):
    """BaseAgent.test of `agents` Cliff Q-tables: lenv_ql_test_population against lenv_ql_rn_inner_loop launched with train_episodes = 0 (all-zero
    tables: the fused loop cannot be handed a trained one) and, for the entry alone, on random tables.  Not a throughput item -- a greedy walk
    on a deterministic grid is serial and short -- so both sides are a launch and a few hundred dependent loads."""
    from learning_environments_amd import engine
    from learning_environments_amd.agents.nes_common import chain_keys
    from learning_environments_amd.config import ql_cfg_from_config
    from learning_environments_amd.envs.gridworld import transition_tables
    import numpy as np
    dev = engine.require_device()
    c = configs.fixed_work(configs.cliff_reward_env_ql(16), 0)
    c["agents"]["ql"]["test_episodes"] = test_episodes
    tables = transition_tables("Cliff")
    cfg = ql_cfg_from_config(c, tables)
    il = engine.QlInnerLoop(cfg, agents, tables)
    keys = torch.from_numpy(chain_keys(seed, 0, np.arange(agents), np.zeros(agents, np.int64)).view(np.int64)).to(dev)
    theta, eps = torch.zeros(il.p_theta, device=dev), torch.zeros((1, il.p_theta), device=dev)
    worker, sign = torch.zeros(agents, dtype=torch.int32, device=dev), torch.zeros(agents, device=dev)
    dtab = dict(next_state=il.next_state, reward=il.reward, done=il.done)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    q_random = torch.randn((agents, cfg.n_states * cfg.n_actions), generator=g, device=dev, dtype=torch.float64)

    def fused():
        il.run(theta, eps, worker, sign, rng_keys=keys)
        return il.final_returns

    forms = (("fused_train_episodes_0", fused),
             ("ql_test_population", lambda: engine.ql_test_population(cfg, il.q_table, dtab, want_rows=False)["returns"]),
             ("ql_test_population_with_rows", lambda: engine.ql_test_population(cfg, il.q_table, dtab, want_rows=True)["returns"]),
             ("ql_test_population_random_tables", lambda: engine.ql_test_population(cfg, q_random, dtab, want_rows=False)["returns"]))
    ref = fused().clone()
    torch.cuda.synchronize()
    assert int(il.status.cpu().abs().max()) == 0
    same = all(bool(torch.equal(ref, fn())) for _, fn in forms[1:3])
    assert same, "lenv_ql_test_population and the fused kernel's closing test differ"
    med, times = _time_forms(forms, runs)
    out = dict(config=name, agents=agents, test_episodes=test_episodes, max_steps=cfg.max_steps, runs_each=runs, test_steps=int(il.stats[:, 3].sum()),
               ms_median={k: 1e3 * v for k, v in med.items()}, ms_min={k: 1e3 * min(v) for k, v in times.items()},
               ms_max={k: 1e3 * max(v) for k, v in times.items()}, ms_samples={k: [round(1e3 * x, 3) for x in v] for k, v in times.items()},
               fused_over_entry=med["fused_train_episodes_0"] / med["ql_test_population"], same_returns=same)
    print(json.dumps(out))
    return out


def run_se_fit(name, models=5, steps=9500, batch=64, rows=2000, runs=7, torch_models=None, seed=0):
    """The supervised VirtualEnv fit at the published CartPole SE shape (6-128-{4,1,1}, leakyrelu): lenv_se_fit_population for `models` models
    in one launch against the only route there was, an eager torch loop (three nn.Sequential, one torch.optim.Adam, F.mse_loss) fitting
    `torch_models` of them one after the other on the device from the same data, initial weights and index tapes (None: all of them; 0: the
    torch side is not run).  Host clock around a synchronise, a warm-up of each, then `runs` runs in alternation; medians and ranges."""
    from learning_environments_amd import engine
    from learning_environments_amd.experiments import mbrl_baseline as mb
    from learning_environments_amd.envs.env_factory import EnvFactory
    import numpy as np
    dev = engine.require_device()
    config = configs.with_vary(configs.cartpole_syn_env_ddqn(num_workers=1))
    config["envs"]["CartPole-v0"]["hidden_size"] = 128
    config["device"] = "cuda"
    fac = EnvFactory(config)
    venv = fac.generate_virtual_env()
    x, y_state, y_reward, y_done = mb.rows_to_dataset(venv, mb.collect_transitions(fac.generate_real_env(), rows, seed=seed))
    descs = venv.env.descs()
    P = engine.se_fit_num_params(descs)
    g = torch.Generator().manual_seed(seed)
    theta0 = ((torch.rand((models, P), generator=g) * 2 - 1) * torch.from_numpy(mb._se_bounds(descs))).to(dev)
    tape = torch.randint(0, rows, (models, steps, batch), generator=g, dtype=torch.int32).to(dev)
    torch_models = models if torch_models is None else torch_models
    last = {}

    def kernel():
        last["kernel"] = engine.se_fit_population(descs, theta0, x, y_state, y_reward, y_done, batch, steps, batch_idx=tape)

    def eager():
        ys = (y_state, y_reward.reshape(-1, 1), y_done.reshape(-1, 1))
        finals, tails = [], []
        for m in range(torch_models):
            nets, off = [], 0
            for d in descs:
                net = torch.nn.Sequential(torch.nn.Linear(d.in_dim, d.hidden), torch.nn.LeakyReLU(), torch.nn.Linear(d.hidden, d.out_dim)).to(dev)
                with torch.no_grad():
                    for prm in net.parameters():
                        prm.copy_(theta0[m, off:off + prm.numel()].reshape(prm.shape))
                        off += prm.numel()
                nets.append(net)
            opt = torch.optim.Adam([p for n in nets for p in n.parameters()], lr=1e-3)
            idx = tape[m].long()
            for t in range(steps):
                opt.zero_grad()
                xb = x[idx[t]]
                total = sum(torch.nn.functional.mse_loss(n(xb), y[idx[t]]) for n, y in zip(nets, ys))
                total.backward()
                opt.step()
                if t >= steps - 10:
                    tails.append(total.detach())
            finals.append(torch.cat([p.detach().reshape(-1) for n in nets for p in n.parameters()]))
        last["torch"], last["torch_loss"] = torch.stack(finals), torch.stack(tails).reshape(torch_models, -1).mean(dim=1)

    forms = (("se_fit_population", kernel),) + ((("torch_eager", eager),) if torch_models else ())
    med, times = _time_forms(forms, runs)
    out = dict(config=name, models=models, torch_models=torch_models, steps=steps, batch=batch, rows=rows, params_per_model=P, runs_each=runs,
               ms_median={k: 1e3 * v for k, v in med.items()}, ms_min={k: 1e3 * min(v) for k, v in times.items()},
               ms_max={k: 1e3 * max(v) for k, v in times.items()}, ms_samples={k: [round(1e3 * x, 3) for x in v] for k, v in times.items()},
               us_per_step_kernel=1e6 * med["se_fit_population"] / steps,
               final_loss_kernel=[float(v) for v in last["kernel"]["loss"][:, -10:].sum(dim=2).mean(dim=1).cpu()][:5])
    if torch_models:
        out["torch_over_kernel_per_model"] = (med["torch_eager"] / torch_models) / (med["se_fit_population"] / models)
        out["final_loss_torch"] = [float(v) for v in last["torch_loss"].cpu()]
        out["max_abs_theta_diff_to_torch"] = float((last["kernel"]["theta"][:torch_models] - last["torch"]).abs().max())
    print(json.dumps(out))
    return out


def _frac(model):
    def f(cfg, st, dt):
        nbytes, flops = model(cfg, st)
        return dict(algorithmic_GBps=nbytes / dt / 1e9, hbm_frac=nbytes / dt / 1e9 / HBM_PEAK_GBPS, fp32_TFLOPs=flops / dt / 1e12,
                    mfma_f32_frac=flops / dt / 1e12 / MFMA_F32_PEAK_TFLOPS, busy_cus=int(st.shape[0]))
    return f


dueling_model, td3_model = _frac(bench.dueling_model), _frac(bench.td3_model)


def ppo_model(cfg, st, dt):
    """PPO.learn's layer products: forward, input gradient and weight gradient of both nets over the N rows = 6 N W flops per epoch per chain
    (W = weights of actor.net + critic.net); the rollout (one row at a time) is not counted.  The fraction is of the busy CUs' share of the peak."""
    from learning_environments_amd.config import ppo_cfg_from_config, ppo_rows
    c = ppo_cfg_from_config(cfg)
    S, A, H, L = c.state_dim, c.action_dim, c.hidden, c.layers
    W = 2 * (S * H + (L - 1) * H * H) + A * H + H
    epochs = float(st[:, 2].sum()) * c.ppo_epochs
    flops = 6.0 * ppo_rows(c) * W * epochs
    busy = min(int(st.shape[0]), 256)
    return dict(rows_per_learn=ppo_rows(c), learn_epochs=int(epochs), us_per_learn_epoch_per_chain=1e6 * dt / max(1.0, epochs / st.shape[0]),
                fp32_TFLOPs=flops / dt / 1e12, mfma_f32_frac_of_busy_cus=flops / dt / 1e12 / (MFMA_F32_PEAK_TFLOPS * busy / 256.0), busy_cus=busy)


if __name__ == "__main__":
    which = sys.argv[1:] or ["2", "3", "4", "5", "td3d"]
    if "2" in which:
        run("cfg2 CartPole SE + DDQN pop 64 (20 episodes)", configs.fixed_work(configs.cartpole_syn_env_ddqn(64), 20))
    if "2full" in which:
        # every CU busy: 85 workers = 255 chains on 256 CUs (BASELINE's metric is quoted at pop 64 = 192 chains)
        run("cfg2 CartPole SE + DDQN pop 85 = 255 chains (20 episodes)", configs.fixed_work(configs.cartpole_syn_env_ddqn(85), 20))
    if "4" in which:
        c = configs.cliff_reward_env_ql(128)
        c["agents"]["gtn"]["quit_when_solved"] = False
        run("cfg4 Cliff RN + QL pop 128 (100 episodes, early-out on)", c)
    if "3" in which:
        c = configs.fixed_work(configs.acrobot_syn_env_duelingddqn(32), 3)
        c["agents"]["duelingddqn"]["init_episodes"] = 1
        c["envs"]["Acrobot-v1"]["max_steps"] = 100
        run("cfg3 Acrobot SE + DuelingDDQN pop 32 (3 episodes x 100 steps)", c, gens=1, extra=dueling_model)
    if "3full" in which:
        # the same workload with every CU busy (85 workers = 255 chains on 256 CUs): what the kernel delivers per chip rather
        # than per BASELINE's 8-GPU shard of 32 workers
        c = configs.fixed_work(configs.acrobot_syn_env_duelingddqn(85), 3)
        c["agents"]["duelingddqn"]["init_episodes"] = 1
        c["envs"]["Acrobot-v1"]["max_steps"] = 100
        run("cfg3 Acrobot SE + DuelingDDQN pop 85 = 255 chains (3 episodes x 100 steps)", c, gens=1, extra=dueling_model)
    if "5full" in which:
        c = configs.fixed_work(configs.halfcheetah_reward_env_td3(85), 3)
        c["agents"]["td3"]["init_episodes"] = 1
        c["envs"]["HalfCheetah-v3"]["max_steps"] = 100
        run("cfg5 HalfCheetah-standin RN + TD3 pop 85 = 255 chains (3 episodes x 100 steps)", c, gens=1, extra=td3_model)
    if "acrobot_ddqn" in which:
        # default_config_acrobot.yaml's ddqn section (Critic_DQN 6-128-128-3, B = 128) on 96 chains: the wave-chain kernel's plain-DQN
        # shape, then the same launch on the GEMM-queue kernel (gtn.kernel_variant = NO_WAVECHAIN)
        from learning_environments_amd import _lib
        for variant, label in ((0, "wave-chain kernel"), (_lib.VARIANT_NO_WAVECHAIN, "GEMM-queue kernel")):
            c = configs.fixed_work(configs.acrobot_syn_env_ddqn(32), 3)
            c["envs"]["Acrobot-v1"]["max_steps"] = 100
            c["agents"]["gtn"]["kernel_variant"] = variant
            run("Acrobot SE + DDQN 6-128-128-3 pop 32 (3 episodes x 100 steps), " + label, c, gens=2)
    if "pendulum_td3" in which:
        # default_config_pendulum_reward_env.yaml (TD3 3-128-128-1 / 4-128-128-1 leakyrelu, B = 192, ten test episodes, reward net with two
        # hidden layers) at its own population (16 workers = 48 chains) and at 32 workers = 96 chains: the wave-chain kernel's second TD3
        # shape (teams of 3 / 2), then the same launches on the GEMM-queue kernel
        from learning_environments_amd import _lib
        for pop in (16, 32):
            for variant, label in ((0, "wave-chain kernel"), (_lib.VARIANT_NO_WAVECHAIN, "GEMM-queue kernel")):
                c = configs.fixed_work(configs.pendulum_reward_env_td3(pop), 3)
                c["agents"]["td3"]["init_episodes"] = 1
                c["envs"]["Pendulum-v0"]["max_steps"] = 100
                c["agents"]["gtn"]["kernel_variant"] = variant
                run("Pendulum RN + TD3 pop %d (3 episodes x 100 steps), %s" % (pop, label), c, gens=2)
    if "cmc_td3" in which:
        # default_config_cmc_reward_env.yaml (TD3 2-128-128-1 / 3-128-128-1 leakyrelu, B = 192, same_action_num 2, one test episode) at its own
        # population (16 workers = 48 chains): the wave-chain kernel's third TD3 shape, then the GEMM-queue kernel
        from learning_environments_amd import _lib
        for pop in (16, 32):
            for variant, label in ((0, "wave-chain kernel"), (_lib.VARIANT_NO_WAVECHAIN, "GEMM-queue kernel")):
                c = configs.fixed_work(configs.cmc_reward_env_td3(pop), 3)
                c["agents"]["td3"]["init_episodes"] = 1
                c["envs"]["MountainCarContinuous-v0"]["max_steps"] = 200
                c["agents"]["gtn"]["kernel_variant"] = variant
                run("MountainCarContinuous RN + TD3 pop %d (3 episodes x 100 agent steps), %s" % (pop, label), c, gens=2)
    if "cmc_venv_td3" in which:
        # default_config_cmc.yaml (TD3 2-128-128-1 / 3-128-128-1 relu, B = 256, policy_delay 2, same_action_num 2, trained on a VirtualEnv
        # of three 3-96-96-x nets) at its own population (128 workers = 384 chains, one workgroup per chain), as one 8-GPU shard (16 workers =
        # 48 chains, teams of 4) and at 4 workers (teams of 8): the wave-chain kernel's fourth TD3 shape, then the GEMM-queue kernel
        from learning_environments_amd import _lib
        for pop in (128, 16, 4):
            for variant, label in ((0, "wave-chain kernel"), (_lib.VARIANT_NO_WAVECHAIN, "GEMM-queue kernel")):
                c = configs.fixed_work(configs.cmc_syn_env_td3(pop), 3)
                c["agents"]["td3"]["init_episodes"] = 1
                c["envs"]["MountainCarContinuous-v0"]["max_steps"] = 200
                c["agents"]["gtn"]["kernel_variant"] = variant
                run("MountainCarContinuous SE + TD3 (B 256, policy_delay 2) pop %d (3 episodes x 100 agent steps), %s" % (pop, label), c, gens=2)
    if "venv_td3" in which:
        # the td3 sections of default_config_pendulum.yaml (16 workers) and default_config_halfcheetah.yaml (one 8-GPU shard of its 128 workers)
        # as fixed-shape agents (`td3_vary` with vary_hp off): wave-chain shapes 5 / 6 (teams of 4), then the GEMM-queue kernel
        from learning_environments_amd import _lib
        for make, env_name, label0, steps in ((configs.pendulum_syn_env_td3, "Pendulum-v0", "Pendulum SE 4-32-32-x", 100), (configs.halfcheetah_syn_env_td3, "HalfCheetah-v3", "HalfCheetah-standin SE 23-128-128-128-x", 100)):
            for variant, label in ((0, "wave-chain kernel"), (_lib.VARIANT_NO_WAVECHAIN, "GEMM-queue kernel")):
                c = configs.fixed_work(make(16), 3)
                c["agents"]["td3"]["init_episodes"] = 1
                c["envs"][env_name]["max_steps"] = steps
                c["agents"]["gtn"]["kernel_variant"] = variant
                run("%s + TD3 (B 256, policy_delay 2, ten test episodes) pop 16 (3 episodes x %d steps), %s" % (label0, steps, label), c, gens=2)
    if "mountaincar_ddqn" in which:
        # default_config_mountaincar.yaml (DDQN 2-256-256-3 relu, B = 128, ten test episodes, 16 workers = 48 chains): the 256-wide wave-chain
        # kernel (teams of 4 at 48 chains, 2 at 96), then the GEMM-queue kernel (gtn.kernel_variant = NO_WAVECHAIN)
        from learning_environments_amd import _lib
        for pop in (16, 32):
            for variant, label in ((0, "wave-chain kernel"), (_lib.VARIANT_NO_WAVECHAIN, "GEMM-queue kernel")):
                c = configs.fixed_work(configs.mountaincar_syn_env_ddqn(pop), 3)
                c["agents"]["ddqn"]["init_episodes"] = 1
                c["envs"]["MountainCar-v0"]["max_steps"] = 100
                c["agents"]["gtn"]["kernel_variant"] = variant
                run("MountainCar SE + DDQN 2-256-256-3 pop %d (3 episodes x 100 steps), %s" % (pop, label), c, gens=2)
    if "cartpole_rn_ddqn" in which:
        # default_config_cartpole_reward_env.yaml (DDQN 4-64-2 leakyrelu, B = 192, trained on the real CartPole with a learned reward, 16 workers)
        # round 6: the register-resident kernel's RENV instantiation (real-env training step + reward net on the env wave), then the GEMM-queue kernel
        for pop in (16, 64):
            for force, label in ((False, "register-resident kernel (RENV)"), (True, "GEMM-queue kernel")):
                c = configs.fixed_work(configs.cartpole_reward_env_ddqn(pop), 6)
                c["agents"]["gtn"]["quit_when_solved"] = False
                run("CartPole RewardEnv + DDQN 4-64-2 pop %d (6 episodes), %s" % (pop, label), c, gens=2, force_gemm=force)
    if "cmc_opt_td3" in which:
        # default_config_cmc_syn_env_opt.yaml-like: TD3 with ONE 64-wide hidden layer on a VirtualEnv of three 3-128-128-128-x nets, B = 256
        # round 6: the DIRECT instantiation (narrow nets skip the product queue), then the queued path (gtn.kernel_variant = NO_DIRECT)
        from learning_environments_amd import _lib
        for pop in (16, 64):
            for variant, label in ((0, "GEMM-queue kernel, DIRECT layer products"), (_lib.VARIANT_NO_DIRECT, "GEMM-queue kernel, queued products")):
                c = configs.fixed_work(configs.cmc_syn_env_td3(pop), 3)
                c["agents"]["td3"].update(init_episodes=1, hidden_size=64, hidden_layer=1, activation_fn="leakyrelu")
                c["envs"]["MountainCarContinuous-v0"].update(max_steps=200, hidden_size=128, hidden_layer=3, activation_fn="relu")
                c["agents"]["gtn"]["kernel_variant"] = variant
                run("MountainCarContinuous SE 128x3 + TD3 64x1 (B 256) pop %d (3 episodes x 100 agent steps), %s" % (pop, label), c, gens=2)
    if "td3d" in which:
        # TD3_discrete_vary as the syn-env YAMLs ship it (510-wide tanh nets, batch 122, hard Gumbel softmax) on an Acrobot SE
        c = configs.fixed_work(configs.acrobot_syn_env_td3_discrete(32), 3)
        c["envs"]["Acrobot-v1"]["max_steps"] = 100
        run("TD3_discrete_vary on an Acrobot SE, pop 32 (3 episodes x 100 steps, shipped 510-wide nets)", c, gens=1)
        c = configs.fixed_work(configs.cartpole_syn_env_td3_discrete(32, hidden_size=128, batch_size=128, use_layer_norm=True, activation_fn="relu"), 3)
        c["envs"]["CartPole-v0"]["max_steps"] = 100
        run("TD3_discrete_vary + LayerNorm on a CartPole SE, pop 32 (128-wide relu nets, batch 128)", c, gens=1)
    if "td3drn" in which:
        # TD3_discrete_vary (the shipped section) on default_config_cartpole_reward_env.yaml's RewardEnv (PReLU 4-64-1, type 2) against the same
        # agent on a CartPole SE, at 16 and 64 workers (48 / 192 chains); per-step cost = seconds per generation / mean env steps of a chain
        per_step = lambda cfg, st, dt: dict(us_per_train_step_per_chain=1e6 * dt / max(1.0, st[:, 1].mean()))
        for pop in (16, 64):
            c = configs.cartpole_reward_env_ddqn(pop)
            c["agents"]["gtn"]["agent_name"] = "TD3_discrete_vary"
            c["agents"].pop("ddqn")
            c["agents"]["td3_discrete_vary"] = configs._td3_discrete_section()
            c = configs.fixed_work(c, 3)
            c["envs"]["CartPole-v0"]["max_steps"] = 100
            run("TD3_discrete_vary on a CartPole RewardEnv (type 2), pop %d (3 episodes x <= 100 steps, shipped 510-wide nets)" % pop, c, gens=1,
                extra=per_step)
            c = configs.fixed_work(configs.cartpole_syn_env_td3_discrete(pop), 3)
            c["envs"]["CartPole-v0"]["max_steps"] = 100
            run("TD3_discrete_vary on a CartPole SE, pop %d (3 episodes x 100 steps, shipped 510-wide nets)" % pop, c, gens=1, extra=per_step)
    if "ppo" in which:
        # PPO (two 64-wide relu layers, 1001 rows x 10 epochs per learn call) on default_config_pendulum_reward_env.yaml's RewardEnv at its own
        # population (16 workers = 48 chains) and at 64 workers = 192 chains; 10 training episodes = 2000 rows = ONE learn call per chain; a warm-up
        # generation, then the median of 7 generations timed one by one
        # (Pendulum episodes never end early: the rollout is the same work whatever the policy, so the difference of two generations that differ
        # in ppo_epochs only is the cost of the extra epochs -- us per learn epoch and the MFMA fraction are taken from it)
        for pop in (16, 64):
            res = {}
            for epochs in (10, 30):
                c = configs.fixed_work(configs.pendulum_reward_env_ppo(pop, train_episodes=10, ppo_epochs=epochs), 10)
                c["agents"]["gtn"]["quit_when_solved"] = False
                res[epochs] = run("Pendulum RN + PPO 64x2 pop %d (10 episodes x 200 steps, 1 learn call x %d epochs x 1001 rows)" % (pop, epochs), c, gens=7,
                                  extra=ppo_model, median=True)
            d_t = res[30]["s_per_generation"] - res[10]["s_per_generation"]
            d_ep = (res[30]["learn_epochs"] - res[10]["learn_epochs"]) / float(res[10]["chains"])
            W = 2 * (3 * 64 + 64 * 64) + 64 + 64
            flops = 6.0 * 1001 * W * d_ep * res[10]["chains"]
            print(json.dumps(dict(config="Pendulum RN + PPO 64x2 pop %d: the extra epochs alone" % pop, chains=res[10]["chains"], extra_epochs_per_chain=d_ep,
                                  us_per_learn_epoch=1e6 * d_t / d_ep, rollout_and_rest_s=res[10]["s_per_generation"] - 10 * d_t / d_ep,
                                  mfma_f32_frac_of_busy_cus=flops / d_t / 1e12 / (MFMA_F32_PEAK_TFLOPS * min(res[10]["chains"], 256) / 256.0))))
    if "ql_se" in which:
        # default_config_gridworld.yaml with synthetic_env_type 0: tabular QL on a Cliff VirtualEnv (three 52-32-x leakyrelu nets), 128 workers = 384
        # chains, 100 training episodes, no early-out; theta = the fitted SE of the g15a fixture so that episodes have realistic lengths.  A warm-up
        # generation, then the median of 7 timed one by one; per-step cost = seconds per generation / mean training steps of a chain
        import numpy as np
        th = np.load(os.path.join(ROOT, "tests", "golden", "g15a_ql_se_cliff_ql.npz"))["theta"]
        c = configs.fixed_work(configs.cliff_syn_env_ql(128), 100)
        c["agents"]["gtn"]["quit_when_solved"] = False
        run("Cliff SE + QL pop 128 = 384 chains (100 episodes, no early-out, fitted SE)", c, gens=7, median=True, theta=th,
            extra=lambda cfg, st, dt: dict(us_per_train_step_per_chain=1e6 * dt / max(1.0, st[:, 1].mean()), train_steps_per_chain=float(st[:, 1].mean()),
                                           test_steps_per_chain=float(st[:, 3].mean())))
        # the same launch on the freshly initialised SE: its done output never passes 0.5, every episode runs its 50 steps (5 000 training steps per
        # chain against about 250 on the fitted SE, the same 100 test episodes) -- the two rows together separate the cost of a training step (three
        # nets + argmax + update) from the cost of a test step (a table walk)
        run("Cliff SE + QL pop 128 = 384 chains (100 episodes x 50 steps, freshly initialised SE)", configs.fixed_work(configs.cliff_syn_env_ql(128), 100),
            gens=7, median=True, extra=lambda cfg, st, dt: dict(train_steps_per_chain=float(st[:, 1].mean()), test_steps_per_chain=float(st[:, 3].mean())))
    if "test_mode1" in which:
        # the evaluation harness's training call on the wave-chain kernels' shapes: Acrobot SE + DuelingDDQN at 96 chains (ten init episodes + two
        # learning ones of up to 500 steps) and the Pendulum RewardEnv + TD3 at 48 chains (twenty init episodes + two learning ones of 200 steps)
        run_test_mode1_ab("Acrobot SE + DuelingDDQN pop 32, test_mode 1 (12 episodes)", configs.fixed_work(configs.acrobot_syn_env_duelingddqn(32), 12))
        run_test_mode1_ab("Pendulum RN + TD3 pop 16, test_mode 1 (22 episodes x 200 steps)", configs.fixed_work(configs.pendulum_reward_env_td3(16), 22))
    if "td3_segments" in which:
        # default_config_cmc.yaml's TD3 shape (2-128-128-1 / 3-128-128-1 relu, B 256, policy_delay 2, same_action_num 2, a VirtualEnv of three
        # 3-96-96-x nets) on 48 chains, 60 episodes of 100 agent steps (6 init episodes): the old entry, one segment, six segments
        c = configs.fixed_work(configs.cmc_syn_env_td3(16), 60)
        c["agents"]["td3"]["init_episodes"] = 6
        c["envs"]["MountainCarContinuous-v0"]["max_steps"] = 200
        run_segments("MountainCarContinuous SE + TD3 (B 256) 48 chains, 60 episodes x 100 agent steps: 1 launch / 1 segment / 6 segments",
                     _td3_loop(c, 48, train_episodes=60), "final_params", 60, 6)
    if "td3d_segments" in which:
        # the evaluation harness's TD3_discrete chains (4-128-128-2 tanh with LayerNorm, test_mode 1) on the reference-written CartPole SE, 48 chains,
        # 60 episodes (6 init episodes) of 40 steps, the checkpoint's max_steps (this SE never reports done): the old entry, one segment, six segments; then the same with ONE chain (no chain
        # waits for another at a boundary: what is left is the cost of splitting itself)
        run_segments("CartPole SE + TD3_discrete 128x2 LayerNorm, 48 chains, 60 episodes x 40 steps: 1 launch / 1 segment / 6 segments",
                     _td3d_loop(48, 60), "final_params", 60, 6, boundary_wait=True)
        run_segments("CartPole SE + TD3_discrete 128x2 LayerNorm, 1 chain, 60 episodes x 40 steps: 1 launch / 1 segment / 6 segments",
                     _td3d_loop(1, 60), "final_params", 60, 6, boundary_wait=True)
    if "td3d_entry_builds" in which:
        # the two old entries on this build against another build of the library (usage: td3d_entry_builds <path of the other .so>): the workload of
        # td3d_segments on the SE, and 48 chains x 30 episodes on the real CartPole for the RENV instantiation
        other = os.path.join(ROOT, which[which.index("td3d_entry_builds") + 1])            # (an absolute path stays what it is)
        run_td3d_entry_builds("lenv_td3d_inner_loop, CartPole SE + TD3_discrete 128x2 LayerNorm, 48 chains, 60 episodes: this build / the other build",
                              _td3d_loop(48, 60), other)
        run_td3d_entry_builds("lenv_td3d_rn_inner_loop, real CartPole + TD3_discrete 128x2 LayerNorm, 48 chains, 30 episodes: this build / the other build",
                              _td3d_loop(48, 30, real_env=True), other)
    if "td3d_episode_time" in which:
        # a full-length learning episode of the harness's chains, on the SE and on the real CartPole (10 init episodes as the comparability block sets)
        # and CartPole-v0's 200 steps per episode
        run_td3d_episode_time("CartPole SE (200 steps) + TD3_discrete 128x2 LayerNorm, 8 chains", _td3d_loop(8, 25, init_episodes=10, max_steps=200))
        run_td3d_episode_time("real CartPole (200 steps) + TD3_discrete 128x2 LayerNorm, 8 chains",
                              _td3d_loop(8, 25, real_env=True, init_episodes=10, max_steps=200))
    if "td3_episode_time" in which:
        # the TD3 *_transfer_vary_hp scripts' chains (a RewardEnv on the real env, full-length episodes): the nominal shape and the largest one
        # their hyper-parameter draw can give (hidden 384, 3 layers, batch 768)
        for make, label in ((configs.cmc_reward_env_td3, "MountainCarContinuous RN (999 steps, same_action_num 2)"),
                            (configs.halfcheetah_reward_env_td3, "HalfCheetah-standin RN (1000 steps)")):
            for shape in ((128, 2, 256), (384, 3, 768)):
                c = configs.fixed_work(make(16), 4)
                c["agents"]["td3"]["test_episodes"] = 1
                run_td3_episode_time(label + " + TD3 %dx%d B %d" % shape, c, shape)
    if "dueling_segments" in which:
        # the CartPole vary_hp transfer script's nominal DDQN chain (4-64-2 relu, batch 32, lr 2.5e-4, eps 1.0 -> 0.1 at 0.9 per episode, one init
        # episode, one test episode per training episode) on the published CartPole RewardEnv (type 2, reward net 4-64-1), 48 chains, 240 episodes of
        # up to 200 steps: the old entry, one segment, six segments
        run_segments("CartPole RN + DDQN 64x1 B 32, 48 chains, 240 episodes of up to 200 steps: 1 launch / 1 segment / 6 segments",
                     _dueling_loop(_cartpole_transfer_config("vary_hp", 240), 48, (64, 1, 32)), "final_online", 240, 6, boundary_wait=True)
        # the same with ONE chain (chain 0 of the 48): no chain waits for another at a boundary, what is left is the cost of splitting itself
        run_segments("CartPole RN + DDQN 64x1 B 32, 1 chain, 240 episodes of up to 200 steps: 1 launch / 1 segment / 6 segments",
                     _dueling_loop(_cartpole_transfer_config("vary_hp", 240), 1, (64, 1, 32)), "final_online", 240, 6, boundary_wait=True)
    if "dueling_episode_time" in which:
        # the CartPole transfer scripts' chains (a RewardEnv on the real env, episodes of up to 200 steps): the nominal shape and the largest one
        # the vary_hp script's draw can give (hidden 192, 2 layers, batch 96), for the plain-DQN agent (vary_hp script) and the dueling one (algo
        # script, feature_dim 128)
        for script, label in (("vary_hp", "DDQN"), ("algo", "DuelingDDQN f128")):
            for shape in ((64, 1, 32), (192, 2, 96)):
                run_dueling_episode_time("CartPole RN (200 steps) + %s %dx%d B %d" % ((label,) + shape), _cartpole_transfer_config(script, 300), shape)
    if "ppo_segments" in which:
        # the README's PPO shape (default_config_pendulum_reward_env.yaml, PPO 64 x 2 relu, a learn call of 10 epochs x 1 001 rows every five episodes)
        # on 48 chains, 60 episodes of 200 steps: the old entry, one segment, six segments of ten episodes
        c = configs.fixed_work(configs.pendulum_reward_env_ppo(16, train_episodes=60), 60)
        run_segments("Pendulum RN + PPO 64x2, 48 chains, 60 episodes x 200 steps: 1 launch / 1 segment / 6 segments",
                     _ppo_loop(c, 48, train_episodes=60), "final_params", 60, 6)
        # the same with ONE chain: no chain waits for another at a boundary, what is left is the cost of splitting itself
        run_segments("Pendulum RN + PPO 64x2, 1 chain, 60 episodes x 200 steps: 1 launch / 1 segment / 6 segments",
                     _ppo_loop(c, 1, train_episodes=60), "final_params", 60, 6)
    if "ppo_episode_time" in which:
        # the PPO *_transfer_algo scripts' chains: 10 models x 10 agents at the scripts' settings, full-length episodes.  MountainCarContinuous: a
        # learn call (1 999 rows x 80 epochs) about every tenth episode; the HalfCheetah stand-in: one (1 001 rows x 10 epochs) in every episode
        # from the second
        run_ppo_episode_time("MountainCarContinuous RN (999 steps, same_action_num 5) + PPO 64x2, 1 999 rows x 80 epochs", "MountainCarContinuous-v0", 23)
        run_ppo_episode_time("HalfCheetah-standin RN (1000 steps) + PPO 128x2 tanh, 1 001 rows x 10 epochs", "HalfCheetah-v3", 7)
    if "ppo_icm" in which:
        from learning_environments_amd.experiments import transfer_algo as ta
        # (a) the README's PPO row shape (64 x 2 relu, Pendulum RewardEnv, 10 episodes x 200 steps = one learn call of 1 001 rows x 10 epochs per chain)
        # at 48 and 192 chains, with the transfer scripts' module (feature_dim 32, hidden 128) against the ICM-less entry of the same build
        icm = dict(ta.ICM_SETTINGS["MountainCarContinuous-v0"])
        for pop in (16, 64):
            c = configs.fixed_work(configs.pendulum_reward_env_ppo(pop, train_episodes=10, ppo_epochs=10), 10)
            run_ppo_icm_cost("Pendulum RN + PPO 64x2, %d chains, 10 episodes x 200 steps, 1 learn call x 10 epochs x 1001 rows: ICM 32/128 against none"
                             % (3 * pop), c, 3 * pop, icm)
        # (b) the two scripts' mode -1 chains (10 x 10 ppo_icm agents on the real env) at full episode length, with and without a learn call
        run_ppo_episode_time("MountainCarContinuous (999 steps, same_action_num 5) + PPO 64x2 + ICM 32/128, 1 999 rows x 80 epochs",
                             "MountainCarContinuous-v0", 23, icm=dict(ta.ICM_SETTINGS["MountainCarContinuous-v0"]))
        run_ppo_episode_time("HalfCheetah-standin (1000 steps) + PPO 128x2 tanh + ICM 32/128, 1 001 rows x 10 epochs", "HalfCheetah-v3", 7,
                             icm=dict(ta.ICM_SETTINGS["HalfCheetah-v3"]))
    if "ppo_entry_builds" in which:
        # (c) the ICM-less single-launch entry on this build against another build of the library (usage: ppo_entry_builds <path of the other .so>):
        # the shape of ppo_segments
        c = configs.fixed_work(configs.pendulum_reward_env_ppo(16, train_episodes=60), 60)
        run_ppo_entry_builds("lenv_ppo_rn_inner_loop, Pendulum RN + PPO 64x2, 48 chains, 60 episodes x 200 steps: this build / the other build", c, 48,
                             which[which.index("ppo_entry_builds") + 1])
    if "rn_step" in which:
        # the one-step population API on a RewardEnv: 192 chains (64 workers) of the HalfCheetah stand-in, reward type 2, reward net 17-128-1, one
        # launch against one env-step launch + 192 shaping launches per repeat; a warm-up, then the medians of 7 alternating runs
        for repeat in (1, 2):
            run_rn_step("HalfCheetah-standin RN 17-128-1 type 2, 192 chains, one step, repeat %d: composed entries / one launch" % repeat, repeat=repeat)
    if "agent_test" in which:
        # BaseAgent.test as a call of its own: 400 fresh agents (the run_vary_hp population) x 10 test episodes, the new entry against the generic
        # kernel launched with train_episodes = 0; a warm-up, then the medians of 7 alternating runs
        run_agent_test("MountainCar-v0, DDQN 2-256-256-3, 400 agents x 10 test episodes of 200 steps: generic kernel (train_episodes 0) / agent_test_population",
                       configs.mountaincar_syn_env_ddqn(16))
        run_agent_test("Acrobot-v1, DuelingDDQN 6-128-128 f128, 400 agents x 10 test episodes of 500 steps: generic kernel (train_episodes 0) / agent_test_population",
                       configs.acrobot_syn_env_duelingddqn(16))
    if "actor_test" in which:
        # BaseAgent.test of TD3 / PPO agents as a call of its own: 400 fresh agents x 10 test episodes, the new entry against the fused entry
        # launched with train_episodes = 0; a warm-up, then the medians of 7 alternating runs
        run_actor_test("Pendulum-v0, PPO 64x2 relu, 400 agents x 10 test episodes of 200 steps: fused entry (train_episodes 0) / actor_test_population",
                       configs.pendulum_reward_env_ppo(16, test_episodes=10), "ppo")
        run_actor_test("HalfCheetah-standin, TD3 17-128-128-6 relu (default_config_halfcheetah.yaml), 400 agents x 10 test episodes of 1000 steps: "
                       "fused entry (train_episodes 0) / GEMM-queue kernel / actor_test_population", configs.halfcheetah_syn_env_td3(16), "td3")
    if "discrete_actor_test" in which:
        # BaseAgent.test of TD3_discrete_vary agents as a call of its own: 400 fresh agents x 10 test episodes at the histogram scripts' shape
        # (td3_discrete_vary_layer_norm_2: 4-128-128-2 tanh with LayerNorm, soft head, temperature 1), the new entry against lenv_td3d_inner_loop
        # launched with train_episodes = 0; a warm-up, then the medians of 7 alternating runs
        run_discrete_actor_test("CartPole-v0, TD3_discrete_vary 4-128-128-2 tanh LayerNorm, 400 agents x 10 test episodes of up to 200 steps: "
                                "fused entry (train_episodes 0) / td3d_test_population",
                                configs.cartpole_syn_env_td3_discrete(16, hidden_size=128, hidden_layer=2, batch_size=128, use_layer_norm=True, gumbel_softmax_temp=1.0,
                                                                      gumbel_softmax_hard=False, action_std=0.1, policy_delay=2, init_episodes=10))
    if "ql_test" in which:
        run_ql_test("Cliff, 400 Q-tables x 10 test episodes of up to 50 steps: lenv_ql_rn_inner_loop (train_episodes 0) / ql_test_population")
    if "se_fit" in which:
        # the supervised (MBRL baseline) fit: 5 models x 9 500 Adam steps at the CartPole SE shape in one launch against an eager torch loop over
        # the models, then 256 models (kernel alone: the eager loop would take 51 x its 5-model time)
        kw = dict(steps=9500, runs=7)
        run_se_fit("CartPole-v0 SE 6-128-{4,1,1}, 5 models x %d Adam steps, batch 64: se_fit_population / eager torch" % kw["steps"], models=5, **kw)
        run_se_fit("CartPole-v0 SE 6-128-{4,1,1}, 256 models x %d Adam steps, batch 64: se_fit_population" % kw["steps"], models=256, torch_models=0, **kw)
    if "5" in which:
        c = configs.fixed_work(configs.halfcheetah_reward_env_td3(32), 3)
        c["agents"]["td3"]["init_episodes"] = 1
        c["envs"]["HalfCheetah-v3"]["max_steps"] = 100
        run("cfg5 HalfCheetah-standin RN + TD3 pop 32 (3 episodes x 100 steps)", c, gens=1, extra=td3_model)
