"""The "Supervised Learning / MBRL Baseline" of the reference's README: VirtualEnvs with the SE's architecture, fitted by regression on real
transitions and then run through run_vary_hp next to the learned SEs.

The reference ships the evaluation half only (experiments/syn_env_evaluate_cartpole_mbrl_baseline.py: load_envs_and_config and
train_test_agents, identical to the harness's; its fit_mbrl_baseline() is a bare `raise NotImplementedError`).  Here is the whole path:

    rows = collect_transitions(real_env, n_transitions)            uniformly random actions on the real env, a population of instances
    models, loss = fit_mbrl_baseline(config, rows)                 fresh VirtualEnvs, all fitted in ONE launch (csrc/se_fit.hip)
    save_models(models, config, model_dir)                         reference-format checkpoints that get_all_files / run_vary_hp pick up
    run_vary_hp(mode, ..., model_dir, load_envs_and_config, train_test_agents, env_name)

The reference's fit hyper-parameters are not in its tree (its loss plot shows about 9 500 Adam iterations): `steps`, `batch_size` and `lr`
are arguments, and their defaults -- 9 500 steps, batches of 64, torch's Adam default 1e-3 -- are this package's own."""
import copy
import os

import numpy as np
import torch

from .. import _lib, engine
from ..agents.nes_common import linear_init_bounds
from ..agents.rollout import ReplayRows
from ..envs.env_factory import EnvFactory
from .syn_env_evaluate import load_envs_and_config, train_test_agents      # noqa: F401  (the reference's script defines them identically)

STREAM_AGENT_INIT = 10        # csrc/lenv_device.cuh: the stream fresh nn.Linear parameters are drawn from


def collect_transitions(real_env, n_transitions, chains=64, seed=0):
    """Exactly `n_transitions` transitions of uniformly random actions on the real env, as ReplayRows: `chains` instances step side by
    side (EnvWrapper.reset_population / step_population), an instance that reports done starts its next episode (episode index + 1 of its
    own reset stream); rows are in step order, chain after chain inside a step."""
    dev = engine.require_device()
    gen = torch.Generator().manual_seed(int(seed))
    discrete = real_env.has_discrete_action_space()
    A = real_env.get_action_dim()
    st = real_env.reset_population(chains, seed=seed, episode=0)
    episode = torch.zeros(chains, dtype=torch.int64)
    parts, have = [], 0
    if not discrete:
        lo, hi = (torch.as_tensor(np.asarray(b, dtype=np.float32)) for b in (real_env.env.action_space.low, real_env.env.action_space.high))
    while have < n_transitions:
        if discrete:
            act = torch.randint(0, A, (chains,), generator=gen, dtype=torch.int32)
        else:
            act = lo + (hi - lo) * torch.rand((chains, A), generator=gen, dtype=torch.float32)
        obs = st.obs.clone()
        obs2, reward, done = real_env.step_population(act.to(dev), st)
        parts.append((obs.cpu(), act.to(torch.float32).reshape(chains, -1), obs2.cpu(), reward.cpu().reshape(chains, 1), done.cpu().reshape(chains, 1)))
        have += chains
        over = parts[-1][4][:, 0] > 0.5
        if bool(over.any()):
            episode[over] += 1
            for e in torch.unique(episode[over]).tolist():
                fresh = real_env.reset_population(chains, seed=seed, episode=int(e))
                pick = (over & (episode == e)).to(dev)
                st.state[pick], st.elapsed[pick], st.obs[pick] = fresh.state[pick], fresh.elapsed[pick], fresh.obs[pick]
    fields = [torch.cat([p[k] for p in parts])[:n_transitions] for k in range(5)]
    return ReplayRows(fields[0].shape[1], *fields, action_dim=1 if discrete else A)


def rows_to_dataset(virtual_env, rows):
    """(x [N,A+S], y_state [N,S], y_reward [N], y_done [N]) as device tensors from any ReplayRows of the real env (collect_transitions',
    rollout.test_agents', ...): x = cat(one_hot(action) | action vector, state), the row EnvWrapper.step followed by VirtualEnv.step hand the
    three nets (env_wrapper.py:20-21, virtual_env.py:49)."""
    dev = engine.require_device()
    if virtual_env.has_discrete_state_space():
        raise NotImplementedError("rows_to_dataset: a gridworld's state indices (the tabular agents' VirtualEnv) are not regression targets here")
    s, a, s2, r, d = rows.get_all()
    A = virtual_env.get_action_dim()
    if virtual_env.has_discrete_action_space():
        if a.shape[1] != 1:
            raise ValueError("rows_to_dataset: a discrete action space takes the action index column")
        a = torch.nn.functional.one_hot(a[:, 0].long(), A).to(torch.float32)
    elif a.shape[1] != A:
        raise ValueError("rows_to_dataset: action vectors of width %d for an action space of %d" % (a.shape[1], A))
    x = torch.cat([a, s], dim=1)
    return tuple(t.to(dev, torch.float32).contiguous() for t in (x, s2, r[:, 0], d[:, 0]))


def _se_bounds(descs):
    """nn.Linear default-init bounds of theta = state | reward | done net"""
    return np.concatenate([linear_init_bounds([(d.in_dim, d.hidden)] + [(d.hidden, d.hidden)] * (d.layers - 1) + [(d.hidden, d.out_dim)]) for d in descs])


def fit_mbrl_baseline(config, rows, models=5, steps=9500, batch_size=64, lr=1e-3, seed=0, steps_per_launch=None):
    """`models` fresh EnvFactory.generate_virtual_env() fitted on `rows` (ReplayRows of the real env) by `steps` Adam steps on the three
    nets' mean squared errors: (list of VirtualEnv wrappers, loss [models,steps,3] on the host).  Model m starts from nn.Linear's default
    init drawn by lenv_chain_uniform_init with the key lenv_chain_key(seed, 0, m, 0) and draws its minibatches from the same key, so a model does
    not depend on how many are fitted next to it.  steps / batch_size / lr: this package's defaults (see the module's head)."""
    dev = engine.require_device()
    factory = EnvFactory(config=config)
    envs = [factory.generate_virtual_env() for _ in range(models)]
    if not envs:
        return [], torch.zeros((0, steps, 3))
    descs = envs[0].env.descs()
    P = engine.se_fit_num_params(descs)
    x, y_state, y_reward, y_done = rows_to_dataset(envs[0], rows)
    L = _lib.lib()
    keys = torch.from_numpy(np.array([L.lenv_chain_key(int(seed), 0, m, 0) for m in range(models)], np.uint64).view(np.int64)).to(dev)
    bounds = torch.from_numpy(_se_bounds(descs)).to(dev)
    assert bounds.numel() == P
    theta = torch.empty((models, P), dtype=torch.float32, device=dev)
    _lib.check(L.lenv_chain_uniform_init(engine._ptr(keys), models, STREAM_AGENT_INIT, P, engine._ptr(bounds), engine._ptr(theta), engine._stream()),
               "lenv_chain_uniform_init")
    out = engine.se_fit_population(descs, theta, x, y_state, y_reward, y_done, batch_size, steps, lr=lr, rng_keys=keys, steps_per_launch=steps_per_launch)
    with torch.no_grad():
        for m, env in enumerate(envs):
            env.env.flat_params().copy_(out["theta"][m])
    return envs, out["loss"].cpu()


def save_models(models, config, model_dir, vary_hp=True):
    """Reference-format checkpoints {'model': state_dict, 'config': config} (agents/GTN_master.py:133-139), one per model, under names that
    hold env_name and end in a unique 9-character tail -- what get_all_files filters and sorts by -- with config['agents']['ddqn_vary']['vary_hp']
    set: run_vary_hp(mode=2 | 1, model_dir=...) takes the models saved with vary_hp on | off.  Returns the file names."""
    cfg = copy.deepcopy(config)
    cfg["agents"].setdefault("ddqn_vary", {})["vary_hp"] = bool(vary_hp)
    os.makedirs(model_dir, exist_ok=True)
    names = []
    for m, env in enumerate(models):
        name = "%s_mbrl_%s%05d.pt" % (cfg["env_name"], "V" if vary_hp else "F", m)
        torch.save({"model": {k: v.detach().cpu().clone() for k, v in env.state_dict().items()}, "config": cfg}, os.path.join(model_dir, name))
        names.append(name)
    return names
