"""Tensor-level host wrappers over the C-ABI (torch is plumbing: device memory + streams).

Every function takes/returns torch CUDA(HIP) tensors and enqueues on torch's current stream.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import DdqnCfg, InnerOut, MlpDesc, PpoCfg, PpoOut, PpoTapes, QlOut, Tapes, Td3Cfg, Td3dCfg, Td3dTapes, Td3Out, Td3Tapes


def require_device():
    if not torch.cuda.is_available():
        raise _lib.LenvError("learning_environments_amd needs a HIP device (MI355X); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, dtype, name):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError("%s must be a contiguous CUDA tensor of dtype %s" % (name, dtype))
    return t


def mlp_desc(in_dim, hidden, layers, out_dim, act, prelu=0.25, use_layer_norm=False):
    return MlpDesc(int(in_dim), int(hidden), int(layers), int(out_dim), _lib.ACT[act] if isinstance(act, str) else int(act),
                   float(prelu), 1 if use_layer_norm else 0)


def mlp_num_params(d):
    return int(_lib.lib().lenv_mlp_num_params(C.byref(d)))


def mlp_forward(d, params, x):
    """y [rows,out] = MLP(x [rows,in]) with the flat parameter vector `params` (device tensors)."""
    dev = require_device()
    _chk(params, torch.float32, "params"); _chk(x, torch.float32, "x")
    rows = x.shape[0]
    y = torch.empty((rows, d.out_dim), dtype=torch.float32, device=dev)
    rc = _lib.lib().lenv_mlp_forward(C.byref(d), _ptr(params), _ptr(x), rows, _ptr(y), _stream())
    _lib.check(rc, "lenv_mlp_forward")
    return y


def rn_num_params(rtype, state_dim, info_dim, hidden, layers):
    """Parameter count of RewardEnv.build_reward_net for a reward type (reference envs/reward_env.py:29-59)."""
    n = _lib.lib().lenv_rn_num_params(int(rtype), int(state_dim), int(info_dim), int(hidden), int(layers))
    _lib.check(int(n) if n < 0 else 0, "lenv_rn_num_params")
    return int(n)


def rn_shape_rows(rtype, rn_desc, state_dim, info_dim, gamma, theta, s, s2, info, r):
    """RewardEnv._calc_reward (reference envs/reward_env.py:68-133) for rows of a vector-state real env; device tensors.
    `info` may be None for the types that do not read it; for the others a missing info raises ValueError like the
    reference."""
    dev = require_device()
    for t, n in ((s, "s"), (s2, "s2"), (r, "r")):
        _chk(t, torch.float32, n)
    rows = s.shape[0]
    out = torch.empty(rows, dtype=torch.float32, device=dev)
    rc = _lib.lib().lenv_rn_shape_rows(int(rtype), C.byref(rn_desc) if rn_desc is not None else None, int(state_dim), int(info_dim),
                                       float(gamma), _ptr(theta) if theta is not None else None, _ptr(s), _ptr(s2),
                                       _ptr(info) if info is not None else None, _ptr(r), rows, _ptr(out), _stream())
    _lib.check(rc, "lenv_rn_shape_rows")
    return out


def se_descs(S, A, hidden, layers, act, prelu=0.25):
    return (mlp_desc(S + A, hidden, layers, S, act, prelu), mlp_desc(S + A, hidden, layers, 1, act, prelu),
            mlp_desc(S + A, hidden, layers, 1, act, prelu))


def se_step_population(descs, theta, eps, worker, sign, state, action):
    """state [chains,S] or [chains,n,S]; action int32 [chains] or [chains,n].  Returns (next_state, reward, done)."""
    dev = require_device()
    sn, rn, dn = descs
    squeeze = state.dim() == 2
    if squeeze:
        state, action = state.unsqueeze(1), action.unsqueeze(1)
    chains, n, S = state.shape
    _chk(theta, torch.float32, "theta"); _chk(state, torch.float32, "state"); _chk(action, torch.int32, "action")
    _chk(eps, torch.float32, "eps"); _chk(worker, torch.int32, "worker"); _chk(sign, torch.float32, "sign")
    ns = torch.empty((chains, n, S), dtype=torch.float32, device=dev)
    r = torch.empty((chains, n), dtype=torch.float32, device=dev)
    d = torch.empty((chains, n), dtype=torch.float32, device=dev)
    rc = _lib.lib().lenv_se_step_population(C.byref(sn), C.byref(rn), C.byref(dn), _ptr(theta), _ptr(eps), _ptr(worker),
                                            _ptr(sign), chains, n, _ptr(state), _ptr(action), _ptr(ns), _ptr(r), _ptr(d),
                                            _stream())
    _lib.check(rc, "lenv_se_step_population")
    if squeeze:
        return ns[:, 0], r[:, 0], d[:, 0]
    return ns, r, d


def se_step_vec_path(descs, n_per_chain=1):
    """Which kernel lenv_se_step_population_vec runs for these nets (host only): 0 = weights resident in LDS, 1 = streamed through it."""
    sn, rn, dn = descs
    path = int(_lib.lib().lenv_se_step_vec_path(C.byref(sn), C.byref(rn), C.byref(dn), int(n_per_chain)))
    _lib.check(path if path < 0 else 0, "lenv_se_step_vec_path")
    return path


def se_step_population_vec(descs, theta, eps, worker, sign, state, action, repeat=1):
    """se_step_population for action VECTORS: state [chains,S] or [chains,n,S]; action fp32 [chains,A] or [chains,n,A], the row the nets
    see (a continuous action, or a one-hot).  `repeat` = same_action_num of EnvWrapper.step's virtual branch: that many SE steps on the
    same action, each fed the previous next state, rewards summed in fp32; next_state / done of the last.  Returns (next_state, reward,
    done) shaped like se_step_population's."""
    dev = require_device()
    sn, rn, dn = descs
    squeeze = state.dim() == 2
    if squeeze:
        state, action = state.unsqueeze(1), action.unsqueeze(1)
    chains, n, S = state.shape
    if tuple(action.shape) != (chains, n, sn.in_dim - S):
        raise ValueError("action must be [chains,n,%d] next to state [chains,n,%d]" % (sn.in_dim - S, S))
    _chk(theta, torch.float32, "theta"); _chk(state, torch.float32, "state"); _chk(action, torch.float32, "action")
    _chk(eps, torch.float32, "eps"); _chk(worker, torch.int32, "worker"); _chk(sign, torch.float32, "sign")
    ns = torch.empty((chains, n, S), dtype=torch.float32, device=dev)
    r = torch.empty((chains, n), dtype=torch.float32, device=dev)
    d = torch.empty((chains, n), dtype=torch.float32, device=dev)
    rc = _lib.lib().lenv_se_step_population_vec(C.byref(sn), C.byref(rn), C.byref(dn), _ptr(theta), _ptr(eps), _ptr(worker),
                                                _ptr(sign), chains, n, int(repeat), _ptr(state), _ptr(action), _ptr(ns), _ptr(r),
                                                _ptr(d), _stream())
    _lib.check(rc, "lenv_se_step_population_vec")
    if squeeze:
        return ns[:, 0], r[:, 0], d[:, 0]
    return ns, r, d


def se_fit_num_params(descs):
    """P of lenv_se_fit_population: the SE theta layout state | reward | done (host only)."""
    sn, rn, dn = descs
    n = int(_lib.lib().lenv_se_fit_num_params(C.byref(sn), C.byref(rn), C.byref(dn)))
    _lib.check(n if n < 0 else 0, "lenv_se_fit_num_params")
    return n


def se_fit_population(descs, theta, x, y_state, y_reward, y_done, batch_size, steps, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, rng_keys=None,
                      batch_idx=None, step_begin=0, adam_m=None, adam_v=None, steps_per_launch=None):
    """Supervised fit of a population of VirtualEnvs (lenv_se_fit_population): model m takes the Adam steps step_begin .. step_begin+steps-1 on
    F.mse_loss of its three nets over minibatches of `batch_size` rows of (x [N,in], y_state [N,S], y_reward [N], y_done [N]).  theta
    [models,P] are the start parameters (not modified); moments that are not given start at zero.  The rows of a step come from rng_keys
    (int64 / uint64 [models], counter mode) or from batch_idx (int32 [models,steps,batch_size], tape mode): exactly one of the two.
    steps_per_launch splits a long fit into consecutive launches that hand the moments on (the same bits).  Returns dict(theta, adam_m, adam_v,
    loss [models,steps,3] = the three losses before each step)."""
    dev = require_device()
    sn, rn, dn = descs
    P = se_fit_num_params(descs)
    if theta.dim() != 2 or theta.shape[1] != P:
        raise ValueError("theta must be [models,%d]" % P)
    models, steps, batch_size, step_begin = theta.shape[0], int(steps), int(batch_size), int(step_begin)
    N = x.shape[0]
    for t, n, shape in ((theta, "theta", (models, P)), (x, "x", (N, sn.in_dim)), (y_state, "y_state", (N, sn.out_dim)), (y_reward, "y_reward", (N,)),
                        (y_done, "y_done", (N,)), (adam_m, "adam_m", (models, P)), (adam_v, "adam_v", (models, P))):
        if t is not None and tuple(_chk(t, torch.float32, n).shape) != shape:
            raise ValueError("%s must be %s" % (n, list(shape)))
    if (rng_keys is None) == (batch_idx is None):
        raise ValueError("exactly one of rng_keys / batch_idx")
    if rng_keys is not None:
        if not rng_keys.is_cuda or rng_keys.dtype not in (torch.int64, torch.uint64) or not rng_keys.is_contiguous() or rng_keys.numel() != models:
            raise ValueError("rng_keys must be a contiguous 64-bit integer CUDA tensor [models]")
    else:
        if tuple(_chk(batch_idx, torch.int32, "batch_idx").shape) != (models, steps, batch_size):
            raise ValueError("batch_idx must be [models,steps,batch_size]")
        if batch_idx.numel() and N > 0 and (int(batch_idx.min()) < 0 or int(batch_idx.max()) >= N):
            raise ValueError("batch_idx holds a row outside the data set")
    L = _lib.lib()
    ws_bytes = int(L.lenv_se_fit_workspace_bytes(C.byref(sn), C.byref(rn), C.byref(dn), batch_size, models))
    _lib.check(ws_bytes if ws_bytes < 0 else 0, "lenv_se_fit_workspace_bytes")
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev) if ws_bytes else None
    out = dict(theta=theta.clone(), adam_m=torch.zeros_like(theta) if adam_m is None else adam_m.clone(),
               adam_v=torch.zeros_like(theta) if adam_v is None else adam_v.clone())
    if steps < 0 or (steps_per_launch is not None and int(steps_per_launch) < 1):
        raise ValueError("steps must not be negative and steps_per_launch must be positive")
    per = max(steps, 1) if steps_per_launch is None else int(steps_per_launch)      # steps == 0: one call that returns without a launch
    losses = []
    for s0 in range(0, max(steps, 1), per):
        n = min(per, steps - s0)
        loss = torch.zeros((models, n, 3), dtype=torch.float32, device=dev)
        idx = batch_idx[:, s0:s0 + n].contiguous() if batch_idx is not None else None
        rc = L.lenv_se_fit_population(C.byref(sn), C.byref(rn), C.byref(dn), _ptr(x), _ptr(y_state), _ptr(y_reward), _ptr(y_done), N, batch_size,
                                      step_begin + s0, step_begin + s0 + n, float(lr), float(betas[0]), float(betas[1]), float(eps),
                                      _ptr(rng_keys), _ptr(idx), models, _ptr(out["theta"]), _ptr(out["adam_m"]), _ptr(out["adam_v"]), _ptr(loss),
                                      _ptr(ws), ws_bytes, _stream())
        _lib.check(rc, "lenv_se_fit_population")
        losses.append(loss)
    out["loss"] = losses[0] if len(losses) == 1 else torch.cat(losses, dim=1)
    return out


# observation words, fp64 state words and action width of the vector-state real envs (csrc/lenv_device.cuh); action width 0 = a discrete index
REAL_ENV_DIMS = {_lib.ENV[k]: v for k, v in {"CartPole-v0": (4, 4, 0), "Acrobot-v1": (6, 4, 0), "MountainCar-v0": (2, 4, 0), "HalfCheetah-v3": (17, 17, 6),
                                                "Pendulum-v0": (3, 2, 1), "MountainCarContinuous-v0": (2, 2, 1)}.items()}


def rn_step_population(env_id, max_steps, rtype, rn_desc, info_dim, gamma, theta, eps, worker, sign, action, state, elapsed, repeat=1):
    """One RewardEnv step of every chain in one launch: chain c steps its own instance of the real env `env_id` (state fp64 [chains,SD],
    elapsed int32 [chains], both updated in place) on its action -- int32 [chains] for the discrete envs, fp32 [chains,A] for the continuous
    ones -- up to `repeat` times (same_action_num of EnvWrapper._step_real: shaped rewards summed, stop after the step that reports done) and
    shapes the rewards with theta + sign[c]*eps[worker[c]] (eps None: the plain theta; `theta` None for reward type 0).  Returns
    (obs [chains,S], reward [chains], done [chains]); device tensors."""
    dev = require_device()
    if int(env_id) not in REAL_ENV_DIMS:
        raise NotImplementedError("lenv_rn_step_population: no vector-state real env with id %d" % int(env_id))
    S, SD, A = REAL_ENV_DIMS[int(env_id)]
    _chk(state, torch.float64, "state"); _chk(elapsed, torch.int32, "elapsed")
    if state.dim() != 2 or state.shape[1] != SD:
        raise ValueError("state must be [chains,%d]" % SD)
    chains = state.shape[0]
    if tuple(elapsed.shape) != (chains,):
        raise ValueError("elapsed must be [chains]")
    if A == 0:
        _chk(action, torch.int32, "action")
        if tuple(action.shape) != (chains,):
            raise ValueError("action must be int32 [chains] next to state [chains,%d]" % SD)
    else:
        _chk(action, torch.float32, "action")
        if tuple(action.shape) != (chains, A):
            raise ValueError("action must be [chains,%d] next to state [chains,%d]" % (A, SD))
    _chk(theta, torch.float32, "theta"); _chk(eps, torch.float32, "eps"); _chk(worker, torch.int32, "worker"); _chk(sign, torch.float32, "sign")
    if eps is not None:
        if theta is None or eps.dim() != 2 or eps.shape[1] != theta.numel():
            raise ValueError("eps must be [pop,%d], a row per worker next to theta" % (0 if theta is None else theta.numel()))
        if worker is None or sign is None or tuple(worker.shape) != (chains,) or tuple(sign.shape) != (chains,):
            raise ValueError("worker and sign must be [chains] next to eps")
    obs = torch.empty((chains, S), dtype=torch.float32, device=dev)
    r = torch.empty(chains, dtype=torch.float32, device=dev)
    d = torch.empty(chains, dtype=torch.float32, device=dev)
    rc = _lib.lib().lenv_rn_step_population(int(env_id), int(max_steps), int(rtype), C.byref(rn_desc) if rn_desc is not None else None, S,
                                            int(info_dim), float(gamma), _ptr(theta), _ptr(eps), _ptr(worker), _ptr(sign), chains, int(repeat),
                                            _ptr(action), _ptr(state), _ptr(elapsed), _ptr(obs), _ptr(r), _ptr(d), _stream())
    _lib.check(rc, "lenv_rn_step_population")
    return obs, r, d


def agent_test_num_params(cfg):
    """Row width of `params` in agent_test_population: the agent's flat parameter vector at cfg's shapes (the final_online rows of the fused
    loops; the shared LayerNorm's weight | bias included).  Computed from the network fields alone, so cfg's training fields may be anything."""
    S, A, H, L = cfg.state_dim, cfg.num_actions, cfg.q_hidden, cfg.q_layers
    dims = [(S, H)] + [(H, H)] * (L - 1)
    if cfg.agent_kind == 1:
        F = cfg.feature_dim
        dims += [(H, F), (F, F), (F, 1), (F, F), (F, A)]
    else:
        dims += [(H, A)]
    return sum(fi * fo + fo for fi, fo in dims) + (2 * H if cfg.q_layer_norm and L >= 2 else 0)


def _mlp_num_params(n_in, hidden, layers, n_out, ln):
    """Parameters of an MLP n_in - `layers` x hidden - n_out with the shared LayerNorm (weight | bias) from two hidden layers on."""
    return (n_in * hidden + hidden) + (layers - 1) * (hidden * hidden + hidden) + (2 * hidden if ln and layers >= 2 else 0) + (n_out * hidden + n_out)


def _tp_inputs(cap_entry, cap_args, params, P, rng_keys, T, vectors, reset_states, SD, tapes=None, A=0):
    """The input checks the *_test_population wrappers share: params fp32 [agents,P], rng_keys int64 [agents], `vectors` (name -> optional int64
    [agents]), reset_states optional fp64 [agents,T,SD] (SD or a callable that gives it), `tapes` (name -> optional fp32 [agents,T,cap,A]).  Returns (agents, cap)."""
    _chk(params, torch.float32, "params"); _chk(rng_keys, torch.int64, "rng_keys")
    for name, v in (tapes or {}).items():
        _chk(v, torch.float32, name)
    for name, v in vectors.items():
        _chk(v, torch.int64, name)
    _chk(reset_states, torch.float64, "reset_states")
    cap = _count(cap_entry, *cap_args)
    if callable(SD):                     # the env's state words, looked up only once the entry has admitted cfg's env
        SD = SD()
    if params.dim() != 2 or params.shape[1] != P:
        raise ValueError("params must be [agents,%d]" % P)
    n = params.shape[0]
    if tuple(rng_keys.shape) != (n,):
        raise ValueError("rng_keys must be [agents]")
    for name, v in vectors.items():
        if v is not None and tuple(v.shape) != (n,):
            raise ValueError("%s must be [agents]" % name)
    if reset_states is not None and tuple(reset_states.shape) != (n, T, SD):
        raise ValueError("reset_states must be [agents,%d,%d]" % (T, SD))
    for name, v in (tapes or {}).items():
        if v is not None and tuple(v.shape) != (n, T, cap, A):
            raise ValueError("%s must be [agents,%d,%d,%d]" % (name, T, cap, A))
    return n, cap


def _tp_outputs(dev, n, T, cap, want_rows, state_shape, state_dtype, action_shape, action_dtype):
    """returns / env_steps / agent_steps [agents,T] and, with want_rows, the five row tensors [agents,T,cap(,...)] (states and actions of the
    given trailing shape and dtype), zero-filled: (the dict the wrappers return, the eight output pointers in ABI order)."""
    z = lambda dt, *shape: torch.zeros((n, T) + shape, dtype=dt, device=dev)
    out = dict(returns=z(torch.float64), env_steps=z(torch.int32), agent_steps=z(torch.int32))
    if want_rows:
        out.update(row_state=z(state_dtype, cap, *state_shape), row_action=z(action_dtype, cap, *action_shape),
                   row_next_state=z(state_dtype, cap, *state_shape), row_reward=z(torch.float32, cap), row_done=z(torch.float32, cap))
    names = ("returns", "env_steps", "agent_steps", "row_state", "row_action", "row_next_state", "row_reward", "row_done")
    return out, [_ptr(out.get(k)) for k in names]


def agent_test_population(cfg, params, rng_keys, episode_offset=None, reset_states=None, want_rows=True):
    """BaseAgent.test of a population of trained DDQN / DuelingDDQN agents in one launch (lenv_agent_test_population): agent i, parameters
    params[i] (fp32 [agents,P] in the layout of the fused loops' final_online), runs T = cfg.test_episodes greedy episodes on the real env.
    Episode e resets from the counter draw (rng_keys[i], test-reset stream, episode_offset[i] + e) -- episode_offset int64 [agents], None = 0
    -- or from reset_states[i][e] (fp64 [agents,T,4]).  Returns a dict of device tensors: returns fp64 [agents,T], env_steps / agent_steps
    int32 [agents,T] and, with want_rows, the transitions row_state / row_next_state fp32 [agents,T,cap,S], row_action int32 /
    row_reward / row_done fp32 [agents,T,cap]; slots at or beyond agent_steps[i][e] are zero (the kernel does not write them)."""
    dev = require_device()
    L = _lib.lib()
    T, S = cfg.test_episodes, cfg.state_dim
    n, cap = _tp_inputs("lenv_agent_test_rows_cap", (C.byref(cfg),), params, agent_test_num_params(cfg), rng_keys, T, dict(episode_offset=episode_offset),
                        reset_states, 4)
    out, ptrs = _tp_outputs(dev, n, T, cap, want_rows, (S,), torch.float32, (), torch.int32)
    rc = L.lenv_agent_test_population(C.byref(cfg), _ptr(params), _ptr(rng_keys), _ptr(episode_offset), _ptr(reset_states), n, *ptrs, _stream())
    _lib.check(rc, "lenv_agent_test_population")
    return out


def _actor_kind(kind):
    k = {"td3": _lib.ACTOR_TD3, "ppo": _lib.ACTOR_PPO}.get(kind.lower(), None) if isinstance(kind, str) else int(kind)
    if k not in (_lib.ACTOR_TD3, _lib.ACTOR_PPO):
        raise NotImplementedError("actor_test_population: kind %r (TD3 and PPO actors only)" % (kind,))
    return k


def actor_test_num_params(kind, cfg):
    """Row width of `params` in actor_test_population: the flat parameter vector of the fused loops' final_params at cfg's shapes -- TD3:
    actor | critic_1 | critic_2 with each net's shared LayerNorm (lenv_td3_num_params), PPO: action_std | actor.net | critic.net
    (lenv_ppo_num_params).  Computed from the network fields alone, so cfg's training fields may be anything."""
    k = _actor_kind(kind)
    S, A, H, L = cfg.state_dim, cfg.action_dim, cfg.hidden, cfg.layers
    if k == _lib.ACTOR_TD3:
        ln = bool(cfg.use_layer_norm)
        return _mlp_num_params(S, H, L, A, ln) + 2 * _mlp_num_params(S + A, H, L, 1, ln)
    return A + _mlp_num_params(S, H, L, A, False) + _mlp_num_params(S, H, L, 1, False)


def actor_test_population(kind, cfg, params, rng_keys, episode_offset=None, reset_states=None, noise=None, want_rows=True):
    """BaseAgent.test of a population of trained TD3 / PPO agents in one launch (lenv_actor_test_population): kind "td3" (cfg a Td3Cfg) or
    "ppo" (a PpoCfg), or _lib.ACTOR_*.  Agent i, parameters params[i] (fp32 [agents,P] in the layout of the fused loops' final_params,
    P = actor_test_num_params(kind, cfg)), runs T = cfg.test_episodes episodes with the test noise of the fused loops' closing test on the
    real env.  Episode e resets from the counter draw (rng_keys[i], test-reset stream, episode_offset[i] + e) -- episode_offset int64
    [agents], None = 0 -- or from reset_states[i][e] (fp64 [agents,T,SD], the env's own state words); noise (fp32 [agents,T,cap,A]) replaces
    the standard-normal draws of the keys' noise streams.  Returns a dict of device tensors: returns fp64 [agents,T], env_steps /
    agent_steps int32 [agents,T] and, with want_rows, the transitions row_state / row_next_state fp32 [agents,T,cap,S], row_action fp32
    [agents,T,cap,A], row_reward / row_done fp32 [agents,T,cap]; slots at or beyond agent_steps[i][e] are zero (the kernel does not write
    them)."""
    dev = require_device()
    L = _lib.lib()
    k = _actor_kind(kind)
    if not isinstance(cfg, Td3Cfg if k == _lib.ACTOR_TD3 else PpoCfg):
        raise TypeError("actor_test_population: kind %r takes a %s" % (kind, "Td3Cfg" if k == _lib.ACTOR_TD3 else "PpoCfg"))
    T, S, A = cfg.test_episodes, cfg.state_dim, cfg.action_dim
    n, cap = _tp_inputs("lenv_actor_test_rows_cap", (k, C.byref(cfg)), params, actor_test_num_params(k, cfg), rng_keys, T,
                        dict(episode_offset=episode_offset), reset_states, lambda: REAL_ENV_DIMS[int(cfg.env_id)][1], dict(noise=noise), A)
    out, ptrs = _tp_outputs(dev, n, T, cap, want_rows, (S,), torch.float32, (A,), torch.float32)
    rc = L.lenv_actor_test_population(k, C.byref(cfg), _ptr(params), _ptr(rng_keys), _ptr(episode_offset), _ptr(reset_states), _ptr(noise), n, *ptrs,
                                      _stream())
    _lib.check(rc, "lenv_actor_test_population")
    return out


def td3d_test_num_params(cfg):
    """Row width of `params` in td3d_test_population: actor | critic_1 | critic_2 with each net's shared LayerNorm (lenv_td3d_num_params).
    Computed from the network fields alone, so cfg's training fields may be anything."""
    S, A, H, L, ln = cfg.state_dim, cfg.action_dim, cfg.hidden, cfg.layers, bool(cfg.use_layer_norm)
    return _mlp_num_params(S, H, L, A, ln) + 2 * _mlp_num_params(S + A, H, L, 1, ln)


def td3d_test_population(cfg, params, rng_keys, episode_offset=None, learn_calls=None, reset_states=None, gumbel=None, noise=None, want_rows=True):
    """BaseAgent.test of a population of trained TD3_discrete_vary agents in one launch (lenv_td3d_test_population): agent i, parameters
    params[i] (fp32 [agents,P] in the layout of the fused loops' final_params, P = td3d_test_num_params(cfg)), runs T = cfg.test_episodes
    episodes on the real env with the Gumbel-softmax head and the test noise of the fused loops' closing test, at the temperature the
    fused loop holds after learn_calls[i] learn calls (int64 [agents], None = 0: column 2 of a fused launch's stats).  Episode e resets from
    the counter draw (rng_keys[i], test-reset stream, episode_offset[i] + e) -- episode_offset int64 [agents], None = 0 -- or from
    reset_states[i][e] (fp64 [agents,T,4]); gumbel / noise (fp32 [agents,T,cap,A], each on its own) replace the draws of the keys' Gumbel /
    noise streams.  Returns a dict of device tensors: returns fp64 [agents,T], env_steps / agent_steps int32 [agents,T] and, with
    want_rows, the transitions row_state / row_next_state fp32 [agents,T,cap,S], row_action fp32 [agents,T,cap,A] (the action VECTORS; the
    env got their argmax), row_reward / row_done fp32 [agents,T,cap]; slots at or beyond agent_steps[i][e] are zero (the kernel does not
    write them)."""
    dev = require_device()
    L = _lib.lib()
    if not isinstance(cfg, Td3dCfg):
        raise TypeError("td3d_test_population takes a Td3dCfg")
    T, S, A = cfg.test_episodes, cfg.state_dim, cfg.action_dim
    n, cap = _tp_inputs("lenv_td3d_test_rows_cap", (C.byref(cfg),), params, td3d_test_num_params(cfg), rng_keys, T,
                        dict(episode_offset=episode_offset, learn_calls=learn_calls), reset_states, 4, dict(gumbel=gumbel, noise=noise), A)
    out, ptrs = _tp_outputs(dev, n, T, cap, want_rows, (S,), torch.float32, (A,), torch.float32)
    rc = L.lenv_td3d_test_population(C.byref(cfg), _ptr(params), _ptr(rng_keys), _ptr(episode_offset), _ptr(learn_calls), _ptr(reset_states),
                                     _ptr(gumbel), _ptr(noise), n, *ptrs, _stream())
    _lib.check(rc, "lenv_td3d_test_population")
    return out


def ql_test_population(cfg, q_table, tables, want_rows=True):
    """BaseAgent.test of a population of trained tabular agents (QL / SARSA and their count-based variants) in one launch
    (lenv_ql_test_population): agent i, Q-table q_table[i] (fp64 [agents, n_states * n_actions], the q_table of the fused tabular launches),
    runs T = cfg.test_episodes greedy episodes on the grid MDP `tables` (a dict next_state / reward / done [n_states, n_actions] of numpy
    arrays, as the fused loops take it, or of device tensors int32 / float64 / uint8).  Returns a dict of device tensors: returns fp64
    [agents,T], env_steps / agent_steps int32 [agents,T] and, with want_rows, row_state / row_action / row_next_state int32, row_reward /
    row_done fp32 [agents,T,cap]; slots at or beyond agent_steps[i][e] are zero (the kernel does not write them)."""
    dev = require_device()
    L = _lib.lib()
    _chk(q_table, torch.float64, "q_table")
    cap = _count("lenv_ql_test_rows_cap", C.byref(cfg))
    N, A, T = cfg.n_states, cfg.n_actions, cfg.test_episodes
    if q_table.dim() != 2 or q_table.shape[1] != N * A:
        raise ValueError("q_table must be [agents,%d]" % (N * A))
    tabs = []
    for name, dt, np_dt in (("next_state", torch.int32, "int32"), ("reward", torch.float64, "float64"), ("done", torch.uint8, "uint8")):
        t = tables[name]
        t = t.to(device=dev, dtype=dt) if torch.is_tensor(t) else torch.from_numpy(t.astype(np_dt)).to(dev)
        if t.numel() != N * A:
            raise ValueError("tables[%r] must be [%d,%d]" % (name, N, A))
        tabs.append(t.contiguous())
    n = q_table.shape[0]
    out, ptrs = _tp_outputs(dev, n, T, cap, want_rows, (), torch.int32, (), torch.int32)
    rc = L.lenv_ql_test_population(C.byref(cfg), _ptr(q_table), _ptr(tabs[0]), _ptr(tabs[1]), _ptr(tabs[2]), n, *ptrs, _stream())
    _lib.check(rc, "lenv_ql_test_population")
    return out


def qnet_td_forward(qd, online, target, replay, idx, gamma):
    """online/target [chains,P]; replay [chains,cap,row_stride]; idx int32 [chains,B] -> (q_sa, y) [chains,B]."""
    dev = require_device()
    for t, n in ((online, "online"), (target, "target"), (replay, "replay")):
        _chk(t, torch.float32, n)
    _chk(idx, torch.int32, "idx")
    chains, cap, stride = replay.shape
    B = idx.shape[1]
    q_sa = torch.empty((chains, B), dtype=torch.float32, device=dev)
    y = torch.empty((chains, B), dtype=torch.float32, device=dev)
    rc = _lib.lib().lenv_qnet_td_forward(C.byref(qd), _ptr(online), _ptr(target), _ptr(replay), cap, stride, _ptr(idx),
                                         chains, B, float(gamma), _ptr(q_sa), _ptr(y), _stream())
    _lib.check(rc, "lenv_qnet_td_forward")
    return q_sa, y


def chain_key(seed, generation, worker, kind):
    return int(_lib.lib().lenv_chain_key(seed, generation, worker, kind))


def _count(name, *args):
    """A non-negative count from a C entry point (a negative one is its error code)."""
    n = int(getattr(_lib.lib(), name)(*args))
    _lib.check(min(n, 0), name)
    return n


class _InnerLoopBase(object):
    """What the four fused inner-loop owners share for a fixed (cfg, chains): the workspace and outputs, the *Out and tapes structs
    that point at them, run()'s argument checks and the *_vary agents' per-chain hyper-parameters.  A family states its structs
    (Out, Tapes, the tapes its kernel reads), the name of its final-parameter buffer, its step trace as (name, trailing shape, dtype)
    with cfg field names for dimensions, and, for set_hp / draw_agent_init / chain_num_params, its cfg class, the cfg fields of the
    maximal batch / width / depth and its *_num_params / *_agent_init* entry points."""
    Out = Tapes = None
    tape_keys = None                      # the tapes the kernel reads (None: every one of Tapes.keys)
    final = None                          # "final_online" / "final_params"
    trace_spec = ()
    cfg_type = hp_fields = num_params_fn = agent_init_fn = None
    p_agent = None                        # QL: a table, no parameter vector

    def __init__(self, cfg, chains):
        self.dev = require_device()
        self.cfg, self.chains = cfg, int(chains)

    def _num_params(self, cfg, *outs):
        """the agent's parameter count at cfg's shapes (the TD3 counters also take optional actor / critic out-pointers)"""
        fn = getattr(_lib.lib(), self.num_params_fn)
        return _count(self.num_params_fn, C.byref(cfg), *(outs or (None,) * (len(fn.argtypes) - 1)))

    def _init_vary(self, vary):
        """Device arrays of include/lenv_hip.h's lenv_chain_hp for the chains + the struct that points at them."""
        self.vary = bool(vary)
        self.hp = self.hp_struct = self.agent_init = None
        if self.vary:
            dev, n = self.dev, self.chains
            self.hp = dict(lr=torch.zeros(n, dtype=torch.float64, device=dev), batch_size=torch.zeros(n, dtype=torch.int32, device=dev),
                           q_hidden=torch.zeros(n, dtype=torch.int32, device=dev), q_layers=torch.zeros(n, dtype=torch.int32, device=dev))
            self.hp_struct = _lib.ChainHp(_ptr(self.hp["lr"]), _ptr(self.hp["batch_size"]), _ptr(self.hp["q_hidden"]), _ptr(self.hp["q_layers"]))
            self.agent_init = torch.zeros((n, self.p_agent), dtype=torch.float32, device=dev)

    def _hp_arg(self):
        return C.byref(self.hp_struct) if self.vary else None

    def _init_icm(self, num_params_fn):
        self.icm = bool(self.cfg.icm_enabled)
        self.icm_init = self.icm_final = self.icm_io = None
        if self.icm:
            self.p_icm = _count(num_params_fn, C.byref(self.cfg))
            self.icm_init = torch.zeros((self.chains, self.p_icm), dtype=torch.float32, device=self.dev)
            self.icm_final = torch.zeros((self.chains, self.p_icm), dtype=torch.float32, device=self.dev)
            self.icm_io = _lib.IcmIo(_ptr(self.icm_init), _ptr(self.icm_final))

    def _icm_arg(self):
        return C.byref(self.icm_io) if self.icm else None

    def _alloc_outputs(self, ws_bytes, want_episode_stats, want_final, trace_cap):
        """The workspace (ws_bytes None: the kernel needs none), the common outputs, the optional final-parameter buffer and step
        trace, and self.out built in the Out struct's field order from the attributes / trace entries of those names."""
        dev, n, cfg = self.dev, self.chains, self.cfg
        if ws_bytes is not None:
            self.ws_bytes = int(ws_bytes)
            self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.score = torch.zeros(n, dtype=torch.float64, device=dev)
        self.stats = torch.zeros((n, 4), dtype=torch.int64, device=dev)
        self.status = torch.zeros(n, dtype=torch.int32, device=dev)
        self.episode_test_mean = self.episode_len = self.final_returns = None
        if want_episode_stats:
            E = max(cfg.train_episodes, 1)
            self.episode_test_mean = torch.zeros((n, E), dtype=torch.float64, device=dev)
            self.episode_len = torch.zeros((n, E), dtype=torch.int32, device=dev)
            self.final_returns = torch.zeros((n, cfg.test_episodes), dtype=torch.float64, device=dev)
        if self.final:
            setattr(self, self.final, torch.zeros((n, self.p_agent), dtype=torch.float32, device=dev) if want_final else None)
        self.trace_cap = int(trace_cap)
        self.trace = None
        if trace_cap:
            self.trace = {name: torch.zeros((n, self.trace_cap) + tuple(getattr(cfg, d) if isinstance(d, str) else d for d in shape),
                                            dtype=dtype, device=dev) for name, shape, dtype in self.trace_spec}
        tr, vals = self.trace or {}, []
        for f, _ in self.Out._fields_:
            if f.endswith("_cap"):                    # trace_cap; a family's own capacities (PPO: learn_cap) are attributes set before
                vals.append(int(getattr(self, f)))
            elif f.startswith("trace_"):
                vals.append(_ptr(tr.get(f[len("trace_"):])))
            else:
                vals.append(_ptr(getattr(self, f)))
        self.out = self.Out(*vals)

    def _tapes_arg(self, tapes):
        """byref of a Tapes struct over the tape tensors [chains, stride] the kernel reads (the other pairs (None, 0)), or None"""
        if tapes is None:
            return None
        keys = self.Tapes.keys if self.tape_keys is None else self.tape_keys
        vals = []
        for k in self.Tapes.keys:
            vals += [_ptr(tapes[k]), tapes[k].shape[1]] if k in keys else [None, 0]
        return C.byref(self.Tapes(*vals))

    def _check_run(self, theta, eps, worker, sign, rng_keys, agent_init=None):
        _chk(theta, torch.float32, "theta"); _chk(eps, torch.float32, "eps"); _chk(worker, torch.int32, "worker")
        _chk(sign, torch.float32, "sign"); _chk(rng_keys, torch.int64, "rng_keys")
        if self.p_agent is not None:
            _chk(agent_init, torch.float32, "agent_init")
            if agent_init.shape != (self.chains, self.p_agent):
                raise ValueError("agent_init must be [chains, %d]" % self.p_agent)

    def _run_args(self, theta, eps, worker, sign, agent_init, rng_keys, tapes):
        """run()'s checks, then what follows the cfg (and hp / icm) of the C launch"""
        self._check_run(theta, eps, worker, sign, rng_keys, agent_init)
        return (_ptr(theta), _ptr(eps), _ptr(worker), _ptr(sign), _ptr(agent_init), _ptr(rng_keys), self._tapes_arg(tapes), self.chains,
                _ptr(self.workspace), self.ws_bytes, C.byref(self.out), _stream())

    def set_hp(self, lr, batch_size, hidden_size, hidden_layer):
        """The chains' own hyper-parameters (host sequences of length `chains`; hidden_layer as the config writes it: the
        network has max(1, hidden_layer) hidden layers, models/model_utils.py:33-37)."""
        if not self.vary:
            raise ValueError("the inner loop was built without vary=True")
        n = self.chains
        if not (len(lr) == len(batch_size) == len(hidden_size) == len(hidden_layer) == n):
            raise ValueError("set_hp: need %d values per hyper-parameter" % n)
        max_batch, max_hidden, max_layers = (getattr(self.cfg, f) for f in self.hp_fields)
        layers = [max(1, int(v)) for v in hidden_layer]
        if max(batch_size) > max_batch or max(hidden_size) > max_hidden or max(layers) > max_layers or min(batch_size) < 1 \
                or min(hidden_size) < 1:
            raise ValueError("set_hp: a chain's hyper-parameters exceed the maxima the inner loop was sized for")
        self.hp["lr"].copy_(torch.tensor([float(v) for v in lr], dtype=torch.float64))
        self.hp["batch_size"].copy_(torch.tensor([int(v) for v in batch_size], dtype=torch.int32))
        self.hp["q_hidden"].copy_(torch.tensor([int(v) for v in hidden_size], dtype=torch.int32))
        self.hp["q_layers"].copy_(torch.tensor(layers, dtype=torch.int32))

    def chain_num_params(self, hidden_size, hidden_layer):
        """Parameter count of one chain's agent at its own shapes (the used prefix of its agent_init / final-parameter row)."""
        probe = self.cfg_type.from_buffer_copy(self.cfg)
        _, width, depth = self.hp_fields
        setattr(probe, width, int(hidden_size))
        setattr(probe, depth, max(1, int(hidden_layer)))
        return self._num_params(probe)

    def draw_agent_init(self, rng_keys):
        """Fresh agents at every chain's own shapes into self.agent_init (nn.Linear default init -- LayerNorm 1 / 0 --, keyed by the
        chain keys)."""
        _chk(rng_keys, torch.int64, "rng_keys")
        rc = getattr(_lib.lib(), self.agent_init_fn)(C.byref(self.cfg), self._hp_arg(), _ptr(rng_keys), self.chains, _ptr(self.agent_init),
                                                     _stream())
        _lib.check(rc, self.agent_init_fn)
        return self.agent_init

    def draw_icm_init(self, rng_keys, bounds):
        """Fresh ICMModel parameters per chain into self.icm_init (nn.Linear default init with `bounds` [p_icm], counter-RNG stream
        12 of every chain key)."""
        _chk(rng_keys, torch.int64, "rng_keys"); _chk(bounds, torch.float32, "bounds")
        rc = _lib.lib().lenv_chain_uniform_init(_ptr(rng_keys), self.chains, 12, self.p_icm, _ptr(bounds), _ptr(self.icm_init), _stream())
        _lib.check(rc, "lenv_chain_uniform_init")
        return self.icm_init


class _SegmentedInnerLoop(_InnerLoopBase):
    """run() of the families whose inner loop also runs as a series of episode segments.  A family states `entry` = (the C entry point of
    the single launch, the name _lib.check reports it under), `segment_entry`, `prefix` = which of the hp / icm arguments stand between the
    cfg and run()'s arguments, `resume_words` = the width of its resume record (words 0..2 = next episode, finished, status in every
    family), and overrides _launch_args for argument checks of its own."""
    entry = segment_entry = resume_words = None
    prefix = ()
    vary = False
    resume = None                         # the segment launches' records [chains, resume_words], allocated by the first

    def _launch_args(self, theta, eps, worker, sign, agent_init, rng_keys, tapes, segment=False):
        """_run_args behind the family's own checks (the *_vary agents: agent_init None = the drawn self.agent_init)"""
        if agent_init is None and self.vary:
            agent_init = self.agent_init
        return self._run_args(theta, eps, worker, sign, agent_init, rng_keys, tapes)

    def _prefix_args(self):
        return tuple(getattr(self, "_%s_arg" % p)() for p in self.prefix)

    def run(self, theta, eps, worker, sign, agent_init=None, rng_keys=None, tapes=None, episodes_per_launch=None, on_segment=None):
        """agent_init None: the drawn self.agent_init, for the families that keep one (the *_vary agents, Td3DiscreteInnerLoop).
        episodes_per_launch None: one launch from the first episode to the final test (asynchronous).  An integer: the same inner loop
        as a series of segment launches of that many episodes each (run_segment; same bits for every split).  After each segment the
        chains' `finished` words and statuses come to the host (one small copy, the only synchronisation), on_segment(episodes_done,
        finished_count) is called if given, then -- after the callback, so that it sees the segment in which a chain failed -- a bad status
        raises as check_status does, and the series stops as soon as every chain is finished.  A cfg without training episodes has no
        segment to run: ValueError (the single launch runs its closing test)."""
        if episodes_per_launch is None:
            fn, label = self.entry
            args = self._launch_args(theta, eps, worker, sign, agent_init, rng_keys, tapes)
            _lib.check(getattr(_lib.lib(), fn)(C.byref(self.cfg), *self._prefix_args(), *args), label)
            return self.score
        step = int(episodes_per_launch)
        if step < 1:
            raise ValueError("episodes_per_launch must be at least 1")
        E = self.cfg.train_episodes
        if E < 1:
            raise ValueError("episodes_per_launch needs a cfg with at least one training episode")
        for begin in range(0, E, step):
            end = min(E, begin + step)
            self.run_segment(theta, eps, worker, sign, agent_init, begin, end, rng_keys=rng_keys, tapes=tapes)
            finished, st = self.segment_state()
            if on_segment is not None:
                on_segment(end, int(finished.sum()))
            if int(st.min()) != 0:
                raise _lib.LenvError("inner loop reported status %s" % st.tolist())
            if int(finished.min()) == 1:
                break
        return self.score

    def run_segment(self, theta, eps, worker, sign, agent_init, episode_begin, episode_end, rng_keys=None, tapes=None):
        """Enqueue episodes [episode_begin, episode_end) of every chain (asynchronous).  episode_begin 0 starts afresh; a later segment goes
        on from self.resume and needs the same arguments and an untouched workspace."""
        args = self._launch_args(theta, eps, worker, sign, agent_init, rng_keys, tapes, segment=True)
        if self.resume is None:
            self.resume = torch.zeros((self.chains, self.resume_words), dtype=torch.int64, device=self.dev)
        rc = getattr(_lib.lib(), self.segment_entry)(C.byref(self.cfg), *self._prefix_args(), *args[:-1], int(episode_begin), int(episode_end),
                                                     _ptr(self.resume), args[-1])
        _lib.check(rc, self.segment_entry)
        return self.score

    def segment_state(self):
        """(finished [chains], status [chains]) on the host after the segments enqueued so far (synchronises): the record's finished word and
        the smaller of the record's status and the status output (a refused continuation, -10, is reported there alone)."""
        both = torch.stack((self.resume[:, 1], torch.minimum(self.resume[:, 2], self.status.to(torch.int64)))).cpu()
        return both[0], both[1]


_TD3_TRACE = (("action", ("action_dim",), torch.float32), ("state", ("state_dim",), torch.float32),
              ("next_state", ("state_dim",), torch.float32), ("reward", (), torch.float32))


class InnerLoop(_SegmentedInnerLoop):
    """Owns the workspace/outputs of lenv_ddqn_se_inner_loop for a fixed (cfg, chains)."""
    Out, Tapes, final = InnerOut, Tapes, "final_online"
    trace_spec = (("action", (), torch.int32), ("state", ("state_dim",), torch.float32), ("next_state", ("state_dim",), torch.float32),
                  ("reward_done", (2,), torch.float32))
    cfg_type, hp_fields = DdqnCfg, ("batch_size", "q_hidden", "q_layers")
    num_params_fn, agent_init_fn = "lenv_dueling_num_params", "lenv_dueling_agent_init_hp"
    segment_entry, resume_words = "lenv_dueling_se_inner_loop_segment", _lib.DUELING_RESUME_WORDS

    def __init__(self, cfg, chains, want_episode_stats=True, want_final_online=False, trace_cap=0, vary=False, segments=False):
        """vary=True: the *_vary agents -- cfg carries the MAXIMAL batch_size / q_hidden / q_layers, every chain runs with its
        own lr / batch_size / hidden_size / hidden_layer (set_hp) in the GEMM-tiled kernel (lenv_dueling_se_inner_loop_icm).
        segments=True: the inner loop will run as segment launches (run(episodes_per_launch=) / run_segment), which exist on the
        GEMM-tiled kernel alone: a cfg the register-resident kernel would take is routed there too (its single launch included; a plain-DQN
        cfg needs grad_chunk 0, the one sequential batch gradient that kernel computes)."""
        super().__init__(cfg, chains)
        L = _lib.lib()
        # DuelingDDQN, and DDQN whose Critic_DQN the register-resident kernel refuses (hidden_layer >= 2 / wide layers),
        # run in the GEMM-tiled kernel; `dueling` keeps its name from the first of the two
        # (a RewardEnv / real-env cfg with an explicit micro-chunk takes the register-resident kernel's RENV instantiations; with grad_chunk 0 --
        # one sequential batch gradient -- the probe refuses it and the GEMM-tiled kernel runs it)
        icm = bool(cfg.icm_enabled)                    # ICM agents (ddqn_icm / duelingddqn_icm): GEMM-tiled kernel only
        self.segments = bool(segments)
        self.dueling = bool(vary) or icm or self.segments or cfg.agent_kind == 1 or (cfg.agent_kind == 0 and L.lenv_ddqn_se_lds_bytes(C.byref(cfg)) <= 0
                                                                    and L.lenv_dueling_num_params(C.byref(cfg)) > 0)
        if self.dueling:       # the GEMM-tiled kernel: per-chain hyper-parameters and the ICM may be NULL
            self.entry, self.prefix = ("lenv_dueling_se_inner_loop_icm", "lenv_dueling_se_inner_loop"), ("hp", "icm")
            self.p_agent = self._num_params(cfg)
            ws_bytes = L.lenv_dueling_se_workspace_bytes(C.byref(cfg), self.chains)
        else:
            self.entry = ("lenv_ddqn_se_inner_loop",) * 2
            self.p_agent = mlp_num_params(mlp_desc(cfg.state_dim, cfg.q_hidden, cfg.q_layers, cfg.num_actions, cfg.q_act))
            ws_bytes = L.lenv_ddqn_se_workspace_bytes(C.byref(cfg), self.chains)
        self._init_vary(vary)
        self._init_icm("lenv_icm_num_params")
        self._alloc_outputs(ws_bytes, want_episode_stats, want_final_online, trace_cap)

    def _launch_args(self, theta, eps, worker, sign, agent_init, rng_keys, tapes, segment=False):
        if segment and not self.segments:
            raise ValueError("segment launches need an inner loop built with segments=True (the GEMM-tiled kernel and its workspace)")
        return super()._launch_args(theta, eps, worker, sign, agent_init, rng_keys, tapes)


class QlInnerLoop(_InnerLoopBase):
    """Owns the outputs of lenv_ql_rn_inner_loop for a fixed (cfg, chains, grid MDP)."""
    Out, Tapes, tape_keys = QlOut, Tapes, ("eps_uniform", "rand_action")
    trace_spec = (("action", (), torch.int32), ("state", (2,), torch.int32), ("reward_done", (2,), torch.float32))

    def __init__(self, cfg, chains, tables, want_episode_stats=True, trace_cap=0):
        super().__init__(cfg, chains)
        N, A = cfg.n_states, cfg.n_actions
        self.next_state = torch.from_numpy(tables["next_state"].astype("int32")).contiguous().to(self.dev)
        self.reward = torch.from_numpy(tables["reward"].astype("float64")).contiguous().to(self.dev)
        self.done = torch.from_numpy(tables["done"].astype("uint8")).contiguous().to(self.dev)
        H = cfg.rn_hidden            # Linear(N, H) | (layers - 1) x Linear(H, H) | Linear(H, 1)
        self.p_theta = N * H + H + (max(1, cfg.rn_layers) - 1) * (H * H + H) + H + 1
        self.q_table = self.shaped = None
        if want_episode_stats:
            self.q_table = torch.zeros((self.chains, N * A), dtype=torch.float64, device=self.dev)
            self.shaped = torch.zeros((self.chains, N * A), dtype=torch.float32, device=self.dev)
        self.hp_alpha = self.hp_gamma = None
        self._alloc_outputs(None, want_episode_stats, False, trace_cap)

    def set_hp(self, alpha=None, gamma=None):
        """The chains' own alpha / gamma (host sequences of length `chains`; None: cfg's value for every chain): run() then goes through
        lenv_ql_rn_inner_loop_hp.  gamma also enters the chain's shaped-reward table (BaseAgent.train hands it to the env)."""
        for name, vals in (("hp_alpha", alpha), ("hp_gamma", gamma)):
            if vals is not None:
                if len(vals) != self.chains:
                    raise ValueError("set_hp: need %d values per hyper-parameter" % self.chains)
                vals = torch.tensor([float(v) for v in vals], dtype=torch.float64).to(self.dev)
            setattr(self, name, vals)

    def run(self, theta, eps, worker, sign, rng_keys=None, tapes=None, shaped_override=None):
        self._check_run(theta, eps, worker, sign, rng_keys)
        _chk(shaped_override, torch.float32, "shaped_override")
        if theta is not None and theta.numel() != self.p_theta and self.cfg.reward_env_type != 0:
            raise ValueError("theta must hold %d reward-net parameters" % self.p_theta)
        args = (_ptr(theta), _ptr(eps), _ptr(worker), _ptr(sign), _ptr(shaped_override), _ptr(self.next_state), _ptr(self.reward),
                _ptr(self.done), _ptr(rng_keys), self._tapes_arg(tapes), self.chains, C.byref(self.out), _stream())
        if self.hp_alpha is None and self.hp_gamma is None:
            rc = _lib.lib().lenv_ql_rn_inner_loop(C.byref(self.cfg), *args)
        else:
            rc = _lib.lib().lenv_ql_rn_inner_loop_hp(C.byref(self.cfg), _ptr(self.hp_alpha), _ptr(self.hp_gamma), *args)
        _lib.check(rc, "lenv_ql_rn_inner_loop")
        return self.score


class QlSeInnerLoop(_InnerLoopBase):
    """Owns the workspace/outputs of lenv_ql_se_inner_loop (the tabular agents on a gridworld VirtualEnv) for a fixed (cfg, chains, grid
    MDP).  trace_cap > 0 also records trace_se [chains, trace_cap, n_states + 2]: the SE's raw next-state vector | reward | done of the last SE
    step of every agent step."""
    Out, Tapes, tape_keys = QlOut, Tapes, ("eps_uniform", "rand_action")
    trace_spec = QlInnerLoop.trace_spec

    def __init__(self, cfg, chains, tables, want_episode_stats=True, trace_cap=0):
        super().__init__(cfg, chains)
        N, A = cfg.n_states, cfg.n_actions
        self.p_theta = _count("lenv_ql_se_num_params", C.byref(cfg))           # a refused cfg raises here, before any allocation
        self.lds_bytes = _count("lenv_ql_se_lds_bytes", C.byref(cfg))
        self.next_state = torch.from_numpy(tables["next_state"].astype("int32")).contiguous().to(self.dev)
        self.reward = torch.from_numpy(tables["reward"].astype("float64")).contiguous().to(self.dev)
        self.done = torch.from_numpy(tables["done"].astype("uint8")).contiguous().to(self.dev)
        self.shaped = None
        self.q_table = torch.zeros((self.chains, N * A), dtype=torch.float64, device=self.dev) if want_episode_stats else None
        self._alloc_outputs(_count("lenv_ql_se_workspace_bytes", C.byref(cfg), self.chains), want_episode_stats, False, trace_cap)
        self.trace_se = torch.zeros((self.chains, self.trace_cap, N + 2), dtype=torch.float32, device=self.dev) if trace_cap else None

    def run(self, theta, eps, worker, sign, rng_keys=None, tapes=None):
        self._check_run(theta, eps, worker, sign, rng_keys)
        if theta is None or theta.numel() != self.p_theta:
            raise ValueError("theta must hold %d SE parameters" % self.p_theta)
        rc = _lib.lib().lenv_ql_se_inner_loop(C.byref(self.cfg), _ptr(theta), _ptr(eps), _ptr(worker), _ptr(sign), _ptr(self.next_state),
                                              _ptr(self.reward), _ptr(self.done), _ptr(rng_keys), self._tapes_arg(tapes), self.chains,
                                              C.byref(self.out), _ptr(self.trace_se), _ptr(self.workspace), self.ws_bytes, _stream())
        _lib.check(rc, "lenv_ql_se_inner_loop")
        return self.score


class Td3InnerLoop(_SegmentedInnerLoop):
    """Owns the workspace/outputs of lenv_td3_rn_inner_loop for a fixed (cfg, chains)."""
    Out, Tapes, final, trace_spec = Td3Out, Td3Tapes, "final_params", _TD3_TRACE
    cfg_type, hp_fields = Td3Cfg, ("batch_size", "hidden", "layers")
    num_params_fn, agent_init_fn = "lenv_td3_num_params", "lenv_td3_agent_init_hp"
    entry, prefix = ("lenv_td3_rn_inner_loop_icm", "lenv_td3_rn_inner_loop"), ("hp", "icm")
    segment_entry, resume_words = "lenv_td3_rn_inner_loop_segment", _lib.TD3_RESUME_WORDS

    def __init__(self, cfg, chains, want_episode_stats=True, want_final_params=False, trace_cap=0, vary=False):
        """vary=True: TD3_vary -- cfg carries the maximal batch_size / hidden / layers, every chain runs with its own
        hyper-parameters (set_hp) through lenv_td3_rn_inner_loop_icm."""
        super().__init__(cfg, chains)
        pa, pc = C.c_int64(), C.c_int64()
        self.p_agent = self._num_params(cfg, C.byref(pa), C.byref(pc))
        self.p_actor, self.p_critic = pa.value, pc.value
        self._init_vary(vary)
        self._init_icm("lenv_td3_icm_num_params")       # TD3(icm=True): select_agent "td3_icm" / "td3_icm_vary"
        self.p_theta = cfg.state_dim * cfg.rn_hidden + 2 * cfg.rn_hidden + 1
        self._alloc_outputs(_lib.lib().lenv_td3_rn_workspace_bytes(C.byref(cfg), self.chains), want_episode_stats, want_final_params,
                            trace_cap)


class Td3DiscreteInnerLoop(_SegmentedInnerLoop):
    """Owns the workspace/outputs of lenv_td3d_inner_loop (TD3_discrete_vary on a VirtualEnv) for a fixed (cfg, chains).
    vary=True: cfg carries the maximal batch_size / hidden / layers, every chain runs with its own draw (set_hp).
    rn (a _lib.Td3dRnCfg): the chains train on RewardEnv(real env) / the real env instead, through lenv_td3d_rn_inner_loop; theta is the
    reward net.  agent_init None (run's default): the drawn self.agent_init, with or without vary."""
    Out, Tapes, final, trace_spec = Td3Out, Td3dTapes, "final_params", _TD3_TRACE
    cfg_type, hp_fields = Td3dCfg, ("batch_size", "hidden", "layers")
    num_params_fn, agent_init_fn = "lenv_td3d_num_params", "lenv_td3d_agent_init"
    resume_words = _lib.TD3D_RESUME_WORDS

    def __init__(self, cfg, chains, want_episode_stats=True, want_final_params=False, trace_cap=0, vary=False, rn=None):
        super().__init__(cfg, chains)
        L = _lib.lib()
        pa, pc = C.c_int64(), C.c_int64()
        self.p_agent = self._num_params(cfg, C.byref(pa), C.byref(pc))
        self.p_actor, self.p_critic = pa.value, pc.value
        self.rn = rn
        if rn is None:
            self.entry, self.segment_entry, self.prefix = ("lenv_td3d_inner_loop",) * 2, "lenv_td3d_inner_loop_segment", ("hp",)
            self.p_theta = int(L.lenv_td3d_se_num_params(C.byref(cfg)))
            ws_bytes = L.lenv_td3d_workspace_bytes(C.byref(cfg), self.chains)
        else:
            self.entry, self.segment_entry, self.prefix = ("lenv_td3d_rn_inner_loop",) * 2, "lenv_td3d_rn_inner_loop_segment", ("rn", "hp")
            self.p_theta = _count("lenv_td3d_rn_num_params", C.byref(cfg), C.byref(rn))
            ws_bytes = L.lenv_td3d_rn_workspace_bytes(C.byref(cfg), C.byref(rn), self.chains)
        self._init_vary(vary)
        if not self.vary:
            self.agent_init = torch.zeros((self.chains, self.p_agent), dtype=torch.float32, device=self.dev)
        self._alloc_outputs(ws_bytes, want_episode_stats, want_final_params, trace_cap)

    def _rn_arg(self):
        return C.byref(self.rn)

    def _launch_args(self, theta, eps, worker, sign, agent_init, rng_keys, tapes, segment=False):
        if agent_init is None:
            agent_init = self.agent_init
        args = self._run_args(theta, eps, worker, sign, agent_init, rng_keys, tapes)
        if theta.numel() != self.p_theta:
            raise ValueError("theta must hold %d %s parameters" % (self.p_theta, "SE" if self.rn is None else "reward-net"))
        return args


class PpoInnerLoop(_SegmentedInnerLoop):
    """Owns the workspace/outputs of lenv_ppo_rn_inner_loop (PPO on a RewardEnv over a continuous real env) for a fixed (cfg, chains).
    learn_cap > 0: the step at which each of the first learn_cap PPO.learn calls fired and the parameters after it are recorded
    (learn_step [chains, learn_cap], learn_params [chains, learn_cap, P])."""
    Out, Tapes, final = PpoOut, PpoTapes, "final_params"
    trace_spec = _TD3_TRACE + (("done", (), torch.float32),)
    cfg_type, num_params_fn = PpoCfg, "lenv_ppo_num_params"
    entry = ("lenv_ppo_rn_inner_loop",) * 2
    segment_entry, resume_words = "lenv_ppo_rn_inner_loop_segment", _lib.PPO_RESUME_WORDS

    def __init__(self, cfg, chains, want_episode_stats=True, want_final_params=False, trace_cap=0, learn_cap=0):
        super().__init__(cfg, chains)
        pa, pc = C.c_int64(), C.c_int64()
        self.p_agent = self._num_params(cfg, C.byref(pa), C.byref(pc))       # action_std [A] | actor.net | critic.net
        self.p_actor, self.p_critic = pa.value, pc.value
        self.rows = _count("lenv_ppo_rows", C.byref(cfg))                    # rows of one learn call
        self.p_theta = _count("lenv_ppo_rn_num_params", C.byref(cfg))
        self.learn_cap = int(learn_cap)
        self.learn_step = self.learn_params = None
        if self.learn_cap:
            self.learn_step = torch.zeros((self.chains, self.learn_cap), dtype=torch.int32, device=self.dev)
            self.learn_params = torch.zeros((self.chains, self.learn_cap, self.p_agent), dtype=torch.float32, device=self.dev)
        self._alloc_outputs(self._workspace_bytes(), want_episode_stats, want_final_params, trace_cap)

    def _workspace_bytes(self):
        return _count("lenv_ppo_rn_workspace_bytes", C.byref(self.cfg), self.chains)

    def _ppo_args(self, theta, eps, worker, sign, agent_init, rng_keys, tapes):
        args = self._run_args(theta, eps, worker, sign, agent_init, rng_keys, tapes)
        if theta is not None and self.cfg.reward_env_type != 0 and theta.numel() != self.p_theta:
            raise ValueError("theta must hold %d reward-net parameters" % self.p_theta)
        return args

    def _launch_args(self, theta, eps, worker, sign, agent_init, rng_keys, tapes, segment=False):
        return self._ppo_args(theta, eps, worker, sign, agent_init, rng_keys, tapes)


class PpoIcmInnerLoop(PpoInnerLoop):
    """PPO(icm=True), the transfer scripts' `ppo_icm` agent, through lenv_ppo_icm_inner_loop: PpoInnerLoop with a fresh Intrinsic
    Curiosity Module per chain.  icm = dict(feature_dim, hidden_size, lr, beta, eta), the config's `icm` section; icm_init
    [chains, p_icm] (fill it, or draw_icm_init) are the modules' start parameters, icm_final receives them after the run."""
    entry = ("lenv_ppo_icm_inner_loop",) * 2
    segment_entry = "lenv_ppo_icm_inner_loop_segment"
    prefix = ("icm_feature_dim", "icm_hidden", "icm_lr", "icm_beta", "icm_eta", "icm")

    def __init__(self, cfg, chains, icm, **kw):
        self.icm_settings = dict(feature_dim=int(icm["feature_dim"]), hidden_size=int(icm["hidden_size"]), lr=float(icm["lr"]),
                                 beta=float(icm["beta"]), eta=float(icm["eta"]))
        self.icm = True
        self.p_icm = _count("lenv_ppo_icm_num_params", C.byref(cfg), self.icm_settings["feature_dim"], self.icm_settings["hidden_size"])
        super().__init__(cfg, chains, **kw)
        self.icm_init = torch.zeros((self.chains, self.p_icm), dtype=torch.float32, device=self.dev)
        self.icm_final = torch.zeros((self.chains, self.p_icm), dtype=torch.float32, device=self.dev)
        self.icm_io = _lib.IcmIo(_ptr(self.icm_init), _ptr(self.icm_final))

    def _workspace_bytes(self):
        return _count("lenv_ppo_icm_workspace_bytes", C.byref(self.cfg), self.icm_settings["feature_dim"], self.icm_settings["hidden_size"],
                      self.chains)

    def _prefix_args(self):
        s = self.icm_settings
        return (s["feature_dim"], s["hidden_size"], s["lr"], s["beta"], s["eta"], self._icm_arg())


def rn_shape_population(cfg, theta, eps, worker, sign, next_state, reward, chains=1):
    """(phi [chains,N], shaped [chains,N,A]) of a population of perturbed reward networks on a grid MDP."""
    dev = require_device()
    N, A = cfg.n_states, cfg.n_actions
    phi = torch.empty((chains, N), dtype=torch.float32, device=dev)
    shaped = torch.empty((chains, N, A), dtype=torch.float32, device=dev)
    rc = _lib.lib().lenv_rn_shape_population(C.byref(cfg), _ptr(theta), _ptr(eps), _ptr(worker), _ptr(sign), chains,
                                             _ptr(next_state), _ptr(reward), _ptr(phi), _ptr(shaped), _stream())
    _lib.check(rc, "lenv_rn_shape_population")
    return phi, shaped


GRAD_EVAL_TYPES = {"mean": 0, "minmax": 1}


def nes_worker_best(chain_scores, pop, mirrored=True, num_grad_evals=1, grad_eval_type="mean", out=None):
    """GTN_Worker.calc_best_score for `pop` workers; chain_scores [pop, 1+2G] = (orig, add_1..G, sub_1..G)."""
    dev = require_device()
    _chk(chain_scores, torch.float64, "chain_scores")
    if grad_eval_type not in GRAD_EVAL_TYPES:
        raise NotImplementedError('Unknown parameter for grad_eval_type: ' + str(grad_eval_type))
    result = out if out is not None else torch.empty((pop, 4), dtype=torch.float64, device=dev)
    _chk(result, torch.float64, "out")
    rc = _lib.lib().lenv_nes_worker_best_multi(_ptr(chain_scores), pop, int(num_grad_evals), 1 if mirrored else 0,
                                               GRAD_EVAL_TYPES[grad_eval_type], _ptr(result), _stream())
    _lib.check(rc, "lenv_nes_worker_best_multi")
    return result


def nes_draw(seed, generation, pop, p_theta, noise_std, chains, chains_per_worker, worker_lo, bounds, want_keys=True):
    """(eps [pop,p_theta], agent_init [chains,p_agent] or None, rng_keys int64 [chains]) of one generation, one launch.
    `generation` may be a device int64 tensor [1] (captured generations: read when the kernel runs)."""
    dev = require_device()
    eps = torch.empty((pop, p_theta), dtype=torch.float32, device=dev)
    init = torch.empty((chains, bounds.numel()), dtype=torch.float32, device=dev) if bounds is not None and chains > 0 else None
    keys = torch.empty(chains, dtype=torch.int64, device=dev) if want_keys and chains > 0 else None
    tail = (pop, p_theta, float(noise_std), _ptr(eps), chains, int(chains_per_worker), int(worker_lo),
            bounds.numel() if bounds is not None else 0, _ptr(bounds), _ptr(init), _ptr(keys), _stream())
    if torch.is_tensor(generation):
        rc = _lib.lib().lenv_nes_draw_dev(int(seed) & (2 ** 64 - 1), _ptr(_chk(generation, torch.int64, "generation")), *tail)
    else:
        rc = _lib.lib().lenv_nes_draw(int(seed) & (2 ** 64 - 1), int(generation), *tail)
    _lib.check(rc, "lenv_nes_draw")
    return eps, init, keys


def nes_status_fold(status, result):
    rc = _lib.lib().lenv_nes_status_fold(_ptr(status), status.numel(), _ptr(result), result.shape[0], _stream())
    _lib.check(rc, "lenv_nes_status_fold")


def nes_rank_update(score_transform_type, gathered, rank_table, theta, eps, step_size, nes_step_size=False, weight_decay=0.0,
                    theta_prev=None, generation=None):
    """In-place theta update; returns the score_transform weights [pop] (float64).  theta_prev / generation (device tensors):
    the captured-generation form, lenv_nes_rank_update_keep (theta_prev <- theta before the update, generation[0] += 1)."""
    dev = require_device()
    _chk(gathered, torch.float64, "gathered"); _chk(rank_table, torch.float64, "rank_table")
    _chk(theta, torch.float32, "theta"); _chk(eps, torch.float32, "eps")
    pop = gathered.shape[0]
    weights = torch.empty(pop, dtype=torch.float64, device=dev)
    head = (int(score_transform_type), _ptr(gathered), _ptr(rank_table), pop, _ptr(theta), _ptr(eps),
            theta.numel() if theta is not None else 0, float(step_size), 1 if nes_step_size else 0, float(weight_decay), _ptr(weights))
    if theta_prev is not None or generation is not None:
        rc = _lib.lib().lenv_nes_rank_update_keep(*head, _ptr(_chk(theta_prev, torch.float32, "theta_prev")),
                                                  _ptr(_chk(generation, torch.int64, "generation")), _stream())
    else:
        rc = _lib.lib().lenv_nes_rank_update(*head, _stream())
    _lib.check(rc, "lenv_nes_rank_update")
    return weights


class HipNesEngine(object):
    """The compute engine GTN_Master/GTN_Worker drive: every method is a thin call into liblenv_hip.so.
    (tests substitute an oracle-backed object with the same methods to exercise the host/distributed logic on CPU)"""
    name = "hip"

    def __init__(self):
        self.device = require_device()

    def make_inner(self, cfg, chains, **kw):
        return InnerLoop(cfg, chains, **kw)

    def make_inner_td3(self, cfg, chains, **kw):
        return Td3InnerLoop(cfg, chains, **kw)

    def make_inner_td3d(self, cfg, chains, **kw):
        return Td3DiscreteInnerLoop(cfg, chains, **kw)

    def inner_scores_td3(self, inner, theta, eps, worker, sign, agent_init, rng_keys, **run_kw):
        return inner.run(theta, eps, worker, sign, agent_init, rng_keys=rng_keys, **run_kw)

    def make_inner_ppo(self, cfg, chains, **kw):
        return PpoInnerLoop(cfg, chains, **kw)

    def inner_scores_ppo(self, inner, theta, eps, worker, sign, agent_init, rng_keys):
        return inner.run(theta, eps, worker, sign, agent_init, rng_keys=rng_keys)

    def make_inner_ql(self, cfg, chains, tables, **kw):
        return QlInnerLoop(cfg, chains, tables, **kw)

    def inner_scores_ql(self, inner, theta, eps, worker, sign, rng_keys):
        return inner.run(theta, eps, worker, sign, rng_keys=rng_keys)

    def make_inner_ql_se(self, cfg, chains, tables, **kw):
        return QlSeInnerLoop(cfg, chains, tables, **kw)

    def inner_scores_ql_se(self, inner, theta, eps, worker, sign, rng_keys):
        return inner.run(theta, eps, worker, sign, rng_keys=rng_keys)

    def inner_scores(self, inner, theta, eps, worker, sign, agent_init, rng_keys, **run_kw):
        return inner.run(theta, eps, worker, sign, agent_init, rng_keys=rng_keys, **run_kw)

    def check_status(self, inner):
        st = inner.status.cpu()
        if int(st.min()) != 0:
            raise _lib.LenvError("inner loop reported status %s" % st.tolist())

    def run_checked(self, inner, *args, **kw):
        """inner.run(...) + host check of the chain statuses (synchronises).  A launch whose teams of workgroups could not assemble
        (status -10: a foreign kernel held CUs, include/lenv_hip.h lenv_ddqn_cfg::team_size) is repeated once with one workgroup per
        chain -- the chains are deterministic functions of their inputs -- and the inner loop keeps that setting."""
        out = inner.run(*args, **kw)
        st = inner.status.cpu()
        if int(st.min()) == _lib.STATUS_TEAM_GAVE_UP and hasattr(inner.cfg, "team_size") and inner.cfg.team_size != 1:
            inner.cfg.team_size = 1
            out = inner.run(*args, **kw)
            st = inner.status.cpu()
        if int(st.min()) != 0:
            raise _lib.LenvError("inner loop reported status %s" % st.tolist())
        return out

    def worker_best(self, chain_scores, pop, mirrored, num_grad_evals=1, grad_eval_type="mean", out=None):
        return nes_worker_best(chain_scores, pop, mirrored, num_grad_evals, grad_eval_type, out=out)

    def draw(self, seed, generation, pop, p_theta, noise_std, chains, chains_per_worker, worker_lo, bounds):
        return nes_draw(seed, generation, pop, p_theta, noise_std, chains, chains_per_worker, worker_lo, bounds)

    def status_fold(self, inner, result):
        nes_status_fold(inner.status, result)

    def rank_update(self, score_transform_type, gathered, rank_table, theta, eps, step_size, nes_step_size, weight_decay,
                    theta_prev=None, generation=None):
        return nes_rank_update(score_transform_type, gathered, rank_table, theta, eps, step_size, nes_step_size, weight_decay,
                               theta_prev=theta_prev, generation=generation)

    graph_capable = True            # every call above only enqueues on the current stream: a generation can be captured
