"""Loader of tests/ppo_icm_ref.c, the CPU restatement of PPO(icm=True) (TEST INFRASTRUCTURE).

tests/ppo_ref.py's recipe: compiled with the oracle Makefile's flags next to the oracle library; the cfg struct is the product's own ctypes
mirror, so one config feeds the kernel and the restatement."""
import ctypes as C
import os
import subprocess

import numpy as np

from learning_environments_amd import _lib
from oracle import oracle as orc
import ppo_ref
from ppo_ref import CFLAGS, Out, Tapes, _fp

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ppo_icm_ref.c")
_DEPS = [_SRC, os.path.join(_HERE, "ppo_ref.c"), os.path.join(os.path.dirname(_HERE), "oracle", "lenv_oracle_icm.inc")]
_OUT = os.path.join(os.path.dirname(_HERE), "oracle", "_build", "libppo_icm_ref.so")


class Icm(C.Structure):
    _fields_ = [("feature_dim", C.c_int32), ("hidden", C.c_int32), ("lr", C.c_double), ("beta", C.c_double), ("eta", C.c_double),
                ("icm_init", C.POINTER(C.c_float)), ("icm_final", C.POINTER(C.c_float)), ("learn_icm", C.POINTER(C.c_float)),
                ("learn_intr", C.POINTER(C.c_float))]


_ref = None


def lib():
    global _ref
    if _ref is None:
        orc_path = orc.build()
        if not os.path.exists(_OUT) or os.path.getmtime(_OUT) < max(os.path.getmtime(p) for p in _DEPS):
            subprocess.check_call([os.environ.get("CC", "gcc")] + CFLAGS + ["-shared", "-o", _OUT, _SRC, "-lm"])
        C.CDLL(orc_path, mode=C.RTLD_GLOBAL)          # the oracle's exported primitives resolve from it
        L = C.CDLL(_OUT)
        L.ppo_icm_ref_num_params.restype = C.c_int64
        L.ppo_icm_ref_num_params.argtypes = [C.POINTER(_lib.PpoCfg), C.c_int, C.c_int]
        L.ppo_icm_ref_chain.restype = C.c_int
        L.ppo_icm_ref_chain.argtypes = [C.POINTER(_lib.PpoCfg), C.POINTER(Icm), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint64,
                                        C.POINTER(Tapes), C.POINTER(Out)]
        _ref = L
    return _ref


def icm_num_params(cfg, feature_dim, hidden_size):
    return int(lib().ppo_icm_ref_num_params(C.byref(cfg), int(feature_dim), int(hidden_size)))


def chain(cfg, icm, icm_init, rn_params, agent_init, rng_key=0, tapes=None, trace_cap=0, learn_cap=0):
    """ppo_ref.chain with a fresh ICM: icm = dict(feature_dim, hidden_size, lr, beta, eta), icm_init [p_icm].  Returns ppo_ref.chain's dict
    plus icm_final [p_icm], learn_icm [learn calls, p_icm] (the module after each recorded call) and learn_intr [learn calls, rows] (that
    call's intrinsic rewards)."""
    L = lib()
    S, A, E, T = cfg.state_dim, cfg.action_dim, max(cfg.train_episodes, 1), cfg.test_episodes
    P, N = ppo_ref.num_params(cfg), ppo_ref.rows(cfg)
    Pi = icm_num_params(cfg, icm["feature_dim"], icm["hidden_size"])
    rn = np.ascontiguousarray(rn_params if rn_params is not None and len(rn_params) else np.zeros(1), dtype=np.float32)
    init = np.ascontiguousarray(agent_init, dtype=np.float32)
    iinit = np.ascontiguousarray(icm_init, dtype=np.float32)
    assert init.size == P and iinit.size == Pi, (init.size, P, iinit.size, Pi)
    keep, tp = [], None
    if tapes is not None:
        an, tn = (np.ascontiguousarray(tapes[k], dtype=np.float32).reshape(-1, A) for k in ("act_noise", "test_noise"))
        tr, te = (np.ascontiguousarray(tapes[k], dtype=np.float64) for k in ("train_reset", "test_reset"))
        keep = [an, tn, tr, te]
        tp = Tapes(_fp(an), an.shape[0], _fp(tn), tn.shape[0], _fp(tr, C.c_double), tr.shape[0], _fp(te, C.c_double), te.shape[0])
    tc, lc = max(int(trace_cap), 1), max(int(learn_cap), 1)
    t_act, t_s, t_ns = np.zeros((tc, A), np.float32), np.zeros((tc, S), np.float32), np.zeros((tc, S), np.float32)
    t_r, t_d = np.zeros(tc, np.float32), np.zeros(tc, np.float32)
    l_step, l_par = np.zeros(lc, np.int32), np.zeros((lc, P), np.float32)
    l_icm, l_intr, ifin = np.zeros((lc, Pi), np.float32), np.zeros((lc, N), np.float32), np.zeros(Pi, np.float32)
    etm, elen, fr, fp_ = np.zeros(E, np.float64), np.zeros(E, np.int32), np.zeros(T, np.float64), np.zeros(P, np.float32)
    out = Out(trace_cap=int(trace_cap), trace_action=_fp(t_act), trace_state=_fp(t_s), trace_next_state=_fp(t_ns), trace_reward=_fp(t_r),
              trace_done=_fp(t_d), learn_cap=int(learn_cap), learn_step=_fp(l_step, C.c_int32), learn_params=_fp(l_par),
              episode_test_mean=_fp(etm, C.c_double), episode_len=_fp(elen, C.c_int32), final_returns=_fp(fr, C.c_double), final_params=_fp(fp_))
    ic = Icm(int(icm["feature_dim"]), int(icm["hidden_size"]), float(icm["lr"]), float(icm["beta"]), float(icm["eta"]), _fp(iinit), _fp(ifin),
             _fp(l_icm), _fp(l_intr))
    rc = L.ppo_icm_ref_chain(C.byref(cfg), C.byref(ic), _fp(rn), _fp(init), C.c_uint64(int(rng_key) & (2 ** 64 - 1)),
                             C.byref(tp) if tp is not None else None, C.byref(out))
    del keep
    n, nl = int(out.trace_n), int(out.learn_n)
    return dict(rc=rc, score=out.score, episodes_run=out.episodes_run, train_steps=out.train_steps, learn_calls=out.learn_calls,
                test_steps=out.test_steps, episode_test_mean=etm[:cfg.train_episodes], episode_len=elen[:cfg.train_episodes], final_returns=fr,
                final_params=fp_, learn_step=l_step[:nl], learn_params=l_par[:nl], icm_final=ifin, learn_icm=l_icm[:nl], learn_intr=l_intr[:nl],
                trace=dict(action=t_act[:n], state=t_s[:n], next_state=t_ns[:n], reward=t_r[:n], done=t_d[:n]))
