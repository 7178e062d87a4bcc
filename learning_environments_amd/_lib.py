"""ctypes loader for liblenv_hip.so (C-ABI: include/lenv_hip.h).  Fails loudly when the library is absent."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblenv_hip.so")
CSRC = os.path.join(_HERE, "csrc")

ACT = {"identity": 0, "relu": 1, "leakyrelu": 2, "tanh": 3, "prelu": 4}
ENV = {"CartPole-v0": 0, "Acrobot-v1": 1, "HalfCheetah-v3": 2, "MountainCar-v0": 3, "Pendulum-v0": 4, "MountainCarContinuous-v0": 5}
RNG_COUNTER, RNG_TAPE = 0, 1
ACTOR_TD3, ACTOR_PPO = 0, 1                      # LENV_ACTOR_*: the `kind` of lenv_actor_test_population (its cfg is a Td3Cfg / PpoCfg)
VARIANT_NO_WAVECHAIN, VARIANT_GENERIC, VARIANT_TEAM_NARROW, VARIANT_NO_DIRECT, VARIANT_NO_EARLY_GRAD = 1, 2, 4, 8, 16     # lenv_ddqn_cfg / lenv_td3_cfg kernel_variant bits (A/B timing, kernel-vs-kernel parity tests)
TD3_RESUME_WORDS = 32                            # LENV_TD3_RESUME_WORDS: int64 words of a chain's record between two segment launches
DUELING_RESUME_WORDS = 32                        # LENV_DUELING_RESUME_WORDS: the same for lenv_dueling_se_inner_loop_segment
PPO_RESUME_WORDS = 32                            # LENV_PPO_RESUME_WORDS: the same for lenv_ppo_rn_inner_loop_segment
TD3D_RESUME_WORDS = 32                           # LENV_TD3D_RESUME_WORDS: the same for lenv_td3d_inner_loop_segment / lenv_td3d_rn_inner_loop_segment
STATUS_TEAM_GAVE_UP = -10                        # a team member waited too long for the others: repeat the launch with team_size 1
STATUS_WRONG_SEGMENT = -10                       # the same value from lenv_td3_rn_inner_loop_segment: the chain's record names another episode_begin
                                                 # (segment launches never run on a team; engine.run_checked's retry is for single launches only)

ERRORS = {-1: ValueError, -2: NotImplementedError, -3: ValueError, -4: RuntimeError, -5: RuntimeError}


class LenvError(RuntimeError):
    pass


class MlpDesc(C.Structure):
    _fields_ = [("in_dim", C.c_int32), ("hidden", C.c_int32), ("layers", C.c_int32), ("out_dim", C.c_int32),
                ("act", C.c_int32), ("prelu", C.c_float), ("use_layer_norm", C.c_int32)]


class DdqnCfg(C.Structure):
    _fields_ = [("env_id", C.c_int32), ("state_dim", C.c_int32), ("num_actions", C.c_int32), ("max_steps", C.c_int32),
                ("se_hidden", C.c_int32), ("se_layers", C.c_int32), ("se_act", C.c_int32), ("se_prelu", C.c_float),
                ("q_hidden", C.c_int32), ("q_layers", C.c_int32), ("q_act", C.c_int32), ("q_prelu", C.c_float),
                ("batch_size", C.c_int32), ("rb_size", C.c_int32),
                ("train_episodes", C.c_int32), ("test_episodes", C.c_int32), ("init_episodes", C.c_int32),
                ("early_out_num", C.c_int32), ("grad_chunk", C.c_int32), ("rng_mode", C.c_int32),
                ("agent_kind", C.c_int32), ("feature_dim", C.c_int32),
                ("solved_reward", C.c_double), ("gamma", C.c_double), ("lr", C.c_double), ("tau", C.c_double),
                ("eps_init", C.c_double), ("eps_min", C.c_double), ("eps_decay", C.c_double),
                ("adam_beta1", C.c_double), ("adam_beta2", C.c_double), ("adam_eps", C.c_double),
                ("step_budget", C.c_int64),
                ("icm_enabled", C.c_int32), ("icm_feature_dim", C.c_int32), ("icm_hidden", C.c_int32), ("se_layer_norm", C.c_int32),
                ("icm_lr", C.c_double), ("icm_beta", C.c_double), ("icm_eta", C.c_double),
                ("synthetic_env_type", C.c_int32), ("reward_env_type", C.c_int32),
                ("same_action_num", C.c_int32),
                ("team_size", C.c_int32),        # workgroups per chain: 0 = automatic, 1 = never a team, G = at most G
                ("kernel_variant", C.c_int32),   # VARIANT_* bits, 0 = fastest
                ("q_layer_norm", C.c_int32), ("test_mode", C.c_int32), ("early_out_virtual_diff", C.c_double)]


def _tape_fields(keys):
    """A tapes struct's fields: one (device pointer, row stride) pair per tape, in `keys` order."""
    return [f for k in keys for f in ((k, C.c_void_p), (k + "_stride", C.c_int64))]


TAPE_KEYS = ("eps_uniform", "rand_action", "replay_idx", "train_reset", "test_reset")
TD3_TAPE_KEYS = ("rand_action", "act_noise", "test_noise", "policy_noise", "replay_idx", "train_reset", "test_reset")
TD3D_TAPE_KEYS = ("rand_action", "act_noise", "test_noise", "policy_noise", "gumbel_act", "gumbel_test", "gumbel_target", "gumbel_actor",
                  "replay_idx", "train_reset", "test_reset")


class Tapes(C.Structure):
    keys = TAPE_KEYS
    _fields_ = _tape_fields(TAPE_KEYS)


class InnerOut(C.Structure):
    _fields_ = [("score", C.c_void_p), ("stats", C.c_void_p), ("status", C.c_void_p),
                ("episode_test_mean", C.c_void_p), ("episode_len", C.c_void_p), ("final_returns", C.c_void_p),
                ("final_online", C.c_void_p), ("trace_cap", C.c_int64), ("trace_action", C.c_void_p),
                ("trace_state", C.c_void_p), ("trace_next_state", C.c_void_p), ("trace_reward_done", C.c_void_p)]


class ChainHp(C.Structure):                  # include/lenv_hip.h: lenv_chain_hp (device arrays [chains])
    _fields_ = [("lr", C.c_void_p), ("batch_size", C.c_void_p), ("q_hidden", C.c_void_p), ("q_layers", C.c_void_p)]


class IcmIo(C.Structure):                    # include/lenv_hip.h: lenv_icm_io
    _fields_ = [("icm_init", C.c_void_p), ("icm_final", C.c_void_p)]


class QlCfg(C.Structure):
    _fields_ = [("n_states", C.c_int32), ("n_actions", C.c_int32), ("start_state", C.c_int32), ("max_steps", C.c_int32),
                ("rn_hidden", C.c_int32), ("rn_layers", C.c_int32), ("rn_act", C.c_int32), ("rn_prelu", C.c_float),
                ("reward_env_type", C.c_int32), ("train_episodes", C.c_int32), ("test_episodes", C.c_int32),
                ("init_episodes", C.c_int32), ("early_out_num", C.c_int32), ("batch_size", C.c_int32), ("rng_mode", C.c_int32),
                ("agent_kind", C.c_int32), ("count_based", C.c_int32),
                ("solved_reward", C.c_double), ("alpha", C.c_double), ("gamma", C.c_double), ("eps_init", C.c_double),
                ("eps_min", C.c_double), ("eps_decay", C.c_double), ("beta", C.c_double), ("step_budget", C.c_int64), ("same_action_num", C.c_int32), ("rn_layer_norm", C.c_int32), ("test_mode", C.c_int32), ("early_out_virtual_diff", C.c_double)]


class QlOut(C.Structure):
    _fields_ = [("score", C.c_void_p), ("stats", C.c_void_p), ("status", C.c_void_p), ("episode_test_mean", C.c_void_p),
                ("episode_len", C.c_void_p), ("final_returns", C.c_void_p), ("q_table", C.c_void_p), ("shaped", C.c_void_p),
                ("trace_cap", C.c_int64), ("trace_action", C.c_void_p), ("trace_state", C.c_void_p),
                ("trace_reward_done", C.c_void_p)]


class Td3Cfg(C.Structure):
    _fields_ = [("env_id", C.c_int32), ("state_dim", C.c_int32), ("action_dim", C.c_int32), ("max_steps", C.c_int32),
                ("rn_hidden", C.c_int32), ("rn_layers", C.c_int32), ("rn_act", C.c_int32), ("rn_prelu", C.c_float),
                ("reward_env_type", C.c_int32), ("info_dim", C.c_int32), ("hidden", C.c_int32), ("layers", C.c_int32), ("act", C.c_int32),
                ("prelu", C.c_float), ("batch_size", C.c_int32), ("rb_size", C.c_int32), ("train_episodes", C.c_int32),
                ("test_episodes", C.c_int32), ("init_episodes", C.c_int32), ("early_out_num", C.c_int32),
                ("policy_delay", C.c_int32), ("rng_mode", C.c_int32),
                ("solved_reward", C.c_double), ("gamma", C.c_double), ("lr", C.c_double), ("tau", C.c_double),
                ("action_std", C.c_double), ("policy_std", C.c_double), ("policy_std_clip", C.c_double),
                ("max_action", C.c_double), ("adam_beta1", C.c_double), ("adam_beta2", C.c_double), ("adam_eps", C.c_double),
                ("step_budget", C.c_int64),
                ("icm_enabled", C.c_int32), ("icm_feature_dim", C.c_int32), ("icm_hidden", C.c_int32), ("use_layer_norm", C.c_int32),
                ("icm_lr", C.c_double), ("icm_beta", C.c_double), ("icm_eta", C.c_double),
                ("virtual_env", C.c_int32), ("same_action_num", C.c_int32), ("team_size", C.c_int32), ("kernel_variant", C.c_int32), ("rn_layer_norm", C.c_int32), ("test_mode", C.c_int32), ("early_out_virtual_diff", C.c_double)]


class Td3Tapes(C.Structure):
    keys = TD3_TAPE_KEYS
    _fields_ = _tape_fields(TD3_TAPE_KEYS)


class Td3dCfg(C.Structure):
    """lenv_td3d_cfg (include/lenv_hip.h): TD3_discrete_vary on a VirtualEnv over a discrete-action real env."""
    _fields_ = [("env_id", C.c_int32), ("state_dim", C.c_int32), ("action_dim", C.c_int32), ("max_steps", C.c_int32),
                ("se_hidden", C.c_int32), ("se_layers", C.c_int32), ("se_act", C.c_int32), ("se_prelu", C.c_float),
                ("hidden", C.c_int32), ("layers", C.c_int32), ("act", C.c_int32), ("prelu", C.c_float),
                ("use_layer_norm", C.c_int32), ("gumbel_hard", C.c_int32),
                ("batch_size", C.c_int32), ("rb_size", C.c_int32), ("train_episodes", C.c_int32), ("test_episodes", C.c_int32),
                ("init_episodes", C.c_int32), ("early_out_num", C.c_int32), ("policy_delay", C.c_int32), ("rng_mode", C.c_int32),
                ("solved_reward", C.c_double), ("gamma", C.c_double), ("lr", C.c_double), ("tau", C.c_double),
                ("action_std", C.c_double), ("policy_std", C.c_double), ("policy_std_clip", C.c_double), ("max_action", C.c_double),
                ("gumbel_temp", C.c_double), ("adam_beta1", C.c_double), ("adam_beta2", C.c_double), ("adam_eps", C.c_double),
                ("step_budget", C.c_int64), ("se_layer_norm", C.c_int32), ("test_mode", C.c_int32), ("early_out_virtual_diff", C.c_double)]


class Td3dRnCfg(C.Structure):
    """lenv_td3d_rn_cfg: the RewardEnv (or, reward_env_type 0, the real env) that lenv_td3d_rn_inner_loop trains TD3_discrete_vary on."""
    _fields_ = [("synthetic_env_type", C.c_int32), ("reward_env_type", C.c_int32), ("rn_hidden", C.c_int32), ("rn_layers", C.c_int32),
                ("rn_act", C.c_int32), ("rn_prelu", C.c_float), ("rn_layer_norm", C.c_int32)]


class Td3dTapes(C.Structure):
    keys = TD3D_TAPE_KEYS
    _fields_ = _tape_fields(TD3D_TAPE_KEYS)


class Td3Out(C.Structure):
    _fields_ = [("score", C.c_void_p), ("stats", C.c_void_p), ("status", C.c_void_p), ("episode_test_mean", C.c_void_p),
                ("episode_len", C.c_void_p), ("final_returns", C.c_void_p), ("final_params", C.c_void_p), ("trace_cap", C.c_int64),
                ("trace_action", C.c_void_p), ("trace_state", C.c_void_p), ("trace_next_state", C.c_void_p), ("trace_reward", C.c_void_p)]


PPO_TAPE_KEYS = ("act_noise", "test_noise", "train_reset", "test_reset")


class PpoCfg(C.Structure):
    """lenv_ppo_cfg (include/lenv_hip.h): PPO on a RewardEnv (or, reward_env_type 0, the real env) over a continuous real env."""
    _fields_ = [("env_id", C.c_int32), ("state_dim", C.c_int32), ("action_dim", C.c_int32), ("max_steps", C.c_int32),
                ("rn_hidden", C.c_int32), ("rn_layers", C.c_int32), ("rn_act", C.c_int32), ("rn_prelu", C.c_float),
                ("reward_env_type", C.c_int32), ("info_dim", C.c_int32), ("hidden", C.c_int32), ("layers", C.c_int32), ("act", C.c_int32),
                ("prelu", C.c_float), ("train_episodes", C.c_int32), ("test_episodes", C.c_int32), ("init_episodes", C.c_int32),
                ("early_out_num", C.c_int32), ("ppo_epochs", C.c_int32), ("same_action_num", C.c_int32), ("rng_mode", C.c_int32),
                ("reserved", C.c_int32),
                ("solved_reward", C.c_double), ("gamma", C.c_double), ("lr", C.c_double), ("action_std", C.c_double),
                ("vf_coef", C.c_double), ("ent_coef", C.c_double), ("eps_clip", C.c_double), ("update_episodes", C.c_double),
                ("adam_beta1", C.c_double), ("adam_beta2", C.c_double), ("adam_eps", C.c_double)]


class PpoTapes(C.Structure):
    keys = PPO_TAPE_KEYS
    _fields_ = _tape_fields(PPO_TAPE_KEYS)


class PpoOut(C.Structure):
    _fields_ = [("score", C.c_void_p), ("stats", C.c_void_p), ("status", C.c_void_p), ("episode_test_mean", C.c_void_p),
                ("episode_len", C.c_void_p), ("final_returns", C.c_void_p), ("final_params", C.c_void_p), ("trace_cap", C.c_int64),
                ("trace_action", C.c_void_p), ("trace_state", C.c_void_p), ("trace_next_state", C.c_void_p), ("trace_reward", C.c_void_p),
                ("trace_done", C.c_void_p), ("learn_cap", C.c_int64), ("learn_step", C.c_void_p), ("learn_params", C.c_void_p)]


# lenv_struct_size(which) order (include/lenv_hip.h)
ABI_STRUCTS = [MlpDesc, DdqnCfg, QlCfg, Td3Cfg, Td3dCfg, Tapes, InnerOut, QlOut, Td3Tapes, Td3Out, Td3dTapes, ChainHp, IcmIo, Td3dRnCfg,
               PpoCfg, PpoTapes, PpoOut]

_vp, _i32, _i64, _f64, _P = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.POINTER
# what follows the cfg (and hp / icm) of an inner-loop launch: theta, eps, worker, sign, agent_init, rng_keys, tapes, chains,
# workspace, workspace_bytes, out, stream
_DDQN_RUN = [_vp] * 6 + [_P(Tapes), _i64, _vp, C.c_size_t, _P(InnerOut), _vp]
_TD3_RUN = [_vp] * 6 + [_P(Td3Tapes), _i64, _vp, C.c_size_t, _P(Td3Out), _vp]
_TD3D_RUN = [_vp] * 6 + [_P(Td3dTapes), _i64, _vp, C.c_size_t, _P(Td3Out), _vp]
_NES_DRAW_TAIL = [_i64, _i64, C.c_float, _vp, _i64, _i32, _i64, _i64, _vp, _vp, _vp, _vp]
_NES_RANK_HEAD = [_i32, _vp, _vp, _i64, _vp, _vp, _i64, _f64, _i32, _f64, _vp]

# name -> (restype, argtypes) of every C-ABI entry point the package binds (include/lenv_hip.h)
SIGNATURES = {
    "lenv_abi_version": (C.c_int, []),
    "lenv_error_string": (C.c_char_p, [C.c_int]),
    "lenv_struct_size": (_i64, [_i32]),
    "lenv_mlp_num_params": (_i64, [_P(MlpDesc)]),
    "lenv_mlp_forward": (C.c_int, [_P(MlpDesc), _vp, _vp, _i64, _vp, _vp]),
    "lenv_se_step_population": (C.c_int, [_P(MlpDesc)] * 3 + [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lenv_se_step_population_vec": (C.c_int, [_P(MlpDesc)] * 3 + [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lenv_se_step_vec_path": (_i32, [_P(MlpDesc)] * 3 + [_i32]),
    "lenv_qnet_td_forward": (C.c_int, [_P(MlpDesc), _vp, _vp, _vp, _i64, _i32, _vp, _i64, _i32, _f64, _vp, _vp, _vp]),
    "lenv_chain_key": (C.c_uint64, [C.c_uint64] * 4),
    "lenv_rng_unit": (_f64, [C.c_uint64, C.c_uint32, C.c_uint64]),
    "lenv_chain_uniform_init": (C.c_int, [_vp, _i64, C.c_uint32, _i64, _vp, _vp, _vp]),
    "lenv_ddqn_se_workspace_bytes": (C.c_size_t, [_P(DdqnCfg), _i64]),
    "lenv_ddqn_se_lds_bytes": (_i64, [_P(DdqnCfg)]),
    "lenv_ddqn_se_team_size": (C.c_int, [_P(DdqnCfg), _i64]),
    "lenv_ddqn_se_forward_split": (C.c_int, [_P(DdqnCfg), _P(_i32), _P(_i32)]),
    "lenv_ddqn_se_forward_deal": (C.c_int, [_P(DdqnCfg), _P(_i32), _P(_i32)]),
    "lenv_ddqn_se_inner_loop": (C.c_int, [_P(DdqnCfg)] + _DDQN_RUN),
    "lenv_dueling_se_workspace_bytes": (C.c_size_t, [_P(DdqnCfg), _i64]),
    "lenv_dueling_num_params": (_i64, [_P(DdqnCfg)]),
    "lenv_dueling_team_size": (C.c_int, [_P(DdqnCfg), _i64]),
    "lenv_dueling_se_inner_loop": (C.c_int, [_P(DdqnCfg)] + _DDQN_RUN),
    "lenv_dueling_se_inner_loop_hp": (C.c_int, [_P(DdqnCfg), _P(ChainHp)] + _DDQN_RUN),
    "lenv_dueling_se_inner_loop_icm": (C.c_int, [_P(DdqnCfg), _P(ChainHp), _P(IcmIo)] + _DDQN_RUN),
    "lenv_dueling_se_inner_loop_segment": (C.c_int, [_P(DdqnCfg), _P(ChainHp), _P(IcmIo)] + _DDQN_RUN[:-1] + [_i32, _i32, _vp, _vp]),
    "lenv_dueling_agent_init_hp": (C.c_int, [_P(DdqnCfg), _P(ChainHp), _vp, _i64, _vp, _vp]),
    "lenv_icm_num_params": (_i64, [_P(DdqnCfg)]),
    "lenv_real_env_reset": (C.c_int, [_i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "lenv_real_env_step": (C.c_int, [_i32, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lenv_cheetah_standin_reset": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "lenv_cheetah_standin_step": (C.c_int, [_i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lenv_cont_env_reset": (C.c_int, [_i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "lenv_cont_env_step": (C.c_int, [_i32, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lenv_ql_rn_inner_loop": (C.c_int, [_P(QlCfg), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(Tapes), _i64, _P(QlOut), _vp]),
    "lenv_ql_rn_inner_loop_hp": (C.c_int, [_P(QlCfg), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(Tapes), _i64, _P(QlOut), _vp]),
    "lenv_ql_se_num_params": (_i64, [_P(QlCfg)]),
    "lenv_ql_se_lds_bytes": (_i64, [_P(QlCfg)]),
    "lenv_ql_se_workspace_bytes": (_i64, [_P(QlCfg), _i64]),
    "lenv_ql_se_inner_loop": (C.c_int, [_P(QlCfg), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(Tapes), _i64, _P(QlOut), _vp, _vp, _i64, _vp]),
    "lenv_rn_shape_population": (C.c_int, [_P(QlCfg), _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "lenv_rn_num_params": (_i64, [_i32] * 5),
    "lenv_rn_shape_rows": (C.c_int, [_i32, _P(MlpDesc), _i32, _i32, _f64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "lenv_rn_step_population": (C.c_int, [_i32, _i32, _i32, _P(MlpDesc), _i32, _i32, _f64, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lenv_agent_test_rows_cap": (_i64, [_P(DdqnCfg)]),
    "lenv_agent_test_population": (C.c_int, [_P(DdqnCfg), _vp, _vp, _vp, _vp, _i64] + [_vp] * 8 + [_vp]),
    # kind (ACTOR_TD3 / ACTOR_PPO), cfg (a Td3Cfg / PpoCfg by reference), ...
    "lenv_actor_test_rows_cap": (_i64, [C.c_int, _vp]),
    "lenv_actor_test_population": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _i64] + [_vp] * 8 + [_vp]),
    # cfg, params, rng_keys, episode_offset, learn_calls, reset_states, gumbel, noise, agents, 3 outputs, 5 row arrays, stream
    "lenv_td3d_test_rows_cap": (_i64, [_P(Td3dCfg)]),
    "lenv_td3d_test_population": (C.c_int, [_P(Td3dCfg), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64] + [_vp] * 8 + [_vp]),
    # cfg, q_table, next_state, reward, done, agents, 3 outputs, 5 row arrays, stream
    "lenv_ql_test_rows_cap": (_i64, [_P(QlCfg)]),
    "lenv_ql_test_population": (C.c_int, [_P(QlCfg), _vp, _vp, _vp, _vp, _i64] + [_vp] * 8 + [_vp]),
    "lenv_td3_rn_workspace_bytes": (C.c_size_t, [_P(Td3Cfg), _i64]),
    "lenv_td3_num_params": (_i64, [_P(Td3Cfg), _P(_i64), _P(_i64)]),
    "lenv_td3_rn_team_size": (C.c_int, [_P(Td3Cfg), _i64]),
    "lenv_td3_rn_inner_loop": (C.c_int, [_P(Td3Cfg)] + _TD3_RUN),
    "lenv_td3_rn_inner_loop_hp": (C.c_int, [_P(Td3Cfg), _P(ChainHp)] + _TD3_RUN),
    "lenv_td3_rn_inner_loop_icm": (C.c_int, [_P(Td3Cfg), _P(ChainHp), _P(IcmIo)] + _TD3_RUN),
    "lenv_td3_rn_inner_loop_segment": (C.c_int, [_P(Td3Cfg), _P(ChainHp), _P(IcmIo)] + _TD3_RUN[:-1] + [_i32, _i32, _vp, _vp]),
    "lenv_td3_agent_init_hp": (C.c_int, [_P(Td3Cfg), _P(ChainHp), _vp, _i64, _vp, _vp]),
    "lenv_td3_icm_num_params": (_i64, [_P(Td3Cfg)]),
    "lenv_td3d_workspace_bytes": (C.c_size_t, [_P(Td3dCfg), _i64]),
    "lenv_td3d_num_params": (_i64, [_P(Td3dCfg), _P(_i64), _P(_i64)]),
    "lenv_td3d_se_num_params": (_i64, [_P(Td3dCfg)]),
    "lenv_td3d_inner_loop": (C.c_int, [_P(Td3dCfg), _P(ChainHp)] + _TD3D_RUN),
    "lenv_td3d_inner_loop_segment": (C.c_int, [_P(Td3dCfg), _P(ChainHp)] + _TD3D_RUN[:-1] + [_i32, _i32, _vp, _vp]),
    "lenv_td3d_agent_init": (C.c_int, [_P(Td3dCfg), _P(ChainHp), _vp, _i64, _vp, _vp]),
    "lenv_td3d_rn_workspace_bytes": (C.c_size_t, [_P(Td3dCfg), _P(Td3dRnCfg), _i64]),
    "lenv_td3d_rn_num_params": (_i64, [_P(Td3dCfg), _P(Td3dRnCfg)]),
    "lenv_td3d_rn_inner_loop": (C.c_int, [_P(Td3dCfg), _P(Td3dRnCfg), _P(ChainHp)] + _TD3D_RUN),
    "lenv_td3d_rn_inner_loop_segment": (C.c_int, [_P(Td3dCfg), _P(Td3dRnCfg), _P(ChainHp)] + _TD3D_RUN[:-1] + [_i32, _i32, _vp, _vp]),
    "lenv_ppo_rows": (_i64, [_P(PpoCfg)]),
    "lenv_ppo_num_params": (_i64, [_P(PpoCfg), _P(_i64), _P(_i64)]),
    "lenv_ppo_rn_num_params": (_i64, [_P(PpoCfg)]),
    "lenv_ppo_rn_lds_bytes": (_i64, [_P(PpoCfg)]),
    "lenv_ppo_rn_workspace_bytes": (_i64, [_P(PpoCfg), _i64]),
    "lenv_ppo_rn_inner_loop": (C.c_int, [_P(PpoCfg)] + [_vp] * 6 + [_P(PpoTapes), _i64, _vp, C.c_size_t, _P(PpoOut), _vp]),
    "lenv_ppo_rn_inner_loop_segment": (C.c_int, [_P(PpoCfg)] + [_vp] * 6 + [_P(PpoTapes), _i64, _vp, C.c_size_t, _P(PpoOut), _i32, _i32, _vp, _vp]),
    "lenv_ppo_icm_num_params": (_i64, [_P(PpoCfg), _i32, _i32]),
    "lenv_ppo_icm_workspace_bytes": (_i64, [_P(PpoCfg), _i32, _i32, _i64]),
    "lenv_ppo_icm_inner_loop": (C.c_int, [_P(PpoCfg), _i32, _i32, C.c_double, C.c_double, C.c_double, _P(IcmIo)] + [_vp] * 6 +
                                [_P(PpoTapes), _i64, _vp, C.c_size_t, _P(PpoOut), _vp]),
    "lenv_ppo_icm_inner_loop_segment": (C.c_int, [_P(PpoCfg), _i32, _i32, C.c_double, C.c_double, C.c_double, _P(IcmIo)] + [_vp] * 6 +
                                        [_P(PpoTapes), _i64, _vp, C.c_size_t, _P(PpoOut), _i32, _i32, _vp, _vp]),
    "lenv_se_fit_num_params": (_i64, [_P(MlpDesc)] * 3),
    "lenv_se_fit_lds_bytes": (_i64, [_P(MlpDesc)] * 3 + [_i32]),
    "lenv_se_fit_workspace_bytes": (_i64, [_P(MlpDesc)] * 3 + [_i32, _i64]),
    "lenv_se_fit_population": (C.c_int, [_P(MlpDesc)] * 3 + [_vp, _vp, _vp, _vp, _i64, _i32, _i64, _i64, _f64, _f64, _f64, _f64, _vp, _vp, _i64,
                                         _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "lenv_nes_worker_best": (C.c_int, [_vp, _i64, _i32, _vp, _vp]),
    "lenv_nes_worker_best_multi": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    "lenv_nes_draw": (C.c_int, [C.c_uint64, C.c_uint64] + _NES_DRAW_TAIL),
    "lenv_nes_draw_dev": (C.c_int, [C.c_uint64, _vp] + _NES_DRAW_TAIL),
    "lenv_nes_status_fold": (C.c_int, [_vp, _i64, _vp, _i64, _vp]),
    "lenv_nes_rank_update": (C.c_int, _NES_RANK_HEAD + [_vp]),
    "lenv_nes_rank_update_keep": (C.c_int, _NES_RANK_HEAD + [_vp, _vp, _vp]),
}
EXPORTS = list(SIGNATURES)


def build(force=False):
    """Compile every HIP source for gfx950 into liblenv_hip.so (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "-s", "clean"])
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j4"])
    return LIB_PATH


_lib = None


def lib():
    """The loaded C-ABI library.  Raises if it has not been built: there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LenvError("liblenv_hip.so is missing (%s). Build it with `python -c 'import __graft_entry__ as g; "
                            "g.build()'` or `make -C learning_environments_amd/csrc`; there is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        if L.lenv_abi_version() != 7:
            raise LenvError("liblenv_hip.so ABI version mismatch")
        for which, cls in enumerate(ABI_STRUCTS):     # the ctypes mirrors must have the library's layout
            if L.lenv_struct_size(which) != C.sizeof(cls):
                raise LenvError("ctypes mirror of %s has %d bytes, the library's struct %d" % (cls.__name__, C.sizeof(cls), L.lenv_struct_size(which)))
        _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().lenv_error_string(rc).decode()
        raise ERRORS.get(rc, LenvError)("%s: %s (%d)" % (what, msg, rc))
