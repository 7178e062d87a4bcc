// ppo_rn_inner_loop.hip -- fused NES inner loop for a PPO agent trained on a RewardEnv (learned reward shaping around a continuous real env,
// or the real env itself), one 512-thread workgroup per chain.
//
// Replaces GTN_Worker.calc_score (agents/GTN_worker.py:187-221) with
//   PPO.train / learn / select_*_action                      agents/PPO.py:64-188
//   Actor_PPO.forward / evaluate / clamp, Critic_V           models/actor_critic.py:38-61,74-81
//   BaseAgent.test, env_solved                               agents/base_agent.py:49-62,155-227
//   EnvWrapper.step (real branch) -> RewardEnv.step          envs/env_wrapper.py:49-70, envs/reward_env.py:61-133
//
// Structure of td3_rn_inner_loop.hip: action_std | actor.net | critic.net with their Adam state and the on-policy row buffer (s, a, r, done;
// lenv_ppo_rows(cfg) rows, no ring, no sampling) live in a per-chain HBM arena; the rollout runs the actor on one row (thread j owns output j
// of a layer: the k-ascending fmaf chain the MFMA product runs), steps ContEnv<ENV> and evaluates the reward net (lenv_rn.cuh: theta in LDS, or in
// the arena for nets of two or more hidden layers; phi(s') of step t is phi(s) of step t + 1).  PPO.learn is the hot part: every layer product over the N rows -- forward, input gradient, weight gradient with
// the reduction running over the rows -- is the canonical-order workgroup GEMM of lenv_gemm.cuh in row blocks of 256; the per-row loss
// derivatives (ppo_row_grads) are one thread per row; the returns scan, their mean and variance run left to right in one thread over an LDS copy.
// Gaussian draws come from tapes (parity mode) or the counter RNG through the deterministic Box-Muller.
//
// The kernel's body is ppo_rn_inner_kernel.inc, compiled three times: ppo_rn_inner_kernel (one launch from the first episode to the final test),
// ppo_rn_segment_kernel (lenv_ppo_rn_inner_loop_segment: episodes [begin, end) with a resume record per chain) and ppo_icm_segment_kernel
// (lenv_ppo_icm_inner_loop / _segment: PPO(icm=True), the segment kernel with the Intrinsic Curiosity Module of lenv_icm.cuh inside learn;
// CPU restatement: tests/ppo_icm_ref.c).
//
// Refused (LENV_ERR_UNSUPPORTED from the queries, before a launch): hidden > 128, more than two hidden layers, rows outside [2, 2048], more than
// 64 test episodes, an agent PReLU (its slope would be a trained parameter), LayerNorm in the agent nets (lenv_ppo_cfg has no field for it:
// config.ppo_cfg_from_config refuses) and in a reward net with two or more hidden layers.  CPU restatement: tests/ppo_ref.c.
#include "lenv_gemm.cuh"
#include "lenv_icm.cuh"
#include "lenv_rn.cuh"
#include "lenv_host.h"
#include "lenv_actor_params.cuh"      // PP_MAXL, PP_MAXW, PP_MAXT, PpoMlp / ppo_mlp

namespace lenv {

constexpr int PP_MAXN = 2048;    // rows of one learn call (the MountainCarContinuous transfer settings need 1999, the HalfCheetah ones 1001)
constexpr int PP_MAXI = 256;     // rows of one product block
constexpr int PP_STD = 8;        // arena floats reserved for action_std in front of actor.net (A <= 6; keeps the nets 16-byte aligned)

struct PpoArgs {
    lenv_ppo_cfg cfg;
    const float *theta, *eps; const int32_t *worker; const float *sign;
    const float *agent_init; const uint64_t *rng_keys;
    lenv_ppo_tapes tapes;
    float *arena; int64_t arena_stride;
    lenv_ppo_out out;
    int N;                                    // rows of one learn call
    int P, Pa, Pc;                            // ABI row: action_std [A] | actor.net [Pa] | critic.net [Pc]
    int oA, oC, PP;                           // the same in the arena: action_std at 0, actor.net at oA, critic.net at oC, PP floats in all (pads never read)
    int P_rn, P_rn_lds;
    int64_t a_params, a_m, a_v, a_grad, a_x, a_act, a_rew, a_done, a_ret, a_oldlp, a_mean, a_val, a_dz, a_gs, a_dv, a_ha[PP_MAXL], a_hc[PP_MAXL],
        a_d[2], a_meter, a_rn;
    // lenv_ppo_rn_inner_loop_segment (ppo_rn_segment_kernel): episodes [ep_begin, ep_end) of every chain, resume records [chains, LENV_PPO_RESUME_WORDS];
    // the other entry point: 0, train_episodes, nullptr.  (Behind everything else: ppo_rn_inner_kernel reads its arguments where they were.)
    int ep_begin, ep_end; int64_t *resume;
    // lenv_ppo_icm_inner_loop[_segment] (ppo_icm_segment_kernel): the module's shapes and settings, fresh parameters per chain, optional final
    // parameters, the arena offsets of the next-observation rows and of the IB_* buffers.  (Behind everything else, as above.)
    int icm_F, icm_H, P_icm;
    double icm_lr, icm_beta, icm_eta;
    const float *icm_init; float *icm_final;
    int64_t a_xn, a_icm[IB_COUNT];
};

// log-probability of action a under Normal(mean, std) summed over the action dims, left to right (torch.distributions.Normal.log_prob);
// lg[k] = (float)log(std[k])
template <int A>
__device__ __forceinline__ float ppo_logprob(const float *a, const float *mean, const float *sd, const float *lg)
{
    float lp = 0.0f;
#pragma unroll
    for (int k = 0; k < A; ++k) {
        const float d = a[k] - mean[k], var = sd[k] * sd[k];
        const float t = (-(d * d)) / (2.0f * var) - lg[k] - 0.9189385332046727f;
        lp = k == 0 ? t : lp + t;
    }
    return lp;
}

// per-row derivatives of loss.mean() (PPO.py:164-179), operation by operation as tests/ppo_ref.c ppo_row_grads: std0 = action_std as the
// log-probability saw it, stdc = after evaluate's clamp (what the entropy and autograd's saved tensors see)
struct PpoRowConsts { float inv_n, lo, hi, gent, cv; };
template <int A>
__device__ __forceinline__ void ppo_row_grads(const PpoRowConsts &c, const float *a, const float *mean, const float *std0, const float *lg0, const float *stdc,
                                              float old_lp, float ret, float v, float *dz, float *gs, float &dv)
{
    const float lp = ppo_logprob<A>(a, mean, std0, lg0);
    const float ratio = det_expf(lp - old_lp);
    const float adv = ret - v;
    const float clipped = ratio < c.lo ? c.lo : (ratio > c.hi ? c.hi : ratio);
    const float surr1 = ratio * adv, surr2 = clipped * adv;
    const float g = -c.inv_n;
    const bool inside = ratio >= c.lo && ratio <= c.hi;
    float dratio;
    if (surr1 < surr2) dratio = g * adv;
    else if (surr1 > surr2) dratio = inside ? g * adv : 0.0f;
    else dratio = inside ? g * adv : (g * 0.5f) * adv;      // a tie splits the gradient; inside the clip range both halves reach the ratio
    const float dlp = dratio * ratio;
#pragma unroll
    for (int k = 0; k < A; ++k) {
        const float d = a[k] - mean[k], var = std0[k] * std0[k];
        dz[k] = (dlp * (d / var)) * fma32(-mean[k], mean[k], 1.0f);
        gs[k] = dlp * (((d * d) * stdc[k]) / (var * var) - 1.0f / stdc[k]) + c.gent / stdc[k];
    }
    dv = c.cv * (v - ret);
}

// The resume record of a chain after a segment (include/lenv_hip.h documents the words): thread 0, behind the barrier that follows the threads'
// atomicMin into the folded status.  std_old = actor_old's action_std (LDS), as the next act() has to see it
__device__ __forceinline__ void ppo_write_record(int64_t *rec, int next_episode, int finished, int status, int64_t n_actn, int64_t n_testn,
                                                 int64_t n_test_ep, int64_t time_step, int n_rows, int train_steps, int test_steps, int episodes_run,
                                                 int learn_calls, const double *pows, const float *std_old)
{
    rec[0] = next_episode; rec[1] = finished; rec[2] = status;
    rec[3] = n_actn; rec[4] = n_testn; rec[5] = n_test_ep; rec[6] = time_step; rec[7] = n_rows;
    rec[8] = train_steps; rec[9] = test_steps; rec[10] = episodes_run; rec[11] = learn_calls;
    for (int i = 0; i < 2; ++i) rec[12 + i] = __double_as_longlong(pows[i]);
    for (int i = 0; i < PP_STD; ++i) rec[14 + i] = (int64_t)__float_as_uint(std_old[i]);
    for (int w = 14 + PP_STD; w < LENV_PPO_RESUME_WORDS; ++w) rec[w] = 0;
}
static_assert(14 + PP_STD <= LENV_PPO_RESUME_WORDS, "the record holds the counters, two Adam powers and actor_old's action_std");

#define PPO_RN_KERNEL ppo_rn_inner_kernel
#define PPO_RN_SEG false
#define PPO_RN_ICM false
#include "ppo_rn_inner_kernel.inc"
#undef PPO_RN_KERNEL
#undef PPO_RN_SEG
#define PPO_RN_KERNEL ppo_rn_segment_kernel
#define PPO_RN_SEG true
#include "ppo_rn_inner_kernel.inc"
#undef PPO_RN_KERNEL
#undef PPO_RN_ICM
#define PPO_RN_KERNEL ppo_icm_segment_kernel
#define PPO_RN_ICM true
#include "ppo_rn_inner_kernel.inc"
#undef PPO_RN_KERNEL
#undef PPO_RN_SEG
#undef PPO_RN_ICM

}  // namespace lenv

using namespace lenv;

static int64_t ppo_rows_of(const lenv_ppo_cfg *cfg)
{
    const int k = cfg->same_action_num > 1 ? cfg->same_action_num : 1;
    if (cfg->max_steps < 1 || !(cfg->update_episodes >= 0.0) || cfg->update_episodes * (double)cfg->max_steps / (double)k > 1e7) return LENV_ERR_UNSUPPORTED;
    // the first n with n * k / max_steps > update_episodes, the reference's own float comparison (PPO.py:100)
    int64_t n = (int64_t)(cfg->update_episodes * (double)cfg->max_steps / (double)k);
    while (n > 1 && (double)((n - 1) * k) / (double)cfg->max_steps > cfg->update_episodes) --n;
    if (n < 1) n = 1;
    while (!((double)(n * k) / (double)cfg->max_steps > cfg->update_episodes)) ++n;
    return n;
}

// icm_F > 0: the layout of lenv_ppo_icm_* (the ICM-less arena, then the next-observation rows and the module's buffers for N rows)
static int ppo_layout(const lenv_ppo_cfg *cfg, PpoArgs &a, size_t *lds_bytes, int icm_F = 0, int icm_H = 0)
{
    const int H = cfg->hidden, L = cfg->layers, T = cfg->test_episodes, Hrn = cfg->rn_hidden;
    const int S = cfg->state_dim, A = cfg->action_dim;
    if (!((cfg->env_id == LENV_ENV_CHEETAH_STANDIN && S == 17 && A == 6) || (cfg->env_id == LENV_ENV_PENDULUM && S == 3 && A == 1) ||
          (cfg->env_id == LENV_ENV_CMC && S == 2 && A == 1)))
        return LENV_ERR_UNSUPPORTED;
    if (cfg->same_action_num < 0 || cfg->same_action_num > 64) return LENV_ERR_UNSUPPORTED;
    const int t = cfg->reward_env_type;
    if (!((t >= 0 && t <= 8) || t == 101 || t == 102)) return LENV_ERR_UNSUPPORTED;          // reward_env.py:49,58 NotImplementedError
    if (cfg->act == LENV_ACT_PRELU || cfg->act < 0 || cfg->act > LENV_ACT_PRELU) return LENV_ERR_UNSUPPORTED;   // a trained PReLU slope is not a parameter here
    const bool uses_info = t == 3 || t == 4 || t == 7 || t == 8 || t > 100;
    if (uses_info && cfg->info_dim != 4) return LENV_ERR_INVALID;                              // the stand-in's info vector has 4 entries
    if (uses_info && cfg->env_id != LENV_ENV_CHEETAH_STANDIN) return LENV_ERR_INVALID;         // the classic-control steps return an empty info dict
    if (L < 1 || L > PP_MAXL || H < 1 || H > PP_MAXW || T < 1 || T > PP_MAXT || cfg->rn_layers < 1 || cfg->rn_layers > 3 || Hrn < 1 || Hrn > 512 ||
        cfg->max_steps < 1 || cfg->train_episodes < 0 || cfg->ppo_epochs < 0 || cfg->reserved != 0)
        return LENV_ERR_UNSUPPORTED;
    const int64_t N = ppo_rows_of(cfg);
    if (N < 0) return (int)N;
    if (N < 2 || N > PP_MAXN) return LENV_ERR_UNSUPPORTED;                                     // (one row: the unbiased std of the returns is NaN)
    a.N = (int)N;
    PpoMlp ma, mc;
    ppo_mlp(ma, S, H, L, A);
    ppo_mlp(mc, S, H, L, 1);
    a.Pa = ma.P; a.Pc = mc.P; a.P = A + ma.P + mc.P;
    a.oA = PP_STD; a.oC = a.oA + ((ma.P + 3) & ~3); a.PP = a.oC + ((mc.P + 3) & ~3);
    a.P_rn = (int)lenv_rn_num_params(t, S, cfg->info_dim, Hrn, cfg->rn_layers);
    a.P_rn_lds = rn_theta_in_lds(t, cfg->rn_layers) ? a.P_rn : 0;             // deeper reward nets are staged in the arena
    lenv_host::ArenaCursor c;
    a.a_params = c.take(a.PP); a.a_m = c.take(a.PP); a.a_v = c.take(a.PP); a.a_grad = c.take(a.PP);
    a.a_x = c.take(N * S); a.a_act = c.take(N * A); a.a_rew = c.take(N); a.a_done = c.take(N); a.a_ret = c.take(N); a.a_oldlp = c.take(N);
    a.a_mean = c.take(N * A); a.a_val = c.take(N); a.a_dz = c.take(N * A); a.a_gs = c.take(N * A); a.a_dv = c.take(N);
    for (int l = 0; l < PP_MAXL; ++l) { a.a_ha[l] = c.take(l < L ? N * H : 0); a.a_hc[l] = c.take(l < L ? N * H : 0); }
    a.a_d[0] = c.take(N * H); a.a_d[1] = c.take(N * H);
    a.a_meter = c.take(2 * (int64_t)(cfg->train_episodes > 0 ? cfg->train_episodes : 1));
    a.a_rn = c.take(rn_theta_in_lds(t, cfg->rn_layers) ? 0 : a.P_rn);
    a.icm_F = icm_F; a.icm_H = icm_H; a.P_icm = 0; a.a_xn = 0;
    for (int i = 0; i < IB_COUNT; ++i) a.a_icm[i] = 0;
    if (icm_F > 0) {
        IcmNet n;
        icm_build(n, S, A, icm_F, icm_H, /*discrete=*/false);
        a.P_icm = n.P;
        a.a_xn = c.take(N * S);
        int64_t sz[IB_COUNT];
        icm_buffer_sizes(n, (int)N, sz);
        for (int i = 0; i < IB_COUNT; ++i) a.a_icm[i] = c.take(sz[i]);
    }
    a.arena_stride = c.total();
    const size_t lds_floats = GemmShape<PP_MAXI>::PS_FLOATS + GemmShape<PP_MAXI>::QS_FLOATS + GEMM_QUEUE_MAX * sizeof(GemmCmd) / sizeof(float) +
                              ((a.P_rn_lds + 3) & ~3) + 2 * ((Hrn + 3) & ~3) + 2 * PP_MAXW + 64 + 48 + 20 + 20 + 8 + 8 + 64 + 2 + 2 * (20 + 20 + PP_MAXT) + 16;
    *lds_bytes = lds_floats * sizeof(float);
    if (*lds_bytes > 160 * 1024) return LENV_ERR_UNSUPPORTED;
    return LENV_OK;
}
static_assert(2 * PP_MAXN <= GemmShape<PP_MAXI>::PS_FLOATS, "the returns scan keeps rewards and done flags of PP_MAXN rows in the staging buffer");

extern "C" int64_t lenv_ppo_rows(const lenv_ppo_cfg *cfg)
{
    if (!cfg) return LENV_ERR_INVALID;
    PpoArgs a;
    size_t lds;
    const int rc = ppo_layout(cfg, a, &lds);
    return rc != LENV_OK ? rc : a.N;
}

extern "C" int64_t lenv_ppo_num_params(const lenv_ppo_cfg *cfg, int64_t *actor_params, int64_t *critic_params)
{
    if (!cfg) return LENV_ERR_INVALID;
    PpoArgs a;
    size_t lds;
    const int rc = ppo_layout(cfg, a, &lds);
    if (rc != LENV_OK) return rc;
    if (actor_params) *actor_params = a.Pa;
    if (critic_params) *critic_params = a.Pc;
    return a.P;
}

extern "C" int64_t lenv_ppo_rn_num_params(const lenv_ppo_cfg *cfg)
{
    if (!cfg) return LENV_ERR_INVALID;
    PpoArgs a;
    size_t lds;
    const int rc = ppo_layout(cfg, a, &lds);
    return rc != LENV_OK ? rc : a.P_rn;
}

extern "C" int64_t lenv_ppo_rn_lds_bytes(const lenv_ppo_cfg *cfg)
{
    if (!cfg) return LENV_ERR_INVALID;
    PpoArgs a;
    size_t lds;
    const int rc = ppo_layout(cfg, a, &lds);
    return rc != LENV_OK ? rc : (int64_t)lds;
}

extern "C" int64_t lenv_ppo_rn_workspace_bytes(const lenv_ppo_cfg *cfg, int64_t chains)
{
    if (!cfg || chains < 0) return LENV_ERR_INVALID;
    PpoArgs a;
    size_t lds;
    const int rc = ppo_layout(cfg, a, &lds);
    if (rc != LENV_OK) return rc;
    return chains * a.arena_stride * (int64_t)sizeof(float) + 256;
}

// the launch behind lenv_ppo_rn_inner_loop (segment false: one launch from the first episode to the final test, resume unused) and
// lenv_ppo_rn_inner_loop_segment (segment true: episodes [ep_begin, ep_end) on ppo_rn_segment_kernel)
static int ppo_launch(const lenv_ppo_cfg *cfg, const float *theta, const float *eps, const int32_t *worker, const float *sign,
                      const float *agent_init, const uint64_t *rng_keys, const lenv_ppo_tapes *tapes, int64_t chains, void *workspace,
                      size_t workspace_bytes, const lenv_ppo_out *out, bool segment, int32_t ep_begin, int32_t ep_end, int64_t *resume, void *stream)
{
    const lenv_host::Segment seg{segment, ep_begin, ep_end, resume};
    if (!lenv_host::launch_args_ok(cfg, nullptr, eps, worker, sign, agent_init, rng_keys, tapes, chains, workspace, out, seg)) return LENV_ERR_INVALID;
    if (!theta && cfg->reward_env_type != 0) return LENV_ERR_INVALID;
    if (cfg->rng_mode == LENV_RNG_TAPE && (!tapes->act_noise || !tapes->test_noise || !tapes->train_reset || !tapes->test_reset)) return LENV_ERR_INVALID;
    if (cfg->rng_mode != LENV_RNG_COUNTER && cfg->rng_mode != LENV_RNG_TAPE) return LENV_ERR_INVALID;
    if (out->trace_reward && out->trace_cap > 0 && (!out->trace_action || !out->trace_state || !out->trace_next_state)) return LENV_ERR_INVALID;
    PpoArgs a;                    // (the layout runs before the chains == 0 return here: an unsupported cfg is refused with zero chains too)
    size_t lds_bytes;
    const int rc = ppo_layout(cfg, a, &lds_bytes);
    if (rc != LENV_OK) return rc;
    if (chains == 0) return LENV_OK;
    if (workspace_bytes < (size_t)chains * a.arena_stride * sizeof(float)) return LENV_ERR_WORKSPACE;
    lenv_host::fill_args(a, cfg, theta, eps, worker, sign, agent_init, rng_keys, tapes, workspace, out);
    lenv_host::fill_segment(a, cfg, seg);
    if (a.out.trace_cap <= 0) a.out.trace_reward = nullptr;
    if (a.out.learn_cap <= 0) a.out.learn_step = nullptr;
    void (*kern)(const PpoArgs) = cfg->env_id == LENV_ENV_PENDULUM ? ppo_rn_inner_kernel<LENV_ENV_PENDULUM>
                                  : (cfg->env_id == LENV_ENV_CMC ? ppo_rn_inner_kernel<LENV_ENV_CMC> : ppo_rn_inner_kernel<LENV_ENV_CHEETAH_STANDIN>);
    if (segment)
        kern = cfg->env_id == LENV_ENV_PENDULUM ? ppo_rn_segment_kernel<LENV_ENV_PENDULUM>
               : (cfg->env_id == LENV_ENV_CMC ? ppo_rn_segment_kernel<LENV_ENV_CMC> : ppo_rn_segment_kernel<LENV_ENV_CHEETAH_STANDIN>);
    return lenv_host::launch(kern, dim3((unsigned)chains), dim3(DNT), lds_bytes, stream, a);
}

extern "C" int lenv_ppo_rn_inner_loop(const lenv_ppo_cfg *cfg, const float *theta, const float *eps, const int32_t *worker, const float *sign,
                                      const float *agent_init, const uint64_t *rng_keys, const lenv_ppo_tapes *tapes, int64_t chains,
                                      void *workspace, size_t workspace_bytes, const lenv_ppo_out *out, void *stream)
{
    return ppo_launch(cfg, theta, eps, worker, sign, agent_init, rng_keys, tapes, chains, workspace, workspace_bytes, out, false, 0, 0, nullptr, stream);
}

extern "C" int lenv_ppo_rn_inner_loop_segment(const lenv_ppo_cfg *cfg, const float *theta, const float *eps, const int32_t *worker, const float *sign,
                                              const float *agent_init, const uint64_t *rng_keys, const lenv_ppo_tapes *tapes, int64_t chains,
                                              void *workspace, size_t workspace_bytes, const lenv_ppo_out *out, int32_t episode_begin,
                                              int32_t episode_end, int64_t *resume, void *stream)
{
    return ppo_launch(cfg, theta, eps, worker, sign, agent_init, rng_keys, tapes, chains, workspace, workspace_bytes, out, true, episode_begin,
                      episode_end, resume, stream);
}

// ---- PPO(icm=True): lenv_ppo_icm_* (ppo_icm_segment_kernel behind both launch entries) ----

static int ppo_icm_layout(const lenv_ppo_cfg *cfg, int32_t F, int32_t H, PpoArgs &a, size_t *lds_bytes)
{
    if (F < 1 || F > 128 || H < 1 || H > 128) return LENV_ERR_UNSUPPORTED;
    return ppo_layout(cfg, a, lds_bytes, F, H);
}

extern "C" int64_t lenv_ppo_icm_num_params(const lenv_ppo_cfg *cfg, int32_t icm_feature_dim, int32_t icm_hidden)
{
    if (!cfg) return LENV_ERR_INVALID;
    PpoArgs a;
    size_t lds;
    const int rc = ppo_icm_layout(cfg, icm_feature_dim, icm_hidden, a, &lds);
    return rc != LENV_OK ? rc : a.P_icm;
}

// the chains' arenas, then (256-byte aligned: the stride is a multiple of 64 floats) the resume records of the single-launch entry
extern "C" int64_t lenv_ppo_icm_workspace_bytes(const lenv_ppo_cfg *cfg, int32_t icm_feature_dim, int32_t icm_hidden, int64_t chains)
{
    if (!cfg || chains < 0) return LENV_ERR_INVALID;
    PpoArgs a;
    size_t lds;
    const int rc = ppo_icm_layout(cfg, icm_feature_dim, icm_hidden, a, &lds);
    if (rc != LENV_OK) return rc;
    return chains * a.arena_stride * (int64_t)sizeof(float) + chains * LENV_PPO_RESUME_WORDS * (int64_t)sizeof(int64_t) + 256;
}

// segment false: episodes [0, train_episodes) in one launch, the records in the workspace behind the arenas
static int ppo_icm_launch(const lenv_ppo_cfg *cfg, int32_t F, int32_t H, double icm_lr, double icm_beta, double icm_eta, const lenv_icm_io *icm,
                          const float *theta, const float *eps, const int32_t *worker, const float *sign, const float *agent_init,
                          const uint64_t *rng_keys, const lenv_ppo_tapes *tapes, int64_t chains, void *workspace, size_t workspace_bytes,
                          const lenv_ppo_out *out, bool segment, int32_t ep_begin, int32_t ep_end, int64_t *resume, void *stream)
{
    const lenv_host::Segment seg{segment, ep_begin, ep_end, resume};
    if (!lenv_host::launch_args_ok(cfg, nullptr, eps, worker, sign, agent_init, rng_keys, tapes, chains, workspace, out, seg)) return LENV_ERR_INVALID;
    if (!icm || !icm->icm_init) return LENV_ERR_INVALID;
    if (!theta && cfg->reward_env_type != 0) return LENV_ERR_INVALID;
    if (cfg->rng_mode == LENV_RNG_TAPE && (!tapes->act_noise || !tapes->test_noise || !tapes->train_reset || !tapes->test_reset)) return LENV_ERR_INVALID;
    if (cfg->rng_mode != LENV_RNG_COUNTER && cfg->rng_mode != LENV_RNG_TAPE) return LENV_ERR_INVALID;
    if (out->trace_reward && out->trace_cap > 0 && (!out->trace_action || !out->trace_state || !out->trace_next_state)) return LENV_ERR_INVALID;
    PpoArgs a;
    size_t lds_bytes;
    const int rc = ppo_icm_layout(cfg, F, H, a, &lds_bytes);
    if (rc != LENV_OK) return rc;
    if (chains == 0) return LENV_OK;
    const size_t arena_bytes = (size_t)chains * a.arena_stride * sizeof(float);
    if (workspace_bytes < arena_bytes + (segment ? 0 : (size_t)chains * LENV_PPO_RESUME_WORDS * sizeof(int64_t))) return LENV_ERR_WORKSPACE;
    lenv_host::fill_args(a, cfg, theta, eps, worker, sign, agent_init, rng_keys, tapes, workspace, out);
    lenv_host::fill_segment(a, cfg, seg);
    if (!segment) a.resume = reinterpret_cast<int64_t *>(static_cast<char *>(workspace) + arena_bytes);
    a.icm_lr = icm_lr; a.icm_beta = icm_beta; a.icm_eta = icm_eta; a.icm_init = icm->icm_init; a.icm_final = icm->icm_final;
    if (a.out.trace_cap <= 0) a.out.trace_reward = nullptr;
    if (a.out.learn_cap <= 0) a.out.learn_step = nullptr;
    void (*kern)(const PpoArgs) = cfg->env_id == LENV_ENV_PENDULUM ? ppo_icm_segment_kernel<LENV_ENV_PENDULUM>
                                  : (cfg->env_id == LENV_ENV_CMC ? ppo_icm_segment_kernel<LENV_ENV_CMC> : ppo_icm_segment_kernel<LENV_ENV_CHEETAH_STANDIN>);
    return lenv_host::launch(kern, dim3((unsigned)chains), dim3(DNT), lds_bytes, stream, a);
}

extern "C" int lenv_ppo_icm_inner_loop(const lenv_ppo_cfg *cfg, int32_t icm_feature_dim, int32_t icm_hidden, double icm_lr, double icm_beta,
                                       double icm_eta, const lenv_icm_io *icm, const float *theta, const float *eps, const int32_t *worker,
                                       const float *sign, const float *agent_init, const uint64_t *rng_keys, const lenv_ppo_tapes *tapes,
                                       int64_t chains, void *workspace, size_t workspace_bytes, const lenv_ppo_out *out, void *stream)
{
    return ppo_icm_launch(cfg, icm_feature_dim, icm_hidden, icm_lr, icm_beta, icm_eta, icm, theta, eps, worker, sign, agent_init, rng_keys, tapes,
                          chains, workspace, workspace_bytes, out, false, 0, 0, nullptr, stream);
}

extern "C" int lenv_ppo_icm_inner_loop_segment(const lenv_ppo_cfg *cfg, int32_t icm_feature_dim, int32_t icm_hidden, double icm_lr,
                                               double icm_beta, double icm_eta, const lenv_icm_io *icm, const float *theta, const float *eps,
                                               const int32_t *worker, const float *sign, const float *agent_init, const uint64_t *rng_keys,
                                               const lenv_ppo_tapes *tapes, int64_t chains, void *workspace, size_t workspace_bytes,
                                               const lenv_ppo_out *out, int32_t episode_begin, int32_t episode_end, int64_t *resume, void *stream)
{
    return ppo_icm_launch(cfg, icm_feature_dim, icm_hidden, icm_lr, icm_beta, icm_eta, icm, theta, eps, worker, sign, agent_init, rng_keys, tapes,
                          chains, workspace, workspace_bytes, out, true, episode_begin, episode_end, resume, stream);
}
