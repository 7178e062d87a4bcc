// td3_rn_inner_loop.hip -- fused NES inner loop for config 5: a TD3 agent trained on a RewardEnv (learned potential shaping
// around a continuous-state real env), one 512-thread workgroup per chain.
//
// Replaces GTN_Worker.calc_score (agents/GTN_worker.py:187-221) with
//   TD3.learn / select_train_action / select_test_action   agents/TD3.py:63-135
//   Actor_TD3, Critic_Q                                      models/actor_critic.py:11-19,64-71
//   BaseAgent.train / test, ReplayBuffer                     agents/base_agent.py:64-227, utils.py:9-72
//   EnvWrapper.step (real branch) -> RewardEnv.step          envs/env_wrapper.py:49-70, envs/reward_env.py:61-133
//   real env: the documented HalfCheetah-v3 STAND-IN (tools/gen_cheetah_standin.py; MuJoCo cannot exist on either box)
//
// Same structure as the DuelingDDQN kernel: actor + twin critics + their targets + Adam state (59 016 parameters x5 at the
// config-5 shapes) live in a per-chain HBM arena; every layer product is the canonical-order workgroup GEMM of
// lenv_gemm.cuh (batch 192 = two row blocks); the reward network (17-128-1) is staged in LDS and evaluated once per env
// step (phi(s') of step t is phi(s) of step t+1).  Gaussian noises come from RNG tapes (parity mode) or from the
// counter RNG through a Box-Muller with deterministic log / cos (production mode).
#include "lenv_gemm.cuh"

#include <type_traits>
#include "lenv_ln.cuh"
#include "lenv_icm.cuh"
#include "lenv_wavechain_host.h"
#include "lenv_host.h"
#include "lenv_actor_params.cuh"      // T3_MAXL, T3_MAXW, MlpOff / mlp_off

namespace lenv {

constexpr int T3_MAXB = 768;   // max batch size  (more than 256 rows run as several row blocks; 768 = 3 x the shipped 256)
constexpr int T3_MAXI = 256;   // rows of one product block
constexpr int T3_DIRECT_H = 64, T3_DIRECT_B = 256;   // the DIRECT instantiations: one hidden layer of at most 64 units, batch <= 256 (see the kernel)
// observation / action dims come from the env (ContEnv<ENV> in lenv_device.cuh): the stand-in 17 / 6, Pendulum-v0 3 / 1

struct Td3Args {
    lenv_td3_cfg cfg;
    const float *theta, *eps; const int32_t *worker; const float *sign;
    const float *agent_init; const uint64_t *rng_keys;
    lenv_td3_tapes tapes;
    float *arena; int64_t arena_stride;
    lenv_td3_out out;
    int64_t rb_cap; int RS;
    MlpOff actor, critic;                     // at cfg's (maximal) shapes
    int P, P_rn;                              // P = row stride of agent_init / final_params; P_rn = parameters of theta
    int P_rn_lds;                             // floats of theta staged in LDS (RewardEnv); a VirtualEnv's three nets live in the arena
    int64_t a_se, a_xse, a_nse;               // VirtualEnv: perturbed SE parameters, its input cat(action, state), its outputs [S + 2]
    int64_t a_seT;                            // ... and a copy with every weight matrix TRANSPOSED ([in][out]: the one-row products read it coalesced)
    // per-chain hyper-parameters (device arrays [chains], all or none): TD3_vary (agents/TD3_vary.py:24-58)
    const double *hp_lr; const int32_t *hp_batch, *hp_hidden, *hp_layers;
    // TD3(icm=True) (agents/TD3.py:44-60,68-70): fresh ICM parameters per chain, optional final parameters, arena offsets
    const float *icm_init; float *icm_final; int P_icm;
    int64_t a_icm[IB_COUNT];
    int64_t a_params, a_targets, a_m, a_v, a_grad, a_replay, a_xc, a_xn, a_xa, a_hc1[T3_MAXL], a_hc2[T3_MAXL], a_ha[T3_MAXL],
        a_ht[T3_MAXL], a_d[2], a_dx, a_act, a_th, a_dz, a_meter, a_xh[3][T3_MAXL], a_rstd;      // a_xh / a_rstd: LayerNorm rows of critic_1 / critic_2 / actor passes
    // lenv_td3_rn_inner_loop_segment (the SEG instantiations): episodes [ep_begin, ep_end) of every chain, resume records [chains, LENV_TD3_RESUME_WORDS];
    // every other entry point: 0, train_episodes, nullptr.  (Behind everything else: the other instantiations read their arguments where they were.)
    int ep_begin, ep_end; int64_t *resume;
};

// Diagnostic build only (-DLENV_PHASE_TIMING): per-phase shader-clock totals of chain 0, never in the shipped library.
#ifdef LENV_PHASE_TIMING
__device__ unsigned long long g_td3_phase_cycles[16];
__device__ unsigned long long g_t3d_sub_cycles[16];      // sub-phases of t3_direct_critics (thread 0 of chain 0)
#define T3D_SUB_DECL unsigned long long sb_last = __builtin_readcyclecounter()
#define T3D_SUB(i) do { unsigned long long sb_now = __builtin_readcyclecounter(); if (blockIdx.x == 0 && threadIdx.x == 0) g_t3d_sub_cycles[i] += sb_now - sb_last; sb_last = sb_now; } while (0)
#define T3D_ENV_SUB(i) do { unsigned long long sb_now = __builtin_readcyclecounter(); if (blockIdx.x == 0 && threadIdx.x == 0) g_t3d_sub_cycles[i] += sb_now - pt_last; } while (0)
#define PT_DECL unsigned long long pt_last = __builtin_readcyclecounter(), pt_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define PT_MARK(i) do { unsigned long long pt_now = __builtin_readcyclecounter(); pt_acc[i] += pt_now - pt_last; pt_last = pt_now; } while (0)
#else
#define PT_DECL
#define PT_MARK(i)
#define T3D_SUB_DECL
#define T3D_SUB(i)
#define T3D_ENV_SUB(i)
#endif

// SHAPE 1 = the published HalfCheetah RewardEnv + TD3 configuration (default_config_halfcheetah_reward_env.yaml = BASELINE
// configs[4]: actor 17-128-128-6 / twin critics 23-128-128-1 relu, batch 192, policy_delay 1, reward net 17-128-1 prelu of type 2,
// one test episode) in production form (counter RNG, no step trace, no per-chain hyper-parameters, no ICM): dimensions and mode
// switches are literals (see the DuelingDDQN kernel for what that buys).
struct Td3Shape { int env, H, L, B, T, Hrn, rn_layers, rn_act, rtype, act, policy_delay, virtual_env, k_rep; };
constexpr Td3Shape kTd3Shapes[] = {
    { -1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 0, 1 },                                                                                          // 0: generic (unused entry)
    { LENV_ENV_CHEETAH_STANDIN, 128, 2, 192, 1, 128, 1, LENV_ACT_PRELU, 2, LENV_ACT_RELU, 1, 0, 1 },      // 1: default_config_halfcheetah_reward_env.yaml = BASELINE configs[4]
    { LENV_ENV_PENDULUM, 128, 2, 192, 10, 128, 2, LENV_ACT_PRELU, 2, LENV_ACT_LEAKYRELU, 1, 0, 1 },       // 2: default_config_pendulum_reward_env.yaml
    { LENV_ENV_CMC, 128, 2, 256, 1, 96, 2, LENV_ACT_LEAKYRELU, 0, LENV_ACT_RELU, 2, 1, 2 },               // 3: default_config_cmc.yaml (VirtualEnv, same_action_num 2)
    { LENV_ENV_CMC, 128, 2, 192, 1, 128, 1, LENV_ACT_TANH, 2, LENV_ACT_LEAKYRELU, 1, 0, 2 },              // 4: default_config_cmc_reward_env.yaml
};

// ---- the DIRECT learn step (see the comment in front of the kernel): out-of-line routines with their own register allocation -- inlined into the
// kernel body they drowned in its scalar-register spills (3 000 v_readlane in the instantiation, 15-25 k cycles per forward pass) ----
struct T3DirectCtx {                           // in LDS, written by thread 0 before every learn step, re-read by the routines
    float *params, *targets, *grad, *xc, *xn;               // the chain's arena
    float *l_act, *l_x, *l_na, *l_w;                         // LDS work areas (t3d_layout): activations [H][257], rows [B][SA], actions [B][A], two staged nets
    float *rr, *dd, *q1, *q2, *tq1, *tq2, *dq1, *dq2;        // LDS vectors [B]
    const float *policy_noise; int64_t policy_noise_rows;    // the chain's tape rows (null: counter RNG)
    uint64_t key;
    int H, B, act_id, Pa, Pc;
    float prelu, ma, g32, policy_std, policy_clip;
};

// LDS work areas of the DIRECT learn step (floats from the start of the product queue's staging buffers), one definition for host and kernel:
// the activation matrix is UNIT-MAJOR, [H][T3D_BP] with T3D_BP = 257: sample b writes h[j] at j * 257 + b (lanes = samples: consecutive banks), the
// reduction for unit j walks its row at consecutive addresses (lanes = units: 257 = 1 mod 32 banks apart) -- every offset inside a block of units /
// samples is an immediate of the ds instruction, whatever H is.  Staged nets start at multiples of four floats (ds_read_b128 of eight units' weights).
constexpr int T3D_BP = T3_DIRECT_B + 1;
struct T3DirectLayout { int x, na, w, w2_actor, w2_critic, ctx, total; };
__host__ __device__ inline T3DirectLayout t3d_layout(int S, int A, int H, int B)
{
    const int SA = S + A, Pa = S * H + H + A * H + A, Pc = SA * H + H + H + 1, PaA = (Pa + 3) & ~3, PcA = (Pc + 3) & ~3;
    T3DirectLayout l;
    l.x = H * T3D_BP; l.na = l.x + B * SA; l.w = (l.na + B * A + 3) & ~3;
    l.w2_actor = PaA; l.w2_critic = PcA;                                   // second staged net: behind the actor / behind a critic
    l.ctx = l.w + 2 * (PaA > PcA ? PaA : PcA);
    l.total = l.ctx + (int)((sizeof(T3DirectCtx) + 3) / 4) + 4;
    return l;
}

typedef float t3d_f4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const t3d_f4 t3d_lf4;
template <int N> __device__ __forceinline__ void t3d_ld4(const lfloat *p, float (&d)[N])     // N floats from a 16-byte aligned LDS address
{
    static_assert(N % 4 == 0, "whole float4s");
    t3d_lf4 *q = (t3d_lf4 *)p;
#pragma unroll
    for (int i = 0; i < N / 4; ++i) { const t3d_f4 v = q[i]; d[4 * i] = v.x; d[4 * i + 1] = v.y; d[4 * i + 2] = v.z; d[4 * i + 3] = v.w; }
}

// one sample through hidden units [j_lo, j_hi) of a one-hidden-layer net whose state-dict-order parameters sit in LDS at w (wave-uniform
// addresses: broadcast reads): the output chains continue in acc (j ascending), the hidden activations go (STORE) to the sample's column of the
// activation matrix.  Units in blocks: a block's weights are requested before its first fmaf.  FAST (H a multiple of eight, w 16-byte aligned,
// j_lo / j_hi multiples of eight): eight units' weights are 2 IN + 2 + 2 OUT ds_read_b128 and no guard; otherwise clamped scalar reads + a guard
// per unit (the run-time switch over the activation, six scalar branches per unit, cost 35 k cycles per pass: ACT is a template parameter).
// (STORE, not a null test of hcol: the activation matrix starts at LDS address 0, which IS the null pointer of address space 3 in an icmp --
// sample 0's activations were silently skipped)
template <int ACT, int IN, int OUT, bool STORE, bool NEED_O, bool FAST>
__device__ __forceinline__ void t3d_net_fwd_range(const lfloat *w, int H, float prelu, const float (&xr)[IN], lfloat *hcol, float (&acc)[OUT], int j_lo, int j_hi)
{
    constexpr int JB = IN <= 8 ? 8 : 4, NO = NEED_O ? OUT : 1;
    const lfloat *W0 = w, *b0 = w + H * IN, *Wo = b0 + H;
#pragma unroll 1
    for (int j0 = j_lo; j0 < j_hi; j0 += JB) {
        float w0[JB * IN], bv[JB], wo[NO][JB];
        if constexpr (FAST) {
            t3d_ld4<JB * IN>(W0 + j0 * IN, w0);
            t3d_ld4<JB>(b0 + j0, bv);
            if constexpr (NEED_O) {
#pragma unroll
                for (int c = 0; c < OUT; ++c) t3d_ld4<JB>(Wo + c * H + j0, wo[c]);
            }
        } else {
#pragma unroll
            for (int u = 0; u < JB; ++u) {
                const int j = j0 + u < j_hi ? j0 + u : j_hi - 1;      // (clamped reads past the last unit, unused)
#pragma unroll
                for (int k = 0; k < IN; ++k) w0[u * IN + k] = W0[j * IN + k];
                bv[u] = b0[j];
                if constexpr (NEED_O) {
#pragma unroll
                    for (int c = 0; c < OUT; ++c) wo[c][u] = Wo[c * H + j];
                }
            }
        }
        lfloat *hc = hcol + j0 * T3D_BP;
#pragma unroll
        for (int u = 0; u < JB; ++u) {
            if (FAST || j0 + u < j_hi) {
                float z = 0.0f;
#pragma unroll
                for (int k = 0; k < IN; ++k) z = fma32(xr[k], w0[u * IN + k], z);
                z = z + bv[u];
                const float hj = act_fwd(ACT, prelu, z);
                if constexpr (STORE) hc[u * T3D_BP] = hj;
                if constexpr (NEED_O) {
#pragma unroll
                    for (int c = 0; c < OUT; ++c) acc[c] = fma32(hj, wo[c][u], acc[c]);
                }
            }
        }
    }
}
template <int ACT, int IN, int OUT, bool STORE, bool NEED_O>
__device__ __forceinline__ void t3d_net_fwd(const lfloat *w, int H, float prelu, const float (&xr)[IN], lfloat *hcol, float (&o)[OUT], int j_lo, int j_hi)
{
    float acc[OUT];
#pragma unroll
    for (int c = 0; c < OUT; ++c) acc[c] = 0.0f;
    if ((H & 7) == 0) t3d_net_fwd_range<ACT, IN, OUT, STORE, NEED_O, true>(w, H, prelu, xr, hcol, acc, j_lo, j_hi);
    else t3d_net_fwd_range<ACT, IN, OUT, STORE, NEED_O, false>(w, H, prelu, xr, hcol, acc, j_lo, j_hi);
    if constexpr (NEED_O) {
        const lfloat *bo = w + H * IN + H + OUT * H;
#pragma unroll
        for (int c = 0; c < OUT; ++c) o[c] = acc[c] + bo[c];
    }
}
// the hidden gradient in place, units [j_lo, j_hi) of one sample's column: h[j] <- act'(h[j]) * sum_c g[c] Wo[c][j]  (c ascending from +0: the
// queued product's k-chain; one output = its single k-step fma(dq, W, +0))
template <int ACT, int NC, bool FAST>
__device__ __forceinline__ void t3d_dz_range(lfloat *hcol, const lfloat *Wo, int H, float prelu, const float (&g)[NC], int j_lo, int j_hi)
{
#pragma unroll 1
    for (int j0 = j_lo; j0 < j_hi; j0 += 8) {
        float hv[8], wo[NC][8];
        lfloat *hc = hcol + j0 * T3D_BP;
        if constexpr (FAST) {
#pragma unroll
            for (int u = 0; u < 8; ++u) hv[u] = hc[u * T3D_BP];
#pragma unroll
            for (int c = 0; c < NC; ++c) t3d_ld4<8>(Wo + c * H + j0, wo[c]);
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 + u < j_hi ? j0 + u : j_hi - 1;
                hv[u] = hcol[j * T3D_BP];
#pragma unroll
                for (int c = 0; c < NC; ++c) wo[c][u] = Wo[c * H + j];
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (FAST || j0 + u < j_hi) {
                float acc = 0.0f;
#pragma unroll
                for (int c = 0; c < NC; ++c) acc = fma32(g[c], wo[c][u], acc);
                hc[u * T3D_BP] = act_bwd(ACT, prelu, hv[u], acc);
            }
        }
    }
}
template <int ACT, int NC>
__device__ __forceinline__ void t3d_dz(lfloat *hcol, const lfloat *Wo, int H, float prelu, const float (&g)[NC], int j_lo, int j_hi)
{
    if ((H & 7) == 0) t3d_dz_range<ACT, NC, true>(hcol, Wo, H, prelu, g, j_lo, j_hi);
    else t3d_dz_range<ACT, NC, false>(hcol, Wo, H, prelu, g, j_lo, j_hi);
}
__device__ __forceinline__ int t3d_split(int H) { return (H & 7) == 0 ? (((H >> 3) + 1) >> 1) << 3 : (H + 1) >> 1; }     // units [0, split) to half 0, the rest to half 1

// sum_{i < B} p[i * SP] * q[i * SQ] as ONE i-ascending chain from 0 (both operands in LDS; strides are literals: immediates), the next eight
// pairs requested before the current eight are consumed
template <int SP, int SQ>
__device__ __forceinline__ float t3d_batch_dot(const lfloat *pp, const lfloat *qq, int B)
{
    // two register blocks of eight pairs, refilled alternately (a "next -> current" copy at the end of an iteration made the compiler wait for
    // the loads it had just issued: 8.5 k cycles per 256-sample chain instead of ~3 k)
    constexpr int U = 8;
    float acc = 0.0f;
    const int nb = B / U;
    int blk = 0;
    float pa[U], qa[U], pb[U], qb[U];
    if (nb > 0) {
#pragma unroll
        for (int u = 0; u < U; ++u) { pa[u] = pp[u * SP]; qa[u] = qq[u * SQ]; }
    }
#pragma unroll 1
    while (blk + 2 <= nb) {                                    // block blk sits in (pa, qa)
        const lfloat *p1 = pp + (blk + 1) * U * SP, *q1 = qq + (blk + 1) * U * SQ;
#pragma unroll
        for (int u = 0; u < U; ++u) { pb[u] = p1[u * SP]; qb[u] = q1[u * SQ]; }
#pragma unroll
        for (int u = 0; u < U; ++u) acc = fma32(pa[u], qa[u], acc);
        if (blk + 2 < nb) {
            const lfloat *p2 = pp + (blk + 2) * U * SP, *q2 = qq + (blk + 2) * U * SQ;
#pragma unroll
            for (int u = 0; u < U; ++u) { pa[u] = p2[u * SP]; qa[u] = q2[u * SQ]; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc = fma32(pb[u], qb[u], acc);
        blk += 2;
    }
    if (blk < nb) {
#pragma unroll
        for (int u = 0; u < U; ++u) acc = fma32(pa[u], qa[u], acc);
        ++blk;
    }
    for (int i = blk * U; i < B; ++i) acc = fma32(pp[i * SP], qq[i * SQ], acc);
    return acc;
}
template <int SP>
__device__ __forceinline__ float t3d_batch_sum(const lfloat *pp, int B)      // plain adds, i ascending (the bias gradients' column sums)
{
    constexpr int U = 16;
    float acc = 0.0f;
    int i = 0;
    for (; i + U <= B; i += U) {
        float pv[U];
        const lfloat *p2 = pp + i * SP;
#pragma unroll
        for (int u = 0; u < U; ++u) pv[u] = p2[u * SP];
#pragma unroll
        for (int u = 0; u < U; ++u) acc = acc + pv[u];
    }
    for (; i < B; ++i) acc = acc + pp[i * SP];
    return acc;
}
__device__ __forceinline__ void t3d_stage(const float *src, int n, lfloat *dst, int tid) { for (int i = tid; i < n; i += DNT) dst[i] = src[i]; }

// TD3.learn up to the critics' gradients (TD3.py:63-95): smoothed target actions, target critics, TD error, both critics' gradients into
// ctx->grad.  Returns non-zero on a policy-noise tape underrun.  Thread b & 255 owns minibatch sample b; half h = tid >> 8 runs critic h
// where the two critics can go side by side, and half of the hidden units where a pass only fills the activation matrix.
template <int S, int A, int ACT>
__device__ __noinline__ int t3_direct_critics(const T3DirectCtx *ctx_, int64_t learn_it_)
{
    constexpr int SA = S + A;
    typedef __attribute__((address_space(3))) const T3DirectCtx LCtx;
    LCtx *c = (LCtx *)uni_ptr(ctx_);
    const int tid = threadIdx.x, half = uni(tid >> 8), b = tid & 255;
    const int H = uni(c->H), B = uni(c->B), Pa = uni(c->Pa), Pc = uni(c->Pc), PcA = (Pc + 3) & ~3;
    const float prelu = unif(c->prelu), ma = unif(c->ma), g32 = unif(c->g32);
    const int64_t learn_it = learn_it_;
    lfloat *l_act = (lfloat *)uni_ptr(c->l_act), *l_x = (lfloat *)uni_ptr(c->l_x), *l_na = (lfloat *)uni_ptr(c->l_na), *l_w = (lfloat *)uni_ptr(c->l_w);
    lfloat *rr = (lfloat *)uni_ptr(c->rr), *dd = (lfloat *)uni_ptr(c->dd), *q1 = (lfloat *)uni_ptr(c->q1), *q2 = (lfloat *)uni_ptr(c->q2);
    lfloat *tq1 = (lfloat *)uni_ptr(c->tq1), *tq2 = (lfloat *)uni_ptr(c->tq2), *dq1 = (lfloat *)uni_ptr(c->dq1), *dq2 = (lfloat *)uni_ptr(c->dq2);
    const float *params = uni_ptr(c->params), *targets = uni_ptr(c->targets), *xc = uni_ptr(c->xc), *xn = uni_ptr(c->xn);
    float *grad = uni_ptr(c->grad);
    const bool live = b < B;
    lfloat *mycol = l_act + b;
    const int Hs = t3d_split(H), my_lo = half ? Hs : 0, my_hi = half ? H : Hs;
    int bad = 0;
    T3D_SUB_DECL;
    // the sample's rows (s, a) and s' from the arena, requested before anything else (their round trip hides behind the first staging)
    float xcr[SA], xnr[S];
#pragma unroll
    for (int k = 0; k < SA; ++k) xcr[k] = live ? xc[b * SA + k] : 0.0f;
#pragma unroll
    for (int k = 0; k < S; ++k) xnr[k] = live ? xn[b * SA + k] : 0.0f;
    // ---- next_actions = (actor_target(s') + clamp(randn * policy_std)).clamp(-max, max)  (TD3.py:72-78) ----
    t3d_stage(targets, Pa, l_w, tid);
    __syncthreads();
    T3D_SUB(0);
    if (half == 0 && live) {
        float o[A];
        t3d_net_fwd<ACT, S, A, false, true>(l_w, H, prelu, xnr, l_w, o, 0, H);
        const float *tape = uni_ptr(c->policy_noise);
        const float pstd = unif(c->policy_std), clipv = unif(c->policy_clip);
        const uint64_t key = c->key;
#pragma unroll
        for (int k = 0; k < A; ++k) {
            const float v0 = det_tanhf(lenv_tanh_table, o[k]) * ma;
            const int64_t n = (learn_it * B + b) * A + k;
            float zn;
            if (tape) { if (n >= c->policy_noise_rows * A) { bad = 1; zn = 0.0f; } else zn = tape[n]; }
            else zn = (float)det_normal(key, STREAM_TD3_POLICY_NOISE, (uint64_t)n);
            float nz = zn * pstd;
            nz = nz < -clipv ? -clipv : (nz > clipv ? clipv : nz);
            const float v = v0 + nz;
            l_na[b * A + k] = v < -ma ? -ma : (v > ma ? ma : v);
        }
    }
    __syncthreads();
    T3D_SUB(1);
    // ---- the target critics on (s', next_actions): half h runs critic h  (TD3.py:80-82) ----
    t3d_stage(targets + Pa, Pc, l_w, tid);
    t3d_stage(targets + Pa + Pc, Pc, l_w + PcA, tid);
    __syncthreads();
    T3D_SUB(2);
    if (live) {
        float xr[SA], o[1];
#pragma unroll
        for (int k = 0; k < S; ++k) xr[k] = xnr[k];
#pragma unroll
        for (int k = 0; k < A; ++k) xr[S + k] = l_na[b * A + k];
        t3d_net_fwd<ACT, SA, 1, false, true>(l_w + half * PcA, H, prelu, xr, l_w, o, 0, H);
        (half ? tq2 : tq1)[b] = o[0];
    }
    __syncthreads();
    T3D_SUB(3);
    // ---- the online critics on (s, a), TD error (TD3.py:84-91): half h runs critic h; critic_1's activations stay in the matrix ----
    t3d_stage(params + Pa, Pc, l_w, tid);
    t3d_stage(params + Pa + Pc, Pc, l_w + PcA, tid);
    __syncthreads();
    T3D_SUB(4);
    if (live) {
        float o[1];
        if (half == 0) {
            t3d_net_fwd<ACT, SA, 1, true, true>(l_w, H, prelu, xcr, mycol, o, 0, H);
            q1[b] = o[0];
#pragma unroll
            for (int k = 0; k < SA; ++k) l_x[b * SA + k] = xcr[k];
        } else {
            t3d_net_fwd<ACT, SA, 1, false, true>(l_w + PcA, H, prelu, xcr, l_w, o, 0, H);
            q2[b] = o[0];
        }
    }
    __syncthreads();
    T3D_SUB(5);
    if (live) {
        const float norm = (float)(2.0 / (double)B);
        const float tq = tq1[b] < tq2[b] ? tq1[b] : tq2[b];
        const float y = rr[b] + ((1.0f - dd[b]) * g32) * tq;       // rewards + (1 - dones) * gamma * target_Q
        if (half == 0) dq1[b] = norm * (q1[b] - y);
        else dq2[b] = norm * (q2[b] - y);
    }
    __syncthreads();
    T3D_SUB(6);
    // ---- critic gradients, one critic after the other through the activation matrix (critic_2's forward pass once more, into the matrix: the
    // two halves fill half of the units each) ----
    const int oW0 = 0, ob0 = H * SA, oWo = ob0 + H, obo = oWo + H;      // state-dict offsets of a one-hidden-layer critic (mlp_off)
#pragma unroll 1
    for (int cc = 0; cc < 2; ++cc) {
        const lfloat *dqv = cc ? dq2 : dq1;
        float *gcr = grad + Pa + cc * Pc;
        const lfloat *wcc = l_w + cc * PcA;
        if (cc == 1) {
            if (live) { float o[1]; t3d_net_fwd<ACT, SA, 1, true, false>(wcc, H, prelu, xcr, mycol, o, my_lo, my_hi); }
            __syncthreads();
        }
        T3D_SUB(7);
        // output layer: gWout[j] = sum_i dq[i] h[i][j], gbout = sum_i dq[i]
        if (tid < H) gcr[oWo + tid] = t3d_batch_dot<1, 1>(dqv, l_act + tid * T3D_BP, B);
        else if (tid == 256) gcr[obo] = t3d_batch_sum<1>(dqv, B);
        __syncthreads();
        T3D_SUB(8);
        // hidden gradient in place: act'(h) * (dq * Wout[j]), half of the units per half
        if (live) { const float g[1] = { dqv[b] }; t3d_dz<ACT, 1>(mycol, wcc + oWo, H, prelu, g, my_lo, my_hi); }
        __syncthreads();
        T3D_SUB(9);
        // first layer: gW0[j][k] = sum_i dz[i][j] x[i][k], gb0[j] = sum_i dz[i][j]
        for (int pp = tid; pp < H * SA + H; pp += DNT) {
            if (pp < H * SA) { const int j = pp / SA, k = pp - j * SA; gcr[oW0 + pp] = t3d_batch_dot<1, SA>(l_act + j * T3D_BP, l_x + k, B); }
            else { const int j = pp - H * SA; gcr[ob0 + j] = t3d_batch_sum<1>(l_act + j * T3D_BP, B); }
        }
        __syncthreads();
        T3D_SUB(10);
    }
    return bad;
}

// the delayed policy update's gradients (TD3.py:101-110): actor_loss = (-critic_1(states, actor(states))).mean() with the UPDATED critic_1,
// the actor's gradient into ctx->grad
template <int S, int A, int ACT>
__device__ __noinline__ void t3_direct_actor(const T3DirectCtx *ctx_)
{
    constexpr int SA = S + A;
    typedef __attribute__((address_space(3))) const T3DirectCtx LCtx;
    LCtx *c = (LCtx *)uni_ptr(ctx_);
    const int tid = threadIdx.x, half = uni(tid >> 8), b = tid & 255;
    const int H = uni(c->H), B = uni(c->B), Pa = uni(c->Pa), Pc = uni(c->Pc), PaA = (Pa + 3) & ~3;
    const float prelu = unif(c->prelu), ma = unif(c->ma);
    lfloat *l_act = (lfloat *)uni_ptr(c->l_act), *l_x = (lfloat *)uni_ptr(c->l_x), *l_na = (lfloat *)uni_ptr(c->l_na), *l_w = (lfloat *)uni_ptr(c->l_w);
    const float *params = uni_ptr(c->params), *xc = uni_ptr(c->xc);
    float *grad = uni_ptr(c->grad);
    const bool live = b < B;
    lfloat *mycol = l_act + b;
    const int Hs = t3d_split(H), my_lo = half ? Hs : 0, my_hi = half ? H : Hs;
    const int oW0 = 0, ob0 = H * S, oWo = ob0 + H, obo = oWo + A * H;  // state-dict offsets of the one-hidden-layer actor
    t3d_stage(params, Pa, l_w, tid);                                   // actor | critic_1, each at a multiple of four floats
    t3d_stage(params + Pa, Pc, l_w + PaA, tid);
    __syncthreads();
    if (half == 0 && live) {
        float xr[SA], xs[S], o[A], th[A];
#pragma unroll
        for (int k = 0; k < S; ++k) { xs[k] = xc[b * SA + k]; xr[k] = xs[k]; }
        t3d_net_fwd<ACT, S, A, true, true>(l_w, H, prelu, xs, mycol, o, 0, H);          // the actor's activations stay in the sample's column
#pragma unroll
        for (int k = 0; k < A; ++k) { th[k] = det_tanhf(lenv_tanh_table, o[k]); xr[S + k] = th[k] * ma; }
        // critic_1 forward on (s, actor(s)) and, unit by unit, its backward down to the action inputs: dq = -1/B per sample,
        // dz1[j] = act'(h1[j]) * (dq * Wout[j]), dx[k] = sum_j dz1[j] W0[j][S + k]  (j ascending)
        const float dqa = -(1.0f / (float)B);
        const lfloat *W0c = l_w + PaA, *b0c = W0c + H * SA, *Woc = b0c + H;
        float dx[A];
#pragma unroll
        for (int k = 0; k < A; ++k) dx[k] = 0.0f;
        constexpr int JB = SA <= 8 ? 8 : 4;
        const bool fast = (H & 7) == 0;
#pragma unroll 1
        for (int j0 = 0; j0 < H; j0 += JB) {
            float w0[JB * SA], bv[JB], wo[JB];
            if (fast) { t3d_ld4<JB * SA>(W0c + j0 * SA, w0); t3d_ld4<JB>(b0c + j0, bv); t3d_ld4<JB>(Woc + j0, wo); }
            else {
#pragma unroll
                for (int u = 0; u < JB; ++u) {
                    const int j = j0 + u < H ? j0 + u : H - 1;
#pragma unroll
                    for (int k = 0; k < SA; ++k) w0[u * SA + k] = W0c[j * SA + k];
                    bv[u] = b0c[j]; wo[u] = Woc[j];
                }
            }
#pragma unroll
            for (int u = 0; u < JB; ++u) {
                if (j0 + u < H) {
                    float z = 0.0f;
#pragma unroll
                    for (int k = 0; k < SA; ++k) z = fma32(xr[k], w0[u * SA + k], z);
                    z = z + bv[u];
                    const float dz1 = act_bwd(ACT, prelu, act_fwd(ACT, prelu, z), fma32(dqa, wo[u], 0.0f));
#pragma unroll
                    for (int k = 0; k < A; ++k) dx[k] = fma32(dz1, w0[u * SA + S + k], dx[k]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < A; ++k) l_na[b * A + k] = (dx[k] * ma) * fma32(-th[k], th[k], 1.0f);       // d(tanh(z)*max_action)
#pragma unroll
        for (int k = 0; k < S; ++k) l_x[b * S + k] = xs[k];
    }
    __syncthreads();
    // actor output layer: gWout[c][j] = sum_i dza[i][c] h[i][j], gbout[c] = sum_i dza[i][c]
    for (int pp = tid; pp < A * H + A; pp += DNT) {
        if (pp < A * H) { const int cidx = pp / H, j = pp - cidx * H; grad[oWo + pp] = t3d_batch_dot<A, 1>(l_na + cidx, l_act + j * T3D_BP, B); }
        else { const int cidx = pp - A * H; grad[obo + cidx] = t3d_batch_sum<A>(l_na + cidx, B); }
    }
    __syncthreads();
    if (live) {                                                        // hidden gradient in place, half of the units per half
        float dza[A];
#pragma unroll
        for (int k = 0; k < A; ++k) dza[k] = l_na[b * A + k];
        t3d_dz<ACT, A>(mycol, l_w + oWo, H, prelu, dza, my_lo, my_hi);
    }
    __syncthreads();
    for (int pp = tid; pp < H * S + H; pp += DNT) {
        if (pp < H * S) { const int j = pp / S, k = pp - j * S; grad[oW0 + pp] = t3d_batch_dot<1, S>(l_act + j * T3D_BP, l_x + k, B); }
        else { const int j = pp - H * S; grad[ob0 + j] = t3d_batch_sum<1>(l_act + j * T3D_BP, B); }
    }
    __syncthreads();
}

// sum_{k < 128} x[k] * Wt[k][j] as ONE k-ascending chain from 0: x in LDS (16-byte aligned), Wt = the transposed matrix in the arena (wt points at
// column j; STRIDE = its row length as a literal, 0 = stride_rt), 64 weights in flight per thread (two register blocks refilled alternately)
template <int STRIDE>
__device__ __forceinline__ float se_chain128(const gfloat *wt, int stride_rt, const lfloat *xin)
{
    const int stride = STRIDE ? STRIDE : stride_rt;
    float wa[32], wb[32], xv[32], z = 0.0f;
#pragma unroll
    for (int u = 0; u < 32; ++u) wa[u] = wt[u * stride];
#pragma unroll
    for (int u = 0; u < 32; ++u) wb[u] = wt[(32 + u) * stride];
    t3d_ld4<32>(xin, xv);
#pragma unroll
    for (int u = 0; u < 32; ++u) z = fma32(xv[u], wa[u], z);
#pragma unroll
    for (int u = 0; u < 32; ++u) wa[u] = wt[(64 + u) * stride];
    t3d_ld4<32>(xin + 32, xv);
#pragma unroll
    for (int u = 0; u < 32; ++u) z = fma32(xv[u], wb[u], z);
#pragma unroll
    for (int u = 0; u < 32; ++u) wb[u] = wt[(96 + u) * stride];
    t3d_ld4<32>(xin + 64, xv);
#pragma unroll
    for (int u = 0; u < 32; ++u) z = fma32(xv[u], wa[u], z);
    t3d_ld4<32>(xin + 96, xv);
#pragma unroll
    for (int u = 0; u < 32; ++u) z = fma32(xv[u], wb[u], z);
    return z;
}

// DIRECT (round 6) = launches whose agent nets have ONE hidden layer of at most T3_DIRECT_H units, no LayerNorm, no ICM, batch <= T3_DIRECT_B
// (default_config_cmc_syn_env_opt.yaml's TD3, the narrow draws of td3_vary): TD3.learn without the product queue.  A queued product costs ~18 k
// cycles whatever its size (staging through LDS, workgroup barriers, a global round trip between products: profiles/r05_generic_shapes.log --
// 456 us per learn step for a 64-wide TD3).  Here ONE THREAD OWNS ONE MINIBATCH SAMPLE: it runs the sample's forward passes with the nets'
// weights broadcast from LDS (the hidden activations stay in its registers), forms the TD target and the per-sample output gradients; the batch
// sums of the parameter gradients then run as one i-ascending chain per parameter over an LDS copy of the activations (unit-major, row stride 257:
// writers = samples and readers = units are both conflict-free, see t3d_layout).  Every chain is the queued product's own k- / i-ascending fmaf chain from 0
// with the epilogues' bias / activation / derivative arithmetic, so the bits are those of the GEMM-queue path and of the oracle.  Its own
// instantiations: as a run-time branch next to the queued learn step the extra live state pushed the Pendulum instantiation into SGPR spills, where
// the ROCm 7.2 backend emits an illegal VALU compare on the LDS aperture register.
// The resume record of a chain after a segment (include/lenv_hip.h documents the words): thread 0, behind the barrier that follows the threads'
// atomicMin into the folded status
__device__ __forceinline__ void td3_write_record(int64_t *rec, int next_episode, int finished, int status, int timed_out_at, int64_t n_rand,
                                                 int64_t n_actn, int64_t n_testn, int64_t n_test_ep, int64_t learn_it, int train_steps,
                                                 int test_steps, int episodes_run, const double *pows, const double *icm_pows)
{
    rec[0] = next_episode; rec[1] = finished; rec[2] = status; rec[3] = timed_out_at;
    rec[4] = n_rand; rec[5] = n_actn; rec[6] = n_testn; rec[7] = n_test_ep; rec[8] = learn_it;
    rec[9] = train_steps; rec[10] = test_steps; rec[11] = episodes_run; rec[12] = train_steps;
    for (int i = 0; i < 4; ++i) rec[13 + i] = __double_as_longlong(pows[i]);
    for (int i = 0; i < 2; ++i) rec[17 + i] = __double_as_longlong(icm_pows[i]);
    for (int w = 19; w < LENV_TD3_RESUME_WORDS; ++w) rec[w] = 0;
}

// SEG (lenv_td3_rn_inner_loop_segment, include/lenv_hip.h) = the queued kernel over the episodes [a.ep_begin, a.ep_end): everything the loop carries
// from episode to episode outside the arena -- the counters, the Adam bias-correction powers, the status -- is read from / written to the chain's
// resume record; the reward net (LDS) is staged by every segment, the agent / ICM only by the first; the closing part runs in the segment in
// which the chain ends.  Its own instantiations: the code of the others is what it was.
template <bool ICM, int ENV, int SHAPE = 0, bool DIRECT = false, bool SEG = false>
__global__ __launch_bounds__(DNT) void td3_rn_inner_kernel(const Td3Args a)
{
    static_assert(!DIRECT || (SHAPE == 0 && !ICM && DNT == 512), "the DIRECT instantiations: generic shapes, no ICM, two 256-thread halves");
    static_assert(!SEG || (SHAPE == 0 && !DIRECT), "the SEG instantiations: the generic GEMM-queue kernel");
    using EnvT = ContEnv<ENV>;
    constexpr bool FIXED = SHAPE != 0;
    constexpr Td3Shape kTd3Shape = kTd3Shapes[SHAPE];
    static_assert(!FIXED || (!ICM && ENV == kTd3Shape.env), "the specialised instantiations: their own env, no ICM");
    extern __shared__ __align__(16) float lds[];
    const lenv_td3_cfg &cfg = a.cfg;
    const int tid = threadIdx.x;
    const int64_t chain = blockIdx.x;
    // the chain's status word starts at 0 (ok); written here rather than by a memset node in front of the launch (a captured
    // generation replayed under rocprofv3 did not run the memset)
    int64_t *rec = nullptr;
    const bool fresh = !SEG || a.ep_begin == 0;          // the arena is initialised by this launch
    if constexpr (SEG) {
        rec = a.resume + chain * LENV_TD3_RESUME_WORDS;
        if (!fresh) {                                    // uniform per chain
            if (rec[1] == 1) return;                     // finished in an earlier segment: the chain and its outputs stay as they are
            if (rec[0] != (int64_t)a.ep_begin) { if (tid == 0 && a.out.status) a.out.status[chain] = -10; return; }
        }
    }
    if (threadIdx.x == 0 && a.out.status) { if (fresh) a.out.status[chain] = 0; }
    constexpr int S = EnvT::S, A = EnvT::A, SA = S + A, SD = EnvT::SD;   // observation / action dims, fp64 words of the env's own state
    const bool vary = FIXED ? false : a.hp_batch != nullptr;
    const int H = FIXED ? kTd3Shape.H : (vary ? a.hp_hidden[chain] : cfg.hidden), L = FIXED ? kTd3Shape.L : (vary ? a.hp_layers[chain] : cfg.layers);
    const int Bm = FIXED ? kTd3Shape.B : cfg.batch_size;                               // LDS is carved for cfg's (maximal) batch
    const int B = FIXED ? kTd3Shape.B : (vary ? a.hp_batch[chain] : cfg.batch_size);
    const double lr = vary ? a.hp_lr[chain] : cfg.lr;
    const int T = FIXED ? kTd3Shape.T : cfg.test_episodes, Hrn = FIXED ? kTd3Shape.Hrn : cfg.rn_hidden, RS = a.RS;
    const int rn_layers = FIXED ? kTd3Shape.rn_layers : cfg.rn_layers, rn_act = FIXED ? kTd3Shape.rn_act : cfg.rn_act;
    const bool virtual_env = FIXED ? kTd3Shape.virtual_env != 0 : cfg.virtual_env != 0;
    const int info_dim = cfg.info_dim, policy_delay = FIXED ? kTd3Shape.policy_delay : cfg.policy_delay;
    if (vary && (H < 1 || H > cfg.hidden || L < 1 || L > cfg.layers || B < 1 || B > Bm)) {   // uniform per chain
        if (tid == 0) {
            if (a.out.status) a.out.status[chain] = -8;
            a.out.score[chain] = 0.0;
            if constexpr (SEG) { for (int w = 0; w < LENV_TD3_RESUME_WORDS; ++w) rec[w] = 0; rec[1] = 1; rec[2] = -8; rec[3] = -1; }
        }
        return;
    }
    MlpOff mo_actor, mo_critic;
    const bool use_ln = FIXED ? false : cfg.use_layer_norm != 0;
    mlp_off(mo_actor, S, H, L, A, use_ln);
    mlp_off(mo_critic, SA, H, L, 1, use_ln);
    MlpOff mo_se[3];                                      // VirtualEnv: state_net | reward_net | done_net on cat(action, state)
    mlp_off(mo_se[0], SA, Hrn, rn_layers, S);
    mlp_off(mo_se[1], SA, Hrn, rn_layers, 1);
    mlp_off(mo_se[2], SA, Hrn, rn_layers, 1);
    // cfg.rn_layer_norm: the env nets' own LayerNorm.  NES perturbs nn.Linear modules only (GTN_worker.py:156-175): no parameters in theta,
    // the rows are normalised with the constructor's weight 1 / bias 0 (ln == 2: a position without a parameter block)
    const bool rn_ln = FIXED ? false : (cfg.rn_layer_norm != 0 && rn_layers >= 2);
    if (rn_ln) mo_se[0].ln = mo_se[1].ln = mo_se[2].ln = 2;
    const int Pa = mo_actor.P, Pc = mo_critic.P, P = Pa + 2 * Pc;
    const int act_id = FIXED ? kTd3Shape.act : cfg.act;
    const float prelu = cfg.prelu, ma = (float)cfg.max_action;

    // ---- LDS carve-up ----
    float *Ps = lds, *Qs = Ps + GemmShape<T3_MAXI>::PS_FLOATS;
    GemmCmd *cmds = reinterpret_cast<GemmCmd *>(Qs + GemmShape<T3_MAXI>::QS_FLOATS);   // [GEMM_QUEUE_MAX] command queue
    float *rn_w = reinterpret_cast<float *>(cmds + GEMM_QUEUE_MAX);   // reward net: W0 [Hrn][S] | b0 [Hrn] | Wout [Hrn] | bout
    float *rn_h = rn_w + ((a.P_rn_lds + 3) & ~3);         // [Hrn]
    float *rn_h2 = rn_h + ((Hrn + 3) & ~3);               // [Hrn] second hidden row of a reward net with more than one hidden layer
    float *q1 = rn_h2 + ((Hrn + 3) & ~3);                 // [B]
    float *q2 = q1 + Bm, *tq1 = q2 + Bm, *tq2 = tq1 + Bm, *rr = tq2 + Bm, *dd = rr + Bm, *dq1 = dd + Bm, *dq2 = dq1 + Bm;
    float *misc = dq2 + Bm;                                // [64]
    double *xs_d = reinterpret_cast<double *>((reinterpret_cast<uintptr_t>(misc + 64) + 7) & ~(uintptr_t)7);   // [17] train env state
    double *xt_d = xs_d + 20;                             // [T][17] test env states
    double *ret = xt_d + 17 * T;                          // [T]
    float *ep_rew = reinterpret_cast<float *>(ret + T);   // [T]
    int *tlen = reinterpret_cast<int *>(ep_rew + T);      // [T] env steps of each test episode
    int *tflag = tlen + T;                                // [T] test episode still running
    float *state = reinterpret_cast<float *>(tflag + T);  // [20] current observation (fp32)
    float *action = state + 20;                           // [8]
    float *newrow = action + 8;                           // [56] replay row [s | a | s' | r | done] + scratch + info[4] at 2S+A+4
    volatile float *ctrl = misc;
    volatile int *ictrl = reinterpret_cast<volatile int *>(misc + 32);
    // the control words in use: ctrl[10..15] (Adam, reward net, LayerNorm rows), ctrl[20..21] (ICM's Adam), ictrl[3..4] = misc[35..36];
    // misc[MISC_STATUS_FOLD] (an int): the SEG instantiations' fold of the threads' status codes.  A new control word takes a free index below it.
    constexpr int MISC_STATUS_FOLD = 48;

    float *arena = a.arena + chain * a.arena_stride;
    float *params = arena + a.a_params, *targets = arena + a.a_targets, *adam_m = arena + a.a_m, *adam_v = arena + a.a_v;
    float *grad = arena + a.a_grad, *rb = arena + a.a_replay;
    float *xc = arena + a.a_xc, *xn = arena + a.a_xn, *xa = arena + a.a_xa;      // [B][SA] critic inputs
    float *dxb = arena + a.a_dx, *thb = arena + a.a_th, *dzb = arena + a.a_dz;
    float *hc1[T3_MAXL], *hc2[T3_MAXL], *ha[T3_MAXL], *ht[T3_MAXL], *dbuf[2] = { arena + a.a_d[0], arena + a.a_d[1] };
    for (int l = 0; l < T3_MAXL; ++l) { hc1[l] = arena + a.a_hc1[l]; hc2[l] = arena + a.a_hc2[l]; ha[l] = arena + a.a_ha[l]; ht[l] = arena + a.a_ht[l]; }
    float *xh1[T3_MAXL], *xh2[T3_MAXL], *xha[T3_MAXL], *rstd1 = arena + a.a_rstd, *rstd2 = rstd1 + T3_MAXL * Bm, *rstda = rstd2 + T3_MAXL * Bm;
    for (int l = 0; l < T3_MAXL; ++l) { xh1[l] = arena + a.a_xh[0][l]; xh2[l] = arena + a.a_xh[1][l]; xha[l] = arena + a.a_xh[2][l]; }
    double *meter = reinterpret_cast<double *>(arena + a.a_meter);

    // ---- stage the perturbed reward network (GTN_worker.py:165-175) and the fresh agent (TD3.py:31-39) ----
    {
        const float sg = a.eps ? a.sign[chain] : 0.0f;
        const float *e = a.eps ? a.eps + (int64_t)a.worker[chain] * a.P_rn : nullptr;
        // VirtualEnv (three nets) and reward nets with several hidden layers are too large for LDS -> arena
        float *dst = (virtual_env || rn_layers > 1) ? arena + a.a_se : rn_w;
        for (int i = tid; i < a.P_rn; i += DNT) dst[i] = e ? fma32(sg, e[i], a.theta[i]) : a.theta[i];
        if (virtual_env) {
            // the same three nets once more with every matrix K-major (Wt[k][j] = W[j][k]): thread j of a one-row product then reads
            // consecutive words with its neighbours instead of a row of its own
            __syncthreads();
            float *dT = arena + a.a_seT;
            int base = 0;
            for (int n = 0; n < 3; ++n) {
                const MlpOff &mo = mo_se[n];
                int n_in = mo.in;
                for (int l = 0; l <= mo.L; ++l) {
                    const int n_out = l == mo.L ? mo.out : mo.H;
                    for (int e2 = tid; e2 < n_out * n_in; e2 += DNT) { const int j = e2 / n_in, k = e2 - j * n_in; dT[base + mo.oW[l] + k * n_out + j] = dst[base + mo.oW[l] + e2]; }
                    for (int j = tid; j < n_out; j += DNT) dT[base + mo.ob[l] + j] = dst[base + mo.ob[l] + j];
                    n_in = mo.H;
                }
                base += mo.P;
            }
        }
    }
    if (fresh) for (int p = tid; p < P; p += DNT) {
        const float w = a.agent_init[chain * a.P + p];
        params[p] = w; targets[p] = w; adam_m[p] = 0.0f; adam_v[p] = 0.0f;
    }
    // fresh ICM (continuous actions: the action vector is the model input, MSE inverse loss -- icm_baseline.py:121-122)
    IcmNet icm;
    double icm_pows[2] = { 1.0, 1.0 };
    if constexpr (ICM) {
        icm_build(icm, S, A, cfg.icm_feature_dim, cfg.icm_hidden, /*discrete=*/false);
        float *ip = arena + a.a_icm[IB_P], *im = arena + a.a_icm[IB_M], *iv = arena + a.a_icm[IB_V];
        if (fresh) for (int p = tid; p < icm.P; p += DNT) { ip[p] = a.icm_init[chain * a.P_icm + p]; im[p] = 0.0f; iv[p] = 0.0f; }
    }
    if (tid < 64) misc[tid] = 0.0f;
    __syncthreads();

    const uint64_t key = a.rng_keys ? a.rng_keys[chain] : 0;
    const bool tape = FIXED ? false : cfg.rng_mode == LENV_RNG_TAPE;
    const int rtype = FIXED ? kTd3Shape.rtype : cfg.reward_env_type;
    int status = 0;
    PT_DECL;
    int64_t n_rand = 0, n_actn = 0, n_testn = 0, n_test_ep = 0, learn_it = 0;
    int train_steps = 0, test_steps = 0, episodes_run = 0;
    double pows[4] = { 1.0, 1.0, 1.0, 1.0 };
    const int rb_cap = (int)a.rb_cap;
    if constexpr (SEG) {
        if (!fresh) {                                    // every thread its copy, like the counters of a single launch
            status = (int)rec[2];
            n_rand = rec[4]; n_actn = rec[5]; n_testn = rec[6]; n_test_ep = rec[7]; learn_it = rec[8];
            train_steps = (int)rec[9]; test_steps = (int)rec[10]; episodes_run = (int)rec[11];
            for (int i = 0; i < 4; ++i) pows[i] = __longlong_as_double(rec[13 + i]);
            for (int i = 0; i < 2; ++i) icm_pows[i] = __longlong_as_double(rec[17 + i]);
        }
    }

    // ---- generic MLP forward over I <= 256 rows (row stride ldx); hidden activations to hid[l][I][H].  The layer products
    // are QUEUED (gq); the caller runs the queue.  final_tanh: out = tanh(net)*max_action (Actor_TD3.forward) with tanh
    // values to th_out; else out = net (Critic_Q).
    GemmQueue gq(cmds);
    constexpr int LNBUF = GemmShape<T3_MAXI>::PS_FLOATS + GemmShape<T3_MAXI>::QS_FLOATS;
    auto mlp_forward = [&](const float *par, const MlpOff &mo, const float *X, int ldx, int I, float *const *hid, float *out,
                           int ldo, int ocol, bool final_tanh, float *th_out, int act = -1, float pr = 0.25f, float *const *xh = nullptr,
                           float *rstd = nullptr) {
        if (act < 0) { act = act_id; pr = prelu; }                // default: the agent's activation
        const float *in = X;
        int n_in = mo.in, ldin = ldx;
        for (int l = 0; l < mo.L; ++l) {
            if (mo.ln && l >= 1) {
                // a LayerNorm position: Linear + bias, the queue runs (everything queued so far, in order), then the row routine normalises,
                // scales and applies the activation (lenv_ln.cuh); xh / rstd: kept for the backward pass
                gq.gemm(in, ldin, 1, par + mo.oW[l], n_in, 1, I, mo.H, n_in, epi_bias(hid[l], mo.H, 0, par + mo.ob[l]));
                gq.run<T3_MAXI>(Ps, Qs);
                ln_rows_forward<LNBUF>(Ps, hid[l], I, mo.H, par + mo.oLN, par + mo.oLN + mo.H, xh ? xh[l] : nullptr, rstd ? rstd + (int64_t)l * Bm : nullptr, act, pr);
            } else gq.gemm(in, ldin, 1, par + mo.oW[l], n_in, 1, I, mo.H, n_in, epi_bias_act(hid[l], mo.H, par + mo.ob[l], act, pr));
            in = hid[l]; n_in = mo.H; ldin = mo.H;
        }
        const float *W = par + mo.oW[mo.L], *bb = par + mo.ob[mo.L];
        if (final_tanh) gq.gemm(in, ldin, 1, W, n_in, 1, I, mo.out, n_in, epi_bias_tanh(out, ldo, ocol, bb, ma, th_out, mo.out));
        else gq.gemm(in, ldin, 1, W, n_in, 1, I, mo.out, n_in, epi_bias(out, ldo, ocol, bb));
    };

    // ---- the actor on ONE row (the training step's action, a single test episode): thread j owns output j of a layer and runs
    // the same k-ascending fmaf chain the MFMA product runs (then + bias, activation; tanh * max_action at the end), so the
    // result is bit-identical to mlp_forward(..., I = 1, ...) at a fraction of a queued product's fixed cost ----
    auto mlp_row1 = [&](const float *par, const MlpOff &mo, const float *x, float *out, int ocol, bool final_tanh, int act, float pr) {
        const float *in = x;
        int n_in = mo.in;
        for (int l = 0; l <= mo.L; ++l) {
            const bool last = l == mo.L;
            const int n_out = last ? mo.out : mo.H;
            const float *W = par + mo.oW[l], *bb = par + mo.ob[l];
            float *h = last ? out + ocol : ht[l];
            const bool lnl = !last && mo.ln && l >= 1;               // a LayerNorm position: reduced by thread 0 (as td3_discrete_inner_loop.hip)
            for (int j = tid; j < n_out; j += DNT) {
                const float *w = W + (int64_t)j * n_in;
                float z = 0.0f;
                if ((n_in & 3) == 0) {
                    int k = 0;
                    for (; k + 32 <= n_in; k += 32) {          // 32 terms requested before the first fmaf (one round trip instead of eight)
                        float4 wv[8], xv[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) { wv[u] = *reinterpret_cast<const float4 *>(w + k + 4 * u); xv[u] = *reinterpret_cast<const float4 *>(in + k + 4 * u); }
#pragma unroll
                        for (int u = 0; u < 8; ++u) { z = fma32(xv[u].x, wv[u].x, z); z = fma32(xv[u].y, wv[u].y, z); z = fma32(xv[u].z, wv[u].z, z); z = fma32(xv[u].w, wv[u].w, z); }
                    }
                    for (; k < n_in; k += 4) {
                        const float4 wv = *reinterpret_cast<const float4 *>(w + k);
                        const float4 xv = *reinterpret_cast<const float4 *>(in + k);
                        z = fma32(xv.x, wv.x, z); z = fma32(xv.y, wv.y, z); z = fma32(xv.z, wv.z, z); z = fma32(xv.w, wv.w, z);
                    }
                } else for (int k = 0; k < n_in; ++k) z = fma32(in[k], w[k], z);
                z = z + bb[j];
                h[j] = last ? (final_tanh ? det_tanhf(lenv_tanh_table, z) * ma : z) : (lnl ? z : act_fwd(act, pr, z));
            }
            __syncthreads();
            if (lnl) {
                if (tid == 0) {
                    float sm = 0.0f, sv = 0.0f;
                    for (int j = 0; j < n_out; ++j) sm = sm + h[j];
                    const float mean = sm / (float)n_out;
                    for (int j = 0; j < n_out; ++j) { const float dj = h[j] - mean; sv = fma32(dj, dj, sv); }
                    ctrl[14] = mean; ctrl[15] = 1.0f / __builtin_sqrtf(sv / (float)n_out + 1e-5f);
                }
                __syncthreads();
                const float mean = ctrl[14], r = ctrl[15];
                const float *lw = par + mo.oLN, *lb = lw + mo.H;
                if (mo.ln == 2) { for (int j = tid; j < n_out; j += DNT) h[j] = act_fwd(act, pr, fma32((h[j] - mean) * r, 1.0f, 0.0f)); }
                else for (int j = tid; j < n_out; j += DNT) h[j] = act_fwd(act, pr, fma32((h[j] - mean) * r, lw[j], lb[j]));
                __syncthreads();
            }
            in = h; n_in = mo.H;
        }
    };
    auto actor_row1 = [&](const float *par, const float *x, float *out) { mlp_row1(par, mo_actor, x, out, 0, true, act_id, prelu); };
    // The three nets of a VirtualEnv (state | reward | done: same input row, same depth and width) side by side: thread group g = tid / 128
    // runs net g with mlp_row1's chains (its hidden rows in row g of ht[l]) on the TRANSPOSED copy of its matrices -- thread j reads
    // Wt[k][j], consecutive words across the wave, 32 terms requested before their fmaf run starts; one barrier per layer for all three.
    // (Row by row -- thread j walking W[j][:] -- every load instruction touches 64 cache lines: the step of a three-layer 128-wide SE cost
    // 250 k cycles, 42 % of a small-net TD3 generation: tools/phase_timing_td3_generic.py.)  Nets wider than 128, LayerNorm nets (their row
    // statistics are one thread's job) and arenas without three rows of room take mlp_row1 net by net.
    const bool se_side_by_side = DNT >= 384 && Hrn <= 128 && !rn_ln && 3 * (int64_t)Hrn <= (int64_t)(Bm > T ? Bm : T) * H;
    auto se_rows = [&](const float *x, float *out) {
        if (!se_side_by_side) {
            const float *sep = arena + a.a_se;
            mlp_row1(sep, mo_se[0], x, out, 0, false, rn_act, cfg.rn_prelu);
            mlp_row1(sep + mo_se[0].P, mo_se[1], x, out, S, false, rn_act, cfg.rn_prelu);
            mlp_row1(sep + mo_se[0].P + mo_se[1].P, mo_se[2], x, out, S + 1, false, rn_act, cfg.rn_prelu);
            return;
        }
        const int g = tid >> 7, j = tid & 127;
        const MlpOff &mo = mo_se[g < 3 ? g : 0];
        const gfloat *par = (const gfloat *)(arena + a.a_seT) + (g == 0 ? 0 : (g == 1 ? mo_se[0].P : mo_se[0].P + mo_se[1].P));
        const int ocol = g == 0 ? 0 : S + g - 1;
        if (Hrn == 128 && mo_se[0].in <= 32) {
            // 128-wide nets (what the YAMLs ship): the hidden rows live in the idle product-staging buffer (LDS, two sets of three), the transposed
            // matrices are walked with literal strides, 64 weights in flight per thread (two register blocks refilled alternately).  The chains
            // are the ones below: k ascending from 0, bias added after.  (The general loop -- input row and weights from the arena, 32 terms
            // requested, waited for, consumed -- took ~50 k cycles per step of a three-layer SE: 56 % of a small-net TD3 generation.)
            lfloat *hb = lds_offset_ptr(Ps);                // (not a cast: see lenv_gemm.cuh)
            if (g < 3) {                                   // first layer: the input row (at most 32 words) from the arena
                const gfloat *wt = par + mo.oW[0] + j, *in0 = (const gfloat *)x;
                const int n_in = mo.in;
                float wv[32], xv[32], z = 0.0f;
#pragma unroll
                for (int u = 0; u < 32; ++u) { const int k = u < n_in ? u : n_in - 1; wv[u] = wt[k * 128]; xv[u] = in0[k]; }
#pragma unroll
                for (int u = 0; u < 32; ++u) if (u < n_in) z = fma32(xv[u], wv[u], z);
                hb[g * 128 + j] = act_fwd(rn_act, cfg.rn_prelu, z + par[mo.ob[0] + j]);
            }
            __syncthreads();
            int cur = 0;
            for (int l = 1; l < mo.L; ++l) {
                if (g < 3) {
                    const float z = se_chain128<128>(par + mo.oW[l] + j, 128, hb + cur * 384 + g * 128);
                    hb[(cur ^ 1) * 384 + g * 128 + j] = act_fwd(rn_act, cfg.rn_prelu, z + par[mo.ob[l] + j]);
                }
                __syncthreads();
                cur ^= 1;
            }
            if (g < 3 && j < mo.out) out[ocol + j] = se_chain128<0>(par + mo.oW[mo.L] + j, mo.out, hb + cur * 384 + g * 128) + par[mo.ob[mo.L] + j];
            __syncthreads();
            return;
        }
        const gfloat *in = (const gfloat *)x;              // (the SE's input row and the hidden rows: arena)
        int n_in = mo.in;
        for (int l = 0; l <= mo.L; ++l) {
            const bool last = l == mo.L;
            const int n_out = last ? mo.out : mo.H;
            float *h = last ? out + ocol : ht[l] + (g < 3 ? g : 0) * mo.H;
            if (g < 3 && j < n_out) {
                const gfloat *wt = par + mo.oW[l] + j;
                float z = 0.0f;
                for (int k0 = 0; k0 < n_in; k0 += 32) {
                    float wv[32], xv[32];
#pragma unroll
                    for (int u = 0; u < 32; ++u) { const int k = k0 + u < n_in ? k0 + u : n_in - 1; wv[u] = wt[k * n_out]; xv[u] = in[k]; }
#pragma unroll
                    for (int u = 0; u < 32; ++u) if (k0 + u < n_in) z = fma32(xv[u], wv[u], z);
                }
                z = z + par[mo.ob[l] + j];
                h[j] = last ? z : act_fwd(rn_act, cfg.rn_prelu, z);
            }
            __syncthreads();
            in = (const gfloat *)h; n_in = mo.H;
        }
    };

    // ---- generic MLP backward: dOut [I][out] -> parameter gradients gpar (may be null) and input gradient dX (may be null);
    // queued like the forward.  The output-layer bias gradient (a handful of columns of an LDS vector) is done in place.
    auto mlp_backward = [&](const float *par, const MlpOff &mo, const float *X, int ldx, int I, float *const *hid, const float *dOut,
                            float *gpar, float *dX, float *const *xh = nullptr, const float *rstd = nullptr) {
        const int Hh = mo.H, O = mo.out;
        // a LayerNorm position (hidden layer lp >= 1): d holds the gradient of the LayerNorm OUTPUT; run the queue, then the row routine
        // turns it into the gradient of the Linear's output and adds the position's share of the shared weight / bias gradient (positions
        // from the top down, as the oracle folds them; gpar null: the input gradient only)
        auto ln_pos = [&](float *d, int lp) {
            if (!(mo.ln && lp >= 1)) return;
            gq.run<T3_MAXI>(Ps, Qs);
            ln_rows_backward<LNBUF, T3_MAXW>(Ps, d, I, Hh, par + mo.oLN, xh[lp], rstd + (int64_t)lp * Bm, gpar ? gpar + mo.oLN : nullptr,
                                             gpar ? gpar + mo.oLN + Hh : nullptr, lp == mo.L - 1);
        };
        if (gpar) {
            gq.gemm(dOut, 1, O, hid[mo.L - 1], 1, Hh, O, Hh, I, epi_store(gpar + mo.oW[mo.L], Hh));
            gq.colsum(dOut, I, O, O, gpar + mo.ob[mo.L]);
        }
        float *dcur = dbuf[0];
        gq.gemm(dOut, O, 1, par + mo.oW[mo.L], 1, Hh, I, Hh, O, epi_act_bwd(dcur, Hh, hid[mo.L - 1], Hh, act_id, prelu));
        ln_pos(dcur, mo.L - 1);
        for (int l = mo.L - 1; l >= 0; --l) {
            const int n_in = l == 0 ? mo.in : Hh;
            const float *inp = l == 0 ? X : hid[l - 1];
            const int ldin = l == 0 ? ldx : Hh;
            if (gpar) {
                gq.gemm(dcur, 1, Hh, inp, 1, ldin, Hh, n_in, I, epi_store(gpar + mo.oW[l], n_in));
                gq.colsum(dcur, I, Hh, Hh, gpar + mo.ob[l]);
            }
            if (l > 0) {
                float *dn = dbuf[(mo.L - l) & 1];
                gq.gemm(dcur, Hh, 1, par + mo.oW[l], 1, n_in, I, n_in, Hh, epi_act_bwd(dn, n_in, hid[l - 1], n_in, act_id, prelu));
                ln_pos(dn, l - 1);
                dcur = dn;
            } else if (dX) {
                gq.gemm(dcur, Hh, 1, par + mo.oW[0], 1, n_in, I, n_in, Hh, epi_store(dX, n_in));
            }
        }
    };

    // torch.optim.Adam single-tensor step on params[p0, p0+n) (pows index pi), thread 0 publishes the bias corrections
    auto adam = [&](int p0, int n, int pi) {
        if (tid == 0) {
            pows[pi] *= cfg.adam_beta1; pows[pi + 1] *= cfg.adam_beta2;
            ctrl[10] = (float)(-(lr / (1.0 - pows[pi])));
            ctrl[11] = (float)__builtin_sqrt(1.0 - pows[pi + 1]);
        }
        __syncthreads();
        const float neg_step = ctrl[10], bc2_sqrt = ctrl[11];
        const float w1 = (float)(1.0 - cfg.adam_beta1), w2 = (float)(1.0 - cfg.adam_beta2), beta2 = (float)cfg.adam_beta2, aeps = (float)cfg.adam_eps;
        const AdamConsts ac{ neg_step, bc2_sqrt, w1, w2, beta2, aeps };
        wg_adam(params, adam_m, adam_v, grad, p0, n, ac, nullptr, 0.0f, 0.0f);
        __syncthreads();
    };

    // phi = reward_net(obs [| info]) for the observation in `obs` (LDS, S floats) -> ctrl[slot].  Types 3,4,7,8 append the
    // real env's info vector to the input (reward_env.py:98-101); 101/102 are Linear(info_dim, 1, bias=False) of it.
    const bool rn_info_in = rtype == 3 || rtype == 4 || rtype == 7 || rtype == 8;
    const int Drn = rn_info_in ? S + info_dim : S;
    auto rn_eval = [&](const float *obs, const float *info, int slot) {
        if (rtype == 0) { if (tid == 0) ctrl[slot] = 0.0f; __syncthreads(); return; }
        if (rtype > 100) {
            if (tid == 0) {
                float acc = 0.0f;
                for (int k = 0; k < info_dim; ++k) acc = fma32(info[k], rn_w[k], acc);
                ctrl[slot] = acc;
            }
            __syncthreads();
            return;
        }
        // build_nn_from_config (model_utils.py:16-29): Linear(D, H) | [Linear(H, H)] x (layers - 1) | Linear(H, 1), flat in
        // Module.parameters() order; one hidden layer lives in LDS, deeper nets in the arena
        const float *rnp = rn_layers > 1 ? arena + a.a_se : rn_w;
        const float *W0 = rnp, *b0 = rnp + Hrn * Drn;
        for (int j = tid; j < Hrn; j += DNT) {
            float z = 0.0f;
            for (int k = 0; k < S; ++k) z = fma32(obs[k], W0[j * Drn + k], z);
            if (rn_info_in) for (int k = 0; k < info_dim; ++k) z = fma32(info[k], W0[j * Drn + S + k], z);
            rn_h[j] = act_fwd(rn_act, cfg.rn_prelu, z + b0[j]);
        }
        __syncthreads();
        const float *hp = rn_h, *Wl = b0 + Hrn;
        float *hn = rn_h2;
        for (int l = 1; l < rn_layers; ++l) {
            const float *bl = Wl + Hrn * Hrn;
            for (int j = tid; j < Hrn; j += DNT) {
                float z = 0.0f;
                for (int k = 0; k < Hrn; ++k) z = fma32(hp[k], Wl[j * Hrn + k], z);
                z = z + bl[j];
                hn[j] = rn_ln ? z : act_fwd(rn_act, cfg.rn_prelu, z);
            }
            __syncthreads();
            if (rn_ln) {                                   // the reward net's LayerNorm row (weight 1 / bias 0), reduced by thread 0 as in mlp_row1
                if (tid == 0) {
                    float sm = 0.0f, sv = 0.0f;
                    for (int j = 0; j < Hrn; ++j) sm = sm + hn[j];
                    const float mean = sm / (float)Hrn;
                    for (int j = 0; j < Hrn; ++j) { const float dj = hn[j] - mean; sv = fma32(dj, dj, sv); }
                    ctrl[14] = mean; ctrl[15] = 1.0f / __builtin_sqrtf(sv / (float)Hrn + 1e-5f);
                }
                __syncthreads();
                const float mean = ctrl[14], r = ctrl[15];
                for (int j = tid; j < Hrn; j += DNT) hn[j] = act_fwd(rn_act, cfg.rn_prelu, fma32((hn[j] - mean) * r, 1.0f, 0.0f));
                __syncthreads();
            }
            const float *t2 = hp; hp = hn; hn = const_cast<float *>(t2);
            Wl = bl + Hrn;
        }
        const float *Wo = Wl, *bo = Wo + Hrn;
        if (tid == 0) {
            float acc = 0.0f;
            for (int j = 0; j < Hrn; ++j) acc = fma32(hp[j], Wo[j], acc);
            ctrl[slot] = acc + bo[0];
        }
        __syncthreads();
    };

    // ---- real-env test phase (BaseAgent.test, base_agent.py:155-227): T episodes in lock-step.  Every chosen action is applied
    // same_action_num times (EnvWrapper.step, env_wrapper.py:56-61: python-float reward sum, the repeats stop at done); an episode
    // ends at the env's own done flag or after max_steps env steps (TimeLimit).  Thread te < Tg owns episode g0 + te's
    // bookkeeping.  With a noise TAPE and an env that can terminate the reference's draws are consumed episode by episode, so
    // the episodes run one after the other there (Tg = 1); everywhere else the noise of (episode, agent step) has a fixed index.
    const int k_rep = FIXED ? kTd3Shape.k_rep : (cfg.same_action_num > 1 ? cfg.same_action_num : 1);
    auto test_phase = [&]() {
        const int nag = (cfg.max_steps + k_rep - 1) / k_rep;               // agent steps of a full-length episode
        const bool serial = tape && EnvT::TERMINATES;
        const int Tg = serial ? 1 : T;
        const int64_t nstride = tape ? nag : cfg.max_steps;                // noise index stride between episodes
        int64_t noise_used = 0;
        float *xt = xn;                                    // [Tg][S] fp32 observations (xn is free outside learn)
        float *at = xa;                                    // [Tg][A] actions
        for (int g0 = 0; g0 < T; g0 += Tg) {
            for (int e = tid; e < Tg * SD; e += DNT) {
                const int te = e / SD, i = e - te * SD;
                const int64_t row = n_test_ep + g0 + te;
                double v;
                if (tape) { if (row >= a.tapes.test_reset_stride) { status = -5; v = 0.0; } else v = a.tapes.test_reset[(chain * a.tapes.test_reset_stride + row) * SD + i]; }
                else v = EnvT::reset_word(key, STREAM_TEST_RESET, row, i);
                xt_d[e] = v;
            }
            if (tid < Tg) { ep_rew[g0 + tid] = 0.0f; tflag[tid] = 1; }
            __syncthreads();
            int my_el = 0;
            bool my_alive = tid < Tg;
            int ai = 0;
            for (; ai < nag; ++ai) {
                for (int e = tid; e < Tg * S; e += DNT) { const int te = e / S; xt[e] = EnvT::obs(e - te * S, xt_d + te * SD); }
                __syncthreads();
                if (Tg == 1) actor_row1(params, xt, at);
                else {
                    mlp_forward(params, mo_actor, xt, S, Tg, ht, at, A, 0, true, nullptr);
                    gq.run<T3_MAXI>(Ps, Qs);
                }
                // select_test_action (TD3.py:126-129): (actor(s) + randn(A)*action_std*max_action).clamp(-max, max)
                for (int e = tid; e < Tg * A; e += DNT) {
                    const int te = e / A, k = e - te * A;
                    const int64_t n = (serial ? n_testn + noise_used + ai : n_testn + (int64_t)(g0 + te) * nstride + ai) * A + k;
                    float zn;
                    if (tape) { if (n >= a.tapes.test_noise_stride * A) { status = -7; zn = 0.0f; } else zn = a.tapes.test_noise[chain * a.tapes.test_noise_stride * A + n]; }
                    else zn = (float)det_normal(key, STREAM_TD3_TEST_NOISE, (uint64_t)n);
                    const float v = at[e] + (zn * (float)cfg.action_std) * ma;
                    at[e] = v < -ma ? -ma : (v > ma ? ma : v);
                }
                __syncthreads();
                double rsum = 0.0;
                const bool started = my_alive;
                for (int r_ = 0; r_ < k_rep; ++r_) {
                    double nx = 0.0, pre = 0.0;
                    const int wte = tid / SD;
                    const bool wstep = tid < Tg * SD && tflag[wte] != 0;
                    if (wstep) nx = EnvT::step_word(tid - wte * SD, xt_d + wte * SD, at + wte * A);
                    if (my_alive) pre = EnvT::reward_pre(xt_d + tid * SD, at + tid * A);     // the part of the reward that sees the OLD state
                    __syncthreads();
                    if (wstep) xt_d[tid] = nx;
                    __syncthreads();
                    if (my_alive) {
                        rsum = rsum + EnvT::reward_post(xt_d + tid * SD, pre);
                        ++my_el;
                        if (EnvT::done(xt_d + tid * SD) || my_el >= cfg.max_steps) { my_alive = false; tflag[tid] = 0; }
                    }
                    __syncthreads();
                }
                if (started) ep_rew[g0 + tid] = ep_rew[g0 + tid] + (float)rsum;
                if (tid == 0) { int c = 0; for (int te = 0; te < Tg; ++te) c += tflag[te]; ictrl[4] = c; }
                __syncthreads();
                const int alive = ictrl[4];
                __syncthreads();
                if (alive == 0) { ++ai; break; }
            }
            if (tid < Tg) tlen[g0 + tid] = my_el;
            noise_used += ai;
            __syncthreads();
        }
        if (tid < T) ret[tid] = (double)ep_rew[tid];
        n_test_ep += T;
        n_testn += serial ? noise_used : (int64_t)T * nstride;
        for (int te = 0; te < T; ++te) test_steps += tlen[te];
        __syncthreads();
    };

    const float g32 = (float)cfg.gamma;
    // Deterministic time-out (lenv_td3_cfg::step_budget, base_agent.py:30-47): elapsed = env steps taken so far
    const bool budgeted = cfg.step_budget > 0;
    int timed_out_at = -1;
    const bool no_test_env = FIXED ? false : cfg.test_mode == 1;      // BaseAgent.train(env, test_env=None): lenv_ddqn_cfg::test_mode
    bool early_out = false;                               // SEG: the loop ended at the early out
    const int ep_first = SEG ? a.ep_begin : 0, ep_last = SEG ? a.ep_end : cfg.train_episodes;
    for (int episode = ep_first; episode < ep_last; ++episode) {
        if (budgeted && (int64_t)train_steps + test_steps > cfg.step_budget) { timed_out_at = episode; break; }   // uniform
        const bool learning = episode >= cfg.init_episodes;
        // env.reset(): RewardEnv.reset -> real_env.reset() (reward_env.py:141-143)
        for (int i = tid; i < SD; i += DNT) {
            double v;
            if (tape) { if (episode >= a.tapes.train_reset_stride) { status = -5; v = 0.0; } else v = a.tapes.train_reset[(chain * a.tapes.train_reset_stride + episode) * SD + i]; }
            else v = EnvT::reset_word(key, STREAM_TRAIN_RESET, (int64_t)episode, i);
            xs_d[i] = v;
        }
        __syncthreads();
        if (tid < S) state[tid] = EnvT::obs(tid, xs_d);
        __syncthreads();
        if (!virtual_env && (rtype == 1 || rtype == 2)) rn_eval(state, nullptr, 12);   // phi(s) of the reset state (carried from step to step)
        int ep_len = 0, env_steps = 0;
        float tr_reward = 0.0f;                                  // base_agent.py:102,121 episode_reward += reward (fp32 tensors; uniform over the threads)
        for (int t = 0; t < cfg.max_steps; t += k_rep) {         // base_agent.py:104 range(0, max_steps, same_action_num)
            const int size_after = train_steps + 1 < rb_cap ? train_steps + 1 : rb_cap;
            const int new_pos = train_steps % rb_cap;
            // ---- select_train_action (TD3.py:118-124) ----
            if (!learning) {
                if (tid < A) {
                    float v;
                    if (tape) { if (n_rand >= a.tapes.rand_action_stride) { status = -3; v = 0.0f; } else v = a.tapes.rand_action[(chain * a.tapes.rand_action_stride + n_rand) * A + tid]; }
                    else v = (float)(-(double)ma + (2.0 * (double)ma) * u64_to_unit(rng_u64(key, STREAM_TD3_RAND_ACTION, (uint64_t)(n_rand * A + tid))));   // action_space.sample()
                    action[tid] = v;
                }
                ++n_rand;
                __syncthreads();
            } else {
                actor_row1(params, state, action);
                if (tid < A) {
                    float zn;
                    if (tape) { if (n_actn >= a.tapes.act_noise_stride) { status = -7; zn = 0.0f; } else zn = a.tapes.act_noise[(chain * a.tapes.act_noise_stride + n_actn) * A + tid]; }
                    else zn = (float)det_normal(key, STREAM_TD3_ACT_NOISE, (uint64_t)(n_actn * A + tid));
                    const float v = action[tid] + (zn * (float)cfg.action_std) * ma;
                    action[tid] = v < -ma ? -ma : (v > ma ? ma : v);
                }
                ++n_actn;
                __syncthreads();
            }
            T3D_ENV_SUB(12);                               // select_train_action
            if (virtual_env) {
                // ---- EnvWrapper.step -> VirtualEnv.step (virtual_env.py:43-54): the three SE nets on cat(action, state) as queued
                // single-row products; reward / done see the pre-transition state; the learned done flag ends the episode ----
                // EnvWrapper.step repeats the SE step same_action_num times whatever the done flag says and sums the fp32 rewards
                // (env_wrapper.py:24-29)
                float *xse = arena + a.a_xse, *nse = arena + a.a_nse;
                if (tid < A) xse[tid] = action[tid];
                if (tid >= 64 && tid < 64 + S) xse[A + tid - 64] = state[tid - 64];
                if (tid >= 128 && tid < 128 + S) newrow[tid - 128] = state[tid - 128];
                if (tid >= 192 && tid < 192 + A) newrow[S + tid - 192] = action[tid - 192];
                __syncthreads();
                for (int r_ = 0; r_ < k_rep; ++r_) {
                    se_rows(xse, nse);
                    if (tid < S) { newrow[S + A + tid] = nse[tid]; xse[A + tid] = nse[tid]; }
                    if (tid == 64) { newrow[2 * S + A] = r_ == 0 ? nse[S] : newrow[2 * S + A] + nse[S]; newrow[2 * S + A + 1] = nse[S + 1]; }
                    if (r_ + 1 < k_rep) __syncthreads();
                }
            } else {
            // ---- EnvWrapper.step -> RewardEnv.step -> real_env.step + TimeLimit, same_action_num times or until done; the shaped
            // rewards of the repeats are summed as python floats (env_wrapper.py:56-61); `state` follows the repeats ----
            if (tid < S) newrow[tid] = state[tid];
            if (tid >= 64 && tid < 64 + A) newrow[S + tid - 64] = action[tid - 64];
            double rsum = 0.0;
            for (int r_ = 0; r_ < k_rep; ++r_) {
            double nx = 0.0, pre = 0.0;
            if (tid < SD) nx = EnvT::step_word(tid, xs_d, action);
            if (tid == 64) pre = EnvT::reward_pre(xs_d, action);                  // the part of the reward that sees the OLD state
            __syncthreads();
            if (tid < SD) xs_d[tid] = nx;
            if (tid == 64) xs_d[18] = pre;
            __syncthreads();
            ++env_steps;
            const bool dn = EnvT::done(xs_d) || env_steps >= cfg.max_steps;      // the env's own flag or TimeLimit (uniform)
            if (tid < S) newrow[S + A + tid] = EnvT::obs(tid, xs_d);
            float *info = newrow + 2 * S + A + 4;          // [4] info vector of this step (fp32, as torch.tensor(list(info.values())))
            if constexpr (EnvT::INFO == 4) {
                if (tid == 64 && rtype >= 3) {
                    info[0] = (float)xs_d[0]; info[1] = (float)xs_d[8]; info[2] = (float)xs_d[8]; info[3] = (float)(-0.1 * xs_d[18]);
                }
            }
            __syncthreads();
            if (rtype == 3 || rtype == 4) rn_eval(state, info, 12);                  // phi([s | info]): not cacheable, info is this step's
            rn_eval(newrow + S + A, info, 13);             // phi(s') / phi([s' | info]) / w . info
            if (tid == 0) {
                const double rew = EnvT::reward_post(xs_d, xs_d[18]);
                const float r32 = (float)rew, phi_s = ctrl[12], phi_s2 = ctrl[13];
                float shaped;                              // RewardEnv._calc_reward (reward_env.py:81-131)
                switch (rtype) {
                case 0: shaped = r32; break;
                case 1: case 3: shaped = g32 * phi_s2 - phi_s; break;
                case 2: case 4: shaped = (r32 + g32 * phi_s2) - phi_s; break;
                case 5: case 7: case 101: shaped = phi_s2; break;
                default: shaped = r32 + phi_s2; break;     // 6, 8, 102
                }
                rsum = rsum + (double)shaped;
                newrow[2 * S + A] = (float)rsum; newrow[2 * S + A + 1] = dn ? 1.0f : 0.0f;
                ctrl[12] = phi_s2;
            }
            __syncthreads();
            if (tid < S) state[tid] = newrow[S + A + tid];                           // RewardEnv.state = next_state
            if (dn) break;
            if (r_ + 1 < k_rep) __syncthreads();
            }
            }
            __syncthreads();
            T3D_ENV_SUB(13);                               // the env step(s)
            if (tid < 2 * S + A + 2) rb[(int64_t)new_pos * RS + tid] = newrow[tid];
            if (!FIXED && a.out.trace_reward && train_steps < a.out.trace_cap) {
                const int64_t k = chain * a.out.trace_cap + train_steps;
                if (tid < S) { a.out.trace_state[k * S + tid] = newrow[tid]; a.out.trace_next_state[k * S + tid] = newrow[S + A + tid]; }
                if (tid < A) a.out.trace_action[k * A + tid] = newrow[S + tid];
                if (tid == 0) a.out.trace_reward[k] = newrow[2 * S + A];
            }
            const float done_now = newrow[2 * S + A + 1];
            tr_reward = tr_reward + newrow[2 * S + A];
            __syncthreads();
            if (tid < S) state[tid] = newrow[S + A + tid];
            ep_len += k_rep; ++train_steps;                  // base_agent.py:122: episode_length += same_action_num
            __syncthreads();

            T3D_ENV_SUB(14);                               // append + trace + bookkeeping
            PT_MARK(0);                                   // act + env step + reward net + append
            if (learning) {
                // ================= TD3.learn (TD3.py:63-116) =================
                for (int b = tid; b < B; b += DNT) {
                    const int64_t n = learn_it * B + b;
                    int idx;
                    if (tape) {
                        if (n >= a.tapes.replay_idx_stride) { status = -4; idx = 0; } else idx = a.tapes.replay_idx[chain * a.tapes.replay_idx_stride + n];
                        if (idx < 0 || idx >= size_after) { status = -6; idx = 0; }
                    } else idx = (int)rng_replay_below(key, (uint64_t)n, (uint32_t)size_after);
                    const float *row = rb + (int64_t)idx * RS;
                    for (int i = 0; i < SA; ++i) xc[b * SA + i] = row[i];                  // [s, a]
                    for (int i = 0; i < S; ++i) xn[b * SA + i] = row[S + A + i];           // s' (action part filled below)
                    rr[b] = row[2 * S + A]; dd[b] = row[2 * S + A + 1];
                }
                __syncthreads();
                if constexpr (ICM) {                     // TD3.py:68-70: icm.train, then rewards += intrinsic rewards
                    IcmStep st{ gq, Ps, Qs, arena, a.a_icm, ctrl, 20, icm, icm_pows, cfg.icm_lr, cfg.icm_beta, cfg.icm_eta, cfg.adam_beta1,
                                cfg.adam_beta2, cfg.adam_eps, B, xc, SA, xn, SA, /*continuous=*/true };
                    icm_train_and_reward<T3_MAXI>(st, [&](int b, int i) { return xc[b * SA + S + i]; }, [&](int b, float r) { rr[b] = rr[b] + r; });
                }
                PT_MARK(1);                               // replay gather
                if constexpr (DIRECT) {
                    // ================= TD3.learn, DIRECT (t3_direct_critics / t3_direct_actor above the kernel) =================
                    // the context record sits behind the work areas in the queue's staging buffers (which the test phases' products overwrite):
                    // thread 0 writes it at every learn step
                    const T3DirectLayout dl = t3d_layout(S, A, H, B);
                    T3DirectCtx *dctx = reinterpret_cast<T3DirectCtx *>(Ps + dl.ctx);
                    if (tid == 0) {
                        T3DirectCtx d;
                        d.params = params; d.targets = targets; d.grad = grad; d.xc = xc; d.xn = xn;
                        d.l_act = Ps; d.l_x = Ps + dl.x; d.l_na = Ps + dl.na; d.l_w = Ps + dl.w;
                        d.rr = rr; d.dd = dd; d.q1 = q1; d.q2 = q2; d.tq1 = tq1; d.tq2 = tq2; d.dq1 = dq1; d.dq2 = dq2;
                        d.policy_noise = tape ? a.tapes.policy_noise + chain * a.tapes.policy_noise_stride * A : nullptr;
                        d.policy_noise_rows = tape ? a.tapes.policy_noise_stride : 0;
                        d.H = H; d.B = B; d.act_id = act_id; d.Pa = Pa; d.Pc = Pc;
                        d.prelu = prelu; d.ma = ma; d.g32 = g32; d.policy_std = (float)cfg.policy_std; d.policy_clip = (float)cfg.policy_std_clip;
                        d.key = key;
                        *dctx = d;
                    }
                    __syncthreads();
                    // (the routines carry the activation as a template parameter: one uniform switch per call instead of one per hidden unit;
                    // an agent PReLU is refused by inner_check)
                    int dbad = 0;
                    switch (act_id) {
                    case LENV_ACT_RELU: dbad = t3_direct_critics<S, A, LENV_ACT_RELU>(dctx, learn_it); break;
                    case LENV_ACT_LEAKYRELU: dbad = t3_direct_critics<S, A, LENV_ACT_LEAKYRELU>(dctx, learn_it); break;
                    case LENV_ACT_TANH: dbad = t3_direct_critics<S, A, LENV_ACT_TANH>(dctx, learn_it); break;
                    default: dbad = t3_direct_critics<S, A, LENV_ACT_IDENTITY>(dctx, learn_it); break;
                    }
                    if (dbad) status = -8;
                    PT_MARK(5);
                    adam(Pa, 2 * Pc, 0);                       // critic_optimizer: critic_1 then critic_2 parameters
                    PT_MARK(6);
                    ++learn_it;
                    if (learn_it % policy_delay == 0) {
                        switch (act_id) {
                        case LENV_ACT_RELU: t3_direct_actor<S, A, LENV_ACT_RELU>(dctx); break;
                        case LENV_ACT_LEAKYRELU: t3_direct_actor<S, A, LENV_ACT_LEAKYRELU>(dctx); break;
                        case LENV_ACT_TANH: t3_direct_actor<S, A, LENV_ACT_TANH>(dctx); break;
                        default: t3_direct_actor<S, A, LENV_ACT_IDENTITY>(dctx); break;
                        }
                        PT_MARK(7);                           // policy update: forwards + backwards
                        adam(0, Pa, 2);
                        const float tau = (float)cfg.tau, omt = (float)(1.0 - cfg.tau);
                        wg_polyak(params, targets, P, tau, omt);
                        __syncthreads();
                        PT_MARK(8);                           // actor adam + polyak
                    }
                } else {
                // next_actions = (actor_target(s') + clamp(randn*policy_std)).clamp(-max, max)
                mlp_forward(targets, mo_actor, xn, SA, B, ht, xn, SA, S, true, nullptr);
                gq.run<T3_MAXI>(Ps, Qs);
                for (int e = tid; e < B * A; e += DNT) {
                    const int b = e / A, k = e - b * A;
                    const int64_t n = (learn_it * B + b) * A + k;
                    float zn;
                    if (tape) { if (n >= a.tapes.policy_noise_stride * A) { status = -8; zn = 0.0f; } else zn = a.tapes.policy_noise[chain * a.tapes.policy_noise_stride * A + n]; }
                    else zn = (float)det_normal(key, STREAM_TD3_POLICY_NOISE, (uint64_t)n);
                    float nz = zn * (float)cfg.policy_std;
                    const float clipv = (float)cfg.policy_std_clip;
                    nz = nz < -clipv ? -clipv : (nz > clipv ? clipv : nz);
                    const float v = xn[b * SA + S + k] + nz;
                    xn[b * SA + S + k] = v < -ma ? -ma : (v > ma ? ma : v);
                }
                __syncthreads();
                PT_MARK(2);                               // actor_target forward + smoothing noise
                mlp_forward(targets + Pa, mo_critic, xn, SA, B, ht, tq1, 1, 0, false, nullptr);
                mlp_forward(targets + Pa + Pc, mo_critic, xn, SA, B, ht, tq2, 1, 0, false, nullptr);
                mlp_forward(params + Pa, mo_critic, xc, SA, B, hc1, q1, 1, 0, false, nullptr, -1, 0.25f, xh1, rstd1);
                mlp_forward(params + Pa + Pc, mo_critic, xc, SA, B, hc2, q2, 1, 0, false, nullptr, -1, 0.25f, xh2, rstd2);
                gq.run<T3_MAXI>(Ps, Qs);                   // 4 critic forwards, one call
                PT_MARK(3);
                {
                    const float norm = (float)(2.0 / (double)B);
                    for (int b = tid; b < B; b += DNT) {
                        const float tq = tq1[b] < tq2[b] ? tq1[b] : tq2[b];
                        const float y = rr[b] + ((1.0f - dd[b]) * g32) * tq;       // rewards + (1 - dones) * gamma * target_Q
                        dq1[b] = norm * (q1[b] - y);
                        dq2[b] = norm * (q2[b] - y);
                    }
                }
                __syncthreads();
                PT_MARK(4);                               // TD error
                mlp_backward(params + Pa, mo_critic, xc, SA, B, hc1, dq1, grad + Pa, nullptr, xh1, rstd1);
                mlp_backward(params + Pa + Pc, mo_critic, xc, SA, B, hc2, dq2, grad + Pa + Pc, nullptr, xh2, rstd2);
                gq.run<T3_MAXI>(Ps, Qs);
                PT_MARK(5);                               // critics backward
                adam(Pa, 2 * Pc, 0);                       // critic_optimizer: critic_1 then critic_2 parameters
                PT_MARK(6);
                ++learn_it;
                if (learn_it % policy_delay == 0) {
                    // actor_loss = (-critic_1(states, actor(states))).mean() with the updated critic_1
                    for (int e = tid; e < B * S; e += DNT) { const int b = e / S, i = e - b * S; xa[b * SA + i] = xc[b * SA + i]; }
                    __syncthreads();
                    mlp_forward(params, mo_actor, xc, SA, B, ha, xa, SA, S, true, thb, -1, 0.25f, xha, rstda);
                    mlp_forward(params + Pa, mo_critic, xa, SA, B, hc1, q1, 1, 0, false, nullptr, -1, 0.25f, xh1, rstd1);
                    gq.run<T3_MAXI>(Ps, Qs);
                    const float dqa = -(1.0f / (float)B);
                    for (int b = tid; b < B; b += DNT) dq1[b] = dqa;
                    __syncthreads();
                    mlp_backward(params + Pa, mo_critic, xa, SA, B, hc1, dq1, nullptr, dxb, xh1, rstd1);
                    gq.run<T3_MAXI>(Ps, Qs);
                    for (int e = tid; e < B * A; e += DNT) {
                        const int b = e / A, k = e - b * A;
                        const float th = thb[e];
                        dzb[e] = (dxb[b * SA + S + k] * ma) * fma32(-th, th, 1.0f);   // d(tanh(z)*max_action)
                    }
                    __syncthreads();
                    mlp_backward(params, mo_actor, xc, SA, B, ha, dzb, grad, nullptr, xha, rstda);
                    gq.run<T3_MAXI>(Ps, Qs);
                    PT_MARK(7);                           // policy update: forwards + backwards
                    adam(0, Pa, 2);
                    const float tau = (float)cfg.tau, omt = (float)(1.0 - cfg.tau);
                    wg_polyak(params, targets, P, tau, omt);
                    __syncthreads();
                    PT_MARK(8);                           // actor adam + polyak
                }
                }       // (the queued learn step)
            }
            if (done_now > 0.5f) break;
        }
        ++episodes_run;
        if (tid == 0 && a.out.episode_len) a.out.episode_len[chain * cfg.train_episodes + episode] = ep_len;
        __syncthreads();
        PT_MARK(10);
        if (!no_test_env) test_phase();                    // per-episode test on the real env (base_agent.py:134-136)
        PT_MARK(9);
        if (tid == 0) {
            double tm;
            if (no_test_env) tm = (double)tr_reward;       // train(env, test_env=None): avg_meter_reward.update(episode_reward) (base_agent.py:138)
            else {
                double sm = 0.0;
                for (int i = 0; i < T; ++i) sm += ret[i];
                tm = sm / (double)T;
            }
            meter[episode] = tm;
            if (a.out.episode_test_mean) a.out.episode_test_mean[chain * cfg.train_episodes + episode] = tm;
            // early out (base_agent.py:49-62,141-148): break_env = the test env (real rule) or, without one, the training env itself
            ictrl[3] = learning && meter_env_solved(meter, episode + 1, cfg.early_out_num, no_test_env && (virtual_env), cfg.solved_reward,
                                                    cfg.early_out_virtual_diff, episode, cfg.init_episodes);
        }
        __syncthreads();
        const int brk = ictrl[3];
        __syncthreads();
        if (brk) { if constexpr (SEG) early_out = true; break; }
    }
    if constexpr (SEG) {
        if (!early_out && timed_out_at < 0 && a.ep_end < cfg.train_episodes) {
            // the chain goes on in the next segment: a checkpoint (cumulative stats, the parameters so far) and the record
            int *st_fold = reinterpret_cast<int *>(misc + MISC_STATUS_FOLD);     // the minimum of the threads' status codes (0 after the clear of misc)
            if (status != 0) { atomicMin(st_fold, status); if (a.out.status) atomicMin(&a.out.status[chain], status); }
            if (a.out.final_params) for (int p = tid; p < P; p += DNT) a.out.final_params[chain * a.P + p] = params[p];
            __syncthreads();
            if (tid == 0) {
                if (a.out.stats) {
                    a.out.stats[chain * 4 + 0] = episodes_run; a.out.stats[chain * 4 + 1] = train_steps;
                    a.out.stats[chain * 4 + 2] = learn_it; a.out.stats[chain * 4 + 3] = test_steps;
                }
                td3_write_record(rec, a.ep_end, 0, *st_fold, timed_out_at, n_rand, n_actn, n_testn, n_test_ep, learn_it, train_steps, test_steps,
                                 episodes_run, pows, icm_pows);
            }
            return;
        }
    }
    PT_MARK(10);
    const int64_t remaining = cfg.step_budget - ((int64_t)train_steps + test_steps);     // time_remaining - elapsed
    const int test_before = test_steps;
    test_phase();
    if (budgeted) {
        // BaseAgent.test under the time-out (base_agent.py:177-184): episode e (tlen[e] env steps) starts only
        // while the earlier ones used <= remaining steps, the rest is padded with the minimum so far (-1e9 if empty)
        int64_t used = 0;
        int stop = T;
        for (int te = 0; te < T; ++te) {
            if (used > remaining) { stop = te; break; }
            used += tlen[te];
        }
        if (tid == 0) {
            double mn = -1e9;
            if (stop > 0) { mn = ret[0]; for (int i = 1; i < stop; ++i) if (ret[i] < mn) mn = ret[i]; }
            for (int te = stop; te < T; ++te) ret[te] = mn;
        }
        test_steps = test_before + (int)used;
        __syncthreads();
    }
    PT_MARK(9);
#ifdef LENV_PHASE_TIMING
    if (tid == 0 && chain == 0) for (int pi = 0; pi < 12; ++pi) g_td3_phase_cycles[pi] = pt_acc[pi];
#endif
    if (tid == 0) {
        double sm = 0.0;
        for (int i = 0; i < T; ++i) sm += ret[i];
        a.out.score[chain] = sm / (double)T;
        if (a.out.final_returns) for (int i = 0; i < T; ++i) a.out.final_returns[chain * T + i] = ret[i];
        if (a.out.stats) {
            a.out.stats[chain * 4 + 0] = episodes_run; a.out.stats[chain * 4 + 1] = train_steps;
            a.out.stats[chain * 4 + 2] = learn_it; a.out.stats[chain * 4 + 3] = test_steps;
        }
        // episodes that never ran: NaN / 0, or -- after a time-out -- time_is_up's padding (base_agent.py:33-44)
        double pad_r = __builtin_nan("");
        int pad_l = 0;
        if (timed_out_at >= 0) {
            pad_r = -1e9; pad_l = 1000000000;
            if (episodes_run > 0) { pad_r = meter[0]; for (int i = 1; i < episodes_run; ++i) if (meter[i] < pad_r) pad_r = meter[i]; }
            if (episodes_run > 0 && a.out.episode_len) {
                pad_l = a.out.episode_len[chain * cfg.train_episodes];
                for (int i = 1; i < episodes_run; ++i) { const int l = a.out.episode_len[chain * cfg.train_episodes + i]; if (l > pad_l) pad_l = l; }
            }
        }
        for (int e = episodes_run; e < cfg.train_episodes; ++e) {
            if (a.out.episode_test_mean) a.out.episode_test_mean[chain * cfg.train_episodes + e] = pad_r;
            if (a.out.episode_len) a.out.episode_len[chain * cfg.train_episodes + e] = pad_l;
        }
    }
    if (a.out.final_params) for (int p = tid; p < P; p += DNT) a.out.final_params[chain * a.P + p] = params[p];
    if constexpr (ICM) {
        if (a.icm_final) for (int p = tid; p < icm.P; p += DNT) a.icm_final[chain * a.P_icm + p] = arena[a.a_icm[IB_P] + p];
    }
    if (a.out.status && status != 0) atomicMin(&a.out.status[chain], status);
    if constexpr (SEG) {
        int *st_fold = reinterpret_cast<int *>(misc + MISC_STATUS_FOLD);
        if (status != 0) atomicMin(st_fold, status);
        __syncthreads();
        if (tid == 0) td3_write_record(rec, a.ep_end, 1, *st_fold, timed_out_at, n_rand, n_actn, n_testn, n_test_ep, learn_it, train_steps, test_steps,
                                       episodes_run, pows, icm_pows);
    }
}

// Fresh TD3 agents (actor | critic_1 | critic_2, TD3.py:31-39) for chains with their own network shapes: nn.Linear's default
// init, drawn like lenv_nes_draw (see dueling_agent_init_kernel)
__global__ void td3_agent_init_kernel(lenv_td3_cfg cfg, const int32_t *hp_hidden, const int32_t *hp_layers, const uint64_t *rng_keys,
                                      int64_t chains, int64_t row_stride, float *agent_init)
{
    const int64_t c = blockIdx.y;
    if (c >= chains) return;
    const int H = hp_hidden ? hp_hidden[c] : cfg.hidden, L = hp_layers ? hp_layers[c] : cfg.layers;
    if (H < 1 || H > cfg.hidden || L < 1 || L > cfg.layers) return;            // the inner loop reports status -8 for this chain
    MlpOff ma, mc;
    const int T3_S = cfg.state_dim, T3_A = cfg.action_dim, T3_SA = T3_S + T3_A;
    mlp_off(ma, T3_S, H, L, T3_A, cfg.use_layer_norm != 0);
    mlp_off(mc, T3_SA, H, L, 1, cfg.use_layer_norm != 0);
    const int P = ma.P + 2 * mc.P;
    const uint64_t key = rng_keys[c];
    const float bS = (float)(1.0 / __builtin_sqrt((double)T3_S)), bSA = (float)(1.0 / __builtin_sqrt((double)T3_SA)),
                bH = (float)(1.0 / __builtin_sqrt((double)H));
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < P; i += gridDim.x * blockDim.x) {
        float bound;
        {   // nn.LayerNorm: weight 1, bias 0
            const MlpOff &mo = i < ma.P ? ma : mc;
            const int j = i < ma.P ? i : (i - ma.P) % mc.P;
            if (mo.ln && j >= mo.oLN && j < mo.oLN + 2 * H) { agent_init[c * row_stride + i] = j < mo.oLN + H ? 1.0f : 0.0f; continue; }
        }
        if (i < ma.P) bound = i < ma.oW[1] ? bS : bH;
        else { const int j = (i - ma.P) % mc.P; bound = j < mc.oW[1] ? bSA : bH; }
        const float u = (float)u64_to_unit(rng_u64(key, STREAM_AGENT_INIT, (uint64_t)i));
        agent_init[c * row_stride + i] = (u * 2.0f - 1.0f) * bound;
    }
}

}  // namespace lenv

using namespace lenv;

static int td3_layout(const lenv_td3_cfg *cfg, Td3Args &a, size_t *lds_bytes)
{
    const int H = cfg->hidden, L = cfg->layers, B = cfg->batch_size, T = cfg->test_episodes, Hrn = cfg->rn_hidden;
    const int T3_S = cfg->state_dim, T3_A = cfg->action_dim, T3_SA = T3_S + T3_A;
    if (!((cfg->env_id == LENV_ENV_CHEETAH_STANDIN && T3_S == 17 && T3_A == 6) || (cfg->env_id == LENV_ENV_PENDULUM && T3_S == 3 && T3_A == 1) ||
          (cfg->env_id == LENV_ENV_CMC && T3_S == 2 && T3_A == 1)))
        return LENV_ERR_UNSUPPORTED;
    if (cfg->same_action_num < 0 || cfg->same_action_num > 64) return LENV_ERR_UNSUPPORTED;
    const int t = cfg->reward_env_type;
    if (!((t >= 0 && t <= 8) || t == 101 || t == 102)) return LENV_ERR_UNSUPPORTED;          // reward_env.py:49,58 NotImplementedError
    if (cfg->act == LENV_ACT_PRELU) return LENV_ERR_UNSUPPORTED;   // trained PReLU slope of the agent nets: not a parameter here yet
    const bool uses_info = t == 3 || t == 4 || t == 7 || t == 8 || t > 100;
    if (uses_info && cfg->info_dim != 4) return LENV_ERR_INVALID;                              // the stand-in's info vector has 4 entries
    if (uses_info && cfg->env_id != LENV_ENV_CHEETAH_STANDIN) return LENV_ERR_INVALID;         // Pendulum's step returns an empty info dict
    if (L < 1 || L > T3_MAXL || H < 1 || H > T3_MAXW || B < 1 || B > T3_MAXB || T < 1 || T * T3_S > DNT || cfg->rn_layers < 1 || cfg->rn_layers > T3_MAXL || Hrn > T3_MAXW || Hrn < 1 ||
        cfg->policy_delay < 1 || cfg->max_steps < 1 || cfg->train_episodes < 0)
        return LENV_ERR_UNSUPPORTED;
    mlp_off(a.actor, T3_S, H, L, T3_A, cfg->use_layer_norm != 0);
    mlp_off(a.critic, T3_SA, H, L, 1, cfg->use_layer_norm != 0);
    a.P = a.actor.P + 2 * a.critic.P;
    a.P_rn = (int)lenv_rn_num_params(t, T3_S, cfg->info_dim, Hrn, cfg->rn_layers);
    a.P_rn_lds = cfg->rn_layers > 1 ? 0 : a.P_rn;             // deeper reward nets are staged in the arena
    if (cfg->virtual_env) {
        MlpOff m;
        mlp_off(m, T3_SA, Hrn, cfg->rn_layers, T3_S); a.P_rn = m.P;
        mlp_off(m, T3_SA, Hrn, cfg->rn_layers, 1); a.P_rn += 2 * m.P;
        a.P_rn_lds = 0;
    }
    a.RS = (2 * T3_S + T3_A + 2 + 3) & ~3;
    int64_t cap = (int64_t)cfg->train_episodes * cfg->max_steps;
    if (cap > cfg->rb_size) cap = cfg->rb_size;
    a.rb_cap = cap < 1 ? 1 : cap;
    const int RB = B > T ? B : T;                               // rows of the batch buffers
    lenv_host::ArenaCursor c;
    a.a_params = c.take(a.P); a.a_targets = c.take(a.P); a.a_m = c.take(a.P); a.a_v = c.take(a.P); a.a_grad = c.take(a.P);
    a.a_replay = c.take(a.rb_cap * a.RS);
    a.a_xc = c.take((int64_t)RB * T3_SA); a.a_xn = c.take((int64_t)RB * T3_SA); a.a_xa = c.take((int64_t)RB * T3_SA);
    for (int l = 0; l < T3_MAXL; ++l) { a.a_hc1[l] = c.take((int64_t)RB * H); a.a_hc2[l] = c.take((int64_t)RB * H); a.a_ha[l] = c.take((int64_t)RB * H); a.a_ht[l] = c.take((int64_t)RB * H); }
    a.a_d[0] = c.take((int64_t)RB * H); a.a_d[1] = c.take((int64_t)RB * H);
    a.a_dx = c.take((int64_t)RB * T3_SA); a.a_act = c.take((int64_t)RB * T3_A); a.a_th = c.take((int64_t)RB * T3_A); a.a_dz = c.take((int64_t)RB * T3_A);
    a.a_meter = c.take(2 * (int64_t)(cfg->train_episodes > 0 ? cfg->train_episodes : 1));
    {   // use_layer_norm: normalised rows / 1 / sqrt(var + eps) of the LayerNorm positions of the passes that are differentiated
        const bool ln = a.actor.ln != 0;
        for (int n = 0; n < 3; ++n) for (int l = 0; l < T3_MAXL; ++l) a.a_xh[n][l] = c.take(ln && l >= 1 && l < L ? (int64_t)RB * H : 0);
        a.a_rstd = c.take(ln ? 3 * (int64_t)T3_MAXL * B : 0);
    }
    a.a_se = a.a_seT = a.a_xse = a.a_nse = 0;
    if (cfg->virtual_env) {
        if ((int64_t)RB * H < Hrn) return LENV_ERR_UNSUPPORTED;          // the SE's hidden rows reuse the agent's temporaries
        a.a_se = c.take(a.P_rn); a.a_seT = c.take(a.P_rn); a.a_xse = c.take(T3_SA); a.a_nse = c.take(T3_S + 2);
    } else if (cfg->rn_layers > 1) a.a_se = c.take(a.P_rn);
    a.P_icm = 0;
    for (int i = 0; i < IB_COUNT; ++i) a.a_icm[i] = 0;
    if (cfg->icm_enabled) {
        if (cfg->icm_feature_dim < 1 || cfg->icm_feature_dim > 128 || cfg->icm_hidden < 1 || cfg->icm_hidden > 128) return LENV_ERR_UNSUPPORTED;
        IcmNet n;
        icm_build(n, T3_S, T3_A, cfg->icm_feature_dim, cfg->icm_hidden, /*discrete=*/false);
        a.P_icm = n.P;
        int64_t sz[IB_COUNT];
        icm_buffer_sizes(n, B, sz);
        for (int i = 0; i < IB_COUNT; ++i) a.a_icm[i] = c.take(sz[i]);
    }
    a.arena_stride = c.total();
    if (lenv_wc_td3_shape(cfg)) {                             // the wave-chain kernel (td3_wavechain.hip) keeps its own arena layout
        const int64_t wfl = lenv_wc_td3_arena_floats(cfg, a.rb_cap, a.RS);
        if (wfl > a.arena_stride) a.arena_stride = wfl;
    }
    const size_t lds_floats = GemmShape<T3_MAXI>::PS_FLOATS + GemmShape<T3_MAXI>::QS_FLOATS + GEMM_QUEUE_MAX * sizeof(GemmCmd) / sizeof(float) + ((a.P_rn_lds + 3) & ~3) + 2 * ((Hrn + 3) & ~3) + 8 * (size_t)B + 64 + 2 + 2 * (20 + 17 * (size_t)T + T) + 3 * (size_t)T + 20 + 8 + 56 + 16;
    *lds_bytes = lds_floats * sizeof(float);
    if (*lds_bytes > 160 * 1024) return LENV_ERR_UNSUPPORTED;
    return LENV_OK;
}

extern "C" size_t lenv_td3_rn_workspace_bytes(const lenv_td3_cfg *cfg, int64_t chains)
{
    if (!cfg || chains < 0) return 0;
    Td3Args a;
    size_t lds;
    if (td3_layout(cfg, a, &lds) != LENV_OK) return 0;
    return (size_t)chains * a.arena_stride * sizeof(float) + 256;
}

extern "C" int lenv_td3_rn_team_size(const lenv_td3_cfg *cfg, int64_t chains)
{
    if (!cfg || chains < 1) return LENV_ERR_INVALID;
    if ((cfg->kernel_variant & (LENV_VARIANT_NO_WAVECHAIN | LENV_VARIANT_GENERIC)) || cfg->icm_enabled || cfg->rng_mode != LENV_RNG_COUNTER || !lenv_wc_td3_shape(cfg)) return 1;
    return lenv_wc_td3_team(cfg, chains);
}

extern "C" int64_t lenv_td3_num_params(const lenv_td3_cfg *cfg, int64_t *actor_params, int64_t *critic_params)
{
    if (!cfg) return LENV_ERR_INVALID;
    Td3Args a;
    size_t lds;
    const int rc = td3_layout(cfg, a, &lds);
    if (rc != LENV_OK) return rc;
    if (actor_params) *actor_params = a.actor.P;
    if (critic_params) *critic_params = a.critic.P;
    return a.P;
}

extern "C" int lenv_td3_rn_inner_loop(const lenv_td3_cfg *cfg, const float *theta, const float *eps, const int32_t *worker,
                                      const float *sign, const float *agent_init, const uint64_t *rng_keys,
                                      const lenv_td3_tapes *tapes, int64_t chains, void *workspace, size_t workspace_bytes,
                                      const lenv_td3_out *out, void *stream)
{
    return lenv_td3_rn_inner_loop_hp(cfg, nullptr, theta, eps, worker, sign, agent_init, rng_keys, tapes, chains, workspace,
                                     workspace_bytes, out, stream);
}

extern "C" int lenv_td3_agent_init_hp(const lenv_td3_cfg *cfg, const lenv_chain_hp *hp, const uint64_t *rng_keys, int64_t chains,
                                      float *agent_init, void *stream)
{
    if (!cfg || !rng_keys || !agent_init || chains < 0) return LENV_ERR_INVALID;
    if (hp && (!hp->q_hidden || !hp->q_layers)) return LENV_ERR_INVALID;
    if (chains == 0) return LENV_OK;
    Td3Args a;
    size_t lds_bytes;
    const int rc = td3_layout(cfg, a, &lds_bytes);
    if (rc != LENV_OK) return rc;
    hipLaunchKernelGGL(td3_agent_init_kernel, dim3(64, (unsigned)chains), dim3(256), 0, static_cast<hipStream_t>(stream), *cfg,
                       hp ? hp->q_hidden : nullptr, hp ? hp->q_layers : nullptr, rng_keys, chains, (int64_t)a.P, agent_init);
    return hipGetLastError() == hipSuccess ? LENV_OK : LENV_ERR_LAUNCH;
}

extern "C" int64_t lenv_td3_icm_num_params(const lenv_td3_cfg *cfg)
{
    if (!cfg || !cfg->icm_enabled) return LENV_ERR_INVALID;
    Td3Args a;
    size_t lds;
    const int rc = td3_layout(cfg, a, &lds);
    return rc != LENV_OK ? rc : a.P_icm;
}

extern "C" int lenv_td3_rn_inner_loop_hp(const lenv_td3_cfg *cfg, const lenv_chain_hp *hp, const float *theta, const float *eps,
                                         const int32_t *worker, const float *sign, const float *agent_init, const uint64_t *rng_keys,
                                         const lenv_td3_tapes *tapes, int64_t chains, void *workspace, size_t workspace_bytes,
                                         const lenv_td3_out *out, void *stream)
{
    if (cfg && cfg->icm_enabled) return LENV_ERR_INVALID;              // TD3(icm=True) needs lenv_td3_rn_inner_loop_icm
    return lenv_td3_rn_inner_loop_icm(cfg, hp, nullptr, theta, eps, worker, sign, agent_init, rng_keys, tapes, chains, workspace,
                                      workspace_bytes, out, stream);
}

// the launch behind lenv_td3_rn_inner_loop_icm (segment false: one launch from the first episode to the final test, resume unused) and
// lenv_td3_rn_inner_loop_segment (segment true: episodes [ep_begin, ep_end) on the SEG instantiations of the queued kernel)
static int td3_launch(const lenv_td3_cfg *cfg, const lenv_chain_hp *hp, const lenv_icm_io *icm, const float *theta, const float *eps,
                      const int32_t *worker, const float *sign, const float *agent_init, const uint64_t *rng_keys, const lenv_td3_tapes *tapes,
                      int64_t chains, void *workspace, size_t workspace_bytes, const lenv_td3_out *out, bool segment, int32_t ep_begin,
                      int32_t ep_end, int64_t *resume, void *stream)
{
    const lenv_host::Segment seg{segment, ep_begin, ep_end, resume};
    if (!lenv_host::launch_args_ok(cfg, hp, eps, worker, sign, agent_init, rng_keys, tapes, chains, workspace, out, seg)) return LENV_ERR_INVALID;
    if ((!theta && cfg->reward_env_type != 0) || !lenv_host::icm_args_ok(cfg, icm)) return LENV_ERR_INVALID;
    if (chains == 0) return LENV_OK;
    Td3Args a;
    size_t lds_bytes;
    const int rc = td3_layout(cfg, a, &lds_bytes);
    if (rc != LENV_OK) return rc;
    if (workspace_bytes < (size_t)chains * a.arena_stride * sizeof(float)) return LENV_ERR_WORKSPACE;
    lenv_host::fill_args(a, cfg, theta, eps, worker, sign, agent_init, rng_keys, tapes, workspace, out);
    lenv_host::fill_segment(a, cfg, seg);
    lenv_host::fill_hp(a, hp);
    lenv_host::fill_icm(a, cfg, icm);
    void (*kern)(const Td3Args) = nullptr;
    // narrow one-hidden-layer agent nets (every chain's: cfg carries the maxima of a *_vary launch) without LayerNorm / ICM whose activation
    // matrix fits the idle staging buffers: the DIRECT instantiations (kernel_variant NO_DIRECT keeps the product queue: A/B runs, tests)
    bool direct = false;
    {
        const int S = cfg->state_dim, A = cfg->action_dim, H = cfg->hidden, B = cfg->batch_size;
        const int64_t need = H <= T3_DIRECT_H && B <= T3_DIRECT_B ? t3d_layout(S, A, H, B).total : INT64_MAX;      // activation matrix + rows + two staged nets + the context record
        direct = !segment && !cfg->icm_enabled && !cfg->use_layer_norm && cfg->layers == 1 && H <= T3_DIRECT_H && B <= T3_DIRECT_B && !(cfg->kernel_variant & LENV_VARIANT_NO_DIRECT) &&
                 need <= (int64_t)(GemmShape<T3_MAXI>::PS_FLOATS + GemmShape<T3_MAXI>::QS_FLOATS);
    }
    if (cfg->env_id == LENV_ENV_PENDULUM) kern = cfg->icm_enabled ? td3_rn_inner_kernel<true, LENV_ENV_PENDULUM> : (direct ? td3_rn_inner_kernel<false, LENV_ENV_PENDULUM, 0, true> : td3_rn_inner_kernel<false, LENV_ENV_PENDULUM>);
    else if (cfg->env_id == LENV_ENV_CMC) kern = cfg->icm_enabled ? td3_rn_inner_kernel<true, LENV_ENV_CMC> : (direct ? td3_rn_inner_kernel<false, LENV_ENV_CMC, 0, true> : td3_rn_inner_kernel<false, LENV_ENV_CMC>);
    else kern = cfg->icm_enabled ? td3_rn_inner_kernel<true, LENV_ENV_CHEETAH_STANDIN> : (direct ? td3_rn_inner_kernel<false, LENV_ENV_CHEETAH_STANDIN, 0, true> : td3_rn_inner_kernel<false, LENV_ENV_CHEETAH_STANDIN>);
    if (segment) {
        if (cfg->env_id == LENV_ENV_PENDULUM) kern = cfg->icm_enabled ? td3_rn_inner_kernel<true, LENV_ENV_PENDULUM, 0, false, true> : td3_rn_inner_kernel<false, LENV_ENV_PENDULUM, 0, false, true>;
        else if (cfg->env_id == LENV_ENV_CMC) kern = cfg->icm_enabled ? td3_rn_inner_kernel<true, LENV_ENV_CMC, 0, false, true> : td3_rn_inner_kernel<false, LENV_ENV_CMC, 0, false, true>;
        else kern = cfg->icm_enabled ? td3_rn_inner_kernel<true, LENV_ENV_CHEETAH_STANDIN, 0, false, true> : td3_rn_inner_kernel<false, LENV_ENV_CHEETAH_STANDIN, 0, false, true>;
    } else {
        // the published HalfCheetah RewardEnv + TD3 shape in production form takes the shape-specialised instantiation
        const bool off = (cfg->kernel_variant & LENV_VARIANT_GENERIC) != 0;
        auto matches = [&](const Td3Shape &sp) {
            return cfg->env_id == sp.env && (cfg->virtual_env != 0) == (sp.virtual_env != 0) && (cfg->same_action_num > 1 ? cfg->same_action_num : 1) == sp.k_rep &&
                   cfg->hidden == sp.H && cfg->layers == sp.L && cfg->batch_size == sp.B && cfg->test_episodes == sp.T && cfg->rn_hidden == sp.Hrn &&
                   cfg->rn_layers == sp.rn_layers && cfg->rn_act == sp.rn_act && cfg->reward_env_type == sp.rtype && cfg->act == sp.act &&
                   cfg->policy_delay == sp.policy_delay && !cfg->use_layer_norm && !(cfg->rn_layer_norm && cfg->rn_layers >= 2) && cfg->test_mode == 0;
        };
        // production launches of the cfg-5 shape: the wave-chain kernel (kernel_variant NO_WAVECHAIN keeps the GEMM-queue kernel for A/B runs)
        if (!off && !(cfg->kernel_variant & LENV_VARIANT_NO_WAVECHAIN) && !cfg->icm_enabled && !hp && cfg->rng_mode == LENV_RNG_COUNTER && !out->trace_reward && lenv_wc_td3_shape(cfg)) {
            return lenv_wc_td3_launch(cfg, theta, eps, worker, sign, agent_init, rng_keys, chains, a.arena, a.arena_stride, a.rb_cap, a.RS, a.P, a.actor.P,
                                      a.critic.P, a.P_rn, out, static_cast<hipStream_t>(stream));
        }
        if (!off && !cfg->icm_enabled && !hp && cfg->rng_mode == LENV_RNG_COUNTER && !out->trace_reward) {
            if (matches(kTd3Shapes[1])) kern = td3_rn_inner_kernel<false, LENV_ENV_CHEETAH_STANDIN, 1>;
            else if (matches(kTd3Shapes[2])) kern = td3_rn_inner_kernel<false, LENV_ENV_PENDULUM, 2>;
            else if (matches(kTd3Shapes[3])) kern = td3_rn_inner_kernel<false, LENV_ENV_CMC, 3>;
            else if (matches(kTd3Shapes[4])) kern = td3_rn_inner_kernel<false, LENV_ENV_CMC, 4>;
        }
    }
    return lenv_host::launch(kern, dim3((unsigned)chains), dim3(DNT), lds_bytes, stream, a);
}

extern "C" int lenv_td3_rn_inner_loop_icm(const lenv_td3_cfg *cfg, const lenv_chain_hp *hp, const lenv_icm_io *icm, const float *theta,
                                          const float *eps, const int32_t *worker, const float *sign, const float *agent_init,
                                          const uint64_t *rng_keys, const lenv_td3_tapes *tapes, int64_t chains, void *workspace,
                                          size_t workspace_bytes, const lenv_td3_out *out, void *stream)
{
    return td3_launch(cfg, hp, icm, theta, eps, worker, sign, agent_init, rng_keys, tapes, chains, workspace, workspace_bytes, out, false, 0, 0,
                      nullptr, stream);
}

extern "C" int lenv_td3_rn_inner_loop_segment(const lenv_td3_cfg *cfg, const lenv_chain_hp *hp, const lenv_icm_io *icm, const float *theta,
                                              const float *eps, const int32_t *worker, const float *sign, const float *agent_init,
                                              const uint64_t *rng_keys, const lenv_td3_tapes *tapes, int64_t chains, void *workspace,
                                              size_t workspace_bytes, const lenv_td3_out *out, int32_t episode_begin, int32_t episode_end,
                                              int64_t *resume, void *stream)
{
    return td3_launch(cfg, hp, icm, theta, eps, worker, sign, agent_init, rng_keys, tapes, chains, workspace, workspace_bytes, out, true,
                      episode_begin, episode_end, resume, stream);
}

#ifdef LENV_PHASE_TIMING
namespace lenv { __global__ void td3_phase_dummy() {} }
extern "C" int lenv_debug_td3_phase_cycles(unsigned long long *host_out)
{
    if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(lenv::g_td3_phase_cycles), sizeof(unsigned long long) * 16) != hipSuccess) return -4;
    return hipMemcpyFromSymbol(host_out + 16, HIP_SYMBOL(lenv::g_t3d_sub_cycles), sizeof(unsigned long long) * 16) == hipSuccess ? 0 : -4;      // (callers pass 32 words)
}
#endif
