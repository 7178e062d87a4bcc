// actor_test_population.hip -- BaseAgent.test (agents/base_agent.py:155-227) with TD3.select_test_action (agents/TD3.py:126-129) or PPO's
// actor_old.forward (models/actor_critic.py:45-49) for a whole population of trained continuous-control agents in one launch: agent i runs
// cfg->test_episodes noisy episodes on the real env (the HalfCheetah-v3 stand-in, Pendulum-v0, MountainCarContinuous-v0) and, when asked,
// records every transition it visits -- the replay buffer the reference's test() returns.
//
// The operations are those of the fused loops' closing test (test_phase of td3_rn_inner_loop.hip and of ppo_rn_inner_kernel.inc): reset, the
// actor's forward, the action with its test noise, repeated same_action_num times or until done, TimeLimit at max_steps env steps, the repeats'
// rewards summed in fp64 and rounded once to fp32 onto an fp32 episode return.  Nothing is restated: the physics, the reset draw, the
// observation and the two halves of the reward are ContEnv<ENV> of lenv_device.cuh, the noise is det_normal on the streams the fused kernels
// draw from, the parameter layouts are mlp_off / ppo_mlp (lenv_actor_params.cuh, the final_params rows of the fused entries), the shared
// LayerNorm of a TD3 actor is ln_rows_forward of lenv_ln.cuh, the layer product is at_layer of lenv_at_layer.cuh.  Every dot product is the
// k-ascending fmaf chain from 0, then the bias, then the activation, so the actions carry the bits of the GEMM-queue forward, of the
// wave-chain kernel and of the one-row actor of the PPO kernel.
//   TD3: a = clamp(max_action * tanh(actor(s)) + (z * (float)action_std) * max_action, +-max_action),
//        z = det_normal(key, STREAM_TD3_TEST_NOISE, ((episode_offset + e) * max_steps + agent_step) * A + k)
//   PPO: a = tanh(net(s)) + z * max(action_std, 0.001f) with action_std the first A words of the row (a final_params row carries the trained,
//        unclamped parameter; actor_old's copy differs from it only by this clamp, which its forward applies in place),
//        z = det_normal(key, STREAM_PPO_TEST_NOISE, ((episode_offset + e) * cap + agent_step) * A + k)
// With a noise tape z = noise[agent][e][agent_step][k] and the streams are not drawn.
//
// Grid (agent, block of at most TP_TB episodes), 512 threads.  The episodes of a block advance in lock-step; a finished one idles until the
// block ends.  The fp64 env state is [rows][SD] in LDS and thread (episode, word) steps it (the stand-in has 17 words: 272 threads per
// repeat instead of 16); thread e < rows owns episode e's bookkeeping (reward sum, step counts, the done flag).
// The block's episodes and their alive mask, the dynamic-LDS layout, the staging and the hidden layers are the shared pieces of
// lenv_at_layer.cuh (tp_block, tp_stage_mlp, tp_trunk) and lenv_tp_layout.h (tp_lds_layout); the launch plan is tp_launch_plan of lenv_host.h.  Here W = H rounded
// up to 4, the LayerNorm is a TD3 actor's, and the actor is staged where all of it stays below AC_LDS_LIMIT.  The widest admitted shape (H
// 512, three hidden layers, LayerNorm) takes 2 * 16 * 512 + 16 * 513 floats = 96.1 KiB and is never staged.
// __launch_bounds__(DNT, 4): four waves per SIMD, i.e. at most 128 VGPRs (a scratch frame of up to 100 B per lane).
#include <hip/hip_runtime.h>
#include "../../include/lenv_hip.h"
#include "lenv_gemm.cuh"
#include "lenv_actor_params.cuh"
#include "lenv_ln.cuh"
#include "lenv_at_layer.cuh"
#include "lenv_host.h"

namespace lenv {

constexpr int AC_XLD = 20;                     // row stride of the observation rows (the stand-in's 17, rounded up to 4)
constexpr int AC_ALD = 8;                      // row stride of the action rows (the stand-in's 6)
constexpr int AC_MAXSD = 17;                   // fp64 words of the widest env state
constexpr int AC_LNBUF = TP_TB * (T3_MAXW | 1);     // ln_rows_forward: every row of a block in one chunk
// The actor is staged where the workgroup's LDS stays within half a CU's 160 KiB: two workgroups then share a CU (the kernel is held to 128
// VGPRs for the same reason), which for a population larger than the 256 CUs is worth more than the staged weights (measured: 400 agents
// 17-128-128-6, 25.7 ms read from global memory two to a CU against 37.9 ms staged one to a CU; one to a CU the staged form is 7 % faster).
constexpr size_t AC_LDS_LIMIT = 80 * 1024 - 8192;   // dynamic bytes of a staged launch, next to the static arrays below (4.7 KiB)

struct AcArgs {
    int kind, H, L, act, ln, T, max_steps, k_rep, cap;
    float ma, astd;                            // TD3: (float)max_action, (float)action_std
    int P, oAct, Pa, W;                        // row stride of params, the actor's place in a row and its parameter count; activation row stride
    int oW[T3_MAXL + 1], ob[T3_MAXL + 1], oLN; // offsets inside the actor (mlp_off / ppo_mlp)
    const float *params; const uint64_t *rng_keys; const int64_t *episode_offset; const double *reset_states; const float *noise;
    double *returns; int32_t *env_steps, *agent_steps;
    float *row_state, *row_action, *row_next_state, *row_reward, *row_done;
};

template <int ENV, bool ST>
__global__ __launch_bounds__(DNT, 4) void actor_test_population_kernel(const AcArgs a)
{
    using EnvT = ContEnv<ENV>;
    constexpr int S = EnvT::S, A = EnvT::A, SD = EnvT::SD;
    static_assert(S <= AC_XLD && A <= AC_ALD && SD <= AC_MAXSD && TP_TB * SD <= DNT, "one thread per (episode, state word)");
    extern __shared__ __align__(16) float lds[];
    __shared__ __align__(16) float xin[TP_TB * AC_XLD];            // the observation each live episode acts on
    __shared__ __align__(16) float araw[TP_TB * AC_ALD];           // the actor's last Linear + bias
    __shared__ __align__(16) float actv[TP_TB * AC_ALD];           // the actions
    __shared__ double xd[TP_TB * SD];                              // the envs' own fp64 state
    __shared__ int tflag[TP_TB];                                   // episode still running (read by the threads that step its words)
    __shared__ unsigned alive_mask;
    const int tid = threadIdx.x;
    const int64_t agent = blockIdx.x;
    const int H = a.H, L = a.L, T = a.T;
    const bool ln = a.ln != 0, ppo = a.kind == LENV_ACTOR_PPO;
    const TpBlock blk = tp_block(T);
    const int ep0 = blk.ep0, rows = blk.rows;

    const TpLds lay = tp_lds_layout(blk.rows_max, a.W, ln, H);
    float *buf0 = lds, *buf1 = lds + lay.act, *lnbuf = buf1 + lay.act, *wst = lnbuf + lay.ln;
    const float *grow = a.params + agent * a.P, *gpar = grow + a.oAct;
    const float *par = ST ? wst : gpar;
    if (ST) tp_stage_mlp(wst, gpar, a.Pa, a.oW, L, S, H, A, tid);

    // ---- env.reset() of every episode of the block ----
    const uint64_t key = a.rng_keys[agent];
    const int64_t off = a.episode_offset ? a.episode_offset[agent] : 0;
    for (int e = tid; e < rows * SD; e += DNT) {
        const int te = e / SD, i = e - te * SD;
        xd[e] = a.reset_states ? a.reset_states[(agent * T + ep0 + te) * SD + i] : EnvT::reset_word(key, STREAM_TEST_RESET, off + ep0 + te, i);
    }
    const bool mine = tid < rows;
    const int64_t ep = agent * T + ep0 + tid;                      // this thread's episode in the [agents, T] outputs
    float ep_rew = 0.0f;
    int my_el = 0, n_agent = 0;
    bool my_alive = mine;
    if (tid < TP_TB) tflag[tid] = mine ? 1 : 0;
    tp_alive_init(&alive_mask, rows, tid);
    __syncthreads();

    for (int ai = 0; ai < a.cap; ++ai) {                           // base_agent.py:194 range(0, max_steps, same_action_num)
        const unsigned alive = alive_mask;
        for (int e = tid; e < rows * S; e += DNT) { const int te = e / S, i = e - te * S; xin[te * AC_XLD + i] = EnvT::obs(i, xd + te * SD); }
        __syncthreads();
        // ---- the actor on the live episodes: Actor_TD3 / Actor_PPO.net (models/actor_critic.py:11-19,38-49) ----
        const TpAct h = tp_trunk<ST, AC_LNBUF>(par, a.oW, a.ob, a.oLN, L, H, ln, xin, S, AC_XLD, buf0, buf1, lnbuf, rows, a.act, 0.0f, alive, tid);
        at_layer<ST>(par + a.oW[L], par + a.ob[L], H, A, h.x, h.ld, araw, AC_ALD, rows, false, 0, 0.0f, alive, tid);
        __syncthreads();
        // ---- select_test_action (TD3.py:126-129) / actor_old.forward (actor_critic.py:45-49) ----
        for (int e = tid; e < rows * A; e += DNT) {
            const int te = e / A, k = e - te * A;
            if (!((alive >> te) & 1u)) continue;
            float zn;
            if (a.noise) zn = a.noise[(((agent * T + ep0 + te) * a.cap) + ai) * A + k];
            else {
                const int64_t n = ((off + ep0 + te) * (int64_t)(ppo ? a.cap : a.max_steps) + ai) * A + k;
                zn = (float)det_normal(key, ppo ? STREAM_PPO_TEST_NOISE : STREAM_TD3_TEST_NOISE, (uint64_t)n);
            }
            const float th = det_tanhf(lenv_tanh_table, araw[te * AC_ALD + k]);
            float v;
            if (ppo) {
                float sd = grow[k];
                if (sd < 0.001f) sd = 0.001f;
                v = th + zn * sd;
            } else {
                const float ma = a.ma;
                v = th * ma + (zn * a.astd) * ma;
                v = v < -ma ? -ma : (v > ma ? ma : v);
            }
            actv[te * AC_ALD + k] = v;
        }
        __syncthreads();
        // ---- EnvWrapper.step on the real env (envs/env_wrapper.py:56-61): thread (episode, word) steps, thread e keeps episode e's books ----
        const bool started = my_alive;
        int64_t slot = 0;
        if (started && a.row_state) {
            slot = ep * a.cap + n_agent;
            for (int i = 0; i < S; ++i) a.row_state[slot * S + i] = xin[tid * AC_XLD + i];
            for (int k = 0; k < A; ++k) a.row_action[slot * A + k] = actv[tid * AC_ALD + k];
        }
        double rsum = 0.0;
        for (int r = 0; r < a.k_rep; ++r) {
            double nx = 0.0, pre = 0.0;
            const int wte = tid / SD;
            const bool wstep = tid < rows * SD && tflag[wte] != 0;
            if (wstep) nx = EnvT::step_word(tid - wte * SD, xd + wte * SD, actv + wte * AC_ALD);
            if (my_alive) pre = EnvT::reward_pre(xd + tid * SD, actv + tid * AC_ALD);       // the part of the reward that sees the OLD state
            __syncthreads();
            if (wstep) xd[tid] = nx;
            __syncthreads();
            if (my_alive) {
                rsum = rsum + EnvT::reward_post(xd + tid * SD, pre);
                ++my_el;
                if (EnvT::done(xd + tid * SD) || my_el >= a.max_steps) { my_alive = false; tflag[tid] = 0; }     // the env's own flag or TimeLimit
            }
            if (__syncthreads_or(my_alive ? 1 : 0) == 0) break;    // uniform: no episode of the block is inside this agent step any more
        }
        if (started) {
            const float r32 = (float)rsum;
            ep_rew = ep_rew + r32;
            if (a.row_state) {
                for (int i = 0; i < S; ++i) a.row_next_state[slot * S + i] = EnvT::obs(i, xd + tid * SD);
                a.row_reward[slot] = r32; a.row_done[slot] = my_alive ? 0.0f : 1.0f;
            }
            ++n_agent;
            if (!my_alive) tp_retire(&alive_mask, tid);
        }
        if (tp_all_retired(&alive_mask)) break;
    }
    if (mine) { a.returns[ep] = (double)ep_rew; a.env_steps[ep] = my_el; a.agent_steps[ep] = n_agent; }
}

}  // namespace lenv

using namespace lenv;

// the entry's own checks of cfg (only the fields the kernel reads) into the launch's shape
static int ac_shape(int kind, const void *cfg_, AcArgs &a, int &env_id)
{
    int S, A, H, L, T, act, san, max_steps;
    bool use_ln = false;                                           // TD3 alone
    a.ma = 1.0f; a.astd = 0.0f;
    if (kind == LENV_ACTOR_TD3) {
        const lenv_td3_cfg *c = static_cast<const lenv_td3_cfg *>(cfg_);
        env_id = c->env_id; S = c->state_dim; A = c->action_dim; H = c->hidden; L = c->layers; T = c->test_episodes; act = c->act;
        san = c->same_action_num; max_steps = c->max_steps;
        use_ln = c->use_layer_norm != 0; a.ma = (float)c->max_action; a.astd = (float)c->action_std;
    } else if (kind == LENV_ACTOR_PPO) {
        const lenv_ppo_cfg *c = static_cast<const lenv_ppo_cfg *>(cfg_);
        env_id = c->env_id; S = c->state_dim; A = c->action_dim; H = c->hidden; L = c->layers; T = c->test_episodes; act = c->act;
        san = c->same_action_num; max_steps = c->max_steps;
    } else return LENV_ERR_UNSUPPORTED;                            // TD3_discrete_vary (Gumbel-softmax actor), the gridworld agents: no kind
    if (max_steps < 1) return LENV_ERR_INVALID;
    if (!lenv_host::tp_cont_env_ok(env_id, S, A)) return LENV_ERR_UNSUPPORTED;
    if (act == LENV_ACT_PRELU || act < 0 || act > LENV_ACT_PRELU) return LENV_ERR_UNSUPPORTED;   // a trained slope in the reference; refused as the fused entries refuse it
    if (san < 0 || san > TP_MAX_REPEAT) return LENV_ERR_UNSUPPORTED;
    // the envelope of the fused entry of the same kind (td3_layout / ppo_layout), as far as the actor and the test go
    if (kind == LENV_ACTOR_TD3) { if (L < 1 || L > T3_MAXL || H < 1 || H > T3_MAXW || T < 1 || T * S > DNT) return LENV_ERR_UNSUPPORTED; }
    else if (L < 1 || L > PP_MAXL || H < 1 || H > PP_MAXW || T < 1 || T > PP_MAXT) return LENV_ERR_UNSUPPORTED;
    a.kind = kind; a.H = H; a.L = L; a.act = act; a.T = T; a.max_steps = max_steps;
    lenv_host::tp_repeat(a, max_steps, san);
    a.W = (H + 3) & ~3;
    for (int l = 0; l <= T3_MAXL; ++l) a.oW[l] = a.ob[l] = 0;
    if (kind == LENV_ACTOR_TD3) {
        MlpOff ma, mc;
        mlp_off(ma, S, H, L, A, use_ln);
        mlp_off(mc, S + A, H, L, 1, use_ln);
        for (int l = 0; l <= L; ++l) { a.oW[l] = ma.oW[l]; a.ob[l] = ma.ob[l]; }
        a.ln = ma.ln; a.oLN = ma.oLN; a.Pa = ma.P; a.oAct = 0; a.P = ma.P + 2 * mc.P;       // actor | critic_1 | critic_2
    } else {
        PpoMlp ma, mc;
        ppo_mlp(ma, S, H, L, A);
        ppo_mlp(mc, S, H, L, 1);
        for (int l = 0; l <= L; ++l) { a.oW[l] = ma.oW[l]; a.ob[l] = ma.ob[l]; }
        a.ln = 0; a.oLN = 0; a.Pa = ma.P; a.oAct = A; a.P = A + ma.P + mc.P;                // action_std | actor.net | critic.net
    }
    return LENV_OK;
}

extern "C" int64_t lenv_actor_test_rows_cap(int kind, const void *cfg)
{
    if (!cfg) return LENV_ERR_INVALID;
    AcArgs a{};
    int env_id = 0;
    const int rc = ac_shape(kind, cfg, a, env_id);
    return rc != LENV_OK ? rc : a.cap;
}

template <bool ST>
static int ac_launch(int env_id, dim3 grid, size_t lds_bytes, void *stream, const AcArgs &a)
{
    if (env_id == LENV_ENV_PENDULUM) return lenv_host::launch(actor_test_population_kernel<LENV_ENV_PENDULUM, ST>, grid, dim3(DNT), lds_bytes, stream, a);
    if (env_id == LENV_ENV_CMC) return lenv_host::launch(actor_test_population_kernel<LENV_ENV_CMC, ST>, grid, dim3(DNT), lds_bytes, stream, a);
    return lenv_host::launch(actor_test_population_kernel<LENV_ENV_CHEETAH_STANDIN, ST>, grid, dim3(DNT), lds_bytes, stream, a);
}

extern "C" int lenv_actor_test_population(int kind, const void *cfg, const float *params, const uint64_t *rng_keys, const int64_t *episode_offset,
                                          const double *reset_states, const float *noise, int64_t agents, double *returns, int32_t *env_steps,
                                          int32_t *agent_steps, float *row_state, float *row_action, float *row_next_state, float *row_reward,
                                          float *row_done, void *stream)
{
    int rc = lenv_host::tp_check_args({ cfg, params, rng_keys, returns, env_steps, agent_steps }, agents, row_state, row_action, row_next_state, row_reward, row_done);
    if (rc != LENV_OK) return rc;
    AcArgs a{};
    int env_id = 0;
    rc = ac_shape(kind, cfg, a, env_id);
    if (rc != LENV_OK || agents == 0) return rc;
    if ((rc = lenv_host::tp_agents_rc(agents, 0x7fffffff)) != LENV_OK) return rc;
    a.params = params; a.rng_keys = rng_keys; a.episode_offset = episode_offset; a.reset_states = reset_states; a.noise = noise;
    a.returns = returns; a.env_steps = env_steps; a.agent_steps = agent_steps;
    a.row_state = row_state; a.row_action = row_action; a.row_next_state = row_next_state; a.row_reward = row_reward; a.row_done = row_done;
    const lenv_host::TpPlan p = lenv_host::tp_launch_plan(agents, a.T, a.W, a.ln != 0, a.H, a.Pa, AC_LDS_LIMIT);   // the actor next to the activations
    return p.staged ? ac_launch<true>(env_id, p.grid, p.lds_bytes, stream, a) : ac_launch<false>(env_id, p.grid, p.lds_bytes, stream, a);
}
