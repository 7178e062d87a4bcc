// discrete_actor_test_population.hip -- BaseAgent.test (agents/base_agent.py:155-227) with TD3_discrete_vary.select_test_action
// (agents/TD3_discrete_vary.py:169-171) for a whole population of trained Gumbel-softmax actors in one launch: agent i runs
// cfg->test_episodes episodes on the real env (CartPole-v0, Acrobot-v1, MountainCar-v0) and, when asked, records every transition it visits
// -- the replay buffer the reference's test() returns, with the action VECTOR in it (discretize_action: the env gets its argmax).
//
// The operations are those of the fused loop's closing test (test_phase of td3_discrete_inner_loop.hip): reset, the actor's forward, the
// Gumbel-softmax head at the annealed temperature plus the test noise, the first-maximum argmax into the env, each step's reward rounded to
// fp32 onto an fp32 episode return, the episode over at the env's done or after max_steps steps.  Nothing is restated: the physics, the
// reset draw and the observation are real_env_step / real_env_reset_draw / real_env_obs of lenv_device.cuh; the parameter layout, the Gumbel
// draw, the temperature, the head and the argmax are dmlp_off / det_gumbel / td3d_temperature / gumbel_softmax_row / argmax_first of
// lenv_td3d_actor.cuh, which the fused kernel includes too; the shared LayerNorm is ln_rows_forward of lenv_ln.cuh, the layer product is
// at_layer of lenv_at_layer.cuh: the k-ascending fmaf chain from 0, then the bias, then the activation, i.e. the bits of the GEMM-queue forward.
//   a = gumbel_softmax_row(actor(s), g, A, max_action, temp, hard) + z * (float)action_std, n = ((episode_offset + e) * max_steps + step) * A + k,
//   g = det_gumbel(key, STREAM_TD3D_GUMBEL_TEST, n), z = det_normal(key, STREAM_TD3_TEST_NOISE, n),
//   temp = td3d_temperature(gumbel_temp, max(learn_calls - 1, 0)): the fused loop reads the temperature before it counts a learn call.
// With a gumbel / noise tape g / z = tape[agent][e][step][k] and that stream is not drawn.
//
// Grid (agent, block of at most TP_TB episodes), 512 threads.  The episodes of a block advance in lock-step; a finished one idles until the
// block ends.  The fp64 env state of episode e lives in the registers of thread e, which also applies the head and the noise to its row
// (A <= 3) and keeps the episode's books.
// The block's episodes and their alive mask, the dynamic-LDS layout, the staging and the hidden layers are the shared pieces of
// lenv_at_layer.cuh (tp_block, tp_stage_mlp, tp_trunk) and lenv_tp_layout.h (tp_lds_layout); the launch plan is tp_launch_plan of lenv_host.h.  Here W = H rounded
// up to 4, and the actor is staged where all of it stays below DA_LDS_LIMIT.
// __launch_bounds__(DNT, 4): four waves per SIMD, i.e. at most 128 VGPRs.  Without the bound the six instantiations compile to 135..142 VGPRs
// (three waves per SIMD: one workgroup of 8 waves per CU, and the staging rule below rests on two); with it to 128 VGPRs and a scratch frame
// of 12..44 B per lane.
#include <hip/hip_runtime.h>
#include "../../include/lenv_hip.h"
#include "lenv_gemm.cuh"
#include "lenv_td3d_actor.cuh"
#include "lenv_ln.cuh"
#include "lenv_at_layer.cuh"
#include "lenv_host.h"

namespace lenv {

constexpr int DA_XLD = 8;                      // row stride of the observation rows (Acrobot's 6, rounded up to 4)
constexpr int DA_ALD = 4;                      // row stride of the raw actor outputs (at most 3 actions)
constexpr int DA_LNBUF = TP_TB * (TD_MAXW | 1);     // ln_rows_forward: every row of a block in one chunk
constexpr int DA_MAXT = 64;                    // test_episodes the fused entry admits (td3d_layout)
// The rule of actor_test_population.hip (AC_LDS_LIMIT): the actor is staged where the workgroup's LDS stays within half a CU's 160 KiB, so that
// two workgroups still share a CU; the static arrays below take under 1 KiB.
constexpr size_t DA_LDS_LIMIT = 80 * 1024 - 8192;

struct DaArgs {
    int H, L, act, ln, hard, T, max_steps;
    float ma, astd;                            // (float)max_action, (float)action_std
    double temp0;                              // gumbel_temp
    int P, Pa, W;                              // row stride of params, the actor's parameter count; activation row stride
    int oW[TD_MAXL + 1], ob[TD_MAXL + 1], oLN; // offsets inside the actor (dmlp_off)
    const float *params; const uint64_t *rng_keys; const int64_t *episode_offset, *learn_calls; const double *reset_states;
    const float *gumbel, *noise;
    double *returns; int32_t *env_steps, *agent_steps;
    float *row_state, *row_action, *row_next_state, *row_reward, *row_done;
};

template <int ENVD, bool ST>
__global__ __launch_bounds__(DNT, 4) void discrete_actor_test_population_kernel(const DaArgs a)
{
    constexpr int S = ENVD == LENV_ENV_CARTPOLE ? 4 : (ENVD == LENV_ENV_ACROBOT ? 6 : 2);
    constexpr int A = ENVD == LENV_ENV_CARTPOLE ? 2 : 3;
    static_assert(S <= DA_XLD && A <= DA_ALD && A <= TD_MAXA && TP_TB <= 32, "row strides and the alive mask");
    extern __shared__ __align__(16) float lds[];
    __shared__ __align__(16) float xin[TP_TB * DA_XLD];            // the observation each live episode acts on
    __shared__ __align__(16) float araw[TP_TB * DA_ALD];           // the actor's last Linear + bias
    __shared__ unsigned alive_mask;
    const int tid = threadIdx.x;
    const int64_t agent = blockIdx.x;
    const int H = a.H, L = a.L, T = a.T;
    const bool ln = a.ln != 0;
    const TpBlock blk = tp_block(T);
    const int ep0 = blk.ep0, rows = blk.rows;

    const TpLds lay = tp_lds_layout(blk.rows_max, a.W, ln, H);
    float *buf0 = lds, *buf1 = lds + lay.act, *lnbuf = buf1 + lay.act, *wst = lnbuf + lay.ln;
    const float *gpar = a.params + agent * a.P;                    // actor | critic_1 | critic_2: the actor comes first
    const float *par = ST ? wst : gpar;
    if (ST) tp_stage_mlp(wst, gpar, a.Pa, a.oW, L, S, H, A, tid);

    // ---- env.reset() of every episode of the block ----
    const uint64_t key = a.rng_keys[agent];
    const int64_t off = a.episode_offset ? a.episode_offset[agent] : 0;
    const int64_t lc = a.learn_calls ? a.learn_calls[agent] : 0;
    const float temp = td3d_temperature(a.temp0, lc > 1 ? lc - 1 : 0);     // what `temp` of the fused loop holds after lc learn calls
    const bool hard = a.hard != 0;
    const bool mine = tid < rows;
    const int64_t ep = agent * T + ep0 + tid;                      // this thread's episode in the [agents, T] outputs
    double st[4] = { 0.0, 0.0, 0.0, 0.0 };
    float ep_rew = 0.0f;
    int tlen = 0;
    bool live = mine;
    if (mine) {
        if (a.reset_states) { for (int i = 0; i < 4; ++i) st[i] = a.reset_states[ep * 4 + i]; }
        else real_env_reset_draw(ENVD, key, STREAM_TEST_RESET, off + ep0 + tid, st);
        float obs[8];
        real_env_obs(ENVD, st, obs);
#pragma unroll
        for (int i = 0; i < S; ++i) xin[tid * DA_XLD + i] = obs[i];
    }
    tp_alive_init(&alive_mask, rows, tid);
    __syncthreads();

    for (int t = 0; t < a.max_steps; ++t) {
        const unsigned alive = alive_mask;
        // ---- Actor_TD3_discrete.net on the live episodes (models/actor_critic.py:22-35) ----
        const TpAct h = tp_trunk<ST, DA_LNBUF>(par, a.oW, a.ob, a.oLN, L, H, ln, xin, S, DA_XLD, buf0, buf1, lnbuf, rows, a.act, 0.0f, alive, tid);
        at_layer<ST>(par + a.oW[L], par + a.ob[L], H, A, h.x, h.ld, araw, DA_ALD, rows, false, 0, 0.0f, alive, tid);
        __syncthreads();
        // ---- select_test_action (:169-171), then EnvWrapper.step on the real env with action.argmax() ----
        if (live) {
            const int64_t slot = ep * a.max_steps + t;             // cap = max_steps: one agent step is one env step
            float raw[A], gm[A], pa[A], av[A];
#pragma unroll
            for (int k = 0; k < A; ++k) {
                raw[k] = araw[tid * DA_ALD + k];
                const uint64_t n = (uint64_t)(((off + ep0 + tid) * (int64_t)a.max_steps + t) * A + k);
                gm[k] = a.gumbel ? a.gumbel[slot * A + k] : det_gumbel(key, STREAM_TD3D_GUMBEL_TEST, n);
            }
            gumbel_softmax_row(raw, gm, A, a.ma, temp, hard, pa, nullptr);
#pragma unroll
            for (int k = 0; k < A; ++k) {
                const uint64_t n = (uint64_t)(((off + ep0 + tid) * (int64_t)a.max_steps + t) * A + k);
                const float zn = a.noise ? a.noise[slot * A + k] : (float)det_normal(key, STREAM_TD3_TEST_NOISE, n);
                av[k] = pa[k] + zn * a.astd;
            }
            double rew;
            int dn = 0;
            real_env_step(ENVD, st, argmax_first(av, A), rew, dn);
            const float r32 = (float)rew;
            ++tlen;
            if (tlen >= a.max_steps) dn = 1;                       // gym.wrappers.TimeLimit
            float obs[8];
            real_env_obs(ENVD, st, obs);
            if (a.row_state) {
#pragma unroll
                for (int i = 0; i < S; ++i) { a.row_state[slot * S + i] = xin[tid * DA_XLD + i]; a.row_next_state[slot * S + i] = obs[i]; }
#pragma unroll
                for (int k = 0; k < A; ++k) a.row_action[slot * A + k] = av[k];
                a.row_reward[slot] = r32; a.row_done[slot] = dn ? 1.0f : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < S; ++i) xin[tid * DA_XLD + i] = obs[i];
            ep_rew = ep_rew + r32;
            if (dn) { live = false; tp_retire(&alive_mask, tid); }
        }
        if (tp_all_retired(&alive_mask)) break;
    }
    if (mine) { a.returns[ep] = (double)ep_rew; a.env_steps[ep] = tlen; a.agent_steps[ep] = tlen; }
}

}  // namespace lenv

using namespace lenv;

// the entry's own checks of cfg (only the fields the kernel reads) into the launch's shape
static int da_shape(const lenv_td3d_cfg *cfg, DaArgs &a)
{
    if (cfg->max_steps < 1) return LENV_ERR_INVALID;
    const int S = cfg->state_dim, A = cfg->action_dim, H = cfg->hidden, L = cfg->layers, T = cfg->test_episodes;
    // the envelope of td3d_layout, as far as the actor and the test go
    if (!lenv_host::tp_discrete_env_ok(cfg->env_id, S, A)) return LENV_ERR_UNSUPPORTED;
    if (cfg->act == LENV_ACT_PRELU || cfg->act < 0 || cfg->act > LENV_ACT_PRELU) return LENV_ERR_UNSUPPORTED;   // a trained slope in the reference
    if (L < 1 || L > TD_MAXL || H < 1 || H > TD_MAXW || T < 1 || T > DA_MAXT || !(cfg->gumbel_temp > 0.0)) return LENV_ERR_UNSUPPORTED;
    DMlpOff ma, mc;
    dmlp_off(ma, S, H, L, A, cfg->use_layer_norm);
    dmlp_off(mc, S + A, H, L, 1, cfg->use_layer_norm);
    a.H = H; a.L = L; a.act = cfg->act; a.ln = ma.ln; a.hard = cfg->gumbel_hard != 0 ? 1 : 0; a.T = T; a.max_steps = cfg->max_steps;
    a.ma = (float)cfg->max_action; a.astd = (float)cfg->action_std; a.temp0 = cfg->gumbel_temp;
    a.P = ma.P + 2 * mc.P; a.Pa = ma.P; a.W = (H + 3) & ~3;
    for (int l = 0; l <= TD_MAXL; ++l) { a.oW[l] = ma.oW[l]; a.ob[l] = ma.ob[l]; }
    a.oLN = ma.oLN;
    return LENV_OK;
}

extern "C" int64_t lenv_td3d_test_rows_cap(const lenv_td3d_cfg *cfg)
{
    if (!cfg) return LENV_ERR_INVALID;
    DaArgs a{};
    const int rc = da_shape(cfg, a);
    return rc != LENV_OK ? rc : a.max_steps;
}

template <bool ST>
static int da_launch(int env_id, dim3 grid, size_t lds_bytes, void *stream, const DaArgs &a)
{
    if (env_id == LENV_ENV_CARTPOLE) return lenv_host::launch(discrete_actor_test_population_kernel<LENV_ENV_CARTPOLE, ST>, grid, dim3(DNT), lds_bytes, stream, a);
    if (env_id == LENV_ENV_ACROBOT) return lenv_host::launch(discrete_actor_test_population_kernel<LENV_ENV_ACROBOT, ST>, grid, dim3(DNT), lds_bytes, stream, a);
    return lenv_host::launch(discrete_actor_test_population_kernel<LENV_ENV_MOUNTAINCAR, ST>, grid, dim3(DNT), lds_bytes, stream, a);
}

extern "C" int lenv_td3d_test_population(const lenv_td3d_cfg *cfg, const float *params, const uint64_t *rng_keys, const int64_t *episode_offset,
                                         const int64_t *learn_calls, const double *reset_states, const float *gumbel, const float *noise,
                                         int64_t agents, double *returns, int32_t *env_steps, int32_t *agent_steps, float *row_state,
                                         float *row_action, float *row_next_state, float *row_reward, float *row_done, void *stream)
{
    int rc = lenv_host::tp_check_args({ cfg, params, rng_keys, returns, env_steps, agent_steps }, agents, row_state, row_action, row_next_state, row_reward, row_done);
    if (rc != LENV_OK) return rc;
    DaArgs a{};
    rc = da_shape(cfg, a);
    if (rc != LENV_OK || agents == 0) return rc;
    if ((rc = lenv_host::tp_agents_rc(agents, 0x7fffffff)) != LENV_OK) return rc;
    a.params = params; a.rng_keys = rng_keys; a.episode_offset = episode_offset; a.learn_calls = learn_calls; a.reset_states = reset_states;
    a.gumbel = gumbel; a.noise = noise;
    a.returns = returns; a.env_steps = env_steps; a.agent_steps = agent_steps;
    a.row_state = row_state; a.row_action = row_action; a.row_next_state = row_next_state; a.row_reward = row_reward; a.row_done = row_done;
    const lenv_host::TpPlan p = lenv_host::tp_launch_plan(agents, a.T, a.W, a.ln != 0, a.H, a.Pa, DA_LDS_LIMIT);   // the actor next to the activations
    return p.staged ? da_launch<true>(cfg->env_id, p.grid, p.lds_bytes, stream, a) : da_launch<false>(cfg->env_id, p.grid, p.lds_bytes, stream, a);
}
