// agent_test_population.hip -- BaseAgent.test (agents/base_agent.py:155-227) with DDQN.select_test_action / DuelingDDQN.select_test_action for
// a whole population of trained agents in one launch: agent i runs cfg->test_episodes greedy episodes on the real env (CartPole-v0,
// Acrobot-v1, MountainCar-v0) and, when asked, records every transition it visits -- the replay buffer the reference's test() returns.
//
// The operations are those of the fused loops' closing test (test_phase of dueling_se_inner_loop.hip): reset, the greedy action with ties
// towards the lower index repeated same_action_num times or until done, TimeLimit at max_steps env steps, the repeats' rewards summed in fp64
// and rounded once to fp32 onto an fp32 episode return.  Nothing is restated: the physics, the reset draw and the observation are
// real_env_step / real_env_reset_draw / real_env_obs of lenv_device.cuh, the parameter layout is duel_param_offsets (the final_online rows of
// lenv_dueling_se_inner_loop), the shared LayerNorm is ln_rows_forward of lenv_ln.cuh.  Every dot product is the k-ascending fmaf chain from 0,
// then the bias, then the activation, so the Q values carry the bits of the GEMM-queue forward and of the register-resident DDQN kernel.
//
// Grid (agent, block of at most TP_TB episodes), 512 threads.  The episodes of a block advance in lock-step; a finished one idles until the
// block ends.  A forward item is (output unit j, group of AT_EPT episodes): consecutive lanes own consecutive units, so the activation reads
// of a wave are LDS broadcasts whatever the row stride, and a weight is loaded once for the group's episodes.  The env state of episode e
// lives in the registers of thread e.
// The block's episodes and their alive mask, the dynamic-LDS layout, the staging and the hidden layers are the shared pieces of
// lenv_at_layer.cuh (tp_block, tp_stage_mlp; the hidden-layer loop of tp_trunk is written out below) and lenv_tp_layout.h (tp_lds_layout); the launch plan is tp_launch_plan of lenv_host.h.  Here W = the
// widest layer (H, or 2 F for the two head hidden layers of a dueling agent, rounded up to 4), and the agent's parameters are staged where
// they still fit into 160 KiB (AT_LDS_LIMIT), every weight matrix transposed (k-major: conflict-free for lanes on consecutive units);
// otherwise the weights are read from global memory, a lane streaming its unit's row.  The widest admitted shape (H 512, three hidden layers,
// LayerNorm) takes 2 * 16 * 512 + 16 * 513 floats = 96.1 KiB.
#include <hip/hip_runtime.h>
#include "../../include/lenv_hip.h"
#include "lenv_gemm.cuh"
#include "lenv_dueling_params.cuh"
#include "lenv_ln.cuh"
#include "lenv_at_layer.cuh"
#include "lenv_host.h"

namespace lenv {

constexpr int AT_XLD = 8;                      // row stride of the observation rows
constexpr int AT_MAXS = 6, AT_MAXA = 3;        // the widest observation (Acrobot) and the most actions of the three envs
constexpr int AT_LNBUF = TP_TB * (D_MAXH | 1); // ln_rows_forward: every row of a block in one chunk
constexpr size_t AT_LDS_LIMIT = 160 * 1024 - 1024;   // dynamic bytes next to the static arrays below (under 1 KiB)

struct AtArgs {
    int env_id, S, A, H, L, F, act, plain, ln, T, max_steps, k_rep, cap;
    float prelu;
    int P, W;
    const float *params; const uint64_t *rng_keys; const int64_t *episode_offset; const double *reset_states;
    double *returns; int32_t *env_steps, *agent_steps;
    float *row_state; int32_t *row_action; float *row_next_state, *row_reward, *row_done;
};

template <bool ST>
__global__ __launch_bounds__(DNT) void agent_test_population_kernel(const AtArgs a)
{
    extern __shared__ __align__(16) float lds[];
    __shared__ __align__(16) float xin[TP_TB * AT_XLD];            // the observation each live episode acts on
    __shared__ float qadv[TP_TB * 4], vhead[TP_TB];                // Q(s, .) of a plain agent / the advantage head; the value head
    __shared__ unsigned alive_mask;
    const int tid = threadIdx.x;
    const int64_t agent = blockIdx.x;
    const int S = a.S, A = a.A, H = a.H, L = a.L, F = a.F, T = a.T;
    const bool plain = a.plain != 0, ln = a.ln != 0;
    const TpBlock blk = tp_block(T);
    const int ep0 = blk.ep0, rows = blk.rows;
    const DuelOffsets po = duel_param_offsets(S, A, H, F, L, plain, ln);

    const TpLds lay = tp_lds_layout(blk.rows_max, a.W, ln, H);
    float *buf0 = lds, *buf1 = lds + lay.act, *lnbuf = buf1 + lay.act, *wst = lnbuf + lay.ln;
    auto buf = [&](int i) { return (i & 1) ? buf1 : buf0; };
    const float *gpar = a.params + agent * a.P;
    const float *par = ST ? wst : gpar;
    if (ST) {
        tp_stage_mlp(wst, gpar, a.P, po.oWf, L, S, H, F, tid);
        if (!plain) {
            at_stage_transposed(wst + po.oWv1, gpar + po.oWv1, F, F, tid);
            at_stage_transposed(wst + po.oWa1, gpar + po.oWa1, F, F, tid);
            at_stage_transposed(wst + po.oWa2, gpar + po.oWa2, A, F, tid);
        }
    }

    // ---- env.reset() of every episode of the block ----
    const bool mine = tid < rows;
    const int64_t ep = agent * T + ep0 + tid;                      // this thread's episode in the [agents, T] outputs
    double st[4] = { 0.0, 0.0, 0.0, 0.0 };
    float ep_rew = 0.0f;
    int tlen = 0, n_agent = 0;
    bool live = mine;
    if (mine) {
        if (a.reset_states) { for (int i = 0; i < 4; ++i) st[i] = a.reset_states[ep * 4 + i]; }
        else real_env_reset_draw(a.env_id, a.rng_keys[agent], STREAM_TEST_RESET, (a.episode_offset ? a.episode_offset[agent] : 0) + ep0 + tid, st);
        float obs[8];
        real_env_obs(a.env_id, st, obs);
#pragma unroll
        for (int i = 0; i < AT_MAXS; ++i) if (i < S) xin[tid * AT_XLD + i] = obs[i];
    }
    tp_alive_init(&alive_mask, rows, tid);
    __syncthreads();

    const int ldh = ln ? H : (H + 3) & ~3;                         // ln_rows_forward takes dense rows
    for (int t = 0; t < a.max_steps; t += a.k_rep) {               // base_agent.py:194 range(0, max_steps, same_action_num)
        const unsigned alive = alive_mask;
        // ---- Q(s, .) of the live episodes: Critic_DQN / Critic_DuelingDQN (models/actor_critic.py:84-122) ----
        // (tp_trunk written out: it takes the offsets through pointers, and po's are computed in registers here, not kernel arguments as in the
        // two actor kernels -- handing them over cost the 2-256-256-3 MountainCar agent 1.8 %, docs/notebook_test_population_refactor.md)
        const float *in = xin;
        int n_in = S, ldi = AT_XLD;
        for (int l = 0; l < L; ++l) {
            float *out = buf(l);
            const bool at_ln = ln && l >= 1;
            at_layer<ST>(par + po.oWf[l], par + po.obf[l], n_in, H, in, ldi, out, ldh, rows, !at_ln, a.act, a.prelu, alive, tid);
            __syncthreads();
            if (at_ln) ln_rows_forward<AT_LNBUF>(lnbuf, out, rows, H, par + po.oLN, par + po.oLN + H, nullptr, nullptr, a.act, a.prelu);
            in = out; n_in = H; ldi = ldh;
        }
        if (plain) {
            at_layer<ST>(par + po.oWf[L], par + po.obf[L], H, A, in, ldi, qadv, 4, rows, false, 0, 0.0f, alive, tid);
        } else {
            float *feat = buf(L), *heads = buf(L + 1);   // heads: [rows][v1 | a1]
            const int ldf = (F + 3) & ~3, ld2 = 2 * ldf;
            at_layer<ST>(par + po.oWf[L], par + po.obf[L], H, F, in, ldi, feat, ldf, rows, false, 0, 0.0f, alive, tid);
            __syncthreads();
            at_layer<ST>(par + po.oWv1, par + po.obv1, F, F, feat, ldf, heads, ld2, rows, true, a.act, a.prelu, alive, tid);
            at_layer<ST>(par + po.oWa1, par + po.oba1, F, F, feat, ldf, heads + ldf, ld2, rows, true, a.act, a.prelu, alive, tid);
            __syncthreads();
            at_layer<ST>(par + po.oWv2, par + po.obv2, F, 1, heads, ld2, vhead, 1, rows, false, 0, 0.0f, alive, tid);
            at_layer<ST>(par + po.oWa2, par + po.oba2, F, A, heads + ldf, ld2, qadv, 4, rows, false, 0, 0.0f, alive, tid);
        }
        __syncthreads();
        // ---- select_test_action, then EnvWrapper.step on the real env (envs/env_wrapper.py:56-61) ----
        if (live) {
            float q[AT_MAXA] = { 0.0f, 0.0f, 0.0f };
            if (plain) {
#pragma unroll
                for (int aa = 0; aa < AT_MAXA; ++aa) if (aa < A) q[aa] = qadv[tid * 4 + aa];
            }
            else {                                                 // q = V + (Adv - Adv.mean()) of the row (finish_q, global_mean false)
                float sum = 0.0f;
#pragma unroll
                for (int aa = 0; aa < AT_MAXA; ++aa) if (aa < A) sum = sum + qadv[tid * 4 + aa];
                const float mean = sum / (float)A;
#pragma unroll
                for (int aa = 0; aa < AT_MAXA; ++aa) if (aa < A) q[aa] = vhead[tid] + (qadv[tid * 4 + aa] - mean);
            }
            int am = 0; float best = q[0];
#pragma unroll
            for (int aa = 1; aa < AT_MAXA; ++aa) if (aa < A && q[aa] > best) { best = q[aa]; am = aa; }
            double rsum = 0.0;
            int nstep = 0, dn = 0;
            for (int r = 0; r < a.k_rep; ++r) {
                double rew;
                real_env_step(a.env_id, st, am, rew, dn);
                rsum = rsum + rew;
                ++nstep;
                if (tlen + nstep >= a.max_steps) dn = 1;           // gym.wrappers.TimeLimit
                if (dn) break;
            }
            const float r32 = (float)rsum;
            float obs[8];
            real_env_obs(a.env_id, st, obs);
            if (a.row_state) {
                const int64_t slot = ep * a.cap + n_agent;
#pragma unroll
                for (int i = 0; i < AT_MAXS; ++i) if (i < S) { a.row_state[slot * S + i] = xin[tid * AT_XLD + i]; a.row_next_state[slot * S + i] = obs[i]; }
                a.row_action[slot] = am; a.row_reward[slot] = r32; a.row_done[slot] = dn ? 1.0f : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < AT_MAXS; ++i) if (i < S) xin[tid * AT_XLD + i] = obs[i];
            ep_rew = ep_rew + r32;
            tlen += nstep; ++n_agent;
            if (dn) { live = false; tp_retire(&alive_mask, tid); }
        }
        if (tp_all_retired(&alive_mask)) break;
    }
    if (mine) { a.returns[ep] = (double)ep_rew; a.env_steps[ep] = tlen; a.agent_steps[ep] = n_agent; }
}

}  // namespace lenv

using namespace lenv;

// the entry's own checks of cfg (only the fields the kernel reads) into the launch's shape
static int at_shape(const lenv_ddqn_cfg *cfg, AtArgs &a)
{
    if (cfg->agent_kind != 0 && cfg->agent_kind != 1) return LENV_ERR_INVALID;
    if (cfg->max_steps < 1) return LENV_ERR_INVALID;
    const bool plain = cfg->agent_kind == 0;
    const int S = cfg->state_dim, A = cfg->num_actions, H = cfg->q_hidden, L = cfg->q_layers, F = plain ? A : cfg->feature_dim, T = cfg->test_episodes;
    if (cfg->q_act == LENV_ACT_PRELU) return LENV_ERR_UNSUPPORTED;     // a trained slope in the reference; refused as the generic kernel refuses it
    if (L < 1 || L > D_MAXL || H < 1 || H > D_MAXH || F < 1 || F > D_MAXW || T < 1 || T > D_MAXW) return LENV_ERR_UNSUPPORTED;
    if (cfg->same_action_num < 0 || cfg->same_action_num > TP_MAX_REPEAT) return LENV_ERR_UNSUPPORTED;
    if (!lenv_host::tp_discrete_env_ok(cfg->env_id, S, A)) return LENV_ERR_UNSUPPORTED;
    a.env_id = cfg->env_id; a.S = S; a.A = A; a.H = H; a.L = L; a.F = F; a.act = cfg->q_act; a.prelu = cfg->q_prelu; a.plain = plain ? 1 : 0;
    a.ln = (cfg->q_layer_norm != 0 && L >= 2) ? 1 : 0;
    a.T = T; a.max_steps = cfg->max_steps;
    lenv_host::tp_repeat(a, cfg->max_steps, cfg->same_action_num);
    a.P = duel_param_offsets(S, A, H, F, L, plain, a.ln != 0).P;
    const int hw = (H + 3) & ~3, fw = 2 * ((F + 3) & ~3);
    a.W = plain || hw > fw ? hw : fw;
    return LENV_OK;
}

extern "C" int64_t lenv_agent_test_rows_cap(const lenv_ddqn_cfg *cfg)
{
    if (!cfg) return LENV_ERR_INVALID;
    AtArgs a{};
    const int rc = at_shape(cfg, a);
    return rc != LENV_OK ? rc : a.cap;
}

extern "C" int lenv_agent_test_population(const lenv_ddqn_cfg *cfg, const float *params, const uint64_t *rng_keys, const int64_t *episode_offset,
                                          const double *reset_states, int64_t agents, double *returns, int32_t *env_steps, int32_t *agent_steps,
                                          float *row_state, int32_t *row_action, float *row_next_state, float *row_reward, float *row_done,
                                          void *stream)
{
    int rc = lenv_host::tp_check_args({ cfg, params, rng_keys, returns, env_steps, agent_steps }, agents, row_state, row_action, row_next_state, row_reward, row_done);
    if (rc != LENV_OK) return rc;
    AtArgs a{};
    rc = at_shape(cfg, a);
    if (rc != LENV_OK || agents == 0) return rc;
    if ((rc = lenv_host::tp_agents_rc(agents, 0x7fffffff)) != LENV_OK) return rc;
    a.params = params; a.rng_keys = rng_keys; a.episode_offset = episode_offset; a.reset_states = reset_states;
    a.returns = returns; a.env_steps = env_steps; a.agent_steps = agent_steps;
    a.row_state = row_state; a.row_action = row_action; a.row_next_state = row_next_state; a.row_reward = row_reward; a.row_done = row_done;
    const lenv_host::TpPlan p = lenv_host::tp_launch_plan(agents, a.T, a.W, a.ln != 0, a.H, a.P, AT_LDS_LIMIT);    // the parameters next to the activations
    if (p.staged) return lenv_host::launch(agent_test_population_kernel<true>, p.grid, dim3(DNT), p.lds_bytes, stream, a);
    return lenv_host::launch(agent_test_population_kernel<false>, p.grid, dim3(DNT), p.lds_bytes, stream, a);
}
