// ql_se_inner_loop.hip -- fused NES inner loop for the tabular agents (QL, SARSA and their count-based variants) on a gridworld
// VirtualEnv (synthetic_env_type 0), one workgroup per chain.
//
// Replaces, for `chains` (theta +/- eps) perturbations of the synthetic environment at once, the reference's
//   GTN_Worker.calc_score                       agents/GTN_worker.py:187-221
//     QL / SARSA select_train_action / learn    agents/QL.py:38-106, agents/SARSA.py:36-91
//     BaseAgent.train / test                    agents/base_agent.py:64-227
//     EnvWrapper.step, virtual branch           envs/env_wrapper.py:17-49  (k steps REGARDLESS of done, fp32 tensor reward sum)
//     VirtualEnv.reset / step                   envs/virtual_env.py:35-54  (three nets on cat(action_onehot, self.state))
// and, for the per-episode tests and the final test, the real grid's transition tables (envs/gridworld.py:38-110 + TimeLimit).
//
// Unlike the RewardEnv loop (ql_rn_inner_loop.hip), nothing can be tabulated up front: the environment state is a continuous N-vector
// that the state net feeds back into itself, so every training step is a three-net MLP evaluation followed by an argmax, two
// thresholds and a tabular update, strictly in sequence.  The chain's perturbed theta is staged once, TRANSPOSED (input-major), so
// that lane = hidden unit / lane = output reads consecutive LDS words while the input row is a broadcast read; a step is
//   A  lane = hidden unit of one of the three nets: z = fmaf chain over the input row, k ascending, bias last, activation
//   A' the second hidden layer, the same way (hidden_layer 2)
//   B  lane = output (N next-state values | reward | done)
//   C  wave 0: first-maximum argmax of the N outputs; thread 0: the agent (fp64 Q-table in LDS), the next action
// with one workgroup barrier behind each.  Every dot product is the canonical order of oracle/lenv_oracle.h (orc_mlp_forward) and of
// se_step_kernel, so the SE outputs equal lenv_se_step_population's bit for bit.  docs/notebook_ql_se.md has the layout's reasoning.
#include "lenv_device.cuh"
#include "lenv_chain_frame.cuh"
#include "lenv_host.h"

namespace lenv {

constexpr int QSE_NT_MAX = 384;            // 3 nets x 128 hidden units: one unit per thread at the widest supported net
constexpr int QSE_LDS_MAX = 160 * 1024;
enum { QSE_RUN = 0, QSE_RESET = 1, QSE_END = 2 };

// Staged (transposed) parameter layout of a chain, U = 3H units (state | reward | done net), O = N + 2 outputs, K = A + N inputs:
//   Wt0 [K][U] | b0 [U] | { Wt1 [H][U] | b1 [U] } | Wto [H][O] | bo [O]        -- as many floats as theta has
struct QlSeLayout {
    int U, O, K;
    int64_t off_b0, off_w1, off_b1, off_wo, off_bo, P;
    int64_t net_P[2];                      // parameters of the state net, of the reward net (= the done net's)
};

__host__ __device__ inline QlSeLayout ql_se_layout(const lenv_ql_cfg &c)
{
    QlSeLayout y;
    const int64_t H = c.rn_hidden, N = c.n_states, A = c.n_actions;
    y.U = (int)(3 * H); y.O = (int)(N + 2); y.K = (int)(A + N);
    y.off_b0 = (int64_t)y.K * y.U;
    int64_t nxt = y.off_b0 + y.U;
    y.off_w1 = y.off_b1 = nxt;
    if (c.rn_layers == 2) { y.off_w1 = nxt; y.off_b1 = y.off_w1 + H * y.U; nxt = y.off_b1 + y.U; }
    y.off_wo = nxt;
    y.off_bo = y.off_wo + H * y.O;
    y.P = y.off_bo + y.O;
    const int64_t body = H * y.K + H + (c.rn_layers == 2 ? H * H + H : 0);
    y.net_P[0] = body + N * H + N;
    y.net_P[1] = body + H + 1;
    return y;
}

// where canonical theta[i] (state_net | reward_net | done_net, each W0[H,K] b0[H] {W1[H,H] b1[H]} Wout[out,H] bout[out]) lives in the staged layout
__device__ __forceinline__ int64_t ql_se_staged_index(const QlSeLayout &y, int64_t i, int N, int H, int L)
{
    int net; int64_t r;
    if (i < y.net_P[0]) { net = 0; r = i; }
    else if (i < y.net_P[0] + y.net_P[1]) { net = 1; r = i - y.net_P[0]; }
    else { net = 2; r = i - y.net_P[0] - y.net_P[1]; }
    const int64_t u0 = (int64_t)net * H;
    if (r < (int64_t)H * y.K) { const int64_t j = r / y.K, k = r - j * y.K; return k * y.U + u0 + j; }
    r -= (int64_t)H * y.K;
    if (r < H) return y.off_b0 + u0 + r;
    r -= H;
    if (L == 2) {
        if (r < (int64_t)H * H) { const int64_t j = r / H, k = r - j * H; return y.off_w1 + k * y.U + u0 + j; }
        r -= (int64_t)H * H;
        if (r < H) return y.off_b1 + u0 + r;
        r -= H;
    }
    const int64_t n_out = net == 0 ? N : 1, col0 = net == 0 ? 0 : N + net - 1;
    if (r < n_out * H) { const int64_t o = r / H, j = r - o * H; return y.off_wo + j * y.O + col0 + o; }
    r -= n_out * H;
    return y.off_bo + col0 + r;
}

// LDS of one chain (byte offsets): the agent's tables first, the SE's rows, then -- while it fits -- the staged theta
struct QlSeLds { size_t q, meter, rets, visits, x, h, rd, ctl, W, fixed_bytes; };

__host__ __device__ inline QlSeLds ql_se_lds(const lenv_ql_cfg &c)
{
    QlSeLds l;
    const size_t NA = (size_t)c.n_states * c.n_actions, Np = ((size_t)c.n_states + 3) & ~(size_t)3, U = 3 * (size_t)c.rn_hidden;
    size_t o = 0;
    l.q = o; o += sizeof(double) * NA;                                   // fp64 Q-table
    l.meter = o; o += sizeof(double) * (size_t)(c.train_episodes > 0 ? c.train_episodes : 0);
    l.rets = o; o += sizeof(double) * (size_t)c.test_episodes;
    l.visits = o; o += sizeof(int) * NA;                                 // n(s,a) of the count-based agents
    o = (o + 15) & ~(size_t)15;
    l.x = o; o += sizeof(float) * 2 * Np;                                // the SE's state vector, ping / pong
    l.h = o; o += sizeof(float) * 2 * U;                                 // hidden rows of the three nets, layer 1 / layer 2
    l.rd = o; o += sizeof(float) * 4;                                    // reward, done of the last SE step
    l.ctl = o; o += sizeof(int) * 4;                                     // thread 0 -> workgroup: mode, action
    l.W = o;
    l.fixed_bytes = o;
    return l;
}

struct QlSeArgs {
    lenv_ql_cfg cfg;
    const float *theta, *eps; const int32_t *worker; const float *sign;
    const int32_t *next_state; const double *reward; const uint8_t *done;      // the real grid: tests only
    const uint64_t *rng_keys;
    lenv_tapes tapes;
    lenv_ql_out out;
    float *trace_se;
    float *ws;                 // [chains][Ppad] staged thetas that do not fit LDS
    int64_t Ppad;
};

__device__ __forceinline__ int qse_argmax_f32(const double *row, int n)
{
    int best = 0;
    float bv = (float)row[0];
    for (int i = 1; i < n; ++i) { const float v = (float)row[i]; if (v > bv) { bv = v; best = i; } }
    return best;
}

// the order torch.argmax uses: a NaN is the maximum (two NaNs tie), so a state vector that overflowed resolves to the first NaN on both sides
__device__ __forceinline__ bool qse_beats(float a, float b) { return (a != a && b == b) || a > b; }

// WLDS: the staged theta lives in LDS (otherwise in the chain's slice of the workspace)
template <bool WLDS>
__global__ __launch_bounds__(QSE_NT_MAX) void ql_se_inner_kernel(const QlSeArgs a)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const lenv_ql_cfg &cfg = a.cfg;
    const int tid = threadIdx.x, NT = blockDim.x;
    const int64_t chain = blockIdx.x;
    const int N = cfg.n_states, A = cfg.n_actions, H = cfg.rn_hidden, L = cfg.rn_layers;
    const QlSeLayout y = ql_se_layout(cfg);
    const QlSeLds lo = ql_se_lds(cfg);
    const int U = y.U, O = y.O;
    double *q = reinterpret_cast<double *>(lds_raw + lo.q);
    double *meter = reinterpret_cast<double *>(lds_raw + lo.meter);
    double *rets = reinterpret_cast<double *>(lds_raw + lo.rets);
    int *visits = reinterpret_cast<int *>(lds_raw + lo.visits);
    float *xbuf = reinterpret_cast<float *>(lds_raw + lo.x);
    float *h0 = reinterpret_cast<float *>(lds_raw + lo.h), *h1 = h0 + U;
    volatile float *rd = reinterpret_cast<float *>(lds_raw + lo.rd);
    volatile int *ctl = reinterpret_cast<int *>(lds_raw + lo.ctl);
    const int Np = (N + 3) & ~3;

    // ---- W = theta + sign * eps[worker] (GTN_worker.py:165-175), staged once per chain: coalesced reads, transposed writes ----
    float *Wst;
    if constexpr (WLDS) Wst = reinterpret_cast<float *>(lds_raw + lo.W);
    else Wst = a.ws + chain * a.Ppad;
    {
        const float sg = a.eps ? a.sign[chain] : 0.0f;
        const float *e = a.eps ? a.eps + (int64_t)a.worker[chain] * y.P : nullptr;
        for (int64_t i = tid; i < y.P; i += NT)
            Wst[ql_se_staged_index(y, i, N, H, L)] = e ? fma32(sg, e[i], a.theta[i]) : a.theta[i];
    }
    const float *W = Wst;
    for (int i = tid; i < N * A; i += NT) { q[i] = 0.0; visits[i] = 0; }     // QL.py:25,33

    // ---- the agent: thread 0's registers ----
    const uint64_t key = a.rng_keys ? a.rng_keys[chain] : 0;
    const bool tape = cfg.rng_mode == LENV_RNG_TAPE;
    const bool sarsa = cfg.agent_kind == 1, cb = cfg.count_based != 0;
    const int k_rep = cfg.same_action_num > 1 ? cfg.same_action_num : 1;   // SE steps per chosen action
    int status = 0, episodes_run = 0, episode = 0, timed_out_at = -1;
    int64_t n_eps = 0, n_act = 0, train_steps = 0, learn_steps = 0, test_steps = 0;
    double eps_g = cfg.eps_init;
    int s = cfg.start_state, st = 0, ep_len = 0, ac = 0;
    float tr_reward = 0.0f, rsum = 0.0f;

    auto draw_u = [&]() -> double {                                        // random.random()
        double u;
        if (tape) { if (n_eps >= a.tapes.eps_uniform_stride) { status = -2; u = 1.0; } else u = a.tapes.eps_uniform[chain * a.tapes.eps_uniform_stride + n_eps]; }
        else u = u64_to_unit(rng_u64(key, STREAM_EPS, (uint64_t)n_eps));
        ++n_eps;
        return u;
    };
    auto draw_a = [&]() -> int {                                           // action_space.sample()
        int r;
        if (tape) {
            if (n_act >= a.tapes.rand_action_stride) { status = -3; r = 0; }
            else { r = a.tapes.rand_action[chain * a.tapes.rand_action_stride + n_act]; if (r < 0 || r >= A) { status = -3; r = 0; } }
        } else r = (int)u64_to_below(rng_u64(key, STREAM_ACTION, (uint64_t)n_act), (uint32_t)A);
        ++n_act;
        return r;
    };
    auto select = [&](int state) -> int {                                  // QL.select_train_action (QL.py:88-94): action | explored << 16
        if (draw_u() < eps_g) return draw_a() | (1 << 16);
        return qse_argmax_f32(q + state * A, A);
    };
    // BaseAgent.test on the REAL grid, as test_phase of ql_rn_inner_kernel: EnvWrapper.step's real branch (the repeats stop at done, python-float
    // reward sum), TimeLimit after max_steps env steps; `budgeted`: time_is_up before every episode (base_agent.py:177-184) and its padding
    auto test_phase = [&](bool budgeted, int64_t remaining) {
        int64_t used = 0;
        for (int te = 0; te < cfg.test_episodes; ++te) {
            if (budgeted && used > remaining) {
                double mn = -1e9;
                if (te > 0) { mn = rets[0]; for (int i = 1; i < te; ++i) if (rets[i] < mn) mn = rets[i]; }
                for (int i = te; i < cfg.test_episodes; ++i) rets[i] = mn;
                break;
            }
            int ts = cfg.start_state, dn = 0, el = 0;
            float ep_reward = 0.0f;                                        // fp32 tensor accumulation, base_agent.py:212
            for (int t = 0; t < cfg.max_steps && !dn; t += k_rep) {        // base_agent.py:194
                const int tac = qse_argmax_f32(q + ts * A, A);
                double rs = 0.0;
                for (int r_ = 0; r_ < k_rep; ++r_) {
                    dn = a.done[ts * A + tac];
                    rs = rs + a.reward[ts * A + tac];
                    ts = a.next_state[ts * A + tac];
                    ++test_steps; ++used; ++el;
                    if (el >= cfg.max_steps) dn = 1;
                    if (dn) break;
                }
                ep_reward = ep_reward + (float)rs;
            }
            rets[te] = (double)ep_reward;
        }
    };
    auto mean_rets = [&]() { double sm = 0.0; for (int i = 0; i < cfg.test_episodes; ++i) sm += rets[i]; return sm / (double)cfg.test_episodes; };
    // the head of BaseAgent.train's episode loop (base_agent.py:89-105): time-out, eps schedule, reset, the first action
    auto begin_episode = [&]() -> int {
        if (episode >= cfg.train_episodes) return QSE_END;
        if (cfg.step_budget > 0 && train_steps + test_steps > cfg.step_budget) { timed_out_at = episode; return QSE_END; }
        if (episode == 0) eps_g = cfg.eps_init;                            // QL.py:100-105
        else { eps_g *= cfg.eps_decay; if (eps_g < cfg.eps_min) eps_g = cfg.eps_min; }
        s = cfg.start_state; st = 0; ep_len = 0; tr_reward = 0.0f;         // VirtualEnv.reset: always the grid's S cell, one-hot
        return QSE_RESET;                                                  // (the caller selects the first action)
    };

    __syncthreads();                                                       // tables zeroed (and the staged theta visible)
    if (tid == 0) { const int m = begin_episode(); if (m == QSE_RESET) ac = select(s); ctl[0] = m; ctl[1] = ac & 0xffff; }
    __syncthreads();

    float *xc = xbuf, *xn = xbuf + Np;
    int64_t agent_step = 0;                                                // = thread 0's train_steps, kept by every thread (trace_se rows)
    for (;;) {
        const int mode = ctl[0], act = ctl[1];
        if (mode == QSE_END) break;
        if (mode == QSE_RESET) {
            for (int i = tid; i < N; i += NT) xc[i] = i == cfg.start_state ? 1.0f : 0.0f;
            __syncthreads();
        }
        for (int rep = 0; rep < k_rep; ++rep) {
            // A: first hidden layer of the three nets on [one_hot(act) | x].  The A one-hot columns come first in the canonical order; with
            // finite weights fmaf(0, w, z) = z and fmaf(1, w, +0) = w + 0, so the A steps collapse to the selected weight (+ 0.0f turns a
            // -0 weight into the chain's +0) -- exact, not an approximation
            for (int u = tid; u < U; u += NT) {
                float z = W[(int64_t)act * U + u] + 0.0f;
                const float *w = W + (int64_t)A * U + u;
                for (int k = 0; k < N; ++k) z = fma32(xc[k], w[(int64_t)k * U], z);
                z = z + W[y.off_b0 + u];
                h0[u] = act_fwd(cfg.rn_act, cfg.rn_prelu, z);
            }
            __syncthreads();
            const float *hin = h0;
            if (L == 2) {
                for (int u = tid; u < U; u += NT) {
                    const float *hp = h0 + (u / H) * H, *w = W + y.off_w1 + u;
                    float z = 0.0f;
                    for (int k = 0; k < H; ++k) z = fma32(hp[k], w[(int64_t)k * U], z);
                    z = z + W[y.off_b1 + u];
                    h1[u] = act_fwd(cfg.rn_act, cfg.rn_prelu, z);
                }
                __syncthreads();
                hin = h1;
            }
            // B: the outputs, lane = output: N next-state values (the raw vector stays the SE's state, virtual_env.py:52), reward, done
            for (int o = tid; o < O; o += NT) {
                const float *hp = hin + (o < N ? 0 : (o - N + 1) * H), *w = W + y.off_wo + o;
                float z = 0.0f;
                for (int j = 0; j < H; ++j) z = fma32(hp[j], w[(int64_t)j * O], z);
                z = z + W[y.off_bo + o];
                if (o < N) xn[o] = z; else rd[o - N] = z;
                if (a.trace_se && rep == k_rep - 1 && agent_step < a.out.trace_cap) a.trace_se[(chain * a.out.trace_cap + agent_step) * O + o] = z;
            }
            __syncthreads();
            if (tid == 0) rsum = rep == 0 ? rd[0] : rsum + rd[0];          // env_wrapper.py:26-29: fp32 tensors, step order, no stop at done
            float *t = xc; xc = xn; xn = t;
        }
        ++agent_step;
        // C: what the agent sees is argmax of the raw vector (from_one_hot_encoding = torch.argmax: the FIRST maximum, a NaN counting as the maximum)
        if (tid < 64) {
            float bv = -__builtin_inff();
            int bi = 0x7fffffff;
            for (int i = tid; i < N; i += 64) { const float v = xc[i]; if (bi == 0x7fffffff || qse_beats(v, bv)) { bv = v; bi = i; } }
            for (int off = 32; off >= 1; off >>= 1) {
                const float ov = __shfl_xor(bv, off, 64);
                const int oi = __shfl_xor(bi, off, 64);
                if (qse_beats(ov, bv) || (!qse_beats(bv, ov) && oi < bi)) { bv = ov; bi = oi; }   // a tie goes to the lower index
            }
            if (tid == 0) {
                const int s2 = bi, ai = ac & 0xffff;                       // ac = action | explored << 16
                const float dn = rd[1];                                    // the done net's raw output; no TimeLimit around a VirtualEnv
                const double r = (double)rsum;                             // reward.item()
                // QL.learn (QL.py:38-73) / SARSA.learn (SARSA.py:36-60), rb_size 1: batch_size times the latest transition
                if (episode >= cfg.init_episodes) {
                    for (int k = 0; k < cfg.batch_size; ++k) {
                        double boot;
                        if (sarsa) {                                       // next_action = select_train_action(next_state)
                            const int a2 = select(s2) & 0xffff;
                            boot = q[s2 * A + a2];
                        } else {
                            boot = q[s2 * A];
                            for (int i = 1; i < A; ++i) if (q[s2 * A + i] > boot) boot = q[s2 * A + i];
                        }
                        double rr = r;
                        if (cb) {                                          // QL.py:52-55
                            visits[s * A + ai] += 1;
                            rr += cfg.beta / (__builtin_sqrt((double)visits[s * A + ai]) + 1e-9);
                        }
                        const double delta = rr + cfg.gamma * boot * (dn < 0.5f ? 1.0 : 0.0) - q[s * A + ai];   // the bootstrap mask: done < 0.5
                        q[s * A + ai] += cfg.alpha * delta;
                    }
                    ++learn_steps;
                }
                if (a.out.trace_action && train_steps < a.out.trace_cap) {
                    const int64_t k = chain * a.out.trace_cap + train_steps;
                    a.out.trace_action[k] = ac;
                    a.out.trace_state[k * 2] = s; a.out.trace_state[k * 2 + 1] = s2;
                    a.out.trace_reward_done[k * 2] = rsum; a.out.trace_reward_done[k * 2 + 1] = dn;
                }
                s = s2;
                tr_reward = tr_reward + rsum;                              // base_agent.py:121, fp32 tensor
                ep_len += k_rep; st += k_rep; ++train_steps;
                int m = QSE_RUN;
                if (dn > 0.5f || st >= cfg.max_steps) {                    // the episode ends on done > 0.5 (base_agent.py:128) or with range()
                    ++episodes_run;
                    if (a.out.episode_len) a.out.episode_len[chain * cfg.train_episodes + episode] = ep_len;
                    // test_mode 1 = train(env) without a test env: the SE's own episode reward feeds the meter and the VIRTUAL rule applies
                    double tm;
                    if (cfg.test_mode == 1) tm = (double)tr_reward;
                    else { test_phase(false, 0); tm = mean_rets(); }
                    meter[episode] = tm;
                    if (a.out.episode_test_mean) a.out.episode_test_mean[chain * cfg.train_episodes + episode] = tm;
                    int solved = 0;
                    if (episode >= cfg.init_episodes)                      // base_agent.py:141-148
                        solved = meter_env_solved_inl(meter, episode + 1, cfg.early_out_num, cfg.test_mode == 1, cfg.solved_reward,
                                                      cfg.early_out_virtual_diff, episode, cfg.init_episodes);
                    ++episode;
                    m = solved ? QSE_END : begin_episode();
                }
                if (m != QSE_END) ac = select(s);
                ctl[0] = m; ctl[1] = ac & 0xffff;
            }
        }
        __syncthreads();
    }
    if (tid != 0) return;

    test_phase(cfg.step_budget > 0, cfg.step_budget - (train_steps + test_steps));
    a.out.score[chain] = mean_rets();
    if (a.out.final_returns) for (int i = 0; i < cfg.test_episodes; ++i) a.out.final_returns[chain * cfg.test_episodes + i] = rets[i];
    chain_write_stats(a.out, chain, episodes_run, train_steps, learn_steps, test_steps);
    chain_pad_episodes(a.out, chain, cfg.train_episodes, episodes_run, meter, timed_out_at);
    if (a.out.q_table) for (int i = 0; i < N * A; ++i) a.out.q_table[chain * N * A + i] = q[i];
    if (a.out.status) a.out.status[chain] = status;
}

}  // namespace lenv

using namespace lenv;

// what the loop takes: every layout of envs/gridworld.py with hidden_size <= 128, hidden_layer 1 or 2, the five activations
static int ql_se_check(const lenv_ql_cfg *cfg)
{
    if (!cfg) return LENV_ERR_INVALID;
    if (cfg->rn_hidden < 1 || cfg->rn_hidden > 128 || cfg->rn_layers < 1 || cfg->rn_layers > 2) return LENV_ERR_UNSUPPORTED;
    if (cfg->rn_act < LENV_ACT_IDENTITY || cfg->rn_act > LENV_ACT_PRELU) return LENV_ERR_UNSUPPORTED;
    if (cfg->rn_layer_norm && cfg->rn_layers >= 2) return LENV_ERR_UNSUPPORTED;      // config.ql_se_cfg_from_config refuses it by name
    if (cfg->n_states < 1 || cfg->n_states > 4096 || cfg->n_actions < 1 || cfg->n_actions > 16 || cfg->test_episodes < 1 || cfg->train_episodes < 0 ||
        cfg->max_steps < 1 || cfg->batch_size < 1 || cfg->start_state < 0 || cfg->start_state >= cfg->n_states)
        return LENV_ERR_UNSUPPORTED;
    if (cfg->agent_kind != 0 && cfg->agent_kind != 1) return LENV_ERR_UNSUPPORTED;
    if (cfg->rng_mode != LENV_RNG_COUNTER && cfg->rng_mode != LENV_RNG_TAPE) return LENV_ERR_UNSUPPORTED;
    if (ql_se_lds(*cfg).fixed_bytes > (size_t)QSE_LDS_MAX) return LENV_ERR_UNSUPPORTED;
    return LENV_OK;
}

static bool ql_se_theta_in_lds(const lenv_ql_cfg *cfg)
{
    return ql_se_lds(*cfg).fixed_bytes + sizeof(float) * (size_t)ql_se_layout(*cfg).P <= (size_t)QSE_LDS_MAX;
}

static int64_t ql_se_ppad(const lenv_ql_cfg *cfg) { return (ql_se_layout(*cfg).P + 63) & ~(int64_t)63; }

extern "C" int64_t lenv_ql_se_num_params(const lenv_ql_cfg *cfg)
{
    const int rc = ql_se_check(cfg);
    return rc != LENV_OK ? rc : ql_se_layout(*cfg).P;
}

extern "C" int64_t lenv_ql_se_lds_bytes(const lenv_ql_cfg *cfg)
{
    const int rc = ql_se_check(cfg);
    if (rc != LENV_OK) return rc;
    return (int64_t)(ql_se_lds(*cfg).fixed_bytes + (ql_se_theta_in_lds(cfg) ? sizeof(float) * (size_t)ql_se_layout(*cfg).P : 0));
}

extern "C" int64_t lenv_ql_se_workspace_bytes(const lenv_ql_cfg *cfg, int64_t chains)
{
    const int rc = ql_se_check(cfg);
    if (rc != LENV_OK) return rc;
    if (chains < 0) return LENV_ERR_INVALID;
    return ql_se_theta_in_lds(cfg) ? 0 : chains * ql_se_ppad(cfg) * (int64_t)sizeof(float);
}

extern "C" int lenv_ql_se_inner_loop(const lenv_ql_cfg *cfg, const float *theta, const float *eps, const int32_t *worker, const float *sign,
                                     const int32_t *next_state, const double *reward, const uint8_t *done, const uint64_t *rng_keys,
                                     const lenv_tapes *tapes, int64_t chains, const lenv_ql_out *out, float *trace_se, void *workspace,
                                     int64_t workspace_bytes, void *stream)
{
    if (!cfg || !theta || !next_state || !reward || !done || !out || !out->score || chains < 0) return LENV_ERR_INVALID;
    if (eps && (!worker || !sign)) return LENV_ERR_INVALID;
    if (cfg->rng_mode == LENV_RNG_TAPE && (!tapes || !tapes->eps_uniform || !tapes->rand_action)) return LENV_ERR_INVALID;
    if (cfg->rng_mode == LENV_RNG_COUNTER && !rng_keys) return LENV_ERR_INVALID;
    if (out->trace_cap > 0 && out->trace_action && (!out->trace_state || !out->trace_reward_done)) return LENV_ERR_INVALID;
    const int rc = ql_se_check(cfg);
    if (rc != LENV_OK) return rc;
    const int64_t need = lenv_ql_se_workspace_bytes(cfg, chains);
    if (need > 0 && (!workspace || workspace_bytes < need)) return LENV_ERR_WORKSPACE;
    if (chains == 0) return LENV_OK;
    QlSeArgs a;
    a.cfg = *cfg;
    a.theta = theta; a.eps = eps; a.worker = worker; a.sign = sign;
    a.next_state = next_state; a.reward = reward; a.done = done; a.rng_keys = rng_keys;
    if (tapes) a.tapes = *tapes; else a.tapes = lenv_tapes{};
    a.out = *out;
    a.trace_se = out->trace_cap > 0 ? trace_se : nullptr;
    a.ws = static_cast<float *>(workspace);
    a.Ppad = ql_se_ppad(cfg);
    const bool wlds = ql_se_theta_in_lds(cfg);
    const size_t lds_bytes = (size_t)lenv_ql_se_lds_bytes(cfg);
    int nt = 3 * cfg->rn_hidden > cfg->n_states + 2 ? 3 * cfg->rn_hidden : cfg->n_states + 2;
    nt = (nt + 63) & ~63;
    if (nt > QSE_NT_MAX) nt = QSE_NT_MAX;
    void (*kern)(const QlSeArgs) = wlds ? ql_se_inner_kernel<true> : ql_se_inner_kernel<false>;
    return lenv_host::launch(kern, dim3((unsigned)chains), dim3((unsigned)nt), lds_bytes, stream, a);
}
