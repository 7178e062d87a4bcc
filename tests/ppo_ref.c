/* ppo_ref.c -- CPU restatement of the PPO inner agent (reference agents/PPO.py, models/actor_critic.py:38-61,74-81) on a RewardEnv over a
 * continuous real env, in the canonical floating-point order of csrc/ppo_rn_inner_loop.hip.  TEST INFRASTRUCTURE: compiled by tests/ppo_ref.py
 * with the oracle Makefile's flags (-ffp-contract=off: an FMA only where fmaf is written) and linked against the oracle library, whose exported
 * primitives (env physics, tanh / exp / log, counter RNG, orc_mlp_forward for the reward net) it calls for everything that is pinned already.
 *
 * Order of every sum (what "bit for bit" means for the kernel):
 *   - a Linear output is the k-ascending fmaf chain from 0.0f, the bias added last with a plain add;
 *   - a weight gradient is the row-ascending fmaf chain from 0.0f over the N rows of the batch, a bias gradient the row-ascending plain sum;
 *   - an input gradient is the output-unit-ascending fmaf chain from 0.0f;
 *   - the discounted returns run backwards over the rows in fp32 (r + gamma * R, no fma); their mean and unbiased variance are left-to-right
 *     fp64 sums, rounded to fp32 once;
 *   - the per-row loss derivatives are written out in ppo_row_grads below, operation by operation.
 * Flat agent parameters: action_std [A] | actor.net | critic.net (state-dict order of Actor_PPO, then Critic_V). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../oracle/lenv_oracle.h"

void orc_pendulum_step(double st[2], const float *action, double *reward);
void orc_cmc_step(double st[2], const float *action, double *reward, int *done);
float orc_expf(float x);

typedef struct {             /* == lenv_ppo_cfg (include/lenv_hip.h) */
    int32_t env_id, state_dim, action_dim, max_steps;
    int32_t rn_hidden, rn_layers, rn_act;
    float rn_prelu;
    int32_t reward_env_type, info_dim;
    int32_t hidden, layers, act;
    float prelu;
    int32_t train_episodes, test_episodes, init_episodes, early_out_num;
    int32_t ppo_epochs, same_action_num, rng_mode, reserved;
    double solved_reward, gamma, lr, action_std, vf_coef, ent_coef, eps_clip, update_episodes;
    double adam_beta1, adam_beta2, adam_eps;
} ppo_cfg;

typedef struct {             /* tapes: rows available */
    const float *act_noise;    int64_t n_act_noise;     /* rows of A: _standard_normal in actor_old.forward while training */
    const float *test_noise;   int64_t n_test_noise;    /* rows of A: the same inside BaseAgent.test, episode by episode */
    const double *train_reset; int64_t n_train_reset;   /* rows of the env's own state */
    const double *test_reset;  int64_t n_test_reset;
} ppo_tapes;

typedef struct {
    int64_t trace_cap, trace_n;
    float *trace_action, *trace_state, *trace_next_state, *trace_reward, *trace_done;
    int64_t learn_cap, learn_n;
    int32_t *learn_step;       /* [learn_cap] rows collected over the whole run when the learn call fired */
    float *learn_params;       /* [learn_cap, P] parameters after the call */
    double *episode_test_mean; int32_t *episode_len; double *final_returns; float *final_params;
    double score; int32_t episodes_run; int64_t train_steps, learn_calls, test_steps;
} ppo_out;

enum { STREAM_TRAIN_RESET = 3, STREAM_TEST_RESET = 4, STREAM_PPO_ACT_NOISE = 13, STREAM_PPO_TEST_NOISE = 14 };
#define PPO_MAXW 128
#define PPO_MAXL 2

typedef struct { int in, H, L, out, oW[PPO_MAXL + 1], ob[PPO_MAXL + 1], P; } mlp_off;
static void mlp_offsets(mlp_off *m, int in, int H, int L, int out)
{
    int o = 0, n_in = in;
    m->in = in; m->H = H; m->L = L; m->out = out;
    for (int l = 0; l < L; ++l) { m->oW[l] = o; o += H * n_in; m->ob[l] = o; o += H; n_in = H; }
    m->oW[L] = o; o += out * H; m->ob[L] = o; o += out;
    m->P = o;
}

static float act_fwd(int act, float prelu, float z)
{
    switch (act) {
    case ORC_ACT_RELU: return z > 0.0f ? z : 0.0f;
    case ORC_ACT_LEAKYRELU: return z > 0.0f ? z : z * 0.01f;
    case ORC_ACT_TANH: return orc_tanhf(z);
    case ORC_ACT_PRELU: return z > 0.0f ? z : prelu * z;
    default: return z;
    }
}
static float act_bwd(int act, float prelu, float a, float g)
{
    switch (act) {
    case ORC_ACT_RELU: return a > 0.0f ? g : 0.0f;
    case ORC_ACT_LEAKYRELU: return a > 0.0f ? g : g * 0.01f;
    case ORC_ACT_TANH: return g * fmaf(-a, a, 1.0f);
    case ORC_ACT_PRELU: return a > 0.0f ? g : prelu * g;
    default: return g;
    }
}

/* one row through the net: hid[l] (H floats each, may be NULL) receive the hidden activations, y the raw outputs */
static void mlp_row(const mlp_off *m, int act, float prelu, const float *p, const float *x, float *y, float *const *hid)
{
    float buf[2][PPO_MAXW];
    const float *in = x;
    int n_in = m->in;
    for (int l = 0; l <= m->L; ++l) {
        const int last = l == m->L, n_out = last ? m->out : m->H;
        float *h = last ? y : (hid ? hid[l] : buf[l & 1]);
        for (int j = 0; j < n_out; ++j) {
            float z = 0.0f;
            for (int k = 0; k < n_in; ++k) z = fmaf(in[k], p[m->oW[l] + j * n_in + k], z);
            z = z + p[m->ob[l] + j];
            h[j] = last ? z : act_fwd(act, prelu, z);
        }
        in = h; n_in = m->H;
    }
}

/* gradients of the net's parameters for dOut [N][out]; hid[l] [N][H]; scratch d0, d1 [N][H] */
static void mlp_backward(const mlp_off *m, int act, float prelu, const float *p, const float *X, int64_t N, float *const *hid, const float *dOut,
                         float *g, float *d0, float *d1)
{
    const int H = m->H, O = m->out, L = m->L;
    for (int o = 0; o < O; ++o) {
        for (int h = 0; h < H; ++h) {
            float acc = 0.0f;
            for (int64_t i = 0; i < N; ++i) acc = fmaf(dOut[i * O + o], hid[L - 1][i * H + h], acc);
            g[m->oW[L] + o * H + h] = acc;
        }
        float s = 0.0f;
        for (int64_t i = 0; i < N; ++i) s = s + dOut[i * O + o];
        g[m->ob[L] + o] = s;
    }
    float *dcur = d0, *dnext = d1;
    for (int64_t i = 0; i < N; ++i)
        for (int h = 0; h < H; ++h) {
            float acc = 0.0f;
            for (int o = 0; o < O; ++o) acc = fmaf(dOut[i * O + o], p[m->oW[L] + o * H + h], acc);
            dcur[i * H + h] = act_bwd(act, prelu, hid[L - 1][i * H + h], acc);
        }
    for (int l = L - 1; l >= 0; --l) {
        const int n_in = l == 0 ? m->in : H;
        const float *inp = l == 0 ? X : hid[l - 1];
        for (int h = 0; h < H; ++h) {
            for (int k = 0; k < n_in; ++k) {
                float acc = 0.0f;
                for (int64_t i = 0; i < N; ++i) acc = fmaf(dcur[i * H + h], inp[i * n_in + k], acc);
                g[m->oW[l] + h * n_in + k] = acc;
            }
            float s = 0.0f;
            for (int64_t i = 0; i < N; ++i) s = s + dcur[i * H + h];
            g[m->ob[l] + h] = s;
        }
        if (l > 0) {
            for (int64_t i = 0; i < N; ++i)
                for (int k = 0; k < n_in; ++k) {
                    float acc = 0.0f;
                    for (int h = 0; h < H; ++h) acc = fmaf(dcur[i * H + h], p[m->oW[l] + h * n_in + k], acc);
                    dnext[i * n_in + k] = act_bwd(act, prelu, hid[l - 1][i * n_in + k], acc);
                }
            float *t = dcur; dcur = dnext; dnext = t;
        }
    }
}

/* log-probability of action a under Normal(mean, std), summed over the action dims (torch.distributions.Normal.log_prob, left to right) */
static float ppo_logprob(int A, const float *a, const float *mean, const float *std)
{
    float lp = 0.0f;
    for (int k = 0; k < A; ++k) {
        const float d = a[k] - mean[k], var = std[k] * std[k];
        const float t = (-(d * d)) / (2.0f * var) - (float)orc_log((double)std[k]) - 0.9189385332046727f;
        lp = k == 0 ? t : lp + t;
    }
    return lp;
}

/* per-row derivatives of loss.mean() (PPO.py:164-179).  std0 = action_std as the log-probability saw it, stdc = after evaluate's clamp to
 * >= 0.01 (what the entropy and autograd's saved tensors see).  Writes dz [A] (gradient of the actor net's raw outputs), gs [A] (the row's
 * share of the action_std gradient) and dv (gradient of the critic's output). */
static void ppo_row_grads(const ppo_cfg *cfg, int64_t N, const float *a, const float *mean, const float *std0, const float *stdc, float old_lp,
                          float ret, float v, float *dz, float *gs, float *dv)
{
    const int A = cfg->action_dim;
    const float inv_n = 1.0f / (float)N, lo = (float)(1.0 - cfg->eps_clip), hi = (float)(1.0 + cfg->eps_clip);
    const float lp = ppo_logprob(A, a, mean, std0);
    const float ratio = orc_expf(lp - old_lp);
    const float adv = ret - v;
    const float clipped = ratio < lo ? lo : (ratio > hi ? hi : ratio);
    const float surr1 = ratio * adv, surr2 = clipped * adv;
    const float g = -inv_n;                                    /* d loss.mean() / d min(surr1, surr2)_i */
    float dratio;
    if (surr1 < surr2) dratio = g * adv;
    else if (surr1 > surr2) dratio = (ratio >= lo && ratio <= hi) ? g * adv : 0.0f;
    else dratio = (ratio >= lo && ratio <= hi) ? g * adv : (g * 0.5f) * adv;      /* a tie splits the gradient; inside the clip range both halves reach the ratio */
    const float dlp = dratio * ratio;
    const float gent = -((float)cfg->ent_coef * inv_n);        /* d / d entropy_i */
    for (int k = 0; k < A; ++k) {
        const float d = a[k] - mean[k], var = std0[k] * std0[k];
        dz[k] = (dlp * (d / var)) * fmaf(-mean[k], mean[k], 1.0f);
        gs[k] = dlp * (((d * d) * stdc[k]) / (var * var) - 1.0f / stdc[k]) + gent / stdc[k];
    }
    *dv = (float)(cfg->vf_coef * 2.0 / (double)N) * (v - ret);
}

int64_t ppo_ref_rows(const ppo_cfg *cfg)
{
    const int k = cfg->same_action_num > 1 ? cfg->same_action_num : 1;
    int64_t n = 1;
    while (!((double)(n * k) / (double)cfg->max_steps > cfg->update_episodes)) ++n;
    return n;
}

int64_t ppo_ref_num_params(const ppo_cfg *cfg)
{
    mlp_off ma, mc;
    mlp_offsets(&ma, cfg->state_dim, cfg->hidden, cfg->layers, cfg->action_dim);
    mlp_offsets(&mc, cfg->state_dim, cfg->hidden, cfg->layers, 1);
    return cfg->action_dim + ma.P + mc.P;
}

static void env_reset_draw(int env_id, uint64_t key, uint32_t stream, int64_t ep, double *xs)
{
    const double pi = 3.141592653589793, unit = 1.0 / 9007199254740992.0;
    if (env_id == ORC_ENV_PENDULUM) {
        xs[0] = -pi + (2 * pi) * ((double)(orc_rng_u64(key, stream, (uint64_t)(ep * 2)) >> 11) * unit);
        xs[1] = -1.0 + 2.0 * ((double)(orc_rng_u64(key, stream, (uint64_t)(ep * 2 + 1)) >> 11) * unit);
    } else if (env_id == ORC_ENV_CMC) {
        xs[0] = -0.6 + 0.2 * ((double)(orc_rng_u64(key, stream, (uint64_t)(ep * 2)) >> 11) * unit);
        xs[1] = 0.0;
    } else for (int i = 0; i < 17; ++i) xs[i] = -0.1 + 0.2 * ((double)(orc_rng_u64(key, stream, (uint64_t)(ep * 17 + i)) >> 11) * unit);
}
static void env_obs(int env_id, const double *xs, float *obs)
{
    if (env_id == ORC_ENV_PENDULUM) { obs[0] = (float)orc_cos(xs[0]); obs[1] = (float)orc_sin(xs[0]); obs[2] = (float)xs[1]; }
    else if (env_id == ORC_ENV_CMC) { obs[0] = (float)xs[0]; obs[1] = (float)xs[1]; }
    else for (int i = 0; i < 17; ++i) obs[i] = (float)xs[i];
}
static int env_step(int env_id, double *xs, const float *action, double *reward)
{
    int done = 0;
    if (env_id == ORC_ENV_PENDULUM) orc_pendulum_step(xs, action, reward);
    else if (env_id == ORC_ENV_CMC) orc_cmc_step(xs, action, reward, &done);
    else orc_cheetah_step(xs, action, reward);
    return done;
}

static float rn_phi(const ppo_cfg *cfg, int Drn, const float *rn, const float *x)
{
    const orc_mlp_desc rd = { Drn, cfg->rn_hidden, cfg->rn_layers, 1, cfg->rn_act, cfg->rn_prelu, 0 };
    float phi = 0.0f;
    orc_mlp_forward(&rd, rn, x, 1, &phi, NULL);
    return phi;
}

static int env_solved(const double *meter, int n, int num, double solved_reward)      /* BaseAgent.env_solved, the real rule */
{
    int lo = n - num; if (lo < 0) lo = 0;
    double sm = 0.0;
    for (int i = lo; i < n; ++i) sm += meter[i];
    return sm / ((double)(n - lo) + 1e-9) >= solved_reward;
}

int ppo_ref_chain(const ppo_cfg *cfg, const float *rn, const float *agent_init, uint64_t key, const ppo_tapes *tapes, ppo_out *out)
{
    const int S = cfg->state_dim, A = cfg->action_dim, H = cfg->hidden, L = cfg->layers, env_id = cfg->env_id, T = cfg->test_episodes;
    if (!((env_id == ORC_ENV_CHEETAH_STANDIN && S == 17 && A == 6) || (env_id == ORC_ENV_PENDULUM && S == 3 && A == 1) || (env_id == ORC_ENV_CMC && S == 2 && A == 1))) return -1;
    if (H < 1 || H > PPO_MAXW || L < 1 || L > PPO_MAXL || T < 1) return -1;
    const int SD = env_id == ORC_ENV_CHEETAH_STANDIN ? 17 : 2, k_rep = cfg->same_action_num > 1 ? cfg->same_action_num : 1;
    const int tape = cfg->rng_mode == ORC_RNG_TAPE, t = cfg->reward_env_type;
    if (tape && !tapes) return -1;
    const int uses_info = t == 3 || t == 4 || t == 7 || t == 8 || t > 100, info_in = uses_info && t < 100;
    if (uses_info && (cfg->info_dim != 4 || env_id != ORC_ENV_CHEETAH_STANDIN)) return -1;
    const int info_dim = cfg->info_dim, Drn = info_in ? S + info_dim : S;
    mlp_off ma, mc;
    mlp_offsets(&ma, S, H, L, A);
    mlp_offsets(&mc, S, H, L, 1);
    const int oA = A, oC = A + ma.P, P = A + ma.P + mc.P;
    const int64_t N = ppo_ref_rows(cfg);
    float *par = malloc(sizeof(float) * P), *am = calloc(P, sizeof(float)), *av = calloc(P, sizeof(float)), *grad = calloc(P, sizeof(float));
    memcpy(par, agent_init, sizeof(float) * P);
    float std_old[8];
    memcpy(std_old, par, sizeof(float) * A);
    float *X = malloc(sizeof(float) * N * S), *ACT = malloc(sizeof(float) * N * A), *REW = malloc(sizeof(float) * N), *DONE = malloc(sizeof(float) * N);
    float *RET = malloc(sizeof(float) * N), *OLDLP = malloc(sizeof(float) * N), *MEAN = malloc(sizeof(float) * N * A), *V = malloc(sizeof(float) * N);
    float *DZ = malloc(sizeof(float) * N * A), *GS = malloc(sizeof(float) * N * A), *DV = malloc(sizeof(float) * N);
    float *ha[PPO_MAXL], *hc[PPO_MAXL], *d0 = malloc(sizeof(float) * N * H), *d1 = malloc(sizeof(float) * N * H);
    for (int l = 0; l < PPO_MAXL; ++l) { ha[l] = malloc(sizeof(float) * N * H); hc[l] = malloc(sizeof(float) * N * H); }
    double *meter = malloc(sizeof(double) * (cfg->train_episodes > 0 ? cfg->train_episodes : 1)), *rets = malloc(sizeof(double) * T);
    double pows[2] = { 1.0, 1.0 };
    const float g32 = (float)cfg->gamma;
    int64_t n_rows = 0, n_actn = 0, n_testn = 0, n_test_ep = 0, train_steps = 0, test_steps = 0, learn_calls = 0, time_step = 0;
    int err = 0, episodes_run = 0;
    out->trace_n = 0; out->learn_n = 0;

    /* actor_old.forward (actor_critic.py:45-49): clamp std_old to >= 0.001, a = tanh(net(s)) + z * std_old */
#define PPO_ACT(obs, noise, n_noise, counter, stream, act_out)                                                             \
    do {                                                                                                                     \
        float raw_[8];                                                                                                       \
        mlp_row(&ma, cfg->act, cfg->prelu, par + oA, (obs), raw_, NULL);                                                     \
        for (int k_ = 0; k_ < A; ++k_) {                                                                                     \
            if (std_old[k_] < 0.001f) std_old[k_] = 0.001f;                                                                  \
            float zn_;                                                                                                       \
            if (tape) { if ((counter) >= (n_noise)) { err = -7; zn_ = 0.0f; } else zn_ = (noise)[(counter) * A + k_]; }      \
            else zn_ = (float)orc_normal(key, (stream), (uint64_t)((counter) * A + k_));                                    \
            (act_out)[k_] = orc_tanhf(raw_[k_]) + zn_ * std_old[k_];                                                         \
        }                                                                                                                    \
    } while (0)
    /* BaseAgent.test: T episodes one after the other; counter mode: the noise of (episode, agent step) sits at a fixed index */
#define PPO_TEST_PHASE()                                                                                                     \
    for (int te = 0; te < T; ++te) {                                                                                         \
        double xs_[17]; float obs_[17], act_[8];                                                                             \
        if (tape) { if (n_test_ep >= tapes->n_test_reset) { err = -5; memset(xs_, 0, sizeof(xs_)); } else memcpy(xs_, tapes->test_reset + n_test_ep * SD, sizeof(double) * SD); } \
        else env_reset_draw(env_id, key, STREAM_TEST_RESET, n_test_ep, xs_);                                                 \
        const int64_t nag_ = (cfg->max_steps + k_rep - 1) / k_rep, noise0_ = tape ? n_testn : n_test_ep * nag_;               \
        int64_t used_ = 0;                                                                                                   \
        ++n_test_ep;                                                                                                         \
        float ep_reward = 0.0f;                                                                                              \
        int tt = 0, dn_ = 0;                                                                                                 \
        for (int ta = 0; ta < cfg->max_steps && !dn_; ta += k_rep) {                                                         \
            env_obs(env_id, xs_, obs_);                                                                                      \
            const int64_t idx_ = noise0_ + used_;                                                                            \
            PPO_ACT(obs_, tapes ? tapes->test_noise : NULL, tapes ? tapes->n_test_noise : 0, idx_, STREAM_PPO_TEST_NOISE, act_); \
            ++used_;                                                                                                         \
            double rsum_ = 0.0;                                                                                              \
            for (int r_ = 0; r_ < k_rep; ++r_) {                                                                             \
                double rew_;                                                                                                 \
                const int env_done_ = env_step(env_id, xs_, act_, &rew_);                                                    \
                rsum_ = rsum_ + rew_;                                                                                        \
                ++test_steps; ++tt;                                                                                          \
                if (env_done_ || tt >= cfg->max_steps) { dn_ = 1; break; }                                                   \
            }                                                                                                                \
            ep_reward = ep_reward + (float)rsum_;                                                                            \
        }                                                                                                                    \
        if (tape) n_testn += used_;                                                                                          \
        rets[te] = (double)ep_reward;                                                                                        \
    }

    for (int episode = 0; episode < cfg->train_episodes; ++episode) {
        double xs[17];
        float state[17], next_state[17], action[8], info[8] = { 0 };
        if (tape) { if (episode >= tapes->n_train_reset) { err = -5; memset(xs, 0, sizeof(xs)); } else memcpy(xs, tapes->train_reset + (int64_t)episode * SD, sizeof(double) * SD); }
        else env_reset_draw(env_id, key, STREAM_TRAIN_RESET, episode, xs);
        env_obs(env_id, xs, state);
        float phi_s = 0.0f;
        if (t == 1 || t == 2) phi_s = rn_phi(cfg, Drn, rn, state);
        int ep_len = 0, env_steps = 0;
        for (int step = 0; step < cfg->max_steps; step += k_rep) {
            time_step += k_rep;
            PPO_ACT(state, tapes ? tapes->act_noise : NULL, tapes ? tapes->n_act_noise : 0, n_actn, STREAM_PPO_ACT_NOISE, action);
            ++n_actn;
            /* EnvWrapper.step on the RewardEnv (env_wrapper.py:56-61): up to same_action_num env steps, python-float reward sum */
            double rsum = 0.0;
            float cur[24];
            memcpy(cur, state, sizeof(float) * S);
            int dn = 0;
            for (int r_ = 0; r_ < k_rep; ++r_) {
                double rew;
                const int env_done = env_step(env_id, xs, action, &rew);
                ++env_steps;
                dn = (env_done || env_steps >= cfg->max_steps) ? 1 : 0;
                env_obs(env_id, xs, next_state);
                const float r32 = (float)rew;
                if (uses_info) {
                    double ctrl = 0.0;
                    for (int k = 0; k < 6; ++k) ctrl = ctrl + (double)action[k] * (double)action[k];
                    info[0] = (float)xs[0]; info[1] = (float)xs[8]; info[2] = (float)xs[8]; info[3] = (float)(-0.1 * ctrl);
                }
                float phi_s2 = 0.0f, shaped, xin[24];       /* RewardEnv._calc_reward (reward_env.py:81-131), fp32 left to right */
                if (t > 100) { float acc = 0.0f; for (int k = 0; k < info_dim; ++k) acc = fmaf(info[k], rn[k], acc); phi_s2 = acc; }
                else if (t != 0) {
                    memcpy(xin, next_state, sizeof(float) * S);
                    if (info_in) memcpy(xin + S, info, sizeof(float) * info_dim);
                    phi_s2 = rn_phi(cfg, Drn, rn, xin);
                    if (t == 3 || t == 4) { memcpy(xin, cur, sizeof(float) * S); phi_s = rn_phi(cfg, Drn, rn, xin); }
                }
                switch (t) {
                case 0: shaped = r32; break;
                case 1: case 3: shaped = g32 * phi_s2 - phi_s; break;
                case 2: case 4: shaped = (r32 + g32 * phi_s2) - phi_s; break;
                case 5: case 7: case 101: shaped = phi_s2; break;
                default: shaped = r32 + phi_s2; break;
                }
                phi_s = phi_s2;
                rsum = rsum + (double)shaped;
                memcpy(cur, next_state, sizeof(float) * S);
                if (dn) break;
            }
            const float shaped_sum = (float)rsum, done_f = dn ? 1.0f : 0.0f;
            if (n_rows >= N) { err = -4; n_rows = N - 1; }
            memcpy(X + n_rows * S, state, sizeof(float) * S); memcpy(ACT + n_rows * A, action, sizeof(float) * A);
            REW[n_rows] = shaped_sum; DONE[n_rows] = done_f;
            ++n_rows;
            if (out->trace_reward && out->trace_n < out->trace_cap) {
                const int64_t k = out->trace_n++;
                memcpy(out->trace_action + k * A, action, sizeof(float) * A); memcpy(out->trace_state + k * S, state, sizeof(float) * S);
                memcpy(out->trace_next_state + k * S, next_state, sizeof(float) * S); out->trace_reward[k] = shaped_sum;
                if (out->trace_done) out->trace_done[k] = done_f;
            }
            memcpy(state, next_state, sizeof(float) * S);
            ep_len += k_rep; ++train_steps;
            if ((double)time_step / (double)cfg->max_steps > cfg->update_episodes) {
                /* ================= PPO.learn (PPO.py:136-188) on rows [0, n_rows) ================= */
                const int64_t n = n_rows;
                float *hida[PPO_MAXL], *hidc[PPO_MAXL];
                {   /* discounted returns: backwards, reset where done > 0.5; normalised with the unbiased std */
                    float disc = 0.0f;
                    for (int64_t i = n - 1; i >= 0; --i) {
                        if (DONE[i] > 0.5f) disc = 0.0f;
                        disc = REW[i] + g32 * disc;
                        RET[i] = disc;
                    }
                    double sm = 0.0, sq = 0.0;
                    for (int64_t i = 0; i < n; ++i) sm += (double)RET[i];
                    const double mean = sm / (double)n;
                    for (int64_t i = 0; i < n; ++i) { const double d = (double)RET[i] - mean; sq += d * d; }
                    const float meanf = (float)mean, stdf = (float)sqrt(sq / (double)(n - 1));
                    for (int64_t i = 0; i < n; ++i) RET[i] = (RET[i] - meanf) / (stdf + 1e-5f);
                }
                for (int it = 0; it < cfg->ppo_epochs; ++it) {
                    float std0[8], stdc[8];
                    for (int64_t i = 0; i < n; ++i) {
                        float raw[8];
                        for (int l = 0; l < L; ++l) { hida[l] = ha[l] + i * H; hidc[l] = hc[l] + i * H; }
                        mlp_row(&ma, cfg->act, cfg->prelu, par + oA, X + i * S, raw, hida);
                        for (int k = 0; k < A; ++k) MEAN[i * A + k] = orc_tanhf(raw[k]);
                        mlp_row(&mc, cfg->act, cfg->prelu, par + oC, X + i * S, V + i, hidc);
                    }
                    if (it == 0) {       /* old_logprobs = actor_old.evaluate(...): the same net, actor_old's own std */
                        for (int64_t i = 0; i < n; ++i) OLDLP[i] = ppo_logprob(A, ACT + i * A, MEAN + i * A, std_old);
                    }
                    for (int k = 0; k < A; ++k) { std0[k] = par[k]; if (par[k] < 0.01f) par[k] = 0.01f; stdc[k] = par[k]; }   /* evaluate's clamp, after the log-probabilities */
                    for (int64_t i = 0; i < n; ++i)
                        ppo_row_grads(cfg, n, ACT + i * A, MEAN + i * A, std0, stdc, OLDLP[i], RET[i], V[i], DZ + i * A, GS + i * A, DV + i);
                    for (int k = 0; k < A; ++k) { float s = 0.0f; for (int64_t i = 0; i < n; ++i) s = s + GS[i * A + k]; grad[k] = s; }
                    mlp_backward(&ma, cfg->act, cfg->prelu, par + oA, X, n, ha, DZ, grad + oA, d0, d1);
                    mlp_backward(&mc, cfg->act, cfg->prelu, par + oC, X, n, hc, DV, grad + oC, d0, d1);
                    {   /* torch.optim.Adam, one step counter for all parameters */
                        pows[0] *= cfg->adam_beta1; pows[1] *= cfg->adam_beta2;
                        const float neg_step = (float)(-(cfg->lr / (1.0 - pows[0]))), bc2_sqrt = (float)sqrt(1.0 - pows[1]);
                        const float w1 = (float)(1.0 - cfg->adam_beta1), w2 = (float)(1.0 - cfg->adam_beta2), beta2 = (float)cfg->adam_beta2, eps = (float)cfg->adam_eps;
                        for (int i = 0; i < P; ++i) {
                            const float mm = fmaf(w1, grad[i] - am[i], am[i]);
                            float vv = av[i] * beta2;
                            vv = fmaf(w2 * grad[i], grad[i], vv);
                            const float denom = sqrtf(vv) / bc2_sqrt + eps;
                            par[i] = par[i] + (neg_step * mm) / denom;
                            am[i] = mm; av[i] = vv;
                        }
                    }
                }
                memcpy(std_old, par, sizeof(float) * A);       /* actor_old.load_state_dict(actor.state_dict()) */
                if (out->learn_step && out->learn_n < out->learn_cap) {
                    out->learn_step[out->learn_n] = (int32_t)train_steps;
                    if (out->learn_params) memcpy(out->learn_params + out->learn_n * P, par, sizeof(float) * P);
                    ++out->learn_n;
                }
                ++learn_calls;
                n_rows = 0; time_step = 0;
            }
            if (dn) break;
        }
        ++episodes_run;
        if (out->episode_len) out->episode_len[episode] = ep_len;
        PPO_TEST_PHASE()
        double sm = 0.0;
        for (int i = 0; i < T; ++i) sm += rets[i];
        meter[episode] = sm / (double)T;
        if (out->episode_test_mean) out->episode_test_mean[episode] = meter[episode];
        if (episode >= cfg->init_episodes && env_solved(meter, episode + 1, cfg->early_out_num, cfg->solved_reward)) break;
    }
    for (int e = episodes_run; e < cfg->train_episodes; ++e) {
        if (out->episode_test_mean) out->episode_test_mean[e] = NAN;
        if (out->episode_len) out->episode_len[e] = 0;
    }
    PPO_TEST_PHASE()
#undef PPO_TEST_PHASE
#undef PPO_ACT
    if (out->final_returns) memcpy(out->final_returns, rets, sizeof(double) * T);
    {
        double sm = 0.0;
        for (int i = 0; i < T; ++i) sm += rets[i];
        out->score = sm / (double)T;
    }
    out->episodes_run = episodes_run; out->train_steps = train_steps; out->learn_calls = learn_calls; out->test_steps = test_steps;
    if (out->final_params) memcpy(out->final_params, par, sizeof(float) * P);
    free(par); free(am); free(av); free(grad); free(X); free(ACT); free(REW); free(DONE); free(RET); free(OLDLP); free(MEAN); free(V);
    free(DZ); free(GS); free(DV); free(d0); free(d1); free(meter); free(rets);
    for (int l = 0; l < PPO_MAXL; ++l) { free(ha[l]); free(hc[l]); }
    return err;
}
