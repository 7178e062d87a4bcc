/* ppo_icm_ref.c -- CPU restatement of PPO(icm=True) (reference agents/PPO.py:46-62,144-145,183-184 with models/icm_baseline.py) on a RewardEnv
 * over a continuous real env, in the canonical floating-point order of csrc/ppo_rn_inner_loop.hip's ppo_icm_segment_kernel.  TEST
 * INFRASTRUCTURE, compiled by tests/ppo_icm_ref.py like tests/ppo_ref.c, which it includes for its helpers (the nets, the per-row loss
 * derivatives, the env glue); the module is the oracle's own restatement, oracle/lenv_oracle_icm.inc, included for its static routines.
 *
 * ppo_icm_ref_chain is ppo_ref_chain with, inside every PPO.learn call on its n rows,
 *   - rewards[i] = rewards[i] + eta * mean_f (features(s'_i) - forward(s_i, a_i))^2 before the return scan, with the module as the previous
 *     call left it (icm_reward_rows: icm_forward and the reward lines of icm_train_and_reward);
 *   - one ICM.train step on all n rows after the last epoch (icm_train_and_reward with its rewards discarded), the module's Adam with a step
 *     counter of its own;
 * and a next-observation row per on-policy row (s' is not the next row's s at an episode end or with same_action_num > 1). */
#include "ppo_ref.c"

/* what oracle/lenv_oracle_icm.inc takes from lenv_oracle.c: linear_fwd, and act_bwd with the pre-activation as a third argument (unused by
 * the activations here: leakyrelu / relu keep its sign in the output) */
static void linear_fwd(const float *W, const float *b, int n_out, int n_in, const float *x, float *y)
{
    for (int o = 0; o < n_out; ++o) {
        float acc = 0.0f;
        const float *w = W + (int64_t)o * n_in;
        for (int k = 0; k < n_in; ++k) acc = fmaf(x[k], w[k], acc);
        y[o] = acc + b[o];
    }
}
#define act_bwd(act, prelu, z, a, g) (act_bwd)((act), (prelu), (a), (g))
#include "../oracle/lenv_oracle_icm.inc"
#undef act_bwd

typedef struct {
    int32_t feature_dim, hidden;
    double lr, beta, eta;
    const float *icm_init;     /* [P_icm] fresh ICMModel parameters, state-dict order */
    float *icm_final;          /* [P_icm] (may be NULL) */
    float *learn_icm;          /* [learn_cap, P_icm] the module's parameters after each recorded learn call (may be NULL) */
    float *learn_intr;         /* [learn_cap, rows] that call's intrinsic rewards (may be NULL) */
} ppo_icm;

int64_t ppo_icm_ref_num_params(const ppo_cfg *cfg, int F, int H) { return orc_icm_num_params_continuous(cfg->state_dim, cfg->action_dim, F, H); }

/* ICM.compute_intrinsic_rewards on rows [0, B): r[b] = eta * mean_f (features(s') - forward)^2 with the parameters p as they are */
static void icm_reward_rows(const icm_net *n, const float *p, float eta, const float *X, const float *XN, const float *ACT, int B, float *r)
{
    const int S = n->S, F = n->F;
    float *X2 = malloc(sizeof(float) * 2 * B * S);
    memcpy(X2, X, sizeof(float) * B * S); memcpy(X2 + (int64_t)B * S, XN, sizeof(float) * B * S);
    icm_acts t;
    icm_acts_alloc(&t, n, B);
    icm_forward(n, p, X2, ACT, B, &t);
    for (int b = 0; b < B; ++b) {
        float s = 0.0f;
        for (int f = 0; f < F; ++f) { const float d = t.fe[(int64_t)(B + b) * F + f] - t.pred[b * F + f]; s = fmaf(d, d, s); }
        r[b] = eta * (s / (float)F);
    }
    free(X2);
    icm_acts_free(&t);
}

int ppo_icm_ref_chain(const ppo_cfg *cfg, const ppo_icm *ic, const float *rn, const float *agent_init, uint64_t key, const ppo_tapes *tapes,
                      ppo_out *out)
{
    const int S = cfg->state_dim, A = cfg->action_dim, H = cfg->hidden, L = cfg->layers, env_id = cfg->env_id, T = cfg->test_episodes;
    if (!((env_id == ORC_ENV_CHEETAH_STANDIN && S == 17 && A == 6) || (env_id == ORC_ENV_PENDULUM && S == 3 && A == 1) || (env_id == ORC_ENV_CMC && S == 2 && A == 1))) return -1;
    if (H < 1 || H > PPO_MAXW || L < 1 || L > PPO_MAXL || T < 1) return -1;
    if (!ic || !ic->icm_init || ic->feature_dim < 1 || ic->feature_dim > 128 || ic->hidden < 1 || ic->hidden > 128) return -1;
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
    /* the chain's fresh ICM (PPO.py:46-62; continuous actions), its Adam state and step counter, the rows' next observations */
    icm_net inet;
    icm_build(&inet, S, A, ic->feature_dim, ic->hidden, 0);
    const icm_hp ihp = { ic->lr, ic->beta, ic->eta, cfg->adam_beta1, cfg->adam_beta2, cfg->adam_eps };
    float *ip = malloc(sizeof(float) * inet.P), *im = calloc(inet.P, sizeof(float)), *iv = calloc(inet.P, sizeof(float));
    memcpy(ip, ic->icm_init, sizeof(float) * inet.P);
    double ipows[2] = { 1.0, 1.0 };
    float *XN = malloc(sizeof(float) * N * S), *rintr = malloc(sizeof(float) * N), *packed = malloc(sizeof(float) * N * (2 * S + A));
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
            memcpy(XN + n_rows * S, next_state, sizeof(float) * S);
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
                /* rewards += icm.compute_intrinsic_rewards(states, next_states, actions): the module as the last call left it */
                icm_reward_rows(&inet, ip, (float)ic->eta, X, XN, ACT, (int)n, rintr);
                for (int64_t i = 0; i < n; ++i) REW[i] = REW[i] + rintr[i];
                if (ic->learn_intr && out->learn_n < out->learn_cap) memcpy(ic->learn_intr + out->learn_n * N, rintr, sizeof(float) * n);
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
                /* icm.train(states, next_states, actions): ICM.train is icm_train_and_reward with its rewards discarded */
                for (int64_t i = 0; i < n; ++i) {
                    float *row = packed + i * (2 * S + A);
                    memcpy(row, X + i * S, sizeof(float) * S); memcpy(row + S, ACT + i * A, sizeof(float) * A); memcpy(row + S + A, XN + i * S, sizeof(float) * S);
                }
                icm_train_and_reward(&inet, &ihp, ip, im, iv, ipows, packed, 2 * S + A, S + A, 0, (int)n, rintr);
                if (ic->learn_icm && out->learn_n < out->learn_cap) memcpy(ic->learn_icm + out->learn_n * inet.P, ip, sizeof(float) * inet.P);
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
    if (ic->icm_final) memcpy(ic->icm_final, ip, sizeof(float) * inet.P);
    free(ip); free(im); free(iv); free(XN); free(rintr); free(packed);
    free(par); free(am); free(av); free(grad); free(X); free(ACT); free(REW); free(DONE); free(RET); free(OLDLP); free(MEAN); free(V);
    free(DZ); free(GS); free(DV); free(d0); free(d1); free(meter); free(rets);
    for (int l = 0; l < PPO_MAXL; ++l) { free(ha[l]); free(hc[l]); }
    return err;
}
