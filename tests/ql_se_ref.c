/* ql_se_ref.c -- CPU restatement of the tabular agents (QL, SARSA, their count-based variants) on a gridworld VirtualEnv, the chain that
 * csrc/ql_se_inner_loop.hip runs: reference agents/GTN_worker.py:187-221 -> BaseAgent.train(env=virtual_env, test_env=real_env) -> agent.test.
 * TEST INFRASTRUCTURE: compiled by tests/ql_se_ref.py with the oracle Makefile's flags and linked against the oracle library; every SE step
 * goes through the oracle's exported orc_mlp_forward (k-ascending fmaf chain from 0.0f, bias added last), every counter draw through
 * orc_rng_u64.  The cfg struct is the product's own lenv_ql_cfg.
 *
 * What is restated (file:line of the reference):
 *   VirtualEnv.reset  envs/virtual_env.py:35-41   one-hot of the grid's S cell; the agent sees its argmax
 *   VirtualEnv.step   envs/virtual_env.py:43-54   three nets on cat(action_onehot, self.state); the RAW state-net output stays self.state
 *   EnvWrapper.step   envs/env_wrapper.py:17-49   same_action_num steps regardless of done, fp32 reward sum in step order, the last done;
 *                                                 the agent sees torch.argmax (first maximum) of the raw vector
 *   BaseAgent.train   agents/base_agent.py:64-153 range(0, max_steps, k); the episode ends on done > 0.5; no TimeLimit on a VirtualEnv
 *   QL / SARSA        agents/QL.py:38-106, agents/SARSA.py:36-91   fp64 table, argmax on the fp32 cast row, mask (done < 0.5)
 *   BaseAgent.test    on the REAL grid's tables (EnvWrapper.step's real branch: the repeats stop at done, python-float sum, TimeLimit). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../include/lenv_hip.h"
#include "../oracle/lenv_oracle.h"

typedef struct {
    const double *eps_uniform;  int64_t n_eps_uniform;     /* random.random() */
    const int32_t *rand_action; int64_t n_rand_action;     /* action_space.sample() */
} qse_tapes;

typedef struct {
    int64_t trace_cap, trace_n;
    int32_t *trace_action;       /* [cap] action | explored << 16 */
    int32_t *trace_state;        /* [cap, 2] agent-visible state, next state */
    float *trace_reward_done;    /* [cap, 2] summed reward, raw done */
    float *trace_se;             /* [cap, N + 2] raw outputs of the last SE step of the agent step */
    double *episode_test_mean; int32_t *episode_len; double *final_returns; double *q_table;
    double score; int32_t episodes_run, status; int64_t train_steps, learn_steps, test_steps;
    double min_q_gap;            /* smallest best-minus-second of an fp32 Q row at a greedy decision where the two differ (training and tests) */
} qse_out;

enum { STREAM_EPS = 0, STREAM_ACTION = 1 };

/* torch.argmax's order: a NaN is the maximum, two NaNs tie */
static int beats(float a, float b) { return (a != a && b == b) || a > b; }

static void se_descs(const lenv_ql_cfg *c, orc_mlp_desc d[3])
{
    for (int n = 0; n < 3; ++n) {
        d[n].in_dim = c->n_actions + c->n_states; d[n].hidden = c->rn_hidden; d[n].layers = c->rn_layers;
        d[n].out_dim = n == 0 ? c->n_states : 1; d[n].act = c->rn_act; d[n].prelu = c->rn_prelu; d[n].use_layer_norm = 0;
    }
}

int64_t ql_se_ref_num_params(const lenv_ql_cfg *c)
{
    orc_mlp_desc d[3];
    se_descs(c, d);
    return orc_mlp_num_params(&d[0]) + orc_mlp_num_params(&d[1]) + orc_mlp_num_params(&d[2]);
}

/* one VirtualEnv.step: out [N + 2] = raw next-state vector | reward | done from the raw state vector x [N] and the action index */
int ql_se_ref_step(const lenv_ql_cfg *c, const float *theta, const float *x, int32_t action, float *out)
{
    orc_mlp_desc d[3];
    const int N = c->n_states, A = c->n_actions;
    float *in = (float *)malloc(sizeof(float) * (size_t)(A + N));
    int rc = 0;
    if (!in) return -1;
    se_descs(c, d);
    for (int i = 0; i < A; ++i) in[i] = i == action ? 1.0f : 0.0f;      /* action first (virtual_env.py:49) */
    memcpy(in + A, x, sizeof(float) * (size_t)N);
    const float *p = theta;
    rc |= orc_mlp_forward(&d[0], p, in, 1, out, NULL); p += orc_mlp_num_params(&d[0]);
    rc |= orc_mlp_forward(&d[1], p, in, 1, out + N, NULL); p += orc_mlp_num_params(&d[1]);
    rc |= orc_mlp_forward(&d[2], p, in, 1, out + N + 1, NULL);
    free(in);
    return rc;
}

typedef struct {
    const lenv_ql_cfg *c; const qse_tapes *tp; uint64_t key; int64_t n_eps, n_act; int status; double eps; const double *q; double min_gap;
} agent_t;

static int argmax_f32(agent_t *g, const double *row, int n)
{
    int best = 0;
    float bv = (float)row[0], second = -INFINITY;
    for (int i = 1; i < n; ++i) { const float v = (float)row[i]; if (v > bv) { second = bv; bv = v; best = i; } else if (v > second) second = v; }
    if (n > 1 && bv != second && (double)bv - (double)second < g->min_gap) g->min_gap = (double)bv - (double)second;
    return best;
}

static double draw_u(agent_t *g)
{
    double u;
    if (g->c->rng_mode == LENV_RNG_TAPE) { if (g->n_eps >= g->tp->n_eps_uniform) { g->status = -2; u = 1.0; } else u = g->tp->eps_uniform[g->n_eps]; }
    else u = (double)(orc_rng_u64(g->key, STREAM_EPS, (uint64_t)g->n_eps) >> 11) * (1.0 / 9007199254740992.0);
    ++g->n_eps;
    return u;
}

static int draw_a(agent_t *g)
{
    int r;
    const int A = g->c->n_actions;
    if (g->c->rng_mode == LENV_RNG_TAPE) {
        if (g->n_act >= g->tp->n_rand_action) { g->status = -3; r = 0; }
        else { r = g->tp->rand_action[g->n_act]; if (r < 0 || r >= A) { g->status = -3; r = 0; } }
    } else r = (int)(((orc_rng_u64(g->key, STREAM_ACTION, (uint64_t)g->n_act) >> 32) * (uint64_t)A) >> 32);
    ++g->n_act;
    return r;
}

static int select_action(agent_t *g, int state, int *explored)
{
    if (draw_u(g) < g->eps) { *explored = 1; return draw_a(g); }
    *explored = 0;
    return argmax_f32(g, g->q + (size_t)state * g->c->n_actions, g->c->n_actions);
}

/* BaseAgent.env_solved over the meter's list (utils.py:94-105: a slice sum over (len + 1e-9)) */
static int env_solved(const double *meter, int n, int num, int virtual_rule, double solved_reward, double virtual_diff, int episode, int init_episodes)
{
    int lo = n - num; if (lo < 0) lo = 0;
    double sm = 0.0;
    for (int i = lo; i < n; ++i) sm += meter[i];
    const double avg = sm / ((double)(n - lo) + 1e-9);
    if (!virtual_rule) return avg >= solved_reward;
    int hi2 = n - num; if (hi2 < 0) hi2 = 0;
    int lo2 = n - 2 * num; if (lo2 < 0) lo2 = 0;
    double s2 = 0.0;
    for (int i = lo2; i < hi2; ++i) s2 += meter[i];
    const double last = s2 / ((double)(hi2 - lo2) + 1e-9);
    return fabs(avg - last) / (fabs(last) + 1e-9) < virtual_diff && episode >= init_episodes + num;
}

int ql_se_ref_chain(const lenv_ql_cfg *c, const float *theta, const int32_t *t_next, const double *t_reward, const uint8_t *t_done,
                    uint64_t key, const qse_tapes *tp, qse_out *o)
{
    const int N = c->n_states, A = c->n_actions, k_rep = c->same_action_num > 1 ? c->same_action_num : 1;
    double *q = (double *)calloc((size_t)N * A, sizeof(double));
    int *visits = (int *)calloc((size_t)N * A, sizeof(int));
    double *meter = (double *)calloc((size_t)(c->train_episodes > 0 ? c->train_episodes : 1), sizeof(double));
    double *rets = (double *)calloc((size_t)c->test_episodes, sizeof(double));
    float *x = (float *)malloc(sizeof(float) * (size_t)N), *se = (float *)malloc(sizeof(float) * (size_t)(N + 2));
    agent_t g = { c, tp, key, 0, 0, 0, c->eps_init, q, INFINITY };
    int episodes_run = 0, timed_out_at = -1;
    int64_t train_steps = 0, learn_steps = 0, test_steps = 0;
    o->trace_n = 0;

#define TEST_PHASE(budgeted, remaining)                                                                                         \
    do {                                                                                                                        \
        int64_t used = 0;                                                                                                       \
        for (int te = 0; te < c->test_episodes; ++te) {                                                                         \
            if ((budgeted) && used > (remaining)) {                                                                             \
                double mn = -1e9;                                                                                               \
                if (te > 0) { mn = rets[0]; for (int i = 1; i < te; ++i) if (rets[i] < mn) mn = rets[i]; }                      \
                for (int i = te; i < c->test_episodes; ++i) rets[i] = mn;                                                       \
                break;                                                                                                          \
            }                                                                                                                   \
            int ts = c->start_state, dn = 0, el = 0;                                                                            \
            float ep_reward = 0.0f;                                                                                             \
            for (int t = 0; t < c->max_steps && !dn; t += k_rep) {                                                              \
                const int tac = argmax_f32(&g, q + (size_t)ts * A, A);                                                          \
                double rs = 0.0;                                                                                                \
                for (int r_ = 0; r_ < k_rep; ++r_) {                                                                            \
                    dn = t_done[ts * A + tac];                                                                                  \
                    rs = rs + t_reward[ts * A + tac];                                                                           \
                    ts = t_next[ts * A + tac];                                                                                  \
                    ++test_steps; ++used; ++el;                                                                                 \
                    if (el >= c->max_steps) dn = 1;                                                                             \
                    if (dn) break;                                                                                              \
                }                                                                                                               \
                ep_reward = ep_reward + (float)rs;                                                                              \
            }                                                                                                                   \
            rets[te] = (double)ep_reward;                                                                                       \
        }                                                                                                                       \
    } while (0)

    for (int episode = 0; episode < c->train_episodes; ++episode) {
        if (c->step_budget > 0 && train_steps + test_steps > c->step_budget) { timed_out_at = episode; break; }
        if (episode == 0) g.eps = c->eps_init;
        else { g.eps *= c->eps_decay; if (g.eps < c->eps_min) g.eps = c->eps_min; }
        int s = c->start_state, ep_len = 0;
        float tr_reward = 0.0f;
        for (int i = 0; i < N; ++i) x[i] = i == c->start_state ? 1.0f : 0.0f;
        for (int st = 0; st < c->max_steps; st += k_rep) {
            int explored;
            const int ac = select_action(&g, s, &explored);
            float rsum = 0.0f;
            for (int rep = 0; rep < k_rep; ++rep) {                       /* regardless of done */
                ql_se_ref_step(c, theta, x, ac, se);
                memcpy(x, se, sizeof(float) * (size_t)N);
                rsum = rep == 0 ? se[N] : rsum + se[N];
            }
            const float dn = se[N + 1];
            int s2 = 0;
            for (int i = 1; i < N; ++i) if (beats(x[i], x[s2])) s2 = i;    /* torch.argmax: the first maximum, a NaN counting as the maximum */
            const double r = (double)rsum;
            if (episode >= c->init_episodes) {
                for (int k = 0; k < c->batch_size; ++k) {
                    double boot;
                    if (c->agent_kind == 1) { int e2; const int a2 = select_action(&g, s2, &e2); boot = q[s2 * A + a2]; }
                    else { boot = q[s2 * A]; for (int i = 1; i < A; ++i) if (q[s2 * A + i] > boot) boot = q[s2 * A + i]; }
                    double rr = r;
                    if (c->count_based) { visits[s * A + ac] += 1; rr += c->beta / (sqrt((double)visits[s * A + ac]) + 1e-9); }
                    const double delta = rr + c->gamma * boot * (dn < 0.5f ? 1.0 : 0.0) - q[s * A + ac];
                    q[s * A + ac] += c->alpha * delta;
                }
                ++learn_steps;
            }
            if (o->trace_action && train_steps < o->trace_cap) {
                const int64_t k = train_steps;
                o->trace_action[k] = ac | (explored << 16);
                o->trace_state[k * 2] = s; o->trace_state[k * 2 + 1] = s2;
                o->trace_reward_done[k * 2] = rsum; o->trace_reward_done[k * 2 + 1] = dn;
                if (o->trace_se) memcpy(o->trace_se + k * (N + 2), se, sizeof(float) * (size_t)(N + 2));
                o->trace_n = k + 1;
            }
            s = s2;
            tr_reward = tr_reward + rsum;
            ep_len += k_rep; ++train_steps;
            if (dn > 0.5f) break;
        }
        ++episodes_run;
        o->episode_len[episode] = ep_len;
        double tm;
        if (c->test_mode == 1) tm = (double)tr_reward;
        else {
            TEST_PHASE(0, 0);
            double sm = 0.0;
            for (int i = 0; i < c->test_episodes; ++i) sm += rets[i];
            tm = sm / (double)c->test_episodes;
        }
        meter[episode] = tm;
        o->episode_test_mean[episode] = tm;
        if (episode >= c->init_episodes &&
            env_solved(meter, episode + 1, c->early_out_num, c->test_mode == 1, c->solved_reward, c->early_out_virtual_diff, episode, c->init_episodes))
            break;
    }
    TEST_PHASE(c->step_budget > 0, c->step_budget - (train_steps + test_steps));
    {
        double sm = 0.0;
        for (int i = 0; i < c->test_episodes; ++i) { sm += rets[i]; o->final_returns[i] = rets[i]; }
        o->score = sm / (double)c->test_episodes;
    }
    double pad_r = NAN;
    int pad_l = 0;
    if (timed_out_at >= 0) {
        pad_r = -1e9; pad_l = 1000000000;
        if (episodes_run > 0) {
            pad_r = meter[0]; pad_l = o->episode_len[0];
            for (int i = 1; i < episodes_run; ++i) { if (meter[i] < pad_r) pad_r = meter[i]; if (o->episode_len[i] > pad_l) pad_l = o->episode_len[i]; }
        }
    }
    for (int e = episodes_run; e < c->train_episodes; ++e) { o->episode_test_mean[e] = pad_r; o->episode_len[e] = pad_l; }
    memcpy(o->q_table, q, sizeof(double) * (size_t)N * A);
    o->episodes_run = episodes_run; o->status = g.status; o->train_steps = train_steps; o->learn_steps = learn_steps; o->test_steps = test_steps;
    o->min_q_gap = g.min_gap;
    free(q); free(visits); free(meter); free(rets); free(x); free(se);
    return 0;
}
