// ql_test_population.hip -- BaseAgent.test (agents/base_agent.py:155-227) with QL.select_test_action / SARSA.select_test_action for a whole
// population of trained tabular agents in one launch: agent i, a python-float64 Q-table, runs cfg->test_episodes greedy episodes on the grid
// MDP given as transition tables and, when asked, records every transition it visits -- the replay buffer the reference's test() returns,
// whose visited states are the heatmap of GTNC_evaluate_gridworld_heatmap.py.
//
// The walk is the repeat form of test_phase in ql_rn_inner_loop.hip (its k_rep > 1 branch, which covers k_rep = 1): start_state, the
// first-maximum argmax of the fp32-cast Q row (ql_argmax_f32 of lenv_ql_policy.cuh, shared with the fused kernel), the action
// same_action_num times or until done, the repeats' rewards summed in fp64 and rounded once to fp32 onto an fp32 episode return; every
// gridworld is wrapped in gym's TimeLimit (envs/env_factory.py:65-89), so the max_steps-th env step of an episode reports done.
//
// One thread per (agent, episode), no LDS.  Not a throughput kernel: a greedy walk on a deterministic grid is serial and short, and the
// episodes of an agent are the same walk -- the reference runs them all, and so do the rows.
#include <hip/hip_runtime.h>
#include "../../include/lenv_hip.h"
#include "lenv_ql_policy.cuh"
#include "lenv_host.h"

namespace lenv {

constexpr int QT_NT = 64;                      // threads of a workgroup
constexpr int QT_MAXA = 8, QT_MAXT = 128;

struct QtArgs {
    int N, A, start, max_steps, T, k_rep, cap;
    int64_t agents;
    const double *q_table; const int32_t *next_state; const double *reward; const uint8_t *done;
    double *returns; int32_t *env_steps, *agent_steps;
    int32_t *row_state, *row_action, *row_next_state; float *row_reward, *row_done;
};

__global__ __launch_bounds__(QT_NT) void ql_test_population_kernel(const QtArgs a)
{
    const int64_t ep = (int64_t)blockIdx.x * QT_NT + threadIdx.x;     // (agent, episode) in the [agents, T] outputs
    if (ep >= a.agents * a.T) return;
    const int64_t agent = ep / a.T;
    const int A = a.A;
    const double *q = a.q_table + agent * (int64_t)a.N * A;
    int s = a.start, dn = 0, el = 0, n_agent = 0;
    float ep_reward = 0.0f;                                            // fp32 tensor accumulation, base_agent.py:212
    for (int st = 0; st < a.max_steps && !dn; st += a.k_rep) {        // base_agent.py:194 range(0, max_steps, same_action_num)
        const int s0 = s, ac = ql_argmax_f32(q + (int64_t)s * A, A);
        double rsum = 0.0;                                             // EnvWrapper.step: python-float sum, the repeats stop at done
        for (int r_ = 0; r_ < a.k_rep; ++r_) {
            dn = a.done[s * A + ac];
            rsum = rsum + a.reward[s * A + ac];
            s = a.next_state[s * A + ac];
            ++el;
            if (el >= a.max_steps) dn = 1;                             // gym.wrappers.TimeLimit
            if (dn) break;
        }
        const float r32 = (float)rsum;
        ep_reward = ep_reward + r32;
        if (a.row_state) {
            const int64_t slot = ep * a.cap + n_agent;
            a.row_state[slot] = s0; a.row_action[slot] = ac; a.row_next_state[slot] = s;
            a.row_reward[slot] = r32; a.row_done[slot] = dn ? 1.0f : 0.0f;
        }
        ++n_agent;
    }
    a.returns[ep] = (double)ep_reward; a.env_steps[ep] = el; a.agent_steps[ep] = n_agent;
}

}  // namespace lenv

using namespace lenv;

// the entry's own checks of cfg (only the fields the kernel reads) into the launch's shape
static int qt_shape(const lenv_ql_cfg *cfg, QtArgs &a)
{
    if (cfg->max_steps < 1) return LENV_ERR_INVALID;
    if (cfg->n_actions < 1 || cfg->n_actions > QT_MAXA || cfg->test_episodes < 1 || cfg->test_episodes > QT_MAXT || cfg->same_action_num < 0 ||
        cfg->same_action_num > TP_MAX_REPEAT || cfg->n_states < 1 || cfg->start_state < 0 || cfg->start_state >= cfg->n_states ||
        (int64_t)cfg->n_states * cfg->n_actions > 0x7fffffff)
        return LENV_ERR_UNSUPPORTED;
    a.N = cfg->n_states; a.A = cfg->n_actions; a.start = cfg->start_state; a.max_steps = cfg->max_steps; a.T = cfg->test_episodes;
    lenv_host::tp_repeat(a, cfg->max_steps, cfg->same_action_num);
    return LENV_OK;
}

extern "C" int64_t lenv_ql_test_rows_cap(const lenv_ql_cfg *cfg)
{
    if (!cfg) return LENV_ERR_INVALID;
    QtArgs a{};
    const int rc = qt_shape(cfg, a);
    return rc != LENV_OK ? rc : a.cap;
}

extern "C" int lenv_ql_test_population(const lenv_ql_cfg *cfg, const double *q_table, const int32_t *next_state, const double *reward,
                                       const uint8_t *done, int64_t agents, double *returns, int32_t *env_steps, int32_t *agent_steps,
                                       int32_t *row_state, int32_t *row_action, int32_t *row_next_state, float *row_reward, float *row_done,
                                       void *stream)
{
    int rc = lenv_host::tp_check_args({ cfg, q_table, next_state, reward, done, returns, env_steps, agent_steps }, agents, row_state, row_action, row_next_state,
                                      row_reward, row_done);
    if (rc != LENV_OK) return rc;
    QtArgs a{};
    rc = qt_shape(cfg, a);
    if (rc != LENV_OK || agents == 0) return rc;
    if ((rc = lenv_host::tp_agents_rc(agents, 0x7fffffff / QT_MAXT)) != LENV_OK) return rc;
    a.agents = agents; a.q_table = q_table; a.next_state = next_state; a.reward = reward; a.done = done;
    a.returns = returns; a.env_steps = env_steps; a.agent_steps = agent_steps;
    a.row_state = row_state; a.row_action = row_action; a.row_next_state = row_next_state; a.row_reward = row_reward; a.row_done = row_done;
    const int64_t eps = agents * a.T;
    return lenv_host::launch(ql_test_population_kernel, dim3((unsigned)((eps + QT_NT - 1) / QT_NT)), dim3(QT_NT), 0, stream, a);
}
