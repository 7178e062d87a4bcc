// lenv_host.h -- the host-side launch path the fused inner loops share (library-internal, host code only).  Plain functions and small templates over
// each family's own cfg / tapes / out / Args types: the Args structs are kernel arguments, so they have no common base and are filled BY NAME here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>

#include "../../include/lenv_hip.h"
#include "lenv_device.cuh"
#include "lenv_tp_layout.h"       // TP_TB and tp_lds_layout: the test-population kernels' own layout function, read by tp_launch_plan

namespace lenv_host {

// Carves one chain's arena: every buffer starts on a multiple of 4 floats (16 bytes), the chain's stride is a multiple of 64 floats.
struct ArenaCursor {
    int64_t off = 0;
    int64_t take(int64_t n) { const int64_t r = off; off += (n + 3) & ~(int64_t)3; return r; }
    int64_t total() const { return (off + 63) & ~(int64_t)63; }
};

struct Segment { bool on; int32_t begin, end; int64_t *resume; };   // episodes [begin, end) of a resumable launch; `on` false = one whole launch

// The argument rules every fused inner loop has (each LENV_ERR_INVALID at the entry point).  A family's own rules (theta, the members of
// its tapes, its trace pointers) stay in its launcher.  hp: null for families without per-chain hyper-parameters.
template <class Cfg, class Tapes, class Out>
inline bool launch_args_ok(const Cfg *cfg, const lenv_chain_hp *hp, const float *eps, const int32_t *worker, const float *sign, const float *agent_init,
                           const uint64_t *rng_keys, const Tapes *tapes, int64_t chains, const void *workspace, const Out *out, const Segment &seg)
{
    if (!cfg || !agent_init || !out || !out->score || !workspace || chains < 0) return false;
    if (hp && (!hp->lr || !hp->batch_size || !hp->q_hidden || !hp->q_layers)) return false;
    if (eps && (!worker || !sign)) return false;
    if (cfg->rng_mode == LENV_RNG_TAPE && !tapes) return false;
    if (cfg->rng_mode == LENV_RNG_COUNTER && !rng_keys) return false;
    if (seg.on && (!seg.resume || seg.begin < 0 || seg.begin >= seg.end || seg.end > cfg->train_episodes)) return false;
    return true;
}
template <class Cfg> inline bool icm_args_ok(const Cfg *cfg, const lenv_icm_io *icm) { return !cfg->icm_enabled || (icm && icm->icm_init); }   // (cfg non-null)

// the population of a launch: theta and its perturbation, the agents' start parameters, the chains' RNG keys
template <class Args>
inline void fill_population(Args &a, const float *theta, const float *eps, const int32_t *worker, const float *sign, const float *agent_init,
                            const uint64_t *rng_keys)
{
    a.theta = theta; a.eps = eps; a.worker = worker; a.sign = sign; a.agent_init = agent_init; a.rng_keys = rng_keys;
}
template <class Args, class Cfg, class Tapes, class Out>
inline void fill_args(Args &a, const Cfg *cfg, const float *theta, const float *eps, const int32_t *worker, const float *sign, const float *agent_init,
                      const uint64_t *rng_keys, const Tapes *tapes, void *workspace, const Out *out)
{
    a.cfg = *cfg;
    fill_population(a, theta, eps, worker, sign, agent_init, rng_keys);
    a.tapes = tapes ? *tapes : Tapes{};
    a.arena = static_cast<float *>(workspace);
    a.out = *out;
}
template <class Args> inline void fill_hp(Args &a, const lenv_chain_hp *hp)
{
    a.hp_lr = hp ? hp->lr : nullptr; a.hp_batch = hp ? hp->batch_size : nullptr;
    a.hp_hidden = hp ? hp->q_hidden : nullptr; a.hp_layers = hp ? hp->q_layers : nullptr;
}
template <class Args, class Cfg> inline void fill_segment(Args &a, const Cfg *cfg, const Segment &seg)
{
    a.ep_begin = seg.on ? seg.begin : 0; a.ep_end = seg.on ? seg.end : cfg->train_episodes; a.resume = seg.on ? seg.resume : nullptr;
}
template <class Args, class Cfg> inline void fill_icm(Args &a, const Cfg *cfg, const lenv_icm_io *icm)
{
    a.icm_init = cfg->icm_enabled ? icm->icm_init : nullptr; a.icm_final = cfg->icm_enabled ? icm->icm_final : nullptr;
}

// The launch tail: the kernel's dynamic-LDS limit, the launch, the launch's error as a LENV code.
template <class... P, class... A>
inline int launch(void (*kern)(P...), dim3 grid, dim3 block, size_t lds_bytes, void *stream, const A &...args)
{
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
        return LENV_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, grid, block, lds_bytes, static_cast<hipStream_t>(stream), args...);
    return hipGetLastError() == hipSuccess ? LENV_OK : LENV_ERR_LAUNCH;
}

// ---- the test-population entries (agent / actor / discrete_actor / ql _test_population.hip) ----

// `required` (cfg, the inputs, the three per-episode outputs) all given, agents >= 0, and the five row arrays all or none: else LENV_ERR_INVALID
inline int tp_check_args(std::initializer_list<const void *> required, int64_t agents, const void *row_state, const void *row_action,
                         const void *row_next_state, const void *row_reward, const void *row_done)
{
    for (const void *p : required) if (!p) return LENV_ERR_INVALID;
    if (agents < 0) return LENV_ERR_INVALID;
    const int n_rows = (row_state != nullptr) + (row_action != nullptr) + (row_next_state != nullptr) + (row_reward != nullptr) + (row_done != nullptr);
    return n_rows != 0 && n_rows != 5 ? LENV_ERR_INVALID : LENV_OK;
}

// behind the shape checks and the `agents == 0` return: more agents than the grid (or the entry's index arithmetic) takes
inline int tp_agents_rc(int64_t agents, int64_t max_agents) { return agents > max_agents ? LENV_ERR_UNSUPPORTED : LENV_OK; }

// base_agent.py:194 range(0, max_steps, same_action_num): env steps per agent step, and the agent steps (the rows) an episode can take
template <class Args> inline void tp_repeat(Args &a, int max_steps, int same_action_num)
{
    a.k_rep = same_action_num > 1 ? same_action_num : 1;
    a.cap = (max_steps + a.k_rep - 1) / a.k_rep;
}

// the real envs of the entries with their observation and action widths
inline bool tp_cont_env_ok(int env_id, int S, int A)
{
    return (env_id == LENV_ENV_CHEETAH_STANDIN && S == 17 && A == 6) || (env_id == LENV_ENV_PENDULUM && S == 3 && A == 1) ||
           (env_id == LENV_ENV_CMC && S == 2 && A == 1);
}
inline bool tp_discrete_env_ok(int env_id, int S, int A)
{
    return (env_id == LENV_ENV_CARTPOLE && S == 4 && A == 2) || (env_id == LENV_ENV_ACROBOT && S == 6 && A == 3) ||
           (env_id == LENV_ENV_MOUNTAINCAR && S == 2 && A == 3);
}

// The launch of the three MLP kernels: the dynamic LDS of tp_lds_layout, with the `params_to_stage` floats behind it where all of it stays
// within `limit` bytes (the kernel's ST instantiation then), on the grid (agent, block of TP_TB episodes).
struct TpPlan { size_t lds_bytes; bool staged; dim3 grid; };
inline TpPlan tp_launch_plan(int64_t agents, int T, int W, bool ln, int H, int params_to_stage, size_t limit)
{
    TpPlan p;
    const lenv::TpLds lay = lenv::tp_lds_layout(T < lenv::TP_TB ? T : lenv::TP_TB, W, ln, H);
    p.lds_bytes = (2 * (size_t)lay.act + lay.ln) * sizeof(float);
    p.staged = p.lds_bytes + (size_t)params_to_stage * sizeof(float) <= limit;
    if (p.staged) p.lds_bytes += (size_t)params_to_stage * sizeof(float);
    p.grid = dim3((unsigned)agents, (unsigned)((T + lenv::TP_TB - 1) / lenv::TP_TB));
    return p;
}

// Wave-chain kernels, a chain on a team of G workgroups.  Workgroups per chain: the first G of `candidates` (largest first) that cfg->team_size
// allows (0 = automatic, 1 = the plain launch, G = at most G), that divides `divides` (0 = no such rule) and for which all
// 8 * ceil(chains / 8) * G workgroups are resident at once (occupancy API: the members of a team wait for each other); else 1.
inline int pick_team(std::initializer_list<int> candidates, int team_size, int divides, int64_t chains, const void *kern, int threads, size_t lds_bytes)
{
    if (team_size == 1 || chains < 1) return 1;
    const int64_t padded = 8 * ((chains + 7) / 8);
    for (int G : candidates)
        if ((divides == 0 || divides % G == 0) && (team_size <= 0 || G <= team_size) && lenv_team_grid_resident(kern, threads, lds_bytes, padded * G)) return G;
    return 1;
}

// zeroes the team barrier counter and the give-up word of every chain (a_bar: their offset in the chain's arena) in front of a team launch
void team_reset(float *arena, int64_t arena_stride, int64_t a_bar, int64_t chains, hipStream_t stream);

// a.G workgroups per chain: blocks are dealt to the 8 XCDs round-robin, so a team launch pads the chains to a multiple of 8
template <class Args>
inline int launch_team(void (*kern)(const Args), unsigned threads, size_t lds_bytes, hipStream_t stream, const Args &a)
{
    unsigned grid = (unsigned)a.chains;
    if (a.G > 1) {
        grid = (unsigned)(8 * ((a.chains + 7) / 8) * a.G);
        team_reset(a.arena, a.arena_stride, a.a_bar, a.chains, stream);
    }
    return launch(kern, dim3(grid), dim3(threads), lds_bytes, stream, a);
}

}  // namespace lenv_host
