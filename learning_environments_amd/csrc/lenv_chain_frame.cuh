// lenv_chain_frame.cuh -- how a fused inner-loop kernel ends a chain: the budget cut of the final test and the closing outputs.  Control code
// outside every hot loop, shared by the kernels the way lenv_host.h shares their host side: plain inlined functions over each family's own Out
// struct (lenv_inner_out, lenv_td3_out, lenv_ql_out).  The returns / lengths pointers are template parameters because the wave-chain kernels
// hold them as LDS-qualified pointers.  Used by the three wave-chain kernels and ql_se_inner_loop.hip; the GEMM-queue kernels, ql_rn and the
// headline kernel carry the same text written out (docs/notebook_chain_frame_refactor.md says why): a fix here is made there too.
#pragma once

#include <stdint.h>

namespace lenv {

// ---- the final test under the time-out ----
// BaseAgent.test (base_agent.py:177-184): test episode e starts only while the earlier episodes of THIS test used <= `remaining` env steps
// (remaining = step_budget - the steps taken when the test starts); the rest of the list is padded with the minimum return so far, -1e9 if
// that range is empty (time_is_up, base_agent.py:33-36).  Test episodes are independent, so the kernels roll out all T and cut the list
// afterwards: `stop` = the first episode that does not start, `used` = the env steps of the episodes that did.
struct BudgetCut { int stop; int64_t used; };

template <class LenP>
__device__ __forceinline__ BudgetCut chain_budget_cut(LenP tlen, int T, int64_t remaining)
{
    int64_t used = 0;
    int stop = T;
    for (int te = 0; te < T; ++te) {
        if (used > remaining) { stop = te; break; }
        used += tlen[te];
    }
    return { stop, used };
}

// one thread: ret[stop..T) = min(ret[0..stop)), or -1e9
template <class RetP>
__device__ __forceinline__ void chain_pad_returns(RetP ret, int stop, int T)
{
    double mn = -1e9;
    if (stop > 0) { mn = ret[0]; for (int i = 1; i < stop; ++i) if (ret[i] < mn) mn = ret[i]; }
    for (int te = stop; te < T; ++te) ret[te] = mn;
}

// ---- the closing outputs (one thread) ----
template <class Out>
__device__ __forceinline__ void chain_write_stats(const Out &out, int64_t chain, int64_t episodes_run, int64_t train_steps, int64_t learn_steps,
                                                  int64_t test_steps)
{
    if (out.stats) {
        out.stats[chain * 4 + 0] = episodes_run; out.stats[chain * 4 + 1] = train_steps;
        out.stats[chain * 4 + 2] = learn_steps; out.stats[chain * 4 + 3] = test_steps;
    }
}

// Episodes that never ran: NaN / 0, or -- after a time-out (timed_out_at >= 0) -- time_is_up's padding (base_agent.py:33-44): rewards with the
// minimum of the meter so far (-1e9 if none), lengths with the maximum so far (1e9 if none)
template <class Out>
__device__ __forceinline__ void chain_pad_episodes(const Out &out, int64_t chain, int train_episodes, int episodes_run, const double *meter,
                                                   int timed_out_at)
{
    double pad_r = __builtin_nan("");
    int pad_l = 0;
    if (timed_out_at >= 0) {
        pad_r = -1e9; pad_l = 1000000000;
        if (episodes_run > 0) { pad_r = meter[0]; for (int i = 1; i < episodes_run; ++i) if (meter[i] < pad_r) pad_r = meter[i]; }
        if (episodes_run > 0 && out.episode_len) {
            pad_l = out.episode_len[chain * train_episodes];
            for (int i = 1; i < episodes_run; ++i) { const int l = out.episode_len[chain * train_episodes + i]; if (l > pad_l) pad_l = l; }
        }
    }
    for (int e = episodes_run; e < train_episodes; ++e) {
        if (out.episode_test_mean) out.episode_test_mean[chain * train_episodes + e] = pad_r;
        if (out.episode_len) out.episode_len[chain * train_episodes + e] = pad_l;
    }
}

// score = statistics.mean(reward_list_test) (GTN_worker.py:199,209; summed in fp64 in list order), the final returns, the counters and the
// padding of the per-episode lists
template <class Out, class RetP>
__device__ __forceinline__ void chain_close(const Out &out, int64_t chain, int T, RetP ret, const double *meter, int train_episodes,
                                            int episodes_run, int64_t train_steps, int64_t learn_steps, int64_t test_steps, int timed_out_at)
{
    double sm = 0.0;
    for (int i = 0; i < T; ++i) sm += ret[i];
    out.score[chain] = sm / (double)T;
    if (out.final_returns) for (int i = 0; i < T; ++i) out.final_returns[chain * T + i] = ret[i];
    chain_write_stats(out, chain, episodes_run, train_steps, learn_steps, test_steps);
    chain_pad_episodes(out, chain, train_episodes, episodes_run, meter, timed_out_at);
}

}  // namespace lenv
