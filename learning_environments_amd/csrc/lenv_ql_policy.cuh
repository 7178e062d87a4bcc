// lenv_ql_policy.cuh -- the greedy action of the tabular agents (ql_rn_inner_loop.hip, ql_test_population.hip).
#pragma once

namespace lenv {

// QL / SARSA.select_test_action: torch.argmax of the fp32 cast of the python-float64 Q row, first maximum
__device__ __forceinline__ int ql_argmax_f32(const double *row, int n)
{
    int best = 0;
    float bv = (float)row[0];
    for (int i = 1; i < n; ++i) { const float v = (float)row[i]; if (v > bv) { bv = v; best = i; } }
    return best;
}

}  // namespace lenv
