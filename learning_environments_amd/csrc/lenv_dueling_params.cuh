// lenv_dueling_params.cuh -- the flat parameter vector of the agents of the GEMM-queue kernel (dueling_se_inner_loop.hip): Critic_DuelingDQN
// (agent_kind 1) and the Critic_DQN that does not fit the register-resident kernel (agent_kind 0), and the widths that kernel admits.  Shared
// with agent_test_population.hip, which reads that kernel's final_online rows.
#pragma once

namespace lenv {

constexpr int D_MAXL = 3;         // feature-stream hidden layers supported (the *_vary agents draw hidden_layer + 1)
constexpr int D_MAXW = 128;       // max feature_dim (head width) and test episodes
constexpr int D_MAXH = 512;       // max hidden_size  (outputs wider than 128 run as several 128-column blocks)

// parameter offsets inside one parameter vector (state-dict order)
struct DuelOffsets {
    int oWf[D_MAXL + 1], obf[D_MAXL + 1];     // feature stream: hidden layers 0..L-1, then the output Linear (index L)
    int oWv1, obv1, oWv2, obv2, oWa1, oba1, oWa2, oba2;
    int oLN;                                  // q_layer_norm with L >= 2: weight [H] | bias [H] of the ONE shared nn.LayerNorm, behind the second Linear (Module.parameters() order)
    int P;
};

__host__ __device__ constexpr DuelOffsets duel_param_offsets(int S, int A, int H, int F, int L, bool plain, bool ln = false)
{
    DuelOffsets d{};
    int o = 0, n_in = S;
    for (int l = 0; l <= D_MAXL; ++l) d.oWf[l] = d.obf[l] = 0;
    for (int l = 0; l < L; ++l) {
        d.oWf[l] = o; o += H * n_in; d.obf[l] = o; o += H; n_in = H;
        if (ln && l == 1) { d.oLN = o; o += 2 * H; }
    }
    d.oWf[L] = o; o += F * H; d.obf[L] = o; o += F;
    if (plain) { d.oWv1 = d.obv1 = d.oWv2 = d.obv2 = d.oWa1 = d.oba1 = d.oWa2 = d.oba2 = o; }       // no heads
    else {
        d.oWv1 = o; o += F * F; d.obv1 = o; o += F; d.oWv2 = o; o += F; d.obv2 = o; o += 1;
        d.oWa1 = o; o += F * F; d.oba1 = o; o += F; d.oWa2 = o; o += A * F; d.oba2 = o; o += A;
    }
    d.P = o;
    return d;
}

}  // namespace lenv
