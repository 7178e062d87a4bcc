// lenv_actor_params.cuh -- the flat parameter layouts of the TD3 and PPO agent nets and the limits their fused entries admit: shared by
// td3_rn_inner_loop.hip / ppo_rn_inner_loop.hip (agent_init, final_params rows) and actor_test_population.hip, which reads the actor out of
// such rows.  One definition, so a row a fused launch wrote is read at the offsets it was written at.
#pragma once

namespace lenv {

constexpr int T3_MAXL = 3;     // hidden layers of actor / critic (TD3_vary draws hidden_layer + 1)
constexpr int T3_MAXW = 512;   // max hidden_size (outputs wider than 128 run as several 128-column blocks)

struct MlpOff { int in, H, L, out; int oW[T3_MAXL + 1], ob[T3_MAXL + 1]; int P; int ln, oLN; };      // ln: the net's shared LayerNorm (weight | bias at oLN, behind the second Linear)

__host__ __device__ inline void mlp_off(MlpOff &m, int in, int H, int L, int out, bool layer_norm = false)
{
    m.in = in; m.H = H; m.L = L; m.out = out;
    m.ln = layer_norm && L >= 2 ? 1 : 0; m.oLN = 0;        // use_layer_norm (model_utils.py:22-37): nothing to normalise with one hidden layer
    int o = 0, n_in = in;
    for (int l = 0; l <= T3_MAXL; ++l) m.oW[l] = m.ob[l] = 0;
    for (int l = 0; l < L; ++l) {
        m.oW[l] = o; o += H * n_in; m.ob[l] = o; o += H; n_in = H;
        if (m.ln && l == 1) { m.oLN = o; o += 2 * H; }
    }
    m.oW[L] = o; o += out * H; m.ob[L] = o; o += out;
    m.P = o;
}

constexpr int PP_MAXL = 2;       // hidden layers of actor.net / critic.net
constexpr int PP_MAXW = 128;     // hidden_size
constexpr int PP_MAXT = 64;      // test episodes

struct PpoMlp { int in, H, L, out; int oW[PP_MAXL + 1], ob[PP_MAXL + 1]; int P; };

__host__ __device__ inline void ppo_mlp(PpoMlp &m, int in, int H, int L, int out)
{
    m.in = in; m.H = H; m.L = L; m.out = out;
    int o = 0, n_in = in;
    for (int l = 0; l <= PP_MAXL; ++l) m.oW[l] = m.ob[l] = 0;
    for (int l = 0; l < L; ++l) { m.oW[l] = o; o += H * n_in; m.ob[l] = o; o += H; n_in = H; }
    m.oW[L] = o; o += out * H; m.ob[L] = o; o += out;
    m.P = o;
}

}  // namespace lenv
