// lenv_td3d_actor.cuh -- what the TD3_discrete_vary kernels share about the Gumbel-softmax actor (td3_discrete_inner_loop.hip,
// discrete_actor_test_population.hip): the flat parameter layout of one net, the counter streams of the Gumbel draws, the draw itself, the
// annealed temperature, the head, and the first-maximum argmax that hands the action vector to the env.
#pragma once

#include "lenv_gemm.cuh"

namespace lenv {

constexpr int TD_MAXL = 3;     // hidden layers of actor / critic (vary_hyperparameters draws hidden_layer + 1)
constexpr int TD_MAXW = 512;   // max hidden_size
constexpr int TD_MAXA = 8;     // max action_dim

enum { STREAM_TD3D_GUMBEL_ACT = 13, STREAM_TD3D_GUMBEL_TEST = 14, STREAM_TD3D_GUMBEL_TARGET = 15, STREAM_TD3D_GUMBEL_ACTOR = 16 };

// flat layout of one net in Module.parameters() order: W0 b0 [W1 b1 [LNw LNb] W2 b2 ...] Wout bout
struct DMlpOff { int in, H, L, out, ln; int oW[TD_MAXL + 1], ob[TD_MAXL + 1], oLN; int P; };

__host__ __device__ inline void dmlp_off(DMlpOff &m, int in, int H, int L, int out, int use_ln)
{
    m.in = in; m.H = H; m.L = L; m.out = out; m.ln = (use_ln && L >= 2) ? 1 : 0; m.oLN = 0;
    int o = 0, n_in = in;
    for (int l = 0; l <= TD_MAXL; ++l) m.oW[l] = m.ob[l] = 0;
    for (int l = 0; l < L; ++l) {
        m.oW[l] = o; o += H * n_in; m.ob[l] = o; o += H; n_in = H;
        if (m.ln && l == 1) { m.oLN = o; o += 2 * H; }
    }
    m.oW[L] = o; o += out * H; m.ob[L] = o; o += out;
    m.P = o;
}

// natural-log based Gumbel(0,1) draw from one counter value (oracle: orc_gumbel)
__device__ __forceinline__ float det_gumbel(uint64_t key, uint32_t stream, uint64_t n)
{
    const double u = ((double)(rng_u64(key, stream, n) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    return (float)(-det_log(-det_log(u)));
}

// np.linspace(temp, temp / 20, 2000)[min(n, 1999)] rounded to fp32 (oracle: orc_td3d_temperature)
__device__ __forceinline__ float td3d_temperature(double temp0, int64_t n)
{
    const double stop = temp0 / 20;
    const double step = (stop - temp0) / 1999.0;
    if (n >= 1999) return (float)stop;
    return (float)((double)n * step + temp0);
}

__device__ __forceinline__ int argmax_first(const float *v, int n)
{
    int best = 0;
    for (int k = 1; k < n; ++k) if (v[k] > v[best]) best = k;
    return best;
}

// gumbel_softmax(raw * max_action, tau, hard) for one row (oracle: td3d_actor_one): out = the returned action, ys = y_soft
__device__ __forceinline__ void gumbel_softmax_row(const float *raw, const float *gum, int A, float ma, float tau, bool hard, float *out, float *ys)
{
    float t[TD_MAXA], e[TD_MAXA], y[TD_MAXA];
    for (int k = 0; k < A; ++k) t[k] = (raw[k] * ma + gum[k]) / tau;
    float mx = t[0];
    for (int k = 1; k < A; ++k) if (t[k] > mx) mx = t[k];
    float sm = 0.0f;
    for (int k = 0; k < A; ++k) { e[k] = det_expf(t[k] - mx); sm = sm + e[k]; }
    for (int k = 0; k < A; ++k) y[k] = e[k] / sm;
    if (hard) {
        int idx = 0;
        for (int k = 1; k < A; ++k) if (y[k] > y[idx]) idx = k;
        for (int k = 0; k < A; ++k) out[k] = ((k == idx ? 1.0f : 0.0f) - y[k]) + y[k];
    } else for (int k = 0; k < A; ++k) out[k] = y[k];
    if (ys) for (int k = 0; k < A; ++k) ys[k] = y[k];
}

}  // namespace lenv
