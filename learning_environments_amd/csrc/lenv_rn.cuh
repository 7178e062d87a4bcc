// lenv_rn.cuh -- RewardEnv on a vector-state real env inside the one-workgroup-per-chain kernels (td3_rn_inner_loop.hip, ppo_rn_inner_loop.hip):
// the perturbed reward net evaluated on one row by the whole workgroup, the stand-in's info vector and RewardEnv._calc_reward
// (envs/reward_env.py:81-131).  Oracle: rn_shape_one (lenv_oracle_td3.inc).  rn_step_population.hip runs the same row evaluation one step at a
// time on a smaller group.
#pragma once

#include "lenv_gemm.cuh"

namespace lenv {

// types 3, 4, 7, 8 append the real env's info vector to the net's input (reward_env.py:98-101)
__host__ __device__ inline bool rn_type_info_in(int rtype) { return rtype == 3 || rtype == 4 || rtype == 7 || rtype == 8; }
// Where a chain keeps its perturbed theta: a reward net with one hidden layer and the Linear(info_dim, 1, bias=False) of types 101 / 102 (which
// has no hidden layers whatever the ENV section's hidden_layer says) fit LDS; deeper nets live in the chain's arena.  One definition for the
// layouts (LDS floats), the staging loops and the row evaluation.
__host__ __device__ inline bool rn_theta_in_lds(int rtype, int rn_layers) { return rn_layers <= 1 || rtype > 100; }

struct RnRow {
    int rtype, S, info_dim, Hrn, layers, act;
    float prelu;
    bool ln;                      // the ENV section's LayerNorm behind hidden Linear 2..L (weight 1 / bias 0: NES never touches the module)
    const float *par;             // the chain's perturbed theta, wherever rn_theta_in_lds put it
    float *h, *h2;                // [Hrn] hidden rows (LDS)
    volatile float *ctrl;         // LDS words: the result goes to ctrl[slot]; ctrl[14], ctrl[15] carry a LayerNorm row's statistics
};

// phi = reward_net(obs [| info]) for the observation in `obs` (LDS, S floats) -> ctrl[slot]; types 101 / 102: w . info; type 0: 0.
// Called by every thread of a group of NT threads; ends with a barrier.  `par` is the chain's theta: a `const float *` (staged by the caller), or any
// type with `par + offset` and `par[i]` that forms element i on the way in (rn_step_population.hip perturbs deep nets like that).  LNP: the
// LayerNorm's weight | bias are part of theta, behind the second Linear (the lenv_mlp_desc layout of the one-step entries); otherwise they are the
// untouched 1 | 0 of the fused loops and theta holds the Linears only.
template <int NT, bool LNP, class Par>
__device__ __forceinline__ void rn_eval_row(const RnRow &n, const Par par, const float *obs, const float *info, int slot)
{
    const int tid = threadIdx.x, Hrn = n.Hrn, S = n.S, info_dim = n.info_dim;
    if (n.rtype == 0) { if (tid == 0) n.ctrl[slot] = 0.0f; __syncthreads(); return; }
    if (n.rtype > 100) {
        if (tid == 0) {
            float acc = 0.0f;
            for (int k = 0; k < info_dim; ++k) acc = fma32(info[k], par[k], acc);
            n.ctrl[slot] = acc;
        }
        __syncthreads();
        return;
    }
    // build_nn_from_config (model_utils.py:16-29): Linear(D, H) | [Linear(H, H)] x (layers - 1) | Linear(H, 1), flat in Module.parameters() order
    const bool info_in = rn_type_info_in(n.rtype);
    const int Drn = info_in ? S + info_dim : S;
    const Par W0 = par, b0 = par + Hrn * Drn;
    const Par lnw = b0 + (Hrn + Hrn * Hrn + Hrn), lnb = lnw + Hrn;       // (LNP only)
    for (int j = tid; j < Hrn; j += NT) {
        float z = 0.0f;
        for (int k = 0; k < S; ++k) z = fma32(obs[k], W0[j * Drn + k], z);
        if (info_in) for (int k = 0; k < info_dim; ++k) z = fma32(info[k], W0[j * Drn + S + k], z);
        n.h[j] = act_fwd(n.act, n.prelu, z + b0[j]);
    }
    __syncthreads();
    const float *hp = n.h;
    Par Wl = b0 + Hrn;
    float *hn = n.h2;
    for (int l = 1; l < n.layers; ++l) {
        const Par bl = Wl + Hrn * Hrn;
        for (int j = tid; j < Hrn; j += NT) {
            float z = 0.0f;
            for (int k = 0; k < Hrn; ++k) z = fma32(hp[k], Wl[j * Hrn + k], z);
            z = z + bl[j];
            hn[j] = n.ln ? z : act_fwd(n.act, n.prelu, z);
        }
        __syncthreads();
        if (n.ln) {                                    // the LayerNorm row, reduced by thread 0
            if (tid == 0) {
                float sm = 0.0f, sv = 0.0f;
                for (int j = 0; j < Hrn; ++j) sm = sm + hn[j];
                const float mean = sm / (float)Hrn;
                for (int j = 0; j < Hrn; ++j) { const float dj = hn[j] - mean; sv = fma32(dj, dj, sv); }
                n.ctrl[14] = mean; n.ctrl[15] = 1.0f / __builtin_sqrtf(sv / (float)Hrn + 1e-5f);
            }
            __syncthreads();
            const float mean = n.ctrl[14], r = n.ctrl[15];
            if constexpr (LNP) { for (int j = tid; j < Hrn; j += NT) hn[j] = act_fwd(n.act, n.prelu, fma32((hn[j] - mean) * r, lnw[j], lnb[j])); }
            else for (int j = tid; j < Hrn; j += NT) hn[j] = act_fwd(n.act, n.prelu, fma32((hn[j] - mean) * r, 1.0f, 0.0f));
            __syncthreads();
        }
        const float *t2 = hp; hp = hn; hn = const_cast<float *>(t2);
        Wl = bl + Hrn;
        if constexpr (LNP) if (n.ln && l == 1) Wl = Wl + 2 * Hrn;
    }
    const Par Wo = Wl, bo = Wo + Hrn;
    if (tid == 0) {
        float acc = 0.0f;
        for (int j = 0; j < Hrn; ++j) acc = fma32(hp[j], Wo[j], acc);
        n.ctrl[slot] = acc + bo[0];
    }
    __syncthreads();
}

// the fused loops' form: the whole workgroup of DNT threads on the theta RnRow points at
__device__ __forceinline__ void wg_rn_eval(const RnRow &n, const float *obs, const float *info, int slot)
{
    rn_eval_row<DNT, false>(n, n.par, obs, info, slot);
}

// the HalfCheetah stand-in's info vector of a step (fp32, as torch.tensor(list(info.values()))): x_new = the state after the step, ctrl_cost =
// sum a^2 (ContEnv::reward_pre)
__device__ __forceinline__ void cheetah_info_row(float *info, const double *x_new, double ctrl_cost)
{
    info[0] = (float)x_new[0]; info[1] = (float)x_new[8]; info[2] = (float)x_new[8]; info[3] = (float)(-0.1 * ctrl_cost);
}

// RewardEnv._calc_reward (reward_env.py:81-131), fp32 left to right
__device__ __forceinline__ float rn_shaped_reward(int rtype, float r32, float g32, float phi_s, float phi_s2)
{
    switch (rtype) {
    case 0: return r32;
    case 1: case 3: return g32 * phi_s2 - phi_s;
    case 2: case 4: return (r32 + g32 * phi_s2) - phi_s;
    case 5: case 7: case 101: return phi_s2;
    default: return r32 + phi_s2;     // 6, 8, 102
    }
}

}  // namespace lenv
