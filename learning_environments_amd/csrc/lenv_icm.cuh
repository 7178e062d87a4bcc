// lenv_icm.cuh -- the reference's Intrinsic Curiosity Module (models/icm_baseline.py:8-172) inside the GEMM-tiled inner loops:
// ICM.train on the gathered minibatch + compute_intrinsic_rewards with the updated model (agents/DDQN.py:74-76,
// agents/TD3.py:68-70); compute_intrinsic_rewards on all rows of a PPO.learn call and ICM.train after its epochs (agents/PPO.py:144-145,
// 183-184).  oracle/lenv_oracle_icm.inc is the canonical restatement; arithmetic and order are the same.
#pragma once

#include "lenv_gemm.cuh"

namespace lenv {

// ---- Intrinsic Curiosity Module (models/icm_baseline.py:8-172; oracle/lenv_oracle_icm.inc is the canonical restatement) ----
struct IcmLin { int in, out, oW, ob; };
struct IcmNet { int S, A, Ai, F, H, C, P; IcmLin feat[3], inv[3], pre[3], res[4][2], post[2]; };

__host__ __device__ inline void icm_lin_set(IcmLin &L, int in, int out, int &o) { L.in = in; L.out = out; L.oW = o; o += in * out; L.ob = o; o += out; }

// ICMModel.__init__ in state-dict order: features S-H-H-F, inverse 2F-H-H-Ai, forward_pre (F+Ai)-H-H-F, four residual blocks
// {fc1, fc2: (F+Ai)-F}, forward_post F-H-F; Ai = 1 for a two-action discrete env (icm_baseline.py:39-40)
__host__ __device__ inline void icm_build(IcmNet &n, int S, int A, int F, int H, bool discrete)
{
    int o = 0;
    n.S = S; n.A = A; n.Ai = (discrete && A == 2) ? 1 : A; n.F = F; n.H = H; n.C = F + n.Ai;
    icm_lin_set(n.feat[0], S, H, o); icm_lin_set(n.feat[1], H, H, o); icm_lin_set(n.feat[2], H, F, o);
    icm_lin_set(n.inv[0], 2 * F, H, o); icm_lin_set(n.inv[1], H, H, o); icm_lin_set(n.inv[2], H, n.Ai, o);
    icm_lin_set(n.pre[0], n.C, H, o); icm_lin_set(n.pre[1], H, H, o); icm_lin_set(n.pre[2], H, F, o);
    for (int k = 0; k < 4; ++k) { icm_lin_set(n.res[k][0], n.C, F, o); icm_lin_set(n.res[k][1], n.C, F, o); }
    icm_lin_set(n.post[0], F, H, o); icm_lin_set(n.post[1], H, F, o);
    n.P = o;
}

// per-chain ICM buffers in the arena
enum { IB_P, IB_M, IB_V, IB_G, IB_X2, IB_ACT, IB_FH0, IB_FH1, IB_FE, IB_IIN, IB_IH0, IB_IH1, IB_IZ, IB_PIN, IB_PH0, IB_PH1,
       IB_XC0, IB_XC1, IB_XC2, IB_XC3, IB_XC4, IB_HC0, IB_HC1, IB_HC2, IB_HC3, IB_QH, IB_PRED,
       IB_DPRED, IB_DZ, IB_DQH, IB_DX, IB_DH, IB_DPH1, IB_DPH0, IB_DFE, IB_DIH1, IB_DIH0, IB_DIIN, IB_DFH1, IB_DFH0, IB_COUNT };


// floats of every ICM buffer of one chain (minibatch B)
__host__ __device__ inline void icm_buffer_sizes(const IcmNet &n, int B, int64_t (&sz)[IB_COUNT])
{
    const int64_t b = B, b2 = 2 * (int64_t)B, H = n.H, F = n.F, C = n.C, Ai = n.Ai;
    const int64_t v[IB_COUNT] = { n.P, n.P, n.P, n.P, b2 * n.S, b * Ai, b2 * H, b2 * H, b2 * F, b * 2 * F, b * H, b * H, b * Ai, b * C, b * H, b * H,
                                  b * C, b * C, b * C, b * C, b * C, b * C, b * C, b * C, b * C, b * H, b * F,
                                  b * F, b * Ai, b * H, b * F, b * F, b * H, b * H, b2 * F, b * H, b * H, b * 2 * F, b2 * H, b2 * H };
    for (int i = 0; i < IB_COUNT; ++i) sz[i] = v[i];
}

// what one ICM step needs from the kernel around it
struct IcmStep {
    GemmQueue &gq; float *Ps, *Qs;            // the kernel's GEMM queue and its LDS staging buffers
    float *arena; const int64_t *a_icm;       // the chain's arena and the offsets of its ICM buffers (IB_*)
    volatile float *ctrl; int ci;             // LDS control words: ctrl[ci], ctrl[ci+1] carry the Adam bias corrections
    const IcmNet &icm; double *pows;          // layout; running beta1^t, beta2^t (thread 0's copy is the live one)
    double lr, beta, eta, adam_beta1, adam_beta2, adam_eps;
    int B;
    const float *s_rows; int lds;             // states [B][lds] and next states [B][ldn] of the minibatch
    const float *n_rows; int ldn;
    bool continuous;                          // TD3: the action vector is the input and the inverse loss is an MSE
};

// the chain's ICM buffers as pointers
struct IcmPtrs {
    float *ip, *ig, *X2, *actin, *fh0, *fh1, *fe, *iin, *ih0, *ih1, *iz, *pin, *ph0, *ph1, *qh, *pred, *xc[5], *hc[4];
};
__device__ __forceinline__ IcmPtrs icm_ptrs(const IcmStep &c)
{
    auto buf = [&](int i) { return c.arena + c.a_icm[i]; };
    IcmPtrs p;
    p.ip = buf(IB_P); p.ig = buf(IB_G); p.X2 = buf(IB_X2); p.actin = buf(IB_ACT);
    p.fh0 = buf(IB_FH0); p.fh1 = buf(IB_FH1); p.fe = buf(IB_FE); p.iin = buf(IB_IIN); p.ih0 = buf(IB_IH0); p.ih1 = buf(IB_IH1); p.iz = buf(IB_IZ);
    p.pin = buf(IB_PIN); p.ph0 = buf(IB_PH0); p.ph1 = buf(IB_PH1); p.qh = buf(IB_QH); p.pred = buf(IB_PRED);
    for (int k = 0; k < 5; ++k) p.xc[k] = buf(IB_XC0 + k);
    for (int k = 0; k < 4; ++k) p.hc[k] = buf(IB_HC0 + k);
    return p;
}

// The four pieces every use of the module is made of.  The three routines behind them: icm_rewards (stage, forward, rewards), icm_train
// (stage, forward, backward + Adam) and icm_train_and_reward (stage, forward, backward + Adam, forward, rewards): a train followed by a
// reward pass on the same rows stages the same values twice and so equals icm_train_and_reward bit for bit.

// stacked states, action inputs (one logit target for two actions, else one-hot: icm_baseline.py:39-40,134-136) and the action columns of
// every concatenated buffer.  action_of(b, i): action input i of sample b
template <class ActFn>
__device__ __forceinline__ void icm_stage(const IcmStep &c, const IcmPtrs &p, ActFn action_of)
{
    const int tid = (int)threadIdx.x;
    const int B = c.B, S = c.icm.S, F = c.icm.F, Ai = c.icm.Ai, C = c.icm.C;
    for (int e = tid; e < B * S; e += DNT) { const int b = e / S, i = e - b * S; p.X2[e] = c.s_rows[b * c.lds + i]; p.X2[B * S + e] = c.n_rows[b * c.ldn + i]; }
    for (int e = tid; e < B * Ai; e += DNT) {
        const int b = e / Ai, i = e - b * Ai;
        const float av = action_of(b, i);
        p.actin[e] = av;
        p.pin[b * C + F + i] = av;
        for (int k = 0; k < 5; ++k) p.xc[k][b * C + F + i] = av;
        for (int k = 0; k < 4; ++k) p.hc[k][b * C + F + i] = av;
    }
    __syncthreads();
}

// ICMModel.forward (icm_baseline.py:80-102) on the staged rows: features_model once on the stacked [s; s'] rows
template <int MAXI>
__device__ __forceinline__ void icm_forward(const IcmStep &c, const IcmPtrs &p)
{
    const int tid = (int)threadIdx.x;
    GemmQueue &gq = c.gq;
    const IcmNet &icm = c.icm;
    const int B = c.B, S = icm.S, F = icm.F, Hi = icm.H, Ai = icm.Ai, C = icm.C;
    float *const ip = p.ip;
    constexpr int LK = LENV_ACT_LEAKYRELU, RL = LENV_ACT_RELU;
    auto lin = [&](const IcmLin &L, const float *X, int ldx, int rows, float *Y, int ldy, int act) {
        if (act >= 0) gq.gemm(X, ldx, 1, ip + L.oW, L.in, 1, rows, L.out, L.in, epi_bias_act(Y, ldy, ip + L.ob, act, 0.25f));
        else gq.gemm(X, ldx, 1, ip + L.oW, L.in, 1, rows, L.out, L.in, epi_bias(Y, ldy, 0, ip + L.ob));
    };
    lin(icm.feat[0], p.X2, S, 2 * B, p.fh0, Hi, LK); lin(icm.feat[1], p.fh0, Hi, 2 * B, p.fh1, Hi, LK); lin(icm.feat[2], p.fh1, Hi, 2 * B, p.fe, F, -1);
    gq.run<MAXI>(c.Ps, c.Qs);
    for (int e = tid; e < B * F; e += DNT) {
        const int b = e / F, f = e - b * F;
        const float vs = p.fe[e], vn = p.fe[B * F + e];
        p.iin[b * 2 * F + f] = vs; p.iin[b * 2 * F + F + f] = vn; p.pin[b * C + f] = vs;
    }
    __syncthreads();
    lin(icm.inv[0], p.iin, 2 * F, B, p.ih0, Hi, RL); lin(icm.inv[1], p.ih0, Hi, B, p.ih1, Hi, RL); lin(icm.inv[2], p.ih1, Hi, B, p.iz, Ai, -1);
    lin(icm.pre[0], p.pin, C, B, p.ph0, Hi, LK); lin(icm.pre[1], p.ph0, Hi, B, p.ph1, Hi, LK); lin(icm.pre[2], p.ph1, Hi, B, p.xc[0], C, -1);
    for (int k = 0; k < 4; ++k) {
        lin(icm.res[k][0], p.xc[k], C, B, p.hc[k], C, LK);
        const IcmLin &L2 = icm.res[k][1];                   // x_{k+1} = x_k + fc2([fc1([x_k | a]) | a])
        gq.gemm(p.hc[k], C, 1, ip + L2.oW, L2.in, 1, B, L2.out, L2.in, epi_bias_add(p.xc[k + 1], C, ip + L2.ob, p.xc[k], C));
    }
    lin(icm.post[0], p.xc[4], C, B, p.qh, Hi, LK); lin(icm.post[1], p.qh, Hi, B, p.pred, F, -1);
    gq.run<MAXI>(c.Ps, c.Qs);
}

// the loss gradients of the forward pass just run, the backward pass and one step of torch.optim.Adam over all ICM parameters (lr = icm.lr)
template <int MAXI>
__device__ __forceinline__ void icm_backward_adam(const IcmStep &c, const IcmPtrs &p)
{
    const int tid = (int)threadIdx.x;
    GemmQueue &gq = c.gq;
    float *const Ps = c.Ps, *const Qs = c.Qs;
    const IcmNet &icm = c.icm;
    volatile float *ctrl = c.ctrl;
    const int B = c.B, S = icm.S, A = icm.A;
    const int F = icm.F, Hi = icm.H, Ai = icm.Ai, C = icm.C;
    auto buf = [&](int i) { return c.arena + c.a_icm[i]; };
    float *const ip = p.ip, *const ig = p.ig, *const X2 = p.X2, *const actin = p.actin;
    float *const fh0 = p.fh0, *const fh1 = p.fh1, *const fe = p.fe, *const iin = p.iin, *const ih0 = p.ih0, *const ih1 = p.ih1, *const iz = p.iz;
    float *const pin = p.pin, *const ph0 = p.ph0, *const ph1 = p.ph1, *const qh = p.qh, *const pred = p.pred;
    float *const *xc = p.xc, *const *hc = p.hc;
    constexpr int LK = LENV_ACT_LEAKYRELU, RL = LENV_ACT_RELU;
    // ---- loss gradients: beta * mse(forward, features(s')) and (1 - beta) * BCEWithLogits | CrossEntropy(inverse, action) ----
    float *dpred = buf(IB_DPRED), *dz = buf(IB_DZ), *dqh = buf(IB_DQH), *dx = buf(IB_DX), *dh = buf(IB_DH), *dph1 = buf(IB_DPH1);
    float *dph0 = buf(IB_DPH0), *dfe = buf(IB_DFE), *dih1 = buf(IB_DIH1), *dih0 = buf(IB_DIH0), *diin = buf(IB_DIIN), *dfh1 = buf(IB_DFH1), *dfh0 = buf(IB_DFH0);
    const float c_mse = (float)(c.beta * 2.0 / ((double)B * F)), c_act = (float)((1.0 - c.beta) / (double)B);
    const float c_amse = (float)((1.0 - c.beta) * 2.0 / ((double)B * A));     // continuous actions: MSELoss on [B, A]
    for (int e = tid; e < B * F; e += DNT) dpred[e] = c_mse * (pred[e] - fe[B * F + e]);
    for (int b = tid; b < B; b += DNT) {
        if (c.continuous) {
            for (int i = 0; i < A; ++i) dz[b * A + i] = c_amse * (iz[b * A + i] - actin[b * A + i]);
        } else if (Ai == 1) {
            const float sg = fma32(0.5f, det_tanhf(lenv_tanh_table, 0.5f * iz[b]), 0.5f);
            dz[b] = c_act * (sg - actin[b]);
        } else {
            float mx = iz[b * A];
            for (int i = 1; i < A; ++i) if (iz[b * A + i] > mx) mx = iz[b * A + i];
            float ex[4], sm = 0.0f;                           // A <= 3 for the supported envs
            for (int i = 0; i < A; ++i) { ex[i] = det_expf(iz[b * A + i] - mx); sm = sm + ex[i]; }
            for (int i = 0; i < A; ++i) dz[b * A + i] = c_act * (ex[i] / sm - actin[b * A + i]);
        }
    }
    __syncthreads();
    // ---- backward: per Linear dW = dY^T X (reduction over the rows), db = column sums, dX = dY W ----
    auto bw_w = [&](const IcmLin &L, const float *dY, int ldd, const float *X, int ldx, int rows) {
        gq.gemm(dY, 1, ldd, X, 1, ldx, L.out, L.in, rows, epi_store(ig + L.oW, L.in));
        gq.colsum(dY, rows, ldd, L.out, ig + L.ob);
    };
    auto bw_x = [&](const IcmLin &L, const float *dY, int ldd, int rows, int ncols, const GemmEpi &ep) {
        gq.gemm(dY, ldd, 1, ip + L.oW, 1, L.in, rows, ncols, L.out, ep);
    };
    bw_w(icm.post[1], dpred, F, qh, Hi, B); bw_x(icm.post[1], dpred, F, B, Hi, epi_act_bwd(dqh, Hi, qh, Hi, LK, 0.25f));
    bw_w(icm.post[0], dqh, Hi, xc[4], C, B); bw_x(icm.post[0], dqh, Hi, B, F, epi_store(dx, F));
    for (int k = 3; k >= 0; --k) {
        bw_w(icm.res[k][1], dx, F, hc[k], C, B); bw_x(icm.res[k][1], dx, F, B, F, epi_act_bwd(dh, F, hc[k], C, LK, 0.25f));
        bw_w(icm.res[k][0], dh, F, xc[k], C, B); bw_x(icm.res[k][0], dh, F, B, F, epi_accum(dx, F));
    }
    gq.run<MAXI>(Ps, Qs);
    bw_w(icm.pre[2], dx, F, ph1, Hi, B); bw_x(icm.pre[2], dx, F, B, Hi, epi_act_bwd(dph1, Hi, ph1, Hi, LK, 0.25f));
    bw_w(icm.pre[1], dph1, Hi, ph0, Hi, B); bw_x(icm.pre[1], dph1, Hi, B, Hi, epi_act_bwd(dph0, Hi, ph0, Hi, LK, 0.25f));
    bw_w(icm.pre[0], dph0, Hi, pin, C, B); bw_x(icm.pre[0], dph0, Hi, B, F, epi_store(dfe, F));
    bw_w(icm.inv[2], dz, Ai, ih1, Hi, B); bw_x(icm.inv[2], dz, Ai, B, Hi, epi_act_bwd(dih1, Hi, ih1, Hi, RL, 0.25f));
    bw_w(icm.inv[1], dih1, Hi, ih0, Hi, B); bw_x(icm.inv[1], dih1, Hi, B, Hi, epi_act_bwd(dih0, Hi, ih0, Hi, RL, 0.25f));
    bw_w(icm.inv[0], dih0, Hi, iin, 2 * F, B); bw_x(icm.inv[0], dih0, Hi, B, 2 * F, epi_store(diin, 2 * F));
    gq.run<MAXI>(Ps, Qs);
    for (int e = tid; e < B * F; e += DNT) {                    // gradient at features([s; s'])
        const int b = e / F, f = e - b * F;
        dfe[e] = dfe[e] + diin[b * 2 * F + f];                 // features(s): forward_pre + inverse
        dfe[B * F + e] = diin[b * 2 * F + F + f] - dpred[e];   // features(s'): inverse + mse target
    }
    __syncthreads();
    bw_w(icm.feat[2], dfe, F, fh1, Hi, 2 * B); bw_x(icm.feat[2], dfe, F, 2 * B, Hi, epi_act_bwd(dfh1, Hi, fh1, Hi, LK, 0.25f));
    bw_w(icm.feat[1], dfh1, Hi, fh0, Hi, 2 * B); bw_x(icm.feat[1], dfh1, Hi, 2 * B, Hi, epi_act_bwd(dfh0, Hi, fh0, Hi, LK, 0.25f));
    bw_w(icm.feat[0], dfh0, Hi, X2, S, 2 * B);
    gq.run<MAXI>(Ps, Qs);
    // ---- torch.optim.Adam over all ICM parameters (lr = icm.lr) ----
    if (tid == 0) {
        c.pows[0] *= c.adam_beta1; c.pows[1] *= c.adam_beta2;
        ctrl[c.ci] = (float)(-(c.lr / (1.0 - c.pows[0])));
        ctrl[c.ci + 1] = (float)__builtin_sqrt(1.0 - c.pows[1]);
    }
    __syncthreads();
    {
        const AdamConsts ac{ ctrl[c.ci], ctrl[c.ci + 1], (float)(1.0 - c.adam_beta1), (float)(1.0 - c.adam_beta2), (float)c.adam_beta2, (float)c.adam_eps };
        wg_adam(ip, buf(IB_M), buf(IB_V), ig, 0, icm.P, ac, nullptr, 0.0f, 0.0f);
    }
    __syncthreads();
}

// add_reward(b, eta * mean_f (features(s') - forward)^2) of the forward pass just run (called by one thread per sample)
template <class RewFn>
__device__ __forceinline__ void icm_reward_rows(const IcmStep &c, const IcmPtrs &p, RewFn add_reward)
{
    const int B = c.B, F = c.icm.F;
    const float eta = (float)c.eta;
    for (int b = (int)threadIdx.x; b < B; b += DNT) {
        float sm = 0.0f;
        for (int f = 0; f < F; ++f) { const float d = p.fe[(B + b) * F + f] - p.pred[b * F + f]; sm = fma32(d, d, sm); }
        add_reward(b, eta * (sm / (float)F));
    }
    __syncthreads();
}

// ICM.compute_intrinsic_rewards (icm_baseline.py:160-172) with the module as it is: one forward pass on the B rows, rewards[b] += r
template <int MAXI, class ActFn, class RewFn>
__device__ __forceinline__ void icm_rewards(const IcmStep &c, ActFn action_of, RewFn add_reward)
{
    const IcmPtrs p = icm_ptrs(c);
    icm_stage(c, p, action_of);
    icm_forward<MAXI>(c, p);
    icm_reward_rows(c, p, add_reward);
}

// ICM.train (icm_baseline.py:134-158): forward, loss gradients, backward, one Adam step
template <int MAXI, class ActFn>
__device__ __forceinline__ void icm_train(const IcmStep &c, ActFn action_of)
{
    const IcmPtrs p = icm_ptrs(c);
    icm_stage(c, p, action_of);
    icm_forward<MAXI>(c, p);
    icm_backward_adam<MAXI>(c, p);
}

// DDQN / TD3: ICM.train on the minibatch, then the intrinsic rewards of the UPDATED model
template <int MAXI, class ActFn, class RewFn>
__device__ __forceinline__ void icm_train_and_reward(const IcmStep &c, ActFn action_of, RewFn add_reward)
{
    const IcmPtrs p = icm_ptrs(c);
    icm_stage(c, p, action_of);
    icm_forward<MAXI>(c, p);
    icm_backward_adam<MAXI>(c, p);
    icm_forward<MAXI>(c, p);
    icm_reward_rows(c, p, add_reward);
}

}  // namespace lenv
