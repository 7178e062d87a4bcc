/* se_fit_ref.c -- CPU restatement of the supervised VirtualEnv fit that csrc/se_fit.hip runs (lenv_se_fit_population, include/lenv_hip.h).
 * TEST INFRASTRUCTURE: compiled by tests/se_fit_ref.py with the oracle Makefile's flags and linked against the oracle library; every forward
 * goes through the oracle's exported orc_mlp_forward (k-ascending fmaf chain from 0.0f, bias added last), every counter draw through
 * orc_rng_u64.  tests/test_se_fit_reference.py holds it to torch autograd and torch.optim.Adam; tests/test_se_fit_gpu.py holds the kernel to it.
 *
 * What is restated:
 *   loss_k = F.mse_loss(net_k(x_b), y_k_b)     fmaf chain of the squared errors, rows ascending, outputs ascending inside a row,
 *                                              / (float)(B * out_dim); dL/dy = (float)(2.0 / (double)(B * out_dim)) * e
 *   backward                                   oracle/lenv_oracle.c mlp_backward_one_ex, row after row in ascending order into one gradient
 *   torch.optim.Adam single-tensor step        oracle/lenv_oracle_td3.inc td3_adam; beta^t by repeated multiplication in double from step 0 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../oracle/lenv_oracle.h"

enum { STREAM_SE_FIT_BATCH = 15 };

static int64_t head_params(const orc_mlp_desc *d) { return (int64_t)d->in_dim * d->hidden + d->hidden; }

static float act_bwd(int act, float a, float g)
{
    switch (act) {
    case ORC_ACT_RELU: return a > 0.0f ? g : 0.0f;
    case ORC_ACT_LEAKYRELU: return a > 0.0f ? g : g * 0.01f;      /* a > 0 exactly where z > 0 */
    case ORC_ACT_TANH: return g * fmaf(-a, a, 1.0f);
    default: return g;
    }
}

/* One gradient evaluation of one net on the minibatch xb [B, in], yb [B, out]: g [P] (overwritten) and the mean loss. */
int se_fit_ref_grad(const orc_mlp_desc *d, const float *p, const float *xb, const float *yb, int32_t B, float *g, float *loss_out)
{
    const int in = d->in_dim, H = d->hidden, L = d->layers, O = d->out_dim;
    if (L < 1 || L > 2 || d->use_layer_norm || d->act == ORC_ACT_PRELU || B < 1) return -1;
    const int64_t P = orc_mlp_num_params(d), oW1 = head_params(d), oWo = oW1 + (L - 1) * ((int64_t)H * H + H), obo = oWo + (int64_t)O * H;
    float *y = malloc(sizeof(float) * (size_t)B * O), *a0 = malloc(sizeof(float) * (size_t)B * H), *a1 = malloc(sizeof(float) * (size_t)B * H);
    float *da = malloc(sizeof(float) * (size_t)H), *dz = malloc(sizeof(float) * (size_t)H), *dout = malloc(sizeof(float) * (size_t)O);
    int rc = 0;
    if (L == 1) rc |= orc_mlp_forward(d, p, xb, B, y, a0);
    else {
        /* the first hidden layer's activations: the same net cut behind its second Linear (whose outputs go unused) */
        orc_mlp_desc d1 = *d;
        float *z1 = malloc(sizeof(float) * (size_t)B * H);
        d1.layers = 1; d1.out_dim = H;
        rc |= orc_mlp_forward(&d1, p, xb, B, z1, a0);
        rc |= orc_mlp_forward(d, p, xb, B, y, a1);
        free(z1);
    }
    const float scale = (float)(2.0 / (double)(B * O));
    float lsum = 0.0f;
    memset(g, 0, sizeof(float) * (size_t)P);
    for (int b = 0; b < B; ++b) {
        const float *x = xb + (size_t)b * in, *al = (L == 2 ? a1 : a0) + (size_t)b * H;
        for (int o = 0; o < O; ++o) {
            const float e = y[(size_t)b * O + o] - yb[(size_t)b * O + o];
            lsum = fmaf(e, e, lsum);
            dout[o] = scale * e;
        }
        for (int o = 0; o < O; ++o) {
            float *gW = g + oWo + (int64_t)o * H;
            for (int j = 0; j < H; ++j) gW[j] = fmaf(dout[o], al[j], gW[j]);
            g[obo + o] = g[obo + o] + dout[o];
        }
        for (int j = 0; j < H; ++j) {
            float acc = 0.0f;
            for (int o = 0; o < O; ++o) acc = fmaf(dout[o], p[oWo + (int64_t)o * H + j], acc);
            da[j] = acc;
        }
        for (int l = L - 1; l >= 0; --l) {
            const int n_in = l == 0 ? in : H;
            const float *inp = l == 0 ? x : a0 + (size_t)b * H, *a = (l == 1 ? a1 : a0) + (size_t)b * H;
            const int64_t oW = l == 0 ? 0 : oW1, ob = oW + (int64_t)H * n_in;
            for (int j = 0; j < H; ++j) dz[j] = act_bwd(d->act, a[j], da[j]);
            for (int j = 0; j < H; ++j) {
                for (int i = 0; i < n_in; ++i) g[oW + (int64_t)j * n_in + i] = fmaf(dz[j], inp[i], g[oW + (int64_t)j * n_in + i]);
                g[ob + j] = g[ob + j] + dz[j];
            }
            if (l > 0)
                for (int i = 0; i < n_in; ++i) {
                    float acc = 0.0f;
                    for (int j = 0; j < H; ++j) acc = fmaf(dz[j], p[oW + (int64_t)j * n_in + i], acc);
                    da[i] = acc;
                }
        }
    }
    *loss_out = lsum / (float)(B * O);
    free(y); free(a0); free(a1); free(da); free(dz); free(dout);
    return rc;
}

/* torch.optim.Adam single-tensor step number `step` (0-based) on n elements with the gradient g */
void se_fit_ref_adam(float *p, float *m, float *v, const float *g, int64_t n, int64_t step, double lr, double beta1, double beta2, double adam_eps)
{
    double b1pow = 1.0, b2pow = 1.0;
    for (int64_t i = 0; i <= step; ++i) { b1pow *= beta1; b2pow *= beta2; }
    const float neg_step = (float)(-(lr / (1.0 - b1pow))), bc2_sqrt = (float)sqrt(1.0 - b2pow);
    const float w1 = (float)(1.0 - beta1), w2 = (float)(1.0 - beta2), fb2 = (float)beta2, eps = (float)adam_eps;
    for (int64_t i = 0; i < n; ++i) {
        const float mm = fmaf(w1, g[i] - m[i], m[i]);
        float vv = v[i] * fb2;
        vv = fmaf(w2 * g[i], g[i], vv);
        const float denom = sqrtf(vv) / bc2_sqrt + eps;
        p[i] = p[i] + (neg_step * mm) / denom;
        m[i] = mm; v[i] = vv;
    }
}

/* the whole fit, with lenv_se_fit_population's arguments (host arrays; no workspace) */
int se_fit_ref_run(const orc_mlp_desc *sn, const orc_mlp_desc *rn, const orc_mlp_desc *dn, const float *x, const float *y_state,
                   const float *y_reward, const float *y_done, int64_t N, int32_t batch, int64_t step_begin, int64_t step_end, double lr,
                   double beta1, double beta2, double adam_eps, const uint64_t *rng_keys, const int32_t *batch_idx, int64_t models, float *theta,
                   float *adam_m, float *adam_v, float *loss)
{
    const orc_mlp_desc *nets[3] = {sn, rn, dn};
    const float *ys[3] = {y_state, y_reward, y_done};
    const int in = sn->in_dim;
    const int64_t Pn[3] = {orc_mlp_num_params(sn), orc_mlp_num_params(rn), orc_mlp_num_params(dn)}, P = Pn[0] + Pn[1] + Pn[2];
    const int64_t nsteps = step_end - step_begin;
    if ((rng_keys != NULL) == (batch_idx != NULL) || N < 1 || batch < 1) return -1;
    float *xb = malloc(sizeof(float) * (size_t)batch * in), *yb = malloc(sizeof(float) * (size_t)batch * sn->out_dim), *g = malloc(sizeof(float) * (size_t)Pn[0]);
    int64_t *rows = malloc(sizeof(int64_t) * (size_t)batch);
    int rc = 0;
    for (int64_t m = 0; m < models; ++m)
        for (int64_t it = 0; it < nsteps; ++it) {
            const int64_t t = step_begin + it;
            for (int j = 0; j < batch; ++j) {
                int64_t r;
                if (batch_idx) r = batch_idx[(m * nsteps + it) * batch + j];
                else r = (int64_t)(((orc_rng_u64(rng_keys[m], STREAM_SE_FIT_BATCH, (uint64_t)(t * batch + j)) >> 32) * (uint64_t)(uint32_t)N) >> 32);
                rows[j] = r < 0 ? 0 : r >= N ? N - 1 : r;
                memcpy(xb + (size_t)j * in, x + rows[j] * in, sizeof(float) * (size_t)in);
            }
            int64_t off = m * P;
            for (int k = 0; k < 3; ++k) {
                const int O = nets[k]->out_dim;
                float l;
                for (int j = 0; j < batch; ++j) memcpy(yb + (size_t)j * O, ys[k] + rows[j] * O, sizeof(float) * (size_t)O);
                rc |= se_fit_ref_grad(nets[k], theta + off, xb, yb, batch, g, &l);
                if (loss) loss[(m * nsteps + it) * 3 + k] = l;
                se_fit_ref_adam(theta + off, adam_m + off, adam_v + off, g, Pn[k], t, lr, beta1, beta2, adam_eps);
                off += Pn[k];
            }
        }
    free(xb); free(yb); free(g); free(rows);
    return rc;
}
